"""GPU: corr_build_grad.hip (scf_corr_build_grad) through ``ops.corr_build_grad`` against the float64 restatement and the
derived bound of tests/test_corr_grad_host.py: `error <= bound` over ALL elements of both outputs (ratio <= 1), the
exact-integer and doubling cases by bit equality, run-to-run and batch independence by bit equality, the reach of a NaN,
canary bands around both destinations (the halves of one (2N, C, h, w) buffer included) and every refusal."""
import numpy as np
import pytest
import torch

from scflow_amd import ops
from scflow_amd._lib import ScflowHipError
import test_corr_grad_host as KH
from test_stream_ops_host import f64, measured, same_bits

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 1234.5
BAND = 256
cpu = lambda t: t.detach().cpu()                                    # noqa: E731


def D(t):
    return t.to(DEV).contiguous()


def run(case, guarded=False, halves=False):
    """ops.corr_build_grad on a host case -> (g_feat1, g_feat2) on the GPU.  ``guarded``: each destination sits between two
    bands of GUARD; ``halves``: the destinations are the halves of ONE (2N, C, h, w) buffer between two bands."""
    dev = {k: D(v) for k, v in case.items()}
    if not (guarded or halves):
        return ops.corr_build_grad(dev['g_vol'], dev['feat1'], dev['feat2'])
    shape = tuple(case['feat1'].shape)
    numel = case['feat1'].numel()
    if halves:
        bufs = [torch.full((2 * numel + 2 * BAND,), GUARD, device=DEV)]
        both = bufs[0][BAND:BAND + 2 * numel].view((2 * shape[0],) + shape[1:])
        out = (both[:shape[0]], both[shape[0]:])
    else:
        bufs = [torch.full((numel + 2 * BAND,), GUARD, device=DEV) for _ in range(2)]
        out = tuple(b[BAND:BAND + numel].view(shape) for b in bufs)
    got = ops.corr_build_grad(dev['g_vol'], dev['feat1'], dev['feat2'], out=out)
    assert got[0] is out[0] and got[1] is out[1]
    for b in bufs:
        assert bool((b[:BAND] == GUARD).all()) and bool((b[-BAND:] == GUARD).all()), 'a guard value was overwritten'
    return got


@pytest.mark.parametrize('shape', KH.SHAPES, ids=str)
def test_against_float64(shape):
    case = KH.grad_case(shape)
    got = run(case, guarded=True)
    v = KH.worst([cpu(g) for g in got], KH.corr_build_grad_ref(**case))
    measured(f'corr_build_grad {shape}: worst error / bound', v)
    assert v <= 1.0
    assert all(bool(torch.isfinite(g).all()) for g in got)
    halves = run(case, halves=True)                                 # the shared encoder's (2N, ...) buffer: the same bits
    assert all(same_bits(a, b) for a, b in zip(got, halves))
    for _ in range(2):                                              # three runs, equal bits
        assert all(same_bits(a, b) for a, b in zip(got, run(case))), 'two runs differ'
    twice = run(dict(case, g_vol=case['g_vol'] * 2))                # doubling the cotangent doubles both outputs
    assert all(same_bits(a * 2, b) for a, b in zip(got, twice))


@pytest.mark.parametrize('shape', KH.EXACT_SHAPES, ids=str)
def test_small_integers_are_exact(shape):
    case = KH.exact_case(shape)
    got = run(case, guarded=True)
    want = KH.corr_build_grad64(**case)
    assert all(np.array_equal(f64(g), w) for g, w in zip(got, want))


@pytest.mark.parametrize('shape', KH.SHAPES, ids=str)
def test_a_sample_alone_gives_the_bits_it_has_in_a_batch_of_three(shape):
    _, c, h, w = shape
    case = KH.grad_case((3, c, h, w), seed=3)
    all3 = run(case)
    for n in range(3):
        one = run(dict(g_vol=case['g_vol'][n * h * w:(n + 1) * h * w], feat1=case['feat1'][n:n + 1], feat2=case['feat2'][n:n + 1]))
        assert all(same_bits(a, b[n:n + 1]) for a, b in zip(one, all3)), n


@pytest.mark.parametrize('shape', KH.SHAPES, ids=str)
def test_a_nan_reaches_its_own_row_and_column_only(shape):
    """a NaN at G[n][i][j] reaches g_feat1[n][:, i] and g_feat2[n][:, j], every other element keeps its bits"""
    n_, c, h, w = shape
    hw = h * w
    case = KH.grad_case(shape, seed=4)
    clean = run(case)
    n, i, j = n_ - 1, (2 * hw) // 3, hw // 3
    bad = dict(case, g_vol=case['g_vol'].clone())
    bad['g_vol'].view(n_, hw, hw)[n, i, j] = float('nan')
    got = run(bad, guarded=True)
    for g, ref, at in ((got[0], clean[0], i), (got[1], clean[1], j)):
        g, ref = g.view(n_, c, hw), ref.view(n_, c, hw)
        assert bool(torch.isnan(g[n, :, at]).all())
        keep = torch.ones((n_, c, hw), dtype=torch.bool, device=DEV)
        keep[n, :, at] = False
        assert same_bits(g[keep], ref[keep])


@pytest.mark.parametrize('off', ['g_vol', 'feat1', 'feat2', 'out0', 'out1'])
def test_operands_one_float_off_16_byte_alignment(off):
    shape = (2, 64, 8, 16)
    case = KH.grad_case(shape, seed=5)
    base = run(case)

    def place(t, shift):
        buf = torch.full((t.numel() + 4 + BAND,), GUARD, device=DEV)
        v = buf[shift:shift + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4 * shift
        return buf, v
    dev = {k: place(v, 1 if k == off else 0)[1] for k, v in case.items()}
    outs = [place(torch.zeros(shape), 1 if off == f'out{k}' else 0) for k in range(2)]
    got = ops.corr_build_grad(dev['g_vol'], dev['feat1'], dev['feat2'], out=[v for _, v in outs])
    assert all(same_bits(a, b) for a, b in zip(got, base))
    for (buf, v), shift in zip(outs, (int(off == 'out0'), int(off == 'out1'))):
        assert bool((buf[:shift] == GUARD).all()) and bool((buf[shift + v.numel():] == GUARD).all())
    v = KH.worst([cpu(g) for g in got], KH.corr_build_grad_ref(**case))
    measured(f'corr_build_grad {shape}, {off} one float off alignment: worst error / bound', v)
    assert v <= 1.0


def test_ops_refusals():
    """every refusal raises before a launch: the destinations keep the bits they had"""
    shape = (2, 8, 4, 4)
    case = {k: D(v) for k, v in KH.grad_case(shape).items()}
    g, f1, f2 = case['g_vol'], case['feat1'], case['feat2']
    o1, o2 = torch.full(shape, GUARD, device=DEV), torch.full(shape, GUARD, device=DEV)
    assert tuple(ops.corr_build_grad(g.view(2, 16, 16), f1, f2)[0].shape) == shape          # (N, hw, hw) is the same volume
    for args, kw, match in (
            ((g, f1, f2[:1]), {}, 'feat2 must be'),
            ((g, f1[0], f2[0]), {}, 'feat1 must be'),
            ((g[:16], f1, f2), {}, 'g_vol must be'),
            ((g, f1, f2), dict(out=[o1]), 'pair'),
            ((g, f1, f2), dict(out=(o1, o2[:1])), r'out\[1\] must be'),
            ((g, f1, f2), dict(out=(o1, o1)), r'out\[0\] overlaps out\[1\]'),
            ((g, f1, f2), dict(out=(f1, o2)), r'out\[0\] overlaps feat1'),
            ((g, f1, f2), dict(out=(o1, f2)), r'out\[1\] overlaps feat2'),
            ((g, f1, f2), dict(out=(g.view(-1)[:f1.numel()].view(shape), o2)), r'out\[0\] overlaps g_vol'),
            ((g.cpu(), f1, f2), {}, 'g_vol'),
            ((g, f1.cpu(), f2), {}, 'feat1'),
            ((g, f1, f2), dict(out=(o1.cpu(), o2)), r'out\[0\]'),
            ((g.double(), f1, f2), {}, 'g_vol: expected float32'),
            ((g, f1, f2.half()), {}, 'feat2: expected float32'),
            ((g.transpose(1, 2), f1, f2), {}, 'g_vol: expected a contiguous'),
            ((g, f1.transpose(2, 3), f2), {}, 'feat1: expected a contiguous'),
            ((g, f1, f2), dict(out=(o1.transpose(2, 3), o2)), r'out\[0\]: expected a contiguous')):
        with pytest.raises(ScflowHipError, match=match):
            ops.corr_build_grad(*args, **kw)
    torch.cuda.synchronize()
    assert bool((o1 == GUARD).all()) and bool((o2 == GUARD).all())
