"""GPU: the first block of a down-sampling residual stage.  Below: its first convolution and shortcut as one launch
(conv_dma.hip, the shared-input form behind ops.conv2d_pair).  Here: its tail, ``ops.instance_norm(x, res=r, res_norm=True)``
(norm.hip, scf_instance_norm_res_norm): relu?(IN(x) + IN(r)) in one pass over both tensors.

What is asserted of the tail:
  * bit equality with the two-pass form it replaces, ``instance_norm(r, out=r)`` then ``instance_norm(x, res=r, relu)``,
    on each register route (VEC4 = 1, 4, 16) and on the two-launch fallback;
  * a float64 restatement under the bound tests/test_stream_ops_host.py derives for ``instance_norm`` (norm_core), with the
    normalised residual carrying its own bound into the addition.
"""
import numpy as np
import pytest
import torch

from scflow_amd import ops
from test_stream_ops_host import U, f64, in_depth, measured, norm_core, worst_ratio  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# (N, C, H, W): planes x HW = 6 x 1024 (VEC4 = 1), 6 x 4096 (VEC4 = 4), 4 x 16384 (VEC4 = 16, the largest fused plane) and
# 4 x 4100 (n4 = 1025 is a VEC4 = 16 plane too; 41 x 100 with a misaligned view below is the generic fallback)
RN_SHAPES = [(2, 3, 32, 32), (2, 3, 64, 64), (2, 2, 128, 128), (2, 2, 41, 100)]
RN_OPERANDS = ['nominal', 'dc50', 'constant_plane', 'nan_plane']


def rn_case(operand, shape, seed=0):
    g = torch.Generator().manual_seed(9100 + 10 * RN_OPERANDS.index(operand) + seed)
    x = 0.5 + 2.0 * torch.randn(shape, generator=g)
    r = -0.25 + 1.5 * torch.randn(shape, generator=g)
    if operand == 'dc50':
        x, r = x + 50.0, r + 50.0
    elif operand == 'constant_plane':
        x[0, -1] = 3.7
        r[-1, 0] = -1e3
    elif operand == 'nan_plane':
        x[0, -1, shape[2] // 2, shape[3] // 3] = float('nan')
        r[-1, -1, 0, 0] = float('nan')
    return x.contiguous(), r.contiguous()


def bits(t):
    return t.contiguous().view(torch.int32)


def two_pass(xd, rd, relu):
    rn = ops.instance_norm(rd)
    return ops.instance_norm(xd, res=rn, relu=relu)


def res_norm_ref(x, r, relu, aligned=True):
    """(float64 reference, per-element bound) of relu?(IN(x) + IN(r))."""
    n, c, h, w = x.shape
    d = in_depth(h * w, aligned)
    yx, bx = norm_core(f64(x).reshape(n, c, h * w), d)
    yr, br = norm_core(f64(r).reshape(n, c, h * w), d)
    b = bx + br + U * (np.abs(yx) + np.abs(yr) + bx + br)           # one addition of two values that carry their bounds
    y = yx + yr
    if relu:
        y = np.maximum(y, 0.0)
    return y.reshape(x.shape), b.reshape(x.shape)


def poisoned(x, r):
    """(N, C) mask of the planes that hold a non-finite value in x or r."""
    return ~(torch.isfinite(x).all(-1).all(-1) & torch.isfinite(r).all(-1).all(-1))


@pytest.mark.parametrize('shape', RN_SHAPES, ids=lambda s: f'{s[0] * s[1]}x{s[2] * s[3]}')
@pytest.mark.parametrize('operand', RN_OPERANDS)
def test_res_norm_is_the_two_pass_form_bit_for_bit(operand, shape):
    x, r = rn_case(operand, shape)
    xd, rd = x.to(DEV), r.to(DEV)
    bad = poisoned(x, r)
    for relu in (False, True):
        want = two_pass(xd, rd, relu)
        got = ops.instance_norm(xd, res=rd.clone(), relu=relu, res_norm=True)
        assert torch.equal(bits(got), bits(want)), (operand, shape, relu)
        xin = xd.clone()                                            # in place, as the encoder calls it
        ops.instance_norm(xin, res=rd.clone(), relu=relu, out=xin, res_norm=True)
        assert torch.equal(bits(xin), bits(want))
        # a poisoned plane is NaN throughout without ReLU and 0 throughout with it (v_max), as in scf_instance_norm
        if bool(bad.any()):
            g = got.cpu()[bad]
            assert bool((g == 0).all()) if relu else bool(torch.isnan(g).all())
        ref, bound = res_norm_ref(x, r, relu)
        ok = ~bad.numpy()
        worst = worst_ratio(got.cpu().numpy()[ok], ref[ok], bound[ok])
        measured(f'res_norm {shape} {operand} relu={relu}, error / bound', worst)
        assert worst <= 1.0


@pytest.mark.parametrize('operand', RN_OPERANDS)
def test_res_norm_fallback_routes(operand):
    """planes the fused kernel does not take run the two launches: a 4 x 4100 plane set whose pointer is not 16-byte aligned
    (generic kernel), HW % 4 != 0 (generic kernel) and a plane past 16384 floats (<8,1024>)."""
    for shape, mis in (((2, 2, 41, 100), True), ((2, 2, 5, 7), False), ((1, 2, 4, 4100), False)):
        x, r = rn_case(operand, shape)
        n = x.numel()

        def place(t):
            base = torch.zeros((n + 8,), device=DEV)
            o = 1 if mis else 4
            base[o:o + n] = t.flatten().to(DEV)
            return base[o:o + n].view(shape)

        xd, rd = place(x), place(r)
        assert (xd.data_ptr() % 16 != 0) == mis
        bad = poisoned(x, r)
        for relu in (False, True):
            want = two_pass(xd, rd, relu)
            got = ops.instance_norm(xd, res=place(r), relu=relu, res_norm=True)
            assert torch.equal(bits(got), bits(want)), (operand, shape, relu)
            ref, bound = res_norm_ref(x, r, relu, aligned=not mis)
            ok = ~bad.numpy()
            worst = worst_ratio(got.cpu().numpy()[ok], ref[ok], bound[ok])
            measured(f'res_norm fallback {shape} {operand} relu={relu}, error / bound', worst)
            assert worst <= 1.0


def test_res_norm_rejects_a_missing_or_misshapen_residual():
    x = torch.zeros((1, 2, 8, 8), device=DEV)
    with pytest.raises(ValueError):
        ops.instance_norm(x, res_norm=True)
    with pytest.raises(ValueError):
        ops.instance_norm(x, res=torch.zeros((1, 2, 8, 4), device=DEV), res_norm=True)


# ======================================================================================================================
# The shared-input launch (conv_dma.hip, SH): the 3x3 / s2 / pad-1 first convolution of a down-sampling block and the
# 1x1 / s2 / pad-0 shortcut on the same input, through ops.conv2d_pair.  Where the 3x3 layer takes a full-grid pixel-split
# tile the pair is ONE launch; the outputs are those of the two ops.conv2d launches bit for bit, the log names both layers.
# ======================================================================================================================
import ctypes as C  # noqa: E402

import torch.nn.functional as F  # noqa: E402

EPS = 2.0 ** -24
DIRECT_BUDGET = 24.0                # err / (eps sum|w||x|) of the direct kernels (tests/test_gpu_ops.py, _winograd_stress)


def rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def pixel_split(pc, x):
    """does the LDS-DMA dispatch give this layer a pixel-split tile at this batch?  (the criterion of tests/test_gpu_gru.py:
    a K-split block holds 32 pixels of one channel fragment, a pixel-split tile at least 128)"""
    d, out = ops.conv2d(pc, x, _launch=False)
    info = (C.c_int32 * 4)()
    assert ops._lib.load().scf_conv2d_query(C.byref(d), info) == 0
    n, _, ho, wo = out.shape
    return not info[2] * 48 > n * ho * wo * (-(-pc.cout // 32))


def block_layers(cin, cout, form, seed):
    """(conv1 3x3 / s2, shortcut 1x1 / s2) of a down-sampling block and their float64 restatements: the IN form has plain
    epilogues, the BN form a folded BatchNorm on both and ReLU on conv1."""
    w3 = rnd((cout, cin, 3, 3), seed, (1.0 / (9 * cin)) ** 0.5)
    w1 = rnd((cout, cin, 1, 1), seed + 1, (1.0 / cin) ** 0.5)
    b3, b1 = rnd((cout,), seed + 2, 0.1), rnd((cout,), seed + 3, 0.1)
    bn3 = bn1 = None
    if form == 'BN':
        mk = lambda s: (1.0 + rnd((cout,), s, 0.1), rnd((cout,), s + 1, 0.1), rnd((cout,), s + 2, 0.1), 0.5 + rnd((cout,), s + 3).abs())
        bn3, bn1 = mk(seed + 10), mk(seed + 20)
    dev = lambda t: None if t is None else tuple(v.to(DEV) for v in t)
    pc3 = ops.PackedConv.from_weight(w3.to(DEV), b3.to(DEV), 2, 1, bn=dev(bn3))
    pc1 = ops.PackedConv.from_weight(w1.to(DEV), b1.to(DEV), 2, 0, bn=dev(bn1))

    def ref(x, w, b, bn, pad, relu):
        """(float64 value, eps-unit scale sum|w||x| + |b|, both through the fold)"""
        y = F.conv2d(x.double(), w.double(), b.double(), stride=2, padding=pad)
        s = F.conv2d(x.double().abs(), w.double().abs(), b.double().abs(), stride=2, padding=pad)
        if bn is not None:
            g, beta, mean, var = (t.double().view(1, -1, 1, 1) for t in bn)
            k = g / torch.sqrt(var + 1e-5)
            y, s = (y - mean) * k + beta, (s + mean.abs()) * k.abs() + beta.abs()
        return (torch.relu(y) if relu else y), s

    act3 = ops.ACT_RELU if form == 'BN' else ops.ACT_NONE
    return (pc3, dict(act=act3), lambda x: ref(x, w3, b3, bn3, 1, form == 'BN')), (pc1, dict(), lambda x: ref(x, w1, b1, bn1, 0, False))


def run_pair(l3, l1, xd):
    rec = ops.record_conv_kernels()
    with rec as ran:
        y3, y1 = ops.conv2d_pair((l3[0], xd, l3[1]), (l1[0], xd, l1[1]))
    torch.cuda.synchronize()
    return y3, y1, ran, rec.paired


def check_pair(n, cin, cout, h, w, form, expect_merged, seed=300):
    l3, l1 = block_layers(cin, cout, form, seed)
    x = rnd((n, cin, h, w), seed + 50)
    xd = x.to(DEV)
    want3 = ops.conv2d(l3[0], xd, **l3[1])
    want1 = ops.conv2d(l1[0], xd, **l1[1])
    y3, y1, ran, paired = run_pair(l3, l1, xd)
    assert torch.equal(y3, want3) and torch.equal(y1, want1), (n, cin, cout, h, w, form)
    assert len(ran) == 2 and [k for _, k in ran] == ['direct-dma', 'direct-dma'], ran
    assert ran[0][0].startswith(f'{cin}->{cout} 3x3/s2') and ran[1][0].startswith(f'{cin}->{cout} 1x1/s2'), ran
    if expect_merged is not None:
        assert paired == ([1, 2] if expect_merged else [0, 0]), (paired, ran)
    prev = ops.tune('conv_pair', 1)
    try:
        o3, o1, ran_off, paired_off = run_pair(l3, l1, xd)
    finally:
        ops.tune('conv_pair', prev)
    assert paired_off == [0, 0] and ran_off == ran
    assert torch.equal(o3, want3) and torch.equal(o1, want1)
    for name, got, layer in (('conv1', y3, l3), ('shortcut', y1, l1)):
        ref, scale = layer[2](x)
        r = float(((got.cpu().double() - ref).abs() / (EPS * scale)).max())
        print(f'[measured] shared-input {form} {cin}->{cout} @{h}x{w} N{n} {name}: err / (eps sum|w||x|) = {r:.2f}')
        assert r <= DIRECT_BUDGET, (name, r)


def smallest_pixel_split_n(cin, cout, h, w, lo=1, hi=64):
    pc3 = block_layers(cin, cout, 'IN', 300)[0][0]
    for n in range(lo, hi + 1):
        if pixel_split(pc3, torch.zeros((n, cin, h, w), device=DEV)):
            return n
    raise AssertionError('no pixel-split batch up to %d' % hi)


@pytest.mark.parametrize('form', ['IN', 'BN'])
@pytest.mark.parametrize('shape', [(16, 64, 96, 128, 128), (32, 96, 128, 64, 64)], ids=lambda s: 'x'.join(map(str, s)))
def test_shared_input_launch_equals_two_launches(shape, form):
    n, cin, cout, h, w = shape
    pc3 = block_layers(cin, cout, 'IN', 300)[0][0]
    if not pixel_split(pc3, torch.zeros((n, cin, h, w), device=DEV)):       # (a device with more CUs)
        n = smallest_pixel_split_n(cin, cout, h, w, lo=n)
    check_pair(n, cin, cout, h, w, form, expect_merged=True)


@pytest.mark.parametrize('form', ['IN', 'BN'])
def test_shared_input_launch_ragged_map(form):
    """60 x 80: Ho = 30 and Wo = 40 are no multiples of the tile (8-column fragments, 16 rows), W % 4 == 0."""
    n = smallest_pixel_split_n(64, 96, 60, 80)
    check_pair(n, 64, 96, 60, 80, form, expect_merged=True)


@pytest.mark.parametrize('form', ['IN', 'BN'])
def test_shared_input_launch_unaligned_width(form):
    """W % 4 != 0: the aligned x4 patch staging is refused, the dword gather stages the patch (odd sizes: the last window
    row and column reach into the padding)."""
    n = smallest_pixel_split_n(64, 96, 61, 78)
    check_pair(n, 64, 96, 61, 78, form, expect_merged=None)
    assert pixel_split(block_layers(64, 96, 'IN', 300)[0][0], torch.zeros((n, 64, 61, 78), device=DEV))


@pytest.mark.parametrize('n', [1, 2])
@pytest.mark.parametrize('form', ['IN', 'BN'])
def test_shared_input_form_on_small_grids_is_two_launches(form, n):
    """batch 1 and 2: the 3x3 layer takes the K-split tile, the pair runs as its two launches"""
    check_pair(n, 64, 96, 64, 64, form, expect_merged=False)
    check_pair(n, 96, 128, 32, 32, form, expect_merged=False)
