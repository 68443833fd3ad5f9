"""GPU: corr_lookup_grad.hip (scf_corr_lookup_grad), MotionEncoder.backward, SCFlowDecoder.keep = 'motion' /
motion_backward and SCFlowRefiner.loss_and_motion_grads against the float64 restatements and the derived bounds of
tests/test_motion_grad_host.py.  Every comparison is `error <= bound` over ALL elements (ratio <= 1) or bit equality; the
one relative tolerance is the fixture's measured float64-vs-fp32 margin.  The measured ratios are recorded in DESIGN.md
section 4.12."""
import numpy as np
import pytest
import torch

from scflow_amd import _lib, ops
from scflow_amd._lib import ScflowHipError
from scflow_amd.modules import MotionEncoder
import test_motion_grad_host as MH
import test_loss_host as HL
from test_head_grad_host import RELU, act_grad_ref, dgrad_ref, wgrad_ref
from test_stream_ops_host import f64, measured, same_bits, worst_ratio  # noqa: E402
from test_gpu_gru_grad import scflow_model  # noqa: F401  (the small random-weight refiner, a module-scoped fixture)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = -7777.25
GUARD = 64
EINVAL, EUNSUPPORTED = -1, -2                   # include/scflow_hip.h
cpu = lambda t: t.detach().cpu()                                    # noqa: E731


def D(t):
    return None if t is None else t.to(DEV).contiguous()


def guarded(q, h, w, prev=None):
    """a (Q, h, w) output between two sentinel guards -> (whole buffer, view)"""
    buf = torch.full((q * h * w + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    out = buf[GUARD:GUARD + q * h * w].view(q, h, w)
    if prev is not None:
        out.copy_(prev)
    return buf, out


def guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


# ===================================================================================================== the lookup adjoint
# (N, T, h, w, r, L): every launch geometry of corr_lookup_grad.hip, listed and explained next to the restatement;
# tests/test_motion_grad_host.py::test_lookup_route_coverage holds the list to the library's own route decision
KERNEL_SHAPES = MH.KERNEL_SHAPES


def _run(g_corr, fl, mask, r, L, prev=None):
    T, n, _, h, w = g_corr.shape
    buf, out = guarded(n * h * w, h, w, prev)
    got = ops.corr_lookup_grad(D(g_corr), D(fl), D(mask), r, L, out=out, accumulate=prev is not None)
    assert got.data_ptr() == out.data_ptr() and guards_intact(buf), 'a guard was written'
    return out


@pytest.mark.parametrize('with_mask', [False, True], ids=['plain', 'masked'])
@pytest.mark.parametrize('shape', KERNEL_SHAPES, ids=MH.shape_id)
def test_lookup_adjoint_against_float64(shape, with_mask):
    n, T, h, w, r, L = shape
    g_corr, fl, mask = MH.adjoint_case(n, T, h, w, r, L, with_mask=with_mask)
    rows = MH.kernel_rows(shape)        # the two largest maps: a few hundred rows restated, every row in the checks below
    ref, bound = MH.lookup_adjoint(g_corr, fl, mask, r, L, rows=rows)
    got = _run(g_corr, fl, mask, r, L)
    assert bool(torch.isfinite(got).all())
    v = worst_ratio(cpu(got if rows is None else got[torch.from_numpy(rows).to(DEV)]), ref, bound)
    measured(f'corr_lookup_grad {shape} mask {with_mask}, worst error / bound', v)
    assert v <= 1.0
    assert same_bits(got, _run(g_corr, fl, mask, r, L)), 'two runs differ'
    # accumulate: previous + result, one fp32 addition
    prev = D(torch.randn((n * h * w, h, w), generator=MH.gen(11)))
    acc = _run(g_corr, fl, mask, r, L, prev=prev)
    assert same_bits(acc, prev + got)
    # a NaN / inf query contributes nothing at its iteration, whatever its cotangents hold, and no other row changes:
    # the same bits as with that query's flow finite and its cotangents zero
    bad = ~torch.isfinite(fl).all(2)                                    # (T, N, h, w)
    assert int(bad.sum()) == 2 * T
    g_nan, g_zero, fl_ok = g_corr.clone(), g_corr.clone(), fl.clone()
    sel = bad[:, :, None].expand_as(g_corr)
    g_nan[sel], g_zero[sel] = float('nan'), 0.0
    fl_ok[bad[:, :, None].expand_as(fl)] = 0.5
    assert same_bits(got, _run(g_nan, fl, mask, r, L)) and same_bits(got, _run(g_zero, fl_ok, mask, r, L))
    if T == 1:                                                          # its own row is then exactly zero
        rows = bad[0].reshape(-1).nonzero().flatten()
        assert not cpu(got)[rows].any()
    if n == 2:                                                          # a sample alone == the same sample inside the batch
        one = _run(g_corr[:, 1:], fl[:, 1:], None if mask is None else mask[:, 1:], r, L)
        assert same_bits(one, got[h * w:])


@pytest.mark.parametrize('with_mask', [False, True], ids=['plain', 'masked'])
@pytest.mark.parametrize('shape', MH.EXACT_SHAPES, ids=MH.shape_id)
def test_lookup_adjoint_on_exact_operands_bit_for_bit(shape, with_mask):
    """operands on which no operation rounds (MH.exact_case; the host test shows fp32 == float64 on them): the kernel's
    bits are float64's, on each route, so a cell that gathers a wrong tap, level or query cannot hide inside a bound"""
    n, T, h, w, r, L = shape
    g_corr, fl, mask = MH.exact_case(n, T, h, w, r, L, with_mask=with_mask)
    ref, _ = MH.lookup_adjoint(g_corr, fl, mask, r, L)
    want = torch.from_numpy(ref.astype(np.float32))
    assert np.array_equal(f64(want), ref)
    got = _run(g_corr, fl, mask, r, L)
    wrong = int((cpu(got).view(torch.int32) != want.view(torch.int32)).sum())
    measured(f'corr_lookup_grad {shape} mask {with_mask} on exact operands, elements whose bits differ', wrong)
    assert wrong == 0
    prev = D(torch.randint(-8, 9, (n * h * w, h, w), generator=MH.gen(12)).float())       # previous + result: exact too
    assert same_bits(_run(g_corr, fl, mask, r, L, prev=prev), prev + D(want))


def test_a_single_iteration_may_come_without_the_leading_axis():
    g_corr, fl, mask = MH.adjoint_case(1, 1, 8, 8, 4, 4)
    a = ops.corr_lookup_grad(D(g_corr), D(fl), D(mask))
    b = ops.corr_lookup_grad(D(g_corr[0]), D(fl[0]), D(mask[0]))
    assert a.shape == (64, 8, 8) and same_bits(a, b)


def test_c_abi_rejections_leave_the_output_unwritten():
    lib = _lib.load()
    T, n, h, w, r, L = 2, 1, 8, 8, 4, 4
    g_corr, fl, mask = (D(v) for v in MH.adjoint_case(n, T, h, w, r, L))
    buf, out = guarded(n * h * w, h, w)
    P = lambda t: t.data_ptr()                                          # noqa: E731
    ok = [P(g_corr), P(fl), P(mask), P(out), 0, T, n, h, w, r, L, None]
    cases = [(0, None, EINVAL), (1, None, EINVAL), (3, None, EINVAL), (5, 0, EINVAL), (5, -1, EINVAL), (6, 0, EINVAL),
             (7, 0, EINVAL), (8, 0, EINVAL), (9, 0, EINVAL), (10, 0, EINVAL), (10, 5, EINVAL),       # 8 >> 4: an empty level
             (10, _lib.MAX_LEVELS + 1, EUNSUPPORTED), (5, ops.TAIL_MAX_T + 1, EUNSUPPORTED)]
    for at, v, code in cases:
        bad = list(ok)
        bad[at] = v
        assert lib.scf_corr_lookup_grad(*bad) == code, (at, v)
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())
    for kw in (dict(radius=0), dict(num_levels=5), dict(num_levels=3), dict(accumulate=True)):
        with pytest.raises(ScflowHipError):
            ops.corr_lookup_grad(g_corr, fl, mask, **kw)
    with pytest.raises(ScflowHipError):
        ops.corr_lookup_grad(g_corr, fl[:1], mask)
    with pytest.raises(ScflowHipError):
        ops.corr_lookup_grad(g_corr, fl, mask[:, :, :, :4])
    with pytest.raises(ScflowHipError):
        ops.corr_lookup_grad(g_corr, fl, mask, out=torch.empty((n * h * w, 1, h, w), device=DEV))
    with pytest.raises(ScflowHipError):
        ops.corr_lookup_grad(cpu(g_corr), cpu(fl))


# ================================================================================================ MotionEncoder.backward
def _encoder(seed=0, params=None):
    enc = MotionEncoder(4, 4, 'Basic', None, None, dict(type='ReLU'))
    gen = torch.Generator().manual_seed(900 + seed)
    with torch.no_grad():
        for name, prm in enc.named_parameters():
            if params is not None:
                prm.copy_(params[name])
            else:
                fan = prm[0].numel() if prm.dim() > 1 else 1
                prm.copy_(torch.randn(prm.shape, generator=gen) * (2.0 * fan ** -0.5 if prm.dim() > 1 else 0.1))
    return enc.to(DEV)


def _enc_forward(enc, corr, flows):
    """the decoder's use of the encoder, an iteration at a time -> saved (corr, x)"""
    x = torch.empty((corr.shape[0], corr.shape[1], 128) + tuple(corr.shape[3:]), device=DEV)
    for t in range(corr.shape[0]):
        enc(corr[t], flows[t], out=x[t])
    return dict(corr=corr.contiguous(), x=x)


def _check_encoder_launches(enc, saved, im, got, prev=None, prefix=''):
    """every launch of MotionEncoder.backward against float64 GIVEN the GPU's own operands of that launch -> worst error /
    bound per kind of launch; no bound is carried from launch to launch"""
    g_corr, g_fl, grads = got
    T, n, kc, h, w = saved['corr'].shape
    m = T * n
    W = {k: f64(v) for k, v in enc.named_parameters()}
    co, cc = 126, 192
    x_, corr_ = cpu(saved['x']).view(m, co + 2, h, w), cpu(saved['corr']).view(m, kc, h, w)
    c1, f1, cf = (cpu(im[k]).flatten(0, 1) for k in ('c1', 'f1', 'cf'))
    g_x, u, g_cf, g_c1, g_f1 = (cpu(im[k]) for k in ('g_x', 'u', 'g_cf', 'g_c1', 'g_f1'))
    worst = {}

    def hold(kind, have, ref, bound):
        worst[kind] = max(worst.get(kind, 0.0), worst_ratio(cpu(have), ref, bound))

    def wgrad(name, g, xin, k):
        pw = None if prev is None else prev[f'{prefix}{name}.conv.weight']
        pb = None if prev is None else prev[f'{prefix}{name}.conv.bias']
        dw, bw, db, bb = wgrad_ref(g, 0.0, xin, *k, prev=pw, prev_b=pb)
        hold('wgrad ' + name, grads[f'{prefix}{name}.conv.weight'], dw, bw)
        hold('bias ' + name, grads[f'{prefix}{name}.conv.bias'], db, bb)

    hold('act_grad', u, *act_grad_ref(g_x[:, :co], 0.0, x_[:, :co], RELU))
    wgrad('out_net.0', u, cf, (3, 3))
    hold('dgrad out_net.0', g_cf, *dgrad_ref(u, 0.0, W['out_net.0.conv.weight'], a=cf, act=RELU))
    wgrad('corr_net.1', g_cf[:, :cc], c1, (3, 3))
    hold('dgrad corr_net.1', g_c1, *dgrad_ref(g_cf[:, :cc], 0.0, W['corr_net.1.conv.weight'], a=c1, act=RELU))
    wgrad('corr_net.0', g_c1, corr_, (1, 1))
    hold('dgrad corr_net.0', im['g_corr'], *dgrad_ref(g_c1, 0.0, W['corr_net.0.conv.weight']))
    wgrad('flow_net.1', g_cf[:, cc:], f1, (3, 3))
    hold('dgrad flow_net.1', g_f1, *dgrad_ref(g_cf[:, cc:], 0.0, W['flow_net.1.conv.weight'], a=f1, act=RELU))
    wgrad('flow_net.0', g_f1, x_[:, co:], (7, 7))
    hold('dgrad flow_net.0', im['g_flow_in'], *dgrad_ref(g_f1, 0.0, W['flow_net.0.conv.weight'], add=g_x[:, co:]))
    # the hand-overs: what is returned is what the last launches wrote
    assert same_bits(g_corr.reshape(m, kc, h, w), im['g_corr'])
    assert all(same_bits(g_fl[t], im['g_flow_in'].view(T, n, 2, h, w)[t]) for t in range(T))
    return worst


@pytest.mark.parametrize('T, hw', [(1, (8, 8)), (2, (12, 20))], ids=['T1-8x8', 'T2-12x20'])
def test_encoder_backward_launch_by_launch(T, hw):
    n = 2
    gen = MH.gen(1200 + T)
    enc = _encoder()
    corr = D(torch.randn((T, n, 324, *hw), generator=gen))
    flows = D(torch.randn((T, n, 2, *hw), generator=gen) * 3)
    saved = _enc_forward(enc, corr, flows)
    g_xs = [D(torch.randn((n, 128, *hw), generator=gen)) for _ in range(T)]
    im = {}
    got = enc.backward(saved, g_xs, intermediates=im)
    g_corr, g_fl, grads = got
    assert sorted(grads) == sorted(MH.ENC_NAMES) == sorted(enc.param_names()) and len(g_fl) == T
    assert g_corr.shape == (T, n, 324, *hw) and all(v.shape == (n, 2, *hw) for v in g_fl)
    # the recomputed activations are the forward's: out_net on the recomputed cf gives the kept x, bit for bit
    for t in range(T):
        assert same_bits(enc.out_net[0](im['cf'][t]), saved['x'][t][:, :126]) and same_bits(saved['x'][t][:, 126:], flows[t])
    again = enc.backward(saved, g_xs)
    assert same_bits(again[0], g_corr) and all(same_bits(a, b) for a, b in zip(again[1], g_fl))
    assert all(same_bits(again[2][k], grads[k]) for k in grads), 'two runs differ'
    for kind, v in _check_encoder_launches(enc, saved, im, got).items():
        measured(f'MotionEncoder.backward {hw} T {T} {kind}, error / bound', v)
        assert v <= 1.0, kind
    # accumulating into a dict passed in: previous + sum, behind a prefix
    prev = {'encoder.' + k: D(torch.randn(v.shape, generator=gen)) for k, v in grads.items()}
    into = {k: v.clone() for k, v in prev.items()}
    into['other'] = prev['encoder.out_net.0.conv.bias']
    im2 = {}
    acc = enc.backward(saved, g_xs, param_grads=into, intermediates=im2, prefix='encoder.')
    assert acc[2] is into and set(into) == set(prev) | {'other'}
    assert all(same_bits(into['encoder.' + k], grads[k] + prev['encoder.' + k]) for k in grads)
    for kind, v in _check_encoder_launches(enc, saved, im2, acc, prev={k: cpu(v) for k, v in prev.items()}, prefix='encoder.').items():
        assert v <= 1.0, kind
    if T == 2:
        one = enc.backward(dict(corr=saved['corr'][1:].contiguous(), x=saved['x'][1:].contiguous()), g_xs[1:])
        assert same_bits(one[0][0], g_corr[1]) and same_bits(one[1][0], g_fl[1])        # a sample's result does not depend on T
        name = MH.ENC_NAMES[0]
        with pytest.raises(ScflowHipError):
            enc.backward(saved, g_xs, param_grads={name: D(torch.zeros_like(cpu(grads[name])))})
        with pytest.raises(ScflowHipError):
            enc.backward(saved, [])
        with pytest.raises(ScflowHipError):
            enc.backward(saved, g_xs[:1])
        with pytest.raises(ScflowHipError):
            enc.backward({'x': saved['x']}, g_xs)
        with pytest.raises(ScflowHipError):
            enc.backward(dict(saved, corr=saved['corr'][:, :, :81]), g_xs)
        with pytest.raises(ScflowHipError):
            enc.backward(dict(saved, x=saved['x'].transpose(3, 4)), g_xs)
        with pytest.raises(ScflowHipError):
            enc.backward(saved, [g[:, :126] for g in g_xs])


def test_encoder_backward_refuses_more_iterations_than_the_tail():
    enc = _encoder()
    T = ops.TAIL_MAX_T + 1
    z = lambda *s: torch.zeros(s, device=DEV)                        # noqa: E731
    with pytest.raises(ScflowHipError):
        enc.backward(dict(corr=z(T, 1, 324, 2, 2), x=z(T, 1, 128, 2, 2)), [z(1, 128, 2, 2)] * T)


# ===================================================================== the reference's own pyramid, lookup and encoder
def test_kernels_against_the_reference_fixture():
    """corr_build, corr_lookup, the encoder, MotionEncoder.backward and corr_lookup_grad on the fixture's seeds against the
    reference's recorded fp32 CPU autograd: two fp32 evaluations around the float64 restatement, held to the margin
    tests/test_motion_grad_host.py measured for the reference's own; the kernels' own, tighter bounds are the tests above."""
    z = np.load(MH.GOLDEN)
    s = MH.GOLDEN_SHAPE
    p, f1, f2, flows, cots = MH.golden_case()
    enc = _encoder(params=p)
    pyr = ops.corr_build(D(f1), D(f2), s['L'])
    fl = D(flows)
    corr = torch.stack([ops.corr_lookup(pyr, fl[t], s['r']) for t in range(s['T'])])
    saved = _enc_forward(enc, corr, fl)
    g_corr, g_fl, grads = enc.backward(saved, [D(cots[t]) for t in range(s['T'])])
    got = dict(grads, g_vol=ops.corr_lookup_grad(g_corr, fl, None, s['r'], s['L']))
    for t in range(s['T']):
        got[f'g_corr.{t}'], got[f'g_flow_in.{t}'] = g_corr[t], g_fl[t]
    for key in MH.GOLDEN_KEYS:
        have = MH.golden_pick(key, cpu(got[key]).numpy())
        rel = float(np.abs(have - z[key]).max() / np.abs(z[key]).max())
        measured(f'kernels - reference fixture {key}, relative to the largest entry', rel)
        assert rel <= MH.GOLDEN_MARGIN, key


# ================================================================================================= the refiner's entry
KEPT = ['c', 'd_flow', 'dm', 'flow_lr', 'h0', 'hv', 'mask', 'pyramid', 'tail_inputs', 'tiled', 'x', 'y0', 'y1', 'y2']


def _check_volume(dec, saved, im, g_vol):
    """the lookup adjoint of motion_backward against float64 GIVEN the GPU's own g_corr"""
    T, n, _, h, w = saved['flow_lr'].shape
    g_corr = cpu(im['g_corr']).view(T, n, -1, h, w)
    mp = None if im['mask_prev'] is None else cpu(im['mask_prev'])
    ref, bound = MH.lookup_adjoint(g_corr, cpu(saved['flow_lr']), mp, dec.radius, dec.num_levels)
    return worst_ratio(cpu(g_vol), ref, bound)


def test_loss_and_motion_grads(scflow_model):  # noqa: F811
    m, case = scflow_model
    data = HL.refiner_data(case, DEV)
    base = m.loss_and_gru_grads(None, data=data)
    loss, log_imgs, log_vars, seq_r, seq_t, grads = m.loss_and_motion_grads(None, data=data)
    assert same_bits(loss, base[0]) and list(log_vars.items()) == list(base[2].items()) and log_imgs is None
    assert sorted(grads) == sorted(list(base[5]) + ['motion'])
    dec = m.decoder
    enc_names = {'decoder.encoder.' + k for k in dict(dec.encoder.named_parameters())}
    assert set(grads['params']) == set(base[5]['params']) | enc_names and len(enc_names) == 10
    assert set(grads['params']) >= {'decoder.' + k for k in dict(dec.named_parameters())}, 'a decoder parameter has no gradient'

    def same(a, b):
        if isinstance(a, dict):
            return sorted(a) == sorted(b) and all(same(a[k], b[k]) for k in a)
        if isinstance(a, (list, tuple)):
            return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
        return same_bits(a, b)
    for key, v in base[5].items():
        assert same({k: grads[key][k] for k in v} if key == 'params' else grads[key], v), key
    assert dec.keep == 'none'
    saved = dec.kept
    assert sorted(saved) == KEPT
    mo = grads['motion']
    T, n, _, h, w = saved['flow_lr'].shape
    assert sorted(mo) == ['correlation', 'flow_inputs'] and len(mo['flow_inputs']) == dec.iters == T
    assert mo['correlation'].shape == (n * h * w, h, w) and all(v.shape == (n, 2, h, w) for v in mo['flow_inputs'])
    # the stage again, with its operands: the same bits, and every launch inside its bound
    im = {}
    g_x = grads['gru']['motion_features']
    g_vol, g_fl, params = dec.motion_backward(saved, g_x, intermediates=im)
    assert same_bits(g_vol, mo['correlation']) and all(same_bits(a, b) for a, b in zip(g_fl, mo['flow_inputs']))
    assert all(same_bits(params[k], grads['params']['decoder.' + k]) for k in params) and len(params) == 10
    for t in range(T):                              # the recomputed lookup feeds the forward's own encoder: it gives the kept x
        assert same_bits(dec.encoder(im['corr'][t], saved['x'][t][:, 126:].contiguous()), saved['x'][t])
    g_corr = im['g_corr'].view(T, n, -1, h, w)
    for kind, v in _check_encoder_launches(dec.encoder, dict(corr=im['corr'], x=saved['x']), im, (g_corr, g_fl, params),
                                           prefix='encoder.').items():
        measured(f'loss_and_motion_grads {kind}, error / bound', v)
        assert v <= 1.0, kind
    v = _check_volume(dec, saved, im, g_vol)
    measured('loss_and_motion_grads correlation volume, error / bound', v)
    assert v <= 1.0 and bool(g_vol.any())
    # accumulation and the error paths of the decoder's entry
    into = {k: v.clone() for k, v in params.items()}
    dec.motion_backward(saved, g_x, param_grads=into)
    assert all(same_bits(into[k], params[k] + params[k]) for k in params)
    with pytest.raises(ScflowHipError):
        dec.motion_backward({k: v for k, v in saved.items() if k != 'flow_lr'}, g_x)
    with pytest.raises(ScflowHipError):
        dec.motion_backward(saved, [])
    with pytest.raises(ScflowHipError):
        dec.motion_backward(saved, g_x[:1])
    with pytest.raises(ScflowHipError):
        dec.motion_backward(dict(saved, flow_lr=saved['flow_lr'][:, :, :1]), g_x)
    with pytest.raises(ScflowHipError):
        dec.motion_backward(saved, g_x, param_grads={'encoder.out_net.0.conv.bias': into['encoder.out_net.0.conv.bias']})
    # the configurations in which a cotangent re-enters iteration t - 1 are refused, by name
    try:
        dec.detach_flow = False
        with pytest.raises(NotImplementedError, match='detach_flow'):
            m.loss_and_motion_grads(None, data=data)
        dec.detach_flow, dec.detach_mask, dec.mask_flow = True, False, True
        with pytest.raises(NotImplementedError, match='detach_mask'):
            m.loss_and_motion_grads(None, data=data)
        dec.mask_flow, dec.mask_corr = False, True
        with pytest.raises(NotImplementedError, match='detach_mask'):
            m.loss_and_motion_grads(None, data=data)
    finally:
        dec.detach_flow, dec.detach_mask, dec.mask_flow, dec.mask_corr = True, True, False, False
    with pytest.raises(NotImplementedError, match='loss_and_motion_grads'):
        m.forward(data, return_loss=True)
    with pytest.raises(NotImplementedError, match='loss_and_gru_grads'):
        m.forward(data, return_loss=True)


def _get_pose(m, data):
    return m.get_pose(data['rendered_images'], data['real_images'], data['ref_rotations'], data['ref_translations'],
                      data['rendered_depths'], data['internel_k'], data['labels'])


def test_keeping_the_motion_inputs_changes_no_bit(scflow_model):  # noqa: F811
    m, case = scflow_model
    data = HL.refiner_data(case, DEV)
    dec = m.decoder
    old = dec.c_iteration
    kept = {}
    try:
        for c_iteration in (True, False):
            dec.c_iteration = c_iteration
            dec.kept = {}
            off = _get_pose(m, data)
            assert dec.kept == {}
            dec.keep = 'motion'
            on = _get_pose(m, data)
            dec.keep = 'none'
            kept[c_iteration] = dict(dec.kept)
            kept[c_iteration]['flow_lr'] = kept[c_iteration]['flow_lr'].clone()
            for a, b in zip(off, on):
                assert all(same_bits(x, y) for x, y in zip(a, b)), f'c_iteration {c_iteration}'
    finally:
        dec.keep, dec.c_iteration = 'none', old
    sc, sp = kept[True], kept[False]
    assert sorted(sc) == sorted(sp) == KEPT
    T, n, _, h, w = sc['x'].shape
    assert sc['flow_lr'].shape == (T, n, 2, h, w) and sc['flow_lr'].is_contiguous() and sc['tiled'] == sp['tiled']
    assert len(sc['pyramid']) == dec.num_levels and all(same_bits(a, b) for a, b in zip(sc['pyramid'], sp['pyramid']))
    assert all(same_bits(sc[k], sp[k]) for k in sc if k not in ('pyramid', 'tiled', 'tail_inputs')), 'the two loop forms keep different tensors'
    assert len(sc['tail_inputs']) == len(sp['tail_inputs']) == T and all(same_bits(a, b) for a, b in zip(sc['tail_inputs'], sp['tail_inputs']))
    assert not same_bits(sc['flow_lr'][0], sc['flow_lr'][1])
    # the kept tensors are the forward's own: lookup + encoder run again from them give the kept x
    for t in range(T):
        corr = ops.corr_lookup(sc['pyramid'], sc['flow_lr'][t], dec.radius, tiled_levels=sc['tiled'])
        assert same_bits(dec.encoder(corr, sc['flow_lr'][t]), sc['x'][t])


def test_motion_backward_under_mask_corr(scflow_model):  # noqa: F811
    """mask_corr with detach_mask: the previous iteration's mask (ones before the first) is the lookup adjoint's per-query
    factor and the recomputed correlation is the masked one"""
    m, case = scflow_model
    data = HL.refiner_data(case, DEV)
    dec = m.decoder
    try:
        dec.mask_corr, dec.keep = True, 'motion'
        _get_pose(m, data)
        saved = dict(dec.kept)
        T, n, _, h, w = saved['x'].shape
        gen = MH.gen(77)
        g_x = [D(torch.randn((n, 128, h, w), generator=gen)) for _ in range(T)]
        im = {}
        g_vol, g_fl, params = dec.motion_backward(saved, g_x, intermediates=im)
        assert same_bits(im['mask_prev'][0], torch.ones_like(saved['mask'][0])) and same_bits(im['mask_prev'][1:], saved['mask'][:-1])
        for t in range(T):
            plain = ops.corr_lookup(saved['pyramid'], saved['flow_lr'][t], dec.radius, tiled_levels=saved['tiled'])
            assert same_bits(im['corr'][t], plain * im['mask_prev'][t])
            assert same_bits(dec.encoder(im['corr'][t], saved['x'][t][:, 126:].contiguous()), saved['x'][t])
        v = _check_volume(dec, saved, im, g_vol)
        measured('motion_backward under mask_corr, correlation volume error / bound', v)
        assert v <= 1.0
        with pytest.raises(ScflowHipError):
            dec.motion_backward({k: v for k, v in saved.items() if k != 'mask'}, g_x)
    finally:
        dec.mask_corr, dec.keep = False, 'none'
        dec.kept = {}
