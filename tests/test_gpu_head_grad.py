"""GPU: conv_s1_grad.hip (scf_conv_s1_dgrad, scf_conv_s1_wgrad, scf_conv_s1_wgrad_workspace, scf_act_grad),
SCFlowDecoder.heads_backward / keep = 'decoder_heads' and SCFlowRefiner.loss_and_decoder_head_grads against the float64
restatements and the derived bounds of tests/test_head_grad_host.py.  Every comparison is `error <= bound` over ALL
elements (ratio <= 1) or bit equality; there is no absolute tolerance.  The measured ratios are recorded in DESIGN.md
section 4.10."""
import json
import os

import numpy as np
import pytest
import torch

import scflow_amd
from scflow_amd import _lib, ops
from scflow_amd._lib import ScflowHipError
import test_head_grad_host as HH
import test_loss_host as HL
from test_fc_host import gamma  # noqa: E402
from test_stream_ops_host import f64, measured, same_bits, worst_ratio  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = -7777.25
GUARD = 64
EINVAL, EUNSUPPORTED = -1, -2       # include/scflow_hip.h
NONE, RELU, SIGMOID, TANH = HH.ACTS
cpu = lambda t: t.detach().cpu()                                    # noqa: E731


def D(t):
    return None if t is None else t.to(DEV).contiguous()


def guarded(shape):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    return buf, buf[GUARD:GUARD + n].view(shape)


def guard_untouched(buf, shape):
    n = int(np.prod(shape))
    want = torch.full_like(buf, SENTINEL)
    return same_bits(buf[:GUARD], want[:GUARD]) and same_bits(buf[GUARD + n:], want[GUARD + n:])


def sliced(t, before=3, after=2):
    """t (M, C, H, W) as a channel slice of a wider GPU tensor whose other channels hold the sentinel -> (wide, view)"""
    m, c, h, w = t.shape
    wide_ = torch.full((m, before + c + after, h, w), SENTINEL, dtype=torch.float32, device=DEV)
    wide_[:, before:before + c] = t.to(DEV)
    return wide_, wide_[:, before:before + c]


def slice_untouched(wide_, c, before=3):
    rest = torch.cat([wide_[:, :before], wide_[:, before + c:]], 1)
    return bool((rest == SENTINEL).all())


# ====================================================================================================== dgrad, wgrad
def _dgrad(g, w, add=None, a=None, act=NONE, check_rows=True, slices=False, scratch=False):
    """-> (M, Cin, H, W) on the CPU; guard bands (or, with `slices`, every operand a channel slice of a wider tensor whose
    other channels stay intact), two runs, and the rows 0, 16, 32 of a 33-sample run as M = 1 runs"""
    m, cin = g.shape[0], w.shape[1]
    shape = (m, cin, *g.shape[2:])
    ws_ = torch.empty((w.numel(),), device=DEV) if scratch else None
    if slices:
        wides = [sliced(t) if t is not None else (None, None) for t in (g, add, a)]
        owide, out = sliced(torch.zeros(shape))
        got = ops.conv_s1_dgrad(wides[0][1], D(w), wides[1][1], wides[2][1], act, out=out, w_scratch=ws_)
        assert slice_untouched(owide, cin) and all(slice_untouched(wd, v.shape[1]) for wd, v in wides if wd is not None)
    else:
        buf, out = guarded(shape)
        got = ops.conv_s1_dgrad(D(g), D(w), D(add), D(a), act, out=out, w_scratch=ws_)
        assert guard_untouched(buf, shape)
    assert not bool((got == SENTINEL).any())
    again = ops.conv_s1_dgrad(D(g), D(w), D(add), D(a), act)
    assert same_bits(got, again), 'two runs (or the slices, or the transposed scratch) differ'
    full = cpu(got).contiguous()
    if check_rows and m == 33:
        for r in (0, 16, 32):
            row = lambda t: None if t is None else D(t[r:r + 1])      # noqa: E731
            assert same_bits(full[r:r + 1], ops.conv_s1_dgrad(row(g), D(w), row(add), row(a), act)), 'a sample depends on its batch'
    return full


def _wgrad(g, x, kh, kw, prev=None, prev_b=None, slices=False, bias=True):
    m, cout, h, w = g.shape
    cin = x.shape[1]
    need = ops.conv_s1_wgrad_workspace(m, cout, cin, h, w, kh, kw)
    wbuf, dw = guarded((cout, cin, kh, kw))
    bbuf, db = guarded((cout,))
    sbuf, ws = guarded((need,))
    if prev is not None:
        dw.copy_(prev)
        db.copy_(prev_b)
    gd, xd = (sliced(g)[1], sliced(x)[1]) if slices else (D(g), D(x))
    ops.conv_s1_wgrad(gd, xd, (kh, kw), dw=dw, db=db if bias else None, bias=bias, accumulate=prev is not None, workspace=ws)
    assert guard_untouched(wbuf, dw.shape) and guard_untouched(sbuf, ws.shape) and guard_untouched(bbuf, db.shape)
    assert not bool((dw == SENTINEL).any()) and bool((db == SENTINEL).any()) != bias
    if prev is None:
        dw2, db2 = ops.conv_s1_wgrad(D(g), D(x), (kh, kw), bias=bias)
        assert same_bits(dw, dw2) and (not bias or same_bits(db, db2)), 'two runs differ'
    return dw.cpu(), db.cpu()


def _check(tag, g, w, x, add=None, a=None, act=NONE, **kw):
    kh, kw_ = w.shape[2:]
    rd = worst_ratio(_dgrad(g, w, add, a, act, **kw), *HH.dgrad_ref(g, 0.0, w, add, 0.0, a, act))
    dw, db = _wgrad(g, x, kh, kw_, slices=kw.get('slices', False))
    ref, bw, rb, bb = HH.wgrad_ref(g, 0.0, x, kh, kw_)
    rw, rbias = worst_ratio(dw, ref, bw), worst_ratio(db, rb, bb)
    measured(f'conv_s1 dgrad {tag}, error / bound', rd)
    measured(f'conv_s1 wgrad {tag}, error / bound', rw)
    measured(f'conv_s1 bias grad {tag}, error / bound', rbias)
    assert rd <= 1.0 and rw <= 1.0 and rbias <= 1.0


@pytest.mark.parametrize('case', HH.CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_dgrad_wgrad_shapes(case):
    g, w, x, _, _, _ = HH.conv_case('nominal', *case)
    _check(case, g, w, x)


@pytest.mark.parametrize('name', sorted(HH.LAYERS))
def test_the_seven_layers(name):
    case, act = HH.LAYERS[name]
    g, w, x, add, a, _ = HH.conv_case('nominal', *case)
    _check(name, g, w, x, add, a if act != NONE else None, act, scratch=HH.wide(*case[1:3]))


ACT_CASES = [(3, 64, 128, 3, 3, 5, 7), (33, 2, 33, 5, 1, 9, 4), (2, 32, 32, 1, 5, 8, 8), (3, 1, 64, 1, 1, 2, 3)]


@pytest.mark.parametrize('act', HH.ACTS, ids=['none', 'relu', 'sigmoid', 'tanh'])
@pytest.mark.parametrize('with_add', [False, True], ids=['plain', 'add'])
def test_every_act_with_and_without_add_on_channel_slices(act, with_add):
    for case in ACT_CASES:
        g, w, x, add, a, _ = HH.conv_case('nominal', *case)
        _check(f'{case} act {act} add {with_add}', g, w, x, add if with_add else None, a if act != NONE else None, act,
               slices=True, scratch=HH.wide(*case[1:3]))
        n = a.numel() // a.shape[0]
        gwide, gv = sliced(add)
        awide, av = sliced(a)
        owide, ov = sliced(torch.zeros_like(add))
        out = ops.act_grad(gv, av if act != NONE else None, act, out=ov)
        assert slice_untouched(owide, add.shape[1]) and same_bits(out, ops.act_grad(D(add), D(a) if act != NONE else None, act))
        r = worst_ratio(cpu(out), *HH.act_grad_ref(add, 0.0, a, act))
        measured(f'act_grad {case} act {act}, error / bound', r)
        assert r <= 1.0 and n > 0


@pytest.mark.parametrize('regime', HH.REGIMES[1:])
def test_dgrad_wgrad_regimes(regime):
    for case in HH.REGIME_CASES:
        kh, kw = case[3:5]
        g, w, x, add, a, scale = HH.conv_case(regime, *case)
        _check(f'{regime} {case}', g, w, x, add, a, TANH, check_rows=False)
        if regime == 'scaled':              # powers of two on the operands: the same bits, scaled
            g1, w1, x1, add1, a1, _ = HH.conv_case('nominal', *case)
            assert same_bits(_dgrad(g, w, add, a, TANH, check_rows=False), _dgrad(g1, w1, add1, a1, TANH, check_rows=False) * scale)
            (dw, db), (dw1, db1) = _wgrad(g, x, kh, kw), _wgrad(g1, x1, kh, kw)
            assert same_bits(dw, dw1 * scale) and same_bits(db, db1 * 2.0 ** HH.SCALES[0])


def test_wgrad_accumulate_is_previous_plus_sum():
    for case in ((3, 64, 128, 3, 3, 5, 7), (33, 33, 2, 3, 3, 8, 8), (33, 32, 32, 1, 5, 8, 8)):
        kh, kw = case[3:5]
        g, w, x, _, _, _ = HH.conv_case('nominal', *case)
        gen = torch.Generator().manual_seed(1)
        prev, prev_b = torch.randn(w.shape, generator=gen), torch.randn(w.shape[0], generator=gen)
        dw, db = _wgrad(g, x, kh, kw, prev, prev_b)
        ref, bw, rb, bb = HH.wgrad_ref(g, 0.0, x, kh, kw, prev=prev, prev_b=prev_b)
        r = max(worst_ratio(dw, ref, bw), worst_ratio(db, rb, bb))
        measured(f'conv_s1 wgrad accumulate {case}, error / bound', r)
        assert r <= 1.0
        dw0, db0 = _wgrad(g, x, kh, kw)
        assert same_bits(dw, dw0 + prev) and same_bits(db, db0 + prev_b)
        dwn, dbn = _wgrad(g, x, kh, kw, bias=False)
        assert same_bits(dwn, dw0) and dbn is not None


def test_adjoint_identities_against_the_forward_kernel():
    """<conv2d(x), g> = <x, dgrad(g)> = <w, wgrad(g, x)> with the project's own forward, inside the summed bounds: the
    forward's is gamma_d sum |x| |w| for any order of its KH KW Cin products (d = KH KW Cin + 8: up to 8 K-slices added
    after)"""
    worst = 0.0
    for case in ((3, 64, 128, 3, 3, 5, 7), (2, 32, 32, 1, 5, 8, 8), (3, 2, 33, 3, 3, 9, 4), (2, 33, 2, 7, 7, 8, 8), (2, 1, 64, 1, 1, 5, 7)):
        m, cout, cin, kh, kw, h, wd = case
        g, w, x, _, _, _ = HH.conv_case('nominal', *case)
        pc = ops.PackedConv.from_weight(D(w), None, stride=1, padding=(kh // 2, kw // 2))
        y = ops.conv2d(pc, D(x)).cpu()
        assert y.shape == g.shape
        gx = _dgrad(g, w, check_rows=False)
        dw, _ = _wgrad(g, x, kh, kw)
        _, bx = HH.dgrad_ref(g, 0.0, w)
        _, bw, _, _ = HH.wgrad_ref(g, 0.0, x, kh, kw)
        by = gamma(kh * kw * cin + 8) * HH.dgrad_sum(np.abs(f64(x)), np.abs(f64(w)).transpose(1, 0, 2, 3)[:, :, ::-1, ::-1])
        a, b, c = (f64(y) * f64(g)).sum(), (f64(x) * f64(gx)).sum(), (f64(w) * f64(dw)).sum()
        ea, eb, ec = (np.abs(f64(g)) * by).sum(), (np.abs(f64(x)) * bx).sum(), (np.abs(f64(w)) * bw).sum()
        worst = max(worst, abs(a - b) / (ea + eb), abs(a - c) / (ea + ec), abs(b - c) / (eb + ec))
    measured('conv_s1 adjoint identities, difference / summed bounds', worst)
    assert worst <= 1.0


@pytest.mark.parametrize('case', [(3, 33, 40, 3, 3, 8, 8), (3, 31, 33, 7, 7, 8, 8), (3, 64, 32, 1, 5, 8, 8)], ids=['wide', 'thin', 'wide1x5'])
def test_zero_cotangents_and_nan_containment(case):
    m, cout, cin, kh, kw, h, wd = case
    g, w, x, add, a, _ = HH.conv_case('nominal', *case)
    zero = torch.zeros_like(g)
    dwz, dbz = _wgrad(zero, x, kh, kw)
    assert bool((_dgrad(zero, w) == 0).all()) and bool((dwz == 0).all()) and bool((dbz == 0).all())
    m0, co0, y0, x0 = 1, 7, 2, 3
    gn = g.clone()
    gn[m0, co0, y0, x0] = float('nan')
    gx = _dgrad(gn, w)
    dw, db = _wgrad(gn, x, kh, kw)
    allowed = torch.zeros(gx.shape, dtype=torch.bool)
    allowed[m0, :, max(y0 - kh // 2, 0):y0 + kh // 2 + 1, max(x0 - kw // 2, 0):x0 + kw // 2 + 1] = True
    assert bool(torch.isnan(gx)[allowed].all()) and not bool(torch.isnan(gx)[~allowed].any())
    others = torch.arange(cout) != co0
    inside = torch.tensor([[0 <= y0 - kh // 2 + ky < h and 0 <= x0 - kw // 2 + kx < wd for kx in range(kw)] for ky in range(kh)])
    assert bool(torch.isnan(dw[co0])[:, inside].all()) and not bool(torch.isnan(dw[others]).any())     # a tap outside the map may skip it
    assert bool(torch.isnan(db[co0])) and not bool(torch.isnan(db[others]).any())
    assert same_bits(gx[~allowed], _dgrad(g, w)[~allowed])


def test_c_abi_rejections():
    lib, st = _lib.load(), ops._stream()
    t = torch.zeros((8192,), device=DEV)
    p = t.data_ptr()
    dg = lambda *a: lib.scf_conv_s1_dgrad(*a)               # noqa: E731
    wg = lambda *a: lib.scf_conv_s1_wgrad(*a)               # noqa: E731
    ag = lambda *a: lib.scf_act_grad(*a)                    # noqa: E731
    # g, g_stride, w, add, add_stride, a, a_stride, act, gx, gx_stride, w_scratch, M, Cout, Cin, H, W, KH, KW
    ok = dict(g=p, gs=32, w=p, add=None, adds=0, a=None, as_=0, act=NONE, gx=p, gxs=48, sc=None, M=1, Cout=2, Cin=3, H=4, W=4, KH=3, KW=3)
    call = lambda **k: dg(*{**ok, **k}.values(), st)        # noqa: E731
    assert call(g=None) == EINVAL and call(w=None) == EINVAL and call(gx=None) == EINVAL
    assert call(KH=2) == EUNSUPPORTED and call(KW=4) == EUNSUPPORTED and call(KH=9) == EUNSUPPORTED and call(KW=9) == EUNSUPPORTED
    assert call(act=4) == EINVAL and call(act=-1) == EINVAL
    assert call(act=RELU) == EINVAL and call(act=SIGMOID, a=None, as_=48) == EINVAL        # act without a
    assert call(M=0) == EINVAL and call(Cout=0) == EINVAL and call(Cin=-1) == EINVAL and call(H=0) == EINVAL and call(W=0) == EINVAL
    assert call(KH=0) == EINVAL and call(KW=-3) == EINVAL
    assert call(gs=31) == EINVAL and call(gxs=47) == EINVAL
    assert call(add=p, adds=47) == EINVAL and call(a=p, as_=47, act=TANH) == EINVAL
    # g, g_stride, x, x_stride, dW, db, accumulate, workspace, floats, M, Cout, Cin, H, W, KH, KW
    need = lib.scf_conv_s1_wgrad_workspace(1, 2, 3, 4, 4, 3, 3)
    assert need == 9 * 2 * 3 + 2
    okw = dict(g=p, gs=32, x=p, xs=48, dW=p, db=p, acc=0, ws=p, n=need, M=1, Cout=2, Cin=3, H=4, W=4, KH=3, KW=3)
    callw = lambda **k: wg(*{**okw, **k}.values(), st)      # noqa: E731
    assert callw(g=None) == EINVAL and callw(x=None) == EINVAL and callw(dW=None) == EINVAL and callw(ws=None) == EINVAL
    assert callw(n=need - 1) == EINVAL                                                   # a short workspace
    assert callw(KH=2) == EUNSUPPORTED and callw(KW=9) == EUNSUPPORTED
    assert callw(M=0) == EINVAL and callw(Cin=0) == EINVAL and callw(H=-1) == EINVAL and callw(KW=0) == EINVAL
    assert callw(gs=31) == EINVAL and callw(xs=47) == EINVAL
    # g, g_stride, a, a_stride, act, out, out_stride, M, n
    assert ag(None, 8, p, 8, RELU, p, 8, 2, 8, st) == EINVAL and ag(p, 8, p, 8, RELU, None, 8, 2, 8, st) == EINVAL
    assert ag(p, 8, None, 8, RELU, p, 8, 2, 8, st) == EINVAL and ag(p, 8, p, 8, 7, p, 8, 2, 8, st) == EINVAL
    assert ag(p, 7, p, 8, RELU, p, 8, 2, 8, st) == EINVAL and ag(p, 8, p, 7, RELU, p, 8, 2, 8, st) == EINVAL
    assert ag(p, 8, p, 8, RELU, p, 7, 2, 8, st) == EINVAL and ag(p, 8, p, 8, RELU, p, 8, 0, 8, st) == EINVAL
    assert ag(p, 8, p, 8, RELU, p, 8, 2, 0, st) == EINVAL
    torch.cuda.synchronize()
    assert bool((t == 0).all())                             # nothing was launched or written
    g = torch.zeros((2, 4, 5, 6), device=DEV)
    w = torch.zeros((4, 3, 3, 3), device=DEV)
    x = torch.zeros((2, 3, 5, 6), device=DEV)
    bad = [lambda: ops.conv_s1_dgrad(g, w[:3].contiguous()), lambda: ops.conv_s1_dgrad(g, torch.zeros((4, 3, 2, 3), device=DEV)),
           lambda: ops.conv_s1_dgrad(g, w, out=torch.zeros((2, 3, 5, 5), device=DEV)), lambda: ops.conv_s1_dgrad(g.double(), w),
           lambda: ops.conv_s1_dgrad(g.cpu(), w), lambda: ops.conv_s1_dgrad(g[:, :, :, :3], w),
           lambda: ops.conv_s1_dgrad(g, w, act=RELU), lambda: ops.conv_s1_dgrad(g, w, a=x), lambda: ops.conv_s1_dgrad(g, w, act=9, a=x),
           lambda: ops.conv_s1_dgrad(g, w, add=x[:1]), lambda: ops.conv_s1_dgrad(g, w, w_scratch=torch.zeros((10,), device=DEV)),
           lambda: ops.conv_s1_dgrad(g, w.transpose(0, 1)),
           lambda: ops.conv_s1_wgrad(g, x[:1], 3), lambda: ops.conv_s1_wgrad(g, x[:, :, :4].contiguous(), 3),
           lambda: ops.conv_s1_wgrad(g, x, 4), lambda: ops.conv_s1_wgrad(g, x, (3, 9)),
           lambda: ops.conv_s1_wgrad(g, x, 3, workspace=torch.zeros((9 * 4 * 3,), device=DEV)),
           lambda: ops.conv_s1_wgrad(g, x, 3, dw=torch.zeros((4, 3, 3), device=DEV)),
           lambda: ops.conv_s1_wgrad(g, x, 3, db=torch.zeros((3,), device=DEV)), lambda: ops.conv_s1_wgrad(g, x, 3, accumulate=True),
           lambda: ops.conv_s1_wgrad(g.view(2, 4, 30), x, 3), lambda: ops.conv_s1_wgrad_workspace(1, 1, 1, 1, 1, 2, 2),
           lambda: ops.act_grad(g, None, RELU), lambda: ops.act_grad(g, g, NONE), lambda: ops.act_grad(g, x, RELU),
           lambda: ops.act_grad(g, g, 5), lambda: ops.act_grad(g, g, RELU, out=x)]
    for i, f in enumerate(bad):
        with pytest.raises(ScflowHipError):
            f()
            pytest.fail(f'call {i} was accepted')


# ===================================================================================================== heads_backward
def _decoder(act_cfg=dict(type='ReLU'), seed=5):
    from scflow_amd.registry import DECODERS, build_from_cfg
    cfg = dict(scflow_amd.scflow_model_cfg()['decoder'], act_cfg=act_cfg)
    dec = build_from_cfg(cfg, DECODERS)
    g = torch.Generator().manual_seed(seed)
    for name, prm in dec.named_parameters():
        if name.split('.')[0] in ('flow_pred', 'mask_pred', 'delta_flow_encoder', 'mask_encoder'):
            fan = prm[0].numel() if prm.dim() > 1 else 1
            prm.data.copy_(torch.randn(prm.shape, generator=g) * (fan ** -0.5 if prm.dim() > 1 else 0.1))
    return dec.to(DEV)


def _saved_of(dec, hvs):
    """what a decoder at keep level 'decoder_heads' keeps, built from the forward's own launches -> (saved, activations)"""
    keep = {k: [] for k in ('hv', 'heads', 'd_flow', 'mask', 'd1', 'm1', 'dm')}
    for hv in hvs:
        n, _, h, w = hv.shape
        heads = ops.conv2d(dec.packed, hv, act=RELU)
        d_flow = dec.flow_pred.predict(heads[:, :256])
        mask = dec.mask_pred.predict(heads[:, 256:], act=SIGMOID)
        dm = torch.empty((n, 96, h, w), device=DEV)
        d1, m1 = dec.delta_flow_encoder[0](d_flow), dec.mask_encoder[0](mask)
        dec.delta_flow_encoder[1](d1, out=dm[:, :64])
        dec.mask_encoder[1](m1, out=dm[:, 64:])
        for k, v in zip(keep, (hv, heads, d_flow, mask, d1, m1, dm)):
            keep[k].append(v)
    acts = {k: torch.stack(v).contiguous() for k, v in keep.items()}
    return {k: acts[k] for k in ('hv', 'dm', 'd_flow', 'mask')}, acts


def _stage_check(dec, acts, cots, got, prev=None):
    """worst error / composed bound per result against the float64 stage GIVEN the kernels' own activations"""
    flat = lambda t: cpu(t).reshape(-1, *t.shape[2:])               # noqa: E731
    p = {k: cpu(v) for k, v in dec.named_parameters() if k in HH.HEAD_NAMES}
    enc_act = dec.delta_flow_encoder[0].act
    stack = lambda seq: torch.cat([cpu(t) for t in seq])            # noqa: E731
    ref, bnd = HH.heads_ref64({k: flat(v) for k, v in acts.items()}, p, *(f64(stack(c)) for c in cots), enc_act, prev=prev,
                              bounds=True)
    g_h, g_df, g_ml, grads = got
    have = dict(g_hidden=stack(g_h), g_delta_flow_total=stack(g_df), g_mask_logit=stack(g_ml), **{k: cpu(grads[k]) for k in HH.HEAD_NAMES})
    return {k: worst_ratio(have[k], ref[k], bnd[k]) for k in ref}


@pytest.mark.parametrize('act_cfg', [dict(type='ReLU'), None], ids=['relu', 'noact'])
@pytest.mark.parametrize('T', [1, 3])
@pytest.mark.parametrize('feat_size', [(8, 8), (5, 7), (12, 20)], ids=lambda v: f'{v[0]}x{v[1]}')
def test_heads_backward_against_float64_given_the_activations(feat_size, T, act_cfg):
    dec = _decoder(act_cfg)
    gen = torch.Generator().manual_seed(600 + T)
    n = 2
    hvs = [D(torch.tanh(torch.randn((n, 128, *feat_size), generator=gen))) for _ in range(T)]
    cots = [[D(torch.randn((n, c, *feat_size), generator=gen)) for _ in range(T)] for c in (128, 96, 2, 1)]
    saved, acts = _saved_of(dec, hvs)
    # the forward's own launches on the saved tensors reproduce the kept ones: the recomputation has the forward's bits
    for t in range(T):
        heads = ops.conv2d(dec.packed, saved['hv'][t], act=RELU)
        assert same_bits(heads, acts['heads'][t])
        assert same_bits(dec.flow_pred.predict(heads[:, :256]), saved['d_flow'][t])
        assert same_bits(dec.mask_pred.predict(heads[:, 256:], act=SIGMOID), saved['mask'][t])
        d1, m1 = dec.delta_flow_encoder[0](saved['d_flow'][t]), dec.mask_encoder[0](saved['mask'][t])
        assert same_bits(d1, acts['d1'][t]) and same_bits(m1, acts['m1'][t])
        assert same_bits(dec.delta_flow_encoder[1](d1), saved['dm'][t][:, :64]) and same_bits(dec.mask_encoder[1](m1), saved['dm'][t][:, 64:])
    got = dec.heads_backward(saved, *cots)
    assert sorted(got[3]) == sorted(HH.HEAD_NAMES)
    assert all(g.shape == (n, c, *feat_size) for seq, c in zip(got[:3], (128, 2, 1)) for g in seq) and all(len(s) == T for s in got[:3])
    again = dec.heads_backward(saved, *cots)
    assert all(same_bits(a, b) for x, y in zip(got[:3], again[:3]) for a, b in zip(x, y))
    assert all(same_bits(got[3][k], again[3][k]) for k in HH.HEAD_NAMES)
    for key, v in _stage_check(dec, acts, cots, got).items():
        measured(f'heads_backward {feat_size} T {T} act {act_cfg} {key}, error / composed bound', v)
        assert v <= 1.0, key
    # accumulating into a dict passed in: previous + sum, the previous value added last
    prev = {k: D(torch.randn(v.shape, generator=gen)) for k, v in got[3].items()}
    into = {k: v.clone() for k, v in prev.items()}
    into['other'] = prev['mask_encoder.1.conv.bias']
    acc = dec.heads_backward(saved, *cots, param_grads=into)
    assert acc[3] is into and set(into) == set(HH.HEAD_NAMES) | {'other'}
    assert all(same_bits(into[k], got[3][k] + prev[k]) for k in HH.HEAD_NAMES)
    for key, v in _stage_check(dec, acts, cots, acc, prev={k: cpu(v) for k, v in prev.items()}).items():
        assert v <= 1.0, key
    if T == 3:
        with pytest.raises(ScflowHipError):
            dec.heads_backward(saved, *cots, param_grads={HH.HEAD_NAMES[0]: prev[HH.HEAD_NAMES[0]]})
        with pytest.raises(ScflowHipError):
            dec.heads_backward(saved, cots[0], cots[1], cots[2], cots[3][:2])
        with pytest.raises(ScflowHipError):
            dec.heads_backward({k: v for k, v in saved.items() if k != 'mask'}, *cots)


def test_other_encoder_activations_raise():
    dec = _decoder()
    dec.mask_encoder[1].act = TANH
    z = lambda c: [torch.zeros((1, c, 4, 4), device=DEV)]           # noqa: E731
    saved = dict(hv=z(128)[0][None], dm=z(96)[0][None], d_flow=z(2)[0][None], mask=z(1)[0][None])
    with pytest.raises(NotImplementedError):
        dec.heads_backward(saved, z(128), z(96), z(2), z(1))


# ================================================================================================= the refiner's entry
@pytest.fixture(scope='module')
def scflow_model(golden_dir):
    """the small random-weight refiner of tests/test_gpu_tail_grad.py (64 x 64, two iterations)"""
    case = HL.refiner_loss_case()
    cfg = scflow_amd.scflow_model_cfg(iters=HL.REFINER_ITERS)
    cfg.update(HL.refiner_loss_cfgs(case))
    cfg['pose_loss_cfg'] = dict(type='SequenceLoss', gamma=0.7, loss_func_cfg=dict(type='RAFTLoss', loss_weight=0.3, max_flow=400.))
    m = scflow_amd.build_refiner(cfg)
    shapes = json.load(open(os.path.join(golden_dir, 'state_dict_keys.json')))['shapes']
    m.load_state_dict(scflow_amd.fill_state_dict(shapes, seed=0), strict=True)
    return m.to(DEV), case


def test_loss_and_decoder_head_grads(scflow_model):
    m, case = scflow_model
    data = HL.refiner_data(case, DEV)
    plain = m.loss(None, data=data)
    base = m.loss_and_pose_head_grads(None, data=data)
    loss, log_imgs, log_vars, seq_r, seq_t, grads = m.loss_and_decoder_head_grads(None, data=data)
    assert same_bits(loss, plain[0]) and list(log_vars.items()) == list(plain[2].items()) and log_imgs is None
    assert sorted(grads) == sorted(list(base[5]) + ['decoder_heads'])
    for key, seq in base[5].items():
        if key == 'params':
            assert all(same_bits(grads['params'][k], v) for k, v in seq.items()), key
        elif key == 'pose_head_inputs':
            assert all(same_bits(a, b) for x, y in zip(grads[key], seq) for a, b in zip(x, y)), key
        else:
            assert all(same_bits(a, b) for a, b in zip(grads[key], seq)), key
    dec = m.decoder
    assert dec.keep == 'none'
    head_names = {'decoder.pose_pred.' + k for k in dict(dec.pose_pred.named_parameters())}
    assert set(grads['params']) == head_names | {'decoder.' + k for k in HH.HEAD_NAMES}
    dh = grads['decoder_heads']
    assert sorted(dh) == ['delta_flow_preds', 'hidden_states', 'mask_logits'] and all(len(v) == dec.iters for v in dh.values())
    saved = dec.kept
    assert sorted(saved) == ['d_flow', 'dm', 'hv', 'mask', 'tail_inputs', 'y0', 'y1', 'y2']
    _, acts = _saved_of(dec, list(saved['hv']))
    assert all(same_bits(acts[k], saved[k]) for k in ('dm', 'd_flow', 'mask')), 'the kept tensors are the forward\'s own'
    g_hvs, g_dms = grads['pose_head_inputs']
    got = (dh['hidden_states'], dh['delta_flow_preds'], dh['mask_logits'], {k: grads['params']['decoder.' + k] for k in HH.HEAD_NAMES})
    for key, v in _stage_check(dec, acts, (g_hvs, g_dms, grads['delta_flow_preds'], grads['masks']), got).items():
        measured(f'loss_and_decoder_head_grads {key}, error / composed bound', v)
        assert v <= 1.0, key
    with pytest.raises(NotImplementedError, match='loss_and_decoder_head_grads'):
        m.forward(data, return_loss=True)


def test_keeping_the_head_inputs_changes_no_bit(scflow_model):
    m, case = scflow_model
    data = HL.refiner_data(case, DEV)
    dec = m.decoder
    get = lambda: m.get_pose(data['rendered_images'], data['real_images'], data['ref_rotations'], data['ref_translations'],   # noqa: E731
                             data['rendered_depths'], data['internel_k'], data['labels'])
    old = dec.c_iteration
    kept = {}
    try:
        for c_iteration in (True, False):
            dec.c_iteration = c_iteration
            dec.kept = {}
            off = get()
            assert dec.kept == {}
            dec.keep = 'decoder_heads'
            on = get()
            dec.keep = 'none'
            assert sorted(dec.kept) == ['d_flow', 'dm', 'hv', 'mask', 'tail_inputs', 'y0', 'y1', 'y2']
            kept[c_iteration] = ({k: v.clone() for k, v in dec.kept.items() if k != 'tail_inputs'},
                                 [t.clone() for t in dec.kept['tail_inputs']])
            for a, b in zip(off, on):
                assert all(same_bits(x, y) for x, y in zip(a, b)), f'c_iteration {c_iteration}'
    finally:
        dec.keep, dec.c_iteration = 'none', old
    (sc, tc), (sp, tp) = kept[True], kept[False]
    assert sorted(sc) == sorted(sp) == ['d_flow', 'dm', 'hv', 'mask', 'y0', 'y1', 'y2'] and len(tc) == len(tp) == dec.iters
    n, (h, w) = sc['hv'].shape[1], sc['hv'].shape[3:]
    assert sc['d_flow'].shape == (dec.iters, n, 2, h, w) and sc['mask'].shape == (dec.iters, n, 1, h, w)
    assert all(same_bits(sc[k], sp[k]) for k in sc), 'the two loop forms keep different tensors'
    assert all(same_bits(a, b) for a, b in zip(tc, tp))
    _, acts = _saved_of(dec, list(sc['hv']))
    assert all(same_bits(acts[k], sc[k]) for k in ('dm', 'd_flow', 'mask'))


# ===================================================================== the reference's own heads and encoders (fixture)
@pytest.mark.parametrize('hw', HH.GOLDEN_MAPS, ids=lambda v: f'{v[0]}x{v[1]}')
def test_kernels_against_the_reference_fixture(hw):
    """heads_backward on the fixture's seeds against the reference's recorded autograd.  Both are fp32 evaluations around
    the float64 backward of tests/test_head_grad_host.py::golden_reference, each inside its room, so they are at most two
    rooms apart; the kernels' own, tighter bounds are held by the tests above."""
    z = np.load(HH.GOLDEN)
    tag, p, h, cots = HH.golden_case(hw)
    dec = _decoder()
    with torch.no_grad():
        for name, prm in dec.named_parameters():
            if name in p:
                prm.copy_(p[name])
    dec.invalidate_packed()
    saved, _ = _saved_of(dec, [D(h)])
    g_h, g_df, g_ml, grads = dec.heads_backward(saved, *([D(c)] for c in cots))
    got = dict(g_hidden=cpu(g_h[0]), g_delta_flow_total=cpu(g_df[0]), g_mask_logit=cpu(g_ml[0]), **{k: cpu(grads[k]) for k in HH.HEAD_NAMES})
    _, ref, room = HH.golden_reference(hw)
    for key in HH.GOLDEN_KEYS:
        v = worst_ratio(HH.golden_pick(key, got[key].numpy()), z[f'{tag}.{key}'], 2.0 * HH.golden_pick(key, room[key]))
        measured(f'kernels - reference fixture {tag} {key}, difference / two rooms', v)
        assert v <= 1.0, key
        fixture = z[f'{tag}.{key}']
        measured(f'kernels - reference fixture {tag} {key}, relative to the largest entry',
                 float(np.abs(HH.golden_pick(key, got[key].numpy()) - fixture).max() / np.abs(fixture).max()))
