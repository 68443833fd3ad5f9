"""GPU: conv_grad.hip (scf_conv_dgrad, scf_conv_wgrad, scf_conv_wgrad_workspace), MultiClassPoseHead.conv_backward,
SCFlowDecoder.keep = 'pose_head' and SCFlowRefiner.loss_and_pose_head_grads against the float64 restatements and the
derived bounds of tests/test_conv_grad_host.py.  Every comparison is `error <= bound` over ALL elements (ratio <= 1) or bit
equality; there is no absolute tolerance.  The measured ratios are recorded in DESIGN.md section 4.8."""
import json
import os

import numpy as np
import pytest
import torch

import scflow_amd
from scflow_amd import _lib, ops
from scflow_amd._lib import ScflowHipError
import test_conv_grad_host as HC
import test_fc_grad_host as HF
import test_loss_host as HL
from test_fc_host import ACT_RELU, fc_depth, fc_gn_ref, fc_operand, gamma, gemm_ref, linear_ref_core, parts_ref  # noqa: E402
from test_stream_ops_host import f64, group_norm_relu_ref, measured, same_bits, worst_ratio  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = -7777.25
GUARD = 64
EINVAL, EUNSUPPORTED = -1, -2       # include/scflow_hip.h


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


# ====================================================================================================== dgrad, wgrad
def _dgrad(g, w, c0, c1, hin, win, check_rows=True):
    """-> (M, C0 + C1, Hin, Win) on the CPU; guard bands, two runs, and the rows 0, 16, 32 of a 33-sample run as M = 1 runs"""
    m = g.shape[0]
    bufs = [guarded((m, c0, hin, win))] + ([guarded((m, c1, hin, win))] if c1 else [])
    outs = [b[1] for b in bufs]
    got = ops.conv_dgrad(D(g), D(w), (hin, win), split=c0 if c1 else None, out=tuple(outs) if c1 else outs[0])
    got = (got,) if not c1 else got
    assert all(guard_untouched(b, o.shape) and not bool((o == SENTINEL).any()) for (b, _), o in zip(bufs, outs))
    again = ops.conv_dgrad(D(g), D(w), (hin, win), split=c0 if c1 else None)
    again = (again,) if not c1 else again
    assert all(same_bits(a, b) for a, b in zip(got, again)), 'two runs differ'
    full = torch.cat([t.cpu() for t in got], 1)
    if check_rows and m == 33:
        for r in (0, 16, 32):
            one = ops.conv_dgrad(D(g[r:r + 1]), D(w), (hin, win))
            assert same_bits(full[r:r + 1], one), 'a sample depends on its batch'
    return full


def _wgrad(g, x, c0, c1, prev=None):
    m, cout, ho, wo = g.shape
    cin = c0 + c1
    need = ops.conv_wgrad_workspace(m, cout, cin, ho, wo)
    wbuf, dw = guarded((cout, cin, 3, 3))
    sbuf, ws = guarded((need,))
    if prev is not None:
        dw.copy_(prev)
    x0, x1 = D(x[:, :c0]), (D(x[:, c0:]) if c1 else None)
    ops.conv_wgrad(D(g), x0, x1, dw=dw, accumulate=prev is not None, workspace=ws)
    assert guard_untouched(wbuf, dw.shape) and guard_untouched(sbuf, ws.shape) and not bool((dw == SENTINEL).any())
    if prev is None:
        assert same_bits(dw, ops.conv_wgrad(D(g), x0, x1)), 'two runs differ'
    return dw.cpu()


@pytest.mark.parametrize('case', HC.CASES + [HC.LAYER0], ids=lambda c: 'x'.join(map(str, c)))
def test_dgrad_wgrad_tiles(case):
    m, cout, c0, c1, hin, win = case
    g, w, x, _ = HC.conv_case('nominal', *case)
    rd = worst_ratio(_dgrad(g, w, c0, c1, hin, win), *HC.dgrad_ref(g, 0.0, w, hin, win))
    rw = worst_ratio(_wgrad(g, x, c0, c1), *HC.wgrad_ref(g, 0.0, x))
    measured(f'conv dgrad {case}, error / bound', rd)
    measured(f'conv wgrad {case}, error / bound', rw)
    assert rd <= 1.0 and rw <= 1.0


@pytest.mark.parametrize('regime', HC.REGIMES[1:])
def test_dgrad_wgrad_regimes(regime):
    for case in HC.REGIME_CASES:
        m, cout, c0, c1, hin, win = case
        g, w, x, scale = HC.conv_case(regime, *case)
        gx, dw = _dgrad(g, w, c0, c1, hin, win, check_rows=False), _wgrad(g, x, c0, c1)
        rd = worst_ratio(gx, *HC.dgrad_ref(g, 0.0, w, hin, win))
        rw = worst_ratio(dw, *HC.wgrad_ref(g, 0.0, x))
        measured(f'conv dgrad {regime} {case}, error / bound', rd)
        measured(f'conv wgrad {regime} {case}, error / bound', rw)
        assert rd <= 1.0 and rw <= 1.0
        if regime == 'scaled':              # powers of two on the operands: the same bits, scaled
            g1, w1, x1, _ = HC.conv_case('nominal', *case)
            assert same_bits(gx, _dgrad(g1, w1, c0, c1, hin, win, check_rows=False) * scale)
            assert same_bits(dw, _wgrad(g1, x1, c0, c1) * scale)


def test_wgrad_accumulate_is_previous_plus_sum():
    for case in (HC.CASES[12], HC.CASES[8]):
        m, cout, c0, c1, hin, win = case
        g, w, x, _ = HC.conv_case('nominal', *case)
        prev = torch.randn(w.shape, generator=torch.Generator().manual_seed(1))
        dw = _wgrad(g, x, c0, c1, prev)
        r = worst_ratio(dw, *HC.wgrad_ref(g, 0.0, x, prev=prev))
        measured(f'conv wgrad accumulate {case}, error / bound', r)
        assert r <= 1.0
        assert same_bits(dw, _wgrad(g, x, c0, c1) + prev)


def test_adjoint_identities_against_the_forward_kernel():
    """<conv2d(x), g> = <x, dgrad(g)> = <w, wgrad(g, x)> with the project's own forward, inside the summed bounds: the
    forward's is gamma_d sum |x| |w| for any order of its 9 Cin products (d = 9 Cin + 8: up to 8 K-slices added after)"""
    worst = 0.0
    for case in (HC.CASES[6], HC.CASES[8], HC.CASES[12], HC.CASES[3], HC.LAYER0):
        m, cout, c0, c1, hin, win = case
        g, w, x, _ = HC.conv_case('nominal', *case)
        pc = ops.PackedConv.from_weight(D(w), None, stride=2, padding=1)
        y = ops.conv2d(pc, D(x[:, :c0]), D(x[:, c0:]) if c1 else None).cpu()
        assert y.shape == g.shape
        gx, dw = _dgrad(g, w, c0, c1, hin, win, check_rows=False), _wgrad(g, x, c0, c1)
        _, bx = HC.dgrad_ref(g, 0.0, w, hin, win)
        _, bw = HC.wgrad_ref(g, 0.0, x)
        by = gamma(9 * (c0 + c1) + 8) * HC.conv_fwd64(np.abs(f64(x)), np.abs(f64(w)))
        a, b, c = (f64(y) * f64(g)).sum(), (f64(x) * f64(gx)).sum(), (f64(w) * f64(dw)).sum()
        ea, eb, ec = (np.abs(f64(g)) * by).sum(), (np.abs(f64(x)) * bx).sum(), (np.abs(f64(w)) * bw).sum()
        worst = max(worst, abs(a - b) / (ea + eb), abs(a - c) / (ea + ec), abs(b - c) / (eb + ec))
    measured('conv adjoint identities, difference / summed bounds', worst)
    assert worst <= 1.0


def test_zero_cotangents_and_nan_containment():
    case = HC.CASES[6]                                     # (3, 33, 33, 31, 8, 8)
    m, cout, c0, c1, hin, win = case
    g, w, x, _ = HC.conv_case('nominal', *case)
    zero = torch.zeros_like(g)
    assert bool((_dgrad(zero, w, c0, c1, hin, win) == 0).all()) and bool((_wgrad(zero, x, c0, c1) == 0).all())
    m0, co0, oy0, ox0 = 1, 7, 2, 3
    gn = g.clone()
    gn[m0, co0, oy0, ox0] = float('nan')
    gx, dw = _dgrad(gn, w, c0, c1, hin, win), _wgrad(gn, x, c0, c1)
    allowed = torch.zeros(gx.shape, dtype=torch.bool)
    allowed[m0, :, max(2 * oy0 - 1, 0):2 * oy0 + 2, max(2 * ox0 - 1, 0):2 * ox0 + 2] = True
    assert bool(torch.isnan(gx)[allowed].all()) and not bool(torch.isnan(gx)[~allowed].any())
    assert bool(torch.isnan(dw[co0]).all()) and not bool(torch.isnan(dw[torch.arange(cout) != co0]).any())
    clean = _dgrad(g, w, c0, c1, hin, win)
    assert same_bits(gx[~allowed], clean[~allowed])
    ci0 = 40                                               # in the second part
    xn = x.clone()
    xn[m0, ci0, 3, 4] = float('nan')
    dw = _wgrad(g, xn, c0, c1)
    assert bool(torch.isnan(dw[:, ci0]).any()) and not bool(torch.isnan(dw[:, torch.arange(c0 + c1) != ci0]).any())


def test_c_abi_rejections():
    lib, st = _lib.load(), ops._stream()
    t = torch.zeros((4096,), device=DEV)
    p = t.data_ptr()
    dg = lambda *a: lib.scf_conv_dgrad(*a)                  # noqa: E731
    wg = lambda *a: lib.scf_conv_wgrad(*a)                  # noqa: E731
    # g, w, gx0, C0, gx1, C1, M, Cout, Ho, Wo, Hin, Win, KH, KW, stride, pad
    assert dg(None, p, p, 2, None, 0, 1, 2, 2, 2, 4, 4, 3, 3, 2, 1, st) == EINVAL
    assert dg(p, None, p, 2, None, 0, 1, 2, 2, 2, 4, 4, 3, 3, 2, 1, st) == EINVAL
    assert dg(p, p, None, 2, None, 0, 1, 2, 2, 2, 4, 4, 3, 3, 2, 1, st) == EINVAL
    assert dg(p, p, p, 2, None, 1, 1, 2, 2, 2, 4, 4, 3, 3, 2, 1, st) == EINVAL              # C1 > 0 without gx1
    assert dg(p, p, p, 2, p, 0, 1, 2, 2, 2, 4, 4, 3, 3, 2, 1, st) == EINVAL                 # gx1 with C1 = 0
    assert dg(p, p, p, 2, None, 0, 1, 2, 3, 2, 4, 4, 3, 3, 2, 1, st) == EINVAL              # Ho = 3 for Hin = 4
    assert dg(p, p, p, 2, None, 0, 1, 2, 2, 2, 5, 4, 3, 3, 2, 1, st) == EINVAL              # Ho = 2 for Hin = 5
    assert dg(p, p, p, 2, None, 0, 1, 2, 4, 4, 4, 4, 3, 3, 1, 1, st) == EUNSUPPORTED        # stride 1
    assert dg(p, p, p, 2, None, 0, 1, 2, 2, 2, 4, 4, 5, 5, 2, 1, st) == EUNSUPPORTED        # 5 x 5
    assert dg(p, p, p, 2, None, 0, 1, 2, 2, 2, 4, 4, 3, 3, 2, 0, st) == EUNSUPPORTED        # no padding
    assert dg(p, p, p, 2, None, 0, 0, 2, 2, 2, 4, 4, 3, 3, 2, 1, st) == EINVAL
    # g, x0, C0, x1, C1, dW, accumulate, workspace, floats, M, Cout, Ho, Wo, Hin, Win, KH, KW, stride, pad
    need = lib.scf_conv_wgrad_workspace(1, 2, 2, 2, 2)
    assert need == 9 * 2 * 2
    assert wg(None, p, 2, None, 0, p, 0, p, need, 1, 2, 2, 2, 4, 4, 3, 3, 2, 1, st) == EINVAL
    assert wg(p, None, 2, None, 0, p, 0, p, need, 1, 2, 2, 2, 4, 4, 3, 3, 2, 1, st) == EINVAL
    assert wg(p, p, 2, None, 0, None, 0, p, need, 1, 2, 2, 2, 4, 4, 3, 3, 2, 1, st) == EINVAL
    assert wg(p, p, 2, None, 0, p, 0, None, need, 1, 2, 2, 2, 4, 4, 3, 3, 2, 1, st) == EINVAL
    assert wg(p, p, 2, None, 1, p, 0, p, 2 * need, 1, 2, 2, 2, 4, 4, 3, 3, 2, 1, st) == EINVAL     # C1 > 0 without x1
    assert wg(p, p, 2, None, 0, p, 0, p, need - 1, 1, 2, 2, 2, 4, 4, 3, 3, 2, 1, st) == EINVAL     # a short workspace
    assert wg(p, p, 2, None, 0, p, 0, p, need, 1, 2, 3, 2, 4, 4, 3, 3, 2, 1, st) == EINVAL         # wrong Ho
    assert wg(p, p, 2, None, 0, p, 0, p, need, 1, 2, 4, 4, 4, 4, 3, 3, 1, 1, st) == EUNSUPPORTED   # stride 1
    assert wg(p, p, 2, None, 0, p, 0, p, need, 1, 2, 2, 2, 4, 4, 5, 5, 2, 1, st) == EUNSUPPORTED   # 5 x 5
    torch.cuda.synchronize()
    assert bool((t == 0).all())                             # nothing was launched
    g = torch.zeros((2, 4, 2, 2), device=DEV)
    w = torch.zeros((4, 3, 3, 3), device=DEV)
    x = torch.zeros((2, 3, 4, 4), device=DEV)
    with pytest.raises(ScflowHipError):
        ops.conv_dgrad(g, w, (5, 4))                        # the map of g does not belong to a 5 x 4 input
    with pytest.raises(ScflowHipError):
        ops.conv_dgrad(g, w[:3].contiguous(), (4, 4))       # Cout of the weight
    with pytest.raises(ScflowHipError):
        ops.conv_dgrad(g, w, (4, 4), out=torch.zeros((2, 3, 4, 3), device=DEV))
    with pytest.raises(ScflowHipError):
        ops.conv_dgrad(g, w, (4, 4), split=3)
    with pytest.raises(ScflowHipError):
        ops.conv_dgrad(g.double(), w, (4, 4))
    with pytest.raises(ScflowHipError):
        ops.conv_dgrad(g.cpu(), w, (4, 4))
    with pytest.raises(ScflowHipError):
        ops.conv_dgrad(g[:, :, :, :1], w, (4, 1))           # not contiguous
    with pytest.raises(ScflowHipError):
        ops.conv_dgrad(g, torch.zeros((4, 3, 5, 5), device=DEV), (4, 4))
    with pytest.raises(ScflowHipError):
        ops.conv_wgrad(g, x[:1])                            # samples
    with pytest.raises(ScflowHipError):
        ops.conv_wgrad(g, x, x[:, :, :3].contiguous())      # the second part's map
    with pytest.raises(ScflowHipError):
        ops.conv_wgrad(g, x, workspace=torch.zeros((9 * 4 * 3 - 1,), device=DEV))
    with pytest.raises(ScflowHipError):
        ops.conv_wgrad(g, x, dw=torch.zeros((4, 3, 3), device=DEV))
    with pytest.raises(ScflowHipError):
        ops.conv_wgrad(g, x, accumulate=True)               # nothing to accumulate into
    with pytest.raises(ScflowHipError):
        ops.conv_wgrad(g, x, stride=1)
    with pytest.raises(ScflowHipError):
        ops.conv_wgrad(g.view(2, 4, 4), x)


# ===================================================================================================== conv_backward
FC_SIZE = {(12, 20): (16, 24)}         # 12x20 maps end as 128 x 2 x 3 = 768 features: fc1 is sized by a 16x24 declaration


def _head(feat_size, seed=5):
    """the head's `feat_size` only sizes fc1 (128 * int(int(int(h w / 4) / 4) / 4) features); the maps fed are feat_size"""
    from scflow_amd.registry import HEAD, build_from_cfg
    cfg = dict(scflow_amd.scflow_model_cfg()['decoder']['pose_head_cfg'], feat_size=FC_SIZE.get(feat_size, feat_size))
    head = build_from_cfg(cfg, HEAD)
    g = torch.Generator().manual_seed(seed)
    for prm in head.parameters():
        prm.data.copy_(torch.randn(prm.shape, generator=g) * (0.05 if prm.dim() > 1 else 0.1))
    with torch.no_grad():
        for blk in head.conv_layers:
            blk.gn.weight.add_(1.0)
    return head.to(DEV)


cpu = lambda t: t.detach().cpu()                                    # noqa: E731


def _tail_refs(head, ys, label, g_rots, g_trans, mode):
    """the float64 tail given the kernel's masks and the composed bound of its input gradient, as
    tests/test_gpu_fc_grad.py::_tail_check builds them -> (g_y reference (M, K), its bound)"""
    T, n = len(ys), g_rots[0].shape[0]
    m = T * n
    y5 = [y if y.dim() == 5 else y[None] for y in ys]
    parts = torch.stack([cpu(y) for y in y5], 1).reshape(y5[0].shape[0], m, -1)
    hw = ys[0].shape[-1] * ys[0].shape[-2]
    k = parts.shape[-1]
    last = head.conv_layers[2]
    gsz = k // last.groups
    p32 = {key: cpu(dict(head.named_parameters())[name]) for key, name in HF.TAIL_NAMES.items()}
    p = {key: f64(v) for key, v in p32.items()}
    x0, a1, a2 = (cpu(t) for t in head._tail(D(parts).view(parts.shape[0], m, -1, *ys[0].shape[-2:]), activations=True))
    masks = tuple(f64(t) > 0 for t in (x0, a1, a2))
    ysum = fc_operand(parts)
    cls = HF.clamp_class(cpu(label).numpy(), m, n, head.num_class, mode)
    g_rot, g_tr = torch.cat([cpu(g) for g in g_rots]), torch.cat([cpu(g) for g in g_trans])
    ref = HF.tail_ref64(f64(ysum), p, cls, f64(g_rot), f64(g_tr), gsz, hw, masks)
    s1, s2 = head.fc_plan()
    if s1:
        _, x0b = fc_gn_ref(f64(ysum), gsz, hw, p32['gamma'], p32['beta'])
        r, b = gemm_ref(ref['x0'], x0b, p['W1'], None, fc_depth(k // s1, False), s1)
        _, a1b = parts_ref(r, b, p32['b1'], True)
        r, b = gemm_ref(ref['a1'], a1b, p['W2'], None, fc_depth(ref['a1'].shape[1] // s2, False), s2)
        _, a2b = parts_ref(r, b, p32['b2'], True)
    else:
        _, x0b = group_norm_relu_ref(parts.view(parts.shape[0], m, k // hw, hw), p32['gamma'], p32['beta'], last.groups)
        x0b = x0b.reshape(m, k)
        _, a1b = linear_ref_core(ref['x0'], x0b, p32['W1'], p32['b1'], ACT_RELU)
        _, a2b = linear_ref_core(ref['a1'], a1b, p32['W2'], p32['b2'], ACT_RELU)
    (_, b_s2), _ = HF.select_ref(g_rot, g_tr, p['Wr'], p['Wt'], ref['a2'], a2b, cls, masks[2])
    _, b_s1 = HF.dgrad_ref(ref['g_s2'], b_s2, p['W2'], masks[1])
    _, b_x0 = HF.dgrad_ref(ref['g_s1'], b_s1, p['W1'])
    (_, b_gy), _, _ = HF.gn_grad_ref(f64(ysum), ref['g_x0'], b_x0, masks[0], p32['gamma'], gsz, hw)
    return ref['g_y'], b_gy


def _conv_check(head, saved, g_y2, b_gy2, g_hvs, g_dms, grads):
    """worst error / composed bound of conv_backward's results against the float64 stack given the kernel's masks and raw
    convolution outputs: every stage's bound goes through the next stage's sum of magnitudes; the bounds of the
    recomputed activations (the forward's GroupNorm) enter the weight gradients."""
    hv, dm = cpu(saved['hv']), cpu(saved['dm'])
    T, n = hv.shape[:2]
    m = T * n
    x = torch.cat([hv, dm], 2).reshape(m, -1, *hv.shape[3:])
    groups = head.conv_layers[0].groups
    p32 = {name: cpu(dict(head.named_parameters())[name]) for name in HC.CONV_NAMES}
    p = {k: f64(v) for k, v in p32.items()}
    ysums, masks, abounds = [], [], []
    for i in (0, 1):
        y = cpu(saved[f'y{i}'])
        c, hh, ww = y.shape[3:]
        parts = y.reshape(y.shape[0], m, c, hh * ww)
        ysums.append(f64(fc_operand(parts.reshape(y.shape[0], m, -1))).reshape(m, c, hh, ww))
        blk = head.conv_layers[i]
        a = cpu(ops.group_norm_relu(D(parts.reshape(y.shape[0], m, c, hh, ww)) if y.shape[0] > 1 else D(parts[0].reshape(m, c, hh, ww)),
                                    blk.gn.weight, blk.gn.bias, blk.groups, blk.gn.eps))
        masks.append(f64(a) > 0)
        _, ab = group_norm_relu_ref(parts, p32[f'conv_layers.{i}.gn.weight'], p32[f'conv_layers.{i}.gn.bias'], groups)
        abounds.append(ab.reshape(m, c, hh, ww))
    h2 = (HC.out_size(ysums[1].shape[2]), HC.out_size(ysums[1].shape[3]))
    g_y2 = g_y2.reshape(m, -1, *h2)
    b_gy2 = np.broadcast_to(b_gy2, (m, g_y2.shape[1] * h2[0] * h2[1])).reshape(g_y2.shape)
    ref = HC.conv_stack_ref64(f64(x), ysums, p, g_y2, groups, masks)
    bounds = HC.conv_stack_bounds(ref, f64(x), p, g_y2, b_gy2, groups, abounds)
    worst = {k: worst_ratio(cpu(grads[k]), ref[k], bounds[k]) for k in HC.CONV_NAMES}
    got_x = torch.cat([torch.stack([cpu(t) for t in g_hvs]), torch.stack([cpu(t) for t in g_dms])], 2).reshape(x.shape)
    worst['g_x'] = worst_ratio(got_x, ref['g_x'], bounds['g_x'])
    return worst


def _saved_of(head, xs):
    """what a decoder at keep level 'pose_head' keeps, built from the head's own launches -> (saved, tail inputs, a0s, a1s)"""
    ys = [head._conv_outputs(x[:, :128].contiguous(), x[:, 128:].contiguous()) for x in xs]
    five = lambda y: y if y.dim() == 5 else y[None]                 # noqa: E731
    saved = dict(hv=torch.stack([x[:, :128] for x in xs]).contiguous(), dm=torch.stack([x[:, 128:] for x in xs]).contiguous())
    for i in range(3):
        saved[f'y{i}'] = torch.stack([five(y[i]) for y in ys], 1).contiguous()
    a0s = [head.conv_layers[0](x[:, :128].contiguous(), x[:, 128:].contiguous()) for x in xs]
    a1s = [head.conv_layers[1](a) for a in a0s]
    return saved, [y[2] for y in ys], a0s, a1s


@pytest.mark.parametrize('fused', [True, False])
@pytest.mark.parametrize('T', [1, 3])
@pytest.mark.parametrize('feat_size', [(8, 8), (16, 16), (32, 32), (12, 20)], ids=lambda v: f'{v[0]}x{v[1]}')
def test_conv_backward_against_float64_given_the_masks(feat_size, T, fused):
    """(12, 20) passes through a 3-row map and gives 128 * 2 * 3 = 768 features; where fc_plan() refuses a geometry the
    scf_linear route is the one that runs under both settings"""
    head = _head(feat_size)
    head.fused_fc = fused
    gen = torch.Generator().manual_seed(400 + T)
    n = 2
    label = torch.tensor([1, 19], dtype=torch.int64, device=DEV)
    xs = [D(torch.randn((n, 224, *feat_size), generator=gen)) for _ in range(T)]
    g_rots = [D(torch.randn((n, 6), generator=gen)) for _ in range(T)]
    g_trans = [D(torch.randn((n, 3), generator=gen)) for _ in range(T)]
    saved, ys, a0s, a1s = _saved_of(head, xs)
    # the activations conv_backward recomputes on the stacked samples are the forward's, bit for bit
    for i, fwd in ((0, a0s), (1, a1s)):
        y, blk = saved[f'y{i}'], head.conv_layers[i]
        yv = y.view(y.shape[0], T * n, *y.shape[3:])
        a = ops.group_norm_relu(yv if y.shape[0] > 1 else yv[0], blk.gn.weight, blk.gn.bias, blk.groups, blk.gn.eps)
        assert same_bits(a, torch.cat(fwd)), f'a{i} recomputed on the stacked samples differs from the forward'
    names = set(dict(head.named_parameters()))
    for mode in (0, 1):
        head.label_mode = mode
        g_ys, tail_grads = head.tail_backward(ys, label, g_rots, g_trans)
        g_hvs, g_dms, grads = head.conv_backward(saved, g_ys, dict(tail_grads))
        assert set(grads) == names, 'every parameter of the head has a gradient'
        assert all(g.shape == (n, 128, *feat_size) for g in g_hvs) and all(g.shape == (n, 96, *feat_size) for g in g_dms)
        assert all(same_bits(grads[k], tail_grads[k]) for k in tail_grads)
        again = head.conv_backward(saved, g_ys)
        assert all(same_bits(a, b) for a, b in zip(g_hvs + g_dms, again[0] + again[1]))
        assert sorted(again[2]) == sorted(HC.CONV_NAMES) and all(same_bits(grads[k], again[2][k]) for k in HC.CONV_NAMES)
        g_y2, b_gy2 = _tail_refs(head, ys, label, g_rots, g_trans, mode)
        worst = _conv_check(head, saved, g_y2, b_gy2, g_hvs, g_dms, grads)
        for key, v in worst.items():
            measured(f'conv_backward {feat_size} T {T} fused {fused} label_mode {mode} {key}, error / composed bound', v)
            assert v <= 1.0, key
    if T == 3 and fused:                # accumulation over calls = one call per iteration, one rounding apart each
        head.label_mode = 0
        g_ys, _ = head.tail_backward(ys, label, g_rots, g_trans)
        one_saved = [{k: (v[t:t + 1] if k in ('hv', 'dm') else v[:, t:t + 1]).contiguous() for k, v in saved.items()} for t in range(T)]
        acc = {}
        for t in range(T):
            head.conv_backward(one_saved[t], g_ys[t:t + 1], acc)
        one = [head.conv_backward(one_saved[t], g_ys[t:t + 1])[2] for t in range(T)]
        for key in HC.CONV_NAMES:
            assert same_bits(acc[key], (one[0][key] + one[1][key]) + one[2][key]), key
        with pytest.raises(ScflowHipError):
            head.conv_backward(saved, g_ys, {HC.CONV_NAMES[0]: acc[HC.CONV_NAMES[0]]})
        with pytest.raises(ScflowHipError):
            head.conv_backward(dict(saved, y0=saved['y0'][:, :2].contiguous()), g_ys)
    head.label_mode = 0


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


def test_loss_and_pose_head_grads(scflow_model):
    m, case = scflow_model
    data = HL.refiner_data(case, DEV)
    plain = m.loss(None, data=data)
    base = m.loss_and_pose_tail_grads(None, data=data)
    loss, log_imgs, log_vars, seq_r, seq_t, grads = m.loss_and_pose_head_grads(None, data=data)
    assert same_bits(loss, plain[0]) and list(log_vars.items()) == list(plain[2].items()) and log_imgs is None
    assert sorted(grads) == sorted(list(base[5]) + ['pose_head_inputs'])
    for key, seq in base[5].items():
        if key == 'params':
            assert all(same_bits(grads['params'][k], v) for k, v in seq.items()), key
        else:
            assert all(same_bits(a, b) for a, b in zip(grads[key], seq)), key
    dec = m.decoder
    head = dec.pose_pred
    assert dec.keep == 'none'
    assert len(dec.kept['tail_inputs']) == dec.iters == HL.REFINER_ITERS
    prefix = 'decoder.pose_pred.'
    assert set(grads['params']) == {prefix + k for k in dict(head.named_parameters())}
    params = {k[len(prefix):]: v for k, v in grads['params'].items()}
    g_hvs, g_dms = grads['pose_head_inputs']
    assert len(g_hvs) == len(g_dms) == dec.iters
    g_y2, b_gy2 = _tail_refs(head, dec.kept['tail_inputs'], data['labels'], grads['delta_rotation_preds'],
                             grads['delta_translation_preds'], head.label_mode)
    worst = _conv_check(head, dec.kept, g_y2, b_gy2, g_hvs, g_dms, params)
    for key, v in worst.items():
        measured(f'loss_and_pose_head_grads {key}, error / composed bound', v)
        assert v <= 1.0, key
    with pytest.raises(NotImplementedError, match='loss_and_pose_head_grads'):
        m.forward(data, return_loss=True)


def test_keeping_the_head_input_changes_no_bit(scflow_model):
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
            dec.keep = 'pose_head'
            on = get()
            dec.keep = 'none'
            assert sorted(dec.kept) == ['dm', 'hv', 'tail_inputs', 'y0', 'y1', 'y2']
            kept[c_iteration] = ({k: v.clone() for k, v in dec.kept.items() if k != 'tail_inputs'},
                                 [t.clone() for t in dec.kept['tail_inputs']])
            for a, b in zip(off, on):
                assert all(same_bits(x, y) for x, y in zip(a, b)), f'c_iteration {c_iteration}'
    finally:
        dec.keep, dec.c_iteration = 'none', old
    (sc, tc), (sp, tp) = kept[True], kept[False]
    assert sorted(sc) == sorted(sp) == ['dm', 'hv', 'y0', 'y1', 'y2'] and len(tc) == len(tp) == dec.iters
    assert all(same_bits(sc[k], sp[k]) for k in sc), 'the two loop forms keep different tensors'
    assert all(same_bits(a, b) for a, b in zip(tc, tp))
    # y2 is the tail input, and the saved raw outputs are the head's own on the saved hv, dm
    head = dec.pose_pred
    for t in range(dec.iters):
        ys = head._conv_outputs(sc['hv'][t], sc['dm'][t])
        for i, y in enumerate(ys):
            assert same_bits(sc[f'y{i}'][:, t], y if y.dim() == 5 else y[None]), (t, i)
        assert same_bits(sc['y2'][:, t], tc[t] if tc[t].dim() == 5 else tc[t][None])


# ==================================================================================== the reference's own head (fixture)
@pytest.mark.parametrize('fs', HC.GOLDEN_FEAT_SIZES, ids=lambda v: f'{v[0]}x{v[1]}')
def test_kernels_against_the_reference_fixture(fs):
    """tail_backward + conv_backward on the fixture's seeds against the reference's recorded autograd.  Both are fp32
    evaluations around the float64 backward of tests/test_conv_grad_host.py::golden_reference, each inside its room, so
    they are at most two rooms apart; the kernels' own, tighter bounds are held by the tests above."""
    z = np.load(HC.GOLDEN)
    tag, x, p, tail, g_rot, g_tr, k0, hw = HC.golden_case(fs)
    head = _head(fs)
    with torch.no_grad():
        for name, prm in head.named_parameters():
            prm.copy_(HF.golden_param(name, tuple(prm.shape), HC.GOLDEN_SEED))
    head.label_mode = 0
    label = torch.tensor(HC.GOLDEN_LABELS, dtype=torch.int64, device=DEV)
    f32 = lambda v: D(torch.from_numpy(v).float())                  # noqa: E731
    saved, ys, _, _ = _saved_of(head, [f32(x)])
    g_ys, tail_grads = head.tail_backward(ys, label, [f32(g_rot)], [f32(g_tr)])
    g_hvs, g_dms, grads = head.conv_backward(saved, g_ys, tail_grads)
    got = {k: cpu(grads[k]) for k in HC.CONV_NAMES}
    got['g_x'] = torch.cat([cpu(g_hvs[0]), cpu(g_dms[0])], 1)
    _, ref, room = HC.golden_reference(fs)
    for key in HC.CONV_NAMES + ['g_x']:
        v = worst_ratio(HC.golden_pick(key, got[key].numpy()), z[f'{tag}.{key}'], 2.0 * HC.golden_pick(key, room[key]))
        measured(f'kernels - reference fixture {tag} {key}, difference / two rooms', v)
        assert v <= 1.0, key
        fixture = z[f'{tag}.{key}']
        measured(f'kernels - reference fixture {tag} {key}, relative to the largest entry',
                 float(np.abs(HC.golden_pick(key, got[key].numpy()) - fixture).max() / np.abs(fixture).max()))
