"""GPU: fc_grad.hip (scf_fc_operand, scf_pose_select_grad, scf_fc_dgrad, scf_fc_wgrad, scf_group_norm_flat_grad),
MultiClassPoseHead.tail_backward, SCFlowDecoder.keep = 'pose_tail' and SCFlowRefiner.loss_and_pose_tail_grads against the
float64 restatements and the derived bounds of tests/test_fc_grad_host.py.  Every comparison is `error <= bound` over ALL
elements (ratio <= 1) or bit equality; there is no absolute tolerance.  The measured ratios are recorded in DESIGN.md
section 4.7."""
import json
import os

import numpy as np
import pytest
import torch

import scflow_amd
from scflow_amd import _lib, ops
from scflow_amd._lib import ScflowHipError
import test_fc_grad_host as HF
import test_loss_host as HL
from test_fc_host import (ACT_NONE, ACT_RELU, FC_GN, FC_HEAD_GEOMETRY, fc_depth, fc_gn_ref, fc_operand, gemm_ref,  # noqa: E402
                          linear_ref_core, parts_ref)
from test_stream_ops_host import IN_EPS, f64, group_norm_relu_ref, measured, same_bits, worst_ratio  # noqa: E402

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
def _dgrad(g, w, a=None):
    gbuf, out = guarded((g.shape[0], w.shape[1]))
    got = ops.fc_dgrad(D(g), D(w), D(a), out=out)
    assert guard_untouched(gbuf, out.shape)
    again = ops.fc_dgrad(D(g), D(w), D(a))
    assert same_bits(got, again), 'two runs differ'
    m = g.shape[0]
    if m > 1:                                   # every row (three of them when M > 65) as a launch of its own
        for r in (range(m) if m <= 65 else (0, m // 2, m - 1)):
            one = ops.fc_dgrad(D(g[r:r + 1]), D(w), None if a is None else D(a[r:r + 1]))
            assert same_bits(got[r:r + 1], one), 'a row depends on its batch'
    return got.cpu()


def _wgrad(g, a, prev=None):
    o, k = g.shape[1], a.shape[1]
    wbuf, dw = guarded((o, k))
    bbuf, db = guarded((o,))
    if prev is not None:
        dw.copy_(prev[0])
        db.copy_(prev[1])
    ops.fc_wgrad(D(g), D(a), dw, db, accumulate=prev is not None)
    assert guard_untouched(wbuf, dw.shape) and guard_untouched(bbuf, db.shape)
    if prev is None:
        dw2, db2 = ops.fc_wgrad(D(g), D(a))
        assert same_bits(dw, dw2) and same_bits(db, db2), 'two runs differ'
    return dw.cpu(), db.cpu()


@pytest.mark.parametrize('m, o, k', HF.gemm_shapes())
def test_dgrad_wgrad_tiles(m, o, k):
    g, w, a, _ = HF.gemm_case('nominal', m, o, k)
    r1 = worst_ratio(_dgrad(g, w, a), *HF.dgrad_ref(g, 0.0, w, f64(a) > 0))
    r2 = worst_ratio(_dgrad(g, w), *HF.dgrad_ref(g, 0.0, w))
    dw, db = _wgrad(g, a)
    rw, rb = HF.wgrad_ref(g, 0.0, a)
    r3, r4 = worst_ratio(dw, *rw), worst_ratio(db, *rb)
    measured(f'dgrad / wgrad M {m} O {o} K {k}, error / bound (masked, plain, dW, db)', max(r1, r2, r3, r4))
    assert max(r1, r2, r3, r4) <= 1.0


@pytest.mark.parametrize('regime', HF.GEMM_REGIMES[1:])
def test_dgrad_wgrad_regimes(regime):
    worst = 0.0
    for m, o, k in HF.gemm_shapes()[::6]:
        g, w, a, scale = HF.gemm_case(regime, m, o, k)
        gs, (dw, db) = _dgrad(g, w, a), _wgrad(g, a)
        rw, rb = HF.wgrad_ref(g, 0.0, a)
        worst = max(worst, worst_ratio(gs, *HF.dgrad_ref(g, 0.0, w, f64(a) > 0)), worst_ratio(dw, *rw), worst_ratio(db, *rb))
        if regime in HF.GRAD_SCALES:                                # powers of two scale the bits
            g1, w1, a1, _ = HF.gemm_case('nominal', m, o, k)
            eg = 2.0 ** HF.GRAD_SCALES[regime][0]
            assert same_bits(gs, _dgrad(g1, w1, a1) * scale)
            dw1, db1 = _wgrad(g1, a1)
            assert same_bits(dw, dw1 * scale) and same_bits(db, db1 * eg)
    measured(f'dgrad / wgrad {regime}, error / bound', worst)
    assert worst <= 1.0


def test_wgrad_accumulate_is_one_more_rounding():
    for m, o, k in ((65, 33, 72), (257, 40, 264), (1, 1, 8)):
        g, _, a, _ = HF.gemm_case('nominal', m, o, k)
        gen = torch.Generator().manual_seed(3)
        prev = (torch.randn((o, k), generator=gen), torch.randn((o,), generator=gen))
        dw, db = _wgrad(g, a, prev)
        one, oneb = _wgrad(g, a)
        assert same_bits(dw, prev[0] + one) and same_bits(db, prev[1] + oneb)       # the stated order: previous value + sum
        rw, rb = HF.wgrad_ref(g, 0.0, a, prev=prev)
        assert worst_ratio(dw, *rw) <= 1.0 and worst_ratio(db, *rb) <= 1.0


def test_adjoint_identity_against_the_forward_kernel():
    """<fc_splitk(a), g> = <a, fc_dgrad(g)> inside the two kernels' bounds"""
    worst = 0.0
    for m, o, k in ((33, 40, 72), (65, 33, 256), (1, 1, 8), (257, 31, 56)):
        g, w, a, _ = HF.gemm_case('nominal', m, o, k)
        y = ops.fc_splitk(D(a), D(w)).cpu()
        gs = _dgrad(g, w)
        _, yb = gemm_ref(f64(a), 0.0, f64(w), None, fc_depth(k, False))
        _, gb = HF.dgrad_ref(g, 0.0, w)
        lhs, rhs = float((f64(y) * f64(g)).sum()), float((f64(a) * f64(gs)).sum())
        room = float((np.abs(f64(g)) * yb[0]).sum() + (np.abs(f64(a)) * gb).sum())
        worst = max(worst, abs(lhs - rhs) / room)
    measured('adjoint identity, |<y, g> - <a, g_s>| / room', worst)
    assert worst <= 1.0


def test_zero_cotangents_and_nan_containment():
    m, o, k = 65, 40, 72
    g, w, a, _ = HF.gemm_case('nominal', m, o, k)
    a = a + 0.5                                                     # every mask open: the NaN must show in the whole row
    z = torch.zeros_like(g)
    assert same_bits(_dgrad(z, w, a), torch.zeros((m, k)))
    dw, db = _wgrad(z, a)
    assert same_bits(dw, torch.zeros((o, k))) and same_bits(db, torch.zeros((o,)))
    m0, o0 = 37, 33
    g[m0, o0] = float('nan')
    gs = _dgrad(g, w, a)
    dw, db = _wgrad(g, a)
    rows = torch.isnan(gs).all(1)
    assert bool(rows[m0]) and int(torch.isnan(gs).sum()) == k
    assert bool(torch.isnan(dw[o0]).all()) and int(torch.isnan(dw).sum()) == k
    assert bool(torch.isnan(db[o0])) and int(torch.isnan(db).sum()) == 1
    a[m0, 5] = 0.0                                                  # a closed mask passes nothing, NaN included
    assert float(_dgrad(g, w, a)[m0, 5]) == 0.0
    a[m0, 6] = float('nan')                                         # a NaN activation is 0 in the forward: no gradient
    assert float(_dgrad(g, w, a)[m0, 6]) == 0.0


# =========================================================================================================== operand
def _staged_by_forward(x, **kw):
    """the operand as the forward staged it: an identity weight makes scf_fc_splitk return it (x 1, + 0: exact)"""
    k = x.shape[-1]
    return ops.fc_splitk(x, torch.eye(k, device=DEV), **kw)


@pytest.mark.parametrize('parts', [1, 2, 5, 9])
def test_operand_equals_the_forwards_staging_bit_for_bit(parts):
    gen = torch.Generator().manual_seed(40 + parts)
    for m, k in ((33, 72), (1, 8), (65, 256)):
        x = D(torch.randn((parts, m, k), generator=gen) * 3)
        b = D(torch.randn((k,), generator=gen))
        for kw in (dict(), dict(x_bias=b), dict(x_bias=b, x_relu=True), dict(x_relu=True)):
            buf, out = guarded((m, k))
            got = ops.fc_operand(x, out=out, **kw)
            assert guard_untouched(buf, out.shape)
            assert same_bits(got + 0.0, _staged_by_forward(x, **kw) + 0.0), (m, k, sorted(kw))
            assert same_bits(got.cpu(), fc_operand(x.cpu(), kw.get('x_bias', None) if kw.get('x_bias') is None else b.cpu(),
                                                   kw.get('x_relu', False)))


@pytest.mark.parametrize('gs, hw, k', [(gs, hw, k) for gs, hw, _, k in FC_GN if k <= 256] + [(4, 1, 128), (64, 16, 256), (64, 1, 128)])
def test_operand_group_norm_equals_the_forwards_fold(gs, hw, k):
    """groups of 64 (fc_group_norm_half<32>): about one group in 300 tells the compiled forward's order of the first two
    squares from the source's, so these cases run 1025 rows (1025 ... 4100 groups) in each of the three tile layouts"""
    gen = torch.Generator().manual_seed(gs + hw + k)
    c = -(-k // hw)
    gam, bet = D(1.0 + 0.5 * torch.randn((c,), generator=gen)), D(0.3 * torch.randn((c,), generator=gen))
    for parts, m in ((1, 1025 if gs == 64 else 33), (4, 2)):
        x = torch.randn((parts, m, k), generator=gen)
        x[0, 0, :gs] = 2.5                                          # a constant group: relu(beta)
        x[1:, 0, :gs] = 0.0
        x = D(x)
        gn = (k // gs, hw, gam, bet, IN_EPS)
        got = ops.fc_operand(x, gn=gn)
        assert same_bits(got + 0.0, _staged_by_forward(x, gn=gn) + 0.0), (parts, m)
        assert same_bits(got, ops.fc_operand(x, gn=gn))
        assert same_bits(got[m - 1:], ops.fc_operand(x[:, m - 1:].contiguous(), gn=gn))


# ========================================================================================================= selection
def _select(case, n, mode, mask=True, grads=None, accumulate=False):
    g_rot, g_trans, wr, wt, a, label = (D(t) for t in case)
    return ops.pose_select_grad(g_rot, g_trans, wr, wt, a, label, n, mode, mask=mask, grads=grads, accumulate=accumulate)


@pytest.mark.parametrize('n, t, k, nc', HF.SELECT_CASES)
def test_select_grad(n, t, k, nc):
    worst = 0.0
    for mode in (0, 1):
        for labels in HF.SELECT_LABELS:
            case = HF.select_case(n, t, k, nc, labels)
            cls = HF.clamp_class(case[5].numpy(), n * t, n, nc, mode)
            gs, grads = _select(case, n, mode)
            gs2, grads2 = _select(case, n, mode)
            assert same_bits(gs, gs2) and all(same_bits(x, y) for x, y in zip(grads, grads2))
            (rg, rb), rgrads = HF.select_ref(*case[:5], 0.0, cls, f64(case[4]) > 0)
            worst = max(worst, worst_ratio(gs.cpu(), rg, rb), *(worst_ratio(x.cpu(), *r) for x, r in zip(grads, rgrads)))
            plain, _ = _select(case, n, mode, mask=False)
            (rg, rb), _ = HF.select_ref(*case[:5], 0.0, cls)
            worst = max(worst, worst_ratio(plain.cpu(), rg, rb))
            for x, wd in zip(grads, (6, 6, 3, 3)):                  # classes no row selected: exact zeros
                x = x.cpu().reshape(nc, -1)
                assert all(bool((x[j] == 0).all()) for j in range(nc) if j not in set(cls.tolist()))
            # accumulate: untouched rows for unselected classes, previous + sum elsewhere
            prev = [torch.full_like(x, 3.25) for x in grads]
            _, acc = _select(case, n, mode, grads=[p.clone() for p in prev], accumulate=True)
            for x, one, wd in zip(acc, grads, (6, 6, 3, 3)):
                assert same_bits(x, 3.25 + one)
    measured(f'pose_select_grad N {n} T {t} K {k} classes {nc}, error / bound', worst)
    assert worst <= 1.0


def test_select_grad_follows_label_mode():
    case = HF.select_case(3, 2, 72, 4)
    a, b = _select(case, 3, 0)[0], _select(case, 3, 1)[0]
    assert not same_bits(a, b) and same_bits(a[0], b[0])            # sample 0 is label[0] in both modes
    zero = (torch.zeros_like(case[0]), torch.zeros_like(case[1])) + tuple(case[2:])
    gs, grads = _select(zero, 3, 1)
    assert same_bits(gs, torch.zeros_like(gs)) and all(same_bits(x, torch.zeros_like(x)) for x in grads)


# ========================================================================================================= GroupNorm
def _gn_launch(y, x0, g_x0, gam, gsz, hw, **kw):
    k = y.shape[-1]
    return ops.group_norm_flat_grad(D(g_x0), D(y) if y.shape[0] > 1 else D(y[0]), D(x0), D(gam), k // gsz, hw, IN_EPS, **kw)


@pytest.mark.parametrize('gsz, hw, k', [(g, h, k) for g, h, _, k in HF.gn_geometries()])
def test_group_norm_flat_grad(gsz, hw, k):
    worst = {}
    for regime in HF.GN_GRAD_REGIMES:
        m, parts = (3 if k > 512 else 33), (4 if gsz == 64 and hw == 16 else 1)
        y, ysum, gam, bet, x0, g_x0, scale = HF.gn_grad_case(regime, gsz, hw, k, m, parts)
        gy, dg, db = _gn_launch(y, x0, g_x0, gam, gsz, hw)
        gy2, dg2, db2 = _gn_launch(y, x0, g_x0, gam, gsz, hw)
        assert same_bits(gy, gy2) and same_bits(dg, dg2) and same_bits(db, db2), 'two runs differ'
        for r in (range(m) if regime == 'nominal' else (m - 1,)):       # every row as a launch of its own
            one = _gn_launch(y[:, r:r + 1], x0[r:r + 1], g_x0[r:r + 1], gam, gsz, hw)[0]
            assert same_bits(gy[r:r + 1], one), 'a row depends on its batch'
        rgy, rdg, rdb = HF.gn_grad_ref(f64(ysum), g_x0, 0.0, f64(x0) > 0, gam, gsz, hw)
        worst[regime] = max(worst_ratio(gy.cpu(), *rgy), worst_ratio(dg.cpu(), *rdg), worst_ratio(db.cpu(), *rdb))
        if regime in HF.GRAD_SCALES:
            n = HF.gn_grad_case('nominal', gsz, hw, k, m, parts)
            gy1, dg1, db1 = _gn_launch(n[0], n[4], n[5], n[2], gsz, hw)
            assert same_bits(gy, gy1 * scale) and same_bits(dg, dg1 * scale) and same_bits(db, db1 * scale)
        if regime == 'nominal':
            z = _gn_launch(y, x0, torch.zeros_like(g_x0), gam, gsz, hw)
            assert all(same_bits(t + 0.0, torch.zeros_like(t)) for t in z)
            prev = (torch.full_like(dg, 1.5), torch.full_like(db, -2.5))
            _, adg, adb = _gn_launch(y, x0, g_x0, gam, gsz, hw, dgamma=prev[0].clone(), dbeta=prev[1].clone(), accumulate=True)
            assert same_bits(adg, 1.5 + dg) and same_bits(adb, -2.5 + db)
    for regime, v in worst.items():
        measured(f'group_norm_flat_grad group {gsz} hw {hw} K {k} {regime}, error / bound', v)
        assert v <= 1.0, regime


def test_group_norm_flat_grad_many_rows():
    """257 rows: a second row per thread of the parameter pass"""
    y, ysum, gam, bet, x0, g_x0, _ = HF.gn_grad_case('nominal', 64, 16, 128, 257, 2)
    gy, dg, db = _gn_launch(y, x0, g_x0, gam, 64, 16)
    rgy, rdg, rdb = HF.gn_grad_ref(f64(ysum), g_x0, 0.0, f64(x0) > 0, gam, 64, 16)
    worst = max(worst_ratio(gy.cpu(), *rgy), worst_ratio(dg.cpu(), *rdg), worst_ratio(db.cpu(), *rdb))
    measured('group_norm_flat_grad 257 rows, error / bound', worst)
    assert worst <= 1.0


# ============================================================================================= sentinels, rejections
def test_sentinel_bands_of_the_raw_entries():
    lib, st = _lib.load(), ops._stream()
    m, k, nc, n = 33, 72, 3, 11
    case = [D(t) for t in HF.select_case(n, 3, k, nc)]
    bufs = [guarded(s) for s in ((m, k), (6 * nc, k), (6 * nc,), (3 * nc, k), (3 * nc,))]
    assert lib.scf_pose_select_grad(*(t.data_ptr() for t in case), n, nc, 1, *(b[1].data_ptr() for b in bufs), 0, m, k, st) == 0
    y, ysum, gam, bet, x0, g_x0, _ = HF.gn_grad_case('nominal', 8, 3, 64, 33, 1)
    c = -(-64 // 3)
    nb = [guarded(s) for s in ((33, 64), (c,), (c,), (33, 8, 2))]
    ins = [D(g_x0), D(y[0]), D(x0), D(gam)]
    assert lib.scf_group_norm_flat_grad(ins[0].data_ptr(), ins[1].data_ptr(), 1, 0, ins[2].data_ptr(), ins[3].data_ptr(), 8, 3,
                                        IN_EPS, nb[0][1].data_ptr(), nb[1][1].data_ptr(), nb[2][1].data_ptr(), 0,
                                        nb[3][1].data_ptr(), 33, 64, st) == 0
    torch.cuda.synchronize()
    for buf, view in bufs + nb:
        assert guard_untouched(buf, view.shape) and not bool((view == SENTINEL).any())


def test_c_abi_rejections():
    lib, st = _lib.load(), ops._stream()
    t = torch.zeros((64, 64), device=DEV)
    lab = torch.zeros((4,), dtype=torch.int64, device=DEV)
    p = t.data_ptr()
    assert lib.scf_fc_dgrad(None, p, None, p, 4, 4, 4, st) == EINVAL and lib.scf_fc_dgrad(p, p, None, p, 0, 4, 4, st) == EINVAL
    assert lib.scf_fc_dgrad(p, p, None, None, 4, 4, 4, st) == EINVAL
    assert lib.scf_fc_wgrad(p, None, p, p, 4, 4, 4, 0, st) == EINVAL and lib.scf_fc_wgrad(p, p, p, None, 4, -1, 4, 0, st) == EINVAL
    assert lib.scf_fc_operand(p, 0, 0, None, 0, 0, 1, None, None, 0.0, p, 4, 8, st) == EINVAL
    assert lib.scf_fc_operand(p, 2, 8, None, 0, 0, 1, None, None, 0.0, p, 4, 8, st) == EINVAL          # parts overlap
    assert lib.scf_fc_operand(p, 1, 0, None, 0, 2, 1, None, p, 1e-5, p, 4, 8, st) == EINVAL           # no gamma
    assert lib.scf_fc_operand(p, 1, 0, None, 0, 3, 1, p, p, 1e-5, p, 4, 8, st) == EINVAL              # 8 % 3
    assert lib.scf_fc_operand(p, 1, 0, None, 0, 2, 1, p, p, 1e-5, p, 4, 6, st) == EUNSUPPORTED        # odd groups
    sel = lambda *a: lib.scf_pose_select_grad(*a)                   # noqa: E731
    assert sel(p, p, p, p, p, lab.data_ptr(), 3, 2, 0, p, None, None, None, None, 0, 4, 8, st) == EINVAL   # 4 % 3
    assert sel(p, p, p, p, p, lab.data_ptr(), 2, 2, 4, p, None, None, None, None, 0, 4, 8, st) == EINVAL   # unknown flag
    assert sel(p, p, p, p, p, lab.data_ptr(), 2, 2, 0, None, p, None, p, p, 0, 4, 8, st) == EINVAL         # three of four
    assert sel(p, p, p, p, None, lab.data_ptr(), 2, 2, 0, None, p, p, p, p, 0, 4, 8, st) == EINVAL         # dW without a
    assert sel(p, p, p, p, p, None, 2, 2, 0, p, None, None, None, None, 0, 4, 8, st) == EINVAL
    gn = lambda *a: lib.scf_group_norm_flat_grad(*a)                # noqa: E731
    assert gn(p, p, 1, 0, p, p, 3, 1, 1e-5, p, p, p, 0, p, 4, 8, st) == EINVAL
    assert gn(p, p, 1, 0, p, p, 2, 1, 1e-5, p, p, p, 0, p, 4, 6, st) == EUNSUPPORTED
    assert gn(p, p, 1, 0, p, p, 2, 1, 1e-5, p, p, None, 0, p, 4, 8, st) == EINVAL
    assert gn(p, p, 1, 0, p, p, 2, 1, 1e-5, p, p, p, 0, None, 4, 8, st) == EINVAL
    torch.cuda.synchronize()
    assert bool((t == 0).all())                                     # nothing was launched
    with pytest.raises(ScflowHipError):
        ops.fc_dgrad(t[:4], t[:5, :8].contiguous())
    with pytest.raises(ScflowHipError):
        ops.fc_wgrad(t[:4], t[:5])
    with pytest.raises(ScflowHipError):
        ops.fc_operand(t, x_bias=t[0, :8].contiguous())
    with pytest.raises(ScflowHipError):
        ops.group_norm_flat_grad(t, t, t[:8], t[0], 2, 1)
    with pytest.raises(ScflowHipError):
        ops.pose_select_grad(t[:4, :6].contiguous(), t[:4, :3].contiguous(), t[:12, :8].contiguous(), t[:5, :8].contiguous(),
                             t[:4, :8].contiguous(), lab, 2)


# ===================================================================================================== tail_backward
def _head(feat_size, seed=5):
    from scflow_amd.registry import HEAD, build_from_cfg
    cfg = dict(scflow_amd.scflow_model_cfg()['decoder']['pose_head_cfg'], feat_size=feat_size)
    head = build_from_cfg(cfg, HEAD)
    g = torch.Generator().manual_seed(seed)
    for prm in head.parameters():
        prm.data.copy_(torch.randn(prm.shape, generator=g) * (0.05 if prm.dim() > 1 else 0.1))
    with torch.no_grad():
        head.conv_layers[2].gn.weight.add_(1.0)
    return head.to(DEV)


NAMES = dict(W1='fc_layers.0.0.weight', b1='fc_layers.0.0.bias', W2='fc_layers.1.0.weight', b2='fc_layers.1.0.bias',
             Wr='rotation_pred.weight', br='rotation_pred.bias', Wt='translation_pred.weight', bt='translation_pred.bias',
             gamma='conv_layers.2.gn.weight', beta='conv_layers.2.gn.bias')


def _tail_check(head, ys, label, g_rots, g_trans, g_ys, grads, mode):
    """worst error / composed bound of tail_backward's results against the float64 tail given the kernel's masks: every
    stage's bound goes through the next stage's sum of magnitudes; the forward's activation bounds (tests/test_fc_host.py)
    enter the weight gradients."""
    cpu = lambda t: t.detach().cpu()                                # noqa: E731
    T, n = len(ys), g_rots[0].shape[0]
    m = T * n
    y5 = [y if y.dim() == 5 else y[None] for y in ys]
    parts = torch.stack([cpu(y) for y in y5], 1).reshape(y5[0].shape[0], m, -1)
    hw = ys[0].shape[-1] * ys[0].shape[-2]
    k = parts.shape[-1]
    last, fc1, fc2 = head.conv_layers[2], head.fc_layers[0][0], head.fc_layers[1][0]
    gsz = k // last.groups
    p32 = {key: cpu(dict(head.named_parameters())[name]) for key, name in NAMES.items()}
    p = {key: f64(v) for key, v in p32.items()}
    x0, a1, a2 = (cpu(t) for t in head._tail(D(parts).view(parts.shape[0], m, -1, *ys[0].shape[-2:]), activations=True))
    masks = tuple(f64(t) > 0 for t in (x0, a1, a2))
    ysum = fc_operand(parts)
    nc = head.num_class
    cls = HF.clamp_class(cpu(label).numpy(), m, n, nc, mode)
    g_rot, g_tr = torch.cat([cpu(g) for g in g_rots]), torch.cat([cpu(g) for g in g_trans])
    ref = HF.tail_ref64(f64(ysum), p, cls, f64(g_rot), f64(g_tr), gsz, hw, masks)
    # ---- the forward's activation bounds
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
    # ---- the backward, stage by stage
    (_, b_s2), hg = HF.select_ref(g_rot, g_tr, p['Wr'], p['Wt'], ref['a2'], a2b, cls, masks[2])
    (_, bw2), (_, bb2) = HF.wgrad_ref(ref['g_s2'], b_s2, ref['a1'], a1b)
    _, b_s1 = HF.dgrad_ref(ref['g_s2'], b_s2, p['W2'], masks[1])
    (_, bw1), (_, bb1) = HF.wgrad_ref(ref['g_s1'], b_s1, ref['x0'], x0b)
    _, b_x0 = HF.dgrad_ref(ref['g_s1'], b_s1, p['W1'])
    (_, b_gy), (_, b_dg), (_, b_db) = HF.gn_grad_ref(f64(ysum), ref['g_x0'], b_x0, masks[0], p32['gamma'], gsz, hw)
    bounds = dict(W1=bw1, b1=bb1, W2=bw2, b2=bb2, Wr=hg[0][1], br=hg[1][1], Wt=hg[2][1], bt=hg[3][1], gamma=b_dg, beta=b_db)
    worst = {key: worst_ratio(cpu(grads[NAMES[key]]), ref[key], bounds[key]) for key in NAMES}
    worst['g_y'] = worst_ratio(torch.cat([cpu(g).reshape(n, -1) for g in g_ys]), ref['g_y'], b_gy)
    return worst


@pytest.mark.parametrize('feat_size', list(FC_HEAD_GEOMETRY) + [(8, 24)], ids=lambda v: f'{v[0]}x{v[1]}')
@pytest.mark.parametrize('T', [1, 3])
def test_tail_backward_against_float64_given_the_masks(feat_size, T):
    """(8, 24): 384 features, a geometry fc_plan() refuses (no whole K-slices of 256): the scf_linear route under both
    settings; the three others take the split-K route with fused_fc and the scf_linear route without"""
    head = _head(feat_size)
    gen = torch.Generator().manual_seed(300 + T)
    n = 2
    label = torch.tensor([1, 19], dtype=torch.int64, device=DEV)
    xs = [D(torch.randn((n, 224, *feat_size), generator=gen)) for _ in range(T)]
    g_rots = [D(torch.randn((n, 6), generator=gen)) for _ in range(T)]
    g_trans = [D(torch.randn((n, 3), generator=gen)) for _ in range(T)]
    for fused in (True, False):
        for mode in (0, 1):
            head.fused_fc, head.label_mode = fused, mode
            ys = [head.tail_input(x) for x in xs]
            g_ys, grads = head.tail_backward(ys, label, g_rots, g_trans)
            assert sorted(grads) == sorted(NAMES.values()) and set(grads) <= set(dict(head.named_parameters()))
            assert all(g.shape == (n, 128, feat_size[0] // 8, feat_size[1] // 8) for g in g_ys)
            again_y, again = head.tail_backward(ys, label, g_rots, g_trans)
            assert all(same_bits(a, b) for a, b in zip(g_ys, again_y)) and all(same_bits(grads[k], again[k]) for k in grads)
            worst = _tail_check(head, ys, label, g_rots, g_trans, g_ys, grads, mode)
            for key, v in worst.items():
                measured(f'tail_backward {feat_size} T {T} fused {fused} label_mode {mode} {key}, error / composed bound', v)
                assert v <= 1.0, key
            if T == 3 and mode == 0:        # accumulation over calls = one call over all iterations, one rounding apart
                acc = {}
                for t in range(T):
                    head.tail_backward(ys[t:t + 1], label, g_rots[t:t + 1], g_trans[t:t + 1], param_grads=acc)
                assert sorted(acc) == sorted(grads)
                one = [head.tail_backward(ys[t:t + 1], label, g_rots[t:t + 1], g_trans[t:t + 1])[1] for t in range(T)]
                for key in grads:
                    assert same_bits(acc[key], (one[0][key] + one[1][key]) + one[2][key]), key
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


def test_loss_and_pose_tail_grads(scflow_model):
    m, case = scflow_model
    data = HL.refiner_data(case, DEV)
    plain = m.loss(None, data=data)
    base = m.loss_and_head_grads(None, data=data)
    loss, log_imgs, log_vars, seq_r, seq_t, grads = m.loss_and_pose_tail_grads(None, data=data)
    assert same_bits(loss, plain[0]) and list(log_vars.items()) == list(plain[2].items()) and log_imgs is None
    assert sorted(grads) == sorted(list(base[5]) + ['pose_tail_inputs', 'params'])
    for key, seq in base[5].items():
        assert all(same_bits(a, b) for a, b in zip(grads[key], seq)), key
    dec = m.decoder
    assert dec.keep == 'none' and len(dec.kept['tail_inputs']) == dec.iters == HL.REFINER_ITERS
    prefix = 'decoder.pose_pred.'
    assert all(k.startswith(prefix) and k in dict(m.named_parameters()) for k in grads['params'])
    params = {k[len(prefix):]: v for k, v in grads['params'].items()}
    worst = _tail_check(dec.pose_pred, dec.kept['tail_inputs'], data['labels'], grads['delta_rotation_preds'],
                        grads['delta_translation_preds'], grads['pose_tail_inputs'], params, dec.pose_pred.label_mode)
    for key, v in worst.items():
        measured(f'loss_and_pose_tail_grads {key}, error / composed bound', v)
        assert v <= 1.0, key
    with pytest.raises(NotImplementedError, match='loss_and_pose_tail_grads'):
        m.forward(data, return_loss=True)


@pytest.mark.parametrize('c_iteration', [True, False])
def test_keeping_the_tail_input_changes_no_bit(scflow_model, c_iteration):
    m, case = scflow_model
    data = HL.refiner_data(case, DEV)
    dec = m.decoder
    get = lambda: m.get_pose(data['rendered_images'], data['real_images'], data['ref_rotations'], data['ref_translations'],   # noqa: E731
                             data['rendered_depths'], data['internel_k'], data['labels'])
    old = dec.c_iteration
    dec.c_iteration = c_iteration
    try:
        dec.kept = {}
        off = get()
        assert dec.kept == {}
        dec.keep = 'pose_tail'
        on = get()
        assert sorted(dec.kept) == ['tail_inputs']
        kept = list(dec.kept['tail_inputs'])
    finally:
        dec.keep, dec.c_iteration = 'none', old
    assert len(kept) == dec.iters
    for a, b in zip(off, on):
        assert all(same_bits(x, y) for x, y in zip(a, b))
    # what was kept is the tail input: the forward's own launches on it give the iteration's pose deltas, bit for bit
    head = dec.pose_pred
    last, fc1, fc2 = head.conv_layers[2], head.fc_layers[0][0], head.fc_layers[1][0]
    s1, s2 = head.fc_plan()
    assert s1 and head.label_mode == 0
    cls = int(data['labels'][0])
    for i, y in enumerate(kept):
        n, hw = y.shape[-4], y.shape[-2] * y.shape[-1]
        yv = y.view(-1, n, fc1.in_features)
        p1 = ops.fc_splitk(yv, fc1.weight, gn=(last.groups, hw, last.gn.weight, last.gn.bias, last.gn.eps), slices=s1)
        p2 = ops.fc_splitk(p1, fc2.weight, x_bias=fc1.bias, x_relu=True, slices=s2)
        rot_all, trans_all = ops.fc_splitk(p2, head.rotation_pred.weight, head.rotation_pred.bias, x_bias=fc2.bias, x_relu=True,
                                           weight2=head.translation_pred.weight, bias2=head.translation_pred.bias)
        assert same_bits(rot_all[:, 6 * cls:6 * cls + 6], on[5][i]) and same_bits(trans_all[:, 3 * cls:3 * cls + 3], on[6][i])
