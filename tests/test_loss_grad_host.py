"""CPU: the GRADIENTS of the supervised losses (loss.hip, scf_seq_pixel_loss_grad / scf_point_matching_loss_grad) restated
in float64 with a bound on any fp32 evaluation in the kernels' operation order, on top of `pixel_decisions`, `pm_ref` and
`EV` of tests/test_loss_host.py; the proof that the closed forms ARE autograd's (torch autograd in float64 on a plain-torch
restatement of the reference's expressions), that the bounds are reachable (the reference's own fp32 gradients,
tests/golden/loss_grads.npz, fall inside) and not vacuous (planted defects fall outside); and the inputs
tests/test_gpu_loss_grad.py feeds the kernels.

Pixel gradients, per sequence, iteration and element:
    g = c * v * sgn(p - q);  v in {0, 1} and sgn in {-1, 0, 1} are exact DECISIONS (sgn compares the operands), so the
    products are exact and the whole error is the coefficient's:
    c = ((upstream * w_i) * loss_weight) / ((float)count + eps)          two products, one addition, one division: 4 U
    (the mask row divides by (float)(N H W), exact below 2**24: 3 roundings, bounded by the same 4 U).
Point matching, per sample and iteration: d = pred[idx] - target carries the coordinate roundings `pm_ref` propagates;
    L2: u = d / |d| -- the norm, then one division; L1: u = sgn(d), exact where |d| exceeds its own error and UNDECIDED
    where it does not: the full swing 2 of such a component stays in the bound, it is not excluded;
    u * x is one fp32 product; the sum over the V points is fp64 (V 2**-53); k and the translation scaling are fp64
    products and the result is rounded to fp32 ONCE.
The comparison with the REFERENCE's fp32 gradients needs torch's own fp32 summation (`torch_sum_term`) and the fp32
chain rule it runs instead of one fp64 scaling (`TORCH_CHAIN` roundings); neither is ever granted to the kernels.
"""
import json
import os
from functools import lru_cache

import numpy as np
import pytest
import torch

import test_loss_host as H
from test_loss_host import (EV, PM_DISENTANGLE, PM_DISENTANGLE_Z, PM_FULL, PM_ROT, PM_SCALE_DEPTH, PM_SCALE_XY, U, a32, a64, f32,
                            gamma_weights, measured, pixel_decisions, pm_ref, torch_sum_term)
from test_stream_ops_host import ev_matvec

U64 = 2.0 ** -53
TORCH_CHAIN = 8             # fp32 roundings of autograd's chain (weights, 1 / V, 1 / diameter, 1 / N, scalings) per element
GOLDEN_FILE = os.path.join(H.GOLDEN, 'loss_grads.npz')


def grad_ratio(got, ev):
    """|got - ev.v| / ev.e, elementwise worst, where the restatement is not NaN; the NaN patterns must be EQUAL."""
    got, v, e = np.asarray(got, dtype=np.float64), np.asarray(ev.v), np.broadcast_to(np.asarray(ev.e), np.asarray(ev.v).shape)
    if got.shape != v.shape or not np.array_equal(np.isnan(got), np.isnan(v)):
        return np.inf
    ok = ~np.isnan(v)
    err = np.abs(got[ok] - v[ok])
    with np.errstate(all='ignore'):
        r = np.where(err == 0, 0.0, err / e[ok])
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max()) if r.size else 0.0


# ================================================================================================== pixel gradients
def sgn_cmp(p, q, zero=0.0):
    """sgn(p - q) decided on the operands: 0 when equal, +-1 for +-inf, NaN when either is NaN."""
    p, q = np.asarray(p, dtype=np.float64), np.asarray(q, dtype=np.float64)
    return np.where(p > q, 1.0, np.where(p < q, -1.0, np.where(p == q, zero, np.nan)))


def pixel_grad_ref(gt, valid, flows=(), masks=None, max_flow=400., weights=(1., 1., 1.), eps=(1e-10, 1e-10), gammas=(.8, .8, .8),
                   mask_gt=None, upstream=(1., 1., 1.), defect=None):
    """-> dict(grads=[[EV per iteration] per flow sequence] + [[EV] mask], coef=the same nesting of scalar EV) in the
    kernel's row order; weights / gammas / upstream by the kernel's row (0, 1 flow sequences, 2 the mask)."""
    n = int(np.prod(a64(gt).shape)) // 2 if gt is not None else int(np.prod(a64(mask_gt).shape))
    out = dict(grads=[], coef=[])
    if gt is not None:
        v, occ = pixel_decisions(gt, valid, max_flow)
        g = a64(gt)
        cnt = float(v.sum())
        vf = np.where(v, 1.0, 0.0)[:, None]
    if mask_gt is not None:
        occ = a64(mask_gt)
    zero = 1.0 if defect == 'sgn0_is_1' else 0.0
    for s, seq in enumerate(flows):
        T = len(seq)
        gws = gamma_weights(gammas[s], T, reverse=(defect == 'gamma_reversed'))
        den = EV(cnt) + EV(float(f32(eps[s])))
        row, coefs = [], []
        for i, p in enumerate(seq):
            c = ((EV(float(f32(upstream[s]))) * EV(gws[i])) * EV(float(f32(weights[s])))) / den
            with np.errstate(invalid='ignore'):
                pat = vf * sgn_cmp(a64(p), g, zero)                         # 0 * NaN = NaN, like valid[:, None] * sgn
                val = float(c.v) * pat
                if defect == 'through_count':                               # a quotient rule that differentiates count(v)
                    S = float(np.where(v[:, None], np.abs(a64(p) - g), 0.0).sum())
                    val = val - float(c.v) * S / float(den.v) * vf
            row.append(EV(val, float(c.e) * np.abs(pat)))
            coefs.append(c)
        out['grads'].append(row)
        out['coef'].append(coefs)
    if masks is not None:
        T = len(masks)
        gws = gamma_weights(gammas[2], T, reverse=(defect == 'gamma_reversed'))
        row, coefs = [], []
        for i, m in enumerate(masks):
            c = ((EV(float(f32(upstream[2]))) * EV(gws[i])) * EV(float(f32(weights[2])))) / H.rnd(EV(float(n)))
            m = a64(m)
            pat = sgn_cmp(m.reshape(occ.shape), occ, zero).reshape(m.shape)
            if defect == 'valid_on_mask':
                pat = pat * np.where(v, 1.0, 0.0).reshape(m.shape)
            row.append(EV(float(c.v) * pat, float(c.e) * np.abs(pat)))
            coefs.append(c)
        out['grads'].append(row)
        out['coef'].append(coefs)
    return out


def torch_pixel_total(gt, valid, flows=(), masks=None, max_flow=400., weights=(1., 1., 1.), eps=(1e-10, 1e-10), gammas=(.8, .8, .8),
                      mask_gt=None, upstream=(1., 1., 1.)):
    """sum_row upstream[row] * total[row] with the reference's expressions (sequence_loss.py:17-24, 36, 74-80) in float64
    torch; flows / masks: float64 tensors (requires_grad).  The fp32 DECISIONS are the kernel's, as in `pixel_ref`."""
    total = 0.
    if gt is not None:
        v, occ = pixel_decisions(gt, valid, max_flow)
        vt, g = torch.from_numpy(np.where(v, 1.0, 0.0)), torch.from_numpy(a64(gt))
        occ = torch.from_numpy(occ)
    if mask_gt is not None:
        occ = torch.from_numpy(a64(mask_gt))
    for s, seq in enumerate(flows):
        loss = 0.
        for w, p in zip(gamma_weights(gammas[s], len(seq)), seq):
            li = (vt[:, None] * (p - g).abs()).sum() / (vt.sum() + float(f32(eps[s])))
            loss = loss + w * (float(f32(weights[s])) * li)
        total = total + float(f32(upstream[s])) * loss
    if masks is not None:
        loss = 0.
        for w, m in zip(gamma_weights(gammas[2], len(masks)), masks):
            loss = loss + w * (torch.mean(torch.abs(m.reshape(occ.shape) - occ)) * float(f32(weights[2])))
        total = total + float(f32(upstream[2])) * loss
    return total


# ================================================================================================== point matching
def _zeros(V):
    return EV(np.zeros(V))


def _unit(d, loss_type, defect=None):
    """d |d| / d d of three EV components -> ([u_x, u_y, u_z] EV, number of undecided L1 components)."""
    if loss_type == 1:
        out, und = [], 0
        for c in d:
            open_ = (np.abs(c.v) <= c.e) & (c.e > 0)                          # the fp32 sign may be anything: swing 2
            und += int(open_.sum())
            out.append(EV(np.sign(c.v), np.where(open_, 2.0, 0.0)))
        return out, und
    nm = H._norm(d, 2)
    zero = (nm.v == 0) & (nm.e == 0)
    safe = EV(np.where(zero, 1.0, nm.v), nm.e)
    out = []
    for c in d:
        q = c / safe
        fill = np.nan if defect == 'nan_at_zero' else 0.0
        out.append(EV(np.where(zero, fill, q.v), np.where(zero, 0.0, q.e)))
    return out, 0


def _fold(terms, torch_sums):
    """the fixed-order fp64 sum of the V per-point terms (EV arrays) -> (value, error)."""
    V = terms.v.shape[0]
    S, A = float(terms.v.sum()), float(np.abs(terms.v).sum())
    e = float(terms.e.sum()) + V * U64 * A
    if torch_sums:
        e += torch_sum_term(V, A)
    return S, e


def pm_grad_ref(verts, labels, symmetric, diameter, seq_r, seq_t, gt_r, gt_t, scale=None, mode=PM_FULL, loss_type=2, flags=0,
                sdf=1., reduction='mean', weight=1., gamma=.8, nn_idx=None, upstream=1., defect=None, torch_sums=False):
    """float64 restatement of the gradients of scf_point_matching_loss_grad with running error bounds, at the fp64
    neighbours of `pm_ref` (or at `nn_idx`) -> dict(grad_r [EV (N,3,3)] per iteration, grad_t [EV (N,3)] or None for
    PM_ROT, undecided: L1 components whose sign the bound cannot decide (their swing is IN the bound))."""
    T, N = len(seq_r), len(labels)
    labels = [int(x) for x in labels]
    if mode == PM_ROT:
        flags = 0
    free = pm_ref(verts, labels, symmetric, diameter, seq_r, seq_t, gt_r, gt_t, scale=scale, mode=mode, loss_type=loss_type,
                  flags=flags, sdf=sdf, nn_idx=nn_idx)
    gws = gamma_weights(gamma, T, reverse=(defect == 'gamma_reversed'))
    tg = H._scaled_t(gt_t, scale, flags, sdf) if mode != PM_ROT else None
    s_all = np.ones(N) if scale is None else a64(scale)
    sdf64 = float(f32(sdf))
    out = dict(grad_r=[], grad_t=[] if mode != PM_ROT else None, undecided=0)
    for t in range(T):
        tp = H._scaled_t(seq_t[t], scale, flags, sdf) if mode != PM_ROT else None
        Rv, Re, Tv, Te = np.zeros((N, 3, 3)), np.zeros((N, 3, 3)), np.zeros((N, 3)), np.zeros((N, 3))
        for n in range(N):
            c = labels[n]
            P = a64(verts[c])
            V = len(P)
            idx = free['nn'][t][n]
            idx = np.arange(V) if idx is None else np.asarray(idx)
            X = P if defect == 'own_point' else P[idx]                         # the NEIGHBOUR's model point, not x_p
            rp, rg = a64(seq_r[t])[n], a64(gt_r)[n]
            gr = ev_matvec(rg, [EV(P[:, i]) for i in range(3)])
            pr = ev_matvec(rp, [EV(P[idx][:, i]) for i in range(3)])
            if mode == PM_ROT:
                tgt, pred, same_add = gr, pr, True
            else:
                tgn, tpn = [H._pick(x, n) for x in tg], [H._pick(x, n) for x in tp]
                tgt = [gr[i] + tgn[i] for i in range(3)]
                add = tgn if mode == PM_DISENTANGLE else tpn
                pred = [pr[i] + add[i] for i in range(3)]
                same_add = all(float(add[i].v) == float(tgn[i].v) for i in range(3))
            # a prediction equal to the ground truth runs the same operations on the same bits: d is EXACTLY zero
            identical = same_add and np.array_equal(idx, np.arange(V)) and np.array_equal(rp, rg)
            d = [_zeros(V)] * 3 if identical else [pred[i] - tgt[i] for i in range(3)]
            u, und = _unit(d, loss_type, defect)
            out['undecided'] += und
            kk = float(f32(upstream)) * gws[t] * float(f32(weight)) / (V * float(f32(diameter[c])))
            if (reduction == 'mean') != (defect == 'sum_for_mean'):
                kk = kk / N
            for i in range(3):
                for j in range(3):
                    S, e = _fold(u[i] * EV(X[:, j]), torch_sums)
                    Rv[n, i, j], Re[n, i, j] = kk * S, abs(kk) * e
            if mode == PM_ROT:
                continue
            tsum = [[0.0, 0.0] for _ in range(3)]

            def add_term(uu):
                for i in range(3):
                    S, e = _fold(uu[i], torch_sums)
                    tsum[i][0] += S
                    tsum[i][1] += e
            if mode == PM_FULL or defect == 'rot_leak':
                add_term(u)
            if mode == PM_DISENTANGLE:
                combos = [[tgn[0], tgn[1], tpn[2]], [tpn[0], tpn[1], tgn[2]]] if flags & PM_DISENTANGLE_Z else [tpn]
                for tt in combos:
                    # (R_gt p + t'') - (R_gt p + t_gt'): a component that takes t_gt' (or an equal t_pred') is exactly zero
                    dd = [_zeros(V) if float(tt[i].v) == float(tgn[i].v) else (gr[i] + tt[i]) - tgt[i] for i in range(3)]
                    ub, und = _unit(dd, loss_type, defect)
                    out['undecided'] += und
                    add_term(ub)
            s = float(s_all[n])
            back = [s if flags & PM_SCALE_XY else 1.0] * 2 + [s * sdf64 if flags & PM_SCALE_DEPTH else sdf64]
            if defect == 'unscaled_t':
                back = [1.0, 1.0, 1.0]
            for i in range(3):
                Tv[n, i], Te[n, i] = kk * back[i] * tsum[i][0], abs(kk * back[i]) * tsum[i][1]
        chain = TORCH_CHAIN * U if torch_sums else 0.0
        fin = lambda v, e: EV._rnd(v, e + (8 * U64 + chain) * np.abs(v))      # fp64 scaling, then ONE fp32 rounding
        out['grad_r'].append(fin(Rv, Re))
        if mode != PM_ROT:
            out['grad_t'].append(fin(Tv, Te))
    return out


def torch_pm_total(verts, labels, symmetric, diameter, seq_r, seq_t, gt_r, gt_t, scale=None, mode=PM_FULL, loss_type=2, flags=0,
                   sdf=1., reduction='mean', weight=1., gamma=.8, nn=None, upstream=1.):
    """upstream * SequenceLoss total with the reference's expressions (point_matching_loss.py:62-103, 160-218, 263-291) in
    float64 torch; seq_r / seq_t: float64 tensors (requires_grad); nn[t][n]: the neighbours (constants), None = own."""
    T, N = len(seq_r), len(labels)
    if mode == PM_ROT:
        flags = 0
    D = lambda x: torch.from_numpy(a64(x))
    sdf, s = float(f32(sdf)), (torch.ones(N, dtype=torch.float64) if scale is None else D(scale))
    gt_r = D(gt_r)

    def scaled(tt):
        xy = tt[:, :2] * s[:, None] if flags & PM_SCALE_XY else tt[:, :2]
        z = tt[:, 2] * s * sdf if flags & PM_SCALE_DEPTH else tt[:, 2] * sdf
        return torch.cat([xy, z[:, None]], dim=1)
    norm = lambda x: torch.mean(torch.linalg.vector_norm(x, dim=-1, ord=loss_type))
    tg = scaled(D(gt_t)) if mode != PM_ROT else None
    total = 0.
    for t, w in enumerate(gamma_weights(gamma, T)):
        tp = scaled(seq_t[t]) if mode != PM_ROT else None
        loss = 0.
        for n in range(N):
            c = int(labels[n])
            P = D(verts[c])
            idx = None if nn is None or nn[t][n] is None else torch.from_numpy(np.asarray(nn[t][n], dtype=np.int64))
            rot_g, rot_p = P @ gt_r[n].T, P @ seq_r[t][n].T
            if mode == PM_ROT:
                tgt, pred = rot_g, rot_p
            else:
                tgt = rot_g + tg[n]
                pred = rot_p + (tg[n] if mode == PM_DISENTANGLE else tp[n])
            if idx is not None:
                pred = pred[idx]
            li = norm(pred - tgt)
            if mode == PM_DISENTANGLE:
                if flags & PM_DISENTANGLE_Z:
                    tz = torch.cat([tg[n][:2], tp[n][2:]])
                    txy = torch.cat([tp[n][:2], tg[n][2:]])
                    li = (norm((rot_g + tz) - tgt) + norm((rot_g + txy) - tgt)) + li
                else:
                    li = norm((rot_g + tp[n]) - tgt) + li
            loss = loss + li / float(f32(diameter[c]))
        if reduction == 'mean':
            loss = loss / N
        total = total + w * (float(f32(weight)) * loss)
    return float(f32(upstream)) * total


def pm_kwargs(opt):
    """an entry of PM_VARIANTS -> the keyword arguments of pm_ref / pm_grad_ref / torch_pm_total."""
    return dict(loss_type=opt.get('loss_type', 2), flags=opt.get('flags', 0), sdf=opt.get('sdf', 1.),
                reduction=opt.get('reduction', 'mean'), weight=opt.get('weight', 1.), gamma=opt.get('gamma', 0.8))


def case_args(case):
    return (case['verts'], case['labels'], None, case['diameter'], case['seq_r'], case['seq_t'], case['gt_r'], case['gt_t'])


def pm_grads_of(case, symmetric, mode, **kw):
    a = case_args(case)
    return pm_grad_ref(a[0], a[1], symmetric, *a[3:], scale=case['scale'], mode=mode, **kw)


@lru_cache(maxsize=None)
def pm_grad_gpu_case(counts, T, mode=PM_FULL, large=False, max_undecided=0):
    """`pm_gpu_case` extended to the gradients: the first seed below 64 whose neighbours are all decided AND whose L1
    components have at most `max_undecided` undecided signs under EVERY translation scaling the mode's variants use."""
    labels = H.PM_GPU_LARGE_LABELS if large else H.PM_GPU_LABELS
    variants = (H.PM_LARGE_VARIANTS if large else H.PM_VARIANTS)[mode]
    scalings = sorted({(v.get('flags', 0) & (PM_SCALE_XY | PM_SCALE_DEPTH | PM_DISENTANGLE_Z), v.get('sdf', 1.)) for v in variants})
    for seed in range(64):
        case = H.pm_case(list(counts), labels, T, seed=seed, layout='lattice' if large else 'cloud')
        worst = 0
        for flags, sdf in scalings:
            ref = pm_ref(case['verts'], labels, [False, True], case['diameter'], case['seq_r'], case['seq_t'], case['gt_r'],
                         case['gt_t'], scale=case['scale'], mode=mode, flags=flags, sdf=sdf, want_d=True)
            if not H.nn_gaps_ok(ref)[0]:
                break
            worst = max(worst, pm_grads_of(case, [False, True], mode, loss_type=1, flags=flags, sdf=sdf)['undecided'])
            if worst > max_undecided:
                break
        else:
            return seed, worst
    raise AssertionError(f'no seed below 64 for {counts}')


# ---------------------------------------------------------------------------------------- exact integer-lattice cases
H_RZ = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], dtype=np.float32)
H_RX = np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0]], dtype=np.float32)


def pm_exact_case(kind):
    """cases whose gradients are exact in every format: integer lattice vertices (64 = 2**6 of them), rotations with
    0 / +-1 entries, integer translations, power-of-two scales, diameters, weights, gamma and sample count.
    'l1': four samples of two classes (class 1 symmetric), predicted rotations that differ from the ground truth by a
    signed permutation, shifted translations; 'l2': the predicted rotation IS the ground truth's and the translation is
    off along one axis, so that every u = d / |d| is a signed unit vector; in both the LAST sample's pose equals the ground
    truth exactly (all zeros)."""
    r = np.arange(-2, 2)
    P = np.stack(np.meshgrid(r, r, r, indexing='ij'), -1).reshape(-1, 3).astype(np.float32)            # 64 points
    Q = (P[np.random.RandomState(1).permutation(64)] * [1, 2, 1] + [0, 1, 0]).astype(np.float32)        # another 64, shuffled
    RZ, RX = H_RZ, H_RX
    gt_r = np.stack([RZ, RX @ RZ, RX, np.eye(3, dtype=np.float32)]).astype(np.float32)
    gt_t = np.array([[3, -4, 704], [0, 8, 640], [-16, 2, 512], [5, 5, 768]], dtype=np.float32)
    labels = np.array([0, 1, 1, 0]) if kind == 'l1' else np.array([0, 0, 0, 1])
    if kind == 'l1':
        pred_r = np.stack([gt_r[0] @ RX, gt_r[1] @ RZ, gt_r[2], gt_r[3]]).astype(np.float32)
        pred_t = gt_t + np.array([[1, 0, -2], [0, 3, 8], [2, -1, 4], [0, 0, 0]], dtype=np.float32)
    else:
        pred_r = gt_r.copy()
        pred_t = gt_t + np.array([[4, 0, 0], [0, -2, 0], [0, 0, 16], [0, 0, 0]], dtype=np.float32)
    return dict(verts=[P, Q], labels=labels, gt_r=gt_r, gt_t=gt_t, seq_r=[pred_r, gt_r.copy()], seq_t=[pred_t, pred_t.copy()],
                scale=np.array([0.5, 2.0, 1.0, 4.0], dtype=np.float32), diameter=[64.0, 128.0])


EXACT_VARIANTS = {
    'l1': [(PM_FULL, dict(loss_type=1, gamma=0.5)), (PM_FULL, dict(loss_type=1, flags=PM_SCALE_XY | PM_SCALE_DEPTH, sdf=0.25, gamma=0.5)),
           (PM_DISENTANGLE, dict(loss_type=1, flags=PM_DISENTANGLE_Z, weight=2., gamma=0.5)),
           (PM_DISENTANGLE, dict(loss_type=1, flags=PM_SCALE_XY, reduction='sum', gamma=0.5)), (PM_ROT, dict(loss_type=1, gamma=0.5))],
    'l2': [(PM_FULL, dict(loss_type=2, gamma=0.5)), (PM_DISENTANGLE, dict(loss_type=2, flags=PM_DISENTANGLE_Z, gamma=0.5)),
           (PM_DISENTANGLE, dict(loss_type=2, flags=PM_SCALE_DEPTH, sdf=0.5, gamma=0.5)), (PM_ROT, dict(loss_type=2, gamma=0.5))],
}


# ------------------------------------------------------------------------------------------ fixture: loss_grads.npz
def grad_fixture_inputs():
    """`fixture_inputs` of test_loss_host.py with what only a gradient sees: a valid and an invalid pixel whose
    prediction EQUALS the ground truth (sgn(0) = 0), a mask cell equal to its target, and a fourth iteration in which the
    predicted pose of samples 0 (symmetric class) and 1 equals the ground truth exactly (|d| = 0 under both norms)."""
    px, pm = H.fixture_inputs()
    v, occ = pixel_decisions(px['gt'], px['valid'], 400.)
    flat_v = v.reshape(-1)
    hw = v.shape[1] * v.shape[2]
    for it, want in ((1, True), (2, False)):
        cell = int(np.nonzero(flat_v == want)[0][3])
        n, r = divmod(cell, hw)
        y, x = divmod(r, v.shape[2])
        px['flow_a'][it] = px['flow_a'][it].clone()
        px['flow_a'][it][n, :, y, x] = px['gt'][n, :, y, x]
    px['masks'][1] = px['masks'][1].clone()
    px['masks'][1][0, 0, :3] = torch.from_numpy(occ[0, 0, :3]).float()
    pm['seq_r'] = list(pm['seq_r']) + [pm['seq_r'][2].copy()]
    pm['seq_t'] = list(pm['seq_t']) + [pm['seq_t'][2].copy()]
    for n in (0, 1):
        pm['seq_r'][3][n] = pm['gt_r'][n]
        pm['seq_t'][3][n] = pm['gt_t'][n]
    return px, pm


@pytest.fixture(scope='module')
def fix():
    d = np.load(GOLDEN_FILE)
    px, pm = grad_fixture_inputs()
    return d, px, pm


def test_fixture_inputs_are_the_seeded_ones(fix):
    d, px, pm = fix
    assert np.array_equal(d['flow_a'], torch.stack(px['flow_a']).numpy()) and np.array_equal(d['masks'], torch.stack(px['masks']).numpy())
    assert np.array_equal(d['seq_r'], np.stack(pm['seq_r'])) and np.array_equal(d['seq_t'], np.stack(pm['seq_t']))
    assert json.loads(str(d['pm_options'])) == H.PM_OPTIONS and json.loads(str(d['pixel_options'])) == H.PIXEL_OPTIONS
    v, _ = pixel_decisions(px['gt'], px['valid'], 400.)
    eq = (px['flow_a'][1] == px['gt']).all(1).numpy()
    assert (eq & v).any() and ((px['flow_a'][2] == px['gt']).all(1).numpy() & ~v).any()
    assert np.array_equal(pm['seq_r'][3][0], pm['gt_r'][0]) and np.array_equal(pm['seq_t'][3][1], pm['gt_t'][1])


def pixel_grad_ref_for(opt, px, gt_occ=None, **kw):
    valid = px['valid'] if opt['valid'] else None
    if opt['cls'] == 'RAFTLoss':
        r = pixel_grad_ref(px['gt'], valid, flows=[px['flow_a']], max_flow=opt['max_flow'], weights=(opt['loss_weight'], 1, 1),
                           gammas=(opt['gamma'],) * 3, **kw)
    else:
        r = pixel_grad_ref(None, None, masks=px['masks'], mask_gt=gt_occ, weights=(1, 1, opt['loss_weight']),
                           gammas=(opt['gamma'],) * 3, **kw)
    return r['grads'][0], r['coef'][0]


def pm_grad_ref_for(opt, pm, symmetric, gamma=0.8, **kw):
    return pm_grad_ref(pm['verts'], pm['labels'], symmetric, pm['diameter'], pm['seq_r'], pm['seq_t'], pm['gt_r'], pm['gt_t'],
                       scale=pm['scale'], mode=H.PM_MODES[opt['cls']], loss_type=int(opt['loss_type'][-1]), flags=H.pm_flags(opt),
                       sdf=opt.get('scale_depth_factor', 1.), reduction=opt.get('reduction', 'mean'),
                       weight=opt.get('loss_weight', 1.), gamma=gamma, **kw)


def gt_occ_of(px):
    return (px['gt'][:, 0] + px['gt'][:, 1] < 400.).float()


# ------------------------------------------------------------------- 1. the closed forms are autograd's, in float64
def _rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max() / max(float(np.abs(want).max()), 1e-300))


def test_pixel_closed_forms_are_autograd_in_float64(fix):
    _, px, _ = fix
    lead = lambda seq: [t.double().requires_grad_() for t in seq]
    fa, fb, mk = lead(px['flow_a']), lead(px['flow_b']), lead(px['masks'])
    kw = dict(max_flow=400., weights=(.1, 2.5, 10.), eps=(1e-10, 1e-6), gammas=(0.8, 0.5, 0.9), upstream=(1., 0.25, 3.))
    torch_pixel_total(px['gt'], px['valid'], flows=[fa, fb], masks=mk, **kw).backward()
    ref = pixel_grad_ref(px['gt'], px['valid'], flows=[px['flow_a'], px['flow_b']], masks=px['masks'], **kw)
    worst = max(_rel(t.grad.numpy(), r.v) for seq, row in zip((fa, fb, mk), ref['grads']) for t, r in zip(seq, row))
    measured('pixel gradients: float64 autograd vs closed form, relative', worst)
    assert worst <= 1e-12


@pytest.mark.parametrize('i', range(len(H.PM_OPTIONS)))
def test_point_matching_closed_forms_are_autograd_in_float64(fix, i):
    _, _, pm = fix
    opt = H.PM_OPTIONS[i]
    ref = pm_grad_ref_for(opt, pm, [False, True], upstream=0.5)
    free = H.pm_ref_for(opt, pm, [False, True])
    sr = [torch.from_numpy(a64(r)).requires_grad_() for r in pm['seq_r']]
    st = [torch.from_numpy(a64(t)).requires_grad_() for t in pm['seq_t']]
    mode = H.PM_MODES[opt['cls']]
    torch_pm_total(pm['verts'], pm['labels'], None, pm['diameter'], sr, st, pm['gt_r'], pm['gt_t'], scale=pm['scale'], mode=mode,
                   loss_type=int(opt['loss_type'][-1]), flags=H.pm_flags(opt), sdf=opt.get('scale_depth_factor', 1.),
                   reduction=opt.get('reduction', 'mean'), weight=opt.get('loss_weight', 1.), nn=free['nn'], upstream=0.5).backward()
    worst = max(_rel(t.grad.numpy(), r.v) for t, r in zip(sr, ref['grad_r']))
    if mode != PM_ROT:
        worst = max([worst] + [_rel(t.grad.numpy(), r.v) for t, r in zip(st, ref['grad_t'])])
        assert not st[3].grad[:2].any()                                         # pose == ground truth: zero, not NaN
    assert not sr[3].grad[:2].any() and ref['undecided'] == 0
    measured(f'point-matching gradients, option {i}: float64 autograd vs closed form, relative', worst)
    assert worst <= 1e-12


# ------------------------------------------------------------------- 2. the reference's fp32 gradients fall inside
def test_reference_pixel_gradients_fall_inside_the_bounds(fix):
    d, px, _ = fix
    worst = 0.0
    for i, opt in enumerate(H.PIXEL_OPTIONS):
        grads, _ = pixel_grad_ref_for(opt, px, gt_occ_of(px))
        for t, g in enumerate(grads):
            worst = max(worst, grad_ratio(d[f'pixel_{i}_grad'][t].reshape(g.v.shape), g))
    measured('reference pixel gradients / coefficient bound', worst)
    assert worst <= 1.0


def test_reference_point_matching_gradients_fall_inside_the_bounds(fix):
    d, _, pm = fix
    worst = 0.0
    for i, opt in enumerate(H.PM_OPTIONS):
        ref = pm_grad_ref_for(opt, pm, [False, True], torch_sums=True, nn_idx=d[f'pm_{i}_nn'])    # at ITS neighbours
        for t in range(4):
            worst = max(worst, grad_ratio(d[f'pm_{i}_grad_r'][t], ref['grad_r'][t]))
            if ref['grad_t'] is not None:
                worst = max(worst, grad_ratio(d[f'pm_{i}_grad_t'][t], ref['grad_t'][t]))
        assert not d[f'pm_{i}_grad_r'][3][:2].any()                             # autograd: |d| = 0 gives 0 under both norms
    measured('reference point-matching gradients / (kernel bound + torch summation and chain terms)', worst)
    assert worst <= 1.0


def test_bounds_are_a_handful_of_u(fix):
    """the derived constants, written down: the coefficient of a pixel gradient carries FOUR roundings; a point-matching
    gradient on the fixture is bounded by the cancellation in d (coordinates ~800 mm, differences ~10 mm)."""
    _, px, pm = fix
    _, coef = pixel_grad_ref_for(H.PIXEL_OPTIONS[0], px)
    rel = max(float(c.e / abs(c.v)) for c in coef) / U
    measured('pixel gradient coefficient bound / U', rel)
    assert 3.9 <= rel <= 4.1
    _, coef = pixel_grad_ref_for(H.PIXEL_OPTIONS[3], px, gt_occ_of(px))
    relm = max(float(c.e / abs(c.v)) for c in coef) / U
    measured('mask gradient coefficient bound / U', relm)
    assert 3.9 <= relm <= 4.1
    ref = pm_grad_ref_for(H.PM_OPTIONS[0], pm, [False, True])
    g = ref['grad_r'][0]
    relp = float(g.e.max() / np.abs(g.v).max()) / U
    measured('point-matching grad_R bound / U of the largest entry (fixture, l2)', relp)
    assert relp < 5000


# ------------------------------------------------------------------- 3. planted defects fall outside
@pytest.mark.parametrize('defect,opt', [('sgn0_is_1', 0), ('gamma_reversed', 0), ('gamma_reversed', 4), ('through_count', 2),
                                        ('valid_on_mask', 3)])
def test_planted_pixel_defects_fall_outside(fix, defect, opt):
    _, px, _ = fix
    occ = gt_occ_of(px)
    good, _ = pixel_grad_ref_for(H.PIXEL_OPTIONS[opt], px, occ)
    if defect == 'valid_on_mask':
        bad = pixel_grad_ref(px['gt'], px['valid'], masks=px['masks'], mask_gt=occ, weights=(1, 1, 10.), defect=defect)['grads'][0]
    else:
        bad, _ = pixel_grad_ref_for(H.PIXEL_OPTIONS[opt], px, occ, defect=defect)
    r = max(grad_ratio(b.v, g) for b, g in zip(bad, good))
    measured(f'planted {defect}: error / bound', r)
    assert r > 10.0


@pytest.mark.parametrize('defect,opt', [('own_point', 1), ('unscaled_t', 4), ('sum_for_mean', 0), ('nan_at_zero', 0),
                                        ('rot_leak', 6), ('rot_leak', 7), ('gamma_reversed', 1)])
def test_planted_point_matching_defects_fall_outside(fix, defect, opt):
    _, _, pm = fix
    good = pm_grad_ref_for(H.PM_OPTIONS[opt], pm, [False, True])
    bad = pm_grad_ref_for(H.PM_OPTIONS[opt], pm, [False, True], defect=defect)
    key = 'grad_t' if defect in ('unscaled_t', 'rot_leak') else 'grad_r'
    r = max(grad_ratio(b.v, g) for b, g in zip(bad[key], good[key]))
    measured(f'planted {defect}: error / bound', r)
    assert r > 10.0


# ------------------------------------------------------------------- 4. the inputs of the GPU tests
@pytest.mark.parametrize('mode', [PM_FULL, PM_DISENTANGLE, PM_ROT])
@pytest.mark.parametrize('counts', H.PM_GPU_COUNTS)
def test_gpu_vertex_sets_decide_every_sign(counts, mode):
    for T in (1, 3):
        seed, und = pm_grad_gpu_case(counts, T, mode)
        assert und == 0, (counts, T, mode, seed)


def test_gpu_vertex_sets_beyond_one_tile_leave_few_signs_open():
    for mode in H.PM_LARGE_VARIANTS:
        seed, und = pm_grad_gpu_case((1023, 1025), 1, mode, True, 4)
        measured(f'V = (1023, 1025), mode {mode}: seed {seed}, undecided L1 components', und)
        assert und <= 4


@pytest.mark.parametrize('kind', ['l1', 'l2'])
def test_exact_lattice_cases_are_exact(kind):
    """every gradient of the exact cases is a float64 number with a short mantissa: rounding it to fp32 changes nothing,
    the pose that equals the ground truth gives zeros, and float64 autograd agrees to the last bit."""
    case = pm_exact_case(kind)
    for mode, opt in EXACT_VARIANTS[kind]:
        ref = pm_grads_of(case, [False, True], mode, **opt)
        free = pm_ref(*case_args(case)[:2], [False, True], *case_args(case)[3:], scale=case['scale'], mode=mode,
                      loss_type=opt['loss_type'], flags=opt.get('flags', 0), sdf=opt.get('sdf', 1.))
        sr = [torch.from_numpy(a64(r)).requires_grad_() for r in case['seq_r']]
        st = [torch.from_numpy(a64(t)).requires_grad_() for t in case['seq_t']]
        torch_pm_total(case['verts'], case['labels'], None, case['diameter'], sr, st, case['gt_r'], case['gt_t'], scale=case['scale'],
                       mode=mode, nn=free['nn'], **opt).backward()
        for t in range(2):
            g = ref['grad_r'][t].v
            assert np.array_equal(g.astype(np.float32).astype(np.float64), g) and np.array_equal(sr[t].grad.numpy(), g)
            assert not g[3].any()
            if mode != PM_ROT:
                gt = ref['grad_t'][t].v
                assert np.array_equal(gt.astype(np.float32).astype(np.float64), gt) and np.array_equal(st[t].grad.numpy(), gt)
                assert not gt[3].any()
        # 'l2' keeps the ground-truth rotation: without a translation the prediction IS the ground truth, all zeros
        assert (kind == 'l2' and mode == PM_ROT) or any(g.v.any() for g in ref['grad_r'] + (ref['grad_t'] or []))


# ================================================================================================== loss() wiring
def torch_wiring_total(kind, seqs, gt_flow, valid, cfgs, max_flow=400., pose=None):
    """`wiring_ref`'s loss (loss_pose + loss_flow + loss_mask, or the RAFT refiners' sums) in float64 torch on sequences
    that require a gradient -- same argument conventions as `H.wiring_ref`."""
    fcfg = lambda c: (c['loss_func_cfg'], c.get('gamma', 0.8))
    if kind == 'flow':
        lf, g = fcfg(cfgs['loss_cfg'])
        return torch_pixel_total(gt_flow, valid, flows=[seqs[0]], max_flow=lf.get('max_flow', 400), weights=(lf.get('loss_weight', 1.), 1, 1),
                                 eps=(lf.get('eps', 1e-10),) * 2, gammas=(g,) * 3)
    if kind == 'flow_mask':
        (lf, gf), (lm, gm) = fcfg(cfgs['flow_loss_cfg']), fcfg(cfgs['occlusion_loss_cfg'])
        return torch_pixel_total(gt_flow, valid, flows=[seqs[0]], masks=seqs[1], max_flow=max_flow,
                                 weights=(lf.get('loss_weight', 1.), 1, lm.get('loss_weight', 1.)), eps=(lf.get('eps', 1e-10),) * 2,
                                 gammas=(gf, 1, gm))
    flow_from_pose, flow_from_pred, rots, trans, masks = seqs
    (lf, gf), (lm, gm), (lp, gp) = fcfg(cfgs['flow_loss_cfg']), fcfg(cfgs['mask_loss_cfg']), fcfg(cfgs['pose_loss_cfg'])
    total = torch_pixel_total(gt_flow, valid, flows=[flow_from_pred], masks=masks, max_flow=max_flow,
                              weights=(lf.get('loss_weight', 1.), 1, lm.get('loss_weight', 1.)), eps=(lf.get('eps', 1e-10),) * 2,
                              gammas=(gf, 1, gm))
    if lp['type'] == 'RAFTLoss':
        return total + torch_pixel_total(gt_flow, valid, flows=[flow_from_pose], max_flow=lp.get('max_flow', 400),
                                         weights=(lp.get('loss_weight', 1.), 1, 1), eps=(lp.get('eps', 1e-10),) * 2, gammas=(gp,) * 3)
    opt = dict(lp, cls=lp['type'])
    return total + torch_pm_total(pose['verts'], pose['labels'], None, pose['diameter'], rots, trans, pose['gt_r'], pose['gt_t'],
                                  scale=pose.get('scale'), mode=H.PM_MODES[lp['type']], loss_type=int(lp.get('loss_type', 'l2')[-1]),
                                  flags=H.pm_flags(opt), sdf=lp.get('scale_depth_factor', 1.), reduction=lp.get('reduction', 'mean'),
                                  weight=lp.get('loss_weight', 1.), gamma=gp, nn=pose.get('nn'))
