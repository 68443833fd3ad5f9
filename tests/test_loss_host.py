"""CPU: the supervised loss values of scflow_amd/losses.py and loss.hip -- SequenceLoss over RAFTLoss / L1Loss (the pixel
kernel) and the three point-matching losses -- restated in float64 with a bound on any fp32 evaluation in the kernels'
operation order; the `loss()` wiring of the refiners restated on top of them; the inputs tests/test_gpu_loss.py feeds the
kernels; and the proof that the bounds are neither unreachable (the reference's own fp32 values, tests/golden/losses.npz,
fall inside) nor vacuous (planted defects fall outside).

Bounds are built from U = 2**-24 with the `EV` running-error class of test_stream_ops_host.py: every fp32 operation of
the kernel source is replayed once on float64 values and adds U |result| to the errors it propagates.

Pixel losses, per sequence and iteration (loss.hip, seq_pixel_*):
    each |p - g| is ONE fp32 rounding (the subtraction; abs and the product with v in {0, 1} are exact)   U * sum
    the fp64 accumulation of n terms                                                              n * 2**-53 * sum
    (float)sum                                                                                               1 U
    (float)count is exact below 2**24; + eps                                                                 1 U
    the division, the product with loss_weight                                                               2 U
  i.e. about 5 U relative to the value; the gamma total adds one product and one addition per iteration.
Point matching: every coordinate R p + t carries the roundings of three products and three additions -- c U (sum |r||p| +
|t|) with c <= 4 -- propagated through the difference, the norm, the fp64 sum, its conversion, the division by V, the
sum of the terms, the division by the diameter, the fp32 sum over the samples and the weight.

The comparison with the REFERENCE's fp32 values needs more room than the kernel does: torch sums n fp32 terms in an
order of its own, which costs up to (n - 1) U sum|x| whatever the order.  `torch_sum_term` is that term; it is added
for the fixture comparison only and never to the bound the kernels are held to.
"""
import json
import math
import os
from collections import OrderedDict
from functools import lru_cache

import numpy as np
import pytest
import torch

import oracle
from test_stream_ops_host import EV, U, ev_matvec, measured

f32 = np.float32
PM_FULL, PM_DISENTANGLE, PM_ROT = 0, 1, 2
PM_DISENTANGLE_Z, PM_SCALE_XY, PM_SCALE_DEPTH = 1, 2, 4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def a64(x):
    return (x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)).astype(np.float64)


def a32(x):
    return (x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)).astype(np.float32)


def rnd(x):
    """one more fp32 rounding of an EV (a conversion, or an operation whose exact result is x.v)."""
    return EV._rnd(x.v, x.e)


def ratio(got, ev):
    """|got - ev.v| / ev.e, elementwise worst; a zero bound demands equality."""
    got, v, e = np.asarray(got, dtype=np.float64), np.asarray(ev.v), np.asarray(ev.e)
    err = np.abs(got - v)
    with np.errstate(all='ignore'):
        r = np.where(err == 0, 0.0, err / e)
    r = np.where(np.isnan(r), np.inf, r)
    return float(np.max(r)) if r.size else 0.0


def torch_sum_term(n, abs_sum):
    """any order of n - 1 fp32 additions: (n - 1) U sum|x| (first order)."""
    return max(n - 1, 0) * U * abs_sum


def gamma_weights(gamma, T, reverse=False):
    """(float)(gamma ** (T - 1 - i)): the Python float the reference multiplies an fp32 tensor with."""
    e = [T - 1 - i for i in range(T)]
    if reverse:
        e = e[::-1]
    return [float(f32(float(gamma) ** k)) for k in e]


def gamma_total(values, gamma, reverse=False):
    """loss = 0.; loss += w_i * l_i in ascending i, on EV values."""
    total = None
    for w, v in zip(gamma_weights(gamma, len(values), reverse), values):
        term = EV(w) * v
        total = term if total is None else total + term           # 0. + x is exact
    return total


def fp32_recombine(values32, gamma):
    """the same in fp32 on the RETURNED per-iteration values: what the combine kernels must reproduce bit for bit."""
    total = f32(0.0)
    for w, v in zip(gamma_weights(gamma, len(values32)), values32):
        total = f32(total + f32(f32(w) * f32(v)))
    return total


# ================================================================================================== pixel losses
def pixel_decisions(gt, valid, max_flow, defect=None):
    """the fp32 decisions, operation by operation (numpy float32 arithmetic rounds every operation): v and occ."""
    gx, gy = a32(gt[:, 0]), a32(gt[:, 1])
    mf = f32(max_flow)
    mag = np.sqrt(gx * gx + gy * gy)
    v = (mag <= mf) if defect == 'mag_le' else (mag < mf)
    if valid is not None:
        vv = a32(valid)
        v = v & ((vv > f32(0.5)) if defect == 'valid_gt' else (vv >= f32(0.5)))
    occ = (mag < mf) if defect == 'occ_magnitude' else ((gx + gy) < mf)
    return v, occ.astype(np.float64)


def pixel_ref(gt, valid, flows=(), masks=None, max_flow=400., weights=(1., 1., 1.), eps=(1e-10, 1e-10), gammas=(.8, .8, .8),
              mask_gt=None, defect=None, torch_sums=False):
    """-> dict(per_iter=[[EV] per flow sequence] + [[EV] mask], totals=[EV]) in the kernel's row order (flow_a, flow_b,
    mask).  torch_sums widens every value by torch's own fp32 summation (fixture comparison only)."""
    n = int(np.prod(a64(gt).shape)) // 2 if gt is not None else int(np.prod(a64(mask_gt).shape))
    out = dict(per_iter=[], totals=[])
    if gt is not None:
        v, occ = pixel_decisions(gt, valid, max_flow, defect)
        g = a64(gt)
        cnt = float(v.sum())
    if mask_gt is not None:
        occ = a64(mask_gt)
    for s, seq in enumerate(flows):
        vals = []
        for p in seq:
            d = np.abs(a64(p) - g)
            with np.errstate(invalid='ignore'):
                S = float((np.where(v[:, None], d, d * 0.0)).sum())             # NaN * 0 = NaN, like valid[:, None] * loss
            e = U * S + 2 * n * 2.0 ** -53 * S
            if torch_sums:
                e += torch_sum_term(2 * n, S)                                  # the count is a sum of 0/1: exact below 2**24
            den = EV(cnt) + EV(float(f32(eps[s])))
            vals.append(EV(float(f32(weights[s]))) * (rnd(EV(S, e)) / den))
        out['per_iter'].append(vals)
        out['totals'].append(gamma_total(vals, gammas[s], reverse=(defect == 'gamma_reversed')))
    if masks is not None:
        vals = []
        for m in masks:
            m = a64(m).reshape(occ.shape)
            S = float(np.abs(m - occ).sum())
            e = U * S + n * 2.0 ** -53 * S
            if torch_sums:
                e += torch_sum_term(n, S)
            den = EV(cnt) if defect == 'mask_by_count' else rnd(EV(float(n)))
            vals.append((rnd(EV(S, e)) / den) * EV(float(f32(weights[2]))))
        out['per_iter'].append(vals)
        out['totals'].append(gamma_total(vals, gammas[2], reverse=(defect == 'gamma_reversed')))
    return out


def find_boundary_cells(max_flow=400., want=24, seed=0):
    """(gx, gy) fp32 pairs whose magnitude straddles max_flow by one ulp: the separately rounded sqrt(gx*gx + gy*gy)
    and the evaluation with gx*gx contracted into an fma fall on different sides of `< max_flow`."""
    rng = np.random.RandomState(seed)
    mf = f32(max_flow)
    found = []
    while len(found) < want:
        th = rng.uniform(0.05, math.pi / 2 - 0.05, size=4096)
        gx = (max_flow * np.cos(th)).astype(f32)
        gy0 = np.sqrt(np.float64(max_flow) ** 2 - gx.astype(np.float64) ** 2).astype(f32)
        for k in range(-3, 4):
            gy = gy0
            for _ in range(abs(k)):
                gy = np.nextafter(gy, f32(np.inf if k > 0 else -np.inf))
            sep = np.sqrt(gx * gx + gy * gy)                                    # mul, mul, add, sqrt: four roundings
            yy = (gy * gy).astype(np.float64)
            fma = np.sqrt((gx.astype(np.float64) ** 2 + yy).astype(f32))        # fma(gx, gx, fl(gy*gy)): gx*gx exact in fp64
            pick = (sep < mf) != (fma < mf)
            for i in np.nonzero(pick)[0]:
                found.append((float(gx[i]), float(gy[i]), bool(sep[i] < mf)))
    return found[:want]


def pixel_case(shape, T, regime='nominal', seed=0, max_flow=400.):
    """inputs of one pixel-kernel launch: dict(gt, valid, flow_a, flow_b, masks) of CPU fp32 tensors."""
    n, h, w = shape
    g = torch.Generator().manual_seed(1000 + seed + 7 * n * h * w + T)
    R = lambda *s: torch.randn(s, generator=g)
    gt = R(n, 2, h, w) * 6
    valid = (torch.rand((n, h, w), generator=g) > 0.3).float()
    flat = gt.permute(0, 2, 3, 1).reshape(-1, 2)                               # a copy, written back below
    vflat = valid.reshape(-1).clone()
    P = flat.shape[0]
    if regime == 'nominal':
        bg = torch.rand((P,), generator=g) < 0.25                               # the 400-background of a filtered ground truth
        flat[bg] = max_flow
    elif regime == 'boundary':
        cells = find_boundary_cells(max_flow, want=min(24, max(P - 1, 1)))
        for i, (x, y, _) in enumerate(cells[:P]):
            flat[i] = torch.tensor([x, y])
            vflat[i] = 1.
        for i, xy in enumerate([(400., 0.), (240., 320.), (300., 200.), (-500., 100.), (0., 400.)]):
            if len(cells) + i < P:
                flat[len(cells) + i] = torch.tensor(xy)                         # mag == max_flow exactly; the quirk cells
                vflat[len(cells) + i] = 1.
    elif regime == 'valid_half':
        vflat[::2] = 0.5
        vflat[1::4] = float(np.nextafter(f32(0.5), f32(0)))
    elif regime == 'all_invalid':
        vflat[:] = 0.
    elif regime == 'all_background':
        flat[:] = max_flow
    gt = flat.reshape(n, h, w, 2).permute(0, 3, 1, 2).contiguous()
    valid = vflat.reshape(n, h, w)
    mk = lambda: [gt + R(n, 2, h, w) * 2 for _ in range(T)]
    flow_a, flow_b = mk(), mk()
    for t in range(T):                                                          # background predictions are 0-ish, not 400
        flow_a[t] = torch.where(gt == max_flow, R(n, 2, h, w), flow_a[t])
    masks = [torch.rand((n, h, w), generator=g) for _ in range(T)]
    return dict(gt=gt, valid=valid, flow_a=flow_a, flow_b=flow_b, masks=masks)


# ================================================================================================== point matching
def _scaled_t(t, s, flags, sdf):
    """the reference's scaled translation of every sample: list of three EV (N,)."""
    t = a64(t)
    sdf = float(f32(sdf))
    if s is None:
        s = np.ones(len(t))
    s = EV(a64(s))
    x = EV(t[:, 0]) * s if flags & PM_SCALE_XY else EV(t[:, 0])
    y = EV(t[:, 1]) * s if flags & PM_SCALE_XY else EV(t[:, 1])
    z = (EV(t[:, 2]) * s) * EV(sdf) if flags & PM_SCALE_DEPTH else EV(t[:, 2]) * EV(sdf)
    return [x, y, z]


def _pick(ev, i):
    return EV(ev.v[i], ev.e[i])


def _norm(d, loss_type):
    if loss_type == 1:
        a = [EV(np.abs(c.v), c.e) for c in d]
        return (a[0] + a[1]) + a[2]
    return ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]).sqrt()


def _mean(norms, torch_sums=False):
    V = norms.v.shape[0]
    S, e = float(norms.v.sum()), float(norms.e.sum())
    e += V * 2.0 ** -53 * S
    if torch_sums:
        e += torch_sum_term(V, S)
    return rnd(EV(S, e)) / EV(float(V))


def pm_ref(verts, labels, symmetric, diameter, seq_r, seq_t, gt_r, gt_t, scale=None, mode=PM_FULL, loss_type=2, flags=0,
           sdf=1., reduction='mean', weight=1., gamma=.8, nn_idx=None, defect=None, torch_sums=False, want_d=False):
    """float64 restatement of scf_point_matching_loss with running error bounds.  verts: list of (V,3) per class;
    symmetric: list of bool per class.  nn_idx (T,N,>=V): evaluate at these neighbours instead of the fp64 argmin.
    -> dict(loss_i [[EV]], per_iter [EV], total EV, nn [[idx array or None]], dist [[EV (V,V) or None]])."""
    T, N = len(seq_r), len(labels)
    labels = [int(x) for x in labels]
    if mode == PM_ROT:
        flags = 0
    tg = _scaled_t(gt_t, scale, flags, sdf) if mode != PM_ROT else None
    out = dict(loss_i=[], per_iter=[], nn=[], dist=[])
    for t in range(T):
        tp = _scaled_t(seq_t[t], scale, flags, sdf) if mode != PM_ROT else None
        row, nn_row, d_row = [], [], []
        for n in range(N):
            c = labels[n]
            P = a64(verts[c])
            pv = [EV(P[:, 0]), EV(P[:, 1]), EV(P[:, 2])]
            rp, rg = a64(seq_r[t])[n], a64(gt_r)[n]
            gr = ev_matvec(rg, pv)
            pr = ev_matvec(rp, pv)
            if mode == PM_ROT:
                tgt, pred = gr, pr
            else:
                tgn, tpn = [_pick(x, n) for x in tg], [_pick(x, n) for x in tp]
                tgt = [gr[i] + tgn[i] for i in range(3)]
                add = tgn if mode == PM_DISENTANGLE else tpn
                pred = [pr[i] + add[i] for i in range(3)]
            idx, D = None, None
            if symmetric[c]:
                dd = [EV(pred[i].v[None, :], pred[i].e[None, :]) - EV(tgt[i].v[:, None], tgt[i].e[:, None]) for i in range(3)]
                D = (dd[0] * dd[0] + dd[1] * dd[1]) + dd[2] * dd[2]
                if nn_idx is not None:
                    idx = np.asarray(nn_idx[t][n][:len(P)], dtype=np.int64)
                elif defect == 'l1_nearest' and loss_type == 1:
                    idx = np.argmin(np.abs(dd[0].v) + np.abs(dd[1].v) + np.abs(dd[2].v), axis=1)
                else:
                    idx = np.argmin(D.v, axis=1)                                # lowest index on exact ties
                pred = [_pick(x, idx) for x in pred]
            val = _mean(_norm([pred[i] - tgt[i] for i in range(3)], loss_type), torch_sums)
            if mode == PM_DISENTANGLE:
                def term(tt):
                    return _mean(_norm([(gr[i] + tt[i]) - tgt[i] for i in range(3)], loss_type), torch_sums)
                if flags & PM_DISENTANGLE_Z:
                    tr = term([tgn[0], tgn[1], tpn[2]]) + term([tpn[0], tpn[1], tgn[2]])
                else:
                    tr = term(tpn)
                val = tr + val
            row.append(val / EV(float(f32(diameter[c]))))
            nn_row.append(idx)
            d_row.append(D if want_d else None)
        out['loss_i'].append(row)
        out['nn'].append(nn_row)
        out['dist'].append(d_row)
        s = row[0]
        for v in row[1:]:
            s = s + v
        if (reduction == 'mean') != (defect == 'mean_for_sum'):
            s = s / EV(float(N))
        out['per_iter'].append(EV(float(f32(weight))) * s)
    out['total'] = gamma_total(out['per_iter'], gamma, reverse=(defect == 'gamma_reversed'))
    return out


def rand_rot(rng, angle):
    ax = rng.randn(3)
    ax /= np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return (np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * K @ K).astype(f32)


def lattice_cloud(rng, v, spacing=10.0, jitter=1.5):
    """v points of a jittered cubic lattice in shuffled order: neighbours are a lattice step apart, so the nearest point
    of a slightly moved copy is decided by a wide margin whatever v is."""
    side = int(math.ceil(v ** (1.0 / 3.0)))
    r = (np.arange(side) - (side - 1) / 2.0) * spacing
    pts = np.stack(np.meshgrid(r, r, r, indexing='ij'), -1).reshape(-1, 3)
    pts = pts[rng.permutation(len(pts))[:v]] + rng.uniform(-jitter, jitter, size=(v, 3))
    return pts.astype(f32)


def pm_case(counts, labels, T, seed=0, angle=0.5, layout='cloud'):
    """class meshes (mm), poses ~800 mm away and T predicted poses per sample -> dict of fp32 arrays.  layout 'cloud':
    Gaussian vertex clouds and predictions `angle` away.  layout 'lattice' (vertex sets beyond one tile of the kernel):
    jittered lattices, a prediction 0.02 rad away and shifted by about one lattice step along the model's x axis, so
    that most points find a neighbour that is not themselves."""
    rng = np.random.RandomState(seed)
    N = len(labels)
    lat = layout == 'lattice'
    verts = [lattice_cloud(rng, v) if lat else (rng.randn(v, 3) * 40).astype(f32) for v in counts]
    gt_r = np.stack([rand_rot(rng, rng.uniform(0, 3)) for _ in range(N)])
    gt_t = (np.array([0, 0, 800.]) + rng.randn(N, 3) * [20, 20, 60]).astype(f32)
    if lat:
        angle = 0.02
    seq_r = [np.stack([rand_rot(rng, angle / (t + 1)) @ gt_r[n] for n in range(N)]).astype(f32) for t in range(T)]
    seq_t = [(gt_t + rng.randn(N, 3) * [4, 4, 20] / (t + 1)).astype(f32) for t in range(T)]
    if lat:
        seq_t = [(gt_t + gt_r[:, :, 0] * 10.3 + rng.randn(N, 3) * 0.3).astype(f32) for t in range(T)]
    scale = rng.uniform(0.5, 2.0, size=N).astype(f32)
    diameter = [float(f32(80 + 17.3 * c)) for c in range(len(counts))]
    return dict(verts=verts, labels=np.asarray(labels, dtype=np.int64), gt_r=gt_r, gt_t=gt_t, seq_r=seq_r, seq_t=seq_t,
                scale=scale, diameter=diameter)


def nn_gaps_ok(ref):
    """every symmetric target: the fp64 nearest candidate beats EVERY other by more than the two fp32 distance slacks
    (so any fp32 evaluation inside the bound picks it), and in particular the gap to the second nearest exceeds twice
    the slack.  -> (ok, smallest margin ratio)."""
    worst = np.inf
    for row in ref['dist']:
        for D in row:
            if D is None or D.v.shape[1] < 2:
                continue
            i = np.argmin(D.v, axis=1)
            r = np.arange(len(i))
            gap = D.v - D.v[r, i][:, None]
            need = D.e + D.e[r, i][:, None]
            gap[r, i] = np.inf
            second = np.argmin(gap, axis=1)
            worst = min(worst, float((gap / need).min()),
                        float((gap[r, second] / (2 * np.maximum(D.e[r, second], D.e[r, i]))).min()))
    return worst > 1.0, worst


PM_GPU_COUNTS = [(1, 63), (64, 65), (255, 256), (257, 600)]
# beyond one tile / LDS chunk of the kernel (1024 points): two blocks per sample and two chunks, a class that ends one
# point into the second tile next to one that ends one point before it; three tiles and chunks next to a class that
# fits one (its blocks of the later tiles return early)
PM_GPU_LARGE = [(1023, 1025), (600, 2500)]
PM_GPU_LABELS, PM_GPU_LARGE_LABELS = (1, 0, 1, 1, 0), (1, 0, 1)
# the option sets the GPU test runs per mode (arguments of pm_ref / of the launch)
PM_VARIANTS = {
    PM_FULL: [dict(loss_type=2), dict(loss_type=1, reduction='sum'), dict(loss_type=2, flags=PM_SCALE_XY),
              dict(loss_type=1, flags=PM_SCALE_DEPTH, sdf=0.25),
              dict(loss_type=2, flags=PM_SCALE_XY | PM_SCALE_DEPTH, sdf=2.0, reduction='sum')],
    PM_DISENTANGLE: [dict(loss_type=1, flags=PM_DISENTANGLE_Z, weight=10.), dict(loss_type=2, flags=PM_DISENTANGLE_Z),
                     dict(loss_type=1), dict(loss_type=2, flags=PM_SCALE_XY | PM_SCALE_DEPTH, sdf=0.5, reduction='sum')],
    PM_ROT: [dict(loss_type=2), dict(loss_type=1, reduction='sum', weight=3.)],
}
PM_LARGE_VARIANTS = {PM_FULL: [dict(loss_type=2), dict(loss_type=1, flags=PM_SCALE_XY, reduction='sum')],
                     PM_DISENTANGLE: [dict(loss_type=1, flags=PM_DISENTANGLE_Z, weight=10.)]}


@lru_cache(maxsize=None)
def pm_gpu_case(counts, T, mode=PM_FULL, large=False):
    """the gap-checked case of the GPU test for two classes of `counts` vertices (class 1 symmetric, labels mixed and
    repeated): the first seed whose nearest neighbours are all decided under EVERY translation scaling the mode's option
    sets use (the scaled translations move the compared points, so each scaling is checked on its own)."""
    labels = PM_GPU_LARGE_LABELS if large else PM_GPU_LABELS
    variants = (PM_LARGE_VARIANTS if large else PM_VARIANTS)[mode]
    scalings = sorted({(v.get('flags', 0) & (PM_SCALE_XY | PM_SCALE_DEPTH), v.get('sdf', 1.)) for v in variants})
    for seed in range(64):
        case = pm_case(list(counts), labels, T, seed=seed, layout='lattice' if large else 'cloud')
        margin = np.inf
        for flags, sdf in scalings:
            ref = pm_ref(case['verts'], labels, [False, True], case['diameter'], case['seq_r'], case['seq_t'], case['gt_r'],
                         case['gt_t'], scale=case['scale'], mode=mode, flags=flags, sdf=sdf, want_d=True)
            ok, m = nn_gaps_ok(ref)
            margin = min(margin, m)
            if not ok:
                break
        else:
            return seed, margin
    raise AssertionError(f'no seed below 64 decides every neighbour for {counts}')


# ---------------------------------------------------------------------------------------------- fixture: losses.npz
PM_OPTIONS = [
    dict(cls='PointMatchingLoss', loss_type='l2'),
    dict(cls='PointMatchingLoss', loss_type='l1', reduction='sum'),
    dict(cls='PointMatchingLoss', loss_type='l2', scale_xy=True),
    dict(cls='PointMatchingLoss', loss_type='l1', scale_depth=True, scale_depth_factor=0.25),
    dict(cls='PointMatchingLoss', loss_type='l2', scale_xy=True, scale_depth=True, scale_depth_factor=2.0, reduction='sum'),
    dict(cls='DisentanglePointMatchingLoss', loss_type='l1', disentangle_z=True, loss_weight=10.0),
    dict(cls='DisentanglePointMatchingLoss', loss_type='l2', disentangle_z=True),
    dict(cls='DisentanglePointMatchingLoss', loss_type='l1'),
    dict(cls='DisentanglePointMatchingLoss', loss_type='l2', reduction='sum', scale_xy=True, scale_depth=True,
         scale_depth_factor=0.5),
    dict(cls='RotPointMatchingLoss', loss_type='l2'),
    dict(cls='RotPointMatchingLoss', loss_type='l1', reduction='sum', loss_weight=3.0),
]
PIXEL_OPTIONS = [
    dict(cls='RAFTLoss', loss_weight=.1, max_flow=400., valid=True, gamma=0.8),
    dict(cls='RAFTLoss', loss_weight=1.0, max_flow=400., valid=False, gamma=0.8),
    dict(cls='RAFTLoss', loss_weight=2.5, max_flow=400., valid=True, gamma=0.5),
    dict(cls='L1Loss', loss_weight=10., valid=True, gamma=0.8),
    dict(cls='L1Loss', loss_weight=100., valid=False, gamma=0.5),
]
FIX_SYMMETRY = {'cls_2': {}}            # a falsy value: membership makes class 1 symmetric, truthiness would not
FIX_LABELS = (1, 0, 1)


def fixture_inputs():
    """the inputs tests/golden/make_golden_loss.py records in losses.npz: T=3, N=3, 24x40; classes of 65 and 300 vertices."""
    px = pixel_case((3, 24, 40), 3, 'nominal', seed=11)
    flat = px['gt'].permute(0, 2, 3, 1).reshape(-1, 2)
    vflat = px['valid'].reshape(-1).clone()
    special = [(400., 0.), (240., 320.), (300., 200.), (-500., 100.), (0., 400.), (300., 200.), (-500., 100.)]
    for i, xy in enumerate(special * 6):
        flat[5 + 3 * i] = torch.tensor(xy)
        vflat[5 + 3 * i] = 1.
    vflat[200:260:2] = 0.5
    px['gt'] = flat.reshape(3, 24, 40, 2).permute(0, 3, 1, 2).contiguous()
    px['valid'] = vflat.reshape(3, 24, 40)
    pm = pm_case([65, 300], FIX_LABELS, 3, seed=3, angle=0.9)
    return px, pm


def pm_flags(opt):
    return ((PM_SCALE_XY if opt.get('scale_xy') else 0) | (PM_SCALE_DEPTH if opt.get('scale_depth') else 0)
            | (PM_DISENTANGLE_Z if opt.get('disentangle_z') else 0))


PM_MODES = dict(PointMatchingLoss=PM_FULL, DisentanglePointMatchingLoss=PM_DISENTANGLE, RotPointMatchingLoss=PM_ROT)


def pm_ref_for(opt, pm, symmetric, gamma=0.8, **kw):
    return pm_ref(pm['verts'], pm['labels'], symmetric, pm['diameter'], pm['seq_r'], pm['seq_t'], pm['gt_r'], pm['gt_t'],
                  scale=pm['scale'], mode=PM_MODES[opt['cls']], loss_type=int(opt['loss_type'][-1]), flags=pm_flags(opt),
                  sdf=opt.get('scale_depth_factor', 1.), reduction=opt.get('reduction', 'mean'),
                  weight=opt.get('loss_weight', 1.), gamma=gamma, **kw)


def pixel_ref_for(opt, px, **kw):
    valid = px['valid'] if opt['valid'] else None
    if opt['cls'] == 'RAFTLoss':
        r = pixel_ref(px['gt'], valid, flows=[px['flow_a']], max_flow=opt['max_flow'], weights=(opt['loss_weight'], 1, 1),
                      gammas=(opt['gamma'],) * 3, **kw)
    else:
        r = pixel_ref(px['gt'], valid, flows=[], masks=px['masks'], weights=(1, 1, opt['loss_weight']),
                      gammas=(opt['gamma'],) * 3, **kw)
    return r['per_iter'][0], r['totals'][0]


@pytest.fixture(scope='module')
def fix():
    d = np.load(os.path.join(GOLDEN, 'losses.npz'))
    px = dict(gt=torch.from_numpy(d['gt']), valid=torch.from_numpy(d['valid']),
              flow_a=list(torch.from_numpy(d['flow_a'])), flow_b=list(torch.from_numpy(d['flow_b'])),
              masks=list(torch.from_numpy(d['masks'])))
    pm = dict(verts=[d['verts0'], d['verts1']], labels=d['labels'], gt_r=d['gt_r'], gt_t=d['gt_t'], seq_r=list(d['seq_r']),
              seq_t=list(d['seq_t']), scale=d['scale'], diameter=[float(x) for x in d['diameter']])
    return d, px, pm


def test_fixture_inputs_are_the_seeded_ones(fix):
    d, px, pm = fix
    px0, pm0 = fixture_inputs()
    assert torch.equal(px['gt'], px0['gt']) and torch.equal(px['valid'], px0['valid'])
    assert all(torch.equal(a, b) for a, b in zip(px['flow_a'], px0['flow_a']))
    assert np.array_equal(pm['verts'][1], pm0['verts'][1]) and np.array_equal(pm['seq_r'][2], pm0['seq_r'][2])
    assert json.loads(str(d['pm_options'])) == PM_OPTIONS and json.loads(str(d['pixel_options'])) == PIXEL_OPTIONS
    assert json.loads(str(d['symmetry_types'])) == FIX_SYMMETRY


# ------------------------------------------------------------------------------------ 1. the fixtures fall inside
def test_reference_pixel_values_fall_inside_the_bounds(fix):
    d, px, _ = fix
    worst = 0.0
    for i, opt in enumerate(PIXEL_OPTIONS):
        vals, total = pixel_ref_for(opt, px, torch_sums=True)
        for t, v in enumerate(vals):
            worst = max(worst, ratio(d[f'pixel_{i}_list'][t], v))
        worst = max(worst, ratio(d[f'pixel_{i}_total'], total))
    measured('reference pixel losses / (kernel bound + torch summation term)', worst)
    assert worst <= 1.0


def test_reference_point_matching_values_fall_inside_the_bounds(fix):
    d, _, pm = fix
    worst = 0.0
    for i, opt in enumerate(PM_OPTIONS):
        ref = pm_ref_for(opt, pm, [False, True], torch_sums=True)
        for t, v in enumerate(ref['per_iter']):
            worst = max(worst, ratio(d[f'pm_{i}_list'][t], v))
        worst = max(worst, ratio(d[f'pm_{i}_total'], ref['total']))
    measured('reference point-matching losses / (kernel bound + torch summation term)', worst)
    assert worst <= 1.0


def test_bounds_are_a_handful_of_u(fix):
    """the derived constants, written down: relative bound of a pixel value and of a point-matching value on the fixture."""
    _, px, pm = fix
    vals, total = pixel_ref_for(PIXEL_OPTIONS[0], px)
    rel = max(float(v.e / abs(v.v)) for v in vals) / U
    measured('pixel value bound / U', rel)
    assert 4.0 <= rel <= 8.0
    ref = pm_ref_for(PM_OPTIONS[0], pm, [False, True])
    relp = max(float(v.e / abs(v.v)) for v in ref['per_iter']) / U
    measured('point-matching value bound / U (coordinates ~800 mm, errors ~10 mm)', relp)
    assert relp < 5000                   # c U 800 mm per coordinate against a ~10 mm norm: cancellation, not slack


# ------------------------------------------------------------------------------------ 2. planted defects fall outside
@pytest.mark.parametrize('defect,opt', [('occ_magnitude', 3), ('valid_gt', 0), ('mag_le', 1), ('mask_by_count', 3),
                                        ('gamma_reversed', 0), ('gamma_reversed', 4)])
def test_planted_pixel_defects_fall_outside(fix, defect, opt):
    _, px, _ = fix
    if defect in ('occ_magnitude', 'mask_by_count'):
        # the fixture's L1Loss target is an explicit mask; the derived target is the refiner's: restate both sides on it
        good = pixel_ref(px['gt'], px['valid'], masks=px['masks'], weights=(1, 1, 10.))
        bad = pixel_ref(px['gt'], px['valid'], masks=px['masks'], weights=(1, 1, 10.), defect=defect)
        good, bad = (good['per_iter'][0], good['totals'][0]), (bad['per_iter'][0], bad['totals'][0])
    else:
        good, bad = pixel_ref_for(PIXEL_OPTIONS[opt], px), pixel_ref_for(PIXEL_OPTIONS[opt], px, defect=defect)
    if defect == 'gamma_reversed':
        r = ratio(bad[1].v, good[1])
    else:
        r = min(ratio(b.v, g) for b, g in zip(bad[0], good[0]))
    measured(f'planted {defect}: error / bound', r)
    assert r > 10.0


@pytest.mark.parametrize('defect', ['truthiness', 'l1_nearest', 'gamma_reversed', 'mean_for_sum'])
def test_planted_point_matching_defects_fall_outside(fix, defect):
    _, _, pm = fix
    opt = PM_OPTIONS[1]                                                          # l1, reduction='sum'
    good = pm_ref_for(opt, pm, [False, True])
    sym = [False, bool(FIX_SYMMETRY['cls_2'])] if defect == 'truthiness' else [False, True]
    bad = pm_ref_for(opt, pm, sym, defect=None if defect == 'truthiness' else defect)
    r = ratio(bad['total'].v, good['total'])
    measured(f'planted {defect}: error / bound', r)
    assert r > 10.0


# ------------------------------------------------------------------------------------ 4. the inputs of the GPU tests
def test_boundary_cells_straddle_max_flow_by_one_ulp():
    cells = find_boundary_cells()
    assert len(cells) >= 16
    mf = f32(400.)
    for x, y, below in cells:
        gx, gy = f32(x), f32(y)
        sep = np.sqrt(f32(f32(gx * gx) + f32(gy * gy)))
        fma = np.sqrt(f32(np.float64(gx) ** 2 + np.float64(f32(gy * gy))))
        assert (sep < mf) == below and (fma < mf) != below
        assert abs(float(sep) - float(fma)) <= float(np.spacing(mf)) and min(sep, fma) < mf <= max(sep, fma)
    assert len({c[2] for c in cells}) == 2                                       # both directions occur


@pytest.mark.parametrize('mode', [PM_FULL, PM_DISENTANGLE, PM_ROT])
@pytest.mark.parametrize('T', [1, 3])
@pytest.mark.parametrize('counts', PM_GPU_COUNTS)
def test_gpu_vertex_sets_decide_every_neighbour(counts, T, mode):
    seed, margin = pm_gpu_case(counts, T, mode)
    measured(f'V = {counts}, T = {T}, mode {mode}: seed {seed}, smallest (gap / slack) margin', margin)
    assert margin > 1.0


@pytest.mark.parametrize('counts,T,mode', [(c, 1, m) for c in PM_GPU_LARGE for m in PM_LARGE_VARIANTS] + [((64, 65), 33, PM_FULL)])
def test_gpu_vertex_sets_beyond_one_tile_decide_every_neighbour(counts, T, mode):
    large = max(counts) > 1024
    seed, margin = pm_gpu_case(counts, T, mode, large)
    case = pm_case(list(counts), PM_GPU_LARGE_LABELS if large else PM_GPU_LABELS, T, seed=seed, layout='lattice' if large else 'cloud')
    measured(f'V = {counts}, T = {T}, mode {mode}: seed {seed}, smallest (gap / slack) margin', margin)
    assert margin > 1.0
    if large and mode == PM_FULL:                   # the shifted prediction sends most points to ANOTHER vertex
        ref = pm_ref(case['verts'], case['labels'], [False, True], case['diameter'], case['seq_r'], case['seq_t'], case['gt_r'],
                     case['gt_t'], scale=case['scale'])
        nn = ref['nn'][0][0]
        assert (nn != np.arange(len(nn))).mean() > 0.5
        if len(nn) > 2048:                          # neighbours in every LDS chunk of the kernel
            assert all(((nn >= lo) & (nn < lo + 1024)).any() for lo in (0, 1024, 2048))


# ================================================================================================== loss() wiring
def wiring_ref(kind, seqs, gt_flow, valid, cfgs, max_flow=400., pose=None, init=None):
    """the refiners' loss() on top of the restatements -> OrderedDict key -> EV, keys in the reference's order.
    kind: 'scflow' (seqs: flow_from_pose, flow_from_pred, rotations, translations, masks), 'flow_mask' (flows, occlusions)
    or 'flow' (flows).  pose: dict(verts, labels, symmetric, diameter, gt_r, gt_t, scale) for a point-matching pose loss."""
    log = OrderedDict()
    fcfg = lambda c: (c['loss_func_cfg'], c.get('gamma', 0.8))
    if kind == 'flow':
        lf, g = fcfg(cfgs['loss_cfg'])
        r = pixel_ref(gt_flow, valid, flows=[seqs[0]], max_flow=lf.get('max_flow', 400), weights=(lf.get('loss_weight', 1.), 1, 1),
                      eps=(lf.get('eps', 1e-10),) * 2, gammas=(g,) * 3)
        for i, v in enumerate(r['per_iter'][0]):
            log[f'seq_{i}_loss'] = v
        log['loss'] = r['totals'][0]
        return log
    if kind == 'flow_mask':
        (lf, gf), (lm, gm) = fcfg(cfgs['flow_loss_cfg']), fcfg(cfgs['occlusion_loss_cfg'])
        r = pixel_ref(gt_flow, valid, flows=[seqs[0]], masks=seqs[1], max_flow=max_flow,
                      weights=(lf.get('loss_weight', 1.), 1, lm.get('loss_weight', 1.)), eps=(lf.get('eps', 1e-10),) * 2,
                      gammas=(gf, 1, gm))
        for i in range(len(seqs[0])):
            log[f'seq_{i}_flow_loss'] = r['per_iter'][0][i]
            log[f'seq_{i}_occ_loss'] = r['per_iter'][1][i]
        log['loss_occ'], log['loss_flow'] = r['totals'][1], r['totals'][0]
        log['loss'] = log['loss_flow'] + log['loss_occ']
        return log
    flow_from_pose, flow_from_pred, rots, trans, masks = seqs
    (lf, gf), (lm, gm), (lp, gp) = fcfg(cfgs['flow_loss_cfg']), fcfg(cfgs['mask_loss_cfg']), fcfg(cfgs['pose_loss_cfg'])
    r = pixel_ref(gt_flow, valid, flows=[flow_from_pred], masks=masks, max_flow=max_flow,
                  weights=(lf.get('loss_weight', 1.), 1, lm.get('loss_weight', 1.)), eps=(lf.get('eps', 1e-10),) * 2,
                  gammas=(gf, 1, gm))
    if lp['type'] == 'RAFTLoss':
        rp = pixel_ref(gt_flow, valid, flows=[flow_from_pose], max_flow=lp.get('max_flow', 400),
                       weights=(lp.get('loss_weight', 1.), 1, 1), eps=(lp.get('eps', 1e-10),) * 2, gammas=(gp,) * 3)
        pose_iter, pose_total = rp['per_iter'][0], rp['totals'][0]
    else:
        opt = dict(lp, cls=lp['type'])
        q = pm_ref(pose['verts'], pose['labels'], pose['symmetric'], pose['diameter'], rots, trans, pose['gt_r'], pose['gt_t'],
                   scale=pose.get('scale'), mode=PM_MODES[lp['type']], loss_type=int(lp.get('loss_type', 'l2')[-1]),
                   flags=pm_flags(opt), sdf=lp.get('scale_depth_factor', 1.), reduction=lp.get('reduction', 'mean'),
                   weight=lp.get('loss_weight', 1.), gamma=gp, nn_idx=pose.get('nn_idx'))
        pose_iter, pose_total = q['per_iter'], q['total']
    if init is not None:
        log['init_add_mean'], log['init_add_std'] = init
    for i in range(len(flow_from_pred)):
        log[f'seq_{i}_pose_loss'] = pose_iter[i]
        log[f'seq_{i}_flow_loss'] = r['per_iter'][0][i]
        log[f'seq_{i}_mask_loss'] = r['per_iter'][1][i]
    log['loss_mask'], log['loss_flow'], log['loss_pose'] = r['totals'][1], r['totals'][0], pose_total
    log['loss'] = (log['loss_pose'] + log['loss_flow']) + log['loss_mask']
    return log


REFINER_N, REFINER_ITERS = 3, 3


def refiner_loss_case(input_seed=7, case_seed=5):
    """what the loss of the `refiner_full` model and inputs is taken against: ground-truth poses near the reference
    poses, a ground-truth mask (the rendered disc with a corner cut off), 21 small random class meshes, the first
    sample's class symmetric, the init_add_error annotations and per-image scale factors."""
    from scflow_amd.synthetic import make_inputs
    inp = make_inputs(REFINER_N, 256, 256, seed=input_seed)
    rng = np.random.RandomState(case_seed)
    gt_r = np.stack([rand_rot(rng, 0.04) @ inp['ref_rotation'][n].numpy() for n in range(REFINER_N)]).astype(f32)
    gt_t = (inp['ref_translation'].numpy() + rng.randn(REFINER_N, 3) * [3, 3, 12]).astype(f32)
    gt_masks = (inp['depth'] > 0).clone()
    gt_masks[:, :100, :110] = False
    verts = [(rng.randn(40 + 5 * c, 3) * 35).astype(f32) for c in range(21)]
    labels = [int(x) for x in inp['label']]
    symmetry_types = {f'cls_{labels[0] + 1}': {}}
    diameter = [float(f32(90 + 7.7 * c)) for c in range(21)]
    init_add_error = torch.from_numpy(rng.uniform(5, 40, size=REFINER_N).astype(f32))
    scale = rng.uniform(0.8, 1.6, size=REFINER_N).astype(f32)
    return dict(inp=inp, gt_r=gt_r, gt_t=gt_t, gt_masks=gt_masks, verts=verts, labels=labels, symmetry_types=symmetry_types,
                diameter=diameter, init_add_error=init_add_error, scale=scale)


def refiner_loss_cfgs(case):
    import scflow_amd
    cfgs = scflow_amd.config.scflow_loss_cfgs(mesh_path='not/a/real/path')
    cfgs['pose_loss_cfg']['loss_func_cfg'].update(symmetry_types=case['symmetry_types'], mesh_diameter=case['diameter'])
    return cfgs


def refiner_data(case, device='cpu'):
    inp = case['inp']
    to = lambda x: (torch.from_numpy(x) if isinstance(x, np.ndarray) else x).to(device)
    sd, mn = torch.std_mean(case['init_add_error'], unbiased=False)
    return dict(ref_rotations=to(inp['ref_rotation']), ref_translations=to(inp['ref_translation']),
                gt_rotations=to(case['gt_r']), gt_translations=to(case['gt_t']), labels=to(inp['label']),
                internel_k=to(inp['internel_k']), rendered_images=to(inp['render_images']), real_images=to(inp['real_images']),
                rendered_masks=to((inp['depth'] > 0).float()), rendered_depths=to(inp['depth']),
                init_add_error_mean=to(mn), init_add_error_std=to(sd), gt_masks=to(case['gt_masks']),
                scale_factors=to(case['scale']))


# |d value| for a perturbation of the network outputs within tol (per element): flow value: both channels of every valid
# pixel, w * 2 tol; mask value: w * tol; pose value (disentangled, l1): per point |dR p|_1 <= 3 tol_R |p|_1 for the rotation
# term, tol_t for the depth term, 2 tol_t for the xy term, over the diameter, times w
def propagated_tolerance(key, cfgs, tol, case):
    w = lambda name: cfgs[name]['loss_func_cfg'].get('loss_weight', 1.)
    p1 = max(float(np.abs(v).sum(1).mean()) for v in case['verts'])
    dmin = min(case['diameter'])
    pose = w('pose_loss_cfg') * (3 * tol['rotation'] * p1 + 3 * tol['translation']) / dmin
    flow, mask = w('flow_loss_cfg') * 2 * tol['flow_from_pred'], w('mask_loss_cfg') * tol['mask']
    gsum = sum(0.8 ** k for k in range(REFINER_ITERS))
    if key.endswith('_pose_loss'):
        return pose
    if key.endswith('_flow_loss'):
        return flow
    if key.endswith('_mask_loss'):
        return mask
    return dict(loss_pose=pose * gsum, loss_flow=flow * gsum, loss_mask=mask * gsum, loss=(pose + flow + mask) * gsum,
                init_add_mean=0., init_add_std=0.)[key]


ORACLE_TOL = dict(flow_from_pose=2e-4, flow_from_pred=1.2e-4, rotation=3e-7, translation=4e-4, mask=2.5e-6)   # test_oracle_golden.py


def test_wiring_reproduces_the_reference_log_vars(golden_dir):
    """3. oracle.get_pose -> the restated wiring == the reference's SCFlowRefiner.loss log_vars (refiner_loss.npz) within the
    oracle's network tolerance propagated to each value, plus the restatement's own bound."""
    from scflow_amd.weights import fill_state_dict
    g = np.load(os.path.join(golden_dir, 'refiner_loss.npz'))
    case = refiner_loss_case(int(g['input_seed']), int(g['case_seed']))
    assert np.array_equal(g['gt_r'], case['gt_r']) and np.array_equal(g['gt_t'], case['gt_t'])
    assert np.array_equal(np.unpackbits(g['gt_masks_bits'])[:case['gt_masks'].numel()].astype(bool),
                          case['gt_masks'].numpy().reshape(-1))
    keys = json.load(open(os.path.join(golden_dir, 'state_dict_keys.json')))['shapes']
    sd = fill_state_dict(keys, seed=int(g['weight_seed']))
    inp = case['inp']
    with torch.no_grad():
        outs = oracle.get_pose(inp['render_images'], inp['real_images'], inp['ref_rotation'], inp['ref_translation'],
                               inp['depth'], inp['internel_k'], inp['label'], sd, iters=REFINER_ITERS)
        gt_flow = oracle.flow_from_delta_pose_and_depth(inp['ref_rotation'], inp['ref_translation'], torch.from_numpy(case['gt_r']),
                                                        torch.from_numpy(case['gt_t']), inp['depth'], inp['internel_k'], 400.)
        gt_flow = oracle.filter_flow_by_mask(gt_flow, case['gt_masks'], 400.)
    cfgs = refiner_loss_cfgs(case)
    sym = [f'cls_{c + 1}' in case['symmetry_types'] for c in range(21)]
    sd_, mn_ = torch.std_mean(case['init_add_error'], unbiased=False)
    log = wiring_ref('scflow', [outs[0], outs[1], outs[2], outs[3], [m[:, 0] for m in outs[4]]], gt_flow,
                     (inp['depth'] > 0).float(), cfgs,
                     pose=dict(verts=case['verts'], labels=case['labels'], symmetric=sym, diameter=case['diameter'],
                               gt_r=case['gt_r'], gt_t=case['gt_t'], scale=case['scale']),
                     init=(EV(float(mn_), 4 * U * float(mn_)), EV(float(sd_), 16 * U * float(mn_))))
    want_keys = [str(k) for k in g['keys']]
    assert list(log.keys()) == want_keys
    worst = 0.0
    for k, want in zip(want_keys, g['values']):
        ev = log[k]
        room = float(ev.e) + propagated_tolerance(k, cfgs, ORACLE_TOL, case)
        r = abs(float(want) - float(ev.v)) / room if room else float(want != ev.v)
        worst = max(worst, r)
        assert r <= 1.0, (k, float(want), float(ev.v), room)
    measured('reference log_vars vs oracle + restated wiring: worst error / propagated tolerance', worst)


def test_refiner_constructors_keep_loss_configs_lazy():
    """the model dicts of scflow_amd.config still build (opaque SequenceLoss dicts, mesh paths that do not exist); loss()
    on an opaque config says what is missing; forward(return_loss=True) still raises."""
    import scflow_amd
    m = scflow_amd.build_refiner(scflow_amd.scflow_model_cfg(iters=2))
    with pytest.raises(ValueError, match='loss_func_cfg'):
        m.loss(None, data={})
    with pytest.raises(NotImplementedError):
        m.forward({}, return_loss=True)
    cfg = scflow_amd.scflow_model_cfg(iters=2)
    cfg.update(scflow_amd.scflow_loss_cfgs())                                   # 'data/ycbv/models_eval' does not exist here
    m = scflow_amd.build_refiner(cfg)
    m._build_loss_funcs()
    assert isinstance(m.pose_loss_func.loss_func, scflow_amd.DisentanglePointMatchingLoss)
    assert m.pose_loss_func.loss_func.disentagle_z and m.flow_loss_func.loss_func.loss_weight == .1
    with pytest.raises(FileNotFoundError):
        m.pose_loss_func.loss_func.meshes
    r = scflow_amd.raft_model_cfg(iters=2)
    r.update(scflow_amd.raft_loss_cfgs(), filter_invalid_flow_by_depth=True)
    rm = scflow_amd.build_refiner(r)
    with pytest.raises(NotImplementedError, match='filter_invalid_flow_by_depth'):
        rm.loss(None, data={})
    m.render_augmentations = [dict(type='RandomGaussianBlur')]
    with pytest.raises(NotImplementedError, match='render_augmentations'):
        m.format_data_train_sup({})
    assert set(scflow_amd.LOSSES.module_dict) >= {'RAFTLoss', 'L1Loss', 'SequenceLoss', 'PointMatchingLoss',
                                                  'DisentanglePointMatchingLoss', 'RotPointMatchingLoss'}
    with pytest.raises(scflow_amd._lib.ScflowHipError):
        scflow_amd.RAFTLoss()(torch.zeros(1, 2, 4, 4), torch.zeros(1, 2, 4, 4))


def test_reference_model_dicts_build_unchanged():
    """the loss keys of configs/refine_models/scflow.py:75-104 and raft.py:49-65, as scflow_amd.config restates them, go
    through build_loss without editing a key."""
    import scflow_amd
    for name, cfg in {**scflow_amd.scflow_loss_cfgs(), **scflow_amd.raft_loss_cfgs()}.items():
        f = scflow_amd.build_loss(cfg)
        assert isinstance(f, scflow_amd.SequenceLoss) and f.gamma == 0.8, name
    sym = scflow_amd.config.YCBV_SYMMETRY_TYPES
    assert sorted(sym) == ['cls_13', 'cls_16', 'cls_19', 'cls_20', 'cls_21'] and len(scflow_amd.config.YCBV_MESH_DIAMETER) == 21
