"""CPU: the backward of the parameter-free tail of an SCFlow iteration (tail_grad.hip: scf_resize_bilinear_grad,
scf_reproject_flow_grad, scf_pose_tail_grad; SCFlowDecoder.tail_backward) restated three times:

* `tail_restatement` / `tail_vjp`: the DEFINITION -- float64 autograd through a plain-torch restatement of the reference's
  expressions (scflow_decoder.py:191-250, models/utils/pose.py:66-169).  The bilinear resize is F.interpolate's
  align_corners arithmetic with its source coordinate fl(fl((in - 1) / (out - 1)) * index) taken in fp32 as the forward
  kernel and ATen define it (`resize_coords(..., 'fp32')`): the weights are inputs of the operation.  `stored`: the fp32
  poses (and, for a loss on top, the fp32 flows and masks) a forward pass produced replace the values of the outputs
  (straight through: the gradient still flows), because the kernels differentiate at the values the forward stored;
* the closed forms of DESIGN.md section 4.5 in numpy float64 (`resize_grad_ref`, `reproject_grad_ref`,
  `scan_closed_form`), equal to the definition to 1e-12, each with a derived per-element bound for the kernel;
* numpy replays of the kernels' operation order (`resize_grad_fp32`, `reproject_grad_fp32`, the scan rounded once),
  which lie inside the bounds while planted defects lie outside.

Bounds (U = 2**-24):
  resize adjoint   |mul| U C S,  S = sum w' |g| with every 1 - l weight widened by its own rounding, C the number of
                   roundings on the longest chain a term of that node passes: the two weight products, the additions
                   inside a quad (<= its terms for the node), one per quad, one per row term, the product with mul
                   (+ 1 for a second addend; an accumulating call adds U |result|);
  re-projection    per pixel through EV (un-projection, R P + t, K p, the three quotients, K^T g_q, the product with P),
                   summed; the fp64 accumulation adds count * 2**-53 * sum |term|;
  pose scan        U |out| + 2**-150 (one rounding, subnormal results included) + |J| bound(incoming sums) + 2**-40 |J| |G| (the fp64 evaluation), J the
                   Jacobian of the outputs with respect to the incoming cotangents (the scan is linear in them).
"""
import itertools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_stream_ops_host import (DEPTH_LINEAR, EV, GEOM_SIZES, POSE_REGIMES, RESIZE_SIZES, U, _inv64, _unproject_ev,
                                  ev_matvec, f64, geom_case, measured, pose_case, pose_select, rand_rot, resize_coords,
                                  worst_ratio)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'tail_grads.npz')
FLAG_COMBOS = list(itertools.product([False, True], repeat=3))       # (detach_flow, detach_pose, detach_depth_for_xy)
F32 = np.float32
TINY = 2.0 ** -150                  # rounding to fp32 below 2**-126 (gradual underflow): half the spacing of the subnormals


# ====================================================================================================== resize adjoint
def axis_taps(n_in, n_out):
    """(i0, i1, l) of every output index as resample.hip and tail_grad.hip define them: f = fl(fl(scale) * index) in
    fp32, i0 = (int)f clamped, i1 the clamped +1 tap, l = f - i0 (exact in fp32)."""
    s = F32(n_in - 1) / F32(n_out - 1) if n_out > 1 else F32(0)
    fc = (s * np.arange(n_out).astype(F32)).astype(F32)
    assert np.array_equal(fc.astype(np.float64), resize_coords(n_in, n_out, 'fp32'))
    i0 = np.minimum(fc.astype(np.int64), n_in - 1)
    return i0, np.minimum(i0 + 1, n_in - 1), (fc - i0.astype(F32)).astype(F32)


def interp_matrix(n_in, n_out, widen=0.0):
    """(n_out, n_in) float64 interpolation matrix of one axis; `widen` is added to every 1 - l weight."""
    i0, i1, l = axis_taps(n_in, n_out)
    m = np.zeros((n_out, n_in))
    np.add.at(m, (np.arange(n_out), i0), 1.0 - l.astype(np.float64) + widen)
    np.add.at(m, (np.arange(n_out), i1), l.astype(np.float64))
    return m


def _chain(n_in, n_out, quads):
    """per input node of one axis: the roundings its longest chain of additions holds (see the module docstring)."""
    i0, i1, _ = axis_taps(n_in, n_out)
    c = np.zeros(n_in)
    for i in range(n_in):
        terms = (i0 == i).astype(int) + (i1 == i).astype(int)
        if not quads:
            c[i] = terms.sum()
            continue
        reach = (i0 == i) | (i0 == i - 1)
        q = np.arange(n_out) // 4
        per_quad = np.bincount(q, weights=terms, minlength=q.max() + 1 if n_out else 1)
        c[i] = (per_quad.max() if n_out else 0) + len(np.unique(q[reach]))
    return c


def resize_grad_ref(g, in_hw, mul=1.0, add=None, dst=None):
    """g (P, Hout, Wout) fp32 -> (reference, bound) of mul * U^T (g + add) (+ dst), (P, Hin, Win)."""
    v = f64(g) + (f64(add) if add is not None else 0.0)
    hin, win = in_hw
    ho, wo = v.shape[-2:]
    uy, ux = interp_matrix(hin, ho), interp_matrix(win, wo)
    ref = float(F32(mul)) * np.einsum('oi,pox,xj->pij', uy, v, ux)
    s = np.einsum('oi,pox,xj->pij', interp_matrix(hin, ho, U), np.abs(v), interp_matrix(win, wo, U))
    c = 3.0 + _chain(hin, ho, False)[:, None] + _chain(win, wo, True)[None, :] + (1.0 if add is not None else 0.0)
    bound = abs(float(F32(mul))) * U * c[None] * s
    if dst is not None:
        ref = ref + f64(dst)
        bound = bound + U * (np.abs(ref) + bound)
    return ref, bound


def resize_grad_fp32(g, in_hw, mul=1.0, add=None, dst=None, defect=None):
    """the kernels' operation order in numpy fp32 (quad partials, quads ascending, rows ascending), one planted defect."""
    v = np.asarray(g, dtype=F32)
    if add is not None:
        v = (v + np.asarray(add, dtype=F32)).astype(F32)
    p, ho, wo = v.shape
    hin, win = in_hw
    if defect == 'forward_matrix':                                  # U in place of U^T (needs Hin Win == Hout Wout)
        full = np.kron(interp_matrix(hin, ho), interp_matrix(win, wo))        # (Hout Wout, Hin Win)
        return (float(F32(mul)) * (v.reshape(p, -1).astype(np.float64) @ full.T)).reshape(p, hin, win).astype(F32)
    x0, x1, lx = axis_taps(win, wo)
    y0, y1, ly = axis_taps(hin, ho)
    hx, hy = (F32(1) - lx).astype(F32), (F32(1) - ly).astype(F32)
    r = np.zeros((p, ho, win), dtype=F32)
    for q in range((wo + 3) // 4):
        part = np.zeros((p, ho, win), dtype=F32)
        touched = set()
        for ox in range(4 * q, min(4 * q + 4, wo)):
            part[:, :, x0[ox]] = part[:, :, x0[ox]] + hx[ox] * v[:, :, ox]
            if not (defect == 'edge_tap' and x1[ox] == x0[ox]):
                part[:, :, x1[ox]] = part[:, :, x1[ox]] + lx[ox] * v[:, :, ox]
            touched |= {int(x0[ox]), int(x1[ox])}
        for ix in touched:
            r[:, :, ix] = r[:, :, ix] + part[:, :, ix]
    acc = np.zeros((p, hin, win), dtype=F32)
    for oy in range(ho):
        acc[:, y0[oy]] = acc[:, y0[oy]] + hy[oy] * r[:, oy]
        if not (defect == 'edge_tap' and y1[oy] == y0[oy]):
            acc[:, y1[oy]] = acc[:, y1[oy]] + ly[oy] * r[:, oy]
    out = acc if defect == 'no_mul' else (F32(mul) * acc).astype(F32)
    if dst is not None:
        out = (np.asarray(dst, dtype=F32) + out).astype(F32)
    return out


def resize_grad_case(planes, out_hw, seed=0, small_int=False):
    g = torch.Generator().manual_seed(21000 + seed + 7 * out_hw[0] + out_hw[1])
    if small_int:
        return torch.randint(-8, 9, (planes, *out_hw), generator=g).float()
    return torch.randn((planes, *out_hw), generator=g)


def find_edge_excess(lo=100, hi=400):
    """(n_in, n_out): the smallest n_in >= lo with an n_out whose last coordinate fl(fl(scale) * (n_out - 1)) lands PAST
    n_in - 1, i.e. on the clamped +1 tap with a weight of one ulp of the coordinate (as (4, 8) -> (10, 50) does at 7)."""
    for n_in in range(lo, hi):
        for n_out in range(n_in + 1, 4 * n_in):
            if F32(F32(n_in - 1) / F32(n_out - 1)) * F32(n_out - 1) > F32(n_in - 1):
                assert axis_taps(n_in, n_out)[2][-1] > 0
                return n_in, n_out
    raise AssertionError('no size with an excess coordinate found')


# ======================================================================================================= re-projection
def _q_ev(depth, k, rot0, trans0, rot, trans):
    fg, xs, ys, obj = _unproject_ev(depth, k, rot0, trans0)
    cam = ev_matvec(f64(rot)[:, None, None], obj, add=f64(trans)[:, None, None])
    return fg, obj, ev_matvec(f64(k)[:, None, None], cam)


def reproject_grad_ref(depth, k, rot0, trans0, rot, trans, g):
    """-> (sums (N, 12), bound (N, 12)): words [0, 9) = sum g_p (x) P, [9, 12) = sum g_p over the foreground, every fp32
    operation of reproject_flow_grad_kernel replayed through EV; g None -> zeros.  A sample whose bound is not finite
    (a pixel with |qz| inside its own error) has bound inf."""
    n = depth.shape[0]
    if g is None:
        return np.zeros((n, 12)), np.zeros((n, 12))
    fg, obj, q = _q_ev(depth, k, rot0, trans0, rot, trans)
    gu, gv = EV(f64(g)[:, 0]), EV(f64(g)[:, 1])
    a, b = gu / q[2], gv / q[2]
    c = (gu * q[0] + gv * q[1]) / (q[2] * q[2])
    c = EV(-c.v, c.e)
    kk = f64(k)[:, None, None]
    gp = [EV(kk[..., 0, j]) * a + EV(kk[..., 1, j]) * b + EV(kk[..., 2, j]) * c for j in range(3)]
    terms = [gp[i] * obj[j] for i in range(3) for j in range(3)] + gp
    ref, bound = np.zeros((n, 12)), np.zeros((n, 12))
    cnt = fg.reshape(n, -1).sum(1)
    with np.errstate(all='ignore'):
        for w, t in enumerate(terms):
            v, e = np.where(fg, t.v, 0.0).reshape(n, -1), np.where(fg, t.e, 0.0).reshape(n, -1)
            ref[:, w] = v.sum(1)
            bound[:, w] = e.sum(1) + cnt * 2.0 ** -53 * np.abs(v).sum(1)
    bad = ~np.isfinite(bound).all(1) | ~np.isfinite(ref).all(1)
    bound[bad] = np.inf
    ref[bad] = 0.0
    return ref, bound


def reproject_grad_coefs(depth, k, rot0, trans0, rot, trans):
    """float64 (A, B) (N, 12, H, W) with sums = sum over pixels of A gu + B gv (0 on the background): the linear map the
    sums are of the cotangent, for the closed form and for carrying a bound of g into the sums."""
    d = f64(depth)
    n, h, w = d.shape
    with np.errstate(all='ignore'):
        fg = d > 0
    dd = np.where(fg, d, 1.0)
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing='ij')
    mv = lambda m, v: np.einsum('nij,njhw->nihw', m, v)             # noqa: E731
    hom = np.stack([xs[None] * dd, ys[None] * dd, dd], 1)
    P = mv(_inv64(rot0), mv(_inv64(k), hom) - f64(trans0)[:, :, None, None])
    q = mv(f64(k), mv(f64(rot), P) + f64(trans)[:, :, None, None])
    kk = f64(k)
    out = []
    for gu, gv in ((1.0, 0.0), (0.0, 1.0)):
        with np.errstate(all='ignore'):
            gq = np.stack([gu / q[:, 2], gv / q[:, 2], -(gu * q[:, 0] + gv * q[:, 1]) / q[:, 2] ** 2], 1)
        gp = np.einsum('nji,njhw->nihw', kk, gq)                    # K^T g_q
        t = np.concatenate([(gp[:, :, None] * P[:, None]).reshape(n, 9, h, w), gp], 1)
        out.append(np.where(fg[:, None], t, 0.0))
    return out[0], out[1]


def reproject_grad_fp32(depth, k, rot0, trans0, rot, trans, g, defect=None):
    """the kernel's operation order in numpy fp32 (inverses: float64, rounded, like inv3x3), products summed in float64."""
    f = F32
    n, h, w = depth.shape
    d = depth.numpy()
    with np.errstate(all='ignore'):
        fg = (d != 0) & ~np.isnan(d) if defect == 'background' else d > 0
    dd = np.where(d > 0, d, f(1)) if defect != 'background' else np.where(fg, d, f(1))
    ys, xs = np.meshgrid(np.arange(h, dtype=f), np.arange(w, dtype=f), indexing='ij')
    kinv, r0inv = _inv64(k).astype(f)[:, None, None], _inv64(rot0).astype(f)[:, None, None]
    kk, rr = k.numpy()[:, None, None], rot.numpy()[:, None, None]
    t0, tt = trans0.numpy()[:, None, None], trans.numpy()[:, None, None]
    mv = lambda m, v: [m[..., r, 0] * v[0] + m[..., r, 1] * v[1] + m[..., r, 2] * v[2] for r in range(3)]   # noqa: E731
    cam = mv(kinv, [xs[None] * dd, ys[None] * dd, dd])
    P = mv(r0inv, [cam[i] - t0[..., i] for i in range(3)])
    p = mv(rr, P)
    q = mv(kk, [p[i] + tt[..., i] for i in range(3)])
    gu, gv = g.numpy()[:, 0], g.numpy()[:, 1]
    with np.errstate(all='ignore'):
        a, b = gu / q[2], gv / q[2]
        c = (gu * q[0] + gv * q[1]) / (q[2] * q[2])
        c = c if defect == 'qz2_sign' else -c
        if defect == 'K_not_transposed':
            gp = [kk[..., j, 0] * a + kk[..., j, 1] * b + kk[..., j, 2] * c for j in range(3)]
        else:
            gp = [kk[..., 0, j] * a + kk[..., 1, j] * b + kk[..., 2, j] * c for j in range(3)]
        terms = [gp[i] * P[j] for i in range(3) for j in range(3)] + gp
        return np.stack([np.where(fg, t, f(0)).astype(np.float64).reshape(n, -1).sum(1) for t in terms], 1)


# =========================================================================================================== pose scan
def _cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], -1)


def _normalize_bwd(v, nrm, den, g):
    with np.errstate(all='ignore'):
        gden = -(g * v).sum(-1, keepdims=True) / (den * den)
        through = np.where(nrm >= 1e-12, v * (gden / np.where(nrm > 0, nrm, 1.0)), 0.0)
        return g / den + through


def scan_closed_form(d_rot, d_trans, rot0, trans0, rots, transs, g_rot, g_trans, detach_pose, detach_depth, linear,
                     defect=None):
    """the reverse scan of DESIGN.md section 4.5 in numpy float64.  d_rot (T, N, 6), d_trans (T, N, 3), rots (T, N, 3, 3),
    transs (T, N, 3): entry i - 1 is the input of iteration i; g_rot / g_trans: the incoming cotangents (loss plus
    re-projection sums) -> (g_d_rot (T, N, 6), g_d_trans (T, N, 3))."""
    d_rot, d_trans, g_rot, g_trans = f64(d_rot), f64(d_trans), f64(g_rot), f64(g_trans)
    T, n = d_rot.shape[:2]
    out_r, out_t = np.zeros((T, n, 6)), np.zeros((T, n, 3))
    c_r, c_t = np.zeros((n, 3, 3)), np.zeros((n, 3))
    carry = (not detach_pose or defect == 'carry_when_detached') and defect != 'no_carry'
    for i in range(T - 1, -1, -1):
        G, Gt = g_rot[i] + c_r, g_trans[i] + c_t
        rp = f64(rot0) if i == 0 else f64(rots[i - 1])
        tp = f64(trans0) if i == 0 else f64(transs[i - 1])
        a, b, dt = d_rot[i][:, :3], d_rot[i][:, 3:], d_trans[i]
        with np.errstate(all='ignore'):
            na = np.sqrt((a * a).sum(-1, keepdims=True))
            da = np.maximum(na, 1e-12)
            x = a / da
            zp = _cross(x, b)
            nz = np.sqrt((zp * zp).sum(-1, keepdims=True))
            dz = np.maximum(nz, 1e-12)
            z = zp / dz
            y = _cross(z, x)
            grd = G @ np.swapaxes(rp, 1, 2)
            gx, gy, gz = grd[:, :, 0], grd[:, :, 1], grd[:, :, 2]
            gz = gz + _cross(x, gy)
            gx = gx + _cross(gy, z)
            gzp = _normalize_bwd(zp, nz, dz, gz)
            gx = gx + _cross(b, gzp)
            gb = _cross(gzp, x)
            ga = _normalize_bwd(a, na, da, gx)
            out_r[i] = np.concatenate([ga, gb], -1)
            tx, ty, tz = tp[:, 0], tp[:, 1], tp[:, 2]
            ez = np.exp(dt[:, 2])
            vz = tz * (dt[:, 2] + 1.0) if linear else tz / ez
            u, v = dt[:, 0] / 10.0 + tx / tz, dt[:, 1] / 10.0 + ty / tz
            keep_vz = not detach_depth or defect == 'vz_not_detached'
            gvz = Gt[:, 2] + ((Gt[:, 0] * u + Gt[:, 1] * v) if keep_vz else 0.0)
            gu, gv = Gt[:, 0] * vz, Gt[:, 1] * vz
            exp_form = (not linear) or defect == 'exp_on_linear'
            out_t[i] = np.stack([gu / 10.0, gv / 10.0, -gvz * vz if exp_form else gvz * tz], -1)
            if carry:
                rd = np.stack([x, y, z], -1)                        # columns
                c_r = rd @ G if defect == 'rd_not_transposed' else np.swapaxes(rd, 1, 2) @ G
                c_t = np.stack([gu / tz, gv / tz,
                                -(gu * tx + gv * ty) / (tz * tz) + (gvz * (dt[:, 2] + 1.0) if linear else gvz / ez)], -1)
            else:
                c_r, c_t = np.zeros((n, 3, 3)), np.zeros((n, 3))
    return out_r, out_t


def scan_ref(d_rot, d_trans, rot0, trans0, rots, transs, g_rot, g_trans, detach_pose, detach_depth, linear,
             g_rot_bound=None, g_trans_bound=None):
    """-> (g_d_rot, bound), (g_d_trans, bound): one rounding per output, the bound of the incoming sums carried through
    |J|, and 2**-40 |J| |G| for the fp64 evaluation (a few hundred operations of 2**-53 each on magnitudes |J| |G|)."""
    args = (d_rot, d_trans, rot0, trans0, rots, transs)
    kw = dict(detach_pose=detach_pose, detach_depth=detach_depth, linear=linear)
    ref_r, ref_t = scan_closed_form(*args, g_rot, g_trans, **kw)
    T, n = ref_r.shape[:2]
    br = np.zeros((T, n, 3, 3)) if g_rot_bound is None else f64(g_rot_bound)
    bt = np.zeros((T, n, 3)) if g_trans_bound is None else f64(g_trans_bound)
    mag_r, mag_t = 2.0 ** -40 * np.abs(f64(g_rot)) + br, 2.0 ** -40 * np.abs(f64(g_trans)) + bt
    prop_r, prop_t = np.zeros_like(ref_r), np.zeros_like(ref_t)
    with np.errstate(all='ignore'):
        for t in range(T):
            for c in range(12):
                er, et = np.zeros((T, n, 3, 3)), np.zeros((T, n, 3))
                if c < 9:
                    er[t, :, c // 3, c % 3] = 1.0
                    m = mag_r[t, :, c // 3, c % 3]
                else:
                    et[t, :, c - 9] = 1.0
                    m = mag_t[t, :, c - 9]
                if not np.any(m):
                    continue
                jr, jt = scan_closed_form(*args, er, et, **kw)
                prop_r += np.abs(jr) * m[None, :, None]
                prop_t += np.abs(jt) * m[None, :, None]
        # the one rounding: half an ulp of a normal result, half the spacing 2**-149 of a result below 2**-126
        return (ref_r, U * np.abs(ref_r) + TINY + prop_r * (1 + U)), (ref_t, U * np.abs(ref_t) + TINY + prop_t * (1 + U))


def scan_case(regime, n, T, seed=0, with_sums=True):
    """T pose updates of `pose_case(regime, n)` (the regime applied to every iteration), the fp32 poses an exact forward
    stores, and cotangents; with_sums: re-projection-sized contributions are added to the cotangents."""
    d_rots, d_transs, rots, transs = [], [], [], []
    rot0 = trans0 = None
    for i in range(T):
        rot_all, trans_all, label, rot, trans = pose_case(regime, n, seed=seed + 31 * i)
        dr, dt = pose_select(rot_all, trans_all, label, 1)
        if i == 0:
            rot0, trans0 = rot, trans
        d_rots.append(dr.contiguous())
        d_transs.append(dt.contiguous())
    g = torch.Generator().manual_seed(23000 + 100 * POSE_REGIMES.index(regime) + n + 7 * T + seed)
    g_rot = torch.randn((T, n, 3, 3), generator=g) * (30.0 if with_sums else 1.0)
    g_trans = torch.randn((T, n, 3), generator=g) * (30.0 if with_sums else 1.0)
    return d_rots, d_transs, rot0.contiguous(), trans0.contiguous(), g_rot, g_trans


def pose_forward64(d_rots, d_transs, rot0, trans0, linear):
    """the fp32-rounded poses of an exact (float64) forward over the T updates: what a forward pass stores."""
    r, t = rot0.double(), trans0.double()
    rots, transs = [], []
    with np.errstate(all='ignore'):
        for dr, dt in zip(d_rots, d_transs):
            r, t = _pose_update_torch(dr.double(), dt.double(), r, t, linear, False)
            r, t = r.float().double(), t.float().double()
            rots.append(r.float())
            transs.append(t.float())
    return rots, transs


# ========================================================================================================= definition
def _pose_update_torch(d_rot, d_trans, rot, trans, linear, detach_depth):
    """get_pose_from_delta_pose (pose.py:124-169), ortho6d rows, weight 10, in the dtype of its arguments."""
    x = F.normalize(d_rot[:, 0:3], p=2, dim=1)
    z = F.normalize(torch.cross(x, d_rot[:, 3:6], dim=1), p=2, dim=1)
    y = torch.cross(z, x, dim=1)
    r_new = torch.bmm(torch.cat((x.view(-1, 3, 1), y.view(-1, 3, 1), z.view(-1, 3, 1)), 2), rot)
    vz = trans[:, 2] * (d_trans[:, 2] + 1) if linear else torch.div(trans[:, 2], torch.exp(d_trans[:, 2]))
    vzs = vz.detach() if detach_depth else vz
    vx = torch.mul(vzs, torch.addcdiv(d_trans[:, 0] / 10., trans[:, 0], trans[:, 2]))
    vy = torch.mul(vzs, torch.addcdiv(d_trans[:, 1] / 10., trans[:, 1], trans[:, 2]))
    return r_new, torch.stack([vx, vy, vz], dim=-1)


def _interp(v, out_hw):
    uy = torch.from_numpy(interp_matrix(v.shape[-2], out_hw[0])).to(v.dtype)
    ux = torch.from_numpy(interp_matrix(v.shape[-1], out_hw[1])).to(v.dtype)
    return uy @ v @ ux.T


def tail_restatement(d_flows, masks, d_rots, d_transs, ref_rot, ref_trans, depth, k, init_flow, invalid, flags,
                     depth_transform='exp', scale=8, stored=None):
    """the tail of T iterations in the dtype of the head outputs (float64 for the definition) -> dict of the five output
    sequences plus `flow_lr`.  flags = (detach_flow, detach_pose, detach_depth_for_xy).  The dense form of
    get_flow_from_delta_pose_and_points: background pixels are the constant `invalid`."""
    detach_flow, detach_pose, detach_depth = flags
    dt = d_flows[0].dtype
    n, H, W = depth.shape
    h, w = H // scale, W // scale
    d = depth.to(dt)
    fg = depth > 0
    dd = torch.where(fg, d, torch.ones_like(d))
    ys, xs = torch.meshgrid(torch.arange(H, dtype=dt), torch.arange(W, dtype=dt), indexing='ij')
    kk, r0, t0 = k.to(dt), ref_rot.to(dt), ref_trans.to(dt)
    hom = torch.stack([xs[None] * dd, ys[None] * dd, dd], 1)
    mv = lambda m, v: torch.einsum('nij,njhw->nihw', m, v)          # noqa: E731
    P = mv(torch.inverse(r0), mv(torch.inverse(kk), hom) - t0[:, :, None, None])
    xy = torch.stack([xs, ys], 0)[None]
    out = dict(flow_from_pose=[], flow_from_pred=[], rotation_preds=[], translation_preds=[], mask_preds=[], flow_lr=[])
    flow, rot, trans = init_flow.to(dt), r0, t0
    for i in range(len(d_flows)):
        flow_in = flow.detach() if detach_flow else flow
        flow_lr = 1 / scale * _interp(flow_in, (h, w))
        flow_pred = scale * _interp(flow_lr + d_flows[i], (H, W))
        up_mask = _interp(masks[i], (H, W))
        rot, trans = _pose_update_torch(d_rots[i], d_transs[i], rot.detach() if detach_pose else rot,
                                        trans.detach() if detach_pose else trans, depth_transform != 'exp', detach_depth)
        if stored is not None and not isinstance(stored, dict):
            stored = dict(rotation_preds=stored[0], translation_preds=stored[1])
        # straight through: the stored values, the same graph
        thru = lambda key, v: v if stored is None or stored.get(key) is None else v + (stored[key][i].to(dt).reshape(v.shape) - v).detach()   # noqa: E731
        rot, trans = thru('rotation_preds', rot), thru('translation_preds', trans)
        q = mv(kk, mv(rot, P) + trans[:, :, None, None])
        flow = torch.where(fg[:, None], q[:, :2] / q[:, 2:3] - xy, torch.full_like(xy, float(invalid)).expand(n, 2, H, W))
        flow, flow_pred, up_mask = thru('flow_from_pose', flow), thru('flow_from_pred', flow_pred), thru('mask_preds', up_mask)
        for key, val in zip(out, (flow, flow_pred, rot, trans, up_mask, flow_lr)):
            out[key].append(val)
    return out


COT_KEYS = ('flow_from_pose', 'flow_from_pred', 'rotation_preds', 'translation_preds', 'mask_preds')
HEAD_KEYS = ('delta_flow_preds', 'masks', 'delta_rotation_preds', 'delta_translation_preds')


def tail_vjp(heads, consts, cots, flags, depth_transform='exp', extra=None, stored=None, dtype=torch.float64):
    """autograd of `tail_restatement`: heads = dict of the four head-output lists, consts = (ref_rot, ref_trans, depth,
    k, init_flow, invalid), cots = dict of cotangent lists under COT_KEYS (missing / None: none) -> dict of numpy lists
    under HEAD_KEYS, and the forward outputs."""
    leaves = {key: [t.detach().to(dtype).clone().requires_grad_() for t in heads[key]] for key in HEAD_KEYS}
    out = tail_restatement(leaves['delta_flow_preds'], leaves['masks'], leaves['delta_rotation_preds'],
                           leaves['delta_translation_preds'], *consts, flags, depth_transform, stored=stored)
    total = torch.zeros((), dtype=dtype)
    for key in COT_KEYS:
        for o, c in zip(out[key], cots.get(key) or [None] * len(out[key])):
            if c is not None:
                total = total + (o * c.to(dtype).reshape(o.shape)).sum()
    for o, c in zip(out['flow_lr'], extra or []):
        if c is not None:
            total = total + (o * c.to(dtype)).sum()
    flat = [t for key in HEAD_KEYS for t in leaves[key]]
    grads = torch.autograd.grad(total, flat, allow_unused=True) if total.requires_grad else [None] * len(flat)
    grads = [np.zeros(tuple(t.shape)) if g is None else g.numpy() for g, t in zip(grads, flat)]
    T = len(heads['masks'])
    return {key: grads[j * T:(j + 1) * T] for j, key in enumerate(HEAD_KEYS)}, out


def tail_closed_form(heads, consts, cots, flags, depth_transform, poses, extra=None, scale=8, with_bounds=False):
    """DESIGN.md section 4.5 assembled in numpy float64 from the closed forms above -> dict under HEAD_KEYS (and, with
    with_bounds, the kernels' bounds under the same keys).  poses = (rots, transs): the values R_i, t_i."""
    detach_flow, detach_pose, detach_depth = flags
    ref_rot, ref_trans, depth, k, _, _ = consts
    T = len(heads['masks'])
    n, H, W = depth.shape
    h, w = H // scale, W // scale
    get = lambda key: list(cots.get(key) or [None] * T)             # noqa: E731
    g_fpose, g_fpred, g_mask = get('flow_from_pose'), get('flow_from_pred'), get('mask_preds')
    zero = lambda *s: (np.zeros(s), np.zeros(s))                    # noqa: E731
    rs = lambda t, c: f64(t).reshape(n * c, *t.shape[-2:])          # noqa: E731
    dflow = [resize_grad_ref(rs(g, 2), (h, w), float(scale)) if g is not None else zero(n * 2, h, w) for g in g_fpred]
    gmask = [resize_grad_ref(rs(g, 1), (h, w), 1.0) if g is not None else zero(n, h, w) for g in g_mask]
    fpose = [(f64(g).reshape(n * 2, H, W), np.zeros((n * 2, H, W))) if g is not None else None for g in g_fpose]
    if not detach_flow:
        for i in range(1, T):
            src = dflow[i][0] if g_fpred[i] is not None else None
            add = None if not extra or extra[i] is None else rs(extra[i], 2)
            if src is None and add is None:
                continue
            if src is None:
                src, add = add, None
            prev = fpose[i - 1]
            ref, bound = resize_grad_ref(src, (H, W), 1.0 / scale, add=add, dst=None if prev is None else prev[0])
            if g_fpred[i] is not None:
                # the kernel reads the fp32 result of the first launch, off by at most its bound: carried through
                # |mul| U^T, and added to the magnitudes the roundings of this launch are taken on
                carried = resize_grad_ref(dflow[i][1], (H, W), 1.0 / scale)
                bound = bound + carried[0] + carried[1]
            fpose[i - 1] = (ref, bound)
    rots, transs = poses
    g_r, g_t = np.zeros((T, n, 3, 3)), np.zeros((T, n, 3))
    b_r, b_t = np.zeros((T, n, 3, 3)), np.zeros((T, n, 3))
    for i in range(T):
        if fpose[i] is not None:
            g32 = torch.from_numpy(fpose[i][0].astype(F32).reshape(n, 2, H, W))
            if with_bounds:
                s, bs = reproject_grad_ref(depth, k, ref_rot, ref_trans, rots[i], transs[i], g32)
            A, B = reproject_grad_coefs(depth, k, ref_rot, ref_trans, rots[i], transs[i])
            g = fpose[i][0].reshape(n, 2, H, W)
            exact = (A * g[:, 0:1] + B * g[:, 1:2]).reshape(n, 12, -1).sum(-1)
            if with_bounds:
                eg = (fpose[i][1] + np.abs(fpose[i][0] - fpose[i][0].astype(F32))).reshape(n, 2, H, W)
                bs = bs + np.abs(s - exact) + (np.abs(A) * eg[:, 0:1] + np.abs(B) * eg[:, 1:2]).reshape(n, 12, -1).sum(-1) * (1 + 64 * U)
                b_r[i], b_t[i] = bs[:, :9].reshape(n, 3, 3), bs[:, 9:]
            g_r[i] += exact[:, :9].reshape(n, 3, 3)
            g_t[i] += exact[:, 9:]
        for key, acc, shape in (('rotation_preds', g_r, (n, 3, 3)), ('translation_preds', g_t, (n, 3))):
            c = get(key)[i]
            if c is not None:
                acc[i] += f64(c).reshape(shape)
    stack = lambda seq: np.stack([f64(t) for t in seq])             # noqa: E731
    args = (stack(heads['delta_rotation_preds']), stack(heads['delta_translation_preds']), ref_rot, ref_trans, stack(rots),
            stack(transs), g_r, g_t, detach_pose, detach_depth, depth_transform != 'exp')
    if with_bounds:
        (gr, gr_b), (gt, gt_b) = scan_ref(*args, g_rot_bound=b_r, g_trans_bound=b_t)
    else:
        gr, gt = scan_closed_form(*args)
        gr_b, gt_b = np.zeros_like(gr), np.zeros_like(gt)
    ref = {'delta_flow_preds': [d[0].reshape(n, 2, h, w) for d in dflow], 'masks': [m[0].reshape(n, 1, h, w) for m in gmask],
           'delta_rotation_preds': list(gr), 'delta_translation_preds': list(gt)}
    bound = {'delta_flow_preds': [d[1].reshape(n, 2, h, w) for d in dflow], 'masks': [m[1].reshape(n, 1, h, w) for m in gmask],
             'delta_rotation_preds': list(gr_b), 'delta_translation_preds': list(gt_b)}
    return (ref, bound) if with_bounds else ref


def tail_case(n=3, hw=(16, 24), T=3, seed=0, scale=8):
    """head outputs, constants and cotangents of a tail: a depth map with background, a reference pose in front of the
    camera, small pose updates.  -> heads, consts, cots, extra."""
    g = torch.Generator().manual_seed(25000 + seed + hw[0] * hw[1] + T)
    H, W = hw
    h, w = H // scale, W // scale
    depth = 0.8 + 0.4 * torch.rand((n, H, W), generator=g)
    depth[torch.rand((n, H, W), generator=g) < 0.3] = 0.0
    depth[0, H // 2, W // 3] = float('nan')
    depth[-1, 1, 1] = -0.5
    k = torch.zeros((n, 3, 3))
    k[:, 0, 0], k[:, 1, 1] = 1.1 * max(H, W), 1.3 * max(H, W)
    k[:, 0, 1], k[:, 0, 2], k[:, 1, 2], k[:, 2, 2] = 0.4, 0.45 * W, 0.55 * H, 1.0
    ref_rot = rand_rot(n, g)
    ref_trans = torch.randn((n, 3), generator=g) * 0.05
    ref_trans[:, 2] = 1.0 + 0.2 * torch.rand((n,), generator=g)
    eye6 = torch.tensor([1.0, 0.0, 0.0, 0.0, 1.0, 0.0])
    heads = {'delta_flow_preds': [torch.randn((n, 2, h, w), generator=g) for _ in range(T)],
             'masks': [torch.rand((n, 1, h, w), generator=g) for _ in range(T)],
             'delta_rotation_preds': [(eye6 + 0.1 * torch.randn((n, 6), generator=g)) * (0.5 + torch.rand((n, 1), generator=g)) for _ in range(T)],
             'delta_translation_preds': [0.05 * torch.randn((n, 3), generator=g) for _ in range(T)]}
    consts = (ref_rot, ref_trans, depth, k, 0.5 * torch.randn((n, 2, H, W), generator=g), 0.0)
    cots = {'flow_from_pose': [torch.randn((n, 2, H, W), generator=g) * 1e-3 for _ in range(T)],
            'flow_from_pred': [torch.randn((n, 2, H, W), generator=g) * 1e-3 for _ in range(T)],
            'rotation_preds': [torch.randn((n, 3, 3), generator=g) for _ in range(T)],
            'translation_preds': [torch.randn((n, 3), generator=g) for _ in range(T)],
            'mask_preds': [torch.randn((n, 1, H, W), generator=g) * 1e-3 for _ in range(T)]}
    extra = [torch.randn((n, 2, h, w), generator=g) * 1e-2 for _ in range(T)]
    return heads, consts, cots, extra


def stored_poses(heads, consts, flags, depth_transform):
    """the fp32 poses of an exact forward of the case (what the GPU forward would have stored, up to its own rounding)."""
    return pose_forward64(heads['delta_rotation_preds'], heads['delta_translation_preds'], consts[0], consts[1],
                          depth_transform != 'exp')


def rel_err(got, ref):
    got, ref = f64(got), f64(ref)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300)) if ref.size else 0.0


# ===================================================================================================== the self-checks
@pytest.mark.parametrize('depth_transform', ['exp', 'linear'])
@pytest.mark.parametrize('flags', FLAG_COMBOS)
def test_closed_forms_equal_float64_autograd(flags, depth_transform):
    heads, consts, cots, extra = tail_case()
    poses = stored_poses(heads, consts, flags, depth_transform)
    for ex in (None, extra):
        want, _ = tail_vjp(heads, consts, cots, flags, depth_transform, extra=ex, stored=poses)
        got = tail_closed_form(heads, consts, cots, flags, depth_transform, poses, extra=ex)
        for key in HEAD_KEYS:
            for i, (a, b) in enumerate(zip(got[key], want[key])):
                assert rel_err(a, b.reshape(a.shape)) <= 1e-12, (key, i, rel_err(a, b.reshape(a.shape)))


@pytest.mark.parametrize('depth_transform', ['exp', 'linear'])
@pytest.mark.parametrize('flags', FLAG_COMBOS)
def test_scan_closed_form_equals_float64_autograd(flags, depth_transform):
    """the scan alone: cotangents on the poses only."""
    heads, consts, cots, _ = tail_case()
    poses = stored_poses(heads, consts, flags, depth_transform)
    only = {key: cots[key] for key in ('rotation_preds', 'translation_preds')}
    want, _ = tail_vjp(heads, consts, only, flags, depth_transform, stored=poses)
    got = tail_closed_form(heads, consts, only, flags, depth_transform, poses)
    for key in ('delta_rotation_preds', 'delta_translation_preds'):
        for a, b in zip(got[key], want[key]):
            assert rel_err(a, b) <= 1e-12


@pytest.mark.parametrize('flags', [(True, True, False), (False, False, False)])
def test_reprojection_and_resize_closed_forms_equal_float64_autograd(flags):
    """cotangents on the pose-induced flow and the mask only, with a caller's cotangent of flow_lr."""
    heads, consts, cots, extra = tail_case()
    poses = stored_poses(heads, consts, flags, 'exp')
    only = {'flow_from_pose': cots['flow_from_pose'], 'mask_preds': cots['mask_preds']}
    want, _ = tail_vjp(heads, consts, only, flags, 'exp', extra=extra, stored=poses)
    got = tail_closed_form(heads, consts, only, flags, 'exp', poses, extra=extra)
    for key in HEAD_KEYS:
        for a, b in zip(got[key], want[key]):
            assert rel_err(a, b.reshape(a.shape)) <= 1e-12, key


RESIZE_HOST = [s for s in RESIZE_SIZES if s[0] <= 8] + [(2, (4, 4), (32, 32))]


@pytest.mark.parametrize('planes,in_hw,out_hw', RESIZE_HOST)
def test_resize_adjoint_replay_lies_inside_the_bound(planes, in_hw, out_hw):
    planes = min(planes, 3)
    g = resize_grad_case(planes, out_hw)
    add, dst = resize_grad_case(planes, out_hw, seed=1), resize_grad_case(planes, in_hw, seed=2)
    worst = 0.0
    for kw in (dict(mul=1.0), dict(mul=8.0), dict(mul=0.125, add=add), dict(mul=-3.7, dst=dst)):
        ref, bound = resize_grad_ref(g, in_hw, **kw)
        worst = max(worst, worst_ratio(resize_grad_fp32(g, in_hw, **kw), ref, bound))
    measured(f'resize adjoint replay {in_hw}->{out_hw}', worst)
    assert worst <= 1.0
    # the adjoint identity in float64: <U a, g> = <a, U^T g>
    a = f64(resize_grad_case(planes, in_hw, seed=3))
    fwd = np.einsum('oi,pij,xj->pox', interp_matrix(in_hw[0], out_hw[0]), a, interp_matrix(in_hw[1], out_hw[1]))
    assert abs((fwd * f64(g)).sum() - (a * resize_grad_ref(g, in_hw)[0]).sum()) <= 1e-11 * np.abs(fwd * f64(g)).sum() + 1e-300


def test_resize_adjoint_defects_fall_outside():
    g = resize_grad_case(3, (5, 3))
    ref, bound = resize_grad_ref(g, (3, 5), 2.0)
    assert worst_ratio(resize_grad_fp32(g, (3, 5), 2.0), ref, bound) <= 1.0
    assert worst_ratio(resize_grad_fp32(g, (3, 5), 2.0, defect='forward_matrix'), ref, bound) > 1e3     # U for U^T, 15 x 15
    g = resize_grad_case(3, (16, 24))
    ref, bound = resize_grad_ref(g, (2, 3), 8.0)
    assert worst_ratio(resize_grad_fp32(g, (2, 3), 8.0, defect='no_mul'), ref, bound) > 1e3
    # the clamped +1 tap carries a weight only where the fp32 coordinate lands past the last node: one ulp of it
    n_in, n_out = find_edge_excess()
    g = torch.zeros((2, 1, n_out))
    g[:, :, -1] = torch.tensor([1.0, -2.75])[:, None]              # the last column alone: nothing else reaches its bound
    ref, bound = resize_grad_ref(g, (1, n_in), 1.0)
    assert worst_ratio(resize_grad_fp32(g, (1, n_in), 1.0), ref, bound) <= 1.0
    r = worst_ratio(resize_grad_fp32(g, (1, n_in), 1.0, defect='edge_tap'), ref, bound)
    measured(f'edge tap dropped at ({n_in}) -> ({n_out})', r)
    assert r > 1.0


GEOM_HOST = [(pose, size, skew) for pose in ('identity', 'large_rotation') for size in GEOM_SIZES[:3] for skew in (True, False)]


def reproject_grad_case(pose, size, skew, seed=0):
    depth, k, rot0, trans0, rot, trans = geom_case(pose, size, skew)
    g = torch.Generator().manual_seed(27000 + seed + size[1] * size[2])
    return depth, k, rot0, trans0, rot, trans, torch.randn((size[0], 2, *size[1:]), generator=g)


@pytest.mark.parametrize('pose,size,skew', GEOM_HOST)
def test_reprojection_replay_lies_inside_the_bound(pose, size, skew):
    case = reproject_grad_case(pose, size, skew)
    ref, bound = reproject_grad_ref(*case)
    assert np.isfinite(bound).all()
    r = worst_ratio(reproject_grad_fp32(*case), ref, bound)
    measured(f'reprojection sums replay {pose} {size}', r)
    assert r <= 1.0
    A, B = reproject_grad_coefs(*case[:6])
    g = f64(case[6])
    exact = (A * g[:, 0:1] + B * g[:, 1:2]).reshape(size[0], 12, -1).sum(-1)
    assert np.abs(exact - ref).max() <= 1e-9 * max(np.abs(ref).max(), 1e-30)


def test_through_camera_leaves_out_the_planted_sample_only():
    """the sample holding the run of pixels with qz ~ 0 has no finite bound; every other sample has one, and the replay
    lies inside it."""
    case = reproject_grad_case('through_camera', (3, 12, 20), True)
    ref, bound = reproject_grad_ref(*case)
    finite = np.isfinite(bound).all(1)
    assert finite.tolist() == [False, True, True]
    assert worst_ratio(reproject_grad_fp32(*case)[finite], ref[finite], bound[finite]) <= 1.0


@pytest.mark.parametrize('defect', ['background', 'K_not_transposed', 'qz2_sign'])
def test_reprojection_defects_fall_outside(defect):
    case = reproject_grad_case('large_rotation', (3, 12, 20), True)
    ref, bound = reproject_grad_ref(*case)
    assert worst_ratio(reproject_grad_fp32(*case, defect=defect), ref, bound) > 1e2


def _scan_inputs(regime, n, T, linear):
    d_rots, d_transs, rot0, trans0, g_rot, g_trans = scan_case(regime, n, T)
    rots, transs = pose_forward64(d_rots, d_transs, rot0, trans0, linear)
    return torch.stack(d_rots), torch.stack(d_transs), rot0, trans0, torch.stack(rots), torch.stack(transs), g_rot, g_trans


@pytest.mark.parametrize('regime', [r for r in POSE_REGIMES if r not in ('zero_a', 'parallel')])
def test_scan_replay_lies_inside_the_bound_and_defects_outside(regime):
    for linear in (False, True):
        args = _scan_inputs(regime, 5, 4, linear)
        for detach_pose, detach_depth in itertools.product([False, True], repeat=2):
            kw = dict(detach_pose=detach_pose, detach_depth=detach_depth, linear=linear)
            (rr, rb), (tr, tb) = scan_ref(*args, **kw)
            got_r, got_t = scan_closed_form(*args, **kw)
            assert worst_ratio(got_r.astype(F32), rr, rb) <= 1.0 and worst_ratio(got_t.astype(F32), tr, tb) <= 1.0
            if regime != 'nominal':
                continue
            defects = ['carry_when_detached'] if detach_pose else ['no_carry', 'rd_not_transposed']
            defects += ['vz_not_detached'] if detach_depth else []
            defects += ['exp_on_linear'] if linear else []
            for defect in defects:
                bad_r, bad_t = scan_closed_form(*args, **kw, defect=defect)
                r = max(worst_ratio(bad_r.astype(F32), rr, rb), worst_ratio(bad_t.astype(F32), tr, tb))
                assert r > 1e2, (defect, r)


DEGENERATE_PATTERNS = {}


@pytest.mark.parametrize('regime', ['zero_a', 'parallel'])
def test_degenerate_rotations_record_what_autograd_gives(regime):
    """a = 0: x = 0 / 1e-12 = 0, so R_d = 0, d / db = 0 exactly and d / da = g_x / 1e-12 (finite); a || b: x X b is 0 or
    rounding noise below 1e-12, z = (x X b) / 1e-12, every gradient finite.  The closed form shows the pattern autograd
    shows; tests/test_gpu_tail_grad.py holds the kernel to it."""
    d_rot, d_trans, rot0, trans0, rots, transs, g_rot, g_trans = _scan_inputs(regime, 5, 4, False)
    heads = {'delta_flow_preds': [torch.zeros((5, 2, 1, 1))] * 4, 'masks': [torch.zeros((5, 1, 1, 1))] * 4,
             'delta_rotation_preds': list(d_rot), 'delta_translation_preds': list(d_trans)}
    consts = (rot0, trans0, torch.zeros((5, 8, 8)), torch.eye(3).repeat(5, 1, 1), torch.zeros((5, 2, 8, 8)), 0.0)
    cots = {'rotation_preds': list(g_rot), 'translation_preds': list(g_trans)}
    want, _ = tail_vjp(heads, consts, cots, (True, False, False), 'exp', stored=(list(rots), list(transs)))
    got_r, got_t = scan_closed_form(d_rot, d_trans, rot0, trans0, rots, transs, g_rot, g_trans, False, False, False)
    auto_r = np.stack(want['delta_rotation_preds'])
    assert np.isfinite(auto_r).all() and np.isfinite(got_r).all()
    assert np.array_equal(auto_r == 0, got_r == 0)
    if regime == 'zero_a':
        assert (auto_r[..., 3:] == 0).all() and (auto_r[0][..., :3] != 0).all()     # R_i = 0 for i >= 1: zeros there
        assert rel_err(got_r, auto_r) <= 1e-12
    assert rel_err(got_t, np.stack(want['delta_translation_preds'])) <= 1e-12


def test_tail_bounds_hold_for_the_fp32_restatement_and_golden():
    """tail_grads.npz: autograd through the reference's own functions in fp32 (make_golden_tail_grad.py).  The float64
    restatement is held to it with room = the kernels' bound + torch's own fp32 terms (an fp32 forward and backward of
    the same expressions: 64 U of the magnitude shadow of each result, taken as the largest magnitude of its tensor)."""
    z = np.load(GOLDEN)
    heads = {key: [torch.from_numpy(a) for a in z[key]] for key in HEAD_KEYS}
    consts = (torch.from_numpy(z['ref_rot']), torch.from_numpy(z['ref_trans']), torch.from_numpy(z['depth']),
              torch.from_numpy(z['k']), torch.from_numpy(z['init_flow']), 0.0)
    cots = {key: [torch.from_numpy(a) for a in z['cot_' + key]] for key in COT_KEYS}
    case = tail_case()
    for key in HEAD_KEYS:                                           # the recorded inputs are the seeded ones
        assert all(torch.equal(a, b) for a, b in zip(heads[key], case[0][key]))
    worst = 0.0
    for tag, flags in (('shipped', (True, True, False)), ('free', (False, False, False))):
        for depth_transform in ('exp', 'linear'):
            poses = ([torch.from_numpy(a) for a in z[f'{tag}_{depth_transform}_rot']],
                     [torch.from_numpy(a) for a in z[f'{tag}_{depth_transform}_trans']])
            want, _ = tail_vjp(heads, consts, cots, flags, depth_transform, stored=poses)
            _, bound = tail_closed_form(heads, consts, cots, flags, depth_transform, poses, with_bounds=True)
            for key in HEAD_KEYS:
                rec = z[f'{tag}_{depth_transform}_{key}']
                for i in range(len(rec)):
                    ref = want[key][i].reshape(rec[i].shape)
                    room = bound[key][i].reshape(rec[i].shape) + 64 * U * np.abs(ref).max()
                    worst = max(worst, worst_ratio(rec[i], ref, room))
    measured('reference fp32 autograd against the float64 restatement / room', worst)
    assert worst <= 1.0


def test_decoder_stores_the_autograd_switches_and_raft_refiners_get_nothing():
    import scflow_amd
    from scflow_amd import refiner
    cfg = scflow_amd.scflow_model_cfg(iters=1)
    cfg['decoder'] = dict(cfg['decoder'], detach_flow=False, detach_pose=True)
    dec = scflow_amd.build_refiner(cfg).decoder
    assert (dec.detach_flow, dec.detach_pose, dec.detach_depth_for_xy) == (False, True, cfg['decoder']['detach_depth_for_xy'])
    assert callable(dec.tail_backward) and hasattr(refiner.SCFlowRefiner, 'loss_and_head_grads')
    # their tail is the convex up-sampling: a different adjoint
    assert not hasattr(refiner.RAFTRefinerFlowMask, 'loss_and_head_grads') and not hasattr(refiner.RAFTRefinerFlow, 'loss_and_head_grads')
