"""CPU: the pose step of the pose-free RAFT refiners (batched RANSAC-EPnP, scflow_amd/csrc/pnp.hip) -- the
correspondence fixture against an in-test torch restatement, mode selection, parameter validation and the C ABI."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import scflow_amd
from scflow_amd import _lib, ops


def _fixture(golden_dir):
    return np.load(os.path.join(golden_dir, 'corr_2d3d.npz'))


def _corr_restated(flow, depth, k, rot, trans, mask=None):
    """get_2d_3d_corr_by_fw_flow (models/utils/pose.py:182-200) restated in torch: per sample the pixels with
    depth > 0 (& mask), row-major, -> (source pixels, target points, object-frame points)."""
    out = []
    for i in range(len(flow)):
        m = depth[i] > 0
        if mask is not None:
            m = m & mask[i]
        ys, xs = torch.nonzero(m, as_tuple=True)
        d = depth[i][m]
        src = torch.stack([xs, ys], dim=-1).float()
        homo = torch.stack([src[:, 0], src[:, 1], torch.ones_like(src[:, 0])], dim=-1) * d[:, None]
        cam = torch.mm(torch.inverse(k[i]), homo.t()).t()
        obj = torch.mm(torch.inverse(rot[i]), (cam - trans[i][None]).t()).t()
        tgt = src + flow[i][:, ys, xs].t()
        out.append((src, tgt, obj))
    return out


@pytest.mark.parametrize('case', ['a', 'b'])
@pytest.mark.parametrize('tag', ['nomask', 'mask'])
def test_corr_restatement_matches_fixture(golden_dir, case, tag):
    g = _fixture(golden_dir)
    f = lambda k: torch.from_numpy(g[f'{case}_{k}'])      # noqa: E731
    flow = f('flow16').float() / 16
    occ = f('occ8').float() / 8
    corr = _corr_restated(flow, f('depth'), f('k'), f('rot'), f('trans'), occ > 0.5 if tag == 'mask' else None)
    assert [len(c[0]) for c in corr] == g[f'{case}_{tag}_count'].tolist()
    src = torch.cat([c[0] for c in corr])
    assert torch.equal(src, f(f'{tag}_src').float())
    step = int(g[f'{case}_{tag}_row_step'])
    torch.testing.assert_close(torch.cat([c[1] for c in corr])[::step], f(f'{tag}_pts2d'), rtol=1e-6, atol=1e-5)
    torch.testing.assert_close(torch.cat([c[2] for c in corr])[::step], f(f'{tag}_pts3d'), rtol=1e-5, atol=1e-3)
    if case == 'a' and tag == 'mask':
        assert int(g['a_mask_count'][-1]) == 0               # the empty-mask sample


def _raft(test_cfg):
    cfg = scflow_amd.raft_model_cfg(iters=2)
    cfg['test_cfg'] = dict(iters=2, **test_cfg)
    return scflow_amd.build_refiner(cfg)


def test_hip_mode_builds_and_cv2_modes_raise():
    m = _raft(dict(solve_pose_mode='hip_ransac_epnp', solve_pose_param=dict(iterationscount=50, reprojectionerror=2.0),
                   sample_points=dict(num=500, mode='topk')))
    assert type(m).__name__ == 'RAFTRefinerFlowMask'
    kw = m._pnp_kwargs()
    assert kw == dict(iterations=50, reproj_error=2.0, seed=0, sample_mode='topk', sample_num=500)
    for mode in ('ransacpnp', None, 'progressive-x', 'magic'):
        m = _raft({} if mode is None else dict(solve_pose_mode=mode))
        with pytest.raises(NotImplementedError, match='hip_ransac_epnp'):
            m.solve_pose()
    f = scflow_amd.build_refiner(dict(scflow_amd.raft_model_cfg(iters=2), type='RAFTRefinerFlow',
                                      decoder=dict(scflow_amd.raft_model_cfg()['decoder'], type='RAFTDecoder')))
    with pytest.raises(NotImplementedError):
        f.solve_pose()


def test_remap_modes():
    m = _raft(dict(solve_pose_mode='hip_ransac_epnp'))
    r, t = [torch.eye(3)[None]], [torch.zeros((1, 3))]
    assert m._remap_pose(r, t, None) == (r, t)
    assert m._remap_pose(r, t, [dict(geometry_transform_mode='adapt_intrinsic')]) == (r, t)
    with pytest.raises(NotImplementedError):
        m._remap_pose(r, t, [dict(geometry_transform_mode='target_intrinsic')])


@pytest.mark.parametrize('bad', [dict(iterations=0), dict(iterations=-3), dict(iterations=2.5),
                                 dict(reproj_error=-1.0), dict(reproj_error=float('nan')),
                                 dict(reproj_error=float('inf')), dict(sample_mode='first'),
                                 dict(sample_mode='topk', sample_num=0), dict(seed=-1)])
def test_bad_parameters_rejected(bad):
    with pytest.raises(_lib.ScflowHipError):
        ops.pnp_params(**bad)


def test_bad_parameters_rejected_by_solve_pose_before_any_launch():
    for prm in (dict(iterationscount=0), dict(reprojectionerror=-0.5)):
        m = _raft(dict(solve_pose_mode='hip_ransac_epnp', solve_pose_param=prm))
        with pytest.raises(_lib.ScflowHipError):
            m.solve_pose()


def test_cabi_symbols_version_and_host_validation():
    lib = _lib.load()
    for name in ('scf_flow_corr_2d3d', 'scf_pnp_ransac', 'scf_pnp_workspace_bytes'):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.scf_version() % 100 == 3
    assert C.sizeof(_lib.PnpParams) == 24
    ok = _lib.PnpParams(100, 3.0, _lib.PNP_SAMPLE_ALL, 0, 0)
    assert lib.scf_pnp_workspace_bytes(4, 1000, C.byref(ok)) == 0
    topk = _lib.PnpParams(100, 3.0, _lib.PNP_SAMPLE_TOPK, 10, 0)
    assert lib.scf_pnp_workspace_bytes(4, 1000, C.byref(topk)) >= 4 * 1000 * 4 + 4 * 4
    for bad in (_lib.PnpParams(0, 3.0, 0, 0, 0), _lib.PnpParams(10, -1.0, 0, 0, 0),
                _lib.PnpParams(10, 3.0, 7, 0, 0), _lib.PnpParams(10, 3.0, _lib.PNP_SAMPLE_RANDOM, 0, 0)):
        assert lib.scf_pnp_workspace_bytes(4, 1000, C.byref(bad)) == -1
    # argument checks return before any launch: no device needed
    assert lib.scf_pnp_ransac(None, None, None, None, 1, 1, None, None, None, C.byref(ok),
                              None, None, None, None, None, None) == -1
    assert lib.scf_flow_corr_2d3d(None, None, None, 0.5, None, None, None, 1, 1, 1, None, None, None, None, None) == -1


# ------------------------------------------------------------------ float64 restatement of scf_pnp_ransac
# Written from the contract in include/scflow_hip.h (the scf_pnp_ransac block) and from EPnP (Lepetit,
# Moreno-Noguer, Fua, IJCV 2009), not from pnp.hip, so that a mistake shared with the kernel cannot cancel: the
# null space comes from an SVD of the explicit 2N x 12 matrix M (the kernel: Jacobi on accumulated M^T M), the
# barycentric coordinates from a 4 x 4 solve, every least-squares step from a pseudo-inverse (the kernel: normal
# equations) and the pose from Kabsch's SVD alignment of the camera-frame points (the kernel: Horn's quaternion).
_U64 = np.uint64
_SEL_SALT = 0x5e1ec7
# the ten products of the four betas, in the column order of L (6 x 10): b11 b12 b22 b13 b23 b33 b14 b24 b34 b44
_QUAD = [(0, 0), (0, 1), (1, 1), (0, 2), (1, 2), (2, 2), (0, 3), (1, 3), (2, 3), (3, 3)]
_PAIRS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
# Lepetit's approximations: the L columns each one solves for (over 4, 2 and 3 null vectors)
_CASE_COLS = ([0, 1, 3, 6], [0, 1, 2], [0, 1, 2, 3, 4])
# Ambiguity band of the fp32 inlier test.  The GPU evaluates q = P X (three 4-term fp32 dot products, contracted to
# FMAs or not), u = qx / qz, du = u - u_obs and du^2 + dv^2 against fp32(thr^2).  Each dot product is off by at most
# ~4 roundings of the sum of its terms' magnitudes S; a one-ulp difference in an entry of P (the GPU's fp64 solve
# rounding to the other side of an fp32 boundary) adds one more.  _GAMMA = 8 units of 2^-24 covers both with room,
# so |u_gpu - u| <= _GAMMA (Sx + |u| Sz) / |qz| + 2^-24 (|u| + |du|), and from there to du^2 + dv^2.  At a 256-px
# image with P near 500 px focal length that is ~1e-4 px; a point inside the band may fall either way on the GPU.
_GAMMA = 8 * 2.0 ** -24


def pnp_mix(z):
    """the splitmix64 finaliser (Steele, Lea, Flood 2014) with its increment: pnp_mix(0) is SplitMix64's first
    output for state 0.  uint64 arrays in, uint64 arrays out (wrapping arithmetic)."""
    z = np.asarray(z, dtype=_U64)
    with np.errstate(over='ignore'):
        z = z + _U64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> _U64(30))) * _U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _U64(27))) * _U64(0x94D049BB133111EB)
        return z ^ (z >> _U64(31))


def pnp_hash(seed, a, b):
    """the counter-based hash of (seed, a, b): mix(mix(mix(seed) ^ a) ^ b)"""
    return pnp_mix(pnp_mix(pnp_mix(_U64(seed)) ^ np.asarray(a, dtype=_U64)) ^ np.asarray(b, dtype=_U64))


def pnp_select(conf, count, capacity, mode, num, seed):
    """the kept point indices (ascending) of one sample: mode None (ALL), 'topk' or 'random'"""
    cnt = min(max(int(count), 0), int(capacity))
    if mode is None or num > cnt:
        return np.arange(cnt)
    if mode == 'topk':
        elig = cnt
        c = np.asarray(conf[:cnt], dtype=np.float64) + 0.0           # -0.0 + 0.0 = +0.0: the zeros tie
        nan = np.isnan(c)
        c[nan] = 0.0
        order = np.lexsort((np.arange(cnt), -c, ~nan))              # NaN first, then descending, then lower index
    else:
        elig = max(cnt - 1, 0)                                        # randperm(count - 1): never the last point
        key = (pnp_hash(seed, _SEL_SALT, np.arange(elig, dtype=_U64)) >> _U64(32)).astype(np.int64)
        order = np.lexsort((np.arange(elig), -key))
    return np.sort(order[:min(int(num), elig)])


def pnp_draws(seed, iterations, m):
    """hypothesis h draws a = 1..64 give hash(seed, h, a) % m; repeats are skipped until 5 distinct points are
    drawn, else the hypothesis is invalid -> (idx (H, 5), drawn (H,))"""
    j = pnp_hash(seed, np.arange(iterations, dtype=_U64)[:, None], np.arange(1, 65, dtype=_U64)[None]) % _U64(m)
    idx = np.zeros((iterations, 5), dtype=np.int64)
    drawn = np.zeros(iterations, dtype=bool)
    for h in range(iterations):
        u = list(dict.fromkeys(j[h].tolist()))[:5]
        if len(u) == 5:
            idx[h], drawn[h] = u, True
    return idx, drawn


def epnp_control(pw, scale='std'):
    """EPnP control points of each point set pw (H, n, 3): the centroid, and the centroid plus sqrt(variance) along
    each principal axis (axes oriented so their largest-magnitude component is positive).  -> (ok (H,), cw (H, 4, 3),
    alphas (H, n, 4)); not ok when collinear or planar: smallest variance <= 1e-8 of the largest.  scale='n' puts the
    control points at sqrt(variance / n) instead (a sensitivity probe, not the contract)."""
    h, n = pw.shape[:2]
    c0 = pw.mean(1)
    d = pw - c0[:, None]
    w, V = np.linalg.eigh(np.einsum('hni,hnj->hij', d, d) / n)
    with np.errstate(invalid='ignore'):
        ok = (w[:, 2] > 0) & (w[:, 0] > 1e-8 * w[:, 2])
    big = np.take_along_axis(V, np.abs(V).argmax(1)[:, None, :], 1)
    V = V * np.where(big < 0, -1.0, 1.0)
    s = np.sqrt(np.maximum(w, 0.0) / (n if scale == 'n' else 1))
    cw = np.concatenate([c0[:, None], c0[:, None] + (V * s[:, None, :]).transpose(0, 2, 1)], 1)
    A = np.concatenate([cw.transpose(0, 2, 1), np.ones((h, 1, 4))], 1)
    A[~ok] = np.eye(4)
    b = np.concatenate([pw, np.ones((h, n, 1))], 2).transpose(0, 2, 1)
    return ok, cw, np.linalg.solve(A, b).transpose(0, 2, 1)


def _betas(B, cs):
    """Lepetit's betas from the linearised solution B of approximation cs"""
    beta = np.zeros((len(B), 4))
    neg = B[:, 0] < 0
    b0 = np.sqrt(np.abs(B[:, 0]))
    if cs == 0:
        beta[:, 0] = b0
        with np.errstate(divide='ignore', invalid='ignore'):
            beta[:, 1:] = np.where(b0[:, None] > 0, B[:, 1:] / b0[:, None] * np.where(neg, -1.0, 1.0)[:, None], 0.0)
        return beta
    beta[:, 0] = np.where(B[:, 1] < 0, -b0, b0)
    beta[:, 1] = np.where(neg, np.sqrt(np.maximum(-B[:, 2], 0.0)), np.sqrt(np.maximum(B[:, 2], 0.0)))
    if cs == 2:
        with np.errstate(divide='ignore', invalid='ignore'):
            beta[:, 2] = np.where(beta[:, 0] != 0, B[:, 3] / beta[:, 0], 0.0)
    return beta


def epnp(pw, uv, K, scale='std', gn_steps=5, cases=(0, 1, 2)):
    """EPnP on each of H correspondence sets: pw (H, n, 3) object points, uv (H, n, 2) pixels, K (3, 3); float64.
    -> dict(ok (H,), R (H, 3, 3), t (H, 3), case (H,), Rc (H, 3, 3, 3), tc (H, 3, 3), err (H, 3)): per case c the
    pose of Lepetit's approximation c followed by gn_steps Gauss-Newton steps on the six control-point distances;
    err the summed pixel reprojection distance (inf when not finite); the case of lowest err is kept (ties: lower)."""
    pw, uv, K = np.asarray(pw, np.float64), np.asarray(uv, np.float64), np.asarray(K, np.float64)
    h, n = pw.shape[:2]
    ray = np.concatenate([uv, np.ones((h, n, 1))], -1) @ np.linalg.inv(K).T
    x, y = ray[..., 0] / ray[..., 2], ray[..., 1] / ray[..., 2]
    ok, cw, al = epnp_control(pw, scale)
    M = np.zeros((h, 2 * n, 12))
    M[:, 0::2, 0::3], M[:, 0::2, 2::3] = al, -al * x[..., None]
    M[:, 1::2, 1::3], M[:, 1::2, 2::3] = al, -al * y[..., None]
    M[~ok] = np.eye(2 * n, 12)
    vt = np.linalg.svd(M, full_matrices=2 * n < 12)[2]
    vv = vt[:, ::-1][:, :4].reshape(h, 4, 4, 3)                 # v_k, k = 0..3 by ascending singular value
    L, rho = np.zeros((h, 6, 10)), np.zeros((h, 6))
    for r, (a, b) in enumerate(_PAIRS):
        dv = vv[:, :, a] - vv[:, :, b]
        G = np.einsum('hkd,hld->hkl', dv, dv)
        for c, (k, l) in enumerate(_QUAD):
            L[:, r, c] = G[:, k, l] * (1 if k == l else 2)
        rho[:, r] = ((cw[:, a] - cw[:, b]) ** 2).sum(-1)
    Rc, tc, err = np.zeros((h, 3, 3, 3)), np.zeros((h, 3, 3)), np.full((h, 3), np.inf)
    for cs in cases:
        beta = _betas((np.linalg.pinv(L[:, :, _CASE_COLS[cs]]) @ rho[..., None])[..., 0], cs)
        for _ in range(gn_steps):
            J = np.zeros((h, 6, 4))
            fit = np.zeros((h, 6))
            for c, (k, l) in enumerate(_QUAD):
                fit += L[:, :, c] * (beta[:, k] * beta[:, l])[:, None]
                J[:, :, k] += L[:, :, c] * beta[:, l, None]
                J[:, :, l] += L[:, :, c] * beta[:, k, None]
            beta = beta + (np.linalg.pinv(J) @ (rho - fit)[..., None])[..., 0]
        ccs = np.einsum('hk,hkjd->hjd', beta, vv)
        pc = np.einsum('hnj,hjd->hnd', al, ccs)
        pc = pc * np.where(pc[..., 2].mean(1) < 0, -1.0, 1.0)[:, None, None]   # the object lies in front
        mw, mc = pw.mean(1), pc.mean(1)
        U, _, Wt = np.linalg.svd(np.einsum('hni,hnj->hij', pw - mw[:, None], pc - mc[:, None]))
        D = np.ones((h, 3))
        D[:, 2] = np.sign(np.linalg.det(Wt.transpose(0, 2, 1) @ U.transpose(0, 2, 1)))
        R = Wt.transpose(0, 2, 1) @ (D[..., None] * U.transpose(0, 2, 1))
        t = mc - np.einsum('hij,hj->hi', R, mw)
        q = (np.einsum('hij,hnj->hni', R, pw) + t[:, None]) @ K.T
        with np.errstate(all='ignore'):
            e = np.sqrt(((q[..., :2] / q[..., 2:] - uv) ** 2).sum(-1)).sum(-1)
        Rc[:, cs], tc[:, cs] = R, t
        err[:, cs] = np.where(np.isfinite(e) & np.isfinite(R).all((1, 2)) & np.isfinite(t).all(1), e, np.inf)
    case = np.argmin(err, 1)
    ok = ok & np.isfinite(err.min(1))
    return dict(ok=ok, R=Rc[np.arange(h), case], t=tc[np.arange(h), case], case=case, Rc=Rc, tc=tc, err=err)


def proj32(K, R, t):
    """P = K [R | t] rounded to fp32, (..., 3, 4)"""
    return (np.asarray(K, np.float64) @ np.concatenate([R, t[..., None]], -1)).astype(np.float32)


def pnp_score(P32, pts2d, pts3d, thr):
    """fp32 inlier test of every point under each fp32 P (H, 3, 4), evaluated in fp64 -> (inlier (H, m),
    ambiguous (H, m)): inlier = qz > 0 and du^2 + dv^2 < thr^2 (NaN: outlier); ambiguous = inside the band of
    _GAMMA where fp32 rounding may decide either way (see _GAMMA)."""
    P = np.asarray(P32, np.float64)
    X, uv = np.asarray(pts3d, np.float64), np.asarray(pts2d, np.float64)
    thr2 = float(thr) ** 2
    with np.errstate(all='ignore'):
        q = np.einsum('hij,mj->him', P[:, :, :3], X) + P[:, :, 3:]
        S = np.einsum('hij,mj->him', np.abs(P[:, :, :3]), np.abs(X)) + np.abs(P[:, :, 3:])
        qz = q[:, 2]
        u, v = q[:, 0] / qz, q[:, 1] / qz
        du, dv = u - uv[:, 0], v - uv[:, 1]
        d2 = du * du + dv * dv
        inl = (qz > 0) & (d2 < thr2)
        u32 = 2.0 ** -24
        eu = _GAMMA * (S[:, 0] + np.abs(u) * S[:, 2]) / np.abs(qz) + u32 * (np.abs(u) + np.abs(du))
        ev = _GAMMA * (S[:, 1] + np.abs(v) * S[:, 2]) / np.abs(qz) + u32 * (np.abs(v) + np.abs(dv))
        e2 = 2 * (np.abs(du) * eu + np.abs(dv) * ev) + eu * eu + ev * ev + 3 * u32 * (d2 + thr2)
        zband = np.abs(qz) <= _GAMMA * S[:, 2]
        amb = zband | ((qz > 0) & (np.abs(d2 - thr2) <= e2))
    return inl, amb


def _score_chunked(P32, pts2d, pts3d, thr, chunk=32):
    cnt, amb = np.zeros(len(P32), np.int64), np.zeros(len(P32), np.int64)
    for i in range(0, len(P32), chunk):
        a, b = pnp_score(P32[i:i + chunk], pts2d, pts3d, thr)
        cnt[i:i + chunk], amb[i:i + chunk] = a.sum(1), b.sum(1)
    return cnt, amb


def _refit(P32w, p2, p3, K, thr, scale='std', gn_steps=5, drop_one=False):
    """the final step from the winner's fp32 P: EPnP over its inliers, re-scored under the refit's fp32 P"""
    inl, amb_w = pnp_score(P32w[None], p2, p3, thr)
    inl = inl[0]
    if drop_one:
        inl = inl.copy()
        inl[np.flatnonzero(inl)[0]] = False
    out = dict(ok=0, amb_winner=int(amb_w.sum()), refit_set=np.flatnonzero(inl))
    if inl.sum() < 5:
        return out
    s = epnp(p3[inl][None].astype(np.float64), p2[inl][None].astype(np.float64), K, scale, gn_steps)
    R, t = s['R'][0], s['t'][0]
    P = proj32(K, R, t)
    if not (s['ok'][0] and np.isfinite(R.astype(np.float32)).all() and np.isfinite(t.astype(np.float32)).all()
            and np.isfinite(P).all()):
        return out
    fin, amb = pnp_score(P[None], p2, p3, thr)
    out.update(ok=1, R=R, t=t, inliers=int(fin.sum()), amb=int(amb.sum()))
    return out


def pnp_reference(pts2d, pts3d, conf, count, K, R_ref, t_ref, iterations=100, reproj_error=3.0, sample_mode=None,
                  sample_num=1000, seed=0, scale='std', gn_steps=5, drop_one=False, candidates=True,
                  dtype=np.float32, extra=0):
    """scf_pnp_ransac for one sample, in float64 from the header contract.  pts2d (C, 2), pts3d (C, 3), conf (C,)
    fp32 arrays of capacity C, count an int, K / R_ref (3, 3), t_ref (3,).
    -> dict(R, t, ok, inliers) plus diagnostics: winner h, counts / amb (per hypothesis), amb_final (points of the
    final re-score inside the band), margin (winner count minus the best other hypothesis'), cands {h: refit} for
    every hypothesis that could win on the GPU (see _GAMMA) -- the winner's own refit included.  scale, gn_steps
    and drop_one perturb the final refit (sensitivity probes); dtype=np.float64 keeps fp64 inputs as they are."""
    pts2d = np.asarray(pts2d, dtype)
    pts3d = np.asarray(pts3d, dtype)
    K = np.asarray(K, dtype).astype(np.float64)
    capacity = len(pts2d)
    fail = dict(R=np.asarray(R_ref, np.float64), t=np.asarray(t_ref, np.float64), ok=0, inliers=0, winner=-1,
                amb_final=0, margin=0, cands={})
    cnt = min(max(int(count), 0), capacity)
    sel = pnp_select(conf, count, capacity, sample_mode, sample_num, seed)
    m = len(sel)
    if cnt < 4 or m < 5:
        return fail
    p2, p3 = pts2d[sel], pts3d[sel]
    idx, valid = pnp_draws(seed, iterations, m)
    with np.errstate(invalid='ignore'):
        valid &= np.isfinite(p2[idx]).all((1, 2)) & np.isfinite(p3[idx]).all((1, 2))
    dummy = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1]], np.float64)
    pw = np.where(valid[:, None, None], p3[idx].astype(np.float64), dummy)
    uv = np.where(valid[:, None, None], p2[idx].astype(np.float64), dummy[:, :2])
    s = epnp(pw, uv, K)
    P32 = proj32(K, s['R'], s['t'])
    valid &= s['ok'] & np.isfinite(P32).all((1, 2))
    counts, amb = _score_chunked(P32, p2, p3, reproj_error)
    counts[~valid], amb[~valid] = -1, 0
    w = int(np.argmax(counts))
    others = np.delete(counts, w)
    res = dict(fail, strict=[w], winner=w, counts=counts, amb=amb, valid=valid, sel=sel,
               margin=int(counts[w] - (others.max() if len(others) else -1)))
    if counts[w] < 5:
        return res
    fin = _refit(P32[w], p2, p3, K, reproj_error, scale, gn_steps, drop_one)
    res['amb_winner'] = fin['amb_winner']
    if fin['ok']:
        res.update(R=fin['R'], t=fin['t'], ok=1, inliers=fin['inliers'], amb_final=fin['amb'])
    if candidates:
        lo = counts[w] - amb[w]
        hs = np.arange(iterations)
        cand = valid & (((hs < w) & (counts + amb >= lo)) | ((hs > w) & (counts + amb > lo)))
        res['cands'] = {w: fin}
        res['strict'] = [w] + np.flatnonzero(cand)[:16].tolist()
        # `extra` more: the next best hypotheses by count (an fp64 5-point solve over noisy points is not unique
        # beyond rounding when its null space is 2-dimensional, so a GPU count may differ from this one)
        top = [int(x) for x in np.argsort(-counts, kind='stable')[:extra] if valid[x]]
        for hh in res['strict'][1:] + top:
            res['cands'][int(hh)] = _refit(P32[hh], p2, p3, K, reproj_error)
    return res


def rot_from_vec(w):
    """rotation matrix of the axis-angle vector w (Rodrigues), float64"""
    w = np.asarray(w, np.float64)
    a = np.linalg.norm(w)
    if a == 0:
        return np.eye(3)
    k = w / a
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx


SKEW_K = np.array([[520.0, 3.5, 141.3], [0.0, 495.0, 117.8], [0.0, 0.0, 1.0]])


def pnp_scene(rng, m, K=SKEW_K, dist=800.0, size=100.0, noise=0.0, outlier_frac=0.0, flat=1.0, img=256.0):
    """m correspondences of an object (a box of edge `size` mm, its third axis scaled by `flat`) under a random
    pose at ~dist mm: pts3d fp32, pts2d its fp64 projection rounded to fp32, plus Gaussian pixel noise and a
    fraction of uniform outliers over an img x img image -> (pts2d, pts3d, R, t, outlier mask)"""
    R = rot_from_vec(rng.uniform(-0.6, 0.6, 3))
    t = np.array([rng.uniform(-0.05, 0.05) * dist, rng.uniform(-0.05, 0.05) * dist, dist])
    p3 = (rng.uniform(-0.5, 0.5, (m, 3)) * size * np.array([1.0, 1.0, flat])).astype(np.float32)
    q = (p3.astype(np.float64) @ R.T + t) @ np.asarray(K, np.float64).T
    uv = q[:, :2] / q[:, 2:] + rng.normal(0.0, 1.0, (m, 2)) * noise
    out = rng.random(m) < outlier_frac
    uv[out] = rng.uniform(0.0, img, (int(out.sum()), 2))
    return uv.astype(np.float32), p3, R, t, out


def rot_err(a, b):
    """angle (rad) between rotations, from the Frobenius distance (well conditioned near 0)"""
    d = np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    return float(2 * np.arcsin(min(d / (2 * np.sqrt(2)), 1.0)))


# the GPU comparison's pose tolerances (test_gpu_pnp.py): rad, mm; ~3x the worst measured on the MI355X (3.8e-8 rad,
# 5.7e-5 mm over every case) and above the fp32 rounding of the outputs (R entries ~6e-8, t at 2 m: ulp 1.2e-4 mm)
POSE_TOL = dict(rot=1e-7, t=1.7e-4)
# the noisy GPU cases that assert POSE_TOL: (data seed, points, hypotheses, RANSAC seed)
NOISY_CASES = [(21, 2000, 100, 5), (22, 1500, 257, 6), (23, 3000, 600, 7)]


def noisy_case(seed, m):
    """0.5-px Gaussian noise and 30 % uniform outliers over the skewed, off-centre SKEW_K"""
    return pnp_scene(np.random.default_rng(seed), m, noise=0.5, outlier_frac=0.3)


def test_hash_anchored_to_splitmix64():
    # SplitMix64 from state 0: its first outputs (the published reference sequence)
    assert int(pnp_mix(0)) == 0xE220A8397B1DCDAF
    assert int(pnp_mix(0x9E3779B97F4A7C15)) == 0x6E789E6AA1B965F4
    assert int(pnp_hash(5, 7, 9)) == int(pnp_mix(pnp_mix(pnp_mix(5) ^ _U64(7)) ^ _U64(9)))


@pytest.mark.parametrize('trial', range(4))
def test_epnp_exact_data_each_case_closed_form(trial):
    rng = np.random.default_rng(100 + trial)
    R = rot_from_vec(rng.uniform(-2, 2, 3))
    t = np.array([rng.uniform(-40, 40), rng.uniform(-40, 40), rng.uniform(500, 1500)])
    pw = rng.uniform(-60, 60, (300, 3))
    q = (pw @ R.T + t) @ SKEW_K.T
    uv = q[:, :2] / q[:, 2:]
    s = epnp(pw[None], uv[None], SKEW_K)
    assert s['ok'][0]
    for c in range(3):
        one = epnp(pw[None], uv[None], SKEW_K, cases=(c,))
        assert one['ok'][0] and one['case'][0] == c
        assert rot_err(one['R'][0], R) <= 1e-9 and np.abs(one['t'][0] - t).max() <= 1e-9 * np.linalg.norm(t)
    # 5 points: the minimal set every hypothesis solves
    s = epnp(pw[None, :5], uv[None, :5], SKEW_K)
    assert rot_err(s['R'][0], R) <= 1e-9 and np.abs(s['t'][0] - t).max() <= 1e-9 * np.linalg.norm(t)
    # the whole RANSAC on fp64 data
    r = pnp_reference(uv, pw, None, 300, SKEW_K, np.eye(3), np.zeros(3), iterations=20, dtype=np.float64)
    assert r['ok'] == 1 and r['inliers'] == 300
    assert rot_err(r['R'], R) <= 1e-9 and np.abs(r['t'] - t).max() <= 1e-9 * np.linalg.norm(t)


def test_degenerate_sets_rejected():
    rng = np.random.default_rng(3)
    line = np.outer(rng.uniform(-50, 50, 40), [1.0, 2.0, -0.5]) + [3.0, 4.0, 5.0]
    plane = np.concatenate([rng.uniform(-50, 50, (40, 2)), np.full((40, 1), 7.0)], 1) @ rot_from_vec([0.3, 0.2, 0.1]).T
    thin = plane + np.outer(rng.uniform(-1, 1, 40), [0.0, 0.0, 1e-4])   # variance ratio ~1e-12
    for pw in (line, plane, thin):
        assert not epnp_control(pw[None])[0][0]
    assert epnp_control(rng.uniform(-50, 50, (40, 3))[None])[0][0]
    # a planar object fails as a whole; four points fail before any hypothesis
    p2, p3, R, t, _ = pnp_scene(rng, 500, flat=0.0)
    assert pnp_reference(p2, p3, None, 500, SKEW_K, np.eye(3), np.zeros(3))['ok'] == 0
    p2, p3, R, t, _ = pnp_scene(rng, 500)
    r = pnp_reference(p2, p3, None, 4, SKEW_K, np.eye(3), np.zeros(3))
    assert r['ok'] == 0 and r['inliers'] == 0 and np.array_equal(r['R'], np.eye(3))
    assert pnp_reference(p2, p3, None, 500, SKEW_K, np.eye(3), np.zeros(3))['ok'] == 1


def test_selection_rules():
    rng = np.random.default_rng(4)
    conf = rng.permutation(5000).astype(np.float32) / 5000
    for num in (1, 100, 4095, 4999):
        want = np.sort(torch.topk(torch.from_numpy(conf), num).indices.numpy())
        assert np.array_equal(pnp_select(conf, 5000, 5000, 'topk', num, 0), want)
    # ties go to the lower index; -0.0 ties with +0.0; NaN ranks above +inf
    c = np.array([0.0, -0.0, 1.0, 0.0, -0.0, np.inf, np.nan, 1.0, -1.0], np.float32)
    assert pnp_select(c, 9, 9, 'topk', 1, 0).tolist() == [6]
    assert pnp_select(c, 9, 9, 'topk', 3, 0).tolist() == [2, 5, 6]
    assert pnp_select(c, 9, 9, 'topk', 5, 0).tolist() == [0, 2, 5, 6, 7]
    assert pnp_select(c, 9, 9, 'topk', 6, 0).tolist() == [0, 1, 2, 5, 6, 7]     # -0.0 at 1 beats +0.0 at 3
    assert pnp_select(c, 9, 9, 'topk', 7, 0).tolist() == [0, 1, 2, 3, 5, 6, 7]
    # count is clamped to [0, capacity]; num > count keeps everything, num == count too
    assert pnp_select(c, 20, 9, 'topk', 10, 0).tolist() == list(range(9))
    assert pnp_select(c, -3, 9, 'topk', 10, 0).tolist() == []
    assert pnp_select(c, 9, 9, 'topk', 9, 0).tolist() == list(range(9))
    # RANDOM: num distinct indices of [0, count - 1), the largest hash keys; every point when num > count
    for num in (10, 998, 999, 1000):
        s = pnp_select(None, 1000, 1000, 'random', num, 3)
        assert len(s) == min(num, 999) and 999 not in s and len(np.unique(s)) == len(s)
    assert pnp_select(None, 1000, 1000, 'random', 1001, 3).tolist() == list(range(1000))
    keys = pnp_hash(3, _SEL_SALT, np.arange(999, dtype=_U64)) >> _U64(32)
    assert keys[pnp_select(None, 1000, 1000, 'random', 10, 3)].min() >= np.sort(keys)[-10]


def test_hypothesis_draws():
    idx, drawn = pnp_draws(9, 300, 7)
    assert drawn.all() and all(len(set(r)) == 5 for r in idx.tolist())
    j = pnp_hash(9, np.arange(300, dtype=_U64)[:, None], np.arange(1, 65, dtype=_U64)[None]) % _U64(7)
    assert idx[:, 0].tolist() == j[:, 0].astype(np.int64).tolist()        # the first draw is always kept
    assert not pnp_draws(9, 50, 4)[1].any()                               # 4 points: never 5 distinct


def test_scoring_band_is_narrow_and_covers_fp32():
    """the band (see _GAMMA) is ~1e-4 px at this scale, and the fp32 evaluation of every point outside it agrees
    with the fp64 one"""
    rng = np.random.default_rng(5)
    p2, p3, R, t, _ = pnp_scene(rng, 20000, noise=2.0)
    P = proj32(SKEW_K, R[None], t[None])
    inl, amb = pnp_score(P, p2, p3, 3.0)
    q = np.einsum('ij,mj->im', P[0, :, :3], p3) + P[0, :, 3:]                 # fp32 throughout
    d = q[:2] / q[2] - p2.T
    in32 = (q[2] > 0) & ((d * d).sum(0) < np.float32(3.0) * np.float32(3.0))
    assert np.array_equal(in32[~amb[0]], inl[0][~amb[0]])
    X = np.asarray(p3, np.float64)
    qq = X @ P[0, :, :3].astype(np.float64).T + P[0, :, 3].astype(np.float64)
    dist = np.linalg.norm(qq[:, :2] / qq[:, 2:] - p2, axis=1)
    width = np.abs(dist[amb[0]] - 3.0).max() if amb.any() else 0.0
    assert width < 2e-4 and amb.sum() < 20


@pytest.mark.parametrize('case', NOISY_CASES)
def test_gpu_tolerances_are_not_vacuous(case):
    """dropping one inlier from the refit, control points at sqrt(var / n) or no Gauss-Newton each move the pose by
    >= 10x POSE_TOL (in rotation or translation) on every noisy case the GPU test holds to POSE_TOL"""
    seed, m, iters, rs = case
    p2, p3, R, t, _ = noisy_case(seed, m)
    kw = dict(iterations=iters, seed=rs, candidates=False)
    r = pnp_reference(p2, p3, None, m, SKEW_K, np.eye(3), np.zeros(3), **kw)
    assert r['ok'] == 1 and rot_err(r['R'], R) < 0.01
    for probe in (dict(drop_one=True), dict(scale='n'), dict(gn_steps=0)):
        o = pnp_reference(p2, p3, None, m, SKEW_K, np.eye(3), np.zeros(3), **kw, **probe)
        moved = max(rot_err(o['R'], r['R']) / POSE_TOL['rot'], np.abs(o['t'] - r['t']).max() / POSE_TOL['t'])
        assert moved >= 10, (probe, moved)
