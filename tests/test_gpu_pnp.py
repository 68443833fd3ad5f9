"""GPU: flow -> 2-D/3-D correspondences and batched RANSAC-EPnP (scflow_amd/csrc/pnp.hip) -- the correspondences
against the reference fixture, pose recovery on exact and on noisy / outlier-ridden data, determinism, batch
invariance, sampling, failure semantics and the RAFT refiners' solve_pose / forward."""
import math
import os

import numpy as np
import pytest
import torch

import scflow_amd
from scflow_amd import _lib, ops
from scflow_amd.synthetic import _rot_xyz, make_inputs

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu


def _rot_angle(a, b):
    """angle (rad) between rotation matrices, from |A - B|_F = 2 sqrt(2) sin(angle / 2): well conditioned near 0,
    where acos of the trace is not (fp32 matrices are orthonormal only to ~1e-7, which acos turns into ~1e-4 rad)."""
    d = (a.double().cpu() - b.double().cpu()).flatten(-2).norm(dim=-1)
    return 2 * torch.asin((d / (2 * math.sqrt(2))).clamp(max=1))


def _scene(n, seed, h=256, w=256):
    """make_inputs' disc depth and reference pose; a random target pose at t ~ (0, 0, 800) mm; the exact flow
    between them (scf_reproject_flow)."""
    inp = make_inputs(n, h, w, seed=seed)
    g = torch.Generator().manual_seed(500 + seed)
    ang = torch.rand((n, 3), generator=g) * 0.4 - 0.2
    rot = torch.stack([_rot_xyz(*[float(a) for a in ang[i]]) for i in range(n)])
    trans = torch.cat([torch.rand((n, 2), generator=g) * 20 - 10, 800 + torch.rand((n, 1), generator=g) * 40 - 20], 1)
    d = {k: inp[k].to(DEV) for k in ('depth', 'internel_k', 'ref_rotation', 'ref_translation')}
    flow = ops.reproject_flow(d['depth'], d['internel_k'], d['ref_rotation'], d['ref_translation'],
                              rot.to(DEV), trans.to(DEV))
    return d, rot, trans, flow


def _corr(d, flow, occ=None):
    return ops.flow_corr_2d3d(flow, d['depth'], d['internel_k'], d['ref_rotation'], d['ref_translation'], occ)


def _ransac(d, pts2d, pts3d, count, conf=None, **kw):
    return ops.pnp_ransac(pts2d, pts3d, count, d['internel_k'], d['ref_rotation'], d['ref_translation'], conf=conf,
                          **kw)


# ------------------------------------------------------------------ correspondences
@pytest.mark.parametrize('case', ['a', 'b'])
@pytest.mark.parametrize('tag', ['nomask', 'mask'])
def test_corr_matches_reference_fixture(golden_dir, case, tag):
    g = np.load(os.path.join(golden_dir, 'corr_2d3d.npz'))
    f = lambda k: torch.from_numpy(g[f'{case}_{k}']).to(DEV)      # noqa: E731
    flow = f('flow16').float() / 16
    occ = f('occ8').float() / 8
    d = dict(depth=f('depth'), internel_k=f('k'), ref_rotation=f('rot'), ref_translation=f('trans'))
    pts2d, pts3d, conf, count = _corr(d, flow.contiguous(), occ if tag == 'mask' else None)
    want_count = g[f'{case}_{tag}_count']
    assert count.cpu().tolist() == want_count.tolist()
    step = int(g[f'{case}_{tag}_row_step'])
    got2, got3, gotc = [], [], []
    for i, c in enumerate(want_count.tolist()):
        got2.append(pts2d[i, :c]); got3.append(pts3d[i, :c]); gotc.append(conf[i, :c])
    got2, got3 = torch.cat(got2).cpu(), torch.cat(got3).cpu()
    src = torch.from_numpy(g[f'{case}_{tag}_src']).float()
    # the full pixel order: the target point minus the flow at the fixture's source pixel is that pixel
    fl = flow.cpu()
    n_of = torch.repeat_interleave(torch.arange(len(want_count)), torch.from_numpy(want_count).long())
    xs, ys = src[:, 0].long(), src[:, 1].long()
    assert torch.equal(got2 - torch.stack([fl[n_of, 0, ys, xs], fl[n_of, 1, ys, xs]], -1), src)
    torch.testing.assert_close(got2[::step], torch.from_numpy(g[f'{case}_{tag}_pts2d']), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(got3[::step], torch.from_numpy(g[f'{case}_{tag}_pts3d']), rtol=1e-5, atol=2e-3)
    gotc = torch.cat(gotc).cpu()
    if tag == 'mask':
        assert torch.equal(gotc, occ.cpu()[n_of, ys, xs])
        if case == 'a':
            assert int(count[-1]) == 0                              # empty mask -> no correspondence
    else:
        assert bool((gotc == 1).all())


# ------------------------------------------------------------------ pose recovery
def test_exact_correspondences_recover_the_pose():
    d, rot, trans, flow = _scene(4, seed=1)
    r, t, ok, inl = ops.pnp(flow, d['depth'], d['internel_k'], d['ref_rotation'], d['ref_translation'])
    _, _, _, count = _corr(d, flow)
    assert int(count.min()) > 15000                                 # ~20 k points per sample
    assert ok.cpu().tolist() == [1] * 4
    assert inl.cpu().tolist() == count.cpu().tolist()
    assert float(_rot_angle(r, rot).max()) < 1e-4
    assert float((t.cpu() - trans).abs().max()) < 0.05


def _noisy(d, flow, seed, sigma=0.5, outlier_frac=0.3):
    pts2d, pts3d, conf, count = _corr(d, flow)
    g = torch.Generator(device=DEV).manual_seed(seed)
    noise = torch.randn(pts2d.shape, generator=g, device=DEV) * sigma
    out = torch.rand(pts2d.shape[:2], generator=g, device=DEV) < outlier_frac
    uni = torch.rand(pts2d.shape, generator=g, device=DEV) * 256
    noisy = torch.where(out[..., None], uni, pts2d + noise).contiguous()
    return noisy, pts2d, pts3d, count, out


def test_noise_and_outliers():
    n = 4
    d, rot, trans, flow = _scene(n, seed=2)
    noisy, clean, pts3d, count, out = _noisy(d, flow, seed=3)
    r, t, ok, inl = _ransac(d, noisy, pts3d, count)
    assert ok.cpu().tolist() == [1] * n
    for i in range(n):
        c = int(count[i])
        err = (noisy[i, :c] - clean[i, :c]).norm(dim=-1)
        true_inl = int((err < 3.0).sum())
        assert int(inl[i]) >= 0.95 * true_inl, (i, int(inl[i]), true_inl)
    assert float(_rot_angle(r, rot).max()) < math.radians(0.5)
    rel = ((t.cpu() - trans).norm(dim=-1) / trans.norm(dim=-1)).max()
    assert float(rel) < 0.01
    # ADD through scf_pose_error (fp64): the object points of sample i as the vertex set
    lib = _lib.load()
    for i in range(n):
        verts = pts3d[i, :int(count[i]):7].double().contiguous()
        diam = float(torch.cdist(verts[::4], verts[::4]).max())
        e3 = torch.zeros(1, dtype=torch.float64, device=DEV)
        e2 = torch.zeros(1, dtype=torch.float64, device=DEV)
        idx = torch.zeros(1, dtype=torch.int32, device=DEV)
        # every operand bound to a name: a temporary's memory could be reused before the kernel reads it
        gr, gt = rot[i:i + 1].double().to(DEV), trans[i:i + 1].double().to(DEV)
        pr, pt = r[i:i + 1].double().contiguous(), t[i:i + 1].double().contiguous()
        kk = d['internel_k'][i:i + 1].double().contiguous()
        _lib.check(lib.scf_pose_error(verts.data_ptr(), verts.shape[0], gr.data_ptr(), gt.data_ptr(), pr.data_ptr(),
                                      pt.data_ptr(), kk.data_ptr(), idx.data_ptr(), 1, 0, e3.data_ptr(), e2.data_ptr(),
                                      ops._stream()), 'scf_pose_error')
        torch.cuda.synchronize()
        assert float(e3) < 0.01 * diam, (i, float(e3), diam)


def test_deterministic_and_batch_invariant():
    n = 32
    d, rot, trans, flow = _scene(n, seed=4)
    noisy, _, pts3d, count, _ = _noisy(d, flow, seed=5)
    a = _ransac(d, noisy, pts3d, count, seed=7)
    b = _ransac(d, noisy, pts3d, count, seed=7)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert int(a[2].sum()) == n
    for i in (0, 13, 31):
        s = slice(i, i + 1)
        one = ops.pnp_ransac(noisy[s].contiguous(), pts3d[s].contiguous(), count[s].contiguous(),
                             d['internel_k'][s].contiguous(), d['ref_rotation'][s].contiguous(),
                             d['ref_translation'][s].contiguous(), seed=7)
        for x, y in zip(one, a):
            assert torch.equal(x[0], y[i]), i


def test_topk_keeps_the_torch_topk_set():
    """distinct confidences; the top-`num` points are exact correspondences and every other point is an outlier,
    so the solve on the kept set finds exactly `num` inliers and the exact pose iff the kept set is torch.topk's."""
    d, rot, trans, flow = _scene(2, seed=6)
    pts2d, pts3d, conf, count = _corr(d, flow)
    g = torch.Generator(device=DEV).manual_seed(8)
    conf = torch.randperm(pts2d.shape[1], generator=g, device=DEV).float()[None].repeat(2, 1) / pts2d.shape[1]
    conf = conf.contiguous()
    num = 3000
    bad = torch.rand(pts2d.shape, generator=g, device=DEV) * 256 + 300   # far off: never an inlier
    keep = torch.zeros(pts2d.shape[:2], dtype=torch.bool, device=DEV)
    for i in range(2):
        c = int(count[i])
        keep[i, torch.topk(conf[i, :c], num).indices] = True
    mixed = torch.where(keep[..., None], pts2d, bad).contiguous()
    r, t, ok, inl = _ransac(d, mixed, pts3d, count, conf=conf, sample_mode='topk', sample_num=num)
    assert ok.cpu().tolist() == [1, 1] and inl.cpu().tolist() == [num, num]
    assert float(_rot_angle(r, rot).max()) < 1e-4
    # 'random' keeps num distinct points of [0, count - 1): at most num inliers on exact data, and all of them
    r, t, ok, inl = _ransac(d, pts2d, pts3d, count, sample_mode='random', sample_num=num, seed=3)
    assert inl.cpu().tolist() == [num, num]
    # num > count keeps every point (the reference's rule)
    _, _, ok, inl = _ransac(d, pts2d, pts3d, count, conf=conf, sample_mode='topk', sample_num=10 ** 6)
    assert inl.cpu().tolist() == count.cpu().tolist()


# ------------------------------------------------------------------ failures
def _assert_failed(res, d, n):
    r, t, ok, inl = res
    for x in (r, t):
        assert bool(torch.isfinite(x).all())
    assert ok.cpu().tolist() == [0] * n and inl.cpu().tolist() == [0] * n
    assert torch.equal(r, d['ref_rotation']) and torch.equal(t, d['ref_translation'])


def test_failure_semantics():
    d, rot, trans, flow = _scene(2, seed=9)
    # count < 4
    few = torch.zeros_like(d['depth'])
    few[:, 100, 100:103] = 800.
    _assert_failed(ops.pnp(flow, few, d['internel_k'], d['ref_rotation'], d['ref_translation']), d, 2)
    # collinear object points: one image row at one depth
    line = torch.zeros_like(d['depth'])
    line[:, 128, 60:200] = 800.
    _assert_failed(ops.pnp(flow, line, d['internel_k'], d['ref_rotation'], d['ref_translation']), d, 2)
    # NaN flow everywhere: every correspondence is an outlier
    nan = torch.full_like(flow, float('nan'))
    _assert_failed(ops.pnp(nan, d['depth'], d['internel_k'], d['ref_rotation'], d['ref_translation']), d, 2)
    # NaN in a band of rows (~15 % of the points): still solved, never NaN.  (With half the points NaN a 5-point draw
    # is all finite with p = 1/32, and 100 hypotheses find none with p ~ 0.04: ok = 0 there is the contract, not a bug.)
    part = flow.clone()
    part[:, :, 60:85] = float('nan')
    r, t, ok, _ = ops.pnp(part, d['depth'], d['internel_k'], d['ref_rotation'], d['ref_translation'])
    assert ok.cpu().tolist() == [1, 1] and bool(torch.isfinite(r).all()) and bool(torch.isfinite(t).all())
    assert float(_rot_angle(r, rot).max()) < 1e-4


# ------------------------------------------------------------------ refiners
def _raft(iters=2, **test_cfg):
    cfg = scflow_amd.raft_model_cfg(iters=iters)
    cfg['test_cfg'] = dict(iters=iters, solve_pose_mode='hip_ransac_epnp', **test_cfg)
    return scflow_amd.build_refiner(cfg)


def test_solve_pose_recovers_the_target_pose():
    m = _raft()
    d, rot, trans, flow = _scene(3, seed=10)
    labels = torch.tensor([1, 2, 3], device=DEV)
    occ = torch.ones_like(d['depth'])
    res = m.solve_pose(flow, d['depth'], d['ref_rotation'], d['ref_translation'], d['internel_k'], labels, [2, 1],
                       occ)
    assert sorted(res) == ['labels', 'rotations', 'scores', 'translations']
    assert [len(x) for x in res['rotations']] == [2, 1]
    r, t = torch.cat(res['rotations']), torch.cat(res['translations'])
    assert float(_rot_angle(r, rot).max()) < 1e-4
    assert float((t.cpu() - trans).abs().max()) < 0.05
    assert torch.equal(torch.cat(res['labels']), labels)
    # a failed sample is dropped from its image's list
    depth = d['depth'].clone()
    depth[1] = 0.
    res = m.solve_pose(flow, depth, d['ref_rotation'], d['ref_translation'], d['internel_k'], labels, [2, 1], occ)
    assert [len(x) for x in res['rotations']] == [1, 1]
    assert torch.cat(res['labels']).cpu().tolist() == [1, 3]


@pytest.mark.parametrize('kind', ['RAFTRefinerFlowMask', 'RAFTRefinerFlow'])
def test_forward_batch8_lists_match_ok(kind):
    m = _raft()
    if kind == 'RAFTRefinerFlow':
        cfg = scflow_amd.raft_model_cfg(iters=2)
        cfg.update(type='RAFTRefinerFlow', decoder=dict(cfg['decoder'], type='RAFTDecoder'),
                   test_cfg=dict(iters=2, solve_pose_mode='hip_ransac_epnp'))
        m = scflow_amd.build_refiner(cfg)
    sd = scflow_amd.fill_state_dict({k: v.shape for k, v in m.state_dict().items()}, seed=9)
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV)
    inp = make_inputs(8, 256, 256, seed=11)
    data = dict(rendered_images=inp['render_images'].to(DEV), real_images=inp['real_images'].to(DEV),
                ref_rotations=inp['ref_rotation'].to(DEV), ref_translations=inp['ref_translation'].to(DEV),
                rendered_depths=inp['depth'].to(DEV), internel_k=inp['internel_k'].to(DEV),
                labels=inp['label'].to(DEV), per_img_patch_num=[3, 5])
    res = m.forward(data, dict(img_metas=[dict(geometry_transform_mode='adapt_intrinsic')] * 2))
    assert [sorted(res)] == [['labels', 'rotations', 'scores', 'translations']] and len(res['rotations']) == 2
    flow_out = m.forward_single_view(data, None, return_pose=False)
    occ = flow_out[1] if kind == 'RAFTRefinerFlowMask' else None
    _, _, ok, _ = ops.pnp(flow_out[0].contiguous(), data['rendered_depths'], data['internel_k'],
                          data['ref_rotations'], data['ref_translations'],
                          None if occ is None else occ.contiguous())
    n_ok = int(ok.sum())
    assert sum(len(x) for x in res['rotations']) == n_ok
    assert sum(len(x) for x in res['labels']) == n_ok
    for x in res['rotations']:
        assert bool(torch.isfinite(x).all())
    with pytest.raises(NotImplementedError):
        m.forward(data, dict(img_metas=[dict(geometry_transform_mode='target_intrinsic')] * 2))


# ------------------------------------------------------------------ against the float64 restatement
# pnp_reference (tests/test_pnp_host.py) restates scf_pnp_ransac from the header contract in float64.  Per sample:
# ok exactly; the inlier count within the points the restatement marks ambiguous under the final fp32 P (usually
# none: then equal); R, t within POSE_TOL of the restated refit -- of the winner's, or, when the winner is not
# decisive (another hypothesis is within the two hypotheses' ambiguous counts), of one of the candidate winners'.
from test_pnp_host import (NOISY_CASES, POSE_TOL, SKEW_K, noisy_case, pnp_reference,  # noqa: E402
                           pnp_scene, rot_err, rot_from_vec)

_MEASURED = {}


def _pack(cases, cap):
    """[(pts2d, pts3d, count, K, conf)] -> GPU tensors of capacity cap; slots past each count hold NaN and huge
    garbage, which no kernel may read"""
    n = len(cases)
    p2 = np.full((n, cap, 2), np.nan, np.float32)
    p3 = np.full((n, cap, 3), 3e38, np.float32)
    p3[:, 1::2] = np.nan
    cf = np.full((n, cap), np.nan, np.float32)
    ks = np.zeros((n, 3, 3), np.float32)
    cnt = np.zeros(n, np.int32)
    for i, (a, b, c, k, cc) in enumerate(cases):
        p2[i, :len(a)], p3[i, :len(b)] = a, b
        if cc is not None:
            cf[i, :len(cc)] = cc
        ks[i], cnt[i] = k, c
    g = lambda x: torch.from_numpy(x).to(DEV).contiguous()        # noqa: E731
    rr = torch.from_numpy(np.stack([rot_from_vec([0.1 * i, 0.2, -0.1]) for i in range(n)]).astype(np.float32))
    tr = torch.tensor([[1.0, 2.0, 500.0 + i] for i in range(n)])
    return g(p2), g(p3), g(cnt), g(ks), g(cf), rr.to(DEV), tr.to(DEV)


def _run_vs_reference(cases, cap, tag, tol=None, **kw):
    """one launch over `cases`; each sample against its own restatement -> [(reference, candidate used)]"""
    p2, p3, cnt, ks, cf, rr, tr = _pack(cases, cap)
    R, t, ok, inl = [x.cpu().numpy() for x in ops.pnp_ransac(p2, p3, cnt, ks, rr, tr, conf=cf, **kw)]
    out = []
    for i, (a, b, c, k, cc) in enumerate(cases):
        ttol = tol[i] if isinstance(tol, list) else (tol or POSE_TOL)
        ref = pnp_reference(p2[i].cpu().numpy(), p3[i].cpu().numpy(), cf[i].cpu().numpy(), int(cnt[i]), k,
                            rr[i].cpu().numpy(), tr[i].cpu().numpy(), extra=ttol.get('extra', 0), **kw)
        what = f'{tag}[{i}]'
        assert int(ok[i]) == ref['ok'], (what, int(ok[i]), ref['ok'], ref.get('counts', [None])[:0])
        if not ref['ok']:
            assert int(inl[i]) == 0 and np.array_equal(R[i], rr[i].cpu().numpy()), what
            assert np.array_equal(t[i], tr[i].cpu().numpy()), what
            out.append((ref, None))
            continue
        fits = []
        for h, c_ in ref['cands'].items():
            if c_['ok']:
                fits.append((rot_err(R[i], c_['R']) / ttol['rot'] + np.abs(t[i] - c_['t']).max() / ttol['t'], h))
        score, h = min(fits)
        c_ = ref['cands'][h]
        er, et = rot_err(R[i], c_['R']), float(np.abs(t[i] - c_['t']).max())
        decisive = len(ref['strict']) == 1 and ref['amb_winner'] == 0
        rank = ref['strict'].index(h) if h in ref['strict'] else -1
        m = _MEASURED.setdefault(tag, dict(rot=0.0, t=0.0, inl=0, nondecisive=0, offwinner=0, n=0))
        m.update(rot=max(m['rot'], er), t=max(m['t'], et), inl=max(m['inl'], abs(int(inl[i]) - c_['inliers'])),
                 nondecisive=m['nondecisive'] + (not decisive), offwinner=m['offwinner'] + (h != ref['winner']),
                 n=m['n'] + 1)
        assert abs(int(inl[i]) - c_['inliers']) <= c_['amb'], (what, int(inl[i]), c_['inliers'], c_['amb'], h)
        assert er <= ttol['rot'] and et <= ttol['t'], (what, er, et, h, ref['winner'], rank)
        if not ttol.get('extra'):
            assert rank >= 0, (what, h, ref['winner'], ref['strict'])
        out.append((ref, h))
    print(f'[measured] {tag}: vs restatement max |dR| {_MEASURED[tag]["rot"]:.2e} rad, max |dt| '
          f'{_MEASURED[tag]["t"]:.2e} mm, max |d inliers| {_MEASURED[tag]["inl"]}, non-decisive '
          f'{_MEASURED[tag]["nondecisive"]} / {_MEASURED[tag]["n"]}, GPU took another hypothesis\'s refit '
          f'{_MEASURED[tag]["offwinner"]}' if tag in _MEASURED else f'[measured] {tag}: all failed as restated')
    return out


# noisy cases: a 5-point fp64 solve over noisy points is not unique past rounding (its null space is
# 2-dimensional, and the GPU's Jacobi and the restatement's SVD pick different bases of it), so a hypothesis' count
# may differ between the two; the GPU pose must still be the refit of one of the restatement's best hypotheses
_NOISY_TOL = dict(POSE_TOL, extra=12)


@pytest.mark.parametrize('iters', [1, 100, 255, 256, 257, 600])
def test_iterations_noisy_vs_reference(iters):
    cases, outs = [], []
    for s in range(3):
        if iters == 1:      # the one hypothesis is the answer: exact inliers, and a seed whose draw is all inliers
            a, b, R, t, out = pnp_scene(np.random.default_rng(40 + s), 1200, outlier_frac=0.3)
        else:
            a, b, R, t, out = noisy_case(40 + s, 1200)
        cases.append((a, b, 1200, SKEW_K, None))
        outs.append(out)
    seed = iters
    if iters == 1:
        from test_pnp_host import pnp_draws
        seed = next(x for x in range(5000) if not any(o[pnp_draws(x, 1, 1200)[0][0]].any() for o in outs))
    _run_vs_reference(cases, 1200, f'noisy iterations={iters}', _NOISY_TOL, iterations=iters, seed=seed)


@pytest.mark.parametrize('case', NOISY_CASES)
def test_noisy_cases_hold_pose_tol(case):
    seed, m, iters, rs = case
    a, b, R, t, _ = noisy_case(seed, m)
    (ref, h), = _run_vs_reference([(a, b, m, SKEW_K, None)], m, f'noisy case {seed}', _NOISY_TOL,
                                  iterations=iters, seed=rs)
    assert ref['ok'] == 1


def _two_pose(lab, seed=0):
    """exact correspondences: label 0 / 1 under pose A (0: on the object plane z = 0, 1: off it), label 2 under
    pose B (A shifted 200 mm sideways: ~130 px apart, never within the threshold of each other).  A hypothesis
    of label-0 points only is planar, hence invalid."""
    rng = np.random.default_rng(seed)
    m = len(lab)
    p3 = rng.uniform(-50, 50, (m, 3))
    p3[lab == 0, 2] = 0.0
    p3[lab == 1, 2] = np.where(np.arange(int((lab == 1).sum())) % 2 == 0, 40.0, -40.0)
    p3 = p3.astype(np.float32)
    R = rot_from_vec([0.2, -0.3, 0.1])
    tA, tB = np.array([-100.0, 5.0, 800.0]), np.array([100.0, 5.0, 800.0])
    isA = (lab < 2)[:, None]
    q = np.where(isA, p3.astype(np.float64) @ R.T + tA, p3.astype(np.float64) @ R.T + tB) @ SKEW_K.T
    return (q[:, :2] / q[:, 2:]).astype(np.float32), p3, R, tA, tB


@pytest.mark.parametrize('name,iters,seed', [
    # equal halves (all off-plane): pure-B hypotheses from h = 8 on, the first pure-A one at h = 262 (round 1),
    # the last pure hypothesis is pure-A: the tie must stay with B (the lowest h), across rounds
    ('tie', 300, 474),
    # 301 A points of which 3 off the plane, 199 B points: pure-B hypotheses from h = 51 on, the first valid pure-A
    # one (more inliers) at h = 571, in the last partial round of 600
    ('late600', 600, 0),
    # ... and at h = 256, alone in the last round of 257
    ('late257', 257, 40)])
def test_winner_rule_two_poses(name, iters, seed):
    m = 500
    if name == 'tie':
        lab = np.where(np.arange(m) % 2 == 0, 1, 2)
    else:
        lab = np.where(np.arange(m) % 5 >= 3, 2, 0)
        lab[[7, 101, 333]] = 1
    a, b, R, tA, tB = _two_pose(lab)
    (ref, h), = _run_vs_reference([(a, b, m, SKEW_K, None)], m, f'two poses {name}', iterations=iters, seed=seed)
    want_a = name != 'tie'
    assert ref['ok'] == 1 and ref['margin'] >= (0 if name == 'tie' else 1)
    assert np.abs(ref['t'] - (tA if want_a else tB)).max() < 1e-3
    assert ref['inliers'] == int((lab < 2).sum() if want_a else (lab == 2).sum())
    assert ref['winner'] == {'tie': 8, 'late600': 571, 'late257': 256}[name]


def _batch_cases():
    """one capacity, one parameter set: point counts across the 256-point scoring stride and the 4096-point
    select chunk, count past capacity / negative / 4, camera and geometry edges -> [(case, tolerance)]"""
    rng = np.random.default_rng(77)
    cap = 4200
    cases, tols = [], []
    loose = POSE_TOL          # the ill-conditioned cases measured within it too

    def add(a, b, c, k=SKEW_K, tol=None):
        cases.append((a, b, c, k, None))
        tols.append(tol or POSE_TOL)

    for m in (5, 6, 255, 256, 257, 4095, 4096, 4097):
        a, b, *_ = pnp_scene(rng, m)
        add(a, b, m)
    a, b, *_ = pnp_scene(rng, cap)
    add(a, b, 10 ** 6)                               # count > capacity: clamped
    add(a, b, -5)                                    # count < 0: fails
    add(a[:4], b[:4], 4)                             # four points: fails
    a, b, *_ = pnp_scene(rng, 3000, noise=0.3, outlier_frac=0.2)
    add(a, b, 3000, tol=dict(POSE_TOL, extra=12))
    K2 = np.array([[1050.0, -2.0, 331.0], [0.0, 1010.0, 262.5], [0.0, 0.0, 1.0]])   # 512 x 640-scale pixels
    a, b, *_ = pnp_scene(rng, 2500, K=K2, img=640.0)
    add(a, b, 2500, K2)
    a, b, *_ = pnp_scene(rng, 2500, K=K2, noise=0.4, outlier_frac=0.3, img=640.0)
    add(a, b, 2500, K2, dict(POSE_TOL, extra=12))
    a, b, *_ = pnp_scene(rng, 2000, dist=2000.0, size=30.0)                         # 30 mm at 2 m
    add(a, b, 2000, tol=loose)
    a, b, *_ = pnp_scene(rng, 2000, dist=2000.0, size=30.0, noise=0.2, outlier_frac=0.2)
    add(a, b, 2000, tol=dict(loose, extra=12))
    # scattered NaN / inf in both point sets
    a, b, *_ = pnp_scene(rng, 3000)
    a, b = a.copy(), b.copy()
    bad = rng.choice(3000, 150, replace=False)
    a[bad[:50], 0], b[bad[50:100], 2], a[bad[100:], 1] = np.nan, np.inf, -np.inf
    add(a, b, 3000)
    # points behind the camera on the rays of visible ones: they project onto the same pixels, and must not count
    a, b, R, t, _ = pnp_scene(rng, 2000)
    cam = b[1000:].astype(np.float64) @ R.T + t
    b2 = b.copy()
    b2[1000:] = ((-cam - t) @ R).astype(np.float32)
    add(a, b2, 2000)
    # planar: fails; near-planar either side of the 1e-8 variance rule (1e-6 and 1e-10 of the largest)
    for flat in (0.0, 1e-3, 1e-5):
        a, b, *_ = pnp_scene(rng, 1500, flat=flat)
        add(a, b, 1500, tol=loose)
    return cases, tols, cap


def test_batch_of_edges_vs_reference():
    cases, tols, cap = _batch_cases()
    assert len(cases) >= 20
    while len(cases) < 32:                            # N >= 32 in one launch
        a, b, *_ = pnp_scene(np.random.default_rng(len(cases)), 300 + 37 * len(cases))
        cases.append((a, b, len(a), SKEW_K, None))
        tols.append(POSE_TOL)
    out = _run_vs_reference(cases, cap, 'edge batch', tols, iterations=300, seed=11)
    oks = [r['ok'] for r, _ in out]
    assert oks[8:11] == [1, 0, 0] and oks[18:21] == [0, 1, 0]      # clamped / negative / four; planar edges
    assert out[17][0]['inliers'] == 1000                              # the behind-camera half never counts
    print('[measured] edge batch ok flags', oks)


def test_thresholds_vs_reference():
    rng = np.random.default_rng(5)
    cases = []
    for s in range(2):
        a, b, *_ = pnp_scene(rng, 800, noise=0.3, outlier_frac=0.2)
        cases.append((a, b, 800, SKEW_K, None))
    out = _run_vs_reference(cases, 800, 'reproj_error=0', iterations=50, reproj_error=0.0)
    assert [r['ok'] for r, _ in out] == [0, 0]
    out = _run_vs_reference(cases, 800, 'reproj_error=1e30', dict(POSE_TOL, extra=12),
                            iterations=50, reproj_error=1e30)
    assert [r['inliers'] for r, _ in out] == [800, 800]


@pytest.mark.parametrize('mode', ['topk-quantised', 'topk-zeros-nan', 'random'])
def test_sampling_kept_set_vs_reference(mode):
    from test_pnp_host import pnp_select
    rng = np.random.default_rng(8)
    m = 5000
    if mode == 'topk-quantised':
        conf = (rng.integers(0, 16, m) / 16).astype(np.float32)
    elif mode == 'topk-zeros-nan':
        conf = rng.choice(np.array([0.0, -0.0, 0.5, -0.5, np.nan, np.inf], np.float32), m, p=[.3, .3, .2, .1, .05, .05])
    else:
        conf = None
    smode = 'random' if mode == 'random' else 'topk'
    for num in (m - 2, m - 1, m, m + 1, 4095, 4096, 4097, 1234):
        sel = pnp_select(conf, m, m, smode, num, 13)
        a, b, *_ = pnp_scene(np.random.default_rng(num), m)
        a = a.copy()
        far = np.ones(m, bool)
        far[sel] = False
        a[far] += 400.0
        cases = [(a, b, m, SKEW_K, conf)]
        (ref, h), = _run_vs_reference(cases, m, f'sampling {mode} num={num}', iterations=20, sample_mode=smode,
                                      sample_num=num, seed=13)
        assert ref['ok'] == 1 and ref['inliers'] == len(sel)


def test_zz_report_measured():
    for k, v in _MEASURED.items():
        print(f'[measured] {k}: {v}')
