"""GPU: the mesh renderer (scflow_amd/csrc/render.hip) against the float64 restatement of test_render_host.py --
coverage, face index, depth and RGB on a cube, icospheres, a triangle soup with heavy occlusion, a non-square
image, a mixed-label batch, faces behind the camera and an object out of view -- plus determinism, batch
invariance, crack-free closed meshes, a 200 k-face batch of 32, and the refiners' rendering data path."""
import json
import math
import os
import time

import numpy as np
import pytest
import torch

import scflow_amd
from scflow_amd import ops
from scflow_amd.mesh import MeshRenderer, MeshStore, icosphere, make_mesh

from test_render_host import (SHIPPED, check_ambiguous_cap, colored_icosphere, cube, intrinsics, look_at_pose,
                              render_reference, sample_zmin)

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu


def _soup(n, seed):
    """n random triangles of 40-120 mm in a 200 mm box: heavy occlusion, random winding and colours."""
    g = np.random.default_rng(seed)
    centers = g.uniform(-100, 100, size=(n, 1, 3))
    verts = (centers + g.uniform(-60, 60, size=(n, 3, 3))).reshape(-1, 3)
    return make_mesh(verts, np.arange(3 * n).reshape(n, 3), colors=g.uniform(0, 1, size=(3 * n, 3)))


def _render(store, labels, poses, Ks, H, W, **kw):
    R = torch.tensor(np.stack([p[0] for p in poses]), device=DEV)
    t = torch.tensor(np.stack([p[1] for p in poses]), device=DEV)
    K = torch.tensor(np.stack(Ks), device=DEV)
    lab = torch.tensor(labels, dtype=torch.int64, device=DEV)
    out = ops.render_mesh(store.on(DEV), lab, R, t, K, (H, W), **kw)
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu()) for k, v in out.items()}


def _check(out, i, mesh, pose, K, H, W, lights=dict(default_lights=True, seperate_lights=True), batch_zmin=None,
           what=''):
    ref = render_reference(mesh, pose[0], pose[1], K, H, W, batch_zmin=batch_zmin, **lights)
    check_ambiguous_cap(ref, what)                 # what the comparison leaves out is at most 1 % of the image
    ok = ~ref['ambiguous']
    face = out['pix_to_face'][i].numpy()
    z = out['zbuf'][i].numpy().astype(np.float64)
    rgb = out['images'][i].numpy().astype(np.float64)
    bad = (face != ref['face']) & ok
    assert not bad.any(), f'{what}: face index differs at {np.argwhere(bad)[:5].tolist()} ({bad.sum()} px)'
    cov = (ref['face'] >= 0) & ok
    assert ((z == -1) == (ref['face'] < 0))[ok].all(), what
    rel = np.abs(z[cov] - ref['zbuf'][cov]) / ref['zbuf'][cov]
    assert rel.size == 0 or rel.max() <= 1e-6, f'{what}: depth rel err {rel.max():.2e}'
    err = np.abs(rgb[..., :3] - ref['rgb'])[ok]
    assert err.size == 0 or err.max() <= 1e-5, f'{what}: rgb err {err.max():.2e}'
    np.testing.assert_array_equal(rgb[..., 3], (face >= 0).astype(np.float64))
    return ref


POSES = [look_at_pose(0.3, -0.4, 0.2, 600.0, 10.0, -5.0), look_at_pose(-0.7, 1.1, 2.5, 450.0, -20.0, 15.0),
         look_at_pose(2.0, 0.1, -0.9, 800.0, 0.0, 0.0)]


@pytest.mark.parametrize('lights', [dict(default_lights=True, seperate_lights=True),
                                    dict(default_lights=True, seperate_lights=False),
                                    dict(default_lights=False, seperate_lights=True),
                                    dict(default_lights=False, seperate_lights=False)])
def test_cube_and_icosphere_vs_reference(lights):
    H = W = 128
    meshes = {0: cube(120.0), 1: colored_icosphere(3, 70.0)}
    store = MeshStore(meshes)
    K = intrinsics(300.0, H, W)
    labels = [0, 1, 0, 1, 0, 1]
    poses = [POSES[i // 2] for i in range(6)]
    out = _render(store, labels, poses, [K] * 6, H, W, **lights)
    bz = min(sample_zmin(meshes[l], *p) for l, p in zip(labels, poses))
    for i, (l, p) in enumerate(zip(labels, poses)):
        ref = _check(out, i, meshes[l], p, K, H, W, lights, batch_zmin=bz, what=f'sample {i}')
        assert (ref['face'] >= 0).sum() > 500


def test_triangle_soup_heavy_occlusion():
    H = W = 64
    mesh = _soup(300, 3)
    K = intrinsics(120.0, H, W)
    out = _render(MeshStore({0: mesh}), [0, 0], POSES[:2], [K, K], H, W)
    for i in range(2):
        ref = _check(out, i, mesh, POSES[i], K, H, W, what=f'soup {i}')
        assert (ref['face'] >= 0).mean() > 0.3


def test_non_square_image():
    H, W = 64, 96
    mesh = colored_icosphere(3, 80.0)
    K = intrinsics(150.0, H, W)
    pose = look_at_pose(0.2, 0.5, 0.1, 500.0, 40.0, -10.0)
    out = _render(MeshStore({0: mesh}), [0], [pose], [K], H, W)
    assert out['zbuf'].shape == (1, H, W) and out['images'].shape == (1, H, W, 4)
    _check(out, 0, mesh, pose, K, H, W, what='64x96')


def test_mixed_label_batch_of_8():
    H = W = 64
    meshes = {0: cube(100.0), 1: colored_icosphere(2, 60.0), 3: _soup(60, 5)}
    store = MeshStore(meshes)
    labels = [3, 0, 1, 1, 0, 3, 0, 1]
    g = np.random.default_rng(8)
    poses = [look_at_pose(*g.uniform(-math.pi, math.pi, 3), g.uniform(350, 700), *g.uniform(-30, 30, 2)) for _ in labels]
    Ks = [intrinsics(g.uniform(90, 140), H, W) for _ in labels]
    out = _render(store, labels, poses, Ks, H, W)
    for i, l in enumerate(labels):
        _check(out, i, meshes[l], poses[i], Ks[i], H, W, what=f'sample {i} label {l}')
    # a label without a mesh (2) or out of range renders background
    out = _render(store, [2, 7], poses[:2], Ks[:2], H, W)
    assert (out['zbuf'] == -1).all() and (out['pix_to_face'] == -1).all() and (out['images'][..., :3] == 0.5).all()


def test_faces_behind_the_camera():
    """a soup straddling the image plane: faces partly behind the camera are rasterised as projected and their
    z <= 0 hits discarded; faces wholly behind are skipped."""
    H = W = 64
    mesh = _soup(200, 11)
    K = intrinsics(60.0, H, W)
    pose = look_at_pose(0.1, 0.2, 0.0, 40.0)                   # the box spans z in about [-100, 180]
    R, t = pose
    z = mesh.verts.astype(np.float64) @ R.T.astype(np.float64) + t
    zf = z[:, 2].reshape(-1, 3)
    assert (zf <= 0).all(1).any() and ((zf <= 0).any(1) & (zf > 0).any(1)).any()
    out = _render(MeshStore({0: mesh}), [0], [pose], [K], H, W)
    ref = _check(out, 0, mesh, pose, K, H, W, what='behind')
    assert (ref['face'] >= 0).any()
    assert (out['zbuf'][0][out['pix_to_face'][0] >= 0] > 0).all()


def test_object_out_of_view():
    H = W = 64
    mesh = colored_icosphere(2, 50.0)
    K = intrinsics(100.0, H, W)
    poses = [look_at_pose(0, 0, 0, 500.0, 2000.0, 0.0), look_at_pose(0, 0, 0, -500.0)]     # beside, behind
    out = _render(MeshStore({0: mesh}), [0, 0], poses, [K, K], H, W)
    assert (out['zbuf'] == -1).all() and (out['pix_to_face'] == -1).all()
    assert (out['images'][..., :3] == 0.5).all() and (out['images'][..., 3] == 0).all()


def test_deterministic_and_batch_invariant():
    H = W = 96
    meshes = {0: colored_icosphere(4, 60.0), 1: _soup(400, 2)}
    store = MeshStore(meshes)
    g = np.random.default_rng(32)
    labels = [int(x) for x in g.integers(0, 2, 32)]
    poses = [look_at_pose(*g.uniform(-math.pi, math.pi, 3), g.uniform(350, 700), *g.uniform(-30, 30, 2)) for _ in labels]
    Ks = [intrinsics(g.uniform(100, 160), H, W) for _ in labels]
    kw = dict(norm=((0.4, 0.45, 0.5), (0.22, 0.23, 0.24)))
    a = _render(store, labels, poses, Ks, H, W, **kw)
    b = _render(store, labels, poses, Ks, H, W, **kw)
    for k in ('zbuf', 'pix_to_face', 'images', 'rgb'):
        assert torch.equal(a[k], b[k]), k
    for i in (0, 13, 31):
        one = _render(store, [labels[i]], [poses[i]], [Ks[i]], H, W, **kw)
        for k in ('zbuf', 'pix_to_face', 'images', 'rgb'):
            assert torch.equal(one[k][0], a[k][i]), (i, k)


def test_closed_convex_mesh_has_no_cracks():
    """a convex closed mesh projects to a convex silhouette: every row and every column of covered pixels is one
    unbroken run (a pixel missed along a shared edge would split it)."""
    H = W = 256
    mesh = make_mesh(*icosphere(4, 90.0))
    g = np.random.default_rng(4)
    poses = [look_at_pose(*g.uniform(-math.pi, math.pi, 3), g.uniform(300, 500), *g.uniform(-40, 40, 2)) for _ in range(4)]
    K = intrinsics(280.0, H, W)
    out = _render(MeshStore({0: mesh}), [0] * 4, poses, [K] * 4, H, W)
    for i in range(4):
        cov = (out['pix_to_face'][i] >= 0).numpy()
        assert cov.sum() > 5000
        for m in (cov, cov.T):
            for line in m:
                idx = np.nonzero(line)[0]
                assert idx.size == 0 or idx[-1] - idx[0] + 1 == idx.size


def test_200k_faces_batch_32_in_time():
    H = W = 256
    v, f = icosphere(7, 90.0)                                  # 327 680 faces
    store = MeshStore({0: make_mesh(v, f)})
    g = np.random.default_rng(7)
    poses = [look_at_pose(*g.uniform(-math.pi, math.pi, 3), g.uniform(350, 600)) for _ in range(32)]
    K = intrinsics(300.0, H, W)
    _render(store, [0], poses[:1], [K], H, W)                  # upload and warm up
    t0 = time.perf_counter()
    out = _render(store, [0] * 32, poses, [K] * 32, H, W)
    dt = time.perf_counter() - t0
    assert dt < 20.0, f'{dt:.1f} s'
    cov = out['pix_to_face'] >= 0
    assert cov.sum() > 32 * 5000 and (out['zbuf'][cov] > 0).all()


# ------------------------------------------------------------------------------------------- refiners
def _golden_shapes():
    here = os.path.dirname(os.path.abspath(__file__))
    return json.load(open(os.path.join(here, 'golden', 'state_dict_keys.json')))['shapes']


@pytest.fixture(scope='module')
def scene():
    H = W = 256
    store = MeshStore({0: colored_icosphere(4, 60.0), 1: cube(90.0), 2: colored_icosphere(2, 70.0)})
    renderer = MeshRenderer(store, (H, W), **SHIPPED)
    g = np.random.default_rng(21)
    n = 4
    poses = [look_at_pose(*g.uniform(-0.5, 0.5, 3), g.uniform(450, 550), *g.uniform(-15, 15, 2)) for _ in range(n)]
    R = torch.tensor(np.stack([p[0] for p in poses]), device=DEV)
    t = torch.tensor(np.stack([p[1] for p in poses]), device=DEV)
    K = torch.tensor(np.stack([intrinsics(320.0, H, W)] * n), device=DEV)
    labels = torch.tensor([0, 1, 2, 0], device=DEV)
    real = torch.rand((n, 3, H, W), generator=torch.Generator().manual_seed(3)).to(DEV)
    norm = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375])
    batch = dict(img=[real[:2], real[2:]],
                 annots=dict(ref_rotations=[R[:2], R[2:]], ref_translations=[t[:2], t[2:]], labels=[labels[:2], labels[2:]],
                             k=[K[:2], K[2:]], gt_masks=[torch.ones((2, H, W), device=DEV), torch.ones((2, H, W), device=DEV)]),
                 img_metas=[dict(img_norm_cfg=norm), dict(img_norm_cfg=norm)])
    return renderer, batch, (R, t, K, labels)


def _model(cycles=1):
    cfg = scflow_amd.scflow_model_cfg()
    cfg['test_cfg'] = dict(iters=2, cycles=cycles)
    m = scflow_amd.build_refiner(cfg)
    m.load_state_dict(scflow_amd.fill_state_dict(_golden_shapes(), seed=0), strict=True)
    return m.to(DEV)


def test_format_data_test_feeds_forward_single_pass(scene):
    renderer, batch, (R, t, K, labels) = scene
    model = _model().attach_renderer(renderer)
    data = model.format_data_test(batch)
    out = renderer(R, t, K, labels)
    norm = batch['img_metas'][0]['img_norm_cfg']
    mean = torch.Tensor(norm['mean']).view(1, 3, 1, 1).to(DEV) / 255.
    std = torch.Tensor(norm['std']).view(1, 3, 1, 1).to(DEV) / 255.
    want = (out['images'][..., :3].permute(0, 3, 1, 2).contiguous() - mean) / std
    torch.testing.assert_close(data['rendered_images'], want, rtol=0, atol=1e-6)
    assert torch.equal(data['rendered_depths'], out['fragments'].zbuf[..., 0])
    assert torch.equal(data['rendered_masks'], (out['fragments'].zbuf[..., 0] > 0).float())
    assert data['per_img_patch_num'] == [2, 2] and data['gt_masks'].dtype == torch.bool
    res = model.forward_single_pass(data)
    assert [r.shape for r in res['rotations']] == [(2, 3, 3), (2, 3, 3)]
    assert all(torch.isfinite(r).all() for r in res['rotations'])


def test_two_cycles_equal_the_manual_loop(scene):
    renderer, batch, _ = scene
    model = _model(cycles=2).attach_renderer(renderer)
    data = model.format_data_test(batch)
    got = model.forward(data)
    first = model.forward_single_pass(data)
    rot, trans = torch.cat(first['rotations']), torch.cat(first['translations'])
    rgb, depth, mask = renderer.render_normalized(rot, trans, data['internel_k'], data['labels'])
    again = dict(data, ref_rotations=rot, ref_translations=trans, rendered_images=rgb, rendered_depths=depth,
                 rendered_masks=mask)
    want = model.forward_single_pass(again)
    for k in ('rotations', 'translations'):
        for a, b in zip(got[k], want[k]):
            assert torch.equal(a, b), k
    assert not torch.equal(torch.cat(got['rotations']), torch.cat(first['rotations']))


def test_closed_loop_pnp_recovers_the_rendering_pose(scene):
    """render at a ground-truth pose; a flow of zeros at that pose through ops.pnp gives the pose back."""
    renderer, _, (R, t, K, labels) = scene
    _, depth, mask = renderer.render_normalized(R, t, K, labels)
    assert (mask.flatten(1).sum(1) > 2000).all()
    flow = torch.zeros((R.shape[0], 2) + depth.shape[1:], device=DEV)
    rot, trans, ok, _ = ops.pnp(flow, depth.contiguous(), K, R, t, iterations=50, reproj_error=1.0)
    assert bool(ok.all())
    assert (rot - R).abs().max() < 1e-3
    assert (trans - t).abs().max() < 0.5
