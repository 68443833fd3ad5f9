"""GPU: the mesh renderer (scflow_amd/csrc/render.hip) against the float64 restatement of test_render_host.py at its
edges -- ragged 16 x 16 tiles in both directions, H > W, min(H, W) = 1, fx != fy, faces far below a pixel, a full
256-face chunk with the winner in a later chunk, the two tie rules on constructed exact ties, the three skip rules
(zero area, vertex index outside the mesh, max_faces), non-finite poses staying inside their sample, every output
combination, guard bands round the four outputs, and norm= against the restatement.  The scene lists and the
comments on which branch each scene takes live next to the restatement (RAGGED_SIZES, anisotropic_scenes, ...); this
file adds what only a launch has.

The measures and bounds are those of test_gpu_render.py: off the restatement's `ambiguous` set -- at
most 1 % of an image, asserted in every comparison -- face index equal, background exactly where the restatement
has none, depth within 1e-6 relative, RGB within 1e-5 absolute, alpha equal to coverage.  Every other comparison is
bit equality or a value stated by construction.  The measured errors are recorded in DESIGN.md section 4.14.
"""
import ctypes as C
import dataclasses
import itertools

import numpy as np
import pytest
import torch

from scflow_amd import _lib, ops
from scflow_amd.mesh import MeshStore

from test_gpu_render import _render
from test_render_host import (CLIP_FACES, LIGHTS, SCENE_LISTS, TIE_POSE, TIE_SIZE, TIE_Z, check_ambiguous_cap,
                              clip_scenes, colored_icosphere, cube, duplicate_face_scene, light_batch_scenes,
                              anisotropic_scenes, ragged_scenes, render_reference, shared_edge_scene, skip_scene)

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu
DEPTH_REL, RGB_ABS = 1e-6, 1e-5
U = 2.0 ** -24                                  # fp32 unit roundoff
OUTPUTS = ('zbuf', 'pix_to_face', 'images', 'rgb')


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32),
                                                                            b.contiguous().view(torch.int32)))


def compare(out, i, ref, what, background=(.5, .5, .5)):
    """sample i of a launch against a restatement -> the measured worst errors and the ambiguous share."""
    share = check_ambiguous_cap(ref, what)
    ok = ~ref['ambiguous']
    face = out['pix_to_face'][i].numpy()
    z = out['zbuf'][i].numpy().astype(np.float64)
    rgba = out['images'][i].numpy()
    bad = (face != ref['face']) & ok
    assert not bad.any(), f'{what}: face index differs at {np.argwhere(bad)[:5].tolist()} ({bad.sum()} px)'
    assert ((z == -1) == (ref['face'] < 0))[ok].all(), f'{what}: zbuf background'
    none = (ref['face'] < 0) & ok
    assert (rgba[none][:, :3] == np.asarray(background, np.float32)).all(), f'{what}: background colour'
    cov = (ref['face'] >= 0) & ok
    rel = np.abs(z[cov] - ref['zbuf'][cov]) / ref['zbuf'][cov]
    err = np.abs(rgba[..., :3].astype(np.float64) - ref['rgb'])[ok]
    m = dict(depth=float(rel.max()) if rel.size else 0.0, rgb=float(err.max()) if err.size else 0.0, ambiguous=share)
    print(f"[measured] {what}: depth rel err {m['depth']:.3g}, rgb abs err {m['rgb']:.3g}, ambiguous {share:.3%}")
    assert m['depth'] <= DEPTH_REL, f"{what}: depth rel err {m['depth']:.2e}"
    assert m['rgb'] <= RGB_ABS, f"{what}: rgb err {m['rgb']:.2e}"
    np.testing.assert_array_equal(rgba[..., 3], (face >= 0).astype(np.float32), err_msg=f'{what}: alpha')
    return m


def render_scene(s, **kw):
    return _render(MeshStore({0: s.mesh}), [0], [s.pose], [s.K], s.H, s.W, **kw)


# ------------------------------------------------------------------------------------------- every scene, every light
# SUBPIXEL's restatement takes over a second per setting: it runs under the shipped lights only
CASES = [(which, li) for which in ('RAGGED', 'ANISOTROPIC', 'CLOSE', 'FULL_CHUNK') for li in range(4)] + [('SUBPIXEL', 0)]


@pytest.mark.parametrize('which,li', CASES)
def test_scene_lists_vs_restatement(which, li):
    lights = LIGHTS[li]
    worst = dict(depth=0.0, rgb=0.0, ambiguous=0.0)
    for s in SCENE_LISTS[which]():
        assert s.all_lights or li == 0
        out = render_scene(s, **lights)
        assert out['zbuf'].shape == (1, s.H, s.W) and out['images'].shape == (1, s.H, s.W, 4)
        ref = s.reference(batch_zmin=None if li < 3 else s.zmin(), **lights)
        m = compare(out, 0, ref, f'{s.name} lights {li}')
        worst = {k: max(worst[k], m[k]) for k in worst}
        assert (out['pix_to_face'][0] >= 0).float().mean() >= s.min_cover - 0.01
        if min(s.H, s.W) == 1:          # one sampling point for the whole long axis: every pixel is the same pixel
            for k in ('zbuf', 'pix_to_face', 'images'):
                flat = out[k][0].reshape(s.H * s.W, -1)
                assert same_bits(flat, flat[:1].expand_as(flat)), (s.name, k)
    print(f"[measured] {which} lights {li} worst: depth {worst['depth']:.3g}, rgb {worst['rgb']:.3g}, "
          f"ambiguous {worst['ambiguous']:.3%}")


@pytest.mark.parametrize('li', range(4))
def test_light_batch(li):
    """one batch with max(zmin - 400, 0) on both sides of the max, and, for the non-separate non-default setting, a
    batch-wide znear that comes from sample 0 while samples 1 and 2 are checked too."""
    scenes = light_batch_scenes()
    s0 = scenes[0]
    bz = min(s.zmin() for s in scenes)
    assert bz == s0.zmin() and np.floor(bz / 100) < np.floor(scenes[1].zmin() / 100)
    out = _render(MeshStore({0: s0.mesh}), [0] * 3, [s.pose for s in scenes], [s.K for s in scenes], s0.H, s0.W,
                  **LIGHTS[li])
    for i, s in enumerate(scenes):
        compare(out, i, s.reference(batch_zmin=bz if li == 3 else None, **LIGHTS[li]), f'{s.name} lights {li}')


# --------------------------------------------------------------------------------------------------- norm=
NORMS = [((0.4, 0.45, 0.5), (0.22, 0.23, 0.24)),
         ((123.675 / 255, 116.28 / 255, 103.53 / 255), (58.395 / 255, 57.12 / 255, 57.375 / 255))]


@pytest.mark.parametrize('mean,std', NORMS)
def test_norm_vs_restatement(mean, std):
    """rgb (NCHW) against y = (ref_rgb - mean) / std in float64.  The kernel computes fl(fl(g - m) / s) with g its
    fp32 colour, |g - ref_rgb| <= 1e-5 (the RGB bound, which includes g's own rounding), m = fl32(mean), |m - mean| <=
    U |mean|, and s = fl32(std) = std (1 + e3).  So g - m = (ref_rgb - mean) + d with |d| <= 1e-5 + U |mean|, and
    the subtraction's and the division's roundings and e3 multiply by (1 + theta), |theta| <= 3 U + O(U^2):
    |got - y| <= (|d| / |std| + 3 U |y|) (1 + 2^-20), the last factor covering the second-order terms."""
    s = ragged_scenes()[0]
    assert (s.H, s.W) == (50, 37)
    out = render_scene(s, norm=(mean, std))
    ref = s.reference()
    compare(out, 0, ref, f'{s.name} with norm')
    mean, std = np.asarray(mean, np.float64), np.asarray(std, np.float64)
    y = (ref['rgb'] - mean) / std
    got = out['rgb'][0].permute(1, 2, 0).numpy().astype(np.float64)
    assert out['rgb'].shape == (1, 3, s.H, s.W)
    bound = ((RGB_ABS + U * np.abs(mean)) / np.abs(std) + 3 * U * np.abs(y)) * (1 + 2.0 ** -20)
    ok = ~ref['ambiguous']
    ratio = (np.abs(got - y) / bound)[ok]
    print(f'[measured] norm std {std[0]:.3f}: worst error / bound {ratio.max():.3g}')
    assert ratio.max() <= 1
    # and exactly the kernel's own expression of its own colour
    g = out['images'][0, ..., :3]
    want = (g - torch.tensor(mean, dtype=torch.float32)) / torch.tensor(std, dtype=torch.float32)
    assert same_bits(out['rgb'][0].permute(1, 2, 0).contiguous(), want)


# --------------------------------------------------------------------------------------------------- ties
@pytest.mark.parametrize('axis', [0, 1])
@pytest.mark.parametrize('first', [0, 1])
def test_shared_edge_on_the_sampling_points(axis, first):
    """both faces that own the shared edge cover the pixels of the line (no crack), their depths are the same bits
    (shared_edge_scene says why), and the lower face index, 1, of the quad listed first, wins: its colour, depth 500."""
    mesh, K, (rows, cols), winner, alone = shared_edge_scene(axis, first)
    out = _render(MeshStore({0: mesh}), [0], [TIE_POSE], [K], TIE_SIZE, TIE_SIZE)
    one = _render(MeshStore({0: alone}), [0], [TIE_POSE], [K], TIE_SIZE, TIE_SIZE)
    face = out['pix_to_face'][0].numpy()
    np.testing.assert_array_equal(face[rows, cols], winner)
    assert (out['zbuf'][0].numpy()[rows, cols] == np.float32(TIE_Z)).all()
    # the winner's quad alone has the same face there, and the same bits: the other quad changes nothing on the line
    np.testing.assert_array_equal(one['pix_to_face'][0].numpy()[rows, cols], winner)
    assert same_bits(out['images'][0][rows, cols], one['images'][0][rows, cols])
    ref_one = render_reference(alone, *TIE_POSE, K, TIE_SIZE, TIE_SIZE)
    err = np.abs(out['images'][0].numpy()[rows, cols, :3].astype(np.float64) - ref_one['rgb'][rows, cols])
    assert err.max() <= RGB_ABS and (out['images'][0].numpy()[rows, cols, 3] == 1).all()
    # one pixel to either side the quads are alone: faces of the first quad (0, 1) on its side, (2, 3) on the other
    side = -1 if first == 0 else 1
    dr, dc = (0, side) if axis == 0 else (side, 0)
    assert (face[rows + dr, cols + dc] <= 1).all() and (face[rows + dr, cols + dc] >= 0).all()
    assert (face[rows - dr, cols - dc] >= 2).all()
    compare(out, 0, render_reference(mesh, *TIE_POSE, K, TIE_SIZE, TIE_SIZE), f'shared edge axis {axis} first {first}')


@pytest.mark.parametrize('first', [0, 1])
def test_duplicate_face_reports_the_lower_index(first):
    mesh, alone, pose, K, H, W = duplicate_face_scene(first)
    out = _render(MeshStore({0: mesh}), [0], [pose], [K], H, W)
    one = _render(MeshStore({0: alone}), [0], [pose], [K], H, W)
    assert (out['pix_to_face'] >= 0).float().mean() > 0.1
    assert int(out['pix_to_face'].max()) == 0               # never face 1
    for k in ('zbuf', 'pix_to_face', 'images'):             # and face 0's colour: the bits of face 0 rendered alone
        assert same_bits(out[k], one[k]), k
    compare(one, 0, render_reference(alone, *pose, K, H, W), f'duplicate face, first {first}')


# --------------------------------------------------------------------------------------------------- skipped faces
def test_zero_area_and_out_of_range_faces_are_skipped():
    """the class under test sits between two others, so the twin's indices -1 and nv stay inside the store."""
    s, oob, _, _ = skip_scene()
    others = {0: cube(100.0), 2: colored_icosphere(1, 50.0)}
    a = _render(MeshStore({**others, 1: s.mesh}), [1], [s.pose], [s.K], s.H, s.W)
    b = _render(MeshStore({**others, 1: oob}), [1], [s.pose], [s.K], s.H, s.W)
    for k in ('zbuf', 'pix_to_face', 'images'):
        assert same_bits(a[k], b[k]), k
    compare(a, 0, s.reference(), s.name)


def test_max_faces_clips_the_face_list():
    first, full, cb = clip_scenes()
    dm = MeshStore({0: cb.mesh, 1: full}).on(DEV)
    assert dm.max_faces == len(full.faces)
    clipped = dataclasses.replace(dm, max_faces=CLIP_FACES)
    t = lambda a: torch.tensor(np.stack(a), device=DEV)   # noqa: E731
    out = ops.render_mesh(clipped, torch.tensor([1, 0], device=DEV), t([first.pose[0], cb.pose[0]]),
                          t([first.pose[1], cb.pose[1]]), t([first.K, cb.K]), (first.H, first.W))
    out = {k: v.cpu() for k, v in out.items() if v is not None}
    assert int(out['pix_to_face'][0].max()) < CLIP_FACES
    compare(out, 0, first.reference(), first.name)
    compare(out, 1, cb.reference(), cb.name)


# --------------------------------------------------------------------------------------------------- containment
@pytest.mark.parametrize('li', range(4))
def test_bad_samples_stay_inside_themselves(li):
    """a NaN in R, a NaN in t and a label without a mesh render background and leave the other samples' bits alone.
    Nothing here is out of bounds: the kernel's isfinite(area) and label-range guards are what is under test."""
    H, W = 31, 64
    a, b = anisotropic_scenes()[2], light_batch_scenes()[1]
    assert (a.H, a.W) == (b.H, b.W) == (H, W)
    store = MeshStore({0: a.mesh, 2: b.mesh})
    labels = [0, 0, 2, 1, 2, 0]
    poses = [a.pose, a.pose, b.pose, a.pose, b.pose, a.pose]
    Ks = [a.K, a.K, b.K, a.K, b.K, a.K]
    bad_r = a.pose[0].copy()
    bad_r[0, 1] = np.nan
    bad_t = b.pose[1].copy()
    bad_t[2] = np.nan
    poses[1], poses[2] = (bad_r, a.pose[1]), (b.pose[0], bad_t)
    out = _render(store, labels, poses, Ks, H, W, **LIGHTS[li])
    for i in (1, 2, 3):
        assert (out['zbuf'][i] == -1).all() and (out['pix_to_face'][i] == -1).all(), i
        assert (out['images'][i][..., 3] == 0).all() and (out['images'][i][..., :3] == 0.5).all(), i
    valid = [0, 4, 5]
    if li == 3:       # the batch-wide znear is part of the result: the valid samples as a batch of their own
        alone = _render(store, [labels[i] for i in valid], [poses[i] for i in valid], [Ks[i] for i in valid], H, W,
                        **LIGHTS[li])
        singles = [{k: alone[k][j:j + 1] for k in ('zbuf', 'pix_to_face', 'images')} for j in range(3)]
    else:
        singles = [_render(store, [labels[i]], [poses[i]], [Ks[i]], H, W, **LIGHTS[li]) for i in valid]
    for i, one in zip(valid, singles):
        assert (one['pix_to_face'] >= 0).any()
        for k in ('zbuf', 'pix_to_face', 'images'):
            assert same_bits(out[k][i], one[k][0]), (i, k)
    bz = min(a.zmin(), b.zmin())
    compare(out, 0, a.reference(batch_zmin=bz if li == 3 else None, **LIGHTS[li]), f'{a.name} beside bad samples')
    compare(out, 4, b.reference(batch_zmin=bz if li == 3 else None, **LIGHTS[li]), f'{b.name} beside bad samples')


# --------------------------------------------------------------------------------------------------- outputs
def _pair_50x37():
    a, b = ragged_scenes()[0], anisotropic_scenes()[0]
    assert (a.H, a.W) == (b.H, b.W) == (50, 37)
    return a, b, MeshStore({0: a.mesh, 1: b.mesh})


def test_output_combinations_and_background():
    a, b, store = _pair_50x37()
    args = (store, [0, 1], [a.pose, b.pose], [a.K, b.K], 50, 37)
    full = _render(*args, images=True, pix_to_face=True, norm=NORMS[0])
    compare(full, 0, a.reference(), a.name)
    compare(full, 1, b.reference(), b.name)
    for images, p2f, norm in itertools.product((False, True), (False, True), (None, NORMS[0])):
        out = _render(*args, images=images, pix_to_face=p2f, norm=norm)
        assert same_bits(out['zbuf'], full['zbuf']), (images, p2f, norm)
        for k, present in (('images', images), ('pix_to_face', p2f), ('rgb', norm is not None)):
            assert (out[k] is not None) == present, (k, images, p2f, norm)
            assert out[k] is None or same_bits(out[k], full[k]), (k, images, p2f, norm)
    bg = (0.1, 0.7, 0.25)
    out = _render(*args, background=bg, norm=NORMS[0])
    none = out['pix_to_face'] < 0
    assert same_bits(out['zbuf'], full['zbuf']) and same_bits(out['pix_to_face'], full['pix_to_face'])
    assert same_bits(out['images'][~none], full['images'][~none])
    want = torch.tensor(bg + (0.,), dtype=torch.float32)
    assert none.any() and same_bits(out['images'][none], want.expand(int(none.sum()), 4))
    g = out['images'][..., :3]
    norm_bg = (g - torch.tensor(NORMS[0][0], dtype=torch.float32)) / torch.tensor(NORMS[0][1], dtype=torch.float32)
    assert same_bits(out['rgb'].permute(0, 2, 3, 1).contiguous(), norm_bg)
    compare(out, 0, a.reference(background=bg), f'{a.name} background {bg}', background=bg)
    compare(out, 1, b.reference(background=bg), f'{b.name} background {bg}', background=bg)


# --------------------------------------------------------------------------------------------------- guard bands
GUARD = 64                    # elements on either side: 256 bytes, so every output pointer keeps its 16-byte alignment
SENTINEL = -7777.25


def _guarded(n, dtype):
    fill = SENTINEL if dtype == torch.float32 else -7777
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0 and buf[GUARD:].data_ptr() % 16 == 0
    return buf, buf[GUARD:GUARD + n]


def test_guard_bands_round_the_four_outputs():
    """the raw entry at N = 2, 50 x 37 (4 x 3 tiles of which the last row and column are ragged) into
    sentinel-filled buffers: the 64 elements before and after each output are untouched, the outputs are those of
    ops.render_mesh."""
    a, b, store = _pair_50x37()
    N, H, W = 2, 50, 37
    dm = store.on(DEV)
    t = lambda x, dt=torch.float32: torch.tensor(np.stack(x), dtype=dt, device=DEV)   # noqa: E731
    lab, R, tr, K = (t([0, 1], torch.int32), t([a.pose[0], b.pose[0]]), t([a.pose[1], b.pose[1]]), t([a.K, b.K]))
    want = ops.render_mesh(dm, lab, R, tr, K, (H, W), norm=NORMS[0])
    bufs = dict(zbuf=_guarded(N * H * W, torch.float32), pix_to_face=_guarded(N * H * W, torch.int32),
                images=_guarded(N * H * W * 4, torch.float32), rgb=_guarded(N * 3 * H * W, torch.float32))
    ms = _lib.MeshStore(dm.verts.data_ptr(), dm.normals.data_ptr(), dm.colors.data_ptr(), dm.faces.data_ptr(),
                        dm.vert_offset.data_ptr(), dm.face_offset.data_ptr(), int(dm.num_classes), int(dm.max_faces))
    f3 = C.c_float * 3
    p = _lib.RenderParams(H, W, 1, 1, f3(.5, .5, .5), f3(*NORMS[0][0]), f3(*NORMS[0][1]))
    lib = _lib.load()
    ws = torch.empty((int(lib.scf_render_workspace_bytes(N, int(dm.max_faces))),), dtype=torch.uint8, device=DEV)
    assert all(v.data_ptr() % 16 == 0 for _, v in bufs.values()) and ws.data_ptr() % 16 == 0
    rc = lib.scf_render_mesh(C.byref(ms), lab.data_ptr(), R.data_ptr(), tr.data_ptr(), K.data_ptr(), N, C.byref(p),
                             bufs['zbuf'][1].data_ptr(), bufs['pix_to_face'][1].data_ptr(),
                             bufs['images'][1].data_ptr(), bufs['rgb'][1].data_ptr(), ws.data_ptr(), ops._stream())
    torch.cuda.synchronize()
    assert rc == 0
    for k in OUTPUTS:
        buf, view = bufs[k]
        sentinel = torch.full_like(buf, SENTINEL if buf.dtype == torch.float32 else -7777)
        assert same_bits(buf[:GUARD], sentinel[:GUARD]), f'{k}: band before the output written'
        assert same_bits(buf[GUARD + view.numel():], sentinel[GUARD + view.numel():]), f'{k}: band after the output written'
        assert same_bits(view, want[k].reshape(-1)), k
        assert not (view == sentinel[0]).any(), f'{k}: an output element was never written'
