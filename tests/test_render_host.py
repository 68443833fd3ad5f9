"""CPU: the mesh renderer's host side -- PLY reader, labels from file names, MeshRenderer's option checks, the
pixel sampling formula, the C entry points' argument checks -- and ``render_reference``, a float64 brute-force
restatement of the semantics render.hip states, checked here on closed-form cases and used by
test_gpu_render.py as the yardstick."""
import ctypes as C
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import scflow_amd
from scflow_amd import _lib, ops
from scflow_amd.mesh import MeshRenderer, MeshStore, icosphere, label_from_path, make_mesh, read_ply

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------ float64 restatement
def pixel_coord(i, size, other):
    """u(c) = (W-1)/2 - (S-1)(W-2c-1)/(2S), S = min(H, W)."""
    s = min(size, other)
    return (size - 1) / 2 - (s - 1) * (size - 2 * np.asarray(i, dtype=np.float64) - 1) / (2 * s)


def _unit(x):
    return x / np.maximum(np.linalg.norm(x, axis=-1, keepdims=True), 1e-6)


def sample_zmin(mesh, R, t):
    return float((mesh.verts.astype(np.float64) @ np.asarray(R, np.float64).T + np.asarray(t, np.float64))[:, 2].min())


def render_reference(mesh, R, t, K, H, W, default_lights=True, seperate_lights=True, background=(.5, .5, .5),
                     batch_zmin=None, edge_tol=1e-4, depth_tol=1e-6):
    """one sample, float64 from the fp32 inputs -> dict(zbuf (H,W), face (H,W), rgb (H,W,3), ambiguous (H,W) bool:
    a sampling point within edge_tol px of a covering face's edge, or a runner-up depth within depth_tol relative)."""
    R = np.asarray(R, np.float64).reshape(3, 3)
    t = np.asarray(t, np.float64).reshape(3)
    K = np.asarray(K, np.float64).reshape(3, 3)
    V = mesh.verts.astype(np.float64)
    Xc = V @ R.T + t
    z = Xc[:, 2]
    with np.errstate(divide='ignore', invalid='ignore'):
        u = K[0, 0] * Xc[:, 0] / z + K[0, 2]
        v = K[1, 1] * Xc[:, 1] / z + K[1, 2]
    xs, ys = pixel_coord(np.arange(W), W, H), pixel_coord(np.arange(H), H, W)
    X, Y = np.meshgrid(xs, ys)
    best_z = np.full((H, W), np.inf)
    second = np.full((H, W), np.inf)
    best_f = np.full((H, W), -1, dtype=np.int64)
    bary = np.zeros((H, W, 3))
    amb = np.zeros((H, W), dtype=bool)
    for f, (ia, ib, ic) in enumerate(mesh.faces.astype(np.int64)):
        if z[ia] <= 0 and z[ib] <= 0 and z[ic] <= 0:
            continue
        ua, ub, uc, va, vb, vc = u[ia], u[ib], u[ic], v[ia], v[ib], v[ic]
        area = (uc - ua) * (vb - va) - (vc - va) * (ub - ua)
        if not np.isfinite(area) or area == 0:
            continue
        c0 = max(int(np.searchsorted(xs, min(ua, ub, uc))) - 1, 0)
        c1 = min(int(np.searchsorted(xs, max(ua, ub, uc))) + 1, W)
        r0 = max(int(np.searchsorted(ys, min(va, vb, vc))) - 1, 0)
        r1 = min(int(np.searchsorted(ys, max(va, vb, vc))) + 1, H)
        if c0 >= c1 or r0 >= r1:
            continue
        x, y = X[r0:r1, c0:c1], Y[r0:r1, c0:c1]
        w0 = (x - ub) * (vc - vb) - (y - vb) * (uc - ub)
        w1 = (x - uc) * (va - vc) - (y - vc) * (ua - uc)
        w2 = (x - ua) * (vb - va) - (y - va) * (ub - ua)
        sg = np.sign(area)
        # signed distance of the sampling point to each edge's line, positive inside: the smallest one within
        # edge_tol of 0 means the point is within edge_tol of the triangle's boundary
        dmin = np.minimum(np.minimum(w0 * sg / np.hypot(uc - ub, vc - vb), w1 * sg / np.hypot(ua - uc, va - vc)),
                          w2 * sg / np.hypot(ub - ua, vb - va))
        b = np.stack([w0, w1, w2], -1) / area
        inside = (b >= 0).all(-1)
        with np.errstate(divide='ignore', invalid='ignore'):
            pb = b / np.array([z[ia], z[ib], z[ic]])
            q = pb.sum(-1)
            zz = 1.0 / q
        hit = inside & (zz > 0) & np.isfinite(zz)
        sub_amb = amb[r0:r1, c0:c1]
        sub_amb |= np.abs(dmin) < edge_tol
        bz, sz, bf, bb = best_z[r0:r1, c0:c1], second[r0:r1, c0:c1], best_f[r0:r1, c0:c1], bary[r0:r1, c0:c1]
        better = hit & (zz < bz)
        sz[hit & ~better] = np.minimum(sz[hit & ~better], zz[hit & ~better])
        sz[better] = bz[better]
        bz[better] = zz[better]
        bf[better] = f
        bb[better] = (pb / q[..., None])[better]
    covered = best_f >= 0
    with np.errstate(invalid="ignore"):
        amb |= covered & (np.abs(second - best_z) <= depth_tol * best_z)
    rgb = np.broadcast_to(np.asarray(background, np.float64), (H, W, 3)).copy()
    if covered.any():
        fv = mesh.faces.astype(np.int64)[best_f[covered]]
        B = bary[covered]
        interp = lambda a: np.einsum('pk,pkj->pj', B, a.astype(np.float64)[fv])   # noqa: E731
        p, n, col = interp(mesh.verts), interp(mesh.normals), interp(mesh.colors)
        la, ld, ls = (.5, .3, .2) if default_lights else (.8, .5, 1.)
        if seperate_lights:
            L = R @ np.array([0, 0, max(sample_zmin(mesh, R, t) - 400, 0)])
        elif default_lights:
            L = np.array([0., 1., 0.])
        else:
            L = R @ np.array([0, 0, np.floor(batch_zmin / 100) * 100 / 4])
        cam = -R.T @ t
        n, l, vd = _unit(n), _unit(L - p), _unit(cam - p)
        cosang = (n * l).sum(-1)
        diffuse = ld * np.maximum(cosang, 0)
        refl = 2 * cosang[:, None] * n - l
        spec = ls * (np.maximum((vd * refl).sum(-1), 0) * (cosang > 0)) ** 64
        rgb[covered] = (la + diffuse)[:, None] * col + spec[:, None]
    return dict(zbuf=np.where(covered, best_z, -1.0), face=best_f, rgb=rgb, ambiguous=amb)


# ------------------------------------------------------------------------------------------- scenes
def look_at_pose(rx, ry, rz, tz, tx=0., ty=0.):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return (Rz @ Ry @ Rx).astype(np.float32), np.array([tx, ty, tz], dtype=np.float32)


def intrinsics(f, H, W):
    return np.array([[f, 0, (W - 1) / 2 + 0.3], [0, f, (H - 1) / 2 - 0.2], [0, 0, 1]], dtype=np.float32)


def colored_icosphere(subdiv, radius):
    v, f = icosphere(subdiv, radius)
    col = 0.5 + 0.5 * v / radius
    return make_mesh(v, f, colors=col)


def cube(size):
    s = size / 2
    v = np.array([[x, y, z] for x in (-s, s) for y in (-s, s) for z in (-s, s)], dtype=np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = [(a, b, c) for a, b, c, d in quads] + [(a, c, d) for a, b, c, d in quads]
    col = (v / size + 0.5).clip(0, 1)
    return make_mesh(v, f, colors=col)


# ------------------------------------------------------------------------------------------- PLY
def _write_ply(path, verts, faces, normals=None, colors=None, binary=False, fmt=None, color_type='uchar'):
    props = [('float', 'x'), ('float', 'y'), ('float', 'z')]
    cols = [verts]
    if normals is not None:
        props += [('float', 'nx'), ('float', 'ny'), ('float', 'nz')]
        cols.append(normals)
    if colors is not None:
        props += [(color_type, 'red'), (color_type, 'green'), (color_type, 'blue'), (color_type, 'alpha')]
        c = np.concatenate([colors, np.ones((len(colors), 1))], 1)
        cols.append(np.round(c * 255) if color_type == 'uchar' else c)
    fmt = fmt or ('binary_little_endian' if binary else 'ascii')
    head = ['ply', f'format {fmt} 1.0', 'comment written by the test', f'element vertex {len(verts)}']
    head += [f'property {t} {n}' for t, n in props]
    head += [f'element face {len(faces)}', 'property list uchar int vertex_indices', 'end_header']
    with open(path, 'wb') as fh:
        fh.write(('\n'.join(head) + '\n').encode())
        table = np.concatenate(cols, 1)
        for row in table:
            if binary:
                fh.write(b''.join(struct.pack('<B' if t == 'uchar' else '<f', int(x) if t == 'uchar' else x)
                                  for (t, _), x in zip(props, row)))
            else:
                fh.write((' '.join(str(int(x)) if t == 'uchar' else repr(float(x)) for (t, _), x in zip(props, row))
                          + '\n').encode())
        for f in faces:
            if binary:
                fh.write(struct.pack('<B', len(f)) + struct.pack(f'<{len(f)}i', *f))
            else:
                fh.write((' '.join(map(str, [len(f), *f])) + '\n').encode())


@pytest.mark.parametrize('binary', [False, True])
@pytest.mark.parametrize('with_normals', [False, True])
@pytest.mark.parametrize('color_type', [None, 'uchar', 'float'])
def test_ply_reader_roundtrip(tmp_path, binary, with_normals, color_type):
    v, f = icosphere(1, 30.0)
    g = np.random.default_rng(0)
    nrm = g.normal(size=v.shape).astype(np.float32) if with_normals else None
    col = (np.round(g.random(v.shape) * 255) / 255).astype(np.float32) if color_type else None
    p = str(tmp_path / 'obj_000003.ply')
    _write_ply(p, v, f, nrm, col, binary=binary, color_type=color_type or 'uchar')
    m = read_ply(p)
    np.testing.assert_array_equal(m.verts, v)
    np.testing.assert_array_equal(m.faces, f)
    if with_normals:
        np.testing.assert_array_equal(m.normals, nrm)                    # the file's normals, as they are
    else:
        fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])  # area-weighted: the sphere's radial direction
        assert np.allclose(np.linalg.norm(m.normals, axis=1), 1, atol=1e-6)
        assert (np.sum(m.normals * v, 1) > 0).all() and fn.shape == f.shape
    if color_type:
        np.testing.assert_allclose(m.colors, col, atol=1e-7)
    else:
        assert (m.colors == 1).all()


@pytest.mark.parametrize('binary', [False, True])
def test_ply_reader_rejects_quads_and_unknown_formats(tmp_path, binary):
    v = np.zeros((4, 3), np.float32)
    p = str(tmp_path / 'quad.ply')
    _write_ply(p, v, [(0, 1, 2), (0, 1, 2, 3)], binary=binary)
    with pytest.raises(ValueError, match='triangles only'):
        read_ply(p)
    _write_ply(p, v, [(0, 1, 2, 3)], binary=binary)
    with pytest.raises(ValueError, match='triangles only'):
        read_ply(p)
    _write_ply(p, v, [(0, 1, 2)], fmt='binary_big_endian')
    with pytest.raises(ValueError, match='binary_big_endian'):
        read_ply(p)
    open(p, 'wb').write(b'not a ply\n')
    with pytest.raises(ValueError):
        read_ply(p)


def test_labels_from_file_names(tmp_path):
    assert label_from_path('/x/obj_000001.ply') == 0
    assert label_from_path('obj_000021.ply') == 20
    assert label_from_path('models/mesh_7.ply') == 6
    v, f = icosphere(0, 10.0)
    for name in ('obj_000002.ply', 'obj_000005.ply'):
        _write_ply(str(tmp_path / name), v, f, binary=True)
    store = MeshStore.from_paths(str(tmp_path))
    assert sorted(store.meshes) == [1, 4] and store.num_classes == 5
    assert store.face_offset.tolist() == [0, 0, 20, 20, 20, 40] and store.max_faces == 20


# ------------------------------------------------------------------------------------------- options
SHIPPED = dict(shader_type='Phong', soft_blending=False, render_mask=False, render_image=True, seperate_lights=True,
               faces_per_pixel=1, blur_radius=0., sigma=1e-12, gamma=1e-12, background_color=(.5, .5, .5))


def _store():
    return MeshStore({0: colored_icosphere(1, 50.0)})


def test_renderer_rejects_unsupported_options():
    r = MeshRenderer(_store(), (64, 96), **SHIPPED)
    assert r.image_size == (64, 96) and r.seperate_lights and r.default_lights
    for key, value, word in (('soft_blending', True, 'soft_blending'), ('render_mask', True, 'render_mask'),
                             ('faces_per_pixel', 2, 'faces_per_pixel'), ('blur_radius', 1e-3, 'blur_radius'),
                             ('shader_type', 'Gouraud', 'Gouraud'), ('shader_type', 'Flat', 'Flat'),
                             ('render_image', False, 'render_image')):
        with pytest.raises(NotImplementedError, match=word):
            MeshRenderer(_store(), (64, 64), **{**SHIPPED, key: value})
    with pytest.raises(NotImplementedError, match='soft_blending'):
        MeshRenderer(_store(), (64, 64))                    # the reference's own defaults are soft


# --------------------------------------------------------------------------------------- sampling points
def test_pixel_sampling_formula():
    # 256 x 256: u(c) = c * 255/256 + 255/512 (derived by hand from scale = 255/2, c0 = 255/2, x_ndc = (255 - 2c)/256)
    for c in (0, 1, 100, 255):
        want = c * 255 / 256 + 255 / 512
        assert ops.render_pixel_coord(c, 256, 256) == pytest.approx(want, abs=1e-12)
        assert pixel_coord(c, 256, 256) == pytest.approx(want, abs=1e-12)
    # H = 64, W = 96: S = 64.  Columns: u(c) = 47.5 - 63 (95 - 2c) / 128; rows: v(r) = 31.5 - 63 (63 - 2r) / 128
    assert ops.render_pixel_coord(0, 96, 64) == pytest.approx(47.5 - 63 * 95 / 128, abs=1e-12)
    assert ops.render_pixel_coord(95, 96, 64) == pytest.approx(47.5 + 63 * 95 / 128, abs=1e-12)
    assert ops.render_pixel_coord(0, 64, 96) == pytest.approx(31.5 - 63 * 63 / 128, abs=1e-12)
    assert ops.render_pixel_coord(40, 64, 96) == pytest.approx(31.5 - 63 * (63 - 80) / 128, abs=1e-12)
    for i in range(96):
        assert ops.render_pixel_coord(i, 96, 64) == pytest.approx(float(pixel_coord(i, 96, 64)), abs=1e-12)
    # the grid is evenly spaced by (S-1)/S and centred on (size-1)/2
    assert ops.render_pixel_coord(48, 96, 64) - ops.render_pixel_coord(47, 96, 64) == pytest.approx(63 / 64)
    assert ops.render_pixel_coord(47, 96, 64) + ops.render_pixel_coord(48, 96, 64) == pytest.approx(95)


# ----------------------------------------------------------------------------------------- C ABI, host side
def test_render_entry_points_validate_on_the_host():
    lib = _lib.load()
    assert lib.scf_render_workspace_bytes(0, 10) == -1 and lib.scf_render_workspace_bytes(4, 0) == -1
    assert lib.scf_render_workspace_bytes(2, 100) >= 2 * 100 * (8 + 48)
    p = _lib.RenderParams(64, 64, 1, 1)
    p.norm_std[:] = [1, 1, 1]
    m = _lib.MeshStore(None, None, None, None, None, None, 1, 1)
    assert lib.scf_render_mesh(None, None, None, None, None, 1, C.byref(p), None, None, None, None, None, None) == -1
    assert lib.scf_render_mesh(C.byref(m), None, None, None, None, 1, None, None, None, None, None, None, None) == -1
    fake = 16     # never dereferenced: every check fails first
    m2 = _lib.MeshStore(fake, fake, fake, fake, fake, fake, 1, 1)
    for bad in (dict(H=0), dict(W=9000), dict(H=-3)):
        q = _lib.RenderParams(64, 64, 1, 1)
        for k, v in bad.items():
            setattr(q, k, v)
        assert lib.scf_render_mesh(C.byref(m2), fake, fake, fake, fake, 1, C.byref(q), fake, None, None, None, fake,
                                   None) == -1
    q = _lib.RenderParams(64, 64, 1, 1)                       # rgb_nchw requested with a zero std
    assert lib.scf_render_mesh(C.byref(m2), fake, fake, fake, fake, 1, C.byref(q), fake, None, None, fake, fake,
                               None) == -1
    assert lib.scf_render_mesh(C.byref(m2), fake, fake, fake, fake, 0, C.byref(p), fake, None, None, None, fake,
                               None) == -1
    m3 = _lib.MeshStore(fake, fake, fake, fake, fake, fake, 0, 1)
    assert lib.scf_render_mesh(C.byref(m3), fake, fake, fake, fake, 1, C.byref(p), fake, None, None, None, fake,
                               None) == -1


def test_render_struct_layouts_match_c():
    src = ('#include "scflow_hip.h"\n#include <stdio.h>\nint main(){printf("%zu %zu\\n", sizeof(scf_mesh_store), '
           'sizeof(scf_render_params));return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, 't.c')
        open(c, 'w').write(src)
        exe = os.path.join(d, 't')
        subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), c, '-o', exe], check=True)
        ms, ps = map(int, subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split())
    assert ms == C.sizeof(_lib.MeshStore) and ps == C.sizeof(_lib.RenderParams)


def test_render_mesh_op_rejects_cpu_tensors():
    store = _store()
    with pytest.raises(Exception):
        ops.render_mesh(store.on('cpu'), torch.zeros(1, dtype=torch.int64), torch.eye(3)[None], torch.zeros(1, 3),
                        torch.eye(3)[None], (32, 32))


# ------------------------------------------------------------------------------------------ refiner
def test_cycles_without_renderer_still_raise():
    cfg = scflow_amd.scflow_model_cfg()
    cfg['test_cfg'] = dict(iters=8, cycles=2)
    model = scflow_amd.build_refiner(cfg)
    assert model.renderer is None                         # the config's renderer dict is not built
    with pytest.raises(NotImplementedError, match='cycles'):
        model.forward(dict(), None)
    model.attach_renderer(MeshRenderer(_store(), (64, 64), **SHIPPED)).attach_renderer(None)
    with pytest.raises(NotImplementedError, match='cycles'):
        model.forward(dict(), None)
    with pytest.raises(RuntimeError, match='attach'):
        model.format_data_test(dict(img=[], annots={}, img_metas=[]))
    raft = scflow_amd.build_refiner(scflow_amd.raft_model_cfg())
    assert hasattr(raft, 'format_data_test') and raft.renderer is None


# ------------------------------------------------------------------------------------- the restatement itself
def test_reference_fronto_parallel_triangle():
    """a triangle at constant depth d, legs along the image axes: depth is exactly d and the covered set is the
    pixels whose sampling point satisfies the three half-planes, written out by hand."""
    H, W, d, f = 48, 64, 700.0, 500.0
    K = np.array([[f, 0, 30.0], [0, f, 20.0], [0, 0, 1]], np.float32)
    # image-plane corners (u, v): (10, 8), (50, 8), (10, 40) -> object points at depth d
    uv = np.array([[10, 8], [50, 8], [10, 40]], np.float64)
    verts = np.stack([(uv[:, 0] - 30) * d / f, (uv[:, 1] - 20) * d / f, np.full(3, d)], 1).astype(np.float32)
    mesh = make_mesh(verts, [(0, 1, 2)])
    out = render_reference(mesh, np.eye(3), np.zeros(3), K, H, W)
    xs, ys = pixel_coord(np.arange(W), W, H), pixel_coord(np.arange(H), H, W)
    X, Y = np.meshgrid(xs, ys)
    want = (X >= 10) & (Y >= 8) & ((X - 10) / 40 + (Y - 8) / 32 <= 1)
    assert want.sum() > 300
    np.testing.assert_array_equal(out['face'] >= 0, want)
    np.testing.assert_allclose(out['zbuf'][want], d, rtol=1e-12)
    assert (out['zbuf'][~want] == -1).all() and (out['rgb'][~want] == 0.5).all()
    # the same triangle flipped (back face) covers the same pixels: no culling
    back = make_mesh(verts, [(0, 2, 1)])
    np.testing.assert_array_equal(render_reference(back, np.eye(3), np.zeros(3), K, H, W)['face'] >= 0, want)


def test_reference_depth_order_and_behind_camera():
    H = W = 32
    K = intrinsics(60.0, H, W)
    big = np.array([[-200, -200, 0], [200, -200, 0], [0, 300, 0]], np.float32)
    near, far = big + [0, 0, 300], big + [0, 0, 500]
    mesh = make_mesh(np.concatenate([far, near]), [(0, 1, 2), (3, 4, 5)])
    out = render_reference(mesh, np.eye(3), np.zeros(3), K, H, W)
    cov = out['face'] >= 0
    assert cov.sum() > 100 and (out['face'][cov] == 1).all()
    np.testing.assert_allclose(out['zbuf'][cov], 300, rtol=1e-12)
    behind = make_mesh(big - [0, 0, 100], [(0, 1, 2)])       # every vertex at z <= 0: skipped
    assert (render_reference(behind, np.eye(3), np.zeros(3), K, H, W)['face'] == -1).all()
