"""CPU: the mesh renderer's host side -- PLY reader, labels from file names, MeshRenderer's option checks, the
pixel sampling formula, the C entry points' argument checks -- and ``render_reference``, a float64 brute-force
restatement of the semantics render.hip states, checked here on closed-form cases and used by
test_gpu_render.py and test_gpu_render_edges.py as the yardstick.  The scene lists of the latter (ragged sizes,
fx != fy, sub-pixel faces, full chunks, skipped faces, constructed ties) live here, next to the restatement, with the
cap on the pixels a comparison may leave out; the CPU tests at the end check both without a GPU."""
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
        with np.errstate(divide='ignore', invalid='ignore'):
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


def intrinsics2(fx, fy, cx, cy):
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], dtype=np.float32)


def soup(n, seed):
    """n random triangles of 40-120 mm in a 200 mm box: heavy occlusion, random winding and colours."""
    g = np.random.default_rng(seed)
    centers = g.uniform(-100, 100, size=(n, 1, 3))
    verts = (centers + g.uniform(-60, 60, size=(n, 3, 3))).reshape(-1, 3)
    return make_mesh(verts, np.arange(3 * n).reshape(n, 3), colors=g.uniform(0, 1, size=(3 * n, 3)))


# ------------------------------------------------------------------- the ambiguous set and its cap
AMBIGUOUS_CAP = 0.01
LIGHTS = [dict(default_lights=True, seperate_lights=True), dict(default_lights=True, seperate_lights=False),
          dict(default_lights=False, seperate_lights=True), dict(default_lights=False, seperate_lights=False)]


def check_ambiguous_cap(ref, what=''):
    """the cap on what a comparison may leave out: at most 1 % of an image's pixels are `ambiguous`."""
    share = float(ref['ambiguous'].sum()) / ref['ambiguous'].size
    assert share <= AMBIGUOUS_CAP, f'{what}: {share:.3%} of the pixels ambiguous (cap 1 %)'
    return share


# ----------------------------------------------------------------- scenes at the renderer's edges
class Scene:
    """one sample: mesh, pose (R, t), K, image size; `all_lights` = cheap enough to restate under the four light
    settings; `min_cover` = the share of covered pixels the restatement must at least report (a scene that renders
    nothing tests nothing)."""

    def __init__(self, name, mesh, pose, K, H, W, all_lights=True, min_cover=0.02):
        self.name, self.mesh, self.pose, self.K, self.H, self.W = name, mesh, pose, K, H, W
        self.all_lights, self.min_cover = all_lights, min_cover
        self._ref = {}

    def reference(self, default_lights=True, seperate_lights=True, batch_zmin=None, background=(.5, .5, .5)):
        """render_reference of the scene, computed once per setting and shared (never modify it)."""
        key = (default_lights, seperate_lights, batch_zmin, tuple(background))
        if key not in self._ref:
            self._ref[key] = render_reference(self.mesh, self.pose[0], self.pose[1], self.K, self.H, self.W,
                                              default_lights, seperate_lights, background, batch_zmin)
        return self._ref[key]

    def zmin(self):
        return sample_zmin(self.mesh, *self.pose)

    def __repr__(self):
        return self.name


EDGE_POSE = look_at_pose(0.3, -0.4, 0.2, 600.0, 10.0, -5.0)

# H > W, W > H, neither a multiple of the 16 x 16 tile, one tile and a part of one, min(H, W) = 1 (pixel_range's
# step = 0: every pixel of the long axis samples the same point, at (1, 5) u = 2.0 for all five columns)
RAGGED_SIZES = [(50, 37), (17, 90), (33, 33), (15, 15), (31, 64), (1, 1), (1, 5), (5, 1), (2, 3)]


def _scenes(build):
    cache = []

    def get():
        if not cache:
            cache.extend(build())
        return cache
    return get


@_scenes
def ragged_scenes():
    """an icosphere under fy = 1.3 fx and an off-centre principal point at every size with min(H, W) >= 15; below
    that a cube under fx = fy = 3, which covers the few sampling points there are."""
    out = []
    ico, cb = colored_icosphere(3, 70.0), cube(120.0)
    for H, W in RAGGED_SIZES:
        s = min(H, W)
        if s >= 15:
            K = intrinsics2(3.0 * s, 3.9 * s, (W - 1) / 2 + 2.3, (H - 1) / 2 - 1.7)
            out.append(Scene(f'ragged {H}x{W}', ico, EDGE_POSE, K, H, W, min_cover=0.05))
        else:
            K = intrinsics2(3.0, 3.0, (W - 1) / 2, (H - 1) / 2)
            out.append(Scene(f'ragged {H}x{W}', cb, EDGE_POSE, K, H, W, min_cover=1 / 6))
    return out


@_scenes
def anisotropic_scenes():
    """fx != fy by 1.5 x or more and a principal point several pixels off centre, H > W and W > H."""
    return [Scene('aniso cube 50x37', cube(120.0), EDGE_POSE, intrinsics2(90, 150, 20.3, 30.1), 50, 37, min_cover=0.3),
            Scene('aniso cube 37x50', cube(120.0), EDGE_POSE, intrinsics2(150, 90, 30.1, 14.3), 37, 50, min_cover=0.3),
            Scene('aniso icosphere 31x64', colored_icosphere(3, 70.0), look_at_pose(-0.7, 1.1, 2.5, 450.0, -20.0, 15.0),
                  intrinsics2(160, 80, 37.4, 12.2), 31, 64, min_cover=0.2)]


@_scenes
def subpixel_scenes():
    """20 480 faces on a disc of 8 px radius: about 93 faces per covered pixel, nearly every face's box is the
    +-1 widening of pixel_range and nothing else."""
    return [Scene('subpixel icosphere(5) 48x40', colored_icosphere(5, 60.0), look_at_pose(0.3, -0.4, 0.2, 900.0, 3.0, -2.0),
                  intrinsics2(120, 120, 20.1, 23.2), 48, 40, all_lights=False, min_cover=0.08)]


@_scenes
def close_scenes():
    """faces many tiles large: a cube that fills the frame from outside, and a soup straddling the image plane
    (faces partly and wholly behind the camera) at a ragged size."""
    return [Scene('close cube 37x50', cube(120.0), look_at_pose(0.05, -0.03, 0.02, 110.0, 2.0, -1.0),
                  intrinsics2(60, 60, 24.8, 17.7), 37, 50, min_cover=1.0),
            Scene('close soup 37x50', soup(200, 11), look_at_pose(0.1, 0.2, 0.0, 40.0),
                  intrinsics2(60, 45, 25.3, 17.1), 37, 50, min_cover=0.3)]


def stacked_triangles(n, reverse):
    """n triangles far larger than the view, 10 mm apart in depth from z = 0 (object frame), one colour each; face
    k is the k-th nearest, or with `reverse` the k-th farthest (the nearest is then face n - 1)."""
    g = np.random.default_rng(5)
    tri = np.array([[-9000, -6000, 0], [9000, -6000, 0], [0, 12000, 0]], np.float64)
    order = np.arange(n)[::-1] if reverse else np.arange(n)
    verts = np.concatenate([tri + [0, 0, 10.0 * d] for d in order])
    colors = np.repeat(g.uniform(0.1, 1, size=(n, 3)), 3, axis=0)
    return make_mesh(verts, np.arange(3 * n).reshape(n, 3), colors=colors)


@_scenes
def full_chunk_scenes():
    """300 faces that each cover the whole image: every one of the first chunk's 256 faces hits every tile (the
    compacted list is full), and with the list reversed the winner, face 299, sits in the second chunk."""
    pose = look_at_pose(0.02, -0.03, 0.01, 500.0, 4.0, -3.0)
    K = intrinsics2(40, 52, 17.2, 15.1)
    return [Scene('full chunk, winner 299', stacked_triangles(300, True), pose, K, 33, 33, min_cover=1.0),
            Scene('full chunk, winner 0', stacked_triangles(300, False), pose, K, 33, 33, min_cover=1.0)]


@_scenes
def light_batch_scenes():
    """one batch of three: zmin - 400 is negative for the first (the light sits at the origin) and positive for
    the others, and the batch-wide znear of the non-separate, non-default setting comes from the first alone."""
    ico = colored_icosphere(2, 70.0)
    K = intrinsics2(70, 95, 33.9, 13.8)
    return [Scene(f'light batch tz={tz}', ico, look_at_pose(0.3, -0.4, 0.2, tz, 10.0, -5.0), K, 31, 64, min_cover=0.01)
            for tz in (300.0, 600.0, 900.0)]


SCENE_LISTS = dict(RAGGED=ragged_scenes, ANISOTROPIC=anisotropic_scenes, SUBPIXEL=subpixel_scenes, CLOSE=close_scenes,
                   FULL_CHUNK=full_chunk_scenes, LIGHT_BATCH=light_batch_scenes)


# ------------------------------------------------------------------------------------------- skipped faces
SKIP_FACES = (0, 68, 128, 148, 255, 257, 308, 319)  # the first, the last, around the chunk boundary of 256, and five
                                                    # that skip_scene's pose sees (68, 128, 148, 257, 308)


def skipped_face_meshes():
    """(degenerate, out_of_range, clean): an icosphere(2) in which the faces SKIP_FACES are, alternately, (a, a, c)
    and three collinear vertices; its twin in which the same faces carry the vertex indices -1 and nv; and the
    mesh with those faces removed, with the map from its face indices to the twins'.  The collinear vertices are
    appended (inside the sphere), and all three meshes share vertices, normals and colours, so the kept faces shade
    alike.  make_mesh refuses indices outside the mesh: the twin is built as a Mesh directly."""
    from scflow_amd.mesh import Mesh
    base = colored_icosphere(2, 60.0)
    extra = np.array([[-20, -10, 5], [0, 0, 5], [20, 10, 5]], np.float32)        # collinear, exactly
    verts = np.concatenate([base.verts, extra])
    normals = np.concatenate([base.normals, np.tile(np.float32([0, 0, 1]), (3, 1))])
    colors = np.concatenate([base.colors, np.full((3, 3), 0.9, np.float32)])
    nv, nb = len(verts), len(base.verts)
    deg, oob = base.faces.copy(), base.faces.copy()
    for j, f in enumerate(SKIP_FACES):
        a, _, c = base.faces[f]
        deg[f] = (a, a, c) if j % 2 == 0 else (nb, nb + 1, nb + 2)
        oob[f] = (a, -1, c) if j % 2 == 0 else (nv, a, c)
    keep = np.setdiff1d(np.arange(len(base.faces)), SKIP_FACES)
    mk = lambda faces: Mesh(verts, np.ascontiguousarray(faces, dtype=np.int32), normals, colors)   # noqa: E731
    return mk(deg), mk(oob), mk(base.faces[keep]), keep


def skip_scene():
    deg, oob, clean, keep = skipped_face_meshes()
    K = intrinsics2(150, 190, 20.9, 27.3)
    return Scene('skipped faces 50x37', deg, EDGE_POSE, K, 50, 37, min_cover=0.2), oob, clean, keep


CLIP_FACES = 50


def clip_scenes():
    """(the soup's first CLIP_FACES faces as a scene, the whole soup, a cube of fewer faces than the clip as a
    scene): a store of the whole soup and the cube whose max_faces is lowered to CLIP_FACES renders the first as
    the restatement of the soup's first CLIP_FACES faces and leaves the second alone.  The clipped mesh keeps every
    vertex, so zmin, and with it the light, is the whole soup's."""
    from scflow_amd.mesh import Mesh
    full = soup(120, 9)
    first = Mesh(full.verts, np.ascontiguousarray(full.faces[:CLIP_FACES]), full.normals, full.colors)
    pose, K = look_at_pose(-0.7, 1.1, 2.5, 450.0, -20.0, 15.0), intrinsics2(70, 95, 17.9, 26.2)
    return (Scene('clip soup[:50] 50x37', first, pose, K, 50, 37, min_cover=0.2), full,
            Scene('clip cube 50x37', cube(120.0), EDGE_POSE, K, 50, 37, min_cover=0.1))


# ------------------------------------------------------------------------------------------- tie scenes
TIE_SIZE, TIE_LINE, TIE_Z, TIE_F = 64, 20, 500.0, 125.0


def tie_coord(i):
    """sampling point i of a 64-pixel axis, (126 i + 63) / 128: exact in fp32."""
    return (126 * i + 63) / 128


def shared_edge_scene(axis, first):
    """two fronto-parallel quads at z = 500 (R = I, t = (0, 0, 500)) sharing the edge X = 0 (axis 0; Y = 0 for axis
    1), projected onto column (row) TIE_LINE of a 64 x 64 image.  `first` = 0 lists the quad on the negative side
    first, 1 the other.  Faces are listed as [inner triangle, edge-owning triangle] per quad, so the faces that own
    the shared edge are 1 and 3 and the expected winner on the line is face 1, of the quad listed first.

    Every number is a small dyadic rational: f / z = 1/4, the corners sit at multiples of 4 mm, the principal point
    and the sampling points are multiples of 1/128 px.  The fp32 records are therefore exact, the edge functions on
    the shared edge are exactly 0 for both owners, and both owners' depths 1 / ((w0 a + w1 a + w2 a) / s), a =
    fl32(1/500), are the same bits: each product has at most 26 + 24 bits, their sum is (w0 + w1 + w2) a, which is
    representable, and the quotient by s is a.  The tie is exact and the face index alone decides it.
    -> (mesh, K, pixels (rows, cols) of the line inside the quads, winner face, the first quad alone as a mesh)."""
    line = tie_coord(TIE_LINE)
    other = 31.3125
    K = intrinsics2(TIE_F, TIE_F, line, other) if axis == 0 else intrinsics2(TIE_F, TIE_F, other, line)
    ext, half = 64.0, 40.0                       # the quads reach 16 px from the edge and +-10 px along it

    def quad(sign, color):
        # corners: e0, e1 on the shared edge, o0, o1 away from it
        e0, e1, o0, o1 = [0, -half], [0, half], [sign * ext, -half], [sign * ext, half]
        c = np.array([o0, e0, e1, o1], np.float64)
        if axis == 1:
            c = c[:, ::-1]
        v = np.concatenate([c, np.zeros((4, 1))], 1)
        return v, np.array([(0, 2, 3), (0, 1, 2)]), np.tile(np.asarray(color, np.float64), (4, 1))   # inner, owner
    quads = [quad(-1, (0.9, 0.2, 0.1)), quad(+1, (0.1, 0.3, 0.8))]
    if first == 1:
        quads = quads[::-1]
    verts = np.concatenate([q[0] for q in quads])
    faces = np.concatenate([quads[0][1], quads[1][1] + 4])
    colors = np.concatenate([q[2] for q in quads])
    nrm = np.tile(np.float32([0, 0, -1]), (8, 1))
    mesh = make_mesh(verts, faces, normals=nrm, colors=colors)
    alone = make_mesh(verts[:4], faces[:2], normals=nrm[:4], colors=colors[:4])
    idx = np.arange(TIE_SIZE)
    c = pixel_coord(idx, TIE_SIZE, TIE_SIZE)
    inside = idx[(c > other - half * TIE_F / TIE_Z) & (c < other + half * TIE_F / TIE_Z)]
    fixed = np.full_like(inside, TIE_LINE)
    pixels = (inside, fixed) if axis == 0 else (fixed, inside)
    return mesh, K, pixels, 1, alone


TIE_POSE = (np.eye(3, dtype=np.float32), np.array([0, 0, TIE_Z], np.float32))


def duplicate_face_scene(first):
    """two faces on identical vertex positions (duplicated vertices, different colours), `first` choosing which
    colour face 0 carries: identical fp32 records, identical depth bits, so every covered pixel is face 0.
    -> (mesh, the mesh of face 0 alone, pose, K, H, W)."""
    tri = np.array([[-70, -50, 10], [80, -30, -25], [-10, 75, 30]], np.float64)
    cols = [np.array([[.9, .1, .1], [.8, .3, .1], [.7, .1, .3]]), np.array([[.1, .2, .9], [.1, .4, .8], [.3, .1, .7]])]
    if first == 1:
        cols = cols[::-1]
    nrm = np.tile(_unit(np.cross(tri[1] - tri[0], tri[2] - tri[0])), (6, 1))
    mesh = make_mesh(np.concatenate([tri, tri]), [(0, 1, 2), (3, 4, 5)], normals=nrm, colors=np.concatenate(cols))
    alone = make_mesh(tri, [(0, 1, 2)], normals=nrm[:3], colors=cols[0])
    return mesh, alone, EDGE_POSE, intrinsics2(110, 150, 19.7, 26.4), 50, 37


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


# ------------------------------------------------------------------------- the edge scenes, restatement only
def _existing_gpu_scenes():
    """every compared scene of test_gpu_render.py, restated here so that its ambiguous share is measured
    without a GPU: (name, mesh, pose, K, H, W)."""
    import math
    poses = [look_at_pose(0.3, -0.4, 0.2, 600.0, 10.0, -5.0), look_at_pose(-0.7, 1.1, 2.5, 450.0, -20.0, 15.0),
             look_at_pose(2.0, 0.1, -0.9, 800.0, 0.0, 0.0)]
    out = []
    meshes = {0: cube(120.0), 1: colored_icosphere(3, 70.0)}
    for i in range(6):
        out.append((f'cube/icosphere {i}', meshes[i % 2], poses[i // 2], intrinsics(300.0, 128, 128), 128, 128))
    for i in range(2):
        out.append((f'soup {i}', soup(300, 3), poses[i], intrinsics(120.0, 64, 64), 64, 64))
    out.append(('64x96', colored_icosphere(3, 80.0), look_at_pose(0.2, 0.5, 0.1, 500.0, 40.0, -10.0),
                intrinsics(150.0, 64, 96), 64, 96))
    meshes = {0: cube(100.0), 1: colored_icosphere(2, 60.0), 3: soup(60, 5)}
    labels = [3, 0, 1, 1, 0, 3, 0, 1]
    g = np.random.default_rng(8)
    ps = [look_at_pose(*g.uniform(-math.pi, math.pi, 3), g.uniform(350, 700), *g.uniform(-30, 30, 2)) for _ in labels]
    Ks = [intrinsics(g.uniform(90, 140), 64, 64) for _ in labels]
    for i, l in enumerate(labels):
        out.append((f'mixed {i}', meshes[l], ps[i], Ks[i], 64, 64))
    out.append(('behind', soup(200, 11), look_at_pose(0.1, 0.2, 0.0, 40.0), intrinsics(60.0, 64, 64), 64, 64))
    return out


def test_existing_gpu_scenes_stay_under_the_ambiguous_cap():
    """_check of test_gpu_render.py asserts the cap on the GPU machine; this is the same condition from the
    restatement alone."""
    for name, mesh, pose, K, H, W in _existing_gpu_scenes():
        ref = render_reference(mesh, pose[0], pose[1], K, H, W)
        print(f'[measured] {name}: ambiguous {check_ambiguous_cap(ref, name):.3%}, covered {(ref["face"] >= 0).mean():.1%}')


@pytest.mark.parametrize('which', ['RAGGED', 'ANISOTROPIC', 'SUBPIXEL', 'CLOSE', 'FULL_CHUNK', 'LIGHT_BATCH'])
def test_edge_scenes_stay_under_the_ambiguous_cap(which):
    """every scene of the new lists through render_reference only: at most 1 % of its pixels are ambiguous, and it
    covers what its list is there for."""
    for s in SCENE_LISTS[which]():
        ref = s.reference()
        share, cover = check_ambiguous_cap(ref, s.name), (ref['face'] >= 0).mean()
        print(f'[measured] {s.name}: ambiguous {share:.3%}, covered {cover:.1%}')
        assert cover >= s.min_cover, f'{s.name}: {cover:.1%} covered'
        assert ref['zbuf'].shape == (s.H, s.W)


def test_edge_scene_lists_reach_their_branches():
    assert {(s.H, s.W) for s in ragged_scenes()} == set(RAGGED_SIZES)
    assert any(s.H > s.W and s.H % 16 and s.W % 16 for s in ragged_scenes())
    assert any(s.W > s.H and s.H % 16 and s.W % 16 for s in ragged_scenes())
    assert sum(min(s.H, s.W) == 1 for s in ragged_scenes()) == 3
    # (1, 5): one sampling point for the five columns, and the restatement renders them alike
    assert (pixel_coord(np.arange(5), 5, 1) == 2.0).all()
    ref = next(s for s in ragged_scenes() if (s.H, s.W) == (1, 5)).reference()
    assert (ref['face'] == ref['face'][0, 0]).all() and ref['face'][0, 0] >= 0 and (ref['zbuf'] == ref['zbuf'][0, 0]).all()
    for s in anisotropic_scenes():
        fx, fy = float(s.K[0, 0]), float(s.K[1, 1])
        assert max(fx / fy, fy / fx) >= 1.3
        assert abs(s.K[0, 2] - (s.W - 1) / 2) >= 1.5 and abs(s.K[1, 2] - (s.H - 1) / 2) >= 1.5
    assert any(s.H > s.W for s in anisotropic_scenes()) and any(s.W > s.H for s in anisotropic_scenes())
    # sub-pixel: far more faces than covered pixels
    s = subpixel_scenes()[0]
    assert len(s.mesh.faces) / max((s.reference()['face'] >= 0).sum(), 1) > 50
    # full chunk: one winner, in the second chunk of 256 for the reversed list and face 0 for the other
    a, b = full_chunk_scenes()
    assert len(a.mesh.faces) >= 300 and (a.reference()['face'] == 299).all() and (b.reference()['face'] == 0).all()
    # the light batch: zmin - 400 on both sides of 0, the batch minimum from the first sample
    z = [s.zmin() for s in light_batch_scenes()]
    assert z[0] < 400 < z[1] < z[2] and np.floor(z[0] / 100) != np.floor(z[1] / 100)
    # the soup has faces wholly and partly behind the camera
    s = close_scenes()[1]
    zf = (s.mesh.verts.astype(np.float64) @ s.pose[0].T.astype(np.float64) + s.pose[1])[:, 2].reshape(-1, 3)
    assert (zf <= 0).all(1).any() and ((zf <= 0).any(1) & (zf > 0).any(1)).any()


def test_skipped_face_meshes_restate_as_the_mesh_without_them():
    s, oob, clean, keep = skip_scene()
    ref = s.reference()
    check_ambiguous_cap(ref, s.name)
    assert (ref['face'] >= 0).mean() >= s.min_cover and not np.isin(ref['face'], SKIP_FACES).any()
    nv = len(oob.verts)
    bad = ((oob.faces < 0) | (oob.faces >= nv)).any(1)
    assert sorted(np.nonzero(bad)[0]) == sorted(SKIP_FACES) and oob.faces.min() == -1 and oob.faces.max() == nv
    np.testing.assert_array_equal(np.delete(oob.faces, SKIP_FACES, 0), np.delete(s.mesh.faces, SKIP_FACES, 0))
    want = render_reference(clean, s.pose[0], s.pose[1], s.K, s.H, s.W)
    ok = ~ref['ambiguous']
    np.testing.assert_array_equal(ref['face'][ok], np.where(want['face'] >= 0, keep[want['face']], -1)[ok])
    np.testing.assert_array_equal(ref['zbuf'][ok], want['zbuf'][ok])
    np.testing.assert_array_equal(ref['rgb'][ok], want['rgb'][ok])
    # some skipped face would have been seen: without its neighbours' cover the test would prove nothing
    vis = render_reference(colored_icosphere(2, 60.0), s.pose[0], s.pose[1], s.K, s.H, s.W)['face']
    assert np.isin(vis, SKIP_FACES).any()


def test_clip_scenes_differ_from_the_whole_mesh():
    first, full, cb = clip_scenes()
    ref = first.reference()
    check_ambiguous_cap(ref, first.name)
    check_ambiguous_cap(cb.reference(), cb.name)
    assert (ref['face'] >= 0).mean() >= first.min_cover and len(cb.mesh.faces) < CLIP_FACES < len(full.faces)
    whole = render_reference(full, *first.pose, first.K, first.H, first.W)
    assert (whole['face'] >= CLIP_FACES).mean() > 0.1       # a renderer that ignores the clip shows other faces
    assert first.zmin() == sample_zmin(full, *first.pose)


@pytest.mark.parametrize('axis', [0, 1])
@pytest.mark.parametrize('first', [0, 1])
def test_shared_edge_scene_is_exact_and_ambiguous_in_the_restatement(axis, first):
    mesh, K, (rows, cols), winner, alone = shared_edge_scene(axis, first)
    assert len(rows) == 20 and winner == 1
    assert np.float32(tie_coord(TIE_LINE)) == tie_coord(TIE_LINE) == pixel_coord(TIE_LINE, TIE_SIZE, TIE_SIZE)
    ref = render_reference(mesh, *TIE_POSE, K, TIE_SIZE, TIE_SIZE)
    assert ref['ambiguous'][rows, cols].all() and (ref['face'][rows, cols] >= 0).all()
    check_ambiguous_cap(ref, 'shared edge')                 # the line is 20 of 4096 pixels: the rest is compared
    np.testing.assert_array_equal(ref['zbuf'][rows, cols], TIE_Z)
    one = render_reference(alone, *TIE_POSE, K, TIE_SIZE, TIE_SIZE)
    assert (one['face'][rows, cols] == 1).all()             # the quad alone: its edge-owning triangle covers the line
    side = one['face'] >= 0
    assert 250 < side.sum() < 400 and side[rows, cols].all()
    # the two orders put different colours on the line
    other = render_reference(shared_edge_scene(axis, 1 - first)[4], *TIE_POSE, K, TIE_SIZE, TIE_SIZE)
    assert np.abs(one['rgb'][rows, cols] - other['rgb'][rows, cols]).max() > 0.1


@pytest.mark.parametrize('first', [0, 1])
def test_duplicate_face_scene(first):
    mesh, alone, pose, K, H, W = duplicate_face_scene(first)
    np.testing.assert_array_equal(mesh.verts[:3], mesh.verts[3:])
    assert np.abs(mesh.colors[:3] - mesh.colors[3:]).max(1).min() > 0.3
    ref = render_reference(alone, *pose, K, H, W)
    check_ambiguous_cap(ref, 'duplicate face')
    assert (ref['face'] >= 0).mean() > 0.1
    both = render_reference(mesh, *pose, K, H, W)
    assert (both['ambiguous'] == ((both['face'] >= 0) | ref['ambiguous'])).all()     # every covered pixel is a depth tie
