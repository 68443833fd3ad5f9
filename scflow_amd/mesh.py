"""Meshes and the mesh renderer: ``read_ply``, ``MeshStore`` and ``MeshRenderer``.

``MeshRenderer`` takes the constructor of the reference ``Renderer`` (models/utils/rendering.py) and renders
with ``scf_render_mesh`` (scflow_amd/csrc/render.hip states the semantics).  It implements the configuration the
reference ships (configs/refine_datasets/ycbv_real.py:148-164): hard rasterisation with one face per pixel and
Phong shading.  Soft blending, silhouette masks, other shaders, ``faces_per_pixel != 1`` and ``blur_radius != 0``
raise ``NotImplementedError`` at construction.  pytorch3d bit parity is not claimed.

Vertex normals come from the PLY's ``nx ny nz`` when the file has them (whether pytorch3d's PLY reader passes
file normals through is unverified); otherwise they are the normalised area-weighted sum of the face normals
(``Meshes.verts_normals``).  A mesh without vertex colours renders white.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from glob import glob
from typing import Dict, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import ops

Tensor = torch.Tensor

_PLY_TYPES = {'char': 'i1', 'int8': 'i1', 'uchar': 'u1', 'uint8': 'u1', 'short': 'i2', 'int16': 'i2',
              'ushort': 'u2', 'uint16': 'u2', 'int': 'i4', 'int32': 'i4', 'uint': 'u4', 'uint32': 'u4',
              'float': 'f4', 'float32': 'f4', 'double': 'f8', 'float64': 'f8'}


@dataclass
class Mesh:
    """one triangle mesh on the host: verts (V,3) float32, faces (F,3) int32, normals (V,3) float32 (unit length),
    colors (V,3) float32 in [0, 1]."""
    verts: np.ndarray
    faces: np.ndarray
    normals: np.ndarray
    colors: np.ndarray


def vertex_normals(verts: np.ndarray, faces: np.ndarray) -> np.ndarray:
    """normalised area-weighted sum of the face normals around each vertex (``Meshes.verts_normals``)."""
    v = verts.astype(np.float64)
    f = faces.astype(np.int64)
    fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])     # |fn| = twice the face's area
    acc = np.zeros_like(v)
    for k in range(3):
        np.add.at(acc, f[:, k], fn)
    norm = np.maximum(np.linalg.norm(acc, axis=1, keepdims=True), 1e-6)
    return (acc / norm).astype(np.float32)


def make_mesh(verts, faces, normals=None, colors=None) -> Mesh:
    """a ``Mesh`` from arrays; normals default to ``vertex_normals``, colours to white."""
    verts = np.ascontiguousarray(np.asarray(verts, dtype=np.float32).reshape(-1, 3))
    faces = np.ascontiguousarray(np.asarray(faces, dtype=np.int64).reshape(-1, 3))
    if faces.size and (faces.min() < 0 or faces.max() >= len(verts)):
        raise ValueError(f'face index out of range [0, {len(verts)})')
    faces = faces.astype(np.int32)
    if normals is None:
        normals = vertex_normals(verts, faces)
    normals = np.ascontiguousarray(np.asarray(normals, dtype=np.float32).reshape(-1, 3))
    if colors is None:
        colors = np.ones_like(verts)
    colors = np.ascontiguousarray(np.asarray(colors, dtype=np.float32).reshape(-1, 3))
    if len(normals) != len(verts) or len(colors) != len(verts):
        raise ValueError('normals and colors need one row per vertex')
    return Mesh(verts, faces, normals, colors)


def icosphere(subdivisions: int = 2, radius: float = 1.0) -> Tuple[np.ndarray, np.ndarray]:
    """a subdivided icosahedron on a sphere: (verts (V,3) float32, faces (F,3) int32), outward winding,
    F = 20 * 4^subdivisions (1: 80, 3: 1280, 5: 20480, 7: 327680)."""
    p = (1 + 5 ** 0.5) / 2
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p),
         (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10),
         (8, 6, 7), (9, 8, 1)]
    verts = np.array(v, dtype=np.float64)
    verts /= np.linalg.norm(verts, axis=1, keepdims=True)
    faces = np.array(f, dtype=np.int64)
    for _ in range(subdivisions):
        edges = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]), axis=1)
        uniq, inv = np.unique(edges, axis=0, return_inverse=True)
        mid = verts[uniq[:, 0]] + verts[uniq[:, 1]]
        mid /= np.linalg.norm(mid, axis=1, keepdims=True)
        m = inv.reshape(-1) + len(verts)
        nf = len(faces)
        a, b, c = faces[:, 0], faces[:, 1], faces[:, 2]
        ab, bc, ca = m[:nf], m[nf:2 * nf], m[2 * nf:]
        faces = np.concatenate([np.stack([a, ab, ca], 1), np.stack([b, bc, ab], 1), np.stack([c, ca, bc], 1),
                                np.stack([ab, bc, ca], 1)])
        verts = np.concatenate([verts, mid])
    return (verts * radius).astype(np.float32), faces.astype(np.int32)


def _parse_header(data: bytes):
    end = data.find(b'end_header')
    if not data.startswith(b'ply') or end < 0:
        raise ValueError('not a PLY file')
    body = data.index(b'\n', end) + 1
    lines = data[:end].decode('ascii', 'replace').splitlines()
    fmt, elements = None, []
    for line in lines[1:]:
        tok = line.split()
        if not tok or tok[0] in ('comment', 'obj_info'):
            continue
        if tok[0] == 'format':
            fmt = tok[1]
        elif tok[0] == 'element':
            elements.append((tok[1], int(tok[2]), []))
        elif tok[0] == 'property':
            if not elements:
                raise ValueError('PLY property before any element')
            if tok[1] == 'list':
                if tok[2] not in _PLY_TYPES or tok[3] not in _PLY_TYPES:
                    raise ValueError(f'unknown PLY type in {line!r}')
                elements[-1][2].append((tok[4], 'list', _PLY_TYPES[tok[2]], _PLY_TYPES[tok[3]]))
            else:
                if tok[1] not in _PLY_TYPES:
                    raise ValueError(f'unknown PLY type {tok[1]!r}')
                elements[-1][2].append((tok[2], 'scalar', _PLY_TYPES[tok[1]], None))
    if fmt not in ('ascii', 'binary_little_endian'):
        raise ValueError(f"PLY format {fmt!r} is not supported (ascii and binary_little_endian are)")
    return fmt, elements, body


def _vertex_arrays(cols: Dict[str, np.ndarray], types: Dict[str, str]):
    verts = np.stack([cols['x'], cols['y'], cols['z']], axis=1)
    normals = np.stack([cols['nx'], cols['ny'], cols['nz']], axis=1) if all(k in cols for k in ('nx', 'ny', 'nz')) else None
    colors = None
    if all(k in cols for k in ('red', 'green', 'blue')):
        colors = np.stack([cols['red'], cols['green'], cols['blue']], axis=1).astype(np.float32)
        if types['red'] == 'u1':
            colors = colors / 255.0
    return verts, normals, colors


def _face_prop(props):
    lists = [p for p in props if p[1] == 'list']
    if len(lists) != 1 or lists[0][0] not in ('vertex_indices', 'vertex_index'):
        raise ValueError('PLY face element needs one list property vertex_indices (or vertex_index)')
    return lists[0]


def read_ply(path: str) -> Mesh:
    """read an ascii or binary_little_endian PLY: vertex x y z, optional nx ny nz and red green blue [alpha]
    (uchar / 255, or float as is), faces as a list of vertex indices.  Anything but triangles raises."""
    with open(path, 'rb') as fh:
        data = fh.read()
    fmt, elements, pos = _parse_header(data)
    names = [e[0] for e in elements]
    if 'vertex' not in names or 'face' not in names:
        raise ValueError(f'{path}: PLY needs vertex and face elements')
    cols: Dict[str, np.ndarray] = {}
    types: Dict[str, str] = {}
    faces = None
    if fmt == 'ascii':
        rows = data[pos:].decode('ascii').split('\n')
        r = 0
        for name, count, props in elements:
            if name == 'vertex':
                if any(p[1] == 'list' for p in props):
                    raise ValueError('list property on PLY vertices')
                table = np.array([rows[r + i].split()[:len(props)] for i in range(count)], dtype=np.float64).reshape(count, len(props))
                for j, p in enumerate(props):
                    cols[p[0]], types[p[0]] = table[:, j], p[2]
            elif name == 'face':
                _face_prop(props)
                out = np.empty((count, 3), dtype=np.int64)
                for i in range(count):
                    tok = rows[r + i].split()
                    off = 0
                    for p in props:             # scalars before the list are skipped
                        if p[1] == 'list':
                            break
                        off += 1
                    if int(tok[off]) != 3:
                        raise ValueError(f'{path}: face {i} has {tok[off]} vertices (triangles only)')
                    out[i] = [int(v) for v in tok[off + 1:off + 4]]
                faces = out
            r += count
    else:
        for name, count, props in elements:
            if faces is not None and 'x' in cols:
                break                            # vertex and face read: later elements are not needed
            if all(p[1] == 'scalar' for p in props):
                dt = np.dtype([(p[0], '<' + p[2]) for p in props])
                table = np.frombuffer(data, dtype=dt, count=count, offset=pos)
                pos += dt.itemsize * count
                if name == 'vertex':
                    for p in props:
                        cols[p[0]], types[p[0]] = table[p[0]].astype(np.float64), p[2]
            elif name == 'face':
                _face_prop(props)
                fields = []
                for p in props:                  # every face assumed a triangle; the first that is not raises
                    if p[1] == 'list':
                        fields += [('n', '<' + p[2]), ('i', '<' + p[3], (3,))]
                    else:
                        fields.append((p[0], '<' + p[2]))
                dt = np.dtype(fields)
                if pos + dt.itemsize * count > len(data):
                    raise ValueError(f'{path}: face data too short (triangles only)')
                table = np.frombuffer(data, dtype=dt, count=count, offset=pos)
                bad = np.nonzero(table['n'] != 3)[0]
                if len(bad):
                    raise ValueError(f'{path}: face {bad[0]} has {table["n"][bad[0]]} vertices (triangles only)')
                faces = table['i'].astype(np.int64)
                pos += dt.itemsize * count
            else:
                raise ValueError(f'{path}: element {name!r} with a list property before the faces')
    verts, normals, colors = _vertex_arrays(cols, types)
    return make_mesh(verts, faces, normals, colors)


def label_from_path(path: str) -> int:
    """rendering.py:121-129: ``obj_000001.ply`` -> 0 (the number after the last '_' of the stem, minus one)."""
    return int(os.path.basename(path).split('.')[0].split('_')[-1]) - 1


@dataclass
class DeviceMesh:
    """a ``MeshStore`` on one device: the tensors behind ``scf_mesh_store``."""
    verts: Tensor
    normals: Tensor
    colors: Tensor
    faces: Tensor
    vert_offset: Tensor
    face_offset: Tensor
    num_classes: int
    max_faces: int


class MeshStore:
    """every class mesh concatenated (class k = label k; missing labels are empty meshes and render background),
    uploaded once per device."""

    def __init__(self, meshes: Dict[int, Mesh]):
        if not meshes:
            raise ValueError('MeshStore needs at least one mesh')
        if min(meshes) < 0:
            raise ValueError(f'negative class label {min(meshes)}')
        self.meshes = dict(sorted(meshes.items()))
        self.num_classes = max(self.meshes) + 1
        vo, fo = [0], [0]
        for k in range(self.num_classes):
            m = self.meshes.get(k)
            vo.append(vo[-1] + (len(m.verts) if m else 0))
            fo.append(fo[-1] + (len(m.faces) if m else 0))
        self.vert_offset = np.array(vo, dtype=np.int64)
        self.face_offset = np.array(fo, dtype=np.int64)
        if vo[-1] >= 2 ** 31 or fo[-1] >= 2 ** 31:
            raise ValueError('mesh store too large (2^31 vertices or faces)')
        self.max_faces = max(1, max(len(m.faces) for m in self.meshes.values()))
        self._dev: Dict[torch.device, DeviceMesh] = {}

    @classmethod
    def from_paths(cls, mesh_dir: str, ext: str = '.ply') -> 'MeshStore':
        """rendering.py:121-129: every ``*.ply`` of a directory (or one file), labels from the file names."""
        paths = sorted(glob(os.path.join(mesh_dir, '*' + ext))) if os.path.isdir(mesh_dir) else [mesh_dir]
        if not paths:
            raise FileNotFoundError(f'no {ext} meshes under {mesh_dir}')
        return cls({label_from_path(p): read_ply(p) for p in paths})

    def on(self, device) -> DeviceMesh:
        device = torch.device(device)
        if device not in self._dev:
            def cat(attr, dtype):
                arrs = [getattr(m, attr) for m in self.meshes.values()]
                return torch.from_numpy(np.concatenate(arrs).astype(dtype)).contiguous().to(device)
            self._dev[device] = DeviceMesh(
                cat('verts', np.float32), cat('normals', np.float32), cat('colors', np.float32), cat('faces', np.int32),
                torch.from_numpy(self.vert_offset.astype(np.int32)).to(device),
                torch.from_numpy(self.face_offset.astype(np.int32)).to(device), self.num_classes, self.max_faces)
        return self._dev[device]


@dataclass
class Fragments:
    """the part of pytorch3d's ``Fragments`` the refiners read.  ``pix_to_face`` is the face index within the
    sample's own mesh (pytorch3d's is an index into the packed batch)."""
    zbuf: Tensor
    pix_to_face: Tensor


class MeshRenderer:
    """``Renderer`` (models/utils/rendering.py) on ``scf_render_mesh``.  ``mesh_dir`` may also be a ``MeshStore``."""

    def __init__(self, mesh_dir: Union[str, MeshStore], image_size: Sequence[int], shader_type: str = 'Phong',
                 soft_blending: bool = True, render_mask: bool = True, render_image: bool = True,
                 faces_per_pixel: int = 1, blur_radius: float = 0., sigma: float = 1e-4, gamma: float = 1e-4,
                 bin_size=None, default_lights: bool = True, seperate_lights: bool = False,
                 background_color: Sequence[float] = (0.5, 0.5, 0.5)):
        unsupported = [(shader_type != 'Phong', f'shader_type={shader_type!r} (only Phong)'),
                       (bool(soft_blending), 'soft_blending=True (hard blending only)'),
                       (bool(render_mask), 'render_mask=True (no silhouette pass)'),
                       (not render_image, 'render_image=False'),
                       (faces_per_pixel != 1, f'faces_per_pixel={faces_per_pixel} (1 only)'),
                       (blur_radius != 0, f'blur_radius={blur_radius} (0 only)')]
        for bad, what in unsupported:
            if bad:
                raise NotImplementedError(f'MeshRenderer: {what}')
        h, w = (int(image_size), int(image_size)) if isinstance(image_size, int) else (int(image_size[0]), int(image_size[1]))
        self.image_size = (h, w)
        self.default_lights = bool(default_lights)
        self.seperate_lights = bool(seperate_lights)
        self.background_color = tuple(float(c) for c in background_color)
        self.shader_type, self.faces_per_pixel, self.blur_radius = shader_type, faces_per_pixel, blur_radius
        self.store = mesh_dir if isinstance(mesh_dir, MeshStore) else MeshStore.from_paths(mesh_dir)

    def to(self, device) -> 'MeshRenderer':
        self.store.on(device)
        return self

    def _render(self, rotations, translations, internel_k, labels, **kw):
        if not (rotations.size(0) == translations.size(0) == internel_k.size(0) == labels.size(0)):
            raise ValueError('rotations, translations, internel_k and labels need the same batch size')
        return ops.render_mesh(self.store.on(rotations.device), labels, rotations.contiguous(),
                               translations.contiguous(), internel_k.contiguous(),
                               self.image_size, default_lights=self.default_lights,
                               seperate_lights=self.seperate_lights, background=self.background_color, **kw)

    def forward(self, rotations: Tensor, translations: Tensor, internel_k: Tensor, labels: Tensor) -> Dict:
        """-> dict(images (N,H,W,4) with alpha = covered, fragments = Fragments(zbuf (N,H,W,1), pix_to_face
        (N,H,W,1))), as the reference's dict.  No host synchronisation."""
        out = self._render(rotations, translations, internel_k, labels, images=True, pix_to_face=True)
        return dict(images=out['images'],
                    fragments=Fragments(out['zbuf'][..., None], out['pix_to_face'][..., None]))

    __call__ = forward

    def render_normalized(self, rotations: Tensor, translations: Tensor, internel_k: Tensor, labels: Tensor,
                          mean: Optional[Sequence[float]] = None, std: Optional[Sequence[float]] = None
                          ) -> Tuple[Tensor, Tensor, Tensor]:
        """what the refiners consume: (rgb (N,3,H,W) = (rgb - mean) / std, depth (N,H,W), mask (N,H,W) float32 =
        depth > 0), written by the kernel in NCHW (no permute).  mean / std in [0, 1] units; None = identity."""
        norm = (mean if mean is not None else (0., 0., 0.), std if std is not None else (1., 1., 1.))
        out = self._render(rotations, translations, internel_k, labels, images=False, pix_to_face=False, norm=norm)
        depth = out['zbuf']
        return out['rgb'], depth, (depth > 0).to(torch.float32)
