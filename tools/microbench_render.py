"""Micro-benchmark of the mesh renderer (``scf_render_mesh``: setup + tile rasteriser + shading, CUDA-event timed,
one call = the whole launch sequence) at 256 x 256, batch 1 / 8 / 32, on procedural icospheres of 1 280, 20 480 and
327 680 faces (subdivisions 3, 5, 7), radius 90 mm at 400-600 mm, the shipped light setting (seperate_lights).
    python tools/microbench_render.py [N ...]      -> one JSON line per (batch, mesh) (median / min microseconds)"""
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from scflow_amd import ops  # noqa: E402
from scflow_amd.mesh import MeshStore, icosphere, make_mesh  # noqa: E402

dev = 'cuda:0'
H = W = 256


def timeit(fn, n=10):
    for _ in range(2):
        fn()
    evs = []
    for _ in range(n):
        s = torch.cuda.Event(enable_timing=True); e = torch.cuda.Event(enable_timing=True)
        s.record(); fn(); e.record(); evs.append((s, e))
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) for a, b in evs)
    return ts[len(ts) // 2] * 1e3, ts[0] * 1e3


def poses(n, seed):
    g = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        a, b, c = g.uniform(-math.pi, math.pi, 3)
        ca, sa, cb, sb, cc, sc = math.cos(a), math.sin(a), math.cos(b), math.sin(b), math.cos(c), math.sin(c)
        R = (np.array([[cc, -sc, 0], [sc, cc, 0], [0, 0, 1]]) @ np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
             @ np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]]))
        out.append((R, np.array([*g.uniform(-20, 20, 2), g.uniform(400, 600)])))
    return out


stores = {sd: MeshStore({0: make_mesh(*icosphere(sd, 90.0))}) for sd in (3, 5, 7)}
for n in [int(a) for a in sys.argv[1:]] or [1, 8, 32]:
    ps = poses(n, n)
    R = torch.tensor(np.stack([p[0] for p in ps]), dtype=torch.float32, device=dev)
    t = torch.tensor(np.stack([p[1] for p in ps]), dtype=torch.float32, device=dev)
    K = torch.tensor([[300., 0, 127.5], [0, 300., 127.5], [0, 0, 1]], device=dev).expand(n, 3, 3).contiguous()
    lab = torch.zeros((n,), dtype=torch.int32, device=dev)
    for sd, store in stores.items():
        mesh = store.on(dev)
        norm = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
        fn = lambda: ops.render_mesh(mesh, lab, R, t, K, (H, W), images=False, pix_to_face=False, norm=norm)  # noqa: E731
        us = timeit(fn)
        cov = float((fn()['zbuf'] > 0).float().mean())
        print(json.dumps(dict(batch=n, faces=int(store.max_faces), size=[H, W], render_us=dict(
            median=round(us[0], 1), min=round(us[1], 1)), covered=round(cov, 3))))
