"""Micro-benchmark of the patch pipeline (``scf_patch_boxes`` + ``scf_patch_extract``, CUDA-event timed): 32 objects
(icospheres of 10 242 vertices, radius 60 mm at 350-900 mm, some hanging over the border) from four 480 x 640 frames
into 256 x 256 patches, the shipped val_pipeline settings.  The same steps as a plain-torch composition on the GPU
(batched projection, min / max, the crop rule, one ``grid_sample`` over the gathered frames, normalisation) are timed
beside it.  It interpolates in floating point and blends across the frame's border and the crop's edge where the
kernels clamp, so its pixels differ from theirs: by under a grey level on average, by more along those edges.
    python tools/microbench_patches.py [N]      -> one JSON line: microseconds (median / min) per path and per launch,
    the algorithmic bytes (the fp32 output plus the source rectangles' uint8 pixels inside the frame) and their rate
    over the patch launch as a fraction of the 8 TB/s HBM peak"""
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from scflow_amd import ops  # noqa: E402
from scflow_amd.mesh import MeshStore, icosphere, make_mesh  # noqa: E402

dev = 'cuda:0'
HF, WF, H, W, S = 480, 640, 256, 256, 256
HBM_PEAK = 8.0e12


def timeit(fn, n=50):
    for _ in range(5):
        fn()
    evs = []
    for _ in range(n):
        s = torch.cuda.Event(enable_timing=True); e = torch.cuda.Event(enable_timing=True)
        s.record(); fn(); e.record(); evs.append((s, e))
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) for a, b in evs)
    return dict(median=round(ts[len(ts) // 2] * 1e3, 1), min=round(ts[0] * 1e3, 1))


def poses(n, seed):
    g = np.random.default_rng(seed)
    Rs, ts = [], []
    for _ in range(n):
        a, b, c = g.uniform(-math.pi, math.pi, 3)
        ca, sa, cb, sb, cc, sc = math.cos(a), math.sin(a), math.cos(b), math.sin(b), math.cos(c), math.sin(c)
        Rs.append(np.array([[cc, -sc, 0], [sc, cc, 0], [0, 0, 1]]) @ np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
                  @ np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]]))
        z = g.uniform(350, 900)
        ts.append(np.array([g.uniform(-0.5, 0.5) * WF * z / 600, g.uniform(-0.5, 0.5) * HF * z / 600, z]))
    return np.stack(Rs), np.stack(ts)


def torch_patches(verts, R, t, K, frames_f, frame_index, ratio=1.1, fill=128.0):
    """the same steps in plain torch, no host synchronisation: -> (N,3,H,W) normalised RGB."""
    n = R.shape[0]
    p = (verts[None] @ R.transpose(1, 2) + t[:, None]) @ K.transpose(1, 2)
    uv = p[..., :2] / (p[..., 2:] + 1e-8)
    lo, hi = uv.amin(1).double(), uv.amax(1).double()
    c, wh = (lo + hi) / 2, (hi - lo)
    side = wh.amax(1, keepdim=True) * ratio
    o1, o2 = torch.trunc(c - side / 2), torch.trunc(c + side / 2)
    pwh = o2 - o1 + 1
    s = S / pwh.amax(1, keepdim=True)
    new = torch.floor(pwh * s + 0.5)
    pad = torch.trunc(torch.tensor([W / 2, H / 2], device=R.device, dtype=torch.float64) - new / 2)
    xs = torch.arange(W, device=R.device, dtype=torch.float64)[None]
    ys = torch.arange(H, device=R.device, dtype=torch.float64)[None]
    dx, dy = xs - pad[:, :1], ys - pad[:, 1:]
    sx = (dx + 0.5) * (pwh[:, :1] / new[:, :1]) - 0.5 + o1[:, :1]
    sy = (dy + 0.5) * (pwh[:, 1:] / new[:, 1:]) - 0.5 + o1[:, 1:]
    inside = ((dx >= 0) & (dx < new[:, :1]))[:, None, :] & ((dy >= 0) & (dy < new[:, 1:]))[:, :, None]
    grid = torch.stack([((2 * sx + 1) / WF - 1)[:, None, :].expand(n, H, W), ((2 * sy + 1) / HF - 1)[:, :, None].expand(n, H, W)], -1)
    src = frames_f[frame_index.long()] - fill                                   # (N,3,Hf,Wf) gather
    out = F.grid_sample(src, grid.float(), mode='bilinear', padding_mode='zeros', align_corners=False) + fill
    out = torch.where(inside[:, None], out, torch.full_like(out, fill))
    return out.flip(1) * (1.0 / 255.0)


n = int(sys.argv[1]) if len(sys.argv) > 1 else 32
store = MeshStore({0: make_mesh(*icosphere(5, 60.0))})
mesh = store.on(dev)
Rn, tn = poses(n, n)
R = torch.tensor(Rn, dtype=torch.float32, device=dev)
t = torch.tensor(tn, dtype=torch.float32, device=dev)
K = torch.tensor([[600., 0, 320.4], [0, 600., 239.8], [0, 0, 1]], device=dev).expand(n, 3, 3).contiguous()
lab = torch.zeros((n,), dtype=torch.int32, device=dev)
nf = 4
frames = torch.randint(0, 256, (nf, HF, WF, 3), dtype=torch.uint8, device=dev, generator=torch.Generator(dev).manual_seed(1))
fidx = (torch.arange(n, device=dev) % nf).to(torch.int32)
params = ops.patch_params((H, W), S)

box = ops.patch_boxes(mesh, lab, R, t, K, (HF, WF), params)
out = torch.empty((n, 3, H, W), device=dev)


def hip():
    b = ops.patch_boxes(mesh, lab, R, t, K, (HF, WF), params)
    return ops.extract_patches(frames, fidx, b['records'], params, out=out)


frames_f = frames.permute(0, 3, 1, 2).float().contiguous()          # the torch path's HWC uint8 -> CHW float, not timed
verts = mesh.verts


def plain():
    return torch_patches(verts, R, t, K, frames_f, fidx)


res = dict(objects=n, frames=[nf, HF, WF], patch=[H, W], vertices=int(verts.shape[0]))
res['hip_us'] = timeit(hip)
res['hip_boxes_us'] = timeit(lambda: ops.patch_boxes(mesh, lab, R, t, K, (HF, WF), params))
res['hip_extract_us'] = timeit(lambda: ops.extract_patches(frames, fidx, box['records'], params, out=out))
res['torch_us'] = timeit(plain)
crop = box['crop'].cpu().numpy().astype(np.int64)
valid = box['valid'].cpu().numpy()
w_in = np.clip(np.minimum(crop[:, 2], WF - 1) - np.maximum(crop[:, 0], 0) + 1, 0, None)
h_in = np.clip(np.minimum(crop[:, 3], HF - 1) - np.maximum(crop[:, 1], 0) + 1, 0, None)
src_bytes = int((w_in * h_in * 3 * valid).sum())
res['bytes'] = dict(output=n * 3 * H * W * 4, source=src_bytes)
res['extract_fraction_of_hbm_peak'] = round((res['bytes']['output'] + src_bytes) / (res['hip_extract_us']['median'] * 1e-6) / HBM_PEAK, 4)
diff = (hip() - plain()).abs() * 255
res['torch_vs_hip_grey_levels'] = dict(max=round(float(diff.max()), 3), mean=round(float(diff.mean()), 4))
res['valid'] = int(valid.sum())
print(json.dumps(res))
