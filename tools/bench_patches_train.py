"""Timing of the train patch stage (``scf_pose_jitter``, ``scf_patch_boxes_train``, ``scf_patch_extract_train``; device
events, 5 warm-up and 50 timed calls, median / min): 32 objects (icospheres of 10 242 vertices, radius 60 mm at 350-900 mm)
from four 480 x 640 frames into 256 x 256 patches with their masks, the shipped train_pipeline settings.  ``extract_patches``
on the SAME records (the head of the train workspace) is timed beside the train extract, and the train extract once more
with every augmentation switched off.
    python tools/bench_patches_train.py [N]      -> one JSON line, microseconds"""
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from scflow_amd import ops  # noqa: E402
from scflow_amd.mesh import MeshStore, icosphere, make_mesh  # noqa: E402
from scflow_amd.patches import TrainPatchPipeline  # noqa: E402

dev = 'cuda:0'
HF, WF, H, W, S = 480, 640, 256, 256, 256


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
        ts.append(np.array([g.uniform(-0.4, 0.4) * WF * z / 600, g.uniform(-0.4, 0.4) * HF * z / 600, z]))
    return np.stack(Rs), np.stack(ts)


n = int(sys.argv[1]) if len(sys.argv) > 1 else 32
store = MeshStore({0: make_mesh(*icosphere(5, 60.0))})
mesh = store.on(dev)
Rn, tn = poses(n, n)
R = torch.tensor(Rn, dtype=torch.float32, device=dev)
t = torch.tensor(tn, dtype=torch.float32, device=dev)
K = torch.tensor([[600., 0, 320.4], [0, 600., 239.8], [0, 0, 1]], device=dev).expand(n, 3, 3).contiguous()
lab = torch.zeros((n,), dtype=torch.int32, device=dev)
diam = torch.tensor([120.0], device=dev)
nf = 4
gen = torch.Generator(dev).manual_seed(1)
frames = torch.randint(0, 256, (nf, HF, WF, 3), dtype=torch.uint8, device=dev, generator=gen)
masks = (torch.rand((n, HF, WF), device=dev, generator=gen) > 0.5).to(torch.uint8)
fidx = (torch.arange(n, device=dev) % nf).to(torch.int32)
counts = [n // nf + (i < n % nf) for i in range(nf)]
order = torch.argsort(fidx.long(), stable=True)               # the pipeline wants the objects in frame order

params = ops.patch_params((H, W), S)
aug = ops.patch_aug_params()
off = ops.patch_aug_params(hsv_p=0.0, noise_p=0.0, smooth_p=0.0)
jit = ops.pose_jitter(mesh, diam, lab, R, t, aug)
box = ops.patch_boxes_train(mesh, lab, jit['rot'], jit['trans'], K, (HF, WF), params, aug)
out = torch.empty((n, 3, H, W), device=dev)
mout = torch.empty((n, H, W), dtype=torch.bool, device=dev)
head = box['records'][:64 * n].clone()
pipe = TrainPatchPipeline(store, [120.0])
Ro, to = R[order].contiguous(), t[order].contiguous()

res = dict(objects=n, frames=[nf, HF, WF], patch=[H, W], vertices=int(mesh.verts.shape[0]))
res['pipeline_us'] = timeit(lambda: pipe(frames, counts, Ro, to, K, lab, masks))
res['jitter_us'] = timeit(lambda: ops.pose_jitter(mesh, diam, lab, R, t, aug))
res['boxes_train_us'] = timeit(lambda: ops.patch_boxes_train(mesh, lab, jit['rot'], jit['trans'], K, (HF, WF), params, aug))
res['extract_train_us'] = timeit(lambda: ops.extract_patches_train(frames, fidx, box['records'], params, aug, masks=masks,
                                                                   out=out, mask_out=mout))
res['extract_train_no_mask_us'] = timeit(lambda: ops.extract_patches_train(frames, fidx, box['records'], params, aug, out=out))
res['extract_train_all_off_us'] = timeit(lambda: ops.extract_patches_train(frames, fidx, box['records'], params, off, out=out))
res['extract_patches_same_records_us'] = timeit(lambda: ops.extract_patches(frames, fidx, head, params, out=out))
draws = box['draws'].cpu().numpy()
crop = box['crop'].cpu().numpy().astype(np.int64)
res['k_counts'] = {str(k): int((draws[:, 5] == k).sum()) for k in (1, 3, 5)}
res['routes'] = {}
for (x1, y1, x2, y2), s, k, v in zip(crop, box['scale'].cpu().numpy().astype(np.float64), draws[:, 5], box['valid'].cpu().numpy()):
    if v:
        ph, pw = y2 - y1 + 1, x2 - x1 + 1
        r = ops.patch_train_route(ph, pw, int(ph * s + 0.5), int(pw * s + 0.5), int(k))
        res['routes'][r] = res['routes'].get(r, 0) + 1
res['jitter_tries'] = dict(max=int(jit['tries'].max()), mean=round(float(jit['tries'].float().mean()), 2), ok=int(jit['ok'].sum()))
res['valid'] = int(box['valid'].sum())
print(json.dumps(res))
