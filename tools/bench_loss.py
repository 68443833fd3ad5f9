"""Micro-benchmark of the loss stage (``scf_seq_pixel_loss`` + ``scf_point_matching_loss``, CUDA-event timed) at batch 32,
256 x 256, 8 iterations.  No YCB-V mesh is available to this repository: the classes are SYNTHETIC -- a symmetric class of
8192 random vertices and a non-symmetric one of the same size; samples alternate between them.
    python tools/bench_loss.py [N] [V]   -> one JSON line
1. the fused pixel pass (two flow sequences + the mask sequence) against the bytes it must move: ground truth and valid
   once, every prediction once, at the 8 TB/s HBM peak;
2. the point-matching launch: pair evaluations (T x symmetric samples x V^2) per second, counted as 8 fp32 operations a
   pair (three differences, three multiply-adds of which the first is a multiply, one compare-select pair counted as two)
   against the 157.3 TFLOP/s fp32 vector peak;
3. the same losses composed from torch operators on the GPU in fp32 (per-iteration loop, per-sample loop with
   ``torch.cdist`` + ``argmin`` for the symmetric classes: the reference's structure) as the baseline;
4. the loss stage as a share of ``get_pose`` on the same batch (seeded weights, synthetic inputs).
The events bracket the Python call: every HIP figure includes the binding's host path (argument checks, pointer arrays,
three allocations) next to the kernels; the roofline fractions are therefore lower limits for the kernels."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import scflow_amd  # noqa: E402
from scflow_amd import losses as L  # noqa: E402

dev = 'cuda:0'
HBM_PEAK, FP32_VECTOR_PEAK = 8.0e12, 157.3e12
OPS_PER_PAIR = 8


def timeit(fn, n=20):
    for _ in range(3):
        fn()
    evs = []
    for _ in range(n):
        s = torch.cuda.Event(enable_timing=True); e = torch.cuda.Event(enable_timing=True)
        s.record(); fn(); e.record(); evs.append((s, e))
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) for a, b in evs)
    return dict(median=round(ts[len(ts) // 2] * 1e3, 1), min=round(ts[0] * 1e3, 1))


n = int(sys.argv[1]) if len(sys.argv) > 1 else 32
V = int(sys.argv[2]) if len(sys.argv) > 2 else 8192
T, H, W = 8, 256, 256
g = torch.Generator(dev).manual_seed(0)
R = lambda *s: torch.randn(s, device=dev, generator=g)
gt = R(n, 2, H, W) * 6
gt[:, :, :64] = 400.
valid = (torch.rand((n, H, W), device=dev, generator=g) > 0.3).float()
flow_a = [gt + R(n, 2, H, W) for _ in range(T)]
flow_b = [gt + R(n, 2, H, W) for _ in range(T)]
masks = [torch.rand((n, H, W), device=dev, generator=g) for _ in range(T)]
W3, EPS, GAM = (.1, .1, 10.), (1e-10, 1e-10, 0.), (.8, .8, .8)


def hip_pixel():
    return L.seq_pixel_loss(gt, valid, flow_a=flow_a, flow_b=flow_b, masks=masks, loss_weight=W3, eps=EPS, gamma=GAM)


def torch_pixel():
    mag = (gt[:, 0] * gt[:, 0] + gt[:, 1] * gt[:, 1]).sqrt()
    v = ((valid >= 0.5) & (mag < 400.)).to(gt)
    occ = (gt[:, 0] + gt[:, 1] < 400.).float()
    tot = [0., 0., 0.]
    for i in range(T):
        wi = 0.8 ** (T - 1 - i)
        for s, seq in enumerate((flow_a, flow_b)):
            tot[s] = tot[s] + wi * (W3[s] * ((v[:, None] * (seq[i] - gt).abs()).sum() / (v.sum() + 1e-10)))
        tot[2] = tot[2] + wi * (torch.mean(torch.abs(masks[i] - occ)) * W3[2])
    return tot


def rot(k):
    q, _ = torch.linalg.qr(R(k, 3, 3))
    return (q * torch.sign(torch.linalg.det(q))[:, None, None]).contiguous()


verts = [R(V, 3) * 40, R(V, 3) * 40]
labels = (torch.arange(n, device=dev) % 2)
gt_r, gt_t = rot(n), (R(n, 3) * 20 + torch.tensor([0., 0., 800.], device=dev)).contiguous()
seq_r = [rot(n) for _ in range(T)]
seq_t = [(gt_t + R(n, 3) * 5).contiguous() for _ in range(T)]
pm = scflow_amd.DisentanglePointMatchingLoss({'cls_1': {}}, [120., 90.], loss_type='l1', disentangle_z=True, loss_weight=10.)
pm.meshes = verts
sym_samples = int((labels == 0).sum())


def hip_pm():
    return pm.sequence(seq_r, seq_t, gt_r, gt_t, labels)


def torch_pm():
    total = 0.
    for i in range(T):
        loss = 0.
        for b in range(n):
            p = verts[int(b % 2)]
            g_rot = p @ gt_r[b].T
            g_rt = g_rot + gt_t[b]
            p_rot = p @ seq_r[i][b].T + gt_t[b]
            if b % 2 == 0:
                p_rot = p_rot[torch.cdist(g_rt[None], p_rot[None])[0].argmin(1)]
            l_rot = torch.linalg.norm(p_rot - g_rt, dim=-1, ord=1).mean()
            tz = gt_t[b].clone(); tz[2] = seq_t[i][b, 2]
            txy = seq_t[i][b].clone(); txy[2] = gt_t[b, 2]
            l_z = torch.linalg.norm((g_rot + tz) - g_rt, dim=-1, ord=1).mean()
            l_xy = torch.linalg.norm((g_rot + txy) - g_rt, dim=-1, ord=1).mean()
            loss = loss + ((l_z + l_xy) + l_rot) / (120. if b % 2 == 0 else 90.)
        total = total + 0.8 ** (T - 1 - i) * (10. * (loss / n))
    return total


res = dict(batch=n, size=[H, W], iters=T, vertices=V, symmetric_samples=sym_samples,
           meshes='synthetic random vertex sets (no YCB-V mesh available)')
res['pixel_hip_us'] = timeit(hip_pixel)
res['pixel_torch_us'] = timeit(torch_pixel, n=5)
pix_bytes = 4 * n * H * W * (2 + 1 + T * (2 + 2 + 1))
res['pixel_bytes'] = pix_bytes
res['pixel_fraction_of_hbm_peak'] = round(pix_bytes / (res['pixel_hip_us']['median'] * 1e-6) / HBM_PEAK, 4)
res['pm_hip_us'] = timeit(hip_pm, n=10)
res['pm_torch_us'] = timeit(torch_pm, n=2)
pairs = T * sym_samples * V * V
res['pm_pairs'] = pairs
res['pm_pairs_per_s'] = round(pairs / (res['pm_hip_us']['median'] * 1e-6), 0)
res['pm_fraction_of_fp32_vector_peak'] = round(pairs * OPS_PER_PAIR / (res['pm_hip_us']['median'] * 1e-6) / FP32_VECTOR_PEAK, 4)
a, b = hip_pixel()[1].cpu().numpy(), np.array([float(x) for x in torch_pixel()])
res['pixel_torch_vs_hip_rel'] = float(np.abs(a - b).max() / np.abs(b).max())
res['pixel_totals'] = dict(hip=[float(x) for x in a], torch=[float(x) for x in b])
res['pm_total'] = dict(hip=float(hip_pm()[0]), torch=float(torch_pm()))
res['pm_torch_vs_hip_rel'] = float(abs(float(hip_pm()[0]) - float(torch_pm())) / abs(float(torch_pm())))

shapes = json.load(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden',
                                     'state_dict_keys.json')))['shapes']
model = scflow_amd.build_refiner(scflow_amd.scflow_model_cfg(iters=T))
model.load_state_dict(scflow_amd.fill_state_dict(shapes, seed=0), strict=True)
model = model.to(dev)
inp = {k: v.to(dev) for k, v in scflow_amd.make_inputs(n, H, W, seed=1).items()}
step = lambda: model.get_pose(inp['render_images'], inp['real_images'], inp['ref_rotation'], inp['ref_translation'],
                              inp['depth'], inp['internel_k'], inp['label'])
res['get_pose_us'] = timeit(step, n=10)
res['loss_share_of_get_pose'] = round((res['pixel_hip_us']['median'] + res['pm_hip_us']['median']) / res['get_pose_us']['median'], 4)
print(json.dumps(res))
