"""Micro-benchmark of the value-and-gradient loss entries (``scf_seq_pixel_loss_grad`` + ``scf_point_matching_loss_grad``)
on the workload of ``tools/bench_loss.py``: batch 32, 256 x 256, 8 iterations, the SYNTHETIC classes of 8192 random vertices
(one symmetric, one not; samples alternate).  Device events bracket a window of calls; every shape is warmed up first.
    python tools/bench_loss_grad.py [N] [V]   -> one JSON line
Three columns per stage (pixel: two flow sequences + the mask sequence; point matching: disentangled, l1, z apart):
1. ``*_grad_us``   the value-and-gradient call (values, neighbours and every gradient from one pass);
2. ``*_value_us``  the forward-only call, as it was before the gradients existed;
3. ``*_torch_us``  torch autograd, forward + backward, of the reference's expressions in fp32 on the same GPU (per-iteration
   loop; per-sample loop with ``torch.cdist`` + ``argmin`` for the symmetric class: the reference's structure).
The pixel pass is also set against the bytes it MUST move at the 8 TB/s HBM peak: every prediction read once, every
gradient written once, the ground truth and ``valid`` read once by the main pass and once by the count pre-pass.
The events bracket the Python calls, so every HIP figure includes the binding's host path and allocations; the fraction
of peak is a lower limit for the kernels.  Gradients of the two implementations are compared at the end."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import scflow_amd  # noqa: E402
from scflow_amd import losses as L  # noqa: E402

dev = 'cuda:0'
HBM_PEAK = 8.0e12


def timeit(fn, n=20, inner=1):
    for _ in range(3):
        fn()
    evs = []
    for _ in range(n):
        s = torch.cuda.Event(enable_timing=True); e = torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(inner):
            fn()
        e.record(); evs.append((s, e))
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) / inner for a, b in evs)
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
PIX = dict(flow_a=flow_a, flow_b=flow_b, masks=masks, loss_weight=W3, eps=EPS, gamma=GAM)


def hip_pixel_grad():
    return L.seq_pixel_loss_grad(gt, valid, **PIX)


def hip_pixel_value():
    return L.seq_pixel_loss(gt, valid, **PIX)


def torch_pixel(fa, fb, mk):
    mag = (gt[:, 0] * gt[:, 0] + gt[:, 1] * gt[:, 1]).sqrt()
    v = ((valid >= 0.5) & (mag < 400.)).to(gt)
    occ = (gt[:, 0] + gt[:, 1] < 400.).float()
    tot = 0.
    for i in range(T):
        wi = 0.8 ** (T - 1 - i)
        for s, seq in enumerate((fa, fb)):
            tot = tot + wi * (W3[s] * ((v[:, None] * (seq[i] - gt).abs()).sum() / (v.sum() + 1e-10)))
        tot = tot + wi * (torch.mean(torch.abs(mk[i] - occ)) * W3[2])
    return tot


def torch_pixel_autograd():
    leaves = [[t.detach().requires_grad_() for t in seq] for seq in (flow_a, flow_b, masks)]
    torch_pixel(*leaves).backward()
    return leaves


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


def hip_pm_grad():
    return pm.sequence_grad(seq_r, seq_t, gt_r, gt_t, labels)


def hip_pm_value():
    return pm.sequence(seq_r, seq_t, gt_r, gt_t, labels)


def torch_pm(sr, st):
    total = 0.
    for i in range(T):
        loss = 0.
        for b in range(n):
            p = verts[int(b % 2)]
            g_rot = p @ gt_r[b].T
            g_rt = g_rot + gt_t[b]
            p_rot = p @ sr[i][b].T + gt_t[b]
            if b % 2 == 0:
                with torch.no_grad():
                    idx = torch.cdist(g_rt[None], p_rot[None])[0].argmin(1)
                p_rot = p_rot[idx]
            l_rot = torch.linalg.norm(p_rot - g_rt, dim=-1, ord=1).mean()
            tz = torch.cat([gt_t[b, :2], st[i][b, 2:]])
            txy = torch.cat([st[i][b, :2], gt_t[b, 2:]])
            l_z = torch.linalg.norm((g_rot + tz) - g_rt, dim=-1, ord=1).mean()
            l_xy = torch.linalg.norm((g_rot + txy) - g_rt, dim=-1, ord=1).mean()
            loss = loss + ((l_z + l_xy) + l_rot) / (120. if b % 2 == 0 else 90.)
        total = total + 0.8 ** (T - 1 - i) * (10. * (loss / n))
    return total


def torch_pm_autograd():
    sr, st = [t.detach().requires_grad_() for t in seq_r], [t.detach().requires_grad_() for t in seq_t]
    torch_pm(sr, st).backward()
    return sr, st


res = dict(batch=n, size=[H, W], iters=T, vertices=V, meshes='synthetic random vertex sets (no YCB-V mesh available)')
res['pixel_grad_us'] = timeit(hip_pixel_grad, inner=5)
res['pixel_value_us'] = timeit(hip_pixel_value, inner=5)
res['pixel_torch_us'] = timeit(torch_pixel_autograd, n=5)
pix_bytes = 4 * n * H * W * (2 * T * (2 + 2 + 1) + 2 * (2 + 1))
res['pixel_grad_bytes'] = pix_bytes
res['pixel_grad_fraction_of_hbm_peak'] = round(pix_bytes / (res['pixel_grad_us']['median'] * 1e-6) / HBM_PEAK, 4)
res['pm_grad_us'] = timeit(hip_pm_grad, n=10)
res['pm_value_us'] = timeit(hip_pm_value, n=10)
res['pm_torch_us'] = timeit(torch_pm_autograd, n=2)
res['grad_beats_torch_autograd'] = dict(pixel=res['pixel_grad_us']['median'] < res['pixel_torch_us']['median'],
                                        pm=res['pm_grad_us']['median'] < res['pm_torch_us']['median'])

rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
hip, ref = hip_pixel_grad()[2], torch_pixel_autograd()
res['pixel_grad_torch_vs_hip_rel'] = max(rel(h, r.grad) for hs, rs in zip(hip, ref) for h, r in zip(hs, rs))
out, (sr, st) = hip_pm_grad(), torch_pm_autograd()
res['pm_grad_torch_vs_hip_rel'] = max([rel(h, r.grad) for h, r in zip(out[4], sr)] + [rel(h, r.grad) for h, r in zip(out[5], st)])
print(json.dumps(res))
