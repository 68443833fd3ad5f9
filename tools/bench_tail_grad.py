"""Micro-benchmark of the iteration-tail backward (``SCFlowDecoder.tail_backward``: ``scf_resize_bilinear_grad``,
``scf_reproject_flow_grad``, ``scf_pose_tail_grad``) on the workload of ``tools/bench_loss_grad.py``: batch 32, 256 x 256,
8 iterations, synthetic head outputs, poses and cotangents.  Device events bracket a window of calls; every shape is
warmed up first.
    python tools/bench_tail_grad.py [N]   -> one JSON line
Three configurations, two columns each:
1. ``shipped``      point-matching pose loss, every ``detach_*`` set: cotangents of flow_from_pred, the masks and the poses;
                    two launches (all up-sampling adjoints, the pose scan);
2. ``flow_pose``    the pose loss a ``RAFTLoss``: cotangents of flow_from_pose instead of the poses; the re-projection
                    sums are a third launch;
3. ``attached``     as 2 with ``detach_flow=False``: a fourth launch takes the 1/8 down-sampling's adjoint into
                    flow_from_pose.
``*_hip_us`` is ``tail_backward``; ``*_torch_us`` is torch autograd on the same GPU of the tail in plain fp32 torch
(``F.interpolate``, ``F.normalize`` / ``torch.cross``, dense re-projection), forward + backward, since autograd needs its
own forward; ``*_torch_backward_us`` times its ``backward()`` alone on a graph built outside the window.
The HIP figures are set against the bytes that MUST move at the 8 TB/s HBM peak: every full-resolution cotangent read
once (201 MB for 1; with the re-projection the 134 MB of flow_from_pose cotangents are read once more: 335 MB).  The
events bracket the Python calls, so every HIP figure includes the binding's host path and allocations: the fraction of
peak is a lower limit for the kernels.  The gradients of the two implementations are compared at the end."""
import json
import os
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import scflow_amd  # noqa: E402,F401
from scflow_amd.modules import SCFlowDecoder  # noqa: E402

dev = 'cuda:0'
HBM_PEAK = 8.0e12


def timeit(fn, n=20, inner=1, setup=None):
    for _ in range(3):
        fn(*(setup() if setup else ()))
    evs = []
    for _ in range(n):
        args = setup() if setup else ()
        s = torch.cuda.Event(enable_timing=True); e = torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(inner):
            fn(*args)
        e.record(); evs.append((s, e))
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) / inner for a, b in evs)
    return dict(median=round(ts[len(ts) // 2] * 1e3, 1), min=round(ts[0] * 1e3, 1))


n = int(sys.argv[1]) if len(sys.argv) > 1 else 32
T, H, W, S = 8, 256, 256, 8
h, w = H // S, W // S
g = torch.Generator(dev).manual_seed(0)
R = lambda *s: torch.randn(s, device=dev, generator=g)       # noqa: E731
depth = 0.8 + 0.4 * torch.rand((n, H, W), device=dev, generator=g)
depth[torch.rand((n, H, W), device=dev, generator=g) < 0.4] = 0.
K = torch.tensor([[280., 0., 128.], [0., 280., 128.], [0., 0., 1.]], device=dev).repeat(n, 1, 1).contiguous()
q, _ = torch.linalg.qr(R(n, 3, 3))
rot0 = (q * torch.sign(torch.linalg.det(q))[:, None, None]).contiguous()
trans0 = (R(n, 3) * 0.05 + torch.tensor([0., 0., 1.], device=dev)).contiguous()
eye6 = torch.tensor([1., 0., 0., 0., 1., 0.], device=dev)
d_flow = [R(n, 2, h, w) for _ in range(T)]
mask = [torch.rand((n, 1, h, w), device=dev, generator=g) for _ in range(T)]
d_rot = [(eye6 + 0.05 * R(n, 6)).contiguous() for _ in range(T)]
d_trans = [(0.02 * R(n, 3)).contiguous() for _ in range(T)]
init_flow = torch.zeros((n, 2, H, W), device=dev)
cot = dict(sequence_flow_from_pose=[R(n, 2, H, W) * 1e-3 for _ in range(T)],
           sequence_flow_from_pred=[R(n, 2, H, W) * 1e-3 for _ in range(T)],
           sequence_masks=[R(n, 1, H, W) * 1e-3 for _ in range(T)],
           seq_rotations=[R(n, 3, 3) for _ in range(T)], seq_translations=[R(n, 3) for _ in range(T)])
CONFIGS = dict(shipped=(('sequence_flow_from_pred', 'sequence_masks', 'seq_rotations', 'seq_translations'), (True, True, True)),
               flow_pose=(('sequence_flow_from_pose', 'sequence_flow_from_pred', 'sequence_masks'), (True, True, True)),
               attached=(('sequence_flow_from_pose', 'sequence_flow_from_pred', 'sequence_masks'), (False, True, True)))


def torch_tail(df, mk, dr, dt, flags):
    """scflow_decoder.py:191-250 without the network, fp32, dense re-projection."""
    detach_flow, detach_pose, detach_depth = flags
    fg = depth > 0
    dd = torch.where(fg, depth, torch.ones_like(depth))
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing='ij')
    mv = lambda m, v: torch.einsum('nij,njhw->nihw', m, v)    # noqa: E731
    P = mv(torch.inverse(rot0), mv(torch.inverse(K), torch.stack([xs[None] * dd, ys[None] * dd, dd], 1)) - trans0[:, :, None, None])
    xy = torch.stack([xs, ys], 0)[None]
    flow, rot, trans = init_flow, rot0, trans0
    out = ([], [], [], [], [])
    for i in range(T):
        if detach_flow:
            flow = flow.detach()
        flow = 1 / S * F.interpolate(flow, scale_factor=(1 / S, 1 / S), mode='bilinear', align_corners=True)
        flow_pred = S * F.interpolate(flow + df[i], scale_factor=(S, S), mode='bilinear', align_corners=True)
        up_mask = F.interpolate(mk[i], scale_factor=(S, S), mode='bilinear', align_corners=True)
        rp, tp = (rot.detach(), trans.detach()) if detach_pose else (rot, trans)
        x = F.normalize(dr[i][:, 0:3], dim=1)
        z = F.normalize(torch.cross(x, dr[i][:, 3:6], dim=1), dim=1)
        rot = torch.bmm(torch.stack([x, torch.cross(z, x, dim=1), z], dim=2), rp)
        vz = tp[:, 2] / torch.exp(dt[i][:, 2])
        vzs = vz.detach() if detach_depth else vz
        trans = torch.stack([vzs * torch.addcdiv(dt[i][:, 0] / 10., tp[:, 0], tp[:, 2]),
                             vzs * torch.addcdiv(dt[i][:, 1] / 10., tp[:, 1], tp[:, 2]), vz], dim=-1)
        qq = mv(K, mv(rot, P) + trans[:, :, None, None])
        flow = torch.where(fg[:, None], qq[:, :2] / qq[:, 2:3] - xy, torch.zeros_like(qq[:, :2]))
        for lst, v in zip(out, (flow, flow_pred, rot, trans, up_mask)):
            lst.append(v)
    return out


ORDER = ('sequence_flow_from_pose', 'sequence_flow_from_pred', 'seq_rotations', 'seq_translations', 'sequence_masks')


def torch_graph(keys, flags):
    leaves = [[t.detach().requires_grad_() for t in seq] for seq in (d_flow, mask, d_rot, d_trans)]
    out = torch_tail(*leaves, flags)
    total = sum((o * c).sum() for key, seq in zip(ORDER, out) if key in keys for o, c in zip(seq, cot[key]))
    return total, leaves


def torch_autograd(keys, flags):
    total, leaves = torch_graph(keys, flags)
    total.backward()
    return leaves


with torch.no_grad():
    fwd = torch_tail(d_flow, mask, d_rot, d_trans, (True, True, True))
outs = (fwd[0], fwd[1], [r.contiguous() for r in fwd[2]], [t.contiguous() for t in fwd[3]], fwd[4], d_rot, d_trans)


def hip_tail(keys, flags):
    dec = types.SimpleNamespace(num_levels=4, detach_flow=flags[0], detach_pose=flags[1], detach_depth_for_xy=flags[2],
                                depth_transform='exp', pose_flags=lambda: 1)
    return SCFlowDecoder.tail_backward(dec, outs, {key: cot[key] for key in keys}, rot0, trans0, depth, K)


res = dict(batch=n, size=[H, W], iters=T)
plane = 4 * n * H * W
BYTES = dict(shipped=plane * T * 3 + plane * T * 3 // 64, flow_pose=plane * T * 5 + plane * T * 3 // 64 + plane,
             attached=plane * T * 5 + plane * T * 3 // 64 + plane + 2 * plane * (T - 1) * 2)
rel = lambda a, b: float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))   # noqa: E731
for name, (keys, flags) in CONFIGS.items():
    res[f'{name}_hip_us'] = timeit(lambda: hip_tail(keys, flags), inner=5)
    res[f'{name}_torch_us'] = timeit(lambda: torch_autograd(keys, flags), n=5)
    res[f'{name}_torch_backward_us'] = timeit(lambda total, leaves: total.backward(), n=5, setup=lambda: torch_graph(keys, flags))
    res[f'{name}_bytes'] = BYTES[name]
    res[f'{name}_fraction_of_hbm_peak'] = round(BYTES[name] / (res[f'{name}_hip_us']['median'] * 1e-6) / HBM_PEAK, 4)
    res[f'{name}_beats_torch_autograd'] = res[f'{name}_hip_us']['median'] < res[f'{name}_torch_us']['median']
    hip, ref = hip_tail(keys, flags), torch_autograd(keys, flags)
    res[f'{name}_torch_vs_hip_rel'] = max(rel(a, b.grad.view(a.shape)) for key, seq in zip(('delta_flow_preds', 'masks', 'delta_rotation_preds',
                                                                                             'delta_translation_preds'), ref)
                                          for a, b in zip(hip[key], seq) if b.grad is not None)
print(json.dumps(res))
