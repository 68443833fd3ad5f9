"""Micro-benchmark of the pose head's fully connected tail backward (``MultiClassPoseHead.tail_backward``:
``scf_fc_operand``, ``scf_pose_select_grad``, ``scf_fc_wgrad``, ``scf_fc_dgrad``, ``scf_group_norm_flat_grad``) at batch 32,
8 iterations, ``feat_size`` 32 x 32 (2048 features: M = 256 rows through every launch), random weights, tail inputs and
cotangents.  Device events bracket a window of calls; every shape is warmed up first.
    python tools/bench_fc_grad.py [N]   -> one JSON line
``hip_us`` is ``tail_backward`` from the saved tail inputs: it recomputes the activations by the forward's launches, so it
is a forward + backward figure.  ``torch_us`` is torch autograd on the same GPU of the same tail in plain fp32 torch
(``F.group_norm``, ``F.linear``, gather), forward + backward, since autograd needs its own forward;
``torch_backward_us`` times its ``backward()`` alone on a graph built outside the window.  ``hip_backward_us`` times the
seven backward launches alone on activations computed outside the window.
The HIP figure is set against the bytes that MUST move at the 8 TB/s HBM peak: every weight read once per GEMM that
contracts it (fc1, fc2 in dgrad; the selected head rows), every weight gradient written once, the activations read by
wgrad and as masks, the cotangents written and read once.  The events bracket the Python calls, so every HIP figure
includes the binding's host path and allocations: the fraction of peak is a lower limit for the kernels.  The gradients of
the two implementations are compared at the end."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import scflow_amd  # noqa: E402
from scflow_amd import ops  # noqa: E402
from scflow_amd.registry import HEAD, build_from_cfg  # noqa: E402

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
T, FEAT = 8, (32, 32)
head = build_from_cfg(dict(scflow_amd.scflow_model_cfg()['decoder']['pose_head_cfg'], feat_size=FEAT), HEAD)
g = torch.Generator().manual_seed(0)
for prm in head.parameters():
    prm.data.copy_(torch.randn(prm.shape, generator=g) * (0.05 if prm.dim() > 1 else 0.1))
with torch.no_grad():
    head.conv_layers[2].gn.weight.add_(1.0)
head = head.to(dev)
last, fc1, fc2 = head.conv_layers[2], head.fc_layers[0][0], head.fc_layers[1][0]
C, hh, ww = 128, FEAT[0] // 8, FEAT[1] // 8
gd = torch.Generator(dev).manual_seed(1)
R = lambda *s: torch.randn(s, device=dev, generator=gd)       # noqa: E731
ys = [R(n, C, hh, ww) for _ in range(T)]
g_rot, g_trans = [R(n, 6) for _ in range(T)], [R(n, 3) for _ in range(T)]
label = torch.randint(0, head.num_class, (n,), device=dev, generator=gd)
M, K0, O1, O2, NC = T * n, C * hh * ww, fc1.out_features, fc2.out_features, head.num_class
PARAMS = [last.gn.weight, last.gn.bias, fc1.weight, fc1.bias, fc2.weight, fc2.bias, head.rotation_pred.weight,
          head.rotation_pred.bias, head.translation_pred.weight, head.translation_pred.bias]
NAMES = ['conv_layers.2.gn.weight', 'conv_layers.2.gn.bias', 'fc_layers.0.0.weight', 'fc_layers.0.0.bias', 'fc_layers.1.0.weight',
         'fc_layers.1.0.bias', 'rotation_pred.weight', 'rotation_pred.bias', 'translation_pred.weight', 'translation_pred.bias']


def torch_graph():
    prm = [p.detach().requires_grad_() for p in PARAMS]
    yl = [y.detach().requires_grad_() for y in ys]
    c = label[0]
    total = 0.
    for t in range(T):
        x = torch.relu(F.group_norm(yl[t], last.groups, prm[0], prm[1], last.gn.eps)).flatten(1)
        x = torch.relu(F.linear(torch.relu(F.linear(x, prm[2], prm[3])), prm[4], prm[5]))
        rot = F.linear(x, prm[6], prm[7]).view(n, NC, 6)[:, c]
        tr = F.linear(x, prm[8], prm[9]).view(n, NC, 3)[:, c]
        total = total + (rot * g_rot[t]).sum() + (tr * g_trans[t]).sum()
    return total, (yl, prm)


def torch_autograd():
    total, leaves = torch_graph()
    total.backward()
    return leaves


def hip_backward():
    return head.tail_backward(ys, label, g_rot, g_trans)


ystack = torch.stack(ys, 0).view(1, M, C, hh, ww)
acts = head._tail(ystack, activations=True)
gr, gt = torch.cat(g_rot), torch.cat(g_trans)


def hip_backward_alone():
    x0, a1, a2 = acts
    g_s2, _ = ops.pose_select_grad(gr, gt, head.rotation_pred.weight, head.translation_pred.weight, a2, label, n, 0)
    ops.fc_wgrad(g_s2, a1)
    g_s1 = ops.fc_dgrad(g_s2, fc2.weight, a1)
    ops.fc_wgrad(g_s1, x0)
    g_x0 = ops.fc_dgrad(g_s1, fc1.weight)
    return ops.group_norm_flat_grad(g_x0, ystack.view(1, M, K0), x0, last.gn.weight, last.groups, hh * ww, last.gn.eps)


res = dict(batch=n, iters=T, feat_size=list(FEAT), rows=M, fc_plan=list(head.fc_plan()))
weights = K0 * O1 + O1 * O2
# dgrad reads fc1 / fc2 once, wgrad writes them once; the forward recomputation reads them once more; activations and
# cotangents: x0, a1, a2 written once and read by wgrad and as masks (3 x), y read by the operand, the forward and the
# GroupNorm backward (3 x), g_s2, g_s1, g_x0 written and read twice (wgrad + dgrad), g_y written
BYTES = 4 * (3 * weights + 9 * NC * O2 + M * (3 * K0 + 4 * (K0 + O1 + O2) + 3 * (O2 + O1 + K0) + K0))
res['hip_us'] = timeit(hip_backward, inner=5)
res['hip_backward_us'] = timeit(hip_backward_alone, inner=5)
res['torch_us'] = timeit(torch_autograd, n=10)
res['torch_backward_us'] = timeit(lambda total, leaves: total.backward(), n=10, setup=torch_graph)
res['bytes'] = BYTES
res['fraction_of_hbm_peak'] = round(BYTES / (res['hip_us']['median'] * 1e-6) / HBM_PEAK, 4)
res['beats_torch_autograd'] = res['hip_us']['median'] < res['torch_us']['median']
res['backward_alone_beats_torch_backward'] = res['hip_backward_us']['median'] < res['torch_backward_us']['median']
(g_ys, grads), (yl, prm) = hip_backward(), torch_autograd()
rel = lambda a, b: float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))   # noqa: E731
res['torch_vs_hip_rel'] = max([rel(a, b.grad) for a, b in zip(g_ys, yl)] + [rel(grads[k], p.grad) for k, p in zip(NAMES, prm)])
print(json.dumps(res))
