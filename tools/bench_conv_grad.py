"""Micro-benchmark of the pose head's convolution backward (``MultiClassPoseHead.conv_backward``: ``scf_conv_wgrad``,
``scf_conv_dgrad``, ``scf_group_norm_flat_grad``) at batch 32, 8 iterations, ``feat_size`` 32 x 32 (M = 256 stacked samples
through every launch), random weights, inputs and cotangents.  Device events bracket a window of calls; every shape is
warmed up first; the HIP and the torch column alternate inside one run.
    python tools/bench_conv_grad.py [N]   -> one JSON line
``hip_us`` is ``conv_backward`` from what the forward saved: the stacking copy, the two GroupNorm forwards that recompute
the activations, the eight backward launches with their combine launches.  ``launch_us`` times each of those launches
alone, with ``mfma_fraction`` = executed flops / time / the 157.3 TF/s fp32 MFMA peak (dgrad executes only the taps that
meet an output pixel: 2 * 9 Cout Cin per 2 x 2 input pixels, like the forward).  ``torch_us`` is torch autograd on the same
GPU of the same three ConvModules in plain fp32 torch (``F.conv2d``, ``F.group_norm``), forward + backward over the 8
iterations one by one, since autograd needs its own forward; ``torch_backward_us`` times its ``backward()`` alone on a
graph built outside the window.  The events bracket the Python calls, so every HIP figure includes the binding's host
path and allocations.  The gradients of the two implementations are compared at the end: the parameter gradients, the
input gradients, and the fraction of input-gradient elements further apart than 1e-4 of the largest entry."""
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
MFMA_PEAK = 157.3e12


def window(fn, inner, args=()):
    s = torch.cuda.Event(enable_timing=True); e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(inner):
        fn(*args)
    e.record()
    return s, e


def alternate(columns, n=15):
    """columns: name -> (fn, inner, setup or None); every repetition times each column once, in turn"""
    for fn, _, setup in columns.values():
        for _ in range(3):
            fn(*(setup() if setup else ()))
    evs = {k: [] for k in columns}
    for _ in range(n):
        for k, (fn, inner, setup) in columns.items():
            evs[k].append((window(fn, inner, setup() if setup else ()), inner))
    torch.cuda.synchronize()
    out = {}
    for k, lst in evs.items():
        ts = sorted(s.elapsed_time(e) / inner for (s, e), inner in lst)
        out[k] = dict(median=round(ts[len(ts) // 2] * 1e3, 1), min=round(ts[0] * 1e3, 1))
    return out


n = int(sys.argv[1]) if len(sys.argv) > 1 else 32
T, FEAT = 8, (32, 32)
head = build_from_cfg(dict(scflow_amd.scflow_model_cfg()['decoder']['pose_head_cfg'], feat_size=FEAT), HEAD)
g = torch.Generator().manual_seed(0)
for prm in head.parameters():
    prm.data.copy_(torch.randn(prm.shape, generator=g) * (0.05 if prm.dim() > 1 else 0.1))
with torch.no_grad():
    for blk in head.conv_layers:
        blk.gn.weight.add_(1.0)
head = head.to(dev)
L0, L1, L2 = head.conv_layers
gd = torch.Generator(dev).manual_seed(1)
R = lambda *s: torch.randn(s, device=dev, generator=gd)       # noqa: E731
M = T * n
hvs, dms = [R(n, 128, *FEAT) for _ in range(T)], [R(n, 96, *FEAT) for _ in range(T)]
sizes = [FEAT]
for _ in range(3):
    sizes.append(((sizes[-1][0] - 1) // 2 + 1, (sizes[-1][1] - 1) // 2 + 1))
g_ys = [R(n, 128, *sizes[3]) for _ in range(T)]
five = lambda y: y if y.dim() == 5 else y[None]                # noqa: E731
raw = [head._conv_outputs(h, d) for h, d in zip(hvs, dms)]
saved = dict(hv=torch.stack(hvs), dm=torch.stack(dms))
for i in range(3):
    saved[f'y{i}'] = torch.stack([five(y[i]) for y in raw], 1).contiguous()
del raw
NAMES = ['conv_layers.0.conv.weight', 'conv_layers.0.gn.weight', 'conv_layers.0.gn.bias', 'conv_layers.1.conv.weight',
         'conv_layers.1.gn.weight', 'conv_layers.1.gn.bias', 'conv_layers.2.conv.weight']
PARAMS = [dict(head.named_parameters())[k] for k in NAMES]


def hip_backward():
    return head.conv_backward(saved, g_ys)


def torch_graph():
    prm = [p.detach().requires_grad_() for p in PARAMS]
    xs = [(h.detach().requires_grad_(), d.detach().requires_grad_()) for h, d in zip(hvs, dms)]
    total = 0.
    for t in range(T):
        a = torch.cat(xs[t], 1)
        a = torch.relu(F.group_norm(F.conv2d(a, prm[0], stride=2, padding=1), L0.groups, prm[1], prm[2], L0.gn.eps))
        a = torch.relu(F.group_norm(F.conv2d(a, prm[3], stride=2, padding=1), L1.groups, prm[4], prm[5], L1.gn.eps))
        total = total + (F.conv2d(a, prm[6], stride=2, padding=1) * g_ys[t]).sum()
    return total, (xs, prm)


def torch_autograd():
    total, leaves = torch_graph()
    total.backward()
    return leaves


# ---- the launches alone, on operands computed outside the window
def act(y, blk, hw):
    yv = y.view(y.shape[0], M, 128, *hw)
    return ops.group_norm_relu(yv if y.shape[0] > 1 else yv[0], blk.gn.weight, blk.gn.bias, blk.groups, blk.gn.eps)


a0, a1 = act(saved['y0'], L0, sizes[1]), act(saved['y1'], L1, sizes[2])
x0, x1 = saved['hv'].view(M, 128, *FEAT), saved['dm'].view(M, 96, *FEAT)
g2 = torch.stack(g_ys).view(M, 128, *sizes[3])
g1, g0 = R(M, 128, *sizes[2]), R(M, 128, *sizes[1])
ws = torch.empty((max(ops.conv_wgrad_workspace(M, 128, c, *hw) for c, hw in zip((224, 128, 128), sizes[1:])),), device=dev)
out_w = [torch.empty_like(b.conv.weight) for b in (L0, L1, L2)]
out_d = [(torch.empty_like(x0), torch.empty_like(x1)), torch.empty_like(a0), torch.empty_like(a1)]


def norm_grad(g_a, y, a, blk, hw):
    k = 128 * hw[0] * hw[1]
    return ops.group_norm_flat_grad(g_a.view(M, k), y.view(y.shape[0], M, k), a.view(M, k), blk.gn.weight, blk.groups,
                                    hw[0] * hw[1], blk.gn.eps)


LAUNCHES = {
    'wgrad2': lambda: ops.conv_wgrad(g2, a1, dw=out_w[2], workspace=ws),
    'dgrad2': lambda: ops.conv_dgrad(g2, L2.conv.weight, sizes[2], out=out_d[2]),
    'gn1_grad': lambda: norm_grad(out_d[2], saved['y1'], a1, L1, sizes[2]),
    'wgrad1': lambda: ops.conv_wgrad(g1, a0, dw=out_w[1], workspace=ws),
    'dgrad1': lambda: ops.conv_dgrad(g1, L1.conv.weight, sizes[1], out=out_d[1]),
    'gn0_grad': lambda: norm_grad(out_d[1], saved['y0'], a0, L0, sizes[1]),
    'wgrad0': lambda: ops.conv_wgrad(g0, x0, x1, dw=out_w[0], workspace=ws),
    'dgrad0': lambda: ops.conv_dgrad(g0, L0.conv.weight, FEAT, split=128, out=out_d[0]),
    'gn_forward_x2': lambda: (act(saved['y0'], L0, sizes[1]), act(saved['y1'], L1, sizes[2])),
}
FLOPS = {f'{k}{i}': 2.0 * M * hw[0] * hw[1] * 9 * 128 * c
         for i, (c, hw) in enumerate(zip((224, 128, 128), sizes[1:])) for k in ('wgrad', 'dgrad')}

res = dict(batch=n, iters=T, feat_size=list(FEAT), samples=M)
columns = {'hip_us': (hip_backward, 3, None)}
try:
    torch_autograd()
    torch.cuda.synchronize()
    columns['torch_us'] = (torch_autograd, 1, None)
    columns['torch_backward_us'] = (lambda total, leaves: total.backward(), 1, torch_graph)
except Exception as exc:                                       # torch's convolution backward cannot run here
    res['torch_error'] = f'{type(exc).__name__}: {exc}'[:200]
res.update(alternate(columns))
res['launch_us'] = alternate({k: (fn, 5, None) for k, fn in LAUNCHES.items()}, n=10)
res['mfma_fraction'] = {k: round(f / (res['launch_us'][k]['median'] * 1e-6) / MFMA_PEAK, 4) for k, f in FLOPS.items()}
res['gflop'] = round(sum(FLOPS.values()) * 1e-9, 1)
res['mfma_fraction_stage'] = round(sum(FLOPS.values()) / (res['hip_us']['median'] * 1e-6) / MFMA_PEAK, 4)
if 'torch_us' in res:
    res['beats_torch_autograd'] = res['hip_us']['median'] < res['torch_us']['median']
    res['beats_torch_backward_alone'] = res['hip_us']['median'] < res['torch_backward_us']['median']
    (g_hvs, g_dms, grads), (xs, prm) = hip_backward(), torch_autograd()
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))   # noqa: E731
    pairs = [(a, x[0].grad) for a, x in zip(g_hvs, xs)] + [(a, x[1].grad) for a, x in zip(g_dms, xs)]
    res['torch_vs_hip_rel_params'] = max(rel(grads[k], p.grad) for k, p in zip(NAMES, prm))
    res['torch_vs_hip_rel_inputs'] = max(rel(a, b) for a, b in pairs)
    # torch's own fp32 forward flips ReLU masks next to zero: single input-gradient elements then differ by whole terms
    res['inputs_beyond_1e-4_fraction'] = (sum(float(((a - b).abs() > 1e-4 * b.abs().max()).sum()) for a, b in pairs)
                                          / sum(a.numel() for a, _ in pairs))
print(json.dumps(res))
