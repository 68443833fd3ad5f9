"""Micro-benchmark of the feature encoder's backward (``RAFTEncoder.in_backward``: ``scf_instance_norm_grad`` /
``scf_instance_norm_res_norm_grad`` and the convolution gradients between them) at the workload of the shared encoder:
2N = 64 stacked images of 3 x 256 x 256, random weights, images and cotangents.  Device events bracket a window of calls;
every column is warmed up first; the columns alternate inside one process, and each figure is the median of the windows
with their 10 % and 90 % points.
    python tools/bench_feature_grad.py [2N]   -> one JSON line
``hip_us`` is ``in_backward`` from what a forward under ``keeping()`` keeps.  ``launch_us`` times each launch of the new
kernel alone, at the operands the stage gives it (``intermediates``); ``floor_fraction`` is its byte floor over its
measured median: 12 (mid: g, u read, du written), 20 (tail: G, y, u read, g', du written) and 24 (tail with a normalised
shortcut: G, y, u, r read, du, dr written) bytes an element at the 6.29 TB/s float4-copy rate of DESIGN.md 4.11.
``torch_us`` is torch autograd on the same GPU of the same encoder built from ``torch.nn.functional`` (``conv2d``,
``instance_norm``, ``relu``), forward + backward -- what these gradients cost a user of torch; ``torch_backward_us`` times
its ``backward()`` alone on a graph built outside the window.  ``not_slower_than_torch`` is the gate of DESIGN.md 4.17:
median(hip) <= median(torch) + the two spreads.  The events bracket the Python calls, so every HIP figure includes the
binding's host path and allocations.  The gradients of the two implementations are compared at the end, relative to the
largest entry (a plausibility figure; the kernels are held to float64 by tests/test_gpu_feature_grad.py)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from scflow_amd import ops  # noqa: E402
from scflow_amd.modules import RAFTEncoder  # noqa: E402

dev = 'cuda:0'
COPY_RATE = 6.29e12


def window(fn, inner, args=()):
    s = torch.cuda.Event(enable_timing=True); e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(inner):
        fn(*args)
    e.record()
    return s, e


def alternate(columns, n=11):
    """columns: name -> (fn, inner, setup or None); every repetition times each column once, in turn"""
    for fn, _, setup in columns.values():
        for _ in range(2):
            fn(*(setup() if setup else ()))
    evs = {k: [] for k in columns}
    for _ in range(n):
        for k, (fn, inner, setup) in columns.items():
            evs[k].append((window(fn, inner, setup() if setup else ()), inner))
    torch.cuda.synchronize()
    out = {}
    for k, lst in evs.items():
        ts = sorted(s.elapsed_time(e) / inner for (s, e), inner in lst)
        out[k] = dict(median=round(ts[len(ts) // 2] * 1e3, 1), p10=round(ts[n // 10] * 1e3, 1), p90=round(ts[n - 1 - n // 10] * 1e3, 1))
    return out


n = int(sys.argv[1]) if len(sys.argv) > 1 else 64
H = W = 256
torch.manual_seed(0)
enc = RAFTEncoder(3, 256, norm_cfg=dict(type='IN'))
with torch.no_grad():
    for name, p in enc.named_parameters():
        p.copy_(torch.randn_like(p) * (0.05 if p.dim() > 1 else 0.1))
enc = enc.to(dev)
x = torch.randn(n, 3, H, W, device=dev)
g = torch.randn(n, 256, H // 8, W // 8, device=dev)
with enc.keeping():
    enc(x)
saved = enc.kept
im = {}
grads = enc.in_backward(saved, g, intermediates=im)
torch.cuda.synchronize()

# ---- the stage and the launches of the new kernel
cols = {'hip': (lambda: enc.in_backward(saved, g), 2, None)}
floors = {}
for key, r in im.items():
    if not (key == 'in1' or key.endswith(('.in1', '.in2'))):
        continue
    form, per = ('mid', 12) if 'y' not in r else ('tail', 20) if 'r' not in r else ('tail_ds', 24)
    name = f"{form} {key}[{r['u'].shape[1]}@{r['u'].shape[2]}]"
    cols[name] = (lambda r=r: ops.instance_norm_grad(r['g'], r['u'], y=r.get('y'), r=r.get('r')), 10, None)
    floors[name] = r['u'].numel() * per / COPY_RATE * 1e6

# ---- torch autograd of the same encoder on the same GPU
P = {k: v.detach().clone().requires_grad_(True) for k, v in enc.state_dict().items()}


def t_layer(v, ckey, stride, pad):
    return F.instance_norm(F.conv2d(v, P[f'{ckey}.weight'], P[f'{ckey}.bias'], stride=stride, padding=pad), eps=1e-5)


def t_forward():
    v = torch.relu(t_layer(x, 'conv1', 2, 3))
    for li, stride in enumerate((1, 2, 2), start=1):
        for j in range(2):
            key, s = f'res_layer{li}.{j}', (stride if j == 0 else 1)
            t = torch.relu(t_layer(v, f'{key}.conv1', s, 1))
            idt = t_layer(v, f'{key}.downsample.0', s, 0) if f'{key}.downsample.0.weight' in P else v
            v = torch.relu(t_layer(t, f'{key}.conv2', 1, 1) + idt)
    return F.conv2d(v, P['conv2.weight'], P['conv2.bias'])


leaves = list(P.values())


def t_both():
    return torch.autograd.grad((t_forward() * g).sum(), leaves)


cols['torch'] = (t_both, 2, None)
cols['torch_backward'] = (lambda loss: torch.autograd.grad(loss, leaves), 1, lambda: ((t_forward() * g).sum(),))

res = alternate(cols)
tg = dict(zip(P, t_both()))
zero = [k for k in grads if k.endswith('.bias') and k != 'conv2.bias']          # exact gradient 0: rounding noise in both
worst = max(float((grads[k] - tg[k]).abs().max() / tg[k].abs().max()) for k in grads if k not in zero)
spread = lambda v: v['p90'] - v['p10']                      # noqa: E731
launch = {k: v for k, v in res.items() if k not in ('hip', 'torch', 'torch_backward')}
out = dict(batch=n, image=[H, W], hip_us=res['hip'], torch_us=res['torch'], torch_backward_us=res['torch_backward'],
           not_slower_than_torch=res['hip']['median'] <= res['torch']['median'] + spread(res['hip']) + spread(res['torch']),
           launch_us=launch,
           floor_fraction={k: round(floors[k] / v['median'], 3) for k, v in launch.items()},
           instance_norm_grad_sum_us=round(sum(v['median'] for v in launch.values()), 1),
           worst_gradient_difference_to_torch=worst)
print(json.dumps(out))
