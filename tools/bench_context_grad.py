"""Micro-benchmark of the context encoder's backward (``RAFTEncoder.backward``: ``scf_conv_stem_wgrad``,
``scf_conv_ds_dgrad`` / ``scf_conv_ds_wgrad``, ``scf_channel_sum``, ``scf_bn_fold`` / ``scf_bn_unfold`` and the
``scf_conv_s1_*`` / ``scf_conv_*grad`` launches between them) at batch 32, 256 x 256 images, random weights with running
statistics away from (0, 1), random images and cotangents.  Device events bracket a window of calls; every shape is
warmed up first; the columns alternate inside one run.
    python tools/bench_context_grad.py [N]   -> one JSON line
``hip_us`` is ``backward`` from what a forward under ``keeping()`` keeps.  ``launch_us`` times each launch of the stage
alone, at the operands the stage gives it (``intermediates``); ``floor_fraction`` is, for each new kernel, its floor over its
measured median: the compulsory traffic at the 6.29 TB/s float4-copy rate of DESIGN.md 4.11 (the stem: ``g`` and ``x`` once;
the shortcut's join: ``g``, ``add``, ``a`` read and ``gx`` written once; the shortcut's weight gradient: ``g`` and the even
rows of ``x``; the channel sum: ``g``), and for the stem also the fp32-MFMA floor, 2 M Ho Wo 64 x 160 padded columns at
157.3 TFLOP/s.  ``torch_us`` is torch autograd on the same GPU of a plain-torch restatement of the encoder (``conv2d``,
``batch_norm(training=False)``, ``relu``, split tanh | relu), forward + backward; ``torch_backward_us`` times its
``backward()`` alone on a graph built outside the window; ``torch_launch_us`` the torch gradients of the stem and of a
shortcut alone (``torch.nn.grad``).  The events bracket the Python calls, so every HIP figure includes the binding's host
path and allocations.  The gradients of the two implementations are compared at the end, relative to the largest entry
(a plausibility figure: a ReLU within rounding of zero is on in one and off in the other; the kernels are held to float64 by
tests/test_gpu_context_grad.py)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from scflow_amd import ops  # noqa: E402
from scflow_amd.modules import RAFTEncoder  # noqa: E402

dev = 'cuda:0'
COPY_RATE, MFMA_RATE = 6.29e12, 157.3e12


def window(fn, inner, args=()):
    s = torch.cuda.Event(enable_timing=True); e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(inner):
        fn(*args)
    e.record()
    return s, e


def alternate(columns, n=7):
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
        out[k] = dict(median=round(ts[len(ts) // 2] * 1e3, 1), min=round(ts[0] * 1e3, 1))
    return out


n = int(sys.argv[1]) if len(sys.argv) > 1 else 32
H = W = 256
HEAD = dict(head_act=ops.ACT_TANH, head_act2=ops.ACT_RELU, head_split=128)
torch.manual_seed(0)
enc = RAFTEncoder(3, 256, norm_cfg=dict(type='BN'))
with torch.no_grad():
    for name, p in enc.named_parameters():
        p.copy_(torch.randn_like(p) * (0.05 if p.dim() > 1 else 0.1) + (1.0 if ('bn' in name or 'downsample.1' in name)
                                                                         and name.endswith('weight') else 0.0))
    for name, b in enc.named_buffers():
        if name.endswith('running_mean'):
            b.copy_(0.3 * torch.randn_like(b))
        elif name.endswith('running_var'):
            b.copy_(0.5 + torch.randn_like(b).abs())
enc = enc.to(dev)
x = torch.randn(n, 3, H, W, device=dev)
g = torch.randn(n, 256, H // 8, W // 8, device=dev)
with enc.keeping():
    enc(x, **HEAD)
saved = enc.kept
im = {}
grads = enc.backward(saved, g, **HEAD, intermediates=im)
torch.cuda.synchronize()

# ---- the stage and its launches
cols = {'hip': (lambda: enc.backward(saved, g, **HEAD), 3, None)}
floors = {}


def add(name, fn, floor_bytes=None, floor_flop=None):
    cols[name] = (fn, 10, None)
    if floor_bytes is not None:
        floors[name] = dict(bytes_us=floor_bytes / COPY_RATE * 1e6)
        if floor_flop is not None:
            floors[name]['mfma_us'] = floor_flop / MFMA_RATE * 1e6


nb = lambda *ts: sum(t.numel() for t in ts) * 4          # noqa: E731
r = im['conv1']
add('stem_wgrad', lambda r=r: ops.conv_stem_wgrad(r['g'], r['x']), nb(r['g'], r['x']),
    2.0 * r['g'].shape[0] * r['g'].shape[2] * r['g'].shape[3] * 64 * 160)
r = im['head']
add('head_wgrad', lambda r=r: ops.conv_s1_wgrad(r['g'], r['x'], (1, 1)))
add('head_dgrad', lambda r=r: ops.conv_s1_dgrad(r['g'], enc.conv2.weight, a=r['x'], act=ops.ACT_RELU))
for key in [k for k in im if k not in ('conv1', 'head')]:
    r = im[key]
    tag = f"{key}[{r['x'].shape[1]}to{r['g'].shape[1]}@{r['g'].shape[2]}]"
    if key.endswith('downsample'):
        in_hw = tuple(r['x'].shape[2:])
        add(f'ds_wgrad {tag}', lambda r=r: ops.conv_ds_wgrad(r['g'], r['x']), nb(r['g']) + nb(r['x']) // 2)
        add(f'ds_dgrad {tag}', lambda r=r, in_hw=in_hw: ops.conv_ds_dgrad(r['g'], r['wf'], in_hw, add=r['add'], a=r['x'], act=ops.ACT_RELU),
            nb(r['g'], r['add'], r['x'], r['gx']))
    elif r['x'].shape[2] != r['g'].shape[2]:
        in_hw = tuple(r['x'].shape[2:])
        add(f's2_wgrad {tag}', lambda r=r: ops.conv_wgrad(r['g'], r['x']))
        add(f'channel_sum {tag}', lambda r=r: ops.channel_sum(r['g']), nb(r['g']))
        add(f's2_dgrad {tag}', lambda r=r, in_hw=in_hw: ops.conv_dgrad(r['g'], r['wf'], in_hw))
    else:
        add(f's1_wgrad {tag}', lambda r=r: ops.conv_s1_wgrad(r['g'], r['x'], (3, 3)))
        add(f's1_dgrad {tag}', lambda r=r: ops.conv_s1_dgrad(r['g'], r['wf'], add=r.get('add'), a=r['x'], act=ops.ACT_RELU))
blk = enc.res_layer3[1]
bn_args = (blk.conv2.weight, blk.conv2.bias, blk.bn2.weight, blk.bn2.bias, blk.bn2.running_mean, blk.bn2.running_var)
r = im['res_layer3.1.conv2']
add('bn_fold [128x1152]', lambda: ops.bn_fold(*bn_args, blk.bn2.eps))
add('bn_unfold [128x1152]', lambda r=r: ops.bn_unfold(bn_args[0], bn_args[1], bn_args[2], bn_args[4], bn_args[5], blk.bn2.eps,
                                                    r['dwf'], r['dbf']))

# ---- torch autograd of the same encoder on the same GPU
P = {k: v.detach().clone().requires_grad_(v.dtype.is_floating_point and 'running' not in k) for k, v in enc.state_dict().items()}


def t_layer(v, ckey, bkey, stride, pad):
    v = F.conv2d(v, P[f'{ckey}.weight'], P[f'{ckey}.bias'], stride=stride, padding=pad)
    return F.batch_norm(v, P[f'{bkey}.running_mean'], P[f'{bkey}.running_var'], P[f'{bkey}.weight'], P[f'{bkey}.bias'],
                        training=False, eps=1e-5)


def t_forward():
    v = torch.relu(t_layer(x, 'conv1', 'bn1', 2, 3))
    for li, stride in enumerate((1, 2, 2), start=1):
        for j in range(2):
            key, s = f'res_layer{li}.{j}', (stride if j == 0 else 1)
            t = torch.relu(t_layer(v, f'{key}.conv1', f'{key}.bn1', s, 1))
            idt = t_layer(v, f'{key}.downsample.0', f'{key}.downsample.1', s, 0) if f'{key}.downsample.0.weight' in P else v
            v = torch.relu(t_layer(t, f'{key}.conv2', f'{key}.bn2', 1, 1) + idt)
    y = F.conv2d(v, P['conv2.weight'], P['conv2.bias'])
    return torch.cat([torch.tanh(y[:, :128]), torch.relu(y[:, 128:])], 1)


leaves = [v for v in P.values() if v.requires_grad]


def t_both():
    return torch.autograd.grad((t_forward() * g).sum(), leaves)


cols['torch'] = (t_both, 3, None)
cols['torch_backward'] = (lambda loss: torch.autograd.grad(loss, leaves), 1, lambda: ((t_forward() * g).sum(),))
r = im['conv1']
cols['torch stem_wgrad'] = (lambda r=r: torch.nn.grad.conv2d_weight(r['x'], (64, 3, 7, 7), r['g'], stride=2, padding=3), 10, None)
r = im['res_layer2.0.downsample']
cols['torch ds_wgrad [64to96]'] = (lambda r=r: torch.nn.grad.conv2d_weight(r['x'], (96, 64, 1, 1), r['g'], stride=2), 10, None)
cols['torch ds_dgrad [64to96]'] = (lambda r=r: torch.nn.grad.conv2d_input(tuple(r['x'].shape), r['wf'], r['g'], stride=2), 10, None)

res = alternate(cols)
tg = dict(zip([k for k, v in P.items() if v.requires_grad], t_both()))
worst = max(float((grads[k] - tg[k]).abs().max() / tg[k].abs().max()) for k in grads)
out = dict(batch=n, image=[H, W],
           hip_us=res['hip'], torch_us=res['torch'], torch_backward_us=res['torch_backward'],
           launch_us={k: v for k, v in res.items() if k not in ('hip', 'torch', 'torch_backward') and not k.startswith('torch ')},
           torch_launch_us={k[6:]: v for k, v in res.items() if k.startswith('torch ')},
           floor_fraction={k: {f: round(us / res[k]['median'], 3) for f, us in v.items()} for k, v in floors.items()},
           launches_sum_us=round(sum(v['median'] for k, v in res.items()
                                     if k not in ('hip', 'torch', 'torch_backward') and not k.startswith(('torch ', 'bn_'))), 1),
           worst_gradient_difference_to_torch=worst)
print(json.dumps(out))
