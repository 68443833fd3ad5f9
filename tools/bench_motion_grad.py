"""Micro-benchmark of the motion-encoder and correlation-lookup backward (``SCFlowDecoder.motion_backward``:
``scf_corr_lookup`` recomputation, ``MotionEncoder.backward`` on ``scf_conv_s1_dgrad`` / ``scf_conv_s1_wgrad``,
``scf_corr_lookup_grad``) at batch 32, 8 iterations, 32 x 32 maps, radius 4, 4 levels, random weights, features, flows and
cotangents.  Device events bracket a window of calls; every shape is warmed up first; the columns alternate inside one run.
    python tools/bench_motion_grad.py [N]   -> one JSON line
``hip_us`` is ``motion_backward`` from what a forward at keep level ``'motion'`` keeps: the T lookups and the
recomputation of ``c1``, ``f1``, ``cf`` by the forward's own launches (``recompute_us`` times both alone), the ten
convolution-gradient launches over the T N stacked samples, and the lookup adjoint.  ``launch_us`` times each kind of
launch alone, at the shape the stage gives it.  ``lookup_grad_floor_us`` is the adjoint's compulsory traffic (``g_corr``
read once, ``g_vol`` written once) at the 6.29 TB/s float4-copy rate of DESIGN.md 4.11, ``lookup_grad_floor_fraction`` =
floor / measured median.  ``torch_us`` is torch autograd on the same GPU of a plain-torch restatement (``avg_pool2d``
pyramid from a level-0 leaf, ``grid_sample`` lookup, ``conv2d`` + ReLU encoder), forward + backward; ``torch_backward_us``
times its ``backward()`` alone on a graph built outside the window.  The events bracket the Python calls, so every HIP
figure includes the binding's host path and allocations.  The gradients of the two implementations are compared at the
end, relative to the largest entry; unlike the GRU's, this stage has ReLUs, and an activation within rounding of zero is
on in one implementation and off in the other (``relu_masks_that_differ_at_x`` counts them at the output layer): each
moves a weight gradient by one pixel's worth and a whole row of the volume cotangent, so the comparison is a plausibility
figure -- the kernels are held to float64 by tests/test_gpu_motion_grad.py."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import scflow_amd  # noqa: E402
from scflow_amd import ops  # noqa: E402

dev = 'cuda:0'
COPY_RATE = 6.29e12


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
T, FEAT, C, R_, L = 8, (32, 32), 256, 4, 4
h, w = FEAT
D = 2 * R_ + 1
K = L * D * D
dec = scflow_amd.build_refiner(scflow_amd.scflow_model_cfg(iters=T)).decoder
enc = dec.encoder
g = torch.Generator().manual_seed(0)
for name, prm in enc.named_parameters():
    prm.data.copy_(torch.randn(prm.shape, generator=g) * (prm[0].numel() ** -0.5 if prm.dim() > 1 else 0.1))
dec = dec.to(dev)
PARAMS = dict(enc.named_parameters())
NAMES = list(enc.param_names())
gd = torch.Generator(dev).manual_seed(1)
R = lambda *s: torch.randn(s, device=dev, generator=gd)       # noqa: E731
E = lambda *s: torch.empty(s, device=dev)                      # noqa: E731
M = T * n

tiled = ops.pyramid_layout(h, w, R_, L)
pyramid = ops.corr_build(R(n, C, h, w), R(n, C, h, w), L, tiled_levels=tiled)
flow_lr = (R(T, n, 2, h, w) * 3).contiguous()
x = E(T, n, 128, h, w)
for t in range(T):
    enc(ops.corr_lookup(pyramid, flow_lr[t], R_, tiled_levels=tiled), flow_lr[t], out=x[t])
saved = dict(x=x, flow_lr=flow_lr, pyramid=pyramid, tiled=tiled)
cots = [R(n, 128, h, w) for _ in range(T)]
level0 = ops.untile_level(pyramid[0], h, w) if tiled & 1 else pyramid[0]


def hip_stage():
    return dec.motion_backward(saved, cots)


def hip_recompute():
    corr, c1, f1, cf = E(T, n, K, h, w), E(T, n, 256, h, w), E(T, n, 128, h, w), E(T, n, 256, h, w)
    for t in range(T):
        ops.corr_lookup(pyramid, flow_lr[t], R_, out=corr[t], tiled_levels=tiled)
        enc.branches(corr[t], x[t][:, 126:], cf[t], c1=c1[t], f1=f1[t])
    return corr


ys, xs = torch.meshgrid(torch.arange(h, device=dev, dtype=torch.float32), torch.arange(w, device=dev, dtype=torch.float32), indexing='ij')
OFF = torch.arange(D, device=dev, dtype=torch.float32) - R_


def torch_graph():
    prm = {k: PARAMS[k].detach().requires_grad_() for k in NAMES}
    conv = lambda v, k: torch.relu(F.conv2d(v, prm[f'{k}.conv.weight'], prm[f'{k}.conv.bias'],     # noqa: E731
                                            padding=prm[f'{k}.conv.weight'].shape[2] // 2))
    leaf = level0.detach().clone().requires_grad_()
    pyr = [leaf]
    for _ in range(L - 1):
        pyr.append(F.avg_pool2d(pyr[-1], 2, 2))
    total, outs = 0., []
    for t in range(T):
        cx, cy = (xs[None] + flow_lr[t, :, 0]).reshape(-1), (ys[None] + flow_lr[t, :, 1]).reshape(-1)
        per = []
        for l, lv in enumerate(pyr):
            lh, lw = lv.shape[-2:]
            gx = 2.0 * (cx[:, None] / 2 ** l + OFF[None, :]) / max(lw - 1, 1) - 1.0
            gy = 2.0 * (cy[:, None] / 2 ** l + OFF[None, :]) / max(lh - 1, 1) - 1.0
            grid = torch.stack([gx[:, :, None].expand(-1, D, D), gy[:, None, :].expand(-1, D, D)], -1)
            per.append(F.grid_sample(lv, grid, mode='bilinear', padding_mode='zeros', align_corners=True).reshape(-1, D * D))
        corr = torch.cat(per, 1).reshape(n, h, w, K).permute(0, 3, 1, 2)
        fl = flow_lr[t]
        cf = torch.cat([conv(conv(corr, 'corr_net.0'), 'corr_net.1'), conv(conv(fl, 'flow_net.0'), 'flow_net.1')], 1)
        outs.append(conv(cf, 'out_net.0'))
        total = total + (torch.cat([outs[-1], fl], 1) * cots[t]).sum()
    return total, (leaf, prm, outs)


def torch_autograd():
    total, leaves = torch_graph()
    total.backward()
    return leaves


# ---- the launches alone, at the shapes the stage gives them, on operands computed outside the window
g_corr, corr_s = R(T, n, K, h, w), R(M, K, h, w)
g_vol = E(n * h * w, h, w)
u126, cf_s, g_cf, c1_s, g_c1, f1_s, g_f1, fl_s = R(M, 126, h, w), R(M, 256, h, w), R(M, 256, h, w), R(M, 256, h, w), R(M, 256, h, w), R(M, 128, h, w), R(M, 128, h, w), R(M, 2, h, w)
W_ = lambda k: PARAMS[f'{k}.conv.weight'].detach()             # noqa: E731
convs = [m_.conv for m_ in (enc.out_net[0], enc.corr_net[1], enc.corr_net[0], enc.flow_net[1], enc.flow_net[0])]
ws = E(max(ops.conv_s1_wgrad_workspace(M, cv.out_channels, cv.in_channels, h, w, *cv.kernel_size) for cv in convs))
scratch = E(max(cv.weight.numel() for cv in convs))
o256, o324, o128, o2 = E(M, 256, h, w), E(M, K, h, w), E(M, 128, h, w), E(M, 2, h, w)
LAUNCHES = {
    'lookup_grad': lambda: ops.corr_lookup_grad(g_corr, flow_lr, None, R_, L, out=g_vol),
    'lookup_forward_T': lambda: [ops.corr_lookup(pyramid, flow_lr[t], R_, out=o324.view(T, n, K, h, w)[t], tiled_levels=tiled) for t in range(T)],
    'recompute': hip_recompute,
    'wgrad_out': lambda: ops.conv_s1_wgrad(u126, cf_s, (3, 3), workspace=ws),
    'dgrad_out': lambda: ops.conv_s1_dgrad(u126, W_('out_net.0'), a=cf_s, act=ops.ACT_RELU, out=o256, w_scratch=scratch),
    'wgrad_corr1': lambda: ops.conv_s1_wgrad(g_cf[:, :192], c1_s, (3, 3), workspace=ws),
    'dgrad_corr1': lambda: ops.conv_s1_dgrad(g_cf[:, :192], W_('corr_net.1'), a=c1_s, act=ops.ACT_RELU, out=o256, w_scratch=scratch),
    'wgrad_corr0': lambda: ops.conv_s1_wgrad(g_c1, corr_s, (1, 1), workspace=ws),
    'dgrad_corr0': lambda: ops.conv_s1_dgrad(g_c1, W_('corr_net.0'), out=o324, w_scratch=scratch),
    'wgrad_flow1': lambda: ops.conv_s1_wgrad(g_cf[:, 192:], f1_s, (3, 3), workspace=ws),
    'dgrad_flow1': lambda: ops.conv_s1_dgrad(g_cf[:, 192:], W_('flow_net.1'), a=f1_s, act=ops.ACT_RELU, out=o128, w_scratch=scratch),
    'wgrad_flow0': lambda: ops.conv_s1_wgrad(g_f1, fl_s, (7, 7), workspace=ws),
    'dgrad_flow0': lambda: ops.conv_s1_dgrad(g_f1, W_('flow_net.0'), add=fl_s, out=o2),
}

res = dict(batch=n, iters=T, feat_size=list(FEAT), samples=M, radius=R_, levels=L, tiled_levels=tiled)
columns = {'hip_us': (hip_stage, 1, None)}
try:
    torch_autograd()
    torch.cuda.synchronize()
    columns['torch_us'] = (torch_autograd, 1, None)
    columns['torch_backward_us'] = (lambda total, leaves: total.backward(), 1, torch_graph)
except Exception as exc:                                       # torch's backward cannot run here
    res['torch_error'] = f'{type(exc).__name__}: {exc}'[:200]
res.update(alternate(columns, n=7))
res['launch_us'] = alternate({k: (fn, 3, None) for k, fn in LAUNCHES.items()}, n=7)
med = lambda k: res['launch_us'][k]['median']                  # noqa: E731
floor = 4.0 * (g_corr.numel() + g_vol.numel()) / COPY_RATE * 1e6
res['lookup_grad_floor_us'] = round(floor, 1)
res['lookup_grad_floor_fraction'] = round(floor / med('lookup_grad'), 4)
res['lookup_grad_gbytes_per_s'] = round(4.0 * (g_corr.numel() + g_vol.numel()) / (med('lookup_grad') * 1e-6) * 1e-9, 1)
res['recompute_share'] = round(med('recompute') / res['hip_us']['median'], 3)
res['lookup_grad_share'] = round(med('lookup_grad') / res['hip_us']['median'], 3)
res['conv_grad_share'] = round(sum(med(k) for k in LAUNCHES if k[:5] in ('wgrad', 'dgrad')) / res['hip_us']['median'], 3)
if 'torch_us' in res:
    res['beats_torch_autograd'] = res['hip_us']['median'] < res['torch_us']['median']
    res['beats_torch_backward_alone'] = res['hip_us']['median'] < res['torch_backward_us']['median']
    (vol, g_fl, grads), (leaf, prm, outs) = hip_stage(), torch_autograd()
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))   # noqa: E731
    res['torch_vs_hip_rel_params'] = max(rel(grads['encoder.' + k], prm[k].grad) for k in NAMES)
    res['torch_vs_hip_rel_volume'] = rel(vol, leaf.grad.reshape(vol.shape))
    # a ReLU whose input is within rounding of zero is on in one implementation and off in the other: each such element
    # moves one pixel's worth of a weight gradient and one query's whole row of the volume cotangent
    res['relu_masks_that_differ_at_x'] = int(sum(((x[t][:, :126] > 0) != (outs[t] > 0)).sum() for t in range(T)))
    res['torch_vs_hip_rel_x_forward'] = max(rel(x[t][:, :126], outs[t].detach()) for t in range(T))
print(json.dumps(res))
