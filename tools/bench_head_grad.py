"""Micro-benchmark of the decoder's head / encoder backward (``SCFlowDecoder.heads_backward``: ``scf_conv_s1_wgrad``,
``scf_conv_s1_dgrad``, ``scf_act_grad``) at batch 32, 8 iterations, 32 x 32 maps (M = 256 stacked samples through every
launch), random weights, inputs and cotangents.  Device events bracket a window of calls; every shape is warmed up first;
the columns alternate inside one run.
    python tools/bench_head_grad.py [N]   -> one JSON line
``hip_us`` is ``heads_backward`` from what the forward saved: the recomputation of ``heads``, ``d1``, ``m1`` by the forward's
own launches (``recompute_us`` times it alone), the stacking copies, and the backward launches with their combine
launches.  ``launch_us`` times each backward launch alone; ``mfma_fraction`` = executed flops / time / the 157.3 TF/s fp32
MFMA peak for the wide layers, ``gbytes_per_s`` = compulsory bytes (every operand once) / time for the thin ones.
``torch_us`` is torch autograd on the same GPU of the same seven convolutions in plain fp32 torch, forward + backward over
the 8 iterations one by one; ``torch_backward_us`` times its ``backward()`` alone on a graph built outside the window.
``hidden_dgrad_as_conv2d_us``: the hidden layer's input gradient computed as ``ops.conv2d`` on the flipped, transposed
weight (the forward's Winograd route), for comparison only: nothing in the product takes that route.  The events bracket
the Python calls, so every HIP figure includes the binding's host path and allocations.  The gradients of the two
implementations are compared at the end."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import scflow_amd  # noqa: E402
from scflow_amd import ops  # noqa: E402
from scflow_amd.ops import ACT_NONE, ACT_RELU, ACT_SIGMOID  # noqa: E402
from scflow_amd.registry import DECODERS, build_from_cfg  # noqa: E402

dev = 'cuda:0'
MFMA_PEAK = 157.3e12


def window(fn, inner, args=()):
    s = torch.cuda.Event(enable_timing=True); e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(inner):
        fn(*args)
    e.record()
    return s, e


def alternate(columns, n=9):
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
T, FEAT = 8, (32, 32)
h, w = FEAT
dec = build_from_cfg(dict(scflow_amd.scflow_model_cfg()['decoder'], act_cfg=dict(type='ReLU')), DECODERS)
g = torch.Generator().manual_seed(0)
NAMES = [f'{m}.{p}' for m in ('flow_pred.layers.0.conv', 'flow_pred.predict_layer', 'mask_pred.layers.0.conv',
                              'mask_pred.predict_layer', 'delta_flow_encoder.0.conv', 'delta_flow_encoder.1.conv',
                              'mask_encoder.0.conv', 'mask_encoder.1.conv') for p in ('weight', 'bias')]
for name, prm in dec.named_parameters():
    if name in NAMES:
        prm.data.copy_(torch.randn(prm.shape, generator=g) * (prm[0].numel() ** -0.5 if prm.dim() > 1 else 0.1))
dec = dec.to(dev)
PARAMS = dict(dec.named_parameters())
gd = torch.Generator(dev).manual_seed(1)
R = lambda *s: torch.randn(s, device=dev, generator=gd)       # noqa: E731
M = T * n
fp, mp, de, me = dec.flow_pred, dec.mask_pred, dec.delta_flow_encoder, dec.mask_encoder


def recompute(hv, d_flow, mask, heads, d1, m1):
    for t in range(T):
        ops.conv2d(dec.packed, hv[t], out=heads[t], act=ACT_RELU)
        de[0](d_flow[t], out=d1[t])
        me[0](mask[t], out=m1[t])


E = lambda *s: torch.empty(s, device=dev)                      # noqa: E731
saved = dict(hv=torch.tanh(R(T, n, 128, h, w)), dm=E(T, n, 96, h, w), d_flow=E(T, n, 2, h, w), mask=E(T, n, 1, h, w))
heads, d1, m1 = E(T, n, 512, h, w), E(T, n, 128, h, w), E(T, n, 64, h, w)
for t in range(T):
    ops.conv2d(dec.packed, saved['hv'][t], out=heads[t], act=ACT_RELU)
    saved['d_flow'][t].copy_(fp.predict(heads[t][:, :256]))
    saved['mask'][t].copy_(mp.predict(heads[t][:, 256:], act=ACT_SIGMOID))
recompute(saved['hv'], saved['d_flow'], saved['mask'], heads, d1, m1)
for t in range(T):
    de[1](d1[t], out=saved['dm'][t][:, :64])
    me[1](m1[t], out=saved['dm'][t][:, 64:])
cots = [[R(n, c, h, w) for _ in range(T)] for c in (128, 96, 2, 1)]


def hip_backward():
    return dec.heads_backward(saved, *cots)


def torch_graph():
    prm = {k: PARAMS[k].detach().requires_grad_() for k in NAMES}
    conv = lambda x, k: F.conv2d(x, prm[f'{k}.weight'], prm[f'{k}.bias'], padding=prm[f'{k}.weight'].shape[2] // 2)   # noqa: E731
    hvs = [saved['hv'][t].detach().requires_grad_() for t in range(T)]
    total = 0.
    for t in range(T):
        hd = torch.relu(torch.cat([conv(hvs[t], 'flow_pred.layers.0.conv'), conv(hvs[t], 'mask_pred.layers.0.conv')], 1))
        d_flow = conv(hd[:, :256], 'flow_pred.predict_layer')
        mask = torch.sigmoid(conv(hd[:, 256:], 'mask_pred.predict_layer'))
        df = torch.relu(conv(torch.relu(conv(d_flow, 'delta_flow_encoder.0.conv')), 'delta_flow_encoder.1.conv'))
        mf = torch.relu(conv(torch.relu(conv(mask, 'mask_encoder.0.conv')), 'mask_encoder.1.conv'))
        total = total + (hvs[t] * cots[0][t]).sum() + (torch.cat([df, mf], 1) * cots[1][t]).sum() + \
            (d_flow * cots[2][t]).sum() + (mask * cots[3][t]).sum()
    return total, (hvs, prm)


def torch_autograd():
    total, leaves = torch_graph()
    total.backward()
    return leaves


# ---- the launches alone, on operands computed outside the window
V = lambda t: t.view(M, *t.shape[2:])                          # noqa: E731
hv_, dm_, df_, mk_, heads_, d1_, m1_ = (V(t) for t in (saved['hv'], saved['dm'], saved['d_flow'], saved['mask'], heads, d1, m1))
S = lambda c: torch.stack(c).view(M, *c[0].shape[1:])          # noqa: E731
g_hv, g_dm, g_df, g_mk = (S(c) for c in cots)
u = ops.act_grad(g_dm, dm_, ACT_RELU)
g_d1, g_m1, g_heads = R(M, 128, h, w), R(M, 64, h, w), R(M, 512, h, w)
w_hidden = torch.cat([fp.layers[0].conv.weight, mp.layers[0].conv.weight], 0).detach()
shapes = [(64, 128, 3), (32, 64, 3), (128, 2, 7), (64, 1, 3), (2, 256, 3), (1, 256, 1), (512, 128, 3)]
ws = E(max(ops.conv_s1_wgrad_workspace(M, co, ci, h, w, k, k) for co, ci, k in shapes))
scratch = E(w_hidden.numel())
o = {c: E(M, c, h, w) for c in (128, 64, 2, 1, 512)}
W = lambda k: PARAMS[f'{k}.weight']                            # noqa: E731
LAUNCHES = {
    'act_grad_dm': lambda: ops.act_grad(g_dm, dm_, ACT_RELU, out=u),
    'wgrad_denc1': lambda: ops.conv_s1_wgrad(u[:, :64], d1_, 3, workspace=ws),
    'dgrad_denc1': lambda: ops.conv_s1_dgrad(u[:, :64], W('delta_flow_encoder.1.conv'), a=d1_, act=ACT_RELU, out=o[128]),
    'wgrad_menc1': lambda: ops.conv_s1_wgrad(u[:, 64:], m1_, 3, workspace=ws),
    'dgrad_menc1': lambda: ops.conv_s1_dgrad(u[:, 64:], W('mask_encoder.1.conv'), a=m1_, act=ACT_RELU, out=o[64]),
    'wgrad_denc0': lambda: ops.conv_s1_wgrad(g_d1, df_, 7, workspace=ws),
    'dgrad_denc0': lambda: ops.conv_s1_dgrad(g_d1, W('delta_flow_encoder.0.conv'), add=g_df, out=o[2]),
    'wgrad_menc0': lambda: ops.conv_s1_wgrad(g_m1, mk_, 3, workspace=ws),
    'dgrad_menc0': lambda: ops.conv_s1_dgrad(g_m1, W('mask_encoder.0.conv'), add=g_mk, a=mk_, act=ACT_SIGMOID, out=o[1]),
    'wgrad_fpred': lambda: ops.conv_s1_wgrad(g_df, heads_[:, :256], 3, workspace=ws),
    'wgrad_mpred': lambda: ops.conv_s1_wgrad(g_mk, heads_[:, 256:], 1, workspace=ws),
    'dgrad_fpred': lambda: ops.conv_s1_dgrad(g_df, W('flow_pred.predict_layer'), a=heads_[:, :256], act=ACT_RELU, out=o[512][:, :256]),
    'dgrad_mpred': lambda: ops.conv_s1_dgrad(g_mk, W('mask_pred.predict_layer'), a=heads_[:, 256:], act=ACT_RELU, out=o[512][:, 256:]),
    'wgrad_hidden': lambda: ops.conv_s1_wgrad(g_heads, hv_, 3, workspace=ws),
    'dgrad_hidden': lambda: ops.conv_s1_dgrad(g_heads, w_hidden, add=g_hv, out=o[128], w_scratch=scratch),
    'recompute': lambda: recompute(saved['hv'], saved['d_flow'], saved['mask'], heads, d1, m1),
}
px = M * h * w
FLOPS = {f'{k}_{name}': 2.0 * px * kk * co * ci for name, (co, ci, kk) in
         dict(denc1=(64, 128, 9), menc1=(32, 64, 9), hidden=(512, 128, 9)).items() for k in ('wgrad', 'dgrad')}
BYTES = {f'{k}_{name}': 4.0 * px * (co + ci * (1 if k == 'wgrad' else extra))
         for name, (co, ci, extra) in dict(denc0=(128, 2, 2), menc0=(64, 1, 3), fpred=(2, 256, 2), mpred=(1, 256, 2)).items()
         for k in ('wgrad', 'dgrad')}           # dgrad: g, gx and what its epilogue reads (add and / or a)

# the hidden layer's dgrad as a forward convolution of the flipped, transposed weight
pc_t = ops.PackedConv.from_weight(w_hidden.flip(2, 3).transpose(0, 1).contiguous(), None, 1, 1)
LAUNCHES['hidden_dgrad_as_conv2d'] = lambda: ops.conv2d(pc_t, g_heads, out=o[128])

res = dict(batch=n, iters=T, feat_size=list(FEAT), samples=M)
columns = {'hip_us': (hip_backward, 2, None)}
try:
    torch_autograd()
    torch.cuda.synchronize()
    columns['torch_us'] = (torch_autograd, 1, None)
    columns['torch_backward_us'] = (lambda total, leaves: total.backward(), 1, torch_graph)
except Exception as exc:                                       # torch's convolution backward cannot run here
    res['torch_error'] = f'{type(exc).__name__}: {exc}'[:200]
res.update(alternate(columns))
res['launch_us'] = alternate({k: (fn, 3, None) for k, fn in LAUNCHES.items()}, n=7)
res['mfma_fraction'] = {k: round(f / (res['launch_us'][k]['median'] * 1e-6) / MFMA_PEAK, 4) for k, f in FLOPS.items()}
res['gbytes_per_s'] = {k: round(b / (res['launch_us'][k]['median'] * 1e-6) * 1e-9, 1) for k, b in BYTES.items()}
res['gflop'] = round(sum(FLOPS.values()) * 1e-9, 1)
res['recompute_share'] = round(res['launch_us']['recompute']['median'] / res['hip_us']['median'], 3)
res['stacked_buffers_mb'] = {k: round(4e-6 * M * c * h * w, 1) for k, c in dict(heads=512, g_heads=512, d1=128, m1=64, g_d1=128, g_m1=64).items()}
res['hidden_dgrad_as_conv2d_us'] = res['launch_us'].pop('hidden_dgrad_as_conv2d')
if 'torch_us' in res:
    res['beats_torch_autograd'] = res['hip_us']['median'] < res['torch_us']['median']
    res['beats_torch_backward_alone'] = res['hip_us']['median'] < res['torch_backward_us']['median']
    (g_h, g_dft, g_ml, grads), (hvs, prm) = hip_backward(), torch_autograd()
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))   # noqa: E731
    res['torch_vs_hip_rel_params'] = max(rel(grads[k], prm[k].grad) for k in NAMES)
    res['torch_vs_hip_rel_hidden'] = max(rel(a, x.grad) for a, x in zip(g_h, hvs))
print(json.dumps(res))
