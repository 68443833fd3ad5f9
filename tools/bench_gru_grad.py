"""Micro-benchmark of the GRU backward (``ConvGRU.backward``: ``scf_gru_gate_grad_q`` / ``_r``, ``scf_conv_s1_dgrad``,
``scf_conv_s1_wgrad``) at batch 32, 8 iterations, 32 x 32 maps, ``net_type='SeqConv'``, random weights, inputs and
cotangents.  Device events bracket a window of calls; every shape is warmed up first; the columns alternate inside one run.
    python tools/bench_gru_grad.py [N]   -> one JSON line
``hip_us`` is ``ConvGRU.backward`` from what the forward saved: the recomputation of the gates by the forward's own
launches (``recompute_us`` times it alone), the scan, the context launches and the weight gradients.  ``launch_us`` times
each kind of launch alone (one launch, at the shape the stage gives it): ``dgrad_*_hx`` are the scan's per-iteration
launches over the [h | x'] columns, ``dgrad_*_full`` the same launches over all 384 columns (the unhoisted form, for
comparison only: nothing in the product takes it), ``dgrad_*_c`` the once-per-pass context launches; ``hoisted_dgrad_us``
/ ``unhoisted_dgrad_us`` add them up over the stage (T iterations, both passes).  ``mfma_fraction`` = executed flops / time /
the 157.3 TF/s fp32 MFMA peak, ``gbytes_per_s`` = compulsory bytes (every operand once) / time for the gate kernels.
``torch_us`` is torch autograd on the same GPU of a plain-torch restatement of the T iterations, forward + backward;
``torch_backward_us`` times its ``backward()`` alone on a graph built outside the window.  The events bracket the Python
calls, so every HIP figure includes the binding's host path and allocations.  The gradients of the two implementations
are compared at the end."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from scflow_amd import ops  # noqa: E402
from scflow_amd.modules import ConvGRU  # noqa: E402

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
T, FEAT, HC, CC, CX = 8, (32, 32), 128, 128, 128
h, w = FEAT
gru = ConvGRU(HC, CC + CX, 'SeqConv')
g = torch.Generator().manual_seed(0)
for name, prm in gru.named_parameters():
    prm.data.copy_(torch.randn(prm.shape, generator=g) * (prm[0].numel() ** -0.5 if prm.dim() > 1 else 0.1))
gru = gru.to(dev)
PARAMS = dict(gru.named_parameters())
NAMES = list(gru.param_names())
gd = torch.Generator(dev).manual_seed(1)
R = lambda *s: torch.randn(s, device=dev, generator=gd)       # noqa: E731
E = lambda *s: torch.empty(s, device=dev)                      # noqa: E731
M = T * n

h0, c, x = torch.tanh(R(n, HC, h, w)), torch.relu(R(n, CC, h, w)), R(T, n, CX, h, w)
hx = torch.cat([h0, c, x[0]], 1).contiguous()
ctx = gru.context_terms(hx[:, HC:HC + CC])
hv = E(T, n, HC, h, w)
for t in range(T):
    ops.copy_channels(x[t], hx[:, HC + CC:])
    hv[t].copy_(gru.forward_inplace(hx, ctx, CC))
saved = dict(h0=h0, c=c, x=x, hv=hv)
cots = [R(n, HC, h, w) for _ in range(T)]


def hip_backward():
    return gru.backward(saved, cots)


def torch_graph():
    prm = {k: PARAMS[k].detach().requires_grad_() for k in NAMES}
    conv = lambda v, k: F.conv2d(v, prm[f'{k}.weight'], prm[f'{k}.bias'],     # noqa: E731
                                 padding=tuple(s // 2 for s in prm[f'{k}.weight'].shape[2:]))
    leaves = dict(h0=h0.detach().requires_grad_(), c=c.detach().requires_grad_(), x=x.detach().requires_grad_())
    hh, total = leaves['h0'], 0.
    for t in range(T):
        xt = torch.cat([leaves['c'], leaves['x'][t]], 1)
        for p in range(2):
            hxx = torch.cat([hh, xt], 1)
            z, r = torch.sigmoid(conv(hxx, f'conv_z.{p}.conv')), torch.sigmoid(conv(hxx, f'conv_r.{p}.conv'))
            q = torch.tanh(conv(torch.cat([r * hh, xt], 1), f'conv_q.{p}.conv'))
            hh = (1 - z) * hh + z * q
        total = total + (hh * cots[t]).sum()
    return total, (leaves, prm)


def torch_autograd():
    total, leaves = torch_graph()
    total.backward()
    return leaves


# ---- the launches alone, at the shapes the stage gives them, on operands computed outside the window
u_q, u_zr, s_q, s_zr = R(n, HC, h, w), R(n, 2 * HC, h, w), R(n, HC, h, w), R(n, 2 * HC, h, w)
U_q, U_zr, H_in, X = R(M, HC, h, w), R(M, 2 * HC, h, w), R(M, HC, h, w), x.view(M, CX, h, w)
g_in, z_, q_, r_, hin = R(n, HC, h, w), torch.sigmoid(R(n, HC, h, w)), torch.tanh(R(n, HC, h, w)), torch.sigmoid(R(n, HC, h, w)), torch.tanh(R(n, HC, h, w))
wz, wr, wq = (PARAMS[f'conv_{k}.0.conv.weight'].detach() for k in 'zrq')          # the 1 x 5 pass; the 5 x 1 pass has the same counts
sel = lambda wt: torch.cat([wt[:, :HC], wt[:, HC + CC:]], 1).contiguous()          # noqa: E731
w_zr = torch.cat([wz, wr], 0)
w_zr_hx, w_q_hx, w_zr_c, w_q_c = sel(w_zr), sel(wq), w_zr[:, HC:HC + CC].contiguous(), wq[:, HC:HC + CC].contiguous()
scratch = E(w_zr.numel())
o256, o384, o128, add256 = E(n, HC + CX, h, w), E(n, HC + CC + CX, h, w), E(n, CC, h, w), R(n, HC + CX, h, w)
o_uq, o_uzr = E(n, HC, h, w), E(n, 2 * HC, h, w)
shapes = [(M, 2 * HC, HC), (M, 2 * HC, CX), (n, 2 * HC, CC), (M, HC, HC)]
ws = E(max(ops.conv_s1_wgrad_workspace(m_, co, ci, h, w, 1, 5) for m_, co, ci in shapes))
LAUNCHES = {
    'gate_grad_q': lambda: ops.gru_gate_grad_q(g_in, hin, z_, q_, u_q=o_uq, u_z=o_uzr[:, :HC], sum_q=s_q, sum_z=s_zr[:, :HC], first=False),
    'gate_grad_r': lambda: ops.gru_gate_grad_r(g_in, z_, o256[:, :HC], hin, r_, u_r=o_uzr[:, HC:], sum_r=s_zr[:, HC:], first=False),
    'dgrad_q_hx': lambda: ops.conv_s1_dgrad(u_q, w_q_hx, out=o256, w_scratch=scratch),
    'dgrad_zr_hx': lambda: ops.conv_s1_dgrad(u_zr, w_zr_hx, add=add256, out=o256, w_scratch=scratch),
    'dgrad_q_full': lambda: ops.conv_s1_dgrad(u_q, wq, out=o384, w_scratch=scratch),
    'dgrad_zr_full': lambda: ops.conv_s1_dgrad(u_zr, w_zr, out=o384, w_scratch=scratch),
    'dgrad_q_c': lambda: ops.conv_s1_dgrad(s_q, w_q_c, out=o128, w_scratch=scratch),
    'dgrad_zr_c': lambda: ops.conv_s1_dgrad(s_zr, w_zr_c, out=o128, w_scratch=scratch),
    'wgrad_zr_h': lambda: ops.conv_s1_wgrad(U_zr, H_in, (1, 5), workspace=ws),
    'wgrad_zr_x': lambda: ops.conv_s1_wgrad(U_zr, X, (1, 5), bias=False, workspace=ws),
    'wgrad_zr_c': lambda: ops.conv_s1_wgrad(s_zr, c, (1, 5), bias=False, workspace=ws),
    'wgrad_q_h': lambda: ops.conv_s1_wgrad(U_q, H_in, (1, 5), workspace=ws),
    'wgrad_q_x': lambda: ops.conv_s1_wgrad(U_q, X, (1, 5), bias=False, workspace=ws),
    'wgrad_q_c': lambda: ops.conv_s1_wgrad(s_q, c, (1, 5), bias=False, workspace=ws),
    'recompute': lambda: gru.recompute_gates(saved),
}
px, pxm = n * h * w, M * h * w
FLOPS = dict(dgrad_q_hx=2.0 * px * 5 * HC * 256, dgrad_zr_hx=2.0 * px * 5 * 256 * 256, dgrad_q_full=2.0 * px * 5 * HC * 384,
             dgrad_zr_full=2.0 * px * 5 * 256 * 384, dgrad_q_c=2.0 * px * 5 * HC * CC, dgrad_zr_c=2.0 * px * 5 * 256 * CC,
             wgrad_zr_h=2.0 * pxm * 5 * 256 * HC, wgrad_zr_x=2.0 * pxm * 5 * 256 * CX, wgrad_zr_c=2.0 * px * 5 * 256 * CC,
             wgrad_q_h=2.0 * pxm * 5 * HC * HC, wgrad_q_x=2.0 * pxm * 5 * HC * CX, wgrad_q_c=2.0 * px * 5 * HC * CC)
BYTES = dict(gate_grad_q=4.0 * px * HC * 10, gate_grad_r=4.0 * px * HC * 9)      # operands read + results written, sums included

res = dict(batch=n, iters=T, feat_size=list(FEAT), samples=M, net_type='SeqConv')
columns = {'hip_us': (hip_backward, 1, None)}
try:
    torch_autograd()
    torch.cuda.synchronize()
    columns['torch_us'] = (torch_autograd, 1, None)
    columns['torch_backward_us'] = (lambda total, leaves: total.backward(), 1, torch_graph)
except Exception as exc:                                       # torch's convolution backward cannot run here
    res['torch_error'] = f'{type(exc).__name__}: {exc}'[:200]
res.update(alternate(columns, n=7))
res['launch_us'] = alternate({k: (fn, 3, None) for k, fn in LAUNCHES.items()}, n=7)
med = lambda k: res['launch_us'][k]['median']                  # noqa: E731
res['mfma_fraction'] = {k: round(f / (med(k) * 1e-6) / MFMA_PEAK, 4) for k, f in FLOPS.items()}
res['gbytes_per_s'] = {k: round(b / (med(k) * 1e-6) * 1e-9, 1) for k, b in BYTES.items()}
res['hoisted_dgrad_us'] = round(2 * (T * (med('dgrad_q_hx') + med('dgrad_zr_hx')) + med('dgrad_q_c') + med('dgrad_zr_c')), 1)
res['unhoisted_dgrad_us'] = round(2 * T * (med('dgrad_q_full') + med('dgrad_zr_full')), 1)
res['recompute_share'] = round(med('recompute') / res['hip_us']['median'], 3)
res['scan_share'] = round(2 * T * (med('gate_grad_q') + med('gate_grad_r') + med('dgrad_q_hx') + med('dgrad_zr_hx')) / res['hip_us']['median'], 3)
res['wgrad_share'] = round(2 * sum(med(k) for k in LAUNCHES if k.startswith('wgrad')) / res['hip_us']['median'], 3)
if 'torch_us' in res:
    res['beats_torch_autograd'] = res['hip_us']['median'] < res['torch_us']['median']
    res['beats_torch_backward_alone'] = res['hip_us']['median'] < res['torch_backward_us']['median']
    (g_h0, g_c, g_x, grads), (leaves, prm) = hip_backward(), torch_autograd()
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))   # noqa: E731
    res['torch_vs_hip_rel_params'] = max(rel(grads[k], prm[k].grad) for k in NAMES)
    res['torch_vs_hip_rel_inputs'] = max([rel(g_h0, leaves['h0'].grad), rel(g_c, leaves['c'].grad)]
                                         + [rel(g_x[t], leaves['x'].grad[t]) for t in range(T)])
print(json.dumps(res))
