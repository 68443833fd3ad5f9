"""CPU: backward of the ConvGRU (gru_grad.hip, ConvGRU.backward) -- the pass backward and the reverse scan over the
iterations restated once, generically, and evaluated by two back ends: float64 with a per-element bound for any fp32
evaluation in the kernels' operation order (B64), and fp32 in that order with fma chains (B32), into which defects are
planted.  The float64 evaluation is held against float64 autograd of the restated forward; the hoisted decomposition
(context columns after the scan, on running sums) against the unhoisted one; the reference's own ConvGRU (a fixture)
against both.

The operation order is the header comment's of gru_grad.hip (each line one rounding, U = 2^-24; underflow is outside
the model, as in test_fc_host):

  grad_q   t1 = g z, dq = fma(-q, q, 1), u_q = t1 dq                      3 roundings of ONE product g z (1 - q^2):
           (b_g + gamma_3 (|g| + b_g)) |z (1 - q^2)|         (the fma rounds the exact 1 - q^2 once: no cancellation)
           d = q - h, t2 = g d, 1 - z, dz = z (1 - z), u_z = t2 dz (+ 0: exact)   5 roundings of one product:
           (b_g + gamma_5 (|g| + b_g)) |(q - h) z (1 - z)|
  grad_r   t3 = g_rh h, 1 - r, dr = r (1 - r), u_r = t3 dr (+ 0)         4 roundings: (b + gamma_4 (|g_rh| + b)) |h r (1 - r)|
           a = 1 - z, b = g a, g_h_direct = fma(g_rh, r, b)              two terms T1 = g (1 - z) (3 roundings), T2 = g_rh r (1):
           gamma_3 (|T1| + |T2|) + (b_g |1 - z| + b_grh |r|) (1 + gamma_3)
  sums / carry   one addition each: U (|a + b| + b_a + b_b) + b_a + b_b
  dgrad / wgrad  the bounds of tests/test_head_grad_host.py (imported), each stage's bound carried into the next
The gates z, r, q, r h and the states h are taken as given: they are what the backward recomputes with the forward's own
launches, and tests/test_gpu_gru_grad.py hands the GPU's to the restatement.
"""
import os
import re

import numpy as np
import pytest
import torch

from test_stream_ops_host import f64, measured, worst_ratio  # noqa: E402
from test_fc_host import U, gamma  # noqa: E402
from test_conv_grad_host import fma  # noqa: E402
import test_head_grad_host as hg  # noqa: E402
from test_head_grad_host import dgrad_ref, wgrad_ref, dgrad_fp32, wgrad_fp32, dgrad_sum  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, 'scflow_amd', 'csrc', 'gru_grad.hip')).read()
F = torch.nn.functional
KERNELS = {'SeqConv': [(1, 5), (5, 1)], 'Conv': [(3, 3)]}
NETS = ['SeqConv', 'Conv']
# the operation order the kernels' header states; the back ends below restate it
ORDER = ('t1 = g * z            dq = fma(-q, q, 1)       u_q = t1 * dq',
         'd  = q - h            t2 = g * d               dz  = z * (1 - z)       u_z = t2 * dz + 0',
         't3 = g_rh * h         dr = r * (1 - r)         u_r = t3 * dr + 0',
         'a  = 1 - z            b  = g * a               g_h_direct = fma(g_rh, r, b)',
         'sum = first ? u : sum + u',
         'out = add ? src + add : src')
GATE_Q_ROUNDINGS, GATE_Z_ROUNDINGS, GATE_R_ROUNDINGS, GATE_H_ROUNDINGS = 3, 5, 4, 3


def param_names(net):
    return [f'conv_{g}.{p}.conv.{k}' for p in range(len(KERNELS[net])) for g in 'zrq' for k in ('weight', 'bias')]


# ============================================================================================================ back ends
class V:
    """float64 value and a bound on |an fp32 evaluation - value|"""

    def __init__(self, v, b=0.0):
        self.v = f64(v)
        self.b = np.broadcast_to(np.asarray(b, dtype=np.float64), self.v.shape) + 0.0


class B64:
    """float64 with bounds"""

    def lift(self, t):
        return V(t)

    def w(self, t):
        return f64(t)

    def zeros(self, like, c):
        return V(np.zeros((like.v.shape[0], c) + like.v.shape[2:]))

    def cat(self, vs, axis=1):
        return V(np.concatenate([a.v for a in vs], axis), np.concatenate([a.b for a in vs], axis))

    def sl(self, a, s, axis=1):
        return V(a.v[:, s], a.b[:, s]) if axis == 1 else V(a.v[s], a.b[s])

    def gate_q(self, g, h, z, q, defect=None):
        h, z, q = f64(h), f64(z), f64(q)
        fq = z * ((1 - q) if defect == 'one_minus_q' else (1 - q * q))
        fz = (q - h) * z * (1 - z)
        bound = lambda f, k: (g.b + gamma(k) * (np.abs(g.v) + g.b)) * np.abs(f)       # noqa: E731
        return V(g.v * fq, bound(fq, GATE_Q_ROUNDINGS)), V(g.v * fz, bound(fz, GATE_Z_ROUNDINGS))

    def gate_r(self, g, z, g_rh, h, r, defect=None):
        z, h, r = f64(z), f64(h), f64(r)
        fr = h if defect == 'r_factor_dropped' else h * r * (1 - r)
        u_r = V(g_rh.v * fr, (g_rh.b + gamma(GATE_R_ROUNDINGS) * (np.abs(g_rh.v) + g_rh.b)) * np.abs(fr))
        t1, t2 = g.v * (1 - z), (0.0 if defect == 'grh_r_missing' else g_rh.v * r)
        gm = gamma(GATE_H_ROUNDINGS)
        return u_r, V(t1 + t2, gm * (np.abs(t1) + np.abs(t2)) + (g.b * np.abs(1 - z) + g_rh.b * np.abs(r)) * (1 + gm))

    def add(self, a, b):
        v, e = a.v + b.v, a.b + b.b
        return V(v, e + U * (np.abs(v) + e))

    def dgrad(self, u, w, add=None):
        return V(*dgrad_ref(u.v, u.b, w, None if add is None else add.v, 0.0 if add is None else add.b))

    def wgrad(self, u, x, k, prev_w=None, prev_b=None):
        dw, bw, db, bb = wgrad_ref(u.v, u.b, x.v, *k, xb=x.b, prev=prev_w, prev_b=prev_b)
        return V(dw, bw), V(db, bb)


class B32:
    """fp32 in the kernels' order"""

    def lift(self, t):
        return t.float()

    def w(self, t):
        return t.float().contiguous()

    def zeros(self, like, c):
        return torch.zeros((like.shape[0], c) + tuple(like.shape[2:]))

    def cat(self, vs, axis=1):
        return torch.cat(vs, axis)

    def sl(self, a, s, axis=1):
        return a[:, s] if axis == 1 else a[s]

    def gate_q(self, g, h, z, q, defect=None):
        h, z, q = h.float(), z.float(), q.float()
        t1 = g * z
        dq = (1.0 - q) if defect == 'one_minus_q' else fma(-q, q, torch.ones_like(q))
        d = q - h
        t2 = g * d
        dz = z * (1.0 - z)
        return t1 * dq, t2 * dz + 0.0

    def gate_r(self, g, z, g_rh, h, r, defect=None):
        z, h, r = z.float(), h.float(), r.float()
        t3 = g_rh * h
        dr = r * (1.0 - r)
        u_r = t3 if defect == 'r_factor_dropped' else t3 * dr + 0.0
        a = 1.0 - z
        b = g * a
        return u_r, (b if defect == 'grh_r_missing' else fma(g_rh, r, b))

    def add(self, a, b):
        return a + b

    def dgrad(self, u, w, add=None):
        return dgrad_fp32(u, w, add)

    def wgrad(self, u, x, k, prev_w=None, prev_b=None):
        if prev_w is None:
            return wgrad_fp32(u, x, *k)
        dw, db = wgrad_fp32(u, x, *k, prev_w.float(), torch.zeros(u.shape[1]) if prev_b is None else prev_b.float())
        return dw, db


def val(a):
    return a.v if isinstance(a, V) else f64(a)


# ======================================================================================= the scan, once for both back ends
DEFECTS = ['r_factor_dropped', 'grh_r_missing', 'one_minus_q', 'zr_rows_swapped', 'passes_forward_order', 'carry_not_added',
           'context_sum_misses_iteration', 'bias_twice']


def gru_scan(be, gates, weights, c, x, g_hs, hoisted=True, defect=None, prev=None):
    """ConvGRU.backward GIVEN the gates.  ``gates``: h_in, zr, rh, q, per pass a (T, N, C, h, w) tensor; ``weights``: per pass
    dict z, r, q -> the raw (Ch, Ch + Cc + Cx, KH, KW) weight; ``c`` (N, Cc, h, w); ``x`` (T, N, Cx, h, w); ``g_hs``: T
    cotangents at hv_t; ``prev``: parameter gradients to accumulate into.  -> dict g_h0, g_c, g_x.t, the parameter
    gradients.  ``hoisted``: the shipped decomposition; False: every launch over all Ch + Cc + Cx columns, the context
    cotangent added up iteration by iteration, one wgrad per gate group."""
    P, T = len(weights), len(g_hs)
    hc, cc = gates['q'][0].shape[2], c.shape[1]
    L = be.lift
    w_zr = [torch.cat([wp['z'], wp['r']], 0) for wp in weights]
    w_q = [wp['q'] for wp in weights]
    hx_cols = lambda wt: be.w(torch.cat([wt[:, :hc], wt[:, hc + cc:]], 1))        # noqa: E731
    c_cols = lambda wt: be.w(wt[:, hc:hc + cc])                                  # noqa: E731
    u_zr, u_q = [[None] * T for _ in range(P)], [[None] * T for _ in range(P)]
    s_zr, s_q = [None] * P, [None] * P
    g_x, g_h, g_c = [None] * T, None, None
    for t in reversed(range(T)):
        g = L(g_hs[t])
        if t < T - 1 and defect != 'carry_not_added':
            g = be.add(g_h, g)
        gx = gc = None
        for p in (range(P) if defect == 'passes_forward_order' else reversed(range(P))):
            h_in, z, r, q = gates['h_in'][p][t], gates['zr'][p][t][:, :hc], gates['zr'][p][t][:, hc:], gates['q'][p][t]
            uq, uz = be.gate_q(g, h_in, z, q, defect)
            zero = be.zeros(uq, hc)
            if hoisted:
                G = be.dgrad(uq, hx_cols(w_q[p]), None if gx is None else be.cat([zero, gx]))
                g_rh, G_rest = be.sl(G, slice(0, hc)), be.sl(G, slice(hc, None))
            else:
                G = be.dgrad(uq, be.w(w_q[p]), None if gx is None else be.cat([zero, gc, gx]))
                g_rh, G_rest = be.sl(G, slice(0, hc)), be.sl(G, slice(hc, None))
            ur, ghd = be.gate_r(g, z, g_rh, h_in, r, defect)
            uzr = be.cat([ur, uz] if defect == 'zr_rows_swapped' else [uz, ur])
            O = be.dgrad(uzr, hx_cols(w_zr[p]) if hoisted else be.w(w_zr[p]), be.cat([ghd, G_rest]))
            g = be.sl(O, slice(0, hc))
            if hoisted:
                gx = be.sl(O, slice(hc, None))
            else:
                gc, gx = be.sl(O, slice(hc, hc + cc)), be.sl(O, slice(hc + cc, None))
            u_zr[p][t], u_q[p][t] = uzr, uq
            if not (defect == 'context_sum_misses_iteration' and t == 0):
                s_zr[p] = uzr if s_zr[p] is None else be.add(s_zr[p], uzr)
                s_q[p] = uq if s_q[p] is None else be.add(s_q[p], uq)
        g_h, g_x[t] = g, gx
        if not hoisted:
            g_c = gc if g_c is None else be.add(g_c, gc)
    if hoisted:
        for p in range(P):
            g_c = be.dgrad(s_zr[p], c_cols(w_zr[p]), g_c)
            g_c = be.dgrad(s_q[p], c_cols(w_q[p]), g_c)
    out = {'g_h0': g_h, 'g_c': g_c}
    out.update((f'g_x.{t}', g_x[t]) for t in range(T))
    xs, cl = be.cat([L(x[t]) for t in range(T)], 0), L(c)
    for p in range(P):
        k = tuple(w_q[p].shape[2:])
        for us, s_, state, mods in ((u_zr[p], s_zr[p], 'h_in', 'zr'), (u_q[p], s_q[p], 'rh', 'q')):
            ust, st = be.cat(us, 0), be.cat([L(gates[state][p][t]) for t in range(T)], 0)
            names = [f'conv_{m_}.{p}.conv' for m_ in mods]
            pw = None if prev is None else torch.cat([prev[f'{n_}.weight'] for n_ in names], 0)
            pb = None if prev is None else torch.cat([prev[f'{n_}.bias'] for n_ in names], 0)
            cols = lambda s: None if pw is None else pw[:, s].contiguous()      # noqa: E731
            if hoisted:
                dw_h, db = be.wgrad(ust, st, k, cols(slice(0, hc)), pb)
                dw_c, _ = be.wgrad(s_, cl, k, cols(slice(hc, hc + cc)))
                dw_x, db_x = be.wgrad(ust, xs, k, cols(slice(hc + cc, None)))
                if defect == 'bias_twice':
                    db = be.add(db, db_x)
                dw = be.cat([dw_h, dw_c, dw_x])
            else:
                dw, db = be.wgrad(ust, be.cat([st, be.cat([cl] * T, 0), xs]), k, pw, pb)
            for i, n_ in enumerate(names):
                out[f'{n_}.weight'], out[f'{n_}.bias'] = (be.sl(v, slice(i * hc, (i + 1) * hc), 0) for v in (dw, db))
    return out


# =========================================================================================== the forward, in plain torch
def gru_params(net, hc, cc, cx, seed=0, dtype=torch.float64):
    gen = torch.Generator().manual_seed(6600 + seed)
    p = {}
    for i, (kh, kw) in enumerate(KERNELS[net]):
        for g in 'zrq':
            p[f'conv_{g}.{i}.conv.weight'] = (torch.randn((hc, hc + cc + cx, kh, kw), generator=gen, dtype=torch.float64)
                                             * ((hc + cc + cx) * kh * kw) ** -0.5 * 2.0).to(dtype)
            p[f'conv_{g}.{i}.conv.bias'] = (torch.randn(hc, generator=gen, dtype=torch.float64) * 0.1).to(dtype)
    return p


def gru_forward_torch(h0, c, x, p, net):
    """raft_decoder.py:235-253 over T iterations, x_t = [c | x[t]] -> (list of h_t, the gates as ``gru_scan`` takes them,
    attached to the graph)"""
    P, T = len(KERNELS[net]), x.shape[0]
    conv = lambda v, k: F.conv2d(v, p[f'{k}.weight'], p[f'{k}.bias'], padding=tuple(s // 2 for s in p[f'{k}.weight'].shape[2:]))  # noqa: E731
    gates = dict(h_in=[[] for _ in range(P)], zr=[[] for _ in range(P)], rh=[[] for _ in range(P)], q=[[] for _ in range(P)])
    hs, h = [], h0
    for t in range(T):
        for i in range(P):
            hx = torch.cat([h, c, x[t]], 1)
            z, r = torch.sigmoid(conv(hx, f'conv_z.{i}.conv')), torch.sigmoid(conv(hx, f'conv_r.{i}.conv'))
            rh = r * h
            q = torch.tanh(conv(torch.cat([rh, c, x[t]], 1), f'conv_q.{i}.conv'))
            for key, v in (('h_in', h), ('zr', torch.cat([z, r], 1)), ('rh', rh), ('q', q)):
                gates[key][i].append(v)
            h = (1 - z) * h + z * q
        hs.append(h)
    return hs, {k: [torch.stack(v_).detach() for v_ in v] for k, v in gates.items()}


def weights_of(p, net):
    return [{g: p[f'conv_{g}.{i}.conv.weight'].detach() for g in 'zrq'} for i in range(len(KERNELS[net]))]


SMALL = dict(hc=6, cc=4, cx=5)


def scan_case(net, n, T, h, w, widths=SMALL, seed=0, dtype=torch.float64):
    gen = torch.Generator().manual_seed(8800 + seed + 3 * n + 5 * T + 7 * h + 11 * w)
    hc, cc, cx = widths['hc'], widths['cc'], widths['cx']
    R = lambda *s: torch.randn(s, generator=gen, dtype=torch.float64)        # noqa: E731
    p = gru_params(net, hc, cc, cx, seed, dtype)
    h0, c, x = torch.tanh(R(n, hc, h, w)).to(dtype), torch.relu(R(n, cc, h, w)).to(dtype), R(T, n, cx, h, w).to(dtype)
    g_hs = [R(n, hc, h, w).to(dtype) for _ in range(T)]
    return p, h0, c, x, g_hs


# ======================================================================================================== the self-checks
def test_symbols_are_declared_exported_and_bound():
    from scflow_amd import _lib, ops
    from scflow_amd.modules import ConvGRU, SCFlowDecoder
    from scflow_amd.refiner import SCFlowRefiner, _GRAD_DEPTHS
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'scflow_hip.h')).read()
    for name in ('scf_gru_gate_grad_q', 'scf_gru_gate_grad_r', 'scf_gru_carry', 'scf_gru_gate_state'):
        assert re.search(rf'\b{name}\s*\(', header), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert all(hasattr(ops, n) for n in ('gru_gate_grad_q', 'gru_gate_grad_r', 'gru_carry', 'gru_gate_state'))
    assert hasattr(ConvGRU, 'backward') and hasattr(SCFlowDecoder, 'gru_backward') and hasattr(SCFlowRefiner, 'loss_and_gru_grads')
    assert _GRAD_DEPTHS[-3:] == ('decoder_heads', 'gru', 'motion')
    for net in NETS:
        assert list(ConvGRU(8, 8, net).param_names()) == param_names(net)
        assert set(param_names(net)) == {k for k, _ in ConvGRU(8, 8, net).named_parameters()}


def test_the_header_states_the_order_the_back_ends_restate():
    flat = re.sub(r'\s+', ' ', SRC)
    for line in ORDER:
        assert re.sub(r'\s+', ' ', line) in flat, line
    # and the kernels spell it with explicit fma, contraction off
    assert '#pragma clang fp contract(off)' in SRC
    assert '__fmaf_rn(-q.v[j], q.v[j], 1.f)' in SRC and '__fmaf_rn(grh.v[j], r.v[j], b)' in SRC
    assert 'z.v[j] * (1.f - z.v[j])' in SRC and 'r.v[j] * (1.f - r.v[j])' in SRC      # scf_act_grad's a * (1.f - a)
    assert 'v * (a * (1.f - a))' in hg.SRC and 'v * __fmaf_rn(-a, a, 1.f)' in hg.SRC


def test_null_pointers_sizes_and_strides_are_refused_on_the_host():
    """the validation runs before any launch: callable without a GPU (pointers are never dereferenced)"""
    from scflow_amd import _lib
    lib = _lib.load()
    P, n = 4096, 8
    ok_q = [P, n, P, n, P, n, P, n, P, n, P, n, None, 0, None, 0, 1, 2, n, None]
    ok_r = [P, n, P, n, P, n, P, n, P, n, P, n, None, 0, 1, 2, n, None]
    ok_c = [P, n, None, 0, P, n, 0, 2, n, None]
    ok_s = [P, n, P, n, None, 0, P, n, 2, n, None]
    for fn, ok, ptrs, m_at in ((lib.scf_gru_gate_grad_q, ok_q, (0, 2, 4, 6, 8, 10), 17), (lib.scf_gru_gate_grad_r, ok_r, (0, 2, 4, 6, 8, 10), 15),
                               (lib.scf_gru_carry, ok_c, (0, 4), 7), (lib.scf_gru_gate_state, ok_s, (0, 2, 6), 8)):
        for i in ptrs:
            bad = list(ok)
            bad[i] = None
            assert fn(*bad) == -1, (fn.__name__, 'null', i)
            bad = list(ok)
            bad[i + 1] = n - 1
            assert fn(*bad) == -1, (fn.__name__, 'stride', i)
        for at, v in ((m_at, 0), (m_at, -1), (m_at + 1, 0), (m_at + 1, -5)):
            bad = list(ok)
            bad[at] = v
            assert fn(*bad) == -1, (fn.__name__, 'size', at)
    bad = list(ok_q)
    bad[12], bad[13] = P, n - 1                    # an optional operand that is present needs its stride too
    assert lib.scf_gru_gate_grad_q(*bad) == -1


@pytest.mark.parametrize('net', NETS)
@pytest.mark.parametrize('hw', [(5, 7), (2, 3)], ids=lambda v: f'{v[0]}x{v[1]}')
def test_restatement_equals_float64_autograd(net, hw):
    p, h0, c, x, g_hs = scan_case(net, 2, 3, *hw)
    pt = {k: v.clone().requires_grad_() for k, v in p.items()}
    h0t, ct, xt = h0.clone().requires_grad_(), c.clone().requires_grad_(), x.clone().requires_grad_()
    hs, gates = gru_forward_torch(h0t, ct, xt, pt, net)
    sum((g * h).sum() for g, h in zip(g_hs, hs)).backward()
    want = {k: v.grad for k, v in pt.items()}
    want.update(g_h0=h0t.grad, g_c=ct.grad)
    want.update((f'g_x.{t}', xt.grad[t]) for t in range(3))
    worst = {}
    for hoisted in (True, False):
        got = gru_scan(B64(), gates, weights_of(p, net), c, x, g_hs, hoisted=hoisted)
        assert set(got) == set(want) == set(param_names(net)) | {'g_h0', 'g_c', 'g_x.0', 'g_x.1', 'g_x.2'}
        worst[hoisted] = max(float(np.abs(val(got[k]) - f64(want[k])).max() / np.abs(f64(want[k])).max()) for k in want)
        measured(f'restated scan (hoisted={hoisted}) against float64 autograd {net} {hw}, relative', worst[hoisted])
    assert max(worst.values()) <= 1e-12


@pytest.mark.parametrize('net', NETS)
def test_hoisted_and_unhoisted_agree_in_float64(net):
    p, h0, c, x, g_hs = scan_case(net, 2, 3, 5, 7, seed=1)
    _, gates = gru_forward_torch(h0, c, x, p, net)
    a = gru_scan(B64(), gates, weights_of(p, net), c, x, g_hs, hoisted=True)
    b = gru_scan(B64(), gates, weights_of(p, net), c, x, g_hs, hoisted=False)
    worst = max(float(np.abs(a[k].v - b[k].v).max() / np.abs(b[k].v).max()) for k in a)
    measured(f'hoisted against unhoisted decomposition {net}, relative', worst)
    assert worst <= 1e-13


def _fp32_case(net, T=3, seed=2, hw=(5, 7)):
    p, h0, c, x, g_hs = scan_case(net, 2, T, *hw, seed=seed, dtype=torch.float32)
    with torch.no_grad():
        _, gates = gru_forward_torch(h0, c, x, p, net)
    return p, gates, c, x, g_hs


def _scan_ratio(net, defect=None, prev=None, T=3):
    p, gates, c, x, g_hs = _fp32_case(net, T)
    ref = gru_scan(B64(), gates, weights_of(p, net), c, x, g_hs, prev=prev)
    got = gru_scan(B32(), gates, weights_of(p, net), c, x, g_hs, defect=defect, prev=prev)
    return {k: worst_ratio(got[k], ref[k].v, ref[k].b) for k in ref}


@pytest.mark.parametrize('net', NETS)
def test_fp32_in_the_stated_order_is_inside_the_bounds(net):
    r = _scan_ratio(net)
    measured(f'fp32 scan in the stated order {net}, worst error / bound', max(r.values()))
    assert max(r.values()) <= 1.0, r
    gen = torch.Generator().manual_seed(3)
    p = gru_params(net, **SMALL, dtype=torch.float32)
    prev = {k: torch.randn(v.shape, generator=gen) for k, v in p.items()}
    r = _scan_ratio(net, prev=prev)
    measured(f'fp32 scan accumulating into param_grads {net}, worst error / bound', max(r.values()))
    assert max(r.values()) <= 1.0, r


@pytest.mark.parametrize('defect', DEFECTS)
def test_planted_defects_outside(defect):
    for net in (['SeqConv'] if defect == 'passes_forward_order' else NETS):
        r = _scan_ratio(net, defect)
        measured(f'defect {defect} {net} / bound', max(r.values()))
        assert max(r.values()) > 1.0


# ==================================================================================================== the gate kernels
GATE_REGIMES = ['nominal', 'saturated', 'h_equals_q', 'zero_cotangent', 'decades']
ONE_BELOW = float(np.float32(1.0) - np.float32(2.0 ** -24))


def gate_case(regime, m, c, h, w, seed=0):
    """-> dict g, g_rh, h, z, r, q: (M, C, H, W) float32"""
    gen = torch.Generator().manual_seed(9900 + seed + m + 3 * c + 5 * h + 7 * w)
    R = lambda: torch.randn((m, c, h, w), generator=gen)       # noqa: E731
    d = dict(g=R(), g_rh=R(), h=torch.tanh(R()), z=torch.sigmoid(R()), r=torch.sigmoid(2 * R()), q=torch.tanh(2 * R()))
    if regime == 'saturated':                  # z, r within an ulp of 0 and of 1, |q| within an ulp of 1
        pick = lambda vals: torch.tensor(vals)[torch.randint(len(vals), (m, c, h, w), generator=gen)]      # noqa: E731
        d['z'], d['r'] = pick([0.0, 2.0 ** -24, ONE_BELOW, 1.0]), pick([0.0, 2.0 ** -24, ONE_BELOW, 1.0])
        d['q'] = pick([1.0, -1.0, ONE_BELOW, -ONE_BELOW])
    if regime == 'h_equals_q':
        d['h'] = d['q'].clone()
    if regime == 'zero_cotangent':
        d['g'], d['g_rh'] = torch.zeros_like(d['g']), torch.zeros_like(d['g'])
    if regime == 'decades':
        d['g'] = d['g'] * 10.0 ** (3 * torch.rand((m, c, h, w), generator=gen) - 1.5)
        d['g_rh'] = d['g_rh'] * 10.0 ** (3 * torch.rand((m, c, h, w), generator=gen) - 1.5)
    return {k: v.contiguous() for k, v in d.items()}


def gate_refs(d):
    """-> dict u_q, u_z, u_r, g_h_direct: V, the cotangents exact"""
    be = B64()
    u_q, u_z = be.gate_q(V(d['g']), d['h'], d['z'], d['q'])
    u_r, g_h = be.gate_r(V(d['g']), d['z'], V(d['g_rh']), d['h'], d['r'])
    return dict(u_q=u_q, u_z=u_z, u_r=u_r, g_h_direct=g_h)


def gate_fp32(d, defect=None):
    be = B32()
    u_q, u_z = be.gate_q(d['g'], d['h'], d['z'], d['q'], defect)
    u_r, g_h = be.gate_r(d['g'], d['z'], d['g_rh'], d['h'], d['r'], defect)
    return dict(u_q=u_q, u_z=u_z, u_r=u_r, g_h_direct=g_h)


@pytest.mark.parametrize('regime', GATE_REGIMES)
def test_gate_arithmetic_in_fp32_is_inside_the_bounds(regime):
    d = gate_case(regime, 3, 33, 5, 7)
    ref, got = gate_refs(d), gate_fp32(d)
    worst = max(worst_ratio(got[k], ref[k].v, ref[k].b) for k in ref)
    measured(f'gate arithmetic fp32 {regime}, worst error / bound', worst)
    assert worst <= 1.0
    if regime == 'zero_cotangent':
        assert all(not torch.signbit(v).any() and not v.any() for v in got.values())          # +0 everywhere
    if regime == 'h_equals_q':
        assert not got['u_z'].any()
    for defect, key in (('one_minus_q', 'u_q'), ('r_factor_dropped', 'u_r'), ('grh_r_missing', 'g_h_direct')):
        if regime in ('nominal', 'decades'):
            assert worst_ratio(gate_fp32(d, defect)[key], ref[key].v, ref[key].b) > 1.0, defect


def test_shared_factors_are_the_activation_backward_s():
    """u_q = act_grad(g z, q, TANH), u_z = act_grad(g (q - h), z, SIGMOID), u_r = act_grad(g_rh h, r, SIGMOID) in the fp32
    emulations of both files, bit for bit"""
    d = gate_case('nominal', 3, 33, 5, 7)
    got = gate_fp32(d)
    assert torch.equal(got['u_q'], hg.act_fp32(d['g'] * d['z'], d['q'], hg.TANH))
    assert torch.equal(got['u_z'], hg.act_fp32(d['g'] * (d['q'] - d['h']), d['z'], hg.SIGMOID))
    assert torch.equal(got['u_r'], hg.act_fp32(d['g_rh'] * d['h'], d['r'], hg.SIGMOID))


# ============================================================================= the reference's own ConvGRU (fixture)
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'gru_grads.npz')
GOLDEN_MAPS = [(6, 5), (8, 8)]
GOLDEN_N, GOLDEN_T, GOLDEN_SEED = 2, 2, 20253
GOLDEN_WIDTHS = dict(hc=128, cc=128, cx=128)
GOLDEN_CHANNELS = [0, 64, 127]                 # channels of d loss / d h0, d c, d x_t that are stored


def golden_keys(net):
    return param_names(net) + ['g_h0', 'g_c'] + [f'g_x.{t}' for t in range(GOLDEN_T)]


def golden_case(net, hw):
    """-> (tag, parameters, h0, c, x (T, N, 128, h, w), the cotangents c_t at h_t) as float32 tensors, from the seeds; the
    weights are shared by the iterations"""
    from test_fc_grad_host import golden_param
    tag = f'{net}.{hw[0]}x{hw[1]}'
    hc, cc, cx = (GOLDEN_WIDTHS[k] for k in ('hc', 'cc', 'cx'))
    p = {}
    for i, k in enumerate(KERNELS[net]):
        for g in 'zrq':
            p[f'conv_{g}.{i}.conv.weight'] = golden_param(f'gru.{net}.conv_{g}.{i}.weight', (hc, hc + cc + cx, *k), GOLDEN_SEED)
            p[f'conv_{g}.{i}.conv.bias'] = golden_param(f'gru.{net}.conv_{g}.{i}.bias', (hc,), GOLDEN_SEED)
    t_ = lambda name, *s: golden_param(f'gru.{name}.{tag}', s, GOLDEN_SEED, scale=1.0)      # noqa: E731
    h0, c = torch.tanh(t_('h0', GOLDEN_N, hc, *hw)), torch.relu(t_('c', GOLDEN_N, cc, *hw))
    x = torch.stack([t_(f'x{t}', GOLDEN_N, cx, *hw) for t in range(GOLDEN_T)])
    cots = [t_(f'cot{t}', GOLDEN_N, hc, *hw) for t in range(GOLDEN_T)]
    return tag, p, h0, c, x, cots


def golden_pick(key, v):
    """the part of a full gradient the fixture stores: of a map the channels GOLDEN_CHANNELS, of a weight the first and the
    last output channel and every fourth input channel of those"""
    if key.startswith('g_'):
        return v[:, GOLDEN_CHANNELS]
    if key.endswith('weight'):
        return v[[0, v.shape[0] - 1]][:, ::4]
    return v


GOLDEN_LONGEST = 9 * 384                         # torch's longest fp32 chain in this stage: the 3 x 3 gates' 9 * 384 products


def golden_reference(net, hw, gates=None):
    """The float64 scan on the fixture's inputs GIVEN fp32 gates, and the room around it -> (tag, reference dict, room dict).
    ``gates`` None: the forward recomputed here in fp32 by the operators the reference's module calls (F.conv2d, sigmoid,
    tanh).  The room is the kernels' composed bound with EVERY dgrad / wgrad depth raised by torch's longest fp32 chain
    (GOLDEN_LONGEST): torch's convolutions add in an order of their own, and a host whose fp32 forward differs from the
    fixture's in the last bits moves the gates by a few ulps, which the raised depths leave room for (the reference sits at
    <= 7e-5 of this room, which therefore decides nothing by itself).  What decides is the float64-vs-fp32-CPU margin,
    |fixture - float64| relative to the largest entry of a gradient: measured at 3.6e-7 ... 5.0e-7 over the four cases
    (a few fp32 roundings through at most four 1920- or 3456-term sums), asserted at 1e-5 by the test below."""
    tag, p, h0, c, x, cots = golden_case(net, hw)
    if gates is None:
        with torch.no_grad():
            _, gates = gru_forward_torch(h0, c, x, p, net)
    old = hg.EXTRA
    hg.EXTRA = GOLDEN_LONGEST
    try:
        got = gru_scan(B64(), gates, weights_of(p, net), c, x, cots)
    finally:
        hg.EXTRA = old
    return tag, {k: v.v for k, v in got.items()}, {k: v.b for k, v in got.items()}


@pytest.mark.parametrize('net', NETS)
@pytest.mark.parametrize('hw', GOLDEN_MAPS, ids=lambda v: f'{v[0]}x{v[1]}')
def test_reference_autograd_agrees_with_the_restatement(net, hw):
    """The reference's fp32 gradients (autograd through its own ConvGRU, T = 2 iterations with shared weights, loss
    sum_t <c_t, h_t>) against the float64 scan.  The room (golden_reference) is for the reference's fp32 alone."""
    z = np.load(GOLDEN)
    tag, ref, room = golden_reference(net, hw)
    margin = 0.0
    for key in golden_keys(net):
        want = golden_pick(key, ref[key])
        v = worst_ratio(z[f'{tag}.{key}'], want, golden_pick(key, room[key]))
        measured(f'reference ConvGRU autograd {tag} {key}, error / (kernels\' bound at torch\'s depth)', v)
        assert v <= 1.0, key
        margin = max(margin, float(np.abs(z[f'{tag}.{key}'] - want).max() / np.abs(want).max()))
    measured(f'reference ConvGRU autograd {tag}, float64-vs-fp32-CPU margin relative to the largest entry', margin)
    assert margin <= 1e-5
    assert os.path.getsize(GOLDEN) < 200 * 1024
