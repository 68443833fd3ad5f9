"""CPU: backward of the pose head's fully connected tail (fc_grad.hip) -- the heads and the class selection, nn.Linear's
input and parameter gradients on the matrix cores, the GroupNorm + ReLU backward on the flattened map -- restated in
float64 with the ReLU masks as INPUTS, with a per-element bound for any fp32 evaluation in the kernels' operation order,
the inputs tests/test_gpu_fc_grad.py feeds the HIP kernels, fp32 emulations in the kernels' order with planted defects,
and the proof that the bounds are neither vacuous nor unreachable.  Helpers (U, EV, f64, worst_ratio, gamma, ...) are
those of tests/test_stream_ops_host.py and tests/test_fc_host.py.

  dgrad      g_s = (g W) [a > 0]:  gamma_d sum_o |g| |W|  +  sum_o (bound of g) |W| (1 + gamma_d),   d = DGRAD_DEPTH(O)
  wgrad      dW = g^T a:           gamma_d sum_m |g| |a|  +  carried bounds of g and of a,            d = WGRAD_DEPTH(M)
  selection  nine products:        gamma_10 sum |g| |W|;  its weight gradients: a chain over the rows, d = 1 + M
  GroupNorm  a running bound (EV) through the kernel's own expression, the sums with their chain depths; the fp32
             recomputation of mean and rstd is part of it, and a constant group (rstd = eps^-1/2) keeps it finite.
v_mfma_f32_32x32x2_f32 may round less often than once per product and accumulation, never more often.  Underflow is
outside the model, as in test_fc_host.
"""
import math
import os
import re

import numpy as np
import pytest
import torch

from test_stream_ops_host import EV, IN_EPS, U, f64, measured, worst_ratio  # noqa: E402
from test_fc_host import FC_GN, FC_HEAD_GEOMETRY, _wave_sum_fp32, gamma  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, 'scflow_amd', 'csrc', 'fc_grad.hip')).read()


def _define(name):
    return int(re.search(rf'#define\s+{name}\s+(\d+)', SRC).group(1))


CHUNK, THREADS = _define('FG_CHUNK'), _define('FG_THREADS')
EXTRA = 0                           # added to every depth: 0 for the kernels; the golden test raises it for torch's own fp32


# ================================================================================================ depths, from the source
def dgrad_depth(o):
    """fg_dgrad_kernel: `acc = mfma_f32_32x32x2f32(ap[o], bp[o * FG_WPITCH], acc)` x FG_CHUNK / 2 per chunk, two columns
    each, over ceil(O / FG_CHUNK) chunks of the zero-filled tiles: 1 product + FG_CHUNK * chunks accumulations."""
    return 1 + CHUNK * -(-o // CHUNK) + EXTRA


def wgrad_depth(m, accumulate=False, bias=False):
    """fg_wgrad_kernel: a chunk's chain (1 product + FG_CHUNK accumulations; `part = part + Gt[m * 32 + tid]`: FG_CHUNK
    additions, no product, for db), `tot[r] = tot[r] + acc[r]` per chunk, `*d + tot[r]` under accumulate."""
    return (0 if bias else 1) + CHUNK + -(-m // CHUNK) + (1 if accumulate else 0) + EXTRA


SELECT_DEPTH = 1 + 9                # fg_select_kernel: `acc = acc + g * W` x 6 + 3


def select_wgrad_depth(m, accumulate=False, bias=False):
    """fg_select_kernel: `acc + gv * p.a[...]` / `acc + gv` over the rows of the class, at most M; `*dst + acc`."""
    return (0 if bias else 1) + m + (1 if accumulate else 0) + EXTRA


def gn_grad_depth(gsz):
    """fg_norm_grad_kernel: `for (i = lane; i < gn_size; i += 64) s = s + ...` then fg_wave_sum: 6 levels."""
    return -(-gsz // 64) + 6 + EXTRA


def gn_param_depth(m, hw, accumulate=False):
    """fg_norm_param_kernel: `dg = dg + gu * xh` over ceil(M / 256) rows x hw features, the tree: log2(256) levels."""
    return 1 + -(-m // THREADS) * hw + int(math.log2(THREADS)) + (1 if accumulate else 0) + EXTRA


# ===================================================================================================== float64 pieces
def clamp_class(label, n_rows, samples, num_class, mode):
    """pose_update_one's class of every stacked row (row m = sample m % samples)."""
    lab = np.asarray(label, dtype=np.int64)
    c = lab[np.arange(n_rows) % samples] if mode & 1 else np.full(n_rows, lab[0])
    c = np.where(c < 0, c + num_class, c)
    return np.clip(c, 0, num_class - 1)


def dgrad_ref(g, gb, w, mask=None):
    g, w = f64(g), f64(w)
    gm = gamma(dgrad_depth(w.shape[0]))
    gb = np.broadcast_to(np.asarray(gb, dtype=np.float64), g.shape)
    with np.errstate(all='ignore'):
        ref, b = g @ w, gm * (np.abs(g) @ np.abs(w)) + (gb @ np.abs(w)) * (1 + gm)
    if mask is not None:
        ref, b = ref * mask, b * mask
    return ref, b


def _outer_ref(g, gb, a, ab, d_w, d_b, prev=None):
    g, a = f64(g), f64(a)
    gb = np.broadcast_to(np.asarray(gb, dtype=np.float64), g.shape)
    ab = np.broadcast_to(np.asarray(ab, dtype=np.float64), a.shape)
    with np.errstate(all='ignore'):
        dw, sh = g.T @ a, np.abs(g).T @ np.abs(a)
        carried = gb.T @ (np.abs(a) + ab) + np.abs(g).T @ ab
        db, shb, cb = g.sum(0), np.abs(g).sum(0), gb.sum(0)
        if prev is not None:
            dw, sh, db, shb = dw + f64(prev[0]), sh + np.abs(f64(prev[0])), db + f64(prev[1]), shb + np.abs(f64(prev[1]))
    return (dw, gamma(d_w) * sh + carried * (1 + gamma(d_w))), (db, gamma(d_b) * shb + cb * (1 + gamma(d_b)))


def wgrad_ref(g, gb, a, ab=0.0, prev=None):
    """-> ((dW, bound), (db, bound)); prev = (dW, db) the call accumulates into."""
    m = g.shape[0]
    return _outer_ref(g, gb, a, ab, wgrad_depth(m, prev is not None), wgrad_depth(m, prev is not None, bias=True), prev)


def select_ref(g_rot, g_trans, wr, wt, a, ab, cls, mask=None, prev=None):
    """-> (g_s, bound), [(dWr, b), (dbr, b), (dWt, b), (dbt, b)]; a: the heads' input with bound ab."""
    g_rot, g_trans, wr, wt, a = f64(g_rot), f64(g_trans), f64(wr), f64(wt), f64(a)
    m, k = a.shape
    nc = wr.shape[0] // 6
    wsel = np.concatenate([wr.reshape(nc, 6, k)[cls], wt.reshape(nc, 3, k)[cls]], 1)          # (M, 9, K)
    g9 = np.concatenate([g_rot, g_trans], 1)
    ref = np.einsum('mr,mrk->mk', g9, wsel)
    b = gamma(SELECT_DEPTH + EXTRA) * np.einsum('mr,mrk->mk', np.abs(g9), np.abs(wsel))
    if mask is not None:
        ref, b = ref * mask, b * mask
    onehot = (cls[:, None] == np.arange(nc)[None]).astype(np.float64)                        # (M, nc)
    out = []
    for i, (g, wd) in enumerate(((g_rot, 6), (g_trans, 3))):
        ge = (onehot[:, :, None] * g[:, None, :]).reshape(m, nc * wd)                        # row m's g in its class' rows
        p = None if prev is None else (prev[2 * i], prev[2 * i + 1])
        w_, b_ = _outer_ref(ge, 0.0, a, ab, select_wgrad_depth(m, prev is not None),
                            select_wgrad_depth(m, prev is not None, bias=True), p)
        out += [w_, b_]
    return (ref, b), out


def ev_sum(x, depth, axis=-1):
    g = gamma(depth)
    with np.errstate(all='ignore'):
        return EV(x.v.sum(axis, keepdims=True), x.e.sum(axis, keepdims=True) * (1 + g) + g * np.abs(x.v).sum(axis, keepdims=True))


def gn_grad_ref(y, g_x0, gxb, mask, gam, gsz, hw, prev=None):
    """y (M, K) float64: the in-order fp32 sum of the parts, exact; g_x0 with bound gxb; mask = [x0 > 0].
    -> (g_y, bound), (dgamma, bound), (dbeta, bound): the kernel's expression through the running bound."""
    m, k = y.shape
    G, n, D = k // gsz, float(gsz), gn_grad_depth(gsz)
    ch = np.arange(k) // hw
    C = -(-k // hw)
    yv = EV(y.reshape(m, G, gsz))
    mean = ev_sum(yv, D) / n
    a = yv - mean
    rstd = EV(1.0) / (ev_sum(a * a, D) / n + EV(float(np.float32(IN_EPS)))).sqrt()
    xh = a * rstd
    gxb = np.broadcast_to(np.asarray(gxb, dtype=np.float64), y.shape)
    gu = EV((f64(g_x0) * mask).reshape(m, G, gsz), (gxb * mask).reshape(m, G, gsz))
    t = EV(f64(gam)[ch].reshape(1, G, gsz)) * gu
    ma, mb = ev_sum(t, D) / n, ev_sum(t * xh, D) / n
    gy = rstd * ((t - ma) - xh * mb)
    onehot = (ch[:, None] == np.arange(C)[None]).astype(np.float64)                           # (K, C)
    acc = prev is not None
    gp = gamma(gn_param_depth(m, hw, acc))
    gpb = gamma(gn_param_depth(m, hw, acc) - 1)
    pr = gu * xh
    out = []
    for ev, gq, pv in ((pr, gp, None if not acc else prev[0]), (gu, gpb, None if not acc else prev[1])):
        v, e = ev.v.reshape(m, k).sum(0) @ onehot, ev.e.reshape(m, k).sum(0) @ onehot
        sh = np.abs(ev.v).reshape(m, k).sum(0) @ onehot
        if pv is not None:
            v, sh = v + f64(pv), sh + np.abs(f64(pv))
        out.append((v, gq * sh + e * (1 + gq)))
    return (gy.v.reshape(m, k), gy.e.reshape(m, k)), out[0], out[1]


def tail_ref64(y, p, cls, g_rot, g_trans, gsz, hw, masks=None):
    """The whole tail in float64, closed forms.  p: dict of float64 arrays (W1, b1, W2, b2, Wr, br, Wt, bt, gamma, beta).
    masks = (x0 > 0, a1 > 0, a2 > 0) or None: decided here.  -> dict of gradients."""
    m, k = y.shape
    G = k // gsz
    ch = np.arange(k) // hw
    yg = y.reshape(m, G, gsz)
    mean = yg.mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(((yg - mean) ** 2).mean(-1, keepdims=True) + float(np.float32(IN_EPS)))
    xh = ((yg - mean) * rstd).reshape(m, k)
    u = xh * p['gamma'][ch] + p['beta'][ch]
    m0 = (u > 0) if masks is None else masks[0]
    x0 = u * m0
    z1 = x0 @ p['W1'].T + p['b1']
    m1 = (z1 > 0) if masks is None else masks[1]
    a1 = z1 * m1
    z2 = a1 @ p['W2'].T + p['b2']
    m2 = (z2 > 0) if masks is None else masks[2]
    a2 = z2 * m2
    (g_s2, _), hg = select_ref(g_rot, g_trans, p['Wr'], p['Wt'], a2, 0.0, cls, m2)
    g_s1 = (g_s2 @ p['W2']) * m1
    g_x0 = g_s1 @ p['W1']
    gu = g_x0 * m0
    t = (gu * p['gamma'][ch]).reshape(m, G, gsz)
    xg = xh.reshape(m, G, gsz)
    g_y = (rstd * (t - t.mean(-1, keepdims=True) - xg * (t * xg).mean(-1, keepdims=True))).reshape(m, k)
    C = -(-k // hw)
    onehot = (ch[:, None] == np.arange(C)[None]).astype(np.float64)
    return dict(g_y=g_y, W1=g_s1.T @ x0, b1=g_s1.sum(0), W2=g_s2.T @ a1, b2=g_s2.sum(0), Wr=hg[0][0], br=hg[1][0],
                Wt=hg[2][0], bt=hg[3][0], gamma=(gu * xh).sum(0) @ onehot, beta=gu.sum(0) @ onehot,
                x0=x0, a1=a1, a2=a2, g_s2=g_s2, g_s1=g_s1, g_x0=g_x0)


# ============================================================================================================= cases
GRAD_REGIMES = ['nominal', 'offset', 'constant_group', 'cancelling', 'scaled_up', 'scaled_down']
GRAD_SCALES = {'scaled_up': (40, 20), 'scaled_down': (-30, -20)}      # powers of two on g and on the other operand
GRAD_M = [1, 31, 32, 33, 65, 257]
GRAD_O = [1, 31, 32, 33, 40]
GRAD_K = [8, 56, 64, 72, 256, 264]
GEMM_REGIMES = ['nominal', 'cancelling', 'scaled_up', 'scaled_down']
GN_GRAD_REGIMES = ['nominal', 'offset', 'constant_group', 'cancelling', 'scaled_up', 'scaled_down']


def gemm_shapes():
    """(M, O, K): every M with two (O, K), every (O, K) pair once"""
    pairs = [(o, k) for o in GRAD_O for k in GRAD_K]
    out = [(GRAD_M[i % len(GRAD_M)], o, k) for i, (o, k) in enumerate(pairs)]
    return out + [(257, 40, 264), (1, 1, 8), (65, 33, 72)]


def gemm_case(regime, m, o, k, seed=0):
    """g (M, O) cotangent, W (O, K) weight, a (M, K) post-ReLU activation (exact zeros on about half its entries)."""
    scaled = regime in GRAD_SCALES
    gen = torch.Generator().manual_seed(7000 + 100 * GRAD_REGIMES.index('nominal' if scaled else regime) + seed + m + 3 * o + 7 * k)
    g = torch.randn((m, o), generator=gen)
    w = torch.randn((o, k), generator=gen) * o ** -0.5
    a = torch.relu(torch.randn((m, k), generator=gen))
    if regime == 'cancelling':              # the two halves of the contraction cancel to 1e-4 of the shadow (dgrad: over o,
        h = o // 2                          # wgrad: over m)
        if h:
            g[:, h:2 * h] = g[:, :h]
            w[h:2 * h] = -w[:h] * (1 + 1e-4 * torch.randn(w[:h].shape, generator=gen))
        hm = m // 2
        if hm:
            a[hm:2 * hm] = a[:hm]
            g[hm:2 * hm] = -g[:hm] * (1 + 1e-4 * torch.randn(g[:hm].shape, generator=gen))
    scale = 1.0
    if scaled:
        eg, ew = GRAD_SCALES[regime]
        g, w, a, scale = g * 2.0 ** eg, w * 2.0 ** ew, a * 2.0 ** ew, 2.0 ** (eg + ew)
    return g.contiguous(), w.contiguous(), a.contiguous(), scale


def gn_geometries():
    return FC_GN + list(FC_HEAD_GEOMETRY.values())


def gn_grad_case(regime, gsz, hw, k, m=3, parts=1, seed=0):
    """y (parts, M, K), gamma, beta, x0 (M, K) the forward's output in float64-rounded-to-fp32 (its sign pattern is the
    mask: an INPUT of the backward), g_x0 (M, K)."""
    scaled = regime in GRAD_SCALES
    gen = torch.Generator().manual_seed(8000 + 100 * GRAD_REGIMES.index('nominal' if scaled else regime) + seed + gsz + 5 * hw + k)
    y = torch.randn((parts, m, k), generator=gen) * parts ** -0.5
    c = -(-k // hw)
    gam, bet = 1.0 + 0.5 * torch.randn((c,), generator=gen), 0.3 * torch.randn((c,), generator=gen)
    g_x0 = torch.randn((m, k), generator=gen)
    if regime == 'offset':
        y[0] += 300.0
    if regime == 'constant_group':
        y[:, :, :gsz] = 0.0
        y[0, :, :gsz] = 2.5
    if regime == 'cancelling':              # every mask open (beta >> |gamma x^|), gamma away from 0, y on a large offset
        gam, bet = gam.abs().clamp_min(0.3), bet.abs() + 8.0
        y[0] += 300.0
    scale = 1.0
    if scaled:                              # the cotangent scales; y does not (GroupNorm is not homogeneous in y + eps)
        scale = 2.0 ** GRAD_SCALES[regime][0]
        g_x0 = g_x0 * scale
    ysum = y[0].clone()
    for s in range(1, parts):
        ysum = (ysum + y[s]).float()
    yg = ysum.double().reshape(m, k // gsz, gsz)
    mean = yg.mean(-1, keepdim=True)
    xh = ((yg - mean) / torch.sqrt(((yg - mean) ** 2).mean(-1, keepdim=True) + IN_EPS)).reshape(m, k)
    ch = torch.arange(k) // hw
    x0 = torch.relu(xh * gam.double()[ch] + bet.double()[ch]).float()
    if regime == 'cancelling':              # t = gamma g_u constant within a group to 1e-4: t - mean_g(t) cancels, and so does
        const = torch.randn((m, k // gsz, 1), generator=gen).expand(m, k // gsz, gsz).reshape(m, k)      # x^ mean_g(t x^)
        g_x0 = (const / gam[ch] * (1 + 1e-4 * torch.randn((m, k), generator=gen))).float()
        assert bool((x0 > 0).all()) or gsz == 2
    return y.contiguous(), ysum, gam, bet, x0.contiguous(), g_x0.contiguous(), scale


SELECT_CASES = [(1, 1, 8, 3), (2, 3, 72, 3), (3, 1, 256, 21), (2, 3, 264, 4), (5, 2, 40, 2)]      # (N, T, K, num_class)
SELECT_LABELS = {'in_range': lambda n, nc: [(3 * i + 1) % nc for i in range(n)],
                 'out_of_range': lambda n, nc: [(nc + 5, -1, -nc - 3, 0, 2 * nc)[i % 5] for i in range(n)]}


def select_case(n, t, k, nc, labels='in_range', seed=0):
    gen = torch.Generator().manual_seed(9100 + n + 10 * t + k + nc + seed)
    m = n * t
    g_rot, g_trans = torch.randn((m, 6), generator=gen), torch.randn((m, 3), generator=gen)
    wr, wt = torch.randn((6 * nc, k), generator=gen) * k ** -0.5, torch.randn((3 * nc, k), generator=gen) * k ** -0.5
    a = torch.relu(torch.randn((m, k), generator=gen))
    label = torch.tensor(SELECT_LABELS[labels](n, nc), dtype=torch.int64)
    return g_rot, g_trans, wr, wt, a, label


# ================================================================================== fp32 emulations in the kernels' order
GRAD_DEFECTS = ['mask_dropped', 'mask_ge_zero', 'w_for_wt', 'label0_under_per_sample', 'per_sample_under_label0',
                'dbeta_without_mask', 'gn_first_mean_term_missing', 'gn_second_mean_term_missing', 'gamma_by_group',
                'wgrad_last_chunk_dropped', 'head2_bias_grad_from_head1']


def dgrad_fp32(g, w, a=None, defect=None):
    o, k = w.shape
    if defect == 'w_for_wt':
        w = w.reshape(k, o).t()             # the (O, K) buffer indexed [k][o]
    acc = torch.zeros((g.shape[0], k))
    for i in range(o):                      # the zero columns past O add +0: no bit changes
        acc = acc + g[:, i, None] * w[i][None]
    if a is None or defect == 'mask_dropped':
        return acc
    return torch.where(a >= 0 if defect == 'mask_ge_zero' else a > 0, acc, torch.zeros(()))


def wgrad_fp32(g, a, prev=None, defect=None):
    m = g.shape[0]
    tot, totb = torch.zeros((g.shape[1], a.shape[1])), torch.zeros((g.shape[1],))
    chunks = range(0, m, CHUNK)
    if defect == 'wgrad_last_chunk_dropped' and m % CHUNK:
        chunks = range(0, m - m % CHUNK, CHUNK)
    for c0 in chunks:
        acc, accb = torch.zeros_like(tot), torch.zeros_like(totb)
        for r in range(c0, min(c0 + CHUNK, m)):
            acc = acc + g[r][:, None] * a[r][None]
            accb = accb + g[r]
        tot, totb = tot + acc, totb + accb
    return (tot, totb) if prev is None else (prev[0] + tot, prev[1] + totb)


def select_fp32(g_rot, g_trans, wr, wt, a, label, samples, mode, mask=True, defect=None):
    m, k = a.shape
    nc = wr.shape[0] // 6
    if defect == 'label0_under_per_sample' and mode & 1 or defect == 'per_sample_under_label0' and not mode & 1:
        mode ^= 1
    cls = torch.from_numpy(clamp_class(label.numpy(), m, samples, nc, mode))
    acc = torch.zeros((m, k))
    for r in range(6):
        acc = acc + g_rot[:, r, None] * wr.reshape(nc, 6, k)[cls, r]
    for r in range(3):
        acc = acc + g_trans[:, r, None] * wt.reshape(nc, 3, k)[cls, r]
    if mask and defect != 'mask_dropped':
        acc = torch.where(a >= 0 if defect == 'mask_ge_zero' else a > 0, acc, torch.zeros(()))
    out = []
    for g, wd in ((g_rot, 6), (g_trans, 3)):
        dw, db = torch.zeros((nc * wd, k)), torch.zeros((nc * wd,))
        for r in range(m):
            rows = slice(int(cls[r]) * wd, int(cls[r]) * wd + wd)
            dw[rows] = dw[rows] + g[r][:, None] * a[r][None]
            db[rows] = db[rows] + g[r]
        out += [dw, db]
    if defect == 'head2_bias_grad_from_head1':
        out[3] = out[1].reshape(nc, 6)[:, :3].reshape(-1).clone()
    return acc, out


def _lane_sum_fp32(v):
    """(..., gsz) -> (..., 1): lane l adds its elements l, l + 64, ... in order, then the xor butterfly."""
    gsz = v.shape[-1]
    pad = -gsz % 64
    v = torch.cat([v, torch.zeros(v.shape[:-1] + (pad,))], -1).reshape(v.shape[:-1] + (-1, 64))
    s = torch.zeros(v.shape[:-2] + (64,))
    for j in range(v.shape[-2]):
        s = s + v[..., j, :]
    return _wave_sum_fp32(s)[..., None]


def gn_grad_fp32(ysum, g_x0, x0, gam, gsz, hw, defect=None):
    m, k = ysum.shape
    G, n = k // gsz, torch.tensor(float(gsz))
    ch = (torch.arange(k) // (gsz if defect == 'gamma_by_group' else hw)) % gam.numel()
    yg = ysum.reshape(m, G, gsz)
    mean = _lane_sum_fp32(yg) / n
    a = yg - mean
    rstd = 1.0 / torch.sqrt(_lane_sum_fp32(a * a) / n + torch.tensor(IN_EPS))
    xh = a * rstd
    gu = torch.where(x0 > 0, g_x0, torch.zeros(())).reshape(m, G, gsz)
    t = gam[ch].reshape(1, G, gsz) * gu
    ma, mb = _lane_sum_fp32(t) / n, _lane_sum_fp32(t * xh) / n
    if defect == 'gn_first_mean_term_missing':
        ma = torch.zeros_like(ma)
    if defect == 'gn_second_mean_term_missing':
        mb = torch.zeros_like(mb)
    gy = (rstd * ((t - ma) - xh * mb)).reshape(m, k)
    # parameters: thread j owns rows j, j + 256, ...; features of the channel ascending inside a row; then the tree
    C = -(-k // hw)
    gub = g_x0.reshape(m, G, gsz) if defect == 'dbeta_without_mask' else gu
    pr, gub = (gu * xh).reshape(m, k), gub.reshape(m, k)
    dg, db = torch.zeros((THREADS, C)), torch.zeros((THREADS, C))
    chh = torch.arange(k) // hw
    for r in range(m):
        for i in range(hw):
            cols = torch.arange(C) * hw + i
            ok = cols < k
            dg[r % THREADS, ok] = dg[r % THREADS, ok] + pr[r, cols[ok]]
            db[r % THREADS, ok] = db[r % THREADS, ok] + gub[r, cols[ok]]
    assert int(chh.max()) == C - 1
    s = THREADS // 2
    while s >= 1:
        dg = dg[:s] + dg[s:2 * s]
        db = db[:s] + db[s:2 * s]
        s //= 2
    return gy, dg[0], db[0]


# ===================================================================================================== the self-checks
def test_depths_are_the_counts_of_the_source():
    assert (CHUNK, THREADS) == (32, 256)
    assert [dgrad_depth(o) for o in (1, 32, 33, 256, 1024)] == [33, 33, 65, 257, 1025]
    assert [wgrad_depth(m) for m in (1, 32, 33, 257)] == [34, 34, 35, 42] and wgrad_depth(257, True, True) == 42
    assert gn_grad_depth(64) == 7 and gn_grad_depth(2) == 7 and gn_grad_depth(256) == 10
    assert gn_param_depth(256, 16) == 25 and gn_param_depth(257, 16) == 41


def _torch_tail(y, p, cls, g_rot, g_trans, gsz, hw):
    """float64 autograd through the tail, the selection by index"""
    t = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in p.items()}
    yt = torch.tensor(y, dtype=torch.float64, requires_grad=True)
    m, k = y.shape
    ch = torch.arange(k) // hw
    yg = yt.reshape(m, k // gsz, gsz)
    mean = yg.mean(-1, keepdim=True)
    xh = ((yg - mean) / torch.sqrt(((yg - mean) ** 2).mean(-1, keepdim=True) + float(np.float32(IN_EPS)))).reshape(m, k)
    x0 = torch.relu(xh * t['gamma'][ch] + t['beta'][ch])
    a1 = torch.relu(x0 @ t['W1'].T + t['b1'])
    a2 = torch.relu(a1 @ t['W2'].T + t['b2'])
    nc = p['Wr'].shape[0] // 6
    rot = (a2 @ t['Wr'].T + t['br']).reshape(m, nc, 6)[torch.arange(m), torch.from_numpy(cls)]
    tr = (a2 @ t['Wt'].T + t['bt']).reshape(m, nc, 3)[torch.arange(m), torch.from_numpy(cls)]
    ((rot * torch.tensor(f64(g_rot))).sum() + (tr * torch.tensor(f64(g_trans))).sum()).backward()
    out = {k: v.grad.numpy() for k, v in t.items()}
    out['g_y'] = yt.grad.numpy()
    return out


def tail_params(k0, o1, o2, nc, hw, seed=0):
    """fp32 parameters of a tail from a fixed seed: dict of torch tensors"""
    rs = np.random.RandomState(1234 + seed)
    c = -(-k0 // hw)
    r = lambda *s: torch.from_numpy(rs.standard_normal(s).astype(np.float32))      # noqa: E731
    return dict(W1=r(o1, k0) * k0 ** -0.5, b1=0.1 * r(o1), W2=r(o2, o1) * o1 ** -0.5, b2=0.1 * r(o2),
                Wr=r(6 * nc, o2) * o2 ** -0.5, br=0.1 * r(6 * nc), Wt=r(3 * nc, o2) * o2 ** -0.5, bt=0.1 * r(3 * nc),
                gamma=1.0 + 0.5 * r(c), beta=0.3 * r(c))


@pytest.mark.parametrize('mode,labels', [(0, 'in_range'), (1, 'in_range'), (1, 'out_of_range'), (0, 'out_of_range')])
def test_closed_forms_equal_float64_autograd(mode, labels):
    worst = 0.0
    for gsz, hw, k0 in ((4, 1, 128), (16, 4, 512), (8, 3, 64)):
        n, T, nc = 3, 2, 3
        p = {k: f64(v) for k, v in tail_params(k0, 40, 24, nc, hw).items()}
        rs = np.random.RandomState(5)
        y = rs.standard_normal((n * T, k0))
        g_rot, g_trans = rs.standard_normal((n * T, 6)), rs.standard_normal((n * T, 3))
        cls = clamp_class(SELECT_LABELS[labels](n, nc), n * T, n, nc, mode)
        got, want = tail_ref64(y, p, cls, g_rot, g_trans, gsz, hw), _torch_tail(y, p, cls, g_rot, g_trans, gsz, hw)
        for key, w in want.items():
            worst = max(worst, float(np.abs(got[key] - w).max() / max(1.0, np.abs(w).max())))
    measured(f'closed forms - float64 autograd, label_mode {mode}, {labels}', worst)
    assert worst <= 1e-12


def _gemm_inputs():
    for m, o, k in gemm_shapes():
        yield 'nominal', m, o, k
    for m, o, k in gemm_shapes()[::6]:
        for regime in GEMM_REGIMES[1:]:
            yield regime, m, o, k


def _gn_inputs():
    for gsz, hw, _, k in gn_geometries():
        for regime in GN_GRAD_REGIMES:
            yield regime, gsz, hw, k, (3 if k > 512 else 33), (4 if gsz == 64 and hw == 16 else 1)
    yield 'nominal', 64, 16, 128, 257, 2          # a second row per thread of the parameter pass


def _select_inputs():
    for n, t, k, nc in SELECT_CASES:
        for mode in (0, 1):
            for labels in SELECT_LABELS:
                yield n, t, k, nc, mode, labels


def _worst(defect=None):
    """worst error / bound of the emulations over every input list; `defect` planted where it applies."""
    worst = {}

    def put(fam, *pairs):
        for got, (ref, b) in pairs:
            worst[fam] = max(worst.get(fam, 0.0), worst_ratio(got, ref, b))

    if defect in (None, 'mask_dropped', 'mask_ge_zero', 'w_for_wt', 'wgrad_last_chunk_dropped'):
        for regime, m, o, k in _gemm_inputs():
            g, w, a, _ = gemm_case(regime, m, o, k)
            if defect != 'wgrad_last_chunk_dropped':
                put('dgrad ' + regime, (dgrad_fp32(g, w, a, defect), dgrad_ref(g, 0.0, w, f64(a) > 0)))
            if defect in (None, 'wgrad_last_chunk_dropped'):
                put('dgrad unmasked ' + regime, (dgrad_fp32(g, w), dgrad_ref(g, 0.0, w)))
                dw, db = wgrad_fp32(g, a, defect=defect)
                rw, rb = wgrad_ref(g, 0.0, a)
                put('wgrad ' + regime, (dw, rw), (db, rb))
    if defect in (None, 'dbeta_without_mask', 'gn_first_mean_term_missing', 'gn_second_mean_term_missing', 'gamma_by_group'):
        for regime, gsz, hw, k, m, parts in _gn_inputs():
            _, ysum, gam, bet, x0, g_x0, _ = gn_grad_case(regime, gsz, hw, k, m, parts)
            gy, dg, db = gn_grad_fp32(ysum, g_x0, x0, gam, gsz, hw, defect)
            rgy, rdg, rdb = gn_grad_ref(f64(ysum), g_x0, 0.0, f64(x0) > 0, gam, gsz, hw)
            put('GroupNorm ' + regime, (gy, rgy), (dg, rdg), (db, rdb))
            assert np.isfinite(rgy[1]).all() and np.isfinite(rdg[1]).all(), (regime, gsz, hw)
    if defect in (None, 'mask_dropped', 'mask_ge_zero', 'label0_under_per_sample', 'per_sample_under_label0',
                  'head2_bias_grad_from_head1'):
        for n, t, k, nc, mode, labels in _select_inputs():
            g_rot, g_trans, wr, wt, a, label = select_case(n, t, k, nc, labels)
            cls = clamp_class(label.numpy(), n * t, n, nc, mode)
            gs, grads = select_fp32(g_rot, g_trans, wr, wt, a, label, n, mode, defect=defect)
            rgs, rgrads = select_ref(g_rot, g_trans, wr, wt, a, 0.0, cls, f64(a) > 0)
            put('selection', (gs, rgs), *zip(grads, rgrads))
    return worst


def test_emulations_inside_the_bounds():
    for fam, v in _worst().items():
        measured(f'fc_grad fp32 emulation / bound, {fam}', v)
        assert v <= 1.0, fam


@pytest.mark.parametrize('defect', GRAD_DEFECTS)
def test_planted_defects_outside(defect):
    worst = max(_worst(defect).values())
    measured(f'defect {defect} / bound (worst case of the GPU lists)', worst)
    assert worst > 1.0


def test_accumulate_is_one_more_rounding():
    g, _, a, _ = gemm_case('nominal', 65, 33, 72)
    prev = (torch.randn((33, 72), generator=torch.Generator().manual_seed(1)), torch.randn((33,), generator=torch.Generator().manual_seed(2)))
    dw, db = wgrad_fp32(g, a, prev)
    rw, rb = wgrad_ref(g, 0.0, a, prev=prev)
    assert worst_ratio(dw, *rw) <= 1.0 and worst_ratio(db, *rb) <= 1.0
    one, oneb = wgrad_fp32(g, a)
    assert torch.equal(dw, prev[0] + one) and torch.equal(db, prev[1] + oneb)


def test_unselected_class_rows_are_exact_zeros():
    g_rot, g_trans, wr, wt, a, label = select_case(2, 3, 72, 3)
    _, grads = select_fp32(g_rot, g_trans, wr, wt, a, label, 2, 0)
    c = int(label[0])
    for t, wd in zip(grads, (6, 6, 3, 3)):
        t = t.reshape(3, wd, -1)
        assert all(bool((t[j] == 0).all()) for j in range(3) if j != c) and bool((t[c] != 0).any())


def test_constant_group_keeps_a_finite_bound():
    _, ysum, gam, bet, x0, g_x0, _ = gn_grad_case('constant_group', 64, 16, 2048)
    (gy, b), _, _ = gn_grad_ref(f64(ysum), g_x0, 0.0, f64(x0) > 0, gam, 64, 16)
    assert np.isfinite(b).all() and float(b[:, :64].max()) < 1e-2 * IN_EPS ** -0.5

# ============================================================================== the reference's own head (golden fixture)
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'fc_grads.npz')
GOLDEN_FEAT_SIZES = [(8, 8), (16, 16)]
GOLDEN_LABELS = [2, 0, 1]           # differing: the reference selects label[0] = 2 for the whole batch
GOLDEN_ROWS = [0, 1, 2, 100, 255, 511, 700, 1023]                   # rows (mod the row count) of dW1 / dW2 that are stored
GOLDEN_SEED = 20240
TAIL_NAMES = dict(W1='fc_layers.0.0.weight', b1='fc_layers.0.0.bias', W2='fc_layers.1.0.weight', b2='fc_layers.1.0.bias',
                  Wr='rotation_pred.weight', br='rotation_pred.bias', Wt='translation_pred.weight', bt='translation_pred.bias',
                  gamma='conv_layers.2.gn.weight', beta='conv_layers.2.gn.bias')


def golden_param(name, shape, seed, scale=None):
    """a pure function of (name, shape, seed): weights N(0, 0.05^2), biases N(0, 0.1^2), GroupNorm weights 1 + N(0, 0.1^2)"""
    import zlib
    rs = np.random.RandomState((seed + zlib.crc32(name.encode())) % 2 ** 32)
    v = rs.standard_normal(shape).astype(np.float32)
    if scale is None:
        scale = 0.05 if len(shape) > 1 else 0.1
    v = v * np.float32(scale)
    if name.endswith('gn.weight'):
        v = v + np.float32(1.0)
    return torch.from_numpy(v)


def tail_bounds(ref, p, ysum, cls, g_rot, g_tr, gsz, hw, masks, act_bounds):
    """the composed bound of the whole backward around the float64 tail `ref` (tail_ref64): every stage's bound goes
    through the next stage; act_bounds = (x0b, a1b, a2b) of the forward's activations.  -> dict like tail_ref64's."""
    x0b, a1b, a2b = act_bounds
    (_, b_s2), hg = select_ref(g_rot, g_tr, p['Wr'], p['Wt'], ref['a2'], a2b, cls, masks[2])
    (_, bw2), (_, bb2) = wgrad_ref(ref['g_s2'], b_s2, ref['a1'], a1b)
    _, b_s1 = dgrad_ref(ref['g_s2'], b_s2, p['W2'], masks[1])
    (_, bw1), (_, bb1) = wgrad_ref(ref['g_s1'], b_s1, ref['x0'], x0b)
    _, b_x0 = dgrad_ref(ref['g_s1'], b_s1, p['W1'])
    (_, b_gy), (_, b_dg), (_, b_db) = gn_grad_ref(ysum, ref['g_x0'], b_x0, masks[0], p['gamma'], gsz, hw)
    return dict(W1=bw1, b1=bb1, W2=bw2, b2=bb2, Wr=hg[0][1], br=hg[1][1], Wt=hg[2][1], bt=hg[3][1], gamma=b_dg, beta=b_db, g_y=b_gy)


def _golden_case(z, fs):
    tag = f'{fs[0]}x{fs[1]}'
    y = f64(z[f'{tag}.y'])
    n, c, h, w = y.shape
    hw, k0 = h * w, c * h * w
    p = {key: f64(golden_param(name, {'W1': (1024, k0), 'b1': (1024,), 'W2': (256, 1024), 'b2': (256,), 'Wr': (18, 256),
                                      'br': (18,), 'Wt': (9, 256), 'bt': (9,), 'gamma': (c,), 'beta': (c,)}[key], GOLDEN_SEED))
         for key, name in TAIL_NAMES.items()}
    g_rot = f64(golden_param('g_rot.' + tag, (n, 6), GOLDEN_SEED, scale=1.0))
    g_tr = f64(golden_param('g_trans.' + tag, (n, 3), GOLDEN_SEED, scale=1.0))
    return tag, y.reshape(n, k0), p, g_rot, g_tr, k0 // 32, hw


@pytest.mark.parametrize('fs', GOLDEN_FEAT_SIZES, ids=lambda v: f'{v[0]}x{v[1]}')
def test_reference_head_autograd_agrees_with_the_restatement(fs):
    """The reference's fp32 gradients against the float64 restatement.  The room is the kernels' composed bound PLUS
    torch's own fp32 terms: its forward activations and its backward sums are some fp32 evaluation whose chains are at
    most as long as the sums themselves, so every depth is raised by the longest sum of the tail (`fc_grad_host.EXTRA`).
    This room is for the reference's fp32 alone; tests/test_gpu_fc_grad.py never grants it to the kernels."""
    from test_fc_host import fc_gn_ref, gemm_ref
    import test_fc_grad_host as me
    z = np.load(GOLDEN)
    tag, y, p, g_rot, g_tr, gsz, hw = _golden_case(z, fs)
    n, k0 = y.shape
    nc = 3
    cls0 = clamp_class(GOLDEN_LABELS, n, n, nc, 0)
    ref = tail_ref64(y, p, cls0, g_rot, g_tr, gsz, hw)
    masks = tuple(ref[key] > 0 for key in ('x0', 'a1', 'a2'))
    longest = max(k0, 1024)
    # torch's forward: GroupNorm (norm_core at the group size), then plain fp32 linears of chain length <= K + 1
    gam_t, bet_t = torch.from_numpy(p['gamma']).float(), torch.from_numpy(p['beta']).float()
    _, x0b = fc_gn_ref(y, gsz, hw, gam_t, bet_t)
    x0b = 2.0 * x0b                                                 # torch's own group sums: twice the fold's bound
    _, a1b = gemm_ref(ref['x0'], x0b, p['W1'], p['b1'], k0 + 1)
    _, a2b = gemm_ref(ref['a1'], a1b[0], p['W2'], p['b2'], 1024 + 1)
    old = me.EXTRA
    me.EXTRA = longest
    try:
        bounds = tail_bounds(ref, p, y, cls0, g_rot, g_tr, gsz, hw, masks, (x0b, a1b[0], a2b[0]))
    finally:
        me.EXTRA = old
    worst = {}
    for key in list(TAIL_NAMES) + ['g_y']:
        want, b = ref[key], bounds[key]
        if key in ('W1', 'W2'):
            rows = [r % want.shape[0] for r in GOLDEN_ROWS]
            want, b = want[rows], b[rows]
        worst[key] = worst_ratio(z[f'{tag}.{key}'].reshape(want.shape), want, b)
    for key, v in worst.items():
        measured(f'reference head autograd {tag} {key}, error / (kernels\' bound + torch fp32 terms)', v)
        assert v <= 1.0, key
    # the fixture's labels differ and the reference used label[0] for all of them: per-sample selection is another function
    per = tail_ref64(y, p, clamp_class(GOLDEN_LABELS, n, n, nc, 1), g_rot, g_tr, gsz, hw, masks)
    assert worst_ratio(z[f'{tag}.Wr'], per['Wr'], bounds['Wr'] + 1e-30) > 10
    assert worst_ratio(z[f'{tag}.g_y'].reshape(n, k0), per['g_y'], bounds['g_y'] + 1e-30) > 10
    assert os.path.getsize(GOLDEN) < 200 * 1024
