"""CPU: backward of the stride-1 convolutions with bias (conv_s1_grad.hip) and of the decoder's heads and encoders
(SCFlowDecoder.heads_backward) -- restated in float64 as explicit index sums, with a per-element bound for any fp32
evaluation in the kernels' operation order, the inputs tests/test_gpu_head_grad.py feeds the HIP kernels, fp32 emulations
in the kernels' order (fma chains) with planted defects, and the composed float64 stage held against float64 autograd.

  dgrad   gx = act'(a) (sum_{tap, co} g w + add):  core gamma_d sum |g| |w| + sum (bound of g) |w| (1 + gamma_d), d =
          DGRAD_DEPTH; a border element's sum holds only the taps that exist.  + add: one rounding U (|core| + |add| + b)
          and add's own bound.  Factor f(a), a taken as given: (b + gamma_k (|v| + b)) |f|, k = 0 (ReLU: a mask), 3
          (sigmoid: 1 - a, a (1 - a), v f), 2 (tanh: fma(-a, a, 1), v f)
  wgrad   dW = sum_{m, y, x} g x:  gamma_d sum |g| |x| + carried bounds of g and of x, d = WGRAD_DEPTH(plan);  db = sum g:
          gamma_d sum |g| + the carried bound, the same d (a bias chain has no product: one rounding fewer)
Underflow is outside the model, as in test_fc_host.
"""
import os
import re

import numpy as np
import pytest
import torch

from test_stream_ops_host import f64, measured, worst_ratio  # noqa: E402
from test_fc_host import U, gamma  # noqa: E402
from test_conv_grad_host import fma  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, 'scflow_amd', 'csrc', 'conv_s1_grad.hip')).read()
F = torch.nn.functional
NONE, RELU, SIGMOID, TANH = 0, 1, 2, 3           # include/scflow_hip.h: SCF_ACT_*
ACTS = (NONE, RELU, SIGMOID, TANH)


def _define(name):
    return int(re.search(rf'#define\s+{name}\s+(\d+)', SRC).group(1))


MFMA_MIN_C, SD_CHUNK, SW_TILE, SW_PIX, SW_MIN_CHUNKS, SW_BLOCKS = (_define(k) for k in (
    'S1_MFMA_MIN_C', 'SD_CHUNK', 'SW_TILE', 'SW_PIX', 'SW_MIN_CHUNKS', 'SW_BLOCKS'))
VW_THREADS, VW_MIN_PIX, VW_BLOCKS = _define('VW_THREADS'), _define('VW_MIN_PIX'), _define('VW_BLOCKS')
EXTRA = 0                           # added to every depth: 0 for the kernels; the golden test raises it for torch's own fp32


def wide(cout, cin):
    """s1_wide: the MFMA route; a function of the channel counts only"""
    return min(cout, cin) >= MFMA_MIN_C


# ================================================================================================ depths, from the source
def dgrad_depth(cout, cin, taps):
    """s1_dgrad_mfma_kernel: SD_CHUNK / 2 `mfma_f32_32x32x2f32` per step over KH KW ceil(Cout / SD_CHUNK) steps of the
    zero-filled tiles; s1_dgrad_valu_kernel: `acc = __fmaf_rn(...)` x Cout per tap that exists.  1 product + that many
    accumulations."""
    return 1 + taps * (SD_CHUNK * -(-cout // SD_CHUNK) if wide(cout, cin) else cout) + EXTRA


def wgrad_plan(m, cout, cin, h, w, kh):
    """s1_wgrad_plan -> (chunks or pixels per split, splits)"""
    if wide(cout, cin):
        chunks = m * h * -(-w // SW_PIX)
        tiles = -(-cout // SW_TILE) * -(-cin // SW_TILE) * kh
        cps = max(SW_MIN_CHUNKS, -(-chunks // max(1, SW_BLOCKS // tiles)))
        return cps, -(-chunks // cps)
    q = m * h * w
    per = max(VW_MIN_PIX, -(-q // max(1, VW_BLOCKS // (cout * cin))))
    per = -(-per // VW_THREADS) * VW_THREADS
    return per, -(-q // per)


def wgrad_depth(m, cout, cin, h, w, kh, accumulate=False):
    """wide: one chain per split (SW_PIX accumulations per chunk, at most cps chunks); thin: a thread's chain of per /
    VW_THREADS terms, then log2(VW_THREADS) pairwise additions; s1_wgrad_combine_kernel: `tot = tot + ws[...]` x (S - 1),
    `tot + *d` under accumulate."""
    per, splits = wgrad_plan(m, cout, cin, h, w, kh)
    if wide(cout, cin):
        chain = SW_PIX * min(per, m * h * -(-w // SW_PIX))
    else:
        chain = -(-min(per, m * h * w) // VW_THREADS) + VW_THREADS.bit_length() - 1
    return 1 + chain + (splits - 1) + (1 if accumulate else 0) + EXTRA


# ===================================================================================================== float64 pieces
def _shifts(n, k, pad=None):
    """per tap index t of a size-k kernel: (t, slice of the positions p whose partner p + pad - t is inside, that slice)"""
    pad = k // 2 if pad is None else pad
    for t in range(k):
        d = pad - t
        lo, hi = max(0, -d), min(n, n - d)
        if lo < hi:
            yield t, slice(lo, hi), slice(lo + d, hi + d)


def dgrad_sum(g, w, pad=None):
    """gx[m, ci, iy, ix] = sum_{ky, kx, co} g[m, co, iy + py - ky, ix + px - kx] w[co, ci, ky, kx] over the taps inside the map"""
    m, cout, h, wd = g.shape
    kh, kw = w.shape[2:]
    py, px = (None, None) if pad is None else pad
    gx = np.zeros((m, w.shape[1], h, wd))
    for ky, iy, oy in _shifts(h, kh, py):
        for kx, ix, ox in _shifts(wd, kw, px):
            gx[:, :, iy, ix] += np.einsum('mohw,oc->mchw', g[:, :, oy, ox], w[:, :, ky, kx], optimize=True)
    return gx


def wgrad_sum(g, x, kh, kw):
    """dW[co, ci, ky, kx] = sum_{m, y, x} g[m, co, y, x] x[m, ci, y - py + ky, x - px + kx], zero outside the map"""
    dw = np.zeros((g.shape[1], x.shape[1], kh, kw))
    for ky, iy, oy in _shifts(g.shape[2], kh):         # iy: rows of x, oy = iy + py - ky: rows of g
        for kx, ix, ox in _shifts(g.shape[3], kw):
            dw[:, :, ky, kx] = np.einsum('mohw,mchw->oc', g[:, :, oy, ox], x[:, :, iy, ix], optimize=True)
    return dw


def tap_count(h, w, kh, kw):
    ty = np.array([sum(1 for _ in (1 for ky in range(kh) if 0 <= y + kh // 2 - ky < h)) for y in range(h)])
    tx = np.array([sum(1 for _ in (1 for kx in range(kw) if 0 <= x + kw // 2 - kx < w)) for x in range(w)])
    return ty[:, None] * tx[None, :]


def act_factor(a, act):
    a = f64(a)
    return {RELU: (a > 0).astype(np.float64), SIGMOID: a * (1 - a), TANH: 1 - a * a}[act]


ACT_ROUNDINGS = {NONE: 0, RELU: 0, SIGMOID: 3, TANH: 2}


def act_grad_ref(g, gb, a, act):
    """-> (g act'(a), bound); a is taken as given"""
    g = f64(g)
    gb = np.broadcast_to(np.asarray(gb, dtype=np.float64), g.shape)
    if act == NONE:
        return g, gb + 0.0
    f = act_factor(a, act)
    return g * f, (gb + gamma(ACT_ROUNDINGS[act]) * (np.abs(g) + gb)) * np.abs(f) if ACT_ROUNDINGS[act] else gb * f


def dgrad_ref(g, gb, w, add=None, addb=0.0, a=None, act=NONE):
    """-> (gx, bound) over (M, Cin, H, W); gb, addb: bounds of g and of add (scalars or arrays)"""
    g, w = f64(g), f64(w)
    cout, cin, kh, kw = w.shape
    gb = np.broadcast_to(np.asarray(gb, dtype=np.float64), g.shape)
    full = kh * kw if wide(cout, cin) else None           # the MFMA route runs every tap's steps, the vector route skips
    taps = tap_count(g.shape[2], g.shape[3], kh, kw)
    gm = np.vectorize(lambda t: gamma(dgrad_depth(cout, cin, full or int(t))))(taps)[None, None]
    with np.errstate(all='ignore'):
        ref = dgrad_sum(g, w)
        b = gm * dgrad_sum(np.abs(g), np.abs(w)) + dgrad_sum(gb, np.abs(w)) * (1 + gm)
        if add is not None:
            add = f64(add)
            b = b + np.broadcast_to(np.asarray(addb, dtype=np.float64), add.shape)
            b = b + U * (np.abs(ref) + np.abs(add) + b)
            ref = ref + add
        return act_grad_ref(ref, b, a, act)


def wgrad_ref(g, gb, x, kh, kw, xb=0.0, prev=None, prev_b=None):
    """-> (dW, its bound, db, its bound); gb, xb: bounds of g and x; prev / prev_b: what the call accumulates into"""
    g, x = f64(g), f64(x)
    gb = np.broadcast_to(np.asarray(gb, dtype=np.float64), g.shape)
    xb = np.broadcast_to(np.asarray(xb, dtype=np.float64), x.shape)
    m, cout, h, w = g.shape
    gm = gamma(wgrad_depth(m, cout, x.shape[1], h, w, kh, prev is not None))
    with np.errstate(all='ignore'):
        ref, sh = wgrad_sum(g, x, kh, kw), wgrad_sum(np.abs(g), np.abs(x), kh, kw)
        carried = wgrad_sum(gb, np.abs(x) + xb, kh, kw) + wgrad_sum(np.abs(g), xb, kh, kw)
        db, dsh, dcar = g.sum((0, 2, 3)), np.abs(g).sum((0, 2, 3)), gb.sum((0, 2, 3))
        if prev is not None:
            ref, sh = ref + f64(prev), sh + np.abs(f64(prev))
        if prev_b is not None:
            db, dsh = db + f64(prev_b), dsh + np.abs(f64(prev_b))
    return ref, gm * sh + carried * (1 + gm), db, gm * dsh + dcar * (1 + gm)


# ============================================================================================================= cases
# (M, Cout, Cin, KH, KW, H, W): every M, kernel, channel pair and map the issue names, each value of each axis several
# times and against several values of every other axis; both routes; more than one split on both routes (M = 33 at 8x8:
# 264 chunks on the MFMA route; the thin route's first 1024 pixels); a 2x3 map narrower than a 7x7's reach
MS, KERNELS = (1, 2, 3, 33), ((1, 1), (3, 3), (7, 7), (1, 5), (5, 1))
CHANNELS = ((1, 1), (1, 64), (64, 1), (2, 33), (33, 2), (31, 33), (32, 32), (64, 128))
MAPS = ((1, 1), (2, 3), (5, 7), (9, 4), (8, 8))


def _cases():
    out, i = [], 0
    for ci, ch in enumerate(CHANNELS):
        for ki, k in enumerate(KERNELS):
            out.append((MS[(ci + ki) % 4], *ch, *k, *MAPS[(ci + 2 * ki + i) % 5]))
        i += 1
    # every (M, map) and (kernel, map) pair at least once on each route
    for mi, m in enumerate(MS):
        for hi, hw in enumerate(MAPS):
            out.append((m, *CHANNELS[6 + (mi + hi) % 2], *KERNELS[(mi + hi) % 5], *hw))
            out.append((m, *CHANNELS[(mi * 5 + hi) % 6], *KERNELS[(mi + 2 * hi + 1) % 5], *hw))
    return sorted(set(out))


CASES = _cases()
# the seven real layers at M = 2, 32x32: (M, Cout, Cin, KH, KW, H, W), the act of the tensor gx belongs to
LAYERS = {'hidden': ((2, 512, 128, 3, 3, 32, 32), NONE), 'flow_predict': ((2, 2, 256, 3, 3, 32, 32), RELU),
          'mask_predict': ((2, 1, 256, 1, 1, 32, 32), RELU), 'delta_flow_encoder.0': ((2, 128, 2, 7, 7, 32, 32), NONE),
          'delta_flow_encoder.1': ((2, 64, 128, 3, 3, 32, 32), RELU), 'mask_encoder.0': ((2, 64, 1, 3, 3, 32, 32), SIGMOID),
          'mask_encoder.1': ((2, 32, 64, 3, 3, 32, 32), RELU)}
REGIMES = ['nominal', 'cancelling', 'offset', 'scaled']
SCALES = (40, 20)                            # powers of two on g and on the other operand
REGIME_CASES = [(3, 64, 128, 3, 3, 5, 7), (33, 32, 32, 1, 5, 8, 8), (2, 31, 33, 7, 7, 2, 3), (33, 2, 33, 5, 1, 9, 4)]


def conv_case(regime, m, cout, cin, kh, kw, h, w, seed=0):
    """g (M, Cout, H, W) cotangent, weight (Cout, Cin, KH, KW), x (M, Cin, H, W) post-ReLU operand, add (M, Cin, H, W) second
    cotangent, a (M, Cin, H, W) in (0, 1) with exact zeros (a post-activation value for every act), scale of the results"""
    gen = torch.Generator().manual_seed(7700 + seed + m + 3 * cout + 7 * cin + 11 * h + 13 * w + 17 * kh + 19 * kw)
    g = torch.randn((m, cout, h, w), generator=gen)
    wt = torch.randn((cout, cin, kh, kw), generator=gen) * (kh * kw * cout) ** -0.5
    x = torch.relu(torch.randn((m, cin, h, w), generator=gen))
    add = torch.randn((m, cin, h, w), generator=gen)
    a = torch.relu(torch.rand((m, cin, h, w), generator=gen) * 1.25 - 0.25)
    if regime == 'cancelling':               # halves of the contraction cancel to 1e-4 of the shadow (dgrad: co, wgrad: m)
        hh = cout // 2
        if hh:
            g[:, hh:2 * hh] = g[:, :hh]
            wt[hh:2 * hh] = -wt[:hh] * (1 + 1e-4 * torch.randn(wt[:hh].shape, generator=gen))
        hm = m // 2
        if hm:
            x[hm:2 * hm] = x[:hm]
            g[hm:2 * hm] = -g[:hm] * (1 + 1e-4 * torch.randn(g[:hm].shape, generator=gen))
    if regime == 'offset':
        g, wt, x = g + 2.0, wt + 1.0, x + 4.0
    scale = 1.0
    if regime == 'scaled':
        g, wt, x, add = g * 2.0 ** SCALES[0], wt * 2.0 ** SCALES[1], x * 2.0 ** SCALES[1], add * 2.0 ** (SCALES[0] + SCALES[1])
        scale = 2.0 ** (SCALES[0] + SCALES[1])
    return g.contiguous(), wt.contiguous(), x.contiguous(), add.contiguous(), a.contiguous(), scale


# ================================================================================ fp32 emulations in the kernels' order
def act_fp32(v, a, act, defect=None):
    if act == NONE:
        return v
    if act == RELU:
        return torch.where(a > 0, v, torch.zeros_like(v))
    if act == SIGMOID:
        return v * a if defect == 'sigmoid_factor_a' else v * (a * (1.0 - a))
    return v * fma(-a, a, torch.ones_like(a))


def dgrad_fp32(g, w, add=None, a=None, act=NONE, defect=None):
    """both dgrad kernels: taps in ascending (ky, kx), co ascending inside a tap, one fma chain from +0 (a tap outside the
    map: zeros on the MFMA route, skipped on the vector route -- the same value); + add; the factor"""
    m, cout, h, wd = g.shape
    cin, kh, kw = w.shape[1:]
    if defect == 'ci_co_exchanged':
        w = w.reshape(cin, cout, kh, kw).permute(1, 0, 2, 3)           # the (Cout, Cin) buffer indexed [ci][co]
    if defect == 'taps_not_flipped_y':
        w = w.flip(2)
    if defect == 'taps_not_flipped_x':
        w = w.flip(3)
    py, px = kh // 2, kw // 2
    if defect == 'pad_x_for_y':
        py = px
    gp = F.pad(g, (kw, kw, max(kh, kw), max(kh, kw)))
    acc = torch.zeros((m, cin, h, wd))
    for ky in range(kh):
        for kx in range(kw):
            y0, x0 = max(kh, kw) + py - ky, kw + px - kx
            gt = gp[:, :, y0:y0 + h, x0:x0 + wd]
            for co in range(cout):
                acc = fma(gt[:, co, None], w[co, :, ky, kx][None, :, None, None], acc)
    if defect == 'add_after_factor':
        return act_fp32(acc, a, act) + add
    if add is not None:
        acc = acc + add
    return act_fp32(acc, a, act, defect)


def wgrad_fp32(g, x, kh, kw, prev=None, prev_b=None, defect=None):
    """s1_wgrad_{mfma,valu}_kernel + combine -> (dW, db): per split the route's order; partial 0, + partial 1 ..., + the
    previous value last"""
    m, cout, h, wd = g.shape
    cin = x.shape[1]
    per, splits = wgrad_plan(m, cout, cin, h, wd, kh)
    xp = F.pad(x, (kw // 2, kw // 2, kh // 2, kh // 2))
    tot, totb = None, None
    for s in range(splits):
        if wide(cout, cin):
            segs = -(-wd // SW_PIX)
            acc, accb = torch.zeros((cout, cin, kh, kw)), torch.zeros((cout,))
            for c in range(s * per, min((s + 1) * per, m * h * segs)):
                seg, y, mm = c % segs, (c // segs) % h, c // (segs * h)
                for xx in range(seg * SW_PIX, min((seg + 1) * SW_PIX, wd)):
                    acc = fma(g[mm, :, y, xx][:, None, None, None], xp[mm, :, y:y + kh, xx:xx + kw][None], acc)
                    accb = accb + g[mm, :, y, xx]
        else:
            q0, q1 = s * per, min((s + 1) * per, m * h * wd)
            acc, accb = torch.zeros((VW_THREADS, cout, cin, kh, kw)), torch.zeros((VW_THREADS, cout))
            for k in range(-(-(q1 - q0) // VW_THREADS)):
                q = q0 + VW_THREADS * k + torch.arange(VW_THREADS)
                ok = (q < q1)
                qc = q.clamp(max=q1 - 1)
                xx, y, mm = qc % wd, (qc // wd) % h, qc // (wd * h)
                gq = g[mm, :, y, xx] * ok[:, None]                                      # (T, Cout); +0 past the end: no change
                idx_y = y[:, None] + torch.arange(kh)[None]
                idx_x = xx[:, None] + torch.arange(kw)[None]
                xq = xp[mm[:, None, None], :, idx_y[:, :, None], idx_x[:, None, :]]     # (T, KH, KW, Cin)
                acc = fma(gq[:, :, None, None, None], xq.permute(0, 3, 1, 2)[:, None], acc)
                accb = accb + gq
            k = VW_THREADS // 2
            while k >= 1:
                acc, accb = acc[:k] + acc[k:2 * k], accb[:k] + accb[k:2 * k]
                k //= 2
            acc, accb = acc[0], accb[0]
        tot = acc if tot is None else tot + acc
        if not (defect == 'db_missing_split' and s == splits - 1 and splits > 1):
            totb = accb if totb is None else totb + accb
    if prev is None or defect == 'accumulate_overwrites':
        return tot, totb
    return tot + prev, totb + prev_b


# ===================================================================================================== the self-checks
def test_symbols_are_declared_exported_and_bound():
    from scflow_amd import _lib, ops
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'scflow_hip.h')).read()
    for name in ('scf_conv_s1_dgrad', 'scf_conv_s1_wgrad', 'scf_conv_s1_wgrad_workspace', 'scf_act_grad'):
        assert re.search(rf'\b{name}\s*\(', header), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert all(hasattr(ops, n) for n in ('conv_s1_dgrad', 'conv_s1_wgrad', 'conv_s1_wgrad_workspace', 'act_grad'))


def test_depths_and_plan_are_the_counts_of_the_source():
    from scflow_amd import _lib
    lib = _lib.load()
    assert (MFMA_MIN_C, SD_CHUNK, SW_TILE, SW_PIX, SW_MIN_CHUNKS, SW_BLOCKS) == (32, 32, 64, 16, 16, 1024)
    assert (VW_THREADS, VW_MIN_PIX, VW_BLOCKS) == (256, 1024, 2048)
    assert [dgrad_depth(*c) for c in ((1, 1, 1), (33, 40, 9), (2, 256, 6), (512, 128, 9))] == [2, 577, 13, 4609]
    assert wgrad_plan(256, 512, 128, 32, 32, 3) == (781, 21) and wgrad_plan(2, 64, 128, 32, 32, 3) == (16, 8)
    assert wgrad_plan(256, 2, 256, 32, 32, 3) == (65536, 4) and wgrad_plan(1, 1, 1, 1, 1, 1) == (1024, 1)
    assert wgrad_depth(33, 31, 33, 8, 8, 3) == 1 + 5 + 8 + 1 and wgrad_depth(2, 64, 128, 32, 32, 3, True) == 1 + 256 + 7 + 1
    shapes = CASES + [v[0] for v in LAYERS.values()] + [(256,) + v[0][1:] for v in LAYERS.values()]
    for m, cout, cin, kh, kw, h, w in shapes:
        want = wgrad_plan(m, cout, cin, h, w, kh)[1] * (kh * kw * cout * cin + cout)
        assert lib.scf_conv_s1_wgrad_workspace(m, cout, cin, h, w, kh, kw) == want
    for bad in ((0, 1, 1, 1, 1, 3, 3), (1, 1, 1, 0, 1, 3, 3), (1, 1, 1, 1, 1, 2, 3), (1, 1, 1, 1, 1, 3, 9), (1, 1, 1, 1, 1, 0, 1)):
        assert lib.scf_conv_s1_wgrad_workspace(*bad) == -1


def test_cases_cover_every_value_of_every_axis_and_both_routes():
    assert {c[0] for c in CASES} == set(MS) and {c[1:3] for c in CASES} == set(CHANNELS)
    assert {c[3:5] for c in CASES} == set(KERNELS) and {c[5:] for c in CASES} == set(MAPS)
    assert {(c[1:3], c[3:5]) for c in CASES} >= {(ch, k) for ch in CHANNELS for k in KERNELS}
    assert {(c[0], c[5:], wide(*c[1:3])) for c in CASES} >= {(m, hw, r) for m in MS for hw in MAPS for r in (False, True)}
    assert any(wgrad_plan(*c[:3], *c[5:], c[3])[1] > 1 and wide(*c[1:3]) for c in CASES)
    assert any(wgrad_plan(*c[:3], *c[5:], c[3])[1] > 1 and not wide(*c[1:3]) for c in CASES)
    assert [wide(*v[0][1:3]) for v in LAYERS.values()] == [True, False, False, False, True, False, True]


def _torch_grads(g, w, x, bias=True):
    xt, wt = torch.from_numpy(x).requires_grad_(), torch.from_numpy(w).requires_grad_()
    bt = torch.zeros(w.shape[0], dtype=torch.float64, requires_grad=True)
    y = F.conv2d(xt, wt, bt, padding=(w.shape[2] // 2, w.shape[3] // 2))
    (y * torch.from_numpy(g)).sum().backward()
    return xt.grad.numpy(), wt.grad.numpy(), bt.grad.numpy()


def test_index_sums_equal_float64_autograd():
    worst = 0.0
    for case in CASES[::3] + REGIME_CASES:
        g, w, x, _, _, _ = conv_case('nominal', *case)
        g, w, x = f64(g), f64(w), f64(x)
        gx, dw, db = _torch_grads(g, w, x)
        for got, ref in ((dgrad_sum(g, w), gx), (wgrad_sum(g, x, *case[3:5]), dw), (g.sum((0, 2, 3)), db)):
            worst = max(worst, float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300)))
    measured('index sums against float64 autograd, relative', worst)
    assert worst <= 1e-13


EMU_CASES = [(3, 64, 128, 3, 3, 5, 7), (33, 32, 32, 1, 5, 8, 8), (2, 31, 33, 7, 7, 2, 3), (33, 2, 33, 5, 1, 9, 4), (33, 33, 2, 3, 3, 8, 8),
             (1, 1, 1, 1, 1, 1, 1), (2, 1, 64, 1, 1, 9, 4)]


def _worst(defect=None, acts=ACTS, cases=None, regimes=('nominal',)):
    worst = 0.0
    for case in cases or EMU_CASES:
        kh, kw = case[3:5]
        for regime in regimes:
            g, w, x, add, a, _ = conv_case(regime, *case)
            if defect in (None, 'ci_co_exchanged', 'taps_not_flipped_y', 'taps_not_flipped_x', 'pad_x_for_y', 'add_after_factor',
                          'sigmoid_factor_a'):
                for act in acts:
                    for ad in ((None, add) if defect is None else (add,)):
                        aa = a if act != NONE else None
                        got = dgrad_fp32(g, w, ad, aa, act, defect)
                        worst = max(worst, worst_ratio(got, *dgrad_ref(g, 0.0, w, ad, 0.0, aa, act)))
            if defect in (None, 'db_missing_split', 'accumulate_overwrites'):
                gen = torch.Generator().manual_seed(1)
                prev, prev_b = torch.randn(w.shape, generator=gen), torch.randn(w.shape[0], generator=gen)
                for pv, pb in (((None, None), (prev, prev_b)) if defect != 'accumulate_overwrites' else ((prev, prev_b),)):
                    dw, db = wgrad_fp32(g, x, kh, kw, pv, pb, defect)
                    ref, bw, rb, bb = wgrad_ref(g, 0.0, x, kh, kw, prev=pv, prev_b=pb)
                    worst = max(worst, worst_ratio(dw, ref, bw), worst_ratio(db, rb, bb))
    return worst


def test_emulations_inside_the_bounds():
    v = _worst(regimes=REGIMES)
    measured('fp32 emulations in the kernels\' order, error / bound', v)
    assert v <= 1.0


DEFECTS = {'ci_co_exchanged': dict(cases=[(3, 64, 128, 3, 3, 5, 7)], acts=(NONE,)),
           'taps_not_flipped_y': dict(cases=[(2, 31, 33, 7, 7, 2, 3), (33, 2, 33, 5, 1, 9, 4)], acts=(NONE,)),
           'taps_not_flipped_x': dict(cases=[(33, 32, 32, 1, 5, 8, 8)], acts=(NONE,)),
           'pad_x_for_y': dict(cases=[(33, 32, 32, 1, 5, 8, 8)], acts=(NONE,)),
           'add_after_factor': dict(cases=[(3, 64, 128, 3, 3, 5, 7)], acts=(RELU, SIGMOID, TANH)),
           'sigmoid_factor_a': dict(cases=[(33, 2, 33, 5, 1, 9, 4)], acts=(SIGMOID,)),
           'db_missing_split': dict(cases=[(33, 32, 32, 1, 5, 8, 8), (33, 33, 2, 3, 3, 8, 8)]),
           'accumulate_overwrites': dict(cases=[(3, 64, 128, 3, 3, 5, 7), (2, 1, 64, 1, 1, 9, 4)])}


@pytest.mark.parametrize('defect', sorted(DEFECTS))
def test_planted_defects_outside(defect):
    for case in DEFECTS[defect]['cases']:
        v = _worst(defect, cases=[case], acts=DEFECTS[defect].get('acts', ACTS))
        measured(f'defect {defect} {case} / bound', v)
        assert v > 1.0


def test_accumulate_is_one_more_rounding():
    case = (3, 64, 128, 3, 3, 5, 7)
    assert wgrad_depth(*case[:3], *case[5:], 3, True) == wgrad_depth(*case[:3], *case[5:], 3) + 1


# ================================================================================================== the composed stage
HEAD_NAMES = [f'{m}.{p}' for m in ('flow_pred.layers.0.conv', 'flow_pred.predict_layer', 'mask_pred.layers.0.conv',
                                   'mask_pred.predict_layer', 'delta_flow_encoder.0.conv', 'delta_flow_encoder.1.conv',
                                   'mask_encoder.0.conv', 'mask_encoder.1.conv') for p in ('weight', 'bias')]
REAL_WIDTHS = dict(hc=128, ch=256, d1=128, df=64, m1=64, mf=32)
HEAD_KERNELS = {'flow_pred.layers.0.conv': (3, 3), 'flow_pred.predict_layer': (3, 3), 'mask_pred.layers.0.conv': (3, 3),
                'mask_pred.predict_layer': (1, 1), 'delta_flow_encoder.0.conv': (7, 7), 'delta_flow_encoder.1.conv': (3, 3),
                'mask_encoder.0.conv': (3, 3), 'mask_encoder.1.conv': (3, 3)}


def head_shapes(wd):
    io = {'flow_pred.layers.0.conv': (wd['ch'], wd['hc']), 'flow_pred.predict_layer': (2, wd['ch']),
          'mask_pred.layers.0.conv': (wd['ch'], wd['hc']), 'mask_pred.predict_layer': (1, wd['ch']),
          'delta_flow_encoder.0.conv': (wd['d1'], 2), 'delta_flow_encoder.1.conv': (wd['df'], wd['d1']),
          'mask_encoder.0.conv': (wd['m1'], 1), 'mask_encoder.1.conv': (wd['mf'], wd['m1'])}
    return {k: io[k] + HEAD_KERNELS[k] for k in io}


def head_params(wd, seed=0):
    gen = torch.Generator().manual_seed(4400 + seed)
    p = {}
    for k, s in head_shapes(wd).items():
        p[f'{k}.weight'] = f64(torch.randn(s, generator=gen) * (s[1] * s[2] * s[3]) ** -0.5)
        p[f'{k}.bias'] = f64(torch.randn(s[0], generator=gen) * 0.1)
    return p


def _act64(v, enc_act):
    return torch.relu(v) if enc_act == RELU else v


def head_forward_torch(hv, p, enc_act):
    """the plain-torch stage: hv -> dict(heads, d_flow, logit, mask, d1, m1, dm), differentiable"""
    conv = lambda x, k: F.conv2d(x, p[f'{k}.weight'], p[f'{k}.bias'], padding=(p[f'{k}.weight'].shape[2] // 2,) * 2)  # noqa: E731
    heads = torch.relu(torch.cat([conv(hv, 'flow_pred.layers.0.conv'), conv(hv, 'mask_pred.layers.0.conv')], 1))
    ch = p['flow_pred.layers.0.conv.weight'].shape[0]
    d_flow = conv(heads[:, :ch], 'flow_pred.predict_layer')
    logit = conv(heads[:, ch:], 'mask_pred.predict_layer')
    mask = torch.sigmoid(logit)
    d1 = _act64(conv(d_flow, 'delta_flow_encoder.0.conv'), enc_act)
    m1 = _act64(conv(mask, 'mask_encoder.0.conv'), enc_act)
    dm = torch.cat([_act64(conv(d1, 'delta_flow_encoder.1.conv'), enc_act), _act64(conv(m1, 'mask_encoder.1.conv'), enc_act)], 1)
    return dict(heads=heads, d_flow=d_flow, logit=logit, mask=mask, d1=d1, m1=m1, dm=dm)


def heads_ref64(saved, p, g_hv, g_dm, g_df, g_mk, enc_act, prev=None, defect=None, bounds=False, xbounds=None):
    """SCFlowDecoder.heads_backward in float64 GIVEN the activations ``saved`` (hv, heads, d_flow, mask, d1, m1, dm over the
    stacked samples): -> dict of g_hidden, g_delta_flow_total, g_mask_logit and the 16 parameter gradients; with
    ``bounds`` a second dict, the composed per-element bounds (each stage's bound carried into the next; ``xbounds``: bounds
    of the activations as wgrad operands, by their key in ``saved``)"""
    s = {k: f64(v) for k, v in saved.items()}
    p = {k: f64(v) for k, v in p.items()}
    ch = p['flow_pred.layers.0.conv.weight'].shape[0]
    c_df = p['delta_flow_encoder.1.conv.weight'].shape[0]
    ref, bnd = {}, {}

    xb_of = lambda k, sl=slice(None): 0.0 if xbounds is None else f64(xbounds[k])[:, sl]      # noqa: E731

    def wgrad(name, g, gb, x, xb=0.0):
        kh, kw = p[f'{name}.weight'].shape[2:]
        pv = None if prev is None else prev[f'{name}.weight']
        pb = None if prev is None else prev[f'{name}.bias']
        ref[f'{name}.weight'], bnd[f'{name}.weight'], ref[f'{name}.bias'], bnd[f'{name}.bias'] = wgrad_ref(
            g, gb, x, kh, kw, xb=xb, prev=pv, prev_b=pb)

    g_dm = f64(g_dm)
    u, ub = act_grad_ref(g_dm, 0.0, s['dm'], enc_act)
    u_df, ub_df = u[:, :c_df], ub[:, :c_df]
    u_mf, ub_mf = (u[:, :u.shape[1] - c_df], ub[:, :u.shape[1] - c_df]) if defect == 'slice_offset_ignored' else (u[:, c_df:], ub[:, c_df:])
    a_ = lambda v: v if enc_act != NONE else None          # noqa: E731
    wgrad('delta_flow_encoder.1.conv', u_df, ub_df, s['d1'], xb_of('d1'))
    mask_d1 = np.broadcast_to(s['m1'][:, :1], s['d1'].shape) if defect == 'mask_from_wrong_layer' else s['d1']
    g_d1, b_d1 = dgrad_ref(u_df, ub_df, p['delta_flow_encoder.1.conv.weight'], a=a_(mask_d1), act=enc_act)
    wgrad('mask_encoder.1.conv', u_mf, ub_mf, s['m1'], xb_of('m1'))
    g_m1, b_m1 = dgrad_ref(u_mf, ub_mf, p['mask_encoder.1.conv.weight'], a=a_(s['m1']), act=enc_act)
    wgrad('delta_flow_encoder.0.conv', g_d1, b_d1, s['d_flow'], xb_of('d_flow'))
    ref['g_delta_flow_total'], bnd['g_delta_flow_total'] = dgrad_ref(g_d1, b_d1, p['delta_flow_encoder.0.conv.weight'], add=g_df)
    wgrad('mask_encoder.0.conv', g_m1, b_m1, s['mask'], xb_of('mask'))
    ref['g_mask_logit'], bnd['g_mask_logit'] = dgrad_ref(g_m1, b_m1, p['mask_encoder.0.conv.weight'], add=g_mk, a=s['mask'],
                                                        act=SIGMOID)
    gt, bt, gl, bl = ref['g_delta_flow_total'], bnd['g_delta_flow_total'], ref['g_mask_logit'], bnd['g_mask_logit']
    wgrad('flow_pred.predict_layer', gt, bt, s['heads'][:, :ch], xb_of('heads', slice(0, ch)))
    wgrad('mask_pred.predict_layer', gl, bl, s['heads'][:, ch:], xb_of('heads', slice(ch, None)))
    hf, hm = s['heads'][:, :ch], s['heads'][:, ch:]
    if defect == 'relu_mask_of_other_head':
        hf, hm = hm, hf
    uf, ufb = dgrad_ref(gt, bt, p['flow_pred.predict_layer.weight'], a=hf, act=RELU)
    um, umb = dgrad_ref(gl, bl, p['mask_pred.predict_layer.weight'], a=hm, act=RELU)
    g_heads, b_heads = np.concatenate([uf, um], 1), np.concatenate([ufb, umb], 1)
    w_h = np.concatenate([p['flow_pred.layers.0.conv.weight'], p['mask_pred.layers.0.conv.weight']], 0)
    names = ['flow_pred.layers.0.conv', 'mask_pred.layers.0.conv']
    pv = None if prev is None else np.concatenate([f64(prev[f'{k}.weight']) for k in names], 0)
    pb = None if prev is None else np.concatenate([f64(prev[f'{k}.bias']) for k in names], 0)
    dw, bw, db, bb = wgrad_ref(g_heads, b_heads, s['hv'], 3, 3, prev=pv, prev_b=pb)
    if defect == 'hidden_rows_to_wrong_head':
        names = names[::-1]
    for k, rows in zip(names, (slice(0, ch), slice(ch, None))):
        ref[f'{k}.weight'], bnd[f'{k}.weight'], ref[f'{k}.bias'], bnd[f'{k}.bias'] = dw[rows], bw[rows], db[rows], bb[rows]
    ref['g_hidden'], bnd['g_hidden'] = dgrad_ref(g_heads, b_heads, w_h, add=g_hv)
    return (ref, bnd) if bounds else ref


SMALL_WIDTHS = dict(hc=6, ch=5, d1=4, df=3, m1=3, mf=2)


def stage_case(wd, m, h, w, enc_act, seed=0):
    """float64 parameters, activations by the plain-torch stage, the four cotangents"""
    gen = torch.Generator().manual_seed(5500 + seed + m + 3 * h + 5 * w)
    p = head_params(wd, seed)
    hv = torch.tanh(torch.randn((m, wd['hc'], h, w), generator=gen, dtype=torch.float64))
    cot = [torch.randn((m, c, h, w), generator=gen, dtype=torch.float64) for c in (wd['hc'], wd['df'] + wd['mf'], 2, 1)]
    return p, hv, cot


@pytest.mark.parametrize('enc_act', [RELU, NONE], ids=['relu', 'none'])
@pytest.mark.parametrize('hw', [(5, 7), (2, 3)], ids=lambda v: f'{v[0]}x{v[1]}')
def test_composed_stage_equals_float64_autograd(hw, enc_act):
    p, hv, (g_hv, g_dm, g_df, g_mk) = stage_case(SMALL_WIDTHS, 3, *hw, enc_act)
    pt = {k: torch.from_numpy(v).requires_grad_() for k, v in p.items()}
    hvt = hv.clone().requires_grad_()
    fw = head_forward_torch(hvt, pt, enc_act)
    fw['d_flow'].retain_grad()
    fw['logit'].retain_grad()
    ((fw['dm'] * g_dm).sum() + (fw['d_flow'] * g_df).sum() + (fw['mask'] * g_mk).sum() + (hvt * g_hv).sum()).backward()
    want = {k: v.grad for k, v in pt.items()}
    want.update(g_hidden=hvt.grad, g_delta_flow_total=fw['d_flow'].grad, g_mask_logit=fw['logit'].grad)
    saved = {k: v.detach() for k, v in fw.items()}
    saved['hv'] = hv
    ref = heads_ref64(saved, p, g_hv, g_dm, g_df, g_mk, enc_act)
    assert set(ref) == set(want) == set(HEAD_NAMES) | {'g_hidden', 'g_delta_flow_total', 'g_mask_logit'}
    worst = max(float(np.abs(ref[k] - f64(want[k])).max() / np.abs(f64(want[k])).max()) for k in want)
    measured(f'composed stage against float64 autograd {hw}, relative', worst)
    assert worst <= 1e-12


STAGE_DEFECTS = ['mask_from_wrong_layer', 'relu_mask_of_other_head', 'hidden_rows_to_wrong_head', 'slice_offset_ignored']


@pytest.mark.parametrize('defect', STAGE_DEFECTS)
def test_planted_stage_defects_outside(defect):
    wd = dict(hc=6, ch=5, d1=4, df=3, m1=3, mf=3)             # df == mf: a slice read at offset 0 has the right shape
    p, hv, (g_hv, g_dm, g_df, g_mk) = stage_case(wd, 3, 5, 7, RELU)
    saved = {k: v.detach() for k, v in head_forward_torch(hv, {k: torch.from_numpy(v) for k, v in p.items()}, RELU).items()}
    saved['hv'] = hv
    ref, bnd = heads_ref64(saved, p, g_hv, g_dm, g_df, g_mk, RELU, bounds=True)
    bad = heads_ref64(saved, p, g_hv, g_dm, g_df, g_mk, RELU, defect=defect)
    worst = max(worst_ratio(bad[k], ref[k], bnd[k]) for k in ref)
    measured(f'stage defect {defect} / composed bound', worst)
    assert worst > 1.0


# ======================================================================= the reference's own heads and encoders (fixture)
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'head_grads.npz')
GOLDEN_MAPS = [(6, 5), (8, 8)]
GOLDEN_N = 2
GOLDEN_SEED = 20252
GOLDEN_H_CHANNELS = [0, 64, 127]                 # channels of d loss / d h that are stored
GOLDEN_KEYS = HEAD_NAMES + ['g_hidden', 'g_delta_flow_total', 'g_mask_logit']


def golden_case(hw):
    """-> (tag, the 16 parameters, h, the cotangents at h, cat(dff, mf), d_flow, sigmoid(mask)) as float32 tensors, from the seeds"""
    from test_fc_grad_host import golden_param
    tag = f'{hw[0]}x{hw[1]}'
    shapes = head_shapes(REAL_WIDTHS)
    p = {}
    for k, s_ in shapes.items():
        p[f'{k}.weight'] = golden_param(f'{k}.weight', s_, GOLDEN_SEED)
        p[f'{k}.bias'] = golden_param(f'{k}.bias', s_[:1], GOLDEN_SEED)
    x = lambda name, c: golden_param(f'{name}.{tag}', (GOLDEN_N, c, *hw), GOLDEN_SEED, scale=1.0)      # noqa: E731
    return tag, p, x('h', 128), (x('c_h', 128), x('c_dm', 96), x('c_df', 2), x('c_mk', 1))


def golden_pick(key, v):
    """the part of a full gradient the fixture stores: of a large weight the first and the last output channel, of a still
    large one every fourth input channel of those"""
    if key == 'g_hidden':
        return v[:, GOLDEN_H_CHANNELS]
    if v.ndim == 4 and v.size > 2048 and key.endswith('weight'):
        v = v[[0, v.shape[0] - 1]]
        if v.size > 2048:
            v = v[:, ::4]
    return v


def golden_reference(hw):
    """The float64 backward on the fixture's inputs GIVEN the fp32 forward, and the room around it for an fp32 backward by
    torch -> (tag, reference dict, room dict).

    The forward (heads, d_flow, mask, d1, m1, dm) is recomputed here in fp32 by the operators the reference's modules call
    (F.conv2d, relu, sigmoid) and enters as given, the way the kernels' kept and recomputed activations enter
    tests/test_gpu_head_grad.py.  The room is the kernels' composed bound (heads_ref64 with ``bounds``) with EVERY depth
    raised by torch's longest fp32 chain (9 * 256 products of the flow head's predict layer) and, on the wgrad operands,
    twice the forward's own rounding bound gamma_{KH KW Cin + 1 + longest} (sum |x| |w| + |b|) per layer: a host whose fp32
    convolution adds in another order than the fixture's differs from it by at most that.  The term is NOT carried through
    the later layers of the forward (the same choice as tests/test_conv_grad_host.py::golden_reference); the raised depths
    leave room for it: the test prints where the reference sits."""
    import test_head_grad_host as me
    tag, p, hv, cots = golden_case(hw)
    with torch.no_grad():
        fw = head_forward_torch(hv, p, RELU)
    saved = {k: v for k, v in fw.items() if k != 'logit'}
    saved['hv'] = hv
    longest = 9 * 256
    ch = REAL_WIDTHS['ch']

    def fwd_bound(x, names):
        out = []
        for k in names:
            w_, b_ = f64(p[f'{k}.weight']), f64(p[f'{k}.bias'])
            sh = dgrad_sum(np.abs(f64(x)), np.abs(w_).transpose(1, 0, 2, 3)[:, :, ::-1, ::-1]) + np.abs(b_)[None, :, None, None]
            out.append(2.0 * gamma(w_[0].size + 1 + longest) * sh)
        return np.concatenate(out, 1)

    xb = dict(heads=fwd_bound(hv, ['flow_pred.layers.0.conv', 'mask_pred.layers.0.conv']),
              d_flow=fwd_bound(fw['heads'][:, :ch], ['flow_pred.predict_layer']),
              mask=0.25 * fwd_bound(fw['heads'][:, ch:], ['mask_pred.predict_layer']) + 4 * U,       # |sigmoid'| <= 1 / 4
              d1=fwd_bound(fw['d_flow'], ['delta_flow_encoder.0.conv']), m1=fwd_bound(fw['mask'], ['mask_encoder.0.conv']))
    old = me.EXTRA
    me.EXTRA = longest
    try:
        ref, room = heads_ref64(saved, p, *cots, RELU, bounds=True, xbounds=xb)
    finally:
        me.EXTRA = old
    return tag, ref, room


@pytest.mark.parametrize('hw', GOLDEN_MAPS, ids=lambda v: f'{v[0]}x{v[1]}')
def test_reference_autograd_agrees_with_the_restatement(hw):
    """The reference's fp32 gradients (autograd through its own XHeads and make_delta_flow_encoder stacks) against the
    float64 stage.  The room is the kernels' composed bound PLUS torch's own fp32 terms (golden_reference); it is for the
    reference's fp32 alone and never granted to the kernels' own checks."""
    z = np.load(GOLDEN)
    tag, ref, room = golden_reference(hw)
    for key in GOLDEN_KEYS:
        v = worst_ratio(z[f'{tag}.{key}'], golden_pick(key, ref[key]), golden_pick(key, room[key]))
        measured(f'reference heads autograd {tag} {key}, error / (kernels\' bound + torch fp32 terms)', v)
        assert v <= 1.0, key
        rel = float(np.abs(z[f'{tag}.{key}'] - golden_pick(key, ref[key])).max() / np.abs(golden_pick(key, ref[key])).max())
        measured(f'reference heads autograd {tag} {key}, error relative to the largest entry', rel)
    assert os.path.getsize(GOLDEN) < 100 * 1024
