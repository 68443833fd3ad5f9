"""CPU: the pose head's fully connected tail -- scf_fc_splitk (fc.hip: split-K fp32 MFMA GEMM, 32 x 32 tiles, the
neighbouring bias / ReLU / GroupNorm folded into the operand load, two weight matrices in one launch) and scf_linear /
scf_linear_pair (norm.hip: wave-per-feature GEMV) -- restated in float64 with a per-element error bound for any fp32
evaluation in the kernel's operation order, the inputs tests/test_gpu_fc.py feeds the HIP kernels, fp32 emulations in
the kernels' order with planted defects, and the proof that the bounds are neither vacuous nor unreachable.  The helpers
(U, f64, worst_ratio, measured, norm_core, ...) are those of tests/test_stream_ops_host.py.

The operand a GEMM contracts is a fixed function of the inputs: the IN-ORDER fp32 sum of the parts, + x_bias in fp32,
ReLU.  These are IEEE additions with nothing to contract, so `fc_operand` gives the kernel's own bits (the argument of
gn_sum_parts) and carries no bound.  Everything after it is float64 with a bound:

  GroupNorm   norm_core with chain depth gn_size / 2 + 1 (FC_GN_DEPTH), then the product with gamma and the addition
              of beta as in group_norm_relu_ref.
  GEMM        gamma_d (sum_k |W| |x|  [+ |bias|])  +  sum_k |W| . (operand bound) (1 + gamma_d),   gamma_d = d U / (1 - d U)
              with d = FC_DEPTH(KS) for fc_splitk (per slice for partial outputs) and LINEAR_DEPTH(K) for scf_linear.
              v_mfma_f32_32x32x2_f32 may round less often than once per product and once per accumulation; it never
              rounds more often, so d is an upper bound -- as with fma contraction elsewhere.
  activation  ReLU: exact and 1-Lipschitz.  sigmoid = 1 / (1 + expf(-v)): Lipschitz 1 / 4, then expf (EXP_ULPS, ASSUMED
              as in test_stream_ops_host), the addition and the division: (2 EXP_ULPS + 3) U relative.  tanhf:
              1-Lipschitz, TANH_ULPS = 2 ASSUMED for the device library's tanhf (no error is stated for it either).

Underflow is outside the model: every case keeps its products and sums above 2**-100 (the `scaled` regime multiplies
nominal O(1e-4 .. 1) products by 2**-50 at the least).
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_stream_ops_host import (EXP_ULPS, IN_EPS, U, f64, measured, norm_core, same_bits, same_nan_pattern,  # noqa: E402
                                  worst_ratio)

ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH = 0, 1, 2, 3
ACTS = [ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH]
TANH_ULPS = 2.0                     # assumed (module docstring)
# the kernels' ReLU forms -- fmaxf(v, 0) in fc_splitk's operand load and its GroupNorm, v > 0 ? v : 0 in scf_apply_act --
# return 0 for NaN where torch.relu returns NaN.  Pinned by tests/test_gpu_fc.py, described in DESIGN.md.
KERNEL_RELU_OF_NAN = 0.0


# ================================================================================================ depths, from the source
def fc_layout(ks):
    """scf_fc_splitk: `const int KS = Ks <= 64 ? 64 : Ks <= 128 ? 128 : 256`"""
    return 64 if ks <= 64 else 128 if ks <= 128 else 256


def fc_depth(ks, bias=True):
    """fc_splitk_kernel<KS>, the longest chain of roundings a product passes through:
      `acc = mfma_f32_32x32x2f32(a, b, acc)` x KS / 8 per wave, two columns each:  1 product
                                                                                   + KS / 4 accumulations
      `((red[0] + red[1]) + red[2]) + red[3]`:                                     + 3 wave additions
      `if (bias) s += bias[o0 + m]` (finished outputs only):                       + 1"""
    return 1 + fc_layout(ks) // 4 + 3 + (1 if bias else 0)


def fc_gn_depth(gn_size):
    """fc_group_norm_half<32> and the generic loop: `for (i < hsz) s += xp[i]` (gn_size / 2 serial additions per
    thread), `s += __shfl_xor(s, 1)` (+ 1)."""
    return gn_size // 2 + 1


def linear_depth(k, bias=True):
    """linear_kernel.  float4 path (K % 4 == 0): `acc += (w.x x.x + w.y x.y) + (w.z x.z + w.w x.w)` -- 1 product, 2 levels
    of the four-term group, one accumulation per piece, ceil(K / 256) pieces per lane (trips of four); scalar path:
    `acc += w * x`, ceil(K / 64) per lane.  Then `wave_sum`: 6 levels, then `s + b[o]`: 1 (`+ 0.f` without bias: exact)."""
    chain = 1 + 2 + -(-k // 256) if k % 4 == 0 else 1 + -(-k // 64)
    return chain + 6 + (1 if bias else 0)


def gamma(d):
    return d * U / (1 - d * U)


# ===================================================================================================== float64 pieces
def gemm_ref(xop, xb, w, bias, depth, slices=1):
    """xop (N, K) float64 with bound xb, w (O, K) -> (ref, bound) of shape (slices, N, O): slice s contracts
    k in [s K / slices, (s + 1) K / slices)."""
    n, k = xop.shape
    o = w.shape[0]
    xs = xop.reshape(n, slices, k // slices)
    xbs = np.broadcast_to(np.asarray(xb, dtype=np.float64), xop.shape).reshape(n, slices, k // slices)
    ws = w.reshape(o, slices, k // slices)
    with np.errstate(all='ignore'):
        ref = np.einsum('nsk,osk->sno', xs, ws)
        shadow = np.einsum('nsk,osk->sno', np.abs(xs), np.abs(ws))
        carried = np.einsum('nsk,osk->sno', xbs, np.abs(ws))
        if bias is not None:
            ref = ref + bias
            shadow = shadow + np.abs(bias)
    g = gamma(depth)
    return ref, g * shadow + carried * (1 + g)


def act_ref(v, b, act):
    """a bound b on v through the activation."""
    with np.errstate(all='ignore'):
        if act == ACT_RELU:
            return np.maximum(v, 0.0), b
        if act == ACT_SIGMOID:
            s = 1.0 / (1.0 + np.exp(-v))
            return s, 0.25 * b + (2 * EXP_ULPS + 3) * U * s
        if act == ACT_TANH:
            t = np.tanh(v)
            return t, b + 2 * TANH_ULPS * U * np.abs(t)
    return v, b


def fc_operand(x, x_bias=None, x_relu=False, defect=None):
    """(parts, N, K) fp32 -> the (N, K) fp32 operand: parts added in order, + x_bias, ReLU -- the kernel's own bits."""
    order = range(x.shape[0])
    if defect == 'slices_reversed':
        order = reversed(order)
    v = None
    for s in order:
        v = x[s].clone() if v is None else (v + x[s]).float()
    if defect == 'relu_before_bias' and x_relu:
        v = torch.relu(v)
    if x_bias is not None:
        v = (v + x_bias).float()
    if x_relu and defect != 'relu_before_bias':
        v = torch.relu(v)
    return v


def gn_channels(k, hw):
    return -(-k // hw)


def fc_gn_ref(v, gn_size, hw, gam, bet):
    """v (N, K) float64, the exact operand -> relu(GroupNorm over gn_size consecutive features * gamma[k // hw] +
    beta[k // hw]) and its bound: norm_core's, then the product and the addition as in group_norm_relu_ref."""
    n, k = v.shape
    y, b = norm_core(v.reshape(n, k // gn_size, gn_size), fc_gn_depth(gn_size), IN_EPS)
    y, b = y.reshape(n, k), b.reshape(n, k)
    c = np.arange(k) // hw
    ga, be = f64(gam)[c][None], f64(bet)[c][None]
    t = y * ga
    bt = np.abs(ga) * b
    bt = bt + U * (np.abs(t) + bt)                                  # the product with gamma
    bt = bt + U * (np.abs(t) + np.abs(be) + bt)                     # the addition of beta
    return np.maximum(t + be, 0.0), bt


def parts_ref(ref, bound, x_bias=None, x_relu=False):
    """(parts, N, K) float64 partial sums the kernel holds only within `bound` -> (operand, bound) of the next load: the
    in-order sum rounds parts - 1 times, the bias once."""
    p = ref.shape[0]
    v, mag, b = ref.sum(0), np.abs(ref).sum(0), bound.sum(0)
    if x_bias is not None:
        v, mag = v + f64(x_bias), mag + np.abs(f64(x_bias))
    b = b + gamma(p - 1 + (x_bias is not None)) * (mag + b)
    return (np.maximum(v, 0.0) if x_relu else v), b


# ============================================================================================================= cases
class Case(dict):
    __getattr__ = dict.__getitem__


FC_REGIMES = ['nominal', 'offset', 'constant_group', 'cancelling_parts', 'cancelling_k', 'scaled_up', 'scaled_down']
SCALES = {'scaled_up': (40, 20), 'scaled_down': (-30, -20)}         # powers of two on x and on W


def fc_shape(n, k, o, o2=0, slices=1, parts=1, act=ACT_NONE, bias=True, x_bias=False, x_relu=False, gn=None):
    """gn = (group size, hw)"""
    return dict(n=n, k=k, o=o, o2=o2, slices=slices, parts=parts, act=act, bias=bias, x_bias=x_bias, x_relu=x_relu, gn=gn)


def _cancel_k(w, x, g):
    """the two halves of the k range cancel to 1e-4 of the shadow; an odd last column is scaled to 1e-4 too"""
    k = w.shape[-1]
    h = k // 2
    if h:
        x[..., h:2 * h] = x[..., :h]
        w[:, h:2 * h] = -w[:, :h] * (1 + 1e-4 * torch.randn(w[:, :h].shape, generator=g))
    if k > 1 and k % 2:
        w[:, -1] *= 1e-4


def fc_case(regime, shape, seed=0):
    s = Case(shape)
    scaled = regime in SCALES
    g = torch.Generator().manual_seed(4000 + 100 * FC_REGIMES.index('nominal' if scaled else regime) + seed)
    x = torch.randn((s.parts, s.n, s.k), generator=g)
    if s.parts > 1:
        x = x * s.parts ** -0.5
    w = torch.randn((s.o, s.k), generator=g) * s.k ** -0.5
    w2 = torch.randn((s.o2, s.k), generator=g) * s.k ** -0.5 if s.o2 else None
    bias = 0.1 * torch.randn((s.o,), generator=g)
    bias2 = 0.1 * torch.randn((max(s.o2, 1),), generator=g)[:s.o2]
    x_bias = 0.1 * torch.randn((s.k,), generator=g)
    gam = bet = None
    if s.gn is not None:
        nc = gn_channels(s.k, s.gn[1])
        gam, bet = 1.0 + 0.5 * torch.randn((nc,), generator=g), 0.3 * torch.randn((nc,), generator=g)
    if regime == 'offset':
        x[0] += 300.0 if s.gn is not None else 50.0
    if regime == 'constant_group':
        x[:, :, :s.gn[0]] = 0.0
        x[0, :, :s.gn[0]] = 2.5
    if regime == 'cancelling_parts' and s.parts > 1:
        x[0] = -x[1] * 1e3 + 1e-3 * x[0]
        x[1] = x[1] * 1e3
    if regime == 'cancelling_k':
        _cancel_k(w, x, g)
        if w2 is not None:
            w2[:, :] = w[torch.arange(s.o2) % s.o] * (1 + 0.5 * torch.rand((s.o2, 1), generator=g))
    c = Case(s, regime=regime, x=x.float().contiguous(), w=w.float().contiguous(), w2=w2,
             bias=bias if s.bias and s.slices == 1 else None, bias2=bias2 if s.bias and s.o2 else None,
             x_bias=x_bias if s.x_bias else None, gamma=gam, beta=bet, scale=1.0)
    if scaled:                                                      # no bias, no GroupNorm, an activation that commutes
        ex, ew = SCALES[regime]
        c.update(x=c.x * 2.0 ** ex, w=c.w * 2.0 ** ew, w2=None if w2 is None else w2 * 2.0 ** ew, bias=None, bias2=None,
                 x_bias=None, gn=None, gamma=None, beta=None, act=s.act if s.act == ACT_RELU else ACT_NONE,
                 scale=2.0 ** (ex + ew))
    return c


def fc_ref(c):
    """-> (ref, bound): (slices, N, O) partial sums for slices > 1, else the finished (N, O + O2) (both heads side by
    side, each element with its own bound)."""
    v = f64(fc_operand(c.x, c.x_bias, c.x_relu))
    vb = 0.0
    if c.gn is not None:
        v, vb = fc_gn_ref(v, c.gn[0], c.gn[1], c.gamma, c.beta)
    ks = c.k // c.slices
    if c.slices > 1:
        return gemm_ref(v, vb, f64(c.w), None, fc_depth(ks, False), c.slices)
    out = []
    for w, b in ((c.w, c.bias), (c.w2, c.bias2)):
        if w is not None:
            r, e = gemm_ref(v, vb, f64(w), None if b is None else f64(b), fc_depth(ks, b is not None))
            out.append(act_ref(r[0], e[0], c.act))
    return np.concatenate([r for r, _ in out], 1), np.concatenate([e for _, e in out], 1)


LINEAR_REGIMES = ['nominal', 'cancelling_k', 'scaled_up', 'scaled_down']


def linear_shape(n, k, o, o2=0, act=ACT_NONE, bias=True):
    return dict(n=n, k=k, o=o, o2=o2, act=act, bias=bias)


def linear_case(regime, shape, seed=0):
    s = Case(shape)
    scaled = regime in SCALES
    g = torch.Generator().manual_seed(5000 + 100 * LINEAR_REGIMES.index('nominal' if scaled else regime) + seed)
    x = torch.randn((s.n, s.k), generator=g)
    w = torch.randn((s.o, s.k), generator=g) * s.k ** -0.5
    w2 = torch.randn((s.o2, s.k), generator=g) * s.k ** -0.5 if s.o2 else None
    bias = 0.1 * torch.randn((s.o,), generator=g)
    bias2 = 0.1 * torch.randn((max(s.o2, 1),), generator=g)[:s.o2]
    if regime == 'cancelling_k':
        _cancel_k(w, x, g)
        if w2 is not None:
            w2[:, :] = w[torch.arange(s.o2) % s.o] * (1 + 0.5 * torch.rand((s.o2, 1), generator=g))
    c = Case(s, regime=regime, x=x.float().contiguous(), w=w.float().contiguous(), w2=w2,
             bias=bias if s.bias else None, bias2=bias2 if s.bias and s.o2 else None, scale=1.0)
    if scaled:
        ex, ew = SCALES[regime]
        c.update(x=c.x * 2.0 ** ex, w=c.w * 2.0 ** ew, w2=None if w2 is None else w2 * 2.0 ** ew, bias=None, bias2=None,
                 act=s.act if s.act == ACT_RELU else ACT_NONE, scale=2.0 ** (ex + ew))
    return c


def linear_ref_core(v, vb, w, bias, act):
    r, e = gemm_ref(v, vb, f64(w), None if bias is None else f64(bias), linear_depth(v.shape[1], bias is not None))
    return act_ref(r[0], e[0], act)


def linear_ref(c):
    """-> (ref, bound) of shape (N, O + O2)"""
    out = [linear_ref_core(f64(c.x), 0.0, w, b, c.act) for w, b in ((c.w, c.bias), (c.w2, c.bias2)) if w is not None]
    return np.concatenate([r for r, _ in out], 1), np.concatenate([e for _, e in out], 1)


# ===================================================================================================== fp32 emulations
FC_DEFECTS = ['slices_reversed', 'relu_before_bias', 'gamma_by_group', 'head2_bias_from_head1', 'drop_last_kstep',
              'wave_order']
LINEAR_DEFECTS = ['linear_tail_piece_dropped', 'pair_boundary_shift']


def act_fp32(v, act):
    return torch.relu(v) if act == ACT_RELU else torch.sigmoid(v) if act == ACT_SIGMOID else torch.tanh(v) if act == ACT_TANH else v


def gn_fp32(v, gn_size, hw, gam, bet, defect=None):
    """the kernel's order: a pair of threads per group, each a serial sum over its half, one exchange"""
    n, k = v.shape
    h = gn_size // 2
    t = v.reshape(n, k // gn_size, 2, h)
    s = torch.zeros(t.shape[:3])
    for i in range(h):
        s = s + t[..., i]
    mean = (s[..., 0] + s[..., 1]) / torch.tensor(float(gn_size))
    a = t - mean[..., None, None]
    q = torch.zeros(t.shape[:3])
    for i in range(h):
        q = q + a[..., i] * a[..., i]
    rstd = 1.0 / torch.sqrt((q[..., 0] + q[..., 1]) / torch.tensor(float(gn_size)) + torch.tensor(IN_EPS))
    c = (torch.arange(k) // (gn_size if defect == 'gamma_by_group' else hw)) % gam.numel()
    y = (a * rstd[..., None, None]).reshape(n, k)
    return torch.relu(y * gam[c][None] + bet[c][None])


def gemm_fp32(xop, w, slices, defect=None):
    """(N, K) x (O, K) -> (slices, N, O): per slice four waves, each a chain over its KS / 4 columns of the zero-filled
    [.][KS] tile, then ((w0 + w1) + w2) + w3"""
    n, k = xop.shape
    o, ks = w.shape[0], k // slices
    kl = fc_layout(ks)
    kw = kl // 4
    xs, ws = torch.zeros((slices, n, kl)), torch.zeros((slices, o, kl))
    xs[:, :, :ks] = xop.reshape(n, slices, ks).permute(1, 0, 2)
    ws[:, :, :ks] = w.reshape(o, slices, ks).permute(1, 0, 2)
    if defect == 'drop_last_kstep' and ks < kl:                     # the last k-step that holds data: two columns
        xs[:, :, ks - 2:ks] = 0.0
    xs, ws = xs.reshape(slices, n, 4, kw).permute(0, 2, 1, 3), ws.reshape(slices, o, 4, kw).permute(0, 2, 1, 3)
    acc = torch.zeros((slices, 4, n, o))
    for j in range(kw):
        acc = acc + xs[..., j][..., :, None] * ws[..., j][..., None, :]
    if defect == 'wave_order':
        return ((acc[:, 3] + acc[:, 2]) + acc[:, 1]) + acc[:, 0]
    return ((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3]


def fc_fp32(c, defect=None):
    v = fc_operand(c.x, c.x_bias, c.x_relu, defect)
    if c.gn is not None:
        v = gn_fp32(v, c.gn[0], c.gn[1], c.gamma, c.beta, defect)
    if c.slices > 1:
        return gemm_fp32(v, c.w, c.slices, defect)
    out = []
    for i, (w, b) in enumerate(((c.w, c.bias), (c.w2, c.bias2))):
        if w is not None:
            y = gemm_fp32(v, w, 1, defect)[0]
            if i == 1 and defect == 'head2_bias_from_head1' and c.bias is not None:
                b = c.bias[torch.arange(c.o2) % c.o]
            out.append(act_fp32(y if b is None else y + b, c.act))
    return torch.cat(out, 1)


def _wave_sum_fp32(v):
    """`for (off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off)` over the last axis (64 lanes); lane 0's value"""
    lanes = torch.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lanes ^ off]
    return v[..., 0]


def _gemv_fp32(x, w, defect=None):
    n, k = x.shape
    o = w.shape[0]
    if k % 4 == 0:
        p = -(-k // 256)
        xp, wp = torch.zeros((n, p * 256)), torch.zeros((o, p * 256))
        xp[:, :k], wp[:, :k] = x, w
        xp, wp = xp.reshape(n, 1, p, 64, 4), wp.reshape(1, o, p, 64, 4)
        acc = torch.zeros((n, o, 64))
        for i in range(p):
            if defect == 'linear_tail_piece_dropped' and i * 256 >= 1024:
                continue
            pr = xp[:, :, i] * wp[:, :, i]
            acc = acc + ((pr[..., 0] + pr[..., 1]) + (pr[..., 2] + pr[..., 3]))
    else:
        p = -(-k // 64)
        xp, wp = torch.zeros((n, p * 64)), torch.zeros((o, p * 64))
        xp[:, :k], wp[:, :k] = x, w
        xp, wp = xp.reshape(n, 1, p, 64), wp.reshape(1, o, p, 64)
        acc = torch.zeros((n, o, 64))
        for i in range(p):
            acc = acc + wp[:, :, i] * xp[:, :, i]
    return _wave_sum_fp32(acc)


def linear_fp32(c, defect=None):
    out = []
    for i, (w, b) in enumerate(((c.w, c.bias), (c.w2, c.bias2))):
        if w is not None:
            if i == 1 and defect == 'pair_boundary_shift':
                idx = torch.clamp(torch.arange(c.o2) + 1, max=c.o2 - 1)
                w, b = w[idx], None if b is None else b[idx]
            y = _gemv_fp32(c.x, w, defect)
            out.append(act_fp32(y if b is None else y + b, c.act))
    return torch.cat(out, 1)


# ============================================================================ the (regime, shape) lists of the GPU file
def _covering(axes, count, steps):
    """`count` tuples that walk every axis cyclically with its own step pattern (value index = (i * a + i // b) % len)."""
    return [tuple(ax[(i * a + i // b) % len(ax)] for ax, (a, b) in zip(axes, steps)) for i in range(count)]


def pairwise_cover(cases, naxes):
    """the least number of distinct values of another axis any value of any axis appears with"""
    least = 10 ** 9
    for i in range(naxes):
        for j in range(naxes):
            if i != j:
                for v in {c[i] for c in cases}:
                    least = min(least, len({c[j] for c in cases if c[i] == v}))
    return least


FC_N, FC_O = [1, 31, 32, 33, 65], [1, 31, 32, 33, 40]
FC_K = [8, 56, 64, 72, 128, 136, 248, 256]          # Ks = K: <64> <64> <64, exact> <128> <128, exact> <256> <256> <256, exact>
# (N, O, K, act, bias): 2a, a covering subset (pairwise_cover >= 2 is asserted below)
FC_FINISHED = _covering([FC_N, FC_O, FC_K, ACTS, [True, False]], 40, [(1, 5), (2, 5), (1, 8), (1, 4), (1, 3)])
# (slices, Ks): 2b, the producers of partial outputs (N = 33: a second row tile of one row; O = 40: a partial feature tile)
FC_PARTIAL = [(s, ks) for s in (2, 3, 8) for ks in (8, 72, 256)]
FC_PARTS = [2, 3, 4, 5, 6, 8, 9]                    # parts - 1 = 1, 2, 3 | 4, 5 | 7, 8: rounds of four, full and partial
FC_PARTS_K = 40                                     # the consumer's K: small, so that a rounding at 1e3 shows (test below)
# (group size, hw, slices, K): 2c.  64: fc_group_norm_half<32>; the others: the generic loop; 256: one group per slice
FC_GN = [(2, 1, 1, 8), (2, 3, 2, 48), (8, 4, 1, 72), (8, 3, 8, 64), (8, 1, 2, 272), (16, 4, 2, 96), (16, 16, 1, 128),
         (16, 3, 8, 384), (64, 16, 8, 2048), (64, 3, 1, 192), (64, 1, 2, 256), (64, 4, 1, 64), (128, 16, 2, 512),
         (128, 4, 1, 128), (128, 3, 8, 2048), (256, 16, 8, 2048), (256, 3, 1, 256), (256, 1, 2, 512), (2, 16, 8, 64),
         (256, 4, 2, 512)]
FC_GN_REGIMES = ['nominal', 'offset', 'constant_group']
# feat_size -> (group size, hw, slices, K) of the folded GroupNorm in front of fc1 (MultiClassPoseHead.fc_plan)
FC_HEAD_GEOMETRY = {(32, 32): (64, 16, 8, 2048), (16, 16): (16, 4, 2, 512), (8, 8): (4, 1, 1, 128)}
FC_TWO_HEADS = [(126, 63), (33, 31), (1, 1), (32, 32), (5, 70)]     # 2d, x N in {1, 33}
LIN_K = [1, 3, 4, 63, 64, 65, 252, 256, 260, 1020, 1024, 1028, 2052]
LIN_N, LIN_O = [1, 7, 8, 9, 17], [1, 3, 4, 5]
# (K, N, O, act, bias): 2e
LINEAR_SINGLE = _covering([LIN_K, LIN_N, LIN_O, ACTS, [True, False]], 39, [(1, 10 ** 6), (1, 5), (2, 5), (1, 13), (1, 3)])
LINEAR_PAIRS = [(126, 63), (1, 1), (5, 2), (3, 4)]
LINEAR_PAIR_KN = [(256, 1), (65, 9), (1028, 7), (3, 17)]


def fc_inputs():
    """every (regime, shape) of tests/test_gpu_fc.py sections 2a - 2d"""
    for n, o, k, act, bias in FC_FINISHED:
        yield 'nominal', fc_shape(n, k, o, act=act, bias=bias)
    for n, o, k, act, bias in FC_FINISHED[::5]:
        for regime in ('offset', 'cancelling_k', 'scaled_up', 'scaled_down'):
            yield regime, fc_shape(n, k, o, act=act, bias=bias)
    for s, ks in FC_PARTIAL:
        yield 'nominal', fc_shape(33, s * ks, 40, slices=s)
        yield 'cancelling_k', fc_shape(33, s * ks, 40, slices=s)
    for parts in FC_PARTS:
        for regime in ('nominal', 'cancelling_parts'):
            yield regime, fc_shape(33, FC_PARTS_K, 33, parts=parts, x_bias=True, x_relu=True, act=ACT_RELU)
    for gs, hw, s, k in FC_GN + list(FC_HEAD_GEOMETRY.values()):
        for regime in FC_GN_REGIMES:
            yield regime, fc_shape(33, k, 33, slices=s, gn=(gs, hw))
    for gs, hw, s, k in [(64, 16, 8, 2048), (8, 3, 8, 64), (16, 4, 2, 96)]:
        yield 'nominal', fc_shape(33, k, 33, slices=s, parts=4, gn=(gs, hw))
    for o, o2 in FC_TWO_HEADS:
        for n in (1, 33):
            yield 'nominal', fc_shape(n, 72, o, o2=o2, parts=2, x_bias=True, x_relu=True)
            yield 'nominal', fc_shape(n, 256, o, o2=o2, act=ACT_TANH)


def linear_inputs():
    for k, n, o, act, bias in LINEAR_SINGLE:
        for regime in LINEAR_REGIMES:
            yield regime, linear_shape(n, k, o, act=act, bias=bias)
    for (o, o2), (k, n) in zip(LINEAR_PAIRS, LINEAR_PAIR_KN):
        for act in ACTS:
            yield 'nominal', linear_shape(n, k, o, o2=o2, act=act)
        yield 'cancelling_k', linear_shape(n, k, o, o2=o2)


# ===================================================================================================== the self-checks
def test_case_lists_cover_every_axis_pair():
    """every value of every axis appears with at least two values of every other axis (2a, 2e), and every GroupNorm
    axis value with two of each other axis (2c)"""
    assert {c[0] for c in FC_FINISHED} == set(FC_N) and {c[1] for c in FC_FINISHED} == set(FC_O)
    assert {c[2] for c in FC_FINISHED} == set(FC_K) and {c[3] for c in FC_FINISHED} == set(ACTS)
    assert pairwise_cover(FC_FINISHED, 5) >= 2
    assert {c[0] for c in LINEAR_SINGLE} == set(LIN_K) and {c[1] for c in LINEAR_SINGLE} == set(LIN_N)
    assert {c[2] for c in LINEAR_SINGLE} == set(LIN_O) and {c[3] for c in LINEAR_SINGLE} == set(ACTS)
    assert pairwise_cover(LINEAR_SINGLE, 5) >= 2
    assert {c[0] for c in FC_GN} == {2, 8, 16, 64, 128, 256} and {c[1] for c in FC_GN} == {1, 3, 4, 16}
    assert {c[2] for c in FC_GN} == {1, 2, 8} and pairwise_cover([c[:3] for c in FC_GN], 3) >= 2
    for gs, hw, s, k in FC_GN + list(FC_HEAD_GEOMETRY.values()):
        ks = k // s
        assert k % s == 0 and ks % 8 == 0 and ks <= 256 and ks % gs == 0 and gs % 2 == 0


def test_depths_are_the_counts_of_the_source():
    assert [fc_depth(ks) for ks in (8, 64, 72, 128, 136, 256)] == [21, 21, 37, 37, 69, 69]
    assert fc_depth(256, bias=False) == 68 and fc_gn_depth(64) == 33 and fc_gn_depth(2) == 2
    assert [linear_depth(k) for k in (1, 3, 65, 4, 256, 260, 1024, 1028, 2052)] == [9, 9, 10, 11, 11, 12, 14, 15, 19]


def test_fc_emulation_inside_the_bound():
    worst = {}
    for regime, shape in fc_inputs():
        c = fc_case(regime, shape)
        ref, bound = fc_ref(c)
        fam = ('gn ' if c.gn else 'two heads ' if c.o2 else 'partial ' if c.slices > 1 else 'parts ' if c.parts > 1 else 'finished ') + regime
        worst[fam] = max(worst.get(fam, 0.0), worst_ratio(fc_fp32(c), ref, bound))
    for fam, v in worst.items():
        measured(f'fc_splitk fp32 emulation / bound, {fam}', v)
        assert v <= 1.0, fam


def test_linear_emulation_inside_the_bound():
    worst = {}
    for regime, shape in linear_inputs():
        c = linear_case(regime, shape)
        ref, bound = linear_ref(c)
        worst[regime] = max(worst.get(regime, 0.0), worst_ratio(linear_fp32(c), ref, bound))
        if c.act in (ACT_NONE, ACT_RELU) and not c.o2:              # torch's own fp32 linear is inside as well
            t = act_fp32(F.linear(c.x, c.w, c.bias), c.act)
            worst['torch ' + regime] = max(worst.get('torch ' + regime, 0.0), worst_ratio(t, ref, bound))
    for regime, v in worst.items():
        measured(f'linear fp32 emulation / bound, {regime}', v)
        assert v <= 1.0, regime


def _defect_worst(defect):
    worst = 0.0
    if defect in LINEAR_DEFECTS:
        for regime, shape in linear_inputs():
            c = linear_case(regime, shape)
            worst = max(worst, worst_ratio(linear_fp32(c, defect), *linear_ref(c)))
    else:
        for regime, shape in fc_inputs():
            if defect == 'wave_order' and regime != 'nominal':
                continue
            c = fc_case(regime, shape)
            worst = max(worst, worst_ratio(fc_fp32(c, defect), *fc_ref(c)))
    return worst


@pytest.mark.parametrize('defect', [d for d in FC_DEFECTS + LINEAR_DEFECTS if d != 'wave_order'])
def test_planted_defects_outside(defect):
    worst = _defect_worst(defect)
    measured(f'defect {defect} / bound (worst case of the GPU lists)', worst)
    assert worst > 1.0


def test_wave_order_is_inside_the_bound_and_only_bits_can_see_it():
    """adding the four wave tiles w3 first is another fp32 evaluation of the same sum: the bound admits it on every
    nominal case, as it must.  What it changes is bits, and only where the wave tiles cancel (`cancelling_k`: waves 0, 1
    against 2, 3) do those differ at all often.  So the order the header promises is held by the bit-for-bit tests of the
    GPU file (run twice, a row of N = 65 against N = 1, a pair launch against two single ones, power-of-two scaling) and
    by reading the source, not by the bound."""
    worst = _defect_worst('wave_order')
    measured('defect wave_order / bound, nominal', worst)
    assert worst <= 1.0
    c = fc_case('cancelling_k', fc_shape(33, 256, 40, bias=False))
    assert not same_bits(fc_fp32(c), fc_fp32(c, 'wave_order'))
    assert worst_ratio(fc_fp32(c, 'wave_order'), *fc_ref(c)) <= 1.0


def test_cancelling_parts_need_the_in_order_sum():
    """parts >= 3 (two parts commute): the reversed sum rounds at the magnitude of the large parts and is outside"""
    for parts in FC_PARTS[1:]:
        c = fc_case('cancelling_parts', fc_shape(33, FC_PARTS_K, 33, parts=parts, x_bias=True, x_relu=True, act=ACT_RELU))
        ref, bound = fc_ref(c)
        good, rev = fc_fp32(c), fc_fp32(c, 'slices_reversed')
        assert worst_ratio(good, ref, bound) <= 1.0 < worst_ratio(rev, ref, bound), parts
        measured(f'slices_reversed / bound, {parts} cancelling parts', worst_ratio(rev, ref, bound))
    c = fc_case('cancelling_parts', fc_shape(33, FC_PARTS_K, 33, parts=2))
    assert same_bits(fc_fp32(c), fc_fp32(c, 'slices_reversed'))


def test_scaled_emulation_is_the_nominal_one_times_a_power_of_two():
    for n, o, k, act, bias in FC_FINISHED[::5]:
        shape = fc_shape(n, k, o, act=act if act == ACT_RELU else ACT_NONE, bias=False)
        base = fc_fp32(fc_case('nominal', shape))
        for regime in SCALES:
            c = fc_case(regime, shape)
            assert same_bits(fc_fp32(c), base * c.scale), (regime, shape)
    for k, n, o, act, bias in LINEAR_SINGLE[::4]:
        shape = linear_shape(n, k, o, act=act if act == ACT_RELU else ACT_NONE, bias=False)
        base = linear_fp32(linear_case('nominal', shape))
        for regime in SCALES:
            c = linear_case(regime, shape)
            assert same_bits(linear_fp32(c), base * c.scale), (regime, shape)


def test_constant_group_is_relu_of_beta():
    c = fc_case('constant_group', fc_shape(33, 192, 33, gn=(64, 3)))
    v, b = fc_gn_ref(f64(fc_operand(c.x)), 64, 3, c.gamma, c.beta)
    ch = np.arange(64) // 3
    assert np.array_equal(v[:, :64], np.broadcast_to(np.maximum(f64(c.beta)[ch], 0.0), (33, 64)))
    assert float(b[:, :64].max()) < 1e-2                            # rstd = 316, |x| = 2.5: (D + 1) U x rstd ~ 1.6e-3 gamma


def nonfinite_case():
    """x (4, 16), W (6, 16): one NaN in x[1, 5]; one +inf in W[2, 9] with x[3, 9] == 0 and every other x[:, 9] != 0"""
    c = fc_case('nominal', fc_shape(4, 16, 6, o2=3))
    c.x[0, :, 9] = torch.tensor([0.5, -0.25, 2.0, 0.0])
    c.x[0, 1, 5] = float('nan')
    c.w[2, 9] = float('inf')
    return c


def nonfinite_pattern(c):
    """what any IEEE evaluation of y = x W^T gives for nonfinite_case: (N, O) codes 0 finite, 1 NaN, 2 +-inf"""
    code = np.zeros((4, 6), dtype=np.int64)
    code[:, 2] = 2
    code[3, 2] = 1                                                  # 0 * inf
    code[1, :] = 1
    return code


def test_nonfinite_reference_agrees_with_torch():
    c = nonfinite_case()
    y = F.linear(c.x[0], c.w, c.bias)
    code = np.where(np.isnan(f64(y)), 1, np.where(np.isinf(f64(y)), 2, 0))
    assert np.array_equal(code, nonfinite_pattern(c))
    y2 = F.linear(c.x[0], c.w2, c.bias2)
    assert bool(torch.isnan(y2[1]).all()) and bool(torch.isfinite(y2[[0, 2, 3]]).all())
    assert same_nan_pattern(linear_fp32(Case(c, x=c.x[0])), torch.cat([y, y2], 1))
    # the divergence: torch.relu keeps a NaN, the kernels' ReLU forms return KERNEL_RELU_OF_NAN
    assert bool(torch.isnan(torch.relu(torch.tensor(float('nan')))))
    assert KERNEL_RELU_OF_NAN == 0.0 and math.isnan(float(torch.relu(y)[1, 0]))
