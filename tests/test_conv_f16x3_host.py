"""CPU: the split-fp16 convolution (conv_f16x3.hip, conv precision 'f16x3') across fp16's range -- the restatement of what
the kernel is specified to compute, two per-element bounds computed from the operands alone, the operand regimes, and the
planted defects the bounds are shown to see.  tests/test_gpu_conv_f16x3.py launches the kernel on these operands.

**The specification.**  Every fp32 operand is split as t = hi + lo' 2^-11 + e, hi = fp16(t), lo' = fp16((t - hi) 2^11)
(``split64``: fp16 roundings through ``torch.half`` on the CPU, round to nearest even, subnormals kept), and the kernel
returns

    S = sum w_hi x_hi + 2^-11 sum (w_hi x_lo' + w_lo' x_hi)                                             (``f16x3_ref64``)

followed by the shared affine epilogue (``epilogue64`` of tests/test_conv_exact_host.py: + bias, BN scale / shift,
+ residual, ReLU).  lo * lo is dropped by design.

**B_acc: the kernel against its specification** (``bounds``).  fp16 x fp16 products are exact in fp32 (22 significant bits).
acc0 receives K such products, acc1 2 K of them, K = taps x input channels padded to the staged chunk (16 NK channels; the
padded products are exact zeros); a sum of m terms accumulated in fp32 in ANY order, each addition rounding once, is within
m U sum |terms| of the exact sum (Jeannerod and Rump 2013; U = 2^-24, no higher-order term: the form (K + c0) U the project
uses for its fma chains).  The merge acc0 + acc1 2^-11 scales by a power of two (exact) and adds once: c0 = 1 on both chains.
With T0 = sum |w_hi||x_hi| and T1 = sum (|w_hi||x_lo'| + |w_lo'||x_hi|):

    |acc - S| <= (K + 1) U T0 + (2 K + 1) U 2^-11 T1  =: A

The epilogue rounds at most four more times (+ bias, the scale, the shift -- or one fma --, + residual), each rounding
relative to an intermediate no larger than M = |s| (|S| + A + |b|) + |shift| + |res|:

    B_acc = |s| A + n_epi U M (1 + 2^-20),      n_epi = the roundings of the variant's epilogue (0 for the plain one)

ReLU rounds nothing and is 1-Lipschitz.  The bound holds wherever hi is finite: fp32 neither overflows nor underflows in any
regime below (checked: the smallest product is 2^-48 2^-11).

**B_model: the specification against the true convolution.**  w x - (w_hi x_hi + w_hi x_l + w_l x_hi) with t_l = lo' 2^-11
equals w_l x_l + e_w x + w e_x - e_w e_x, so

    |S - sum w x| <= sum (|w_l||x_l| + |e_w||x| + |w||e_x| + |e_w||e_x|)  =: B_model

**The domain** (``test_model_constant``).  For 2^-14 <= |t| < 65520 (hi finite and normal): |t_l| = |t - hi| <= 2^-11 |t|
(round to nearest), and lo' is t_l 2^11 rounded to 11 bits, or -- below 2^-14 -- to a multiple of 2^-24 (error <= 2^-25,
i.e. 2^-36 <= 2^-22 |t| of t): |e| <= 2^-22 |t|.  Hence inside the domain B_model <= c_m 2^-22 sum |w||x| with
c_m = 1 (lo lo) + 1 (e_w x) + 1 (w e_x) + 2^-22 = 3 + 2^-22.  Below 2^-14 the errors stop shrinking with the operand:
|t_l| <= 2^-25 and |e| <= 2^-36 ABSOLUTE (graceful degradation: the relative error of a layer at 1e-6 is 2^-5);
from 65520 on hi is infinite and everything it touches is non-finite.

**The weight criterion** (``ops.f16x3_weight_excess``, the same arithmetic): a layer is handed to the route only while, for
every output channel, sum |e_w| + 2^-11 sum |w_l| <= 2 x 2^-22 sum |w| -- the bound the two terms have inside the domain.
``test_weight_criterion`` pins which regimes pass.

Measured factors by which each planted defect leaves B_acc are printed by ``test_planted_defects_leave_the_bound`` and
listed in DESIGN.md."""
import math
import zlib

import pytest
import torch
import torch.nn.functional as F

from scflow_amd import ops
import test_conv_exact_host as H
from test_conv_exact_host import NONE, RELU, Row, P1, conv64, epilogue64

U = 2.0 ** -24
LO = 2048.0
F16_MIN_NORMAL = 2.0 ** -14
C_M = 3.0 + 2.0 ** -22
CRITERION = 2.0                     # sum|e_w| + 2^-11 sum|w_l| <= CRITERION 2^-22 sum|w| per output channel

# ------------------------------------------------------------------------------------------------------------------- rows
# the six f16-* rows of the route table, one <2, 1, *> row whose Cout is no multiple of 32 (the masked tail of the second
# 32-channel fragment, ragged 17x23 map, two segments), and the stride-2 row: the kernel's staging budget (cells of the
# input window per thread) holds no stride-2 3x3 window at any fragment shape, so under 'f16x3' such a layer goes on down the
# walk to the fp32 LDS-DMA kernel.  The row pins that and holds the result to the fp32 bound.
NEW_ROWS = [
    Row('f16-21-cout48', 128, 40, 48, (3, 3), 1, P1, 17, 23, 32, dict(f16=True), 'f16x3', (2, 1, 640, -54), '<2, 1, 1>'),
    Row('f16-s2-refused', 2, 40, 48, (3, 3), 2, P1, 17, 23, 32, dict(f16=True), 'direct-dma', (1, 1, 20, -36), 'stride 2: not on this route'),
]
ROWS = [r for r in H.ROUTES if r.family == 'f16x3'] + NEW_ROWS
BY_ID = {r.id: r for r in ROWS}
IDS = [r.id for r in ROWS]
INSTANTIATIONS = ((2, 1, 1), (2, 1, 2), (1, 2, 1), (1, 1, 1), (1, 1, 2))
PERIOD = 2                          # distinct samples of a row's input: sample n repeats sample n % PERIOD


def instantiation(row, info=None):
    """(WM, WN, NK) from the dry run's info {WM, WN, blocks, -(T NK 3 WM WN)} of a launch the split-fp16 kernel takes"""
    wm, wn, _, m = info if info is not None else row.info
    t = row.k[0] * row.k[1]
    assert m < 0 and -m % (3 * t * wm * wn) == 0, (row.id, info)
    return wm, wn, -m // (3 * t * wm * wn)


def chain_length(row):
    """K: taps x input channels padded to the staged chunk of the row's instantiation (fp32 rows: the 32-channel packing)"""
    kc = 16 * instantiation(row)[2] if row.family == 'f16x3' else 32
    return row.k[0] * row.k[1] * ((row.cin + kc - 1) // kc * kc)


def variants(row):
    plain = dict(bias=False, res=False, bn=False, act=NONE, act2=NONE, split=0, two=False)
    v = {'plain': plain, 'bias_relu': dict(plain, bias=True, act=RELU), 'bn_res': dict(plain, bias=True, bn=True, res=True)}
    if row.c0:
        v['two'] = dict(plain, bias=True, two=True)
    return v


def epilogue_roundings(spec):
    return int(spec['bias']) + 2 * int(spec['bn']) + int(spec['res'])


# ------------------------------------------------------------------------------------------------------------------ split
def _flush16(h):
    return torch.where(h.abs() < F16_MIN_NORMAL, torch.zeros_like(h), h)


def _trunc16(t):
    """fp16 toward zero"""
    h = t.half()
    over = h.float().abs() > t.abs()
    bits = h.view(torch.int16)
    return torch.where(over & torch.isfinite(t), bits - 1, bits).view(torch.half)       # sign-magnitude: one step towards zero


def split64(t, flush=(), truncate=False, unscaled_lo=False):
    """t (fp32) -> (hi, lo', e) as float64 with t = hi + lo' 2^-11 + e exactly.  ``flush``: 'hi' / 'lo' -- fp16 subnormals
    of that half read as zero (a conversion or a matrix-core operand that flushes); ``truncate``: hi rounded toward zero;
    ``unscaled_lo``: lo' = fp16(t - hi), the residual without its 2^11 (planted defects)."""
    t = t.float()
    hi = (_trunc16(t) if truncate else t.half()).float()
    if 'hi' in flush:
        hi = _flush16(hi)
    r = t - hi                                            # exact in fp32 (the kernel's own subtraction)
    lo = (r if unscaled_lo else r * LO).half().float()    # r 2^11 is exact in fp32; one fp16 rounding
    if 'lo' in flush:
        lo = _flush16(lo)
    hi, lo = hi.double(), lo.double()
    return hi, lo, t.double() - hi - lo / LO


def _halves(row, x, w, **kw):
    xs, ws = split64(x, **kw), split64(w, **kw)
    return xs, ws


def f16x3_ref64(row, x, w, case=None, spec=None, samples=slice(None), drop=(), scale=1.0 / LO, **split_kw):
    """S (float64, three conv64 calls), then the epilogue of ``spec`` on ``case``'s parameters.  ``drop``: 'hl' (w_hi x_lo')
    / 'lh' (w_lo' x_hi) left out; ``scale``: the factor acc1 is merged with; ``split_kw``: see ``split64``."""
    (xh, xl, _), (wh, wl, _) = _halves(row, x[samples], w, **split_kw)
    s = conv64(row, xh, wh)
    cross = torch.zeros_like(s)
    if 'hl' not in drop:
        cross = cross + conv64(row, xl, wh)
    if 'lh' not in drop:
        cross = cross + conv64(row, xh, wl)
    s = s + cross * scale
    return s if spec is None else epilogue64(case, s, spec, samples)


def _core(row, case, samples):
    """the convolutions of ``bounds``, once per (case, samples): kept in the case like ``reference``'s conv64"""
    key = ('f16x3 core', samples.start, samples.stop)
    if key not in case:
        x, w = case['x'][samples], case['w']
        (xh, xl, xe), (wh, wl, we) = _halves(row, x, w)
        a = lambda t: t.abs()
        case[key] = dict(
            t0=conv64(row, a(xh), a(wh)), t1=conv64(row, a(xl), a(wh)) + conv64(row, a(xh), a(wl)),
            model=(conv64(row, a(xl) / LO, a(wl) / LO) + conv64(row, a(x.double()), a(we)) + conv64(row, a(xe), a(w.double()))
                   + conv64(row, a(xe), a(we))),
            s=conv64(row, xh, wh) + (conv64(row, xl, wh) + conv64(row, xh, wl)) / LO,
            true=conv64(row, x, w), mag=conv64(row, a(x.double()), a(w.double())))
    return case[key]


def bounds(row, case, spec, samples=slice(None)):
    """-> dict of float64 tensors: ref (the specification), true (float64 convolution + epilogue), b_acc, b_model (both
    already carried through the epilogue's scale), mag (|s| sum |w||x|: the unit of the fp32-class statements)"""
    c = _core(row, case, samples)
    k = chain_length(row)
    a = lambda t: t.abs()
    s, true, model, mag = c['s'], c['true'], c['model'], c['mag']
    acc = (k + 1) * U * c['t0'] + (2 * k + 1) * U * c['t1'] / LO
    sc = torch.ones(row.cout, dtype=torch.float64)
    m = a(s) + acc
    if spec['bias']:
        m = m + a(case['b'].double()).view(1, -1, 1, 1)
    if spec['bn']:
        sc, shift = H.bn_affine(case)
        sc = a(sc)
        m = m * sc.view(1, -1, 1, 1) + a(shift).view(1, -1, 1, 1)
    if spec['res']:
        m = m + a(case['res'][samples].double())
    sc = sc.view(1, -1, 1, 1)
    return dict(ref=epilogue64(case, s, spec, samples), true=epilogue64(case, true, spec, samples),
                b_acc=sc * acc + epilogue_roundings(spec) * U * m * (1 + 2.0 ** -20), b_model=sc * model, mag=sc * mag,
                finite=bool(torch.isfinite(s).all()))


def fp32_bound(row, case, spec, samples=slice(None)):
    """an fp32 kernel against the true convolution: (K + 8) U sum |w||x| (one rounding per term of a chain in any order, up
    to 8 partial sums combined afterwards) carried through the epilogue like ``bounds``' B_acc"""
    x, w = case['x'][samples], case['w']
    mag = conv64(row, x.double().abs(), w.double().abs())
    acc = (chain_length(row) + 8) * U * mag
    m = conv64(row, x, w).abs() + acc
    sc = torch.ones(row.cout, dtype=torch.float64)
    if spec['bias']:
        m = m + case['b'].double().abs().view(1, -1, 1, 1)
    if spec['bn']:
        sc, shift = H.bn_affine(case)
        sc = sc.abs()
        m = m * sc.view(1, -1, 1, 1) + shift.abs().view(1, -1, 1, 1)
    if spec['res']:
        m = m + case['res'][samples].double().abs()
    return sc.view(1, -1, 1, 1) * acc + epilogue_roundings(spec) * U * m * (1 + 2.0 ** -20)


# ---------------------------------------------------------------------------------------------------------------- regimes
# (row, regime, seed) -> operands; seeds 0 and 1 of every regime are used, the seed also picks the regime's variant
REGIMES = ['nominal', 'three_decades', 'pow2_scaled', 'small_w', 'small_x', 'subnormal_band', 'near_max', 'over_range',
           'cancelling', 'one_huge_among_small']
SEEDS = (0, 1)
FINITE = [r for r in REGIMES if r != 'over_range']
POW2_GRID = ((-8, -8), (-8, 12), (12, -8), (12, 12), (5, 0), (0, -3))     # every hi and lo' normal: see _pow2_operand
NEAR_MAX = (65504.0, 65519.99609375, 65504.0 - 2.0 ** -8, -65504.0, -65519.99609375)
OVER = 1e5


def _gen(row, regime, seed):
    return torch.Generator().manual_seed(zlib.crc32(f'{row.id}/{regime}'.encode()) % (2 ** 31) + 7919 * seed)


def _pow2_operand(shape, g):
    """t = H + L 2^-11 with H an fp16 number in [1/4, 4) and L an 8-bit fp16 number, 2^-3 <= |L| / 2^floor(log2 |H|) < 1:
    hi = H and lo' = L exactly, t is an fp32 number, and for -8 <= a <= 12 both halves of 2^a t are normal fp16 numbers --
    scaling by 2^a then commutes with every rounding of the kernel"""
    e = torch.randint(-2, 2, shape, generator=g).double()
    hm = torch.randint(1024, 2048, shape, generator=g).double() * 2.0 ** -10
    el = e - torch.randint(1, 4, shape, generator=g).double()
    lm = torch.randint(128, 256, shape, generator=g).double() * 2.0 ** -7
    sign = lambda: torch.randint(0, 2, shape, generator=g).double() * 2 - 1
    return (sign() * hm * 2.0 ** e + sign() * lm * 2.0 ** el / LO).float()


def _plant(t, g, values, count=4):
    """``count`` copies of each value at random places of every leading slice of t"""
    flat = t.reshape(t.shape[0], -1)
    for i in range(flat.shape[0]):
        idx = torch.randperm(flat.shape[1], generator=g)[:count * len(values)]
        flat[i, idx] = torch.tensor(values, dtype=t.dtype).repeat(count)
    return flat.reshape(t.shape)


def _pow2_floor(v):
    return 2.0 ** math.floor(math.log2(v)) if v > 0 and math.isfinite(v) else 1.0


_CASES = {}


def operands(row, regime, seed):
    """cached (the last few cases): the tests share one case per (row, regime, seed) and leave it unchanged"""
    key = (row.id, regime, seed)
    if key not in _CASES:
        while len(_CASES) >= 6:
            _CASES.pop(next(iter(_CASES)))
        _CASES[key] = _operands(row, regime, seed)
    return _CASES[key]


def _operands(row, regime, seed):
    """the case of (row, regime, seed): x (sample n = sample n % PERIOD), w, and epilogue parameters on the scale of the
    outputs: bias, residual, BN shift are small integers times a power of two near the median of sum |w||x|, the BN scale
    is +-1, +-2 times {2, 1, 1/2, 1/4} (exact in fp32, as in the route table's cases).  Cached; the tests leave it unchanged."""
    g = _gen(row, regime, 0 if regime == 'pow2_scaled' else seed)        # pow2_scaled: one base, the seed picks (a, b)
    n, cin, cout, (kh, kw) = row.n, row.cin, row.cout, row.k
    ho, wo = H.out_hw(row)
    xs, ws = (min(n, PERIOD), cin, row.H, row.W), (cout, cin, kh, kw)
    rn = lambda shape: torch.randn(shape, generator=g)
    x, w = rn(xs), rn(ws) * (1.0 / (cin * kh * kw)) ** 0.5
    note = ''
    if regime == 'three_decades':
        w = w * 10.0 ** (-3.0 * torch.rand(ws, generator=g))
    elif regime == 'pow2_scaled':
        x, w = _pow2_operand(xs, g), _pow2_operand(ws, g)
        a, b = POW2_GRID[seed]
        x, w, note = x * 2.0 ** a, w * 2.0 ** b, f'2^{a} x, 2^{b} w'
    elif regime == 'small_w':
        w, note = w * (1e-4, 1e-6)[seed], f'w x {(1e-4, 1e-6)[seed]:g}'
    elif regime == 'small_x':
        x, note = x * (1e-5, 1e-7)[seed], f'x x {(1e-5, 1e-7)[seed]:g}'
    elif regime == 'subnormal_band':
        band = lambda shape: torch.sign(rn(shape)) * 2.0 ** (-24.0 + 10.0 * torch.rand(shape, generator=g))
        x, w = band(xs), band(ws)
        x, w = x.clamp(-F16_MIN_NORMAL, F16_MIN_NORMAL), w.clamp(-F16_MIN_NORMAL, F16_MIN_NORMAL)
    elif regime == 'near_max':
        if seed == 0:
            x, note = _plant(x * 1000.0, g, NEAR_MAX), '|x| up to 65519.996'
        else:
            w, note = _plant(w * 1000.0, g, NEAR_MAX, count=1), '|w| up to 65519.996'
    elif regime == 'over_range':
        if seed == 0:
            x, note = _plant(x, g, (OVER,), count=1), 'one activation of 1e5 per sample'
        else:
            w, note = _plant(w.reshape(1, -1), g, (OVER,), count=1).reshape(ws), 'one weight of 1e5'
    elif regime == 'cancelling':
        x = 1.0 + 1e-5 * x
        w = w - w.mean(dim=(1, 2, 3), keepdim=True)
    elif regime == 'one_huge_among_small':
        if seed == 0:
            x, note = _plant(1e-3 * x, g, (60000.0, -60000.0), count=2), '60000 in x'
        else:
            w, note = _plant(1e-3 * rn(ws), g, (60000.0, -60000.0), count=1), '60000 in w'
    x = x.float().repeat((n + xs[0] - 1) // xs[0], 1, 1, 1)[:n].contiguous()
    w = w.float().contiguous()
    finite = torch.isfinite(x.half().float()).all() and torch.isfinite(w.half().float()).all()
    mag = conv64(row, x[:1].double().abs().clamp(max=65504.0), w.double().abs().clamp(max=65504.0))
    unit = _pow2_floor(float(mag.median()))
    ri = lambda lo, hi, shape: torch.randint(lo, hi + 1, shape, generator=g).float()
    pm = lambda shape: ri(0, 1, shape) * 2 - 1
    res = (ri(-3, 3, (min(n, PERIOD), cout, ho, wo)) * unit).repeat((n + PERIOD - 1) // PERIOD, 1, 1, 1)[:n].contiguous()
    var = torch.tensor(H.BN_VARS)[torch.randint(0, 4, (cout,), generator=g)].float()
    return dict(regime=regime, seed=seed, note=note, unit=unit, pow2=POW2_GRID[seed] if regime == 'pow2_scaled' else None, hi_finite=bool(finite), x=x, w=w,
                b=ri(-3, 3, (cout,)) * unit, res=res,
                bn=(ri(1, 2, (cout,)) * pm((cout,)), ri(-3, 3, (cout,)) * unit, ri(-1, 1, (cout,)) * unit, var))


def weight_excess(w):
    """per output channel: (sum |e_w| + 2^-11 sum |w_l|) / (2^-22 sum |w|) by ``split64`` (0 for an all-zero channel,
    inf where some hi is infinite)"""
    _, lo, e = split64(w)
    num = (e.abs() + lo.abs() / LO / LO).flatten(1).sum(1)
    den = 2.0 ** -22 * w.double().abs().flatten(1).sum(1)
    out = torch.where(num == 0, torch.zeros_like(num), num / den)
    return torch.where(torch.isfinite(out), out, torch.full_like(out, math.inf))


# ---------------------------------------------------------------------------------------------------- fp32 restatements
def _patches(row, t):
    """(n, cin, taps, L) of a float64 tensor by the row's geometry"""
    n, c = t.shape[:2]
    cols = F.unfold(F.pad(t, (row.pad[1], row.pad[1], row.pad[0], row.pad[0])), row.k, stride=row.stride)
    return cols.view(n, c, row.k[0] * row.k[1], -1)


def s_fp32(row, x, w, order):
    """S with two fp32 accumulators and the merge, every addition rounding to fp32: 'channel' (taps innermost), 'tap' (channels
    innermost), 'pairwise' (a balanced tree).  One sample."""
    (xh, xl, _), (wh, wl, _) = _halves(row, x[:1], w)
    ph, pl = _patches(row, xh)[0].float(), _patches(row, xl)[0].float()            # (cin, taps, L)
    wh, wl = wh.flatten(2).float(), wl.flatten(2).float()                             # (cout, cin, taps)
    cin, taps = ph.shape[:2]
    terms = [(c, t) for c in range(cin) for t in range(taps)] if order != 'tap' else [(c, t) for t in range(taps) for c in range(cin)]
    if order == 'pairwise':
        def tree(v):                                                                  # (cout, m, L) -> (cout, L)
            while v.shape[1] > 1:
                if v.shape[1] % 2:
                    v = torch.cat([v, torch.zeros_like(v[:, :1])], 1)
                v = v[:, 0::2] + v[:, 1::2]
            return v[:, 0]
        p, q = ph.flatten(0, 1), pl.flatten(0, 1)
        a, b = wh.flatten(1), wl.flatten(1)
        acc0 = tree(a[:, :, None] * p[None])
        acc1 = tree(torch.cat([a[:, :, None] * q[None], b[:, :, None] * p[None]], 1))
    else:
        acc0 = torch.zeros((w.shape[0], ph.shape[2]))
        acc1 = torch.zeros_like(acc0)
        for c, t in terms:
            acc0 = acc0 + wh[:, c, t, None] * ph[c, t][None]                          # fp16 x fp16: the product is exact
            acc1 = acc1 + wh[:, c, t, None] * pl[c, t][None]
            acc1 = acc1 + wl[:, c, t, None] * ph[c, t][None]
    ho, wo = H.out_hw(row)
    return (acc0 + acc1 * (1.0 / LO)).double().view(1, -1, ho, wo)


# ---------------------------------------------------------------------------------------------------------------- defects
def _tail_reads_element0(row, x, w):
    """the zero padding of the last 16-channel chunk replaced by the chunk's first channel, in the staged window and in the
    packed weights alike (either one alone is absorbed by the other's zeros while the operands are finite)"""
    pad = -row.cin % 16
    first = row.cin // 16 * 16
    return (torch.cat([x, x[:, first:first + 1].expand(-1, pad, -1, -1)], 1),
            torch.cat([w, w[:, first:first + 1].expand(-1, pad, -1, -1)], 1))


def defects(row, case):
    """name -> the defective restatement (float64, PERIOD samples) on the case's operands; only those that apply to the row"""
    sm = slice(0, PERIOD)
    x, w = case['x'], case['w']
    d = {
        'w_hi x_lo dropped': lambda: f16x3_ref64(row, x, w, samples=sm, drop=('hl',)),
        'w_lo x_hi dropped': lambda: f16x3_ref64(row, x, w, samples=sm, drop=('lh',)),
        'low-half scale 2^-10': lambda: f16x3_ref64(row, x, w, samples=sm, scale=2.0 ** -10),
        'low-half scale 2^-12': lambda: f16x3_ref64(row, x, w, samples=sm, scale=2.0 ** -12),
        'acc1 merged unscaled': lambda: f16x3_ref64(row, x, w, samples=sm, scale=1.0),
        'lo from the unscaled residual': lambda: f16x3_ref64(row, x, w, samples=sm, unscaled_lo=True),
        'hi truncated': lambda: f16x3_ref64(row, x, w, samples=sm, truncate=True),
        'subnormals flushed in hi': lambda: f16x3_ref64(row, x, w, samples=sm, flush=('hi',)),
        'subnormals flushed in lo': lambda: f16x3_ref64(row, x, w, samples=sm, flush=('lo',)),
        'subnormals flushed in both': lambda: f16x3_ref64(row, x, w, samples=sm, flush=('hi', 'lo')),
    }
    if row.cin % 16:
        d['tail channels read as channel 0'] = lambda: f16x3_ref64(row, *_tail_reads_element0(row, x[sm], w))
    if row.c0:
        d['second segment offset by one'] = lambda: f16x3_ref64(row, torch.cat([x[sm, :row.c0], x[sm, row.c0:].roll(1, 1)], 1), w)
    return d


# the regime in which each defect must leave B_acc, and by at least which factor (worst element over the rows it applies to;
# the measured factors are printed and stand in DESIGN.md).  'hi truncated' shows where a truncated hi leaves a residual of
# a whole fp16 ulp: 65504 - 2^-8 -> hi 65472, lo' = 31.996 x 2048 = 65528 -> inf.  The cross-term defects are named beside
# one_huge_among_small: B_acc grows like K U sum|w||x| while a cross term of random signs grows like sqrt(K) 2^-12, so in the
# nominal regime a dropped cross term is only 2.5 - 7 bounds away; where one product of 60000 x w dominates the sum, the
# bound is K U of that product and its own low half stands 2^12 / K bounds clear (60000 is an fp16 number: the OTHER operand
# carries the low half, hence seed 1 for w_hi x_lo).
DEFECT_REGIME = {
    'w_hi x_lo dropped': ('one_huge_among_small', 1, 2.0), 'w_lo x_hi dropped': ('one_huge_among_small', 0, 2.0),
    'low-half scale 2^-10': ('one_huge_among_small', 0, 2.0), 'low-half scale 2^-12': ('one_huge_among_small', 0, 2.0),
    'acc1 merged unscaled': ('nominal', 0, 1e3), 'lo from the unscaled residual': ('one_huge_among_small', 0, 2.0),
    'hi truncated': ('near_max', 0, math.inf),
    'subnormals flushed in hi': ('subnormal_band', 0, 1e3), 'subnormals flushed in lo': ('subnormal_band', 0, 2.0),
    'subnormals flushed in both': ('subnormal_band', 0, 1e3),
    'tail channels read as channel 0': ('nominal', 0, 1e3), 'second segment offset by one': ('nominal', 0, 1e3),
}
HOST_ROWS = ['f16-11-nk1', 'f16-11-nk2', 'f16-s2-refused']        # the small rows: the CPU tests run on these
DEFECT_ROWS = HOST_ROWS[:2] + ['f16-21-nk1', 'f16-12', 'f16-21-nk2']    # PERIOD samples of the large ones


def leave_factor(bad, b):
    """worst |bad - ref| / B_acc over the elements (inf where bad is non-finite and ref is not)"""
    ref, lim = b['ref'], b['b_acc']
    d = (bad - ref).abs() / lim
    d = torch.where(torch.isfinite(bad) | ~torch.isfinite(ref), d, torch.full_like(d, math.inf))
    return float(d[~torch.isnan(d)].max())


# ------------------------------------------------------------------------------------------------------------------ tests
def test_rows_reach_every_instantiation():
    assert {instantiation(r) for r in ROWS if r.family == 'f16x3'} == set(INSTANTIATIONS)
    assert {r.cin for r in ROWS} >= {16, 20, 36, 40} and any(r.cout % 32 and instantiation(r)[0] == 2 for r in ROWS if r.family == 'f16x3')


@pytest.mark.parametrize('rid', [r.id for r in NEW_ROWS])
def test_new_rows_match_the_dispatch_at_256_cus(rid):
    if torch.cuda.is_available() and torch.cuda.get_device_properties(0).multi_processor_count != 256:
        pytest.skip('the table is pinned for 256 CUs')
    rc, info = H.host_query(BY_ID[rid])
    assert rc == 0 and info == tuple(BY_ID[rid].info), (rid, rc, info)


def test_split_is_exact_and_halves_are_fp16():
    g = torch.Generator().manual_seed(1)
    t = torch.cat([torch.randn(4096, generator=g) * s for s in (1.0, 1e-3, 1e-5, 1e-7, 3e4)] + [torch.tensor(NEAR_MAX)])
    t = t[t.abs() < 65520.0]                              # 3e4 N(0, 1) goes beyond: hi would be infinite
    hi, lo, e = split64(t)
    assert torch.equal(hi + lo / LO + e, t.double()) and bool((t.abs() > 65504.0).any())
    assert torch.equal(hi.half().double(), hi) and torch.equal(lo.half().double(), lo)
    inside = (t.abs() >= F16_MIN_NORMAL) & (t.abs() < 65520.0)
    assert bool((e.abs() <= 2.0 ** -22 * t.double().abs())[inside].all())
    assert bool(((t.double() - hi).abs() <= 2.0 ** -11 * t.double().abs())[inside].all())
    below = t.abs() < F16_MIN_NORMAL
    assert bool(below.any()) and bool((e.abs() <= 2.0 ** -36)[below].all()) and bool(((t.double() - hi).abs() <= 2.0 ** -25)[below].all())
    # the switches: flushed halves hold no subnormal, a truncated hi never exceeds |t|
    fh, fl, fe = split64(t, flush=('hi', 'lo'))
    assert not bool(((fh != 0) & (fh.abs() < F16_MIN_NORMAL)).any()) and not bool(((fl != 0) & (fl.abs() < F16_MIN_NORMAL)).any())
    assert torch.equal(fh + fl / LO + fe, t.double())
    th = split64(t, truncate=True)[0]
    assert bool((th.abs() <= t.double().abs()).all()) and bool((th != hi).any())


@pytest.mark.parametrize('regime', ['nominal', 'pow2_scaled', 'near_max', 'cancelling', 'one_huge_among_small'])
def test_model_constant(regime):
    """inside the domain B_model <= c_m 2^-22 sum |w||x|; operands of these regimes below 2^-14 (a few of a normal draw) are
    raised to it first -- the statement is about the domain"""
    for rid in HOST_ROWS[:2]:
        row = BY_ID[rid]
        for seed in SEEDS:
            case = {k: v for k, v in operands(row, regime, seed).items() if not isinstance(k, tuple)}
            for k in 'xw':
                t = case[k]
                case[k] = torch.where((t != 0) & (t.abs() < F16_MIN_NORMAL), torch.sign(t) * F16_MIN_NORMAL, t)
            b = bounds(row, case, variants(row)['plain'], slice(0, PERIOD))
            worst = float((b['b_model'] / (2.0 ** -22 * b['mag'])).max())
            print(f'[measured] {rid} {regime}/{seed}: B_model <= {worst:.3f} x 2^-22 sum|w||x| (c_m = {C_M:.6f})')
            assert worst <= C_M


def test_regimes_are_what_they_claim():
    row = BY_ID['f16-11-nk2']
    plain = variants(row)['plain']
    sm = slice(0, PERIOD)
    for regime in REGIMES:
        for seed in SEEDS:
            case = operands(row, regime, seed)
            assert case['x'].shape[0] == row.n and torch.equal(case['x'][PERIOD:], case['x'][:row.n - PERIOD])
            assert bool(torch.isfinite(case['x']).all() and torch.isfinite(case['w']).all())
            if regime in FINITE:
                assert case['hi_finite'] and bounds(row, case, plain, sm)['finite'], (regime, seed)
    x, w = operands(row, 'subnormal_band', 0)['x'], operands(row, 'subnormal_band', 0)['w']
    assert float(x.abs().min()) >= 2.0 ** -24 and float(x.abs().max()) <= F16_MIN_NORMAL and float(w.abs().max()) <= F16_MIN_NORMAL
    assert float(operands(row, 'near_max', 0)['x'].abs().max()) == 65519.99609375
    assert float(operands(row, 'near_max', 0)['x'].half().float().abs().max()) == 65504.0
    for seed, k in ((0, 'x'), (1, 'w')):
        over = operands(row, 'over_range', seed)
        assert not over['hi_finite'] and int((over[k] == OVER).sum()) == (row.n if k == 'x' else 1)
        assert float(operands(row, 'one_huge_among_small', seed)[k].abs().max()) == 60000.0
    c = operands(row, 'cancelling', 0)
    b = bounds(row, c, plain, sm)
    assert float((b['mag'] >= 1e4 * b['true'].abs()).double().mean()) >= 0.5        # the interior: borders see a partial kernel
    for seed in range(len(POW2_GRID)):          # every half of every grid point is a normal fp16 number or zero
        p = operands(row, 'pow2_scaled', seed)
        for t in (p['x'], p['w']):
            hi, lo, e = split64(t)
            assert bool((e == 0).all()) and float(hi.abs().min()) >= F16_MIN_NORMAL and float(lo.abs().min()) >= F16_MIN_NORMAL
            assert float(hi.abs().max()) <= 65504.0


@pytest.mark.parametrize('regime', FINITE)
def test_fp32_restatements_stay_inside(regime):
    """S evaluated in fp32 with two accumulators, in three summation orders, is within B_acc of f16x3_ref64"""
    plain = None
    for rid in HOST_ROWS[:2]:
        row = BY_ID[rid]
        plain = variants(row)['plain']
        for seed in SEEDS:
            case = operands(row, regime, seed)
            b = bounds(row, case, plain, slice(0, 1))
            for order in ('channel', 'tap', 'pairwise'):
                got = s_fp32(row, case['x'], case['w'], order)
                ratio = float(((got - b['ref']).abs() / b['b_acc']).nan_to_num(0.0).max())
                print(f'[measured] {rid} {regime}/{seed} {order}-major fp32: {ratio:.3f} of B_acc')
                assert bool(torch.isfinite(got).all()) and ratio <= 1.0, (rid, regime, seed, order, ratio)


@pytest.mark.parametrize('name', list(DEFECT_REGIME))
def test_planted_defects_leave_the_bound(name):
    regime, seed, floor = DEFECT_REGIME[name]
    factors = {}
    for rid in DEFECT_ROWS:
        row = BY_ID[rid]
        case = operands(row, regime, seed)
        make = defects(row, case).get(name)
        if make is None:
            continue
        b = bounds(row, case, variants(row)['plain'], slice(0, PERIOD))
        factors[rid] = leave_factor(make(), b)
    print(f'[measured] "{name}" in {regime}/{seed}: leaves B_acc by ' + ', '.join(f'{k}: {v:.3g}' for k, v in factors.items()))
    assert factors and min(factors.values()) >= floor, (name, factors)


def test_weight_criterion():
    """which layers the packer hands to the route: every regime whose weights lie in the domain, not small_w, not a weight
    beyond fp16's range; the unsplit restatement of small_w is outside the fp32-class bound, as the issue's emulation found"""
    row = BY_ID['f16-11-nk1']
    verdict = {}
    for regime in REGIMES:
        for seed in SEEDS:
            w = operands(row, regime, seed)['w']
            ex = float(weight_excess(w).max())
            verdict[(regime, seed)] = ex
            assert float(ops.f16x3_weight_excess(w)) == ex
            print(f'[measured] {regime}/{seed}: worst channel at {ex:.3g} x 2^-22 sum|w| (refused above {CRITERION:g})')
    refused = {k for k, v in verdict.items() if v > CRITERION}
    assert refused == {('small_w', 0), ('small_w', 1), ('subnormal_band', 0), ('subnormal_band', 1), ('over_range', 1)}, verdict
    for seed in SEEDS:
        case = operands(row, 'small_w', seed)
        b = bounds(row, case, variants(row)['plain'], slice(0, PERIOD))
        over = float(((b['ref'] - b['true']).abs() / (C_M * 2.0 ** -22 * b['mag'] + b['b_acc'])).max())
        print(f'[measured] small_w/{seed}: the split restatement is at {over:.3g} of c_m 2^-22 sum|w||x| + B_acc')
        pc = ops.PackedConv.from_weight(case['w'], None, stride=row.stride, padding=row.pad)
        assert pc.wp16 is None
        if seed == 1:
            assert over > 1.0
    assert ops.PackedConv.from_weight(operands(row, 'nominal', 0)['w'], None, padding=row.pad).wp16 is not None
    assert ops.PackedConv.from_weight(torch.zeros(row.cout, row.cin, 3, 3), None, padding=row.pad).wp16 is not None
