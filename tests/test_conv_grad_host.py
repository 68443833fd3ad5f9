"""CPU: backward of the pose head's convolutions (conv_grad.hip) -- the input and the weight gradient of a 3x3 / stride-2 /
pad-1 convolution on the matrix cores -- restated in float64 as explicit index sums, with a per-element bound for any
fp32 evaluation in the kernels' operation order, the inputs tests/test_gpu_conv_grad.py feeds the HIP kernels, fp32
emulations in the kernels' order (fma chains) with planted defects, and the composed float64 head (three convolutions,
GroupNorms 0 and 1, the fully connected tail of tests/test_fc_grad_host.py) held against float64 autograd.

  dgrad   gx = sum_{tap, co} g w:   gamma_d sum |g| |w|  +  sum (bound of g) |w| (1 + gamma_d),  d = DGRAD_DEPTH(Cout, taps)
          taps = 1, 2, 2 or 4 by the parity of (iy, ix); a border element's sum holds only the taps that exist
  wgrad   dW = sum_{m, oy, ox} g x: gamma_d sum |g| |x|  +  carried bounds of g and of x,        d = WGRAD_DEPTH(plan)
v_mfma_f32_32x32x2_f32 rounds once per fused multiply-add; underflow is outside the model, as in test_fc_host.
"""
import os
import re

import numpy as np
import pytest
import torch

from test_stream_ops_host import IN_EPS, f64, measured, worst_ratio  # noqa: E402
from test_fc_host import gamma  # noqa: E402
import test_fc_grad_host as HF  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, 'scflow_amd', 'csrc', 'conv_grad.hip')).read()


def _define(name):
    return int(re.search(rf'#define\s+{name}\s+(\d+)', SRC).group(1))


DG_CHUNK, DG_PIX, DG_CI = _define('DG_CHUNK'), _define('DG_PIX'), _define('DG_CI')
WG_TILE, WG_PIX, WG_MIN_CHUNKS, WG_BLOCKS = _define('WG_TILE'), _define('WG_PIX'), _define('WG_MIN_CHUNKS'), _define('WG_BLOCKS')
EXTRA = 0                           # added to every depth: 0 for the kernels; the golden test raises it for torch's own fp32


def out_size(n):
    return (n - 1) // 2 + 1


# ================================================================================================ depths, from the source
def dgrad_depth(cout, taps):
    """cg_dgrad_kernel: `acc = mfma_f32_32x32x2f32(a, bp[...], acc)` x DG_CHUNK / 2 per step, two columns each, over
    taps x ceil(Cout / DG_CHUNK) steps of the zero-filled tiles: 1 product + that many accumulations."""
    return 1 + taps * DG_CHUNK * -(-cout // DG_CHUNK) + EXTRA


def wgrad_plan(q, cout, cin):
    """cg_wgrad_plan: (chunks per split, splits) of a contraction over q output pixels."""
    tiles = -(-cout // WG_TILE) * -(-cin // WG_TILE)
    chunks = -(-q // WG_PIX)
    cps = max(WG_MIN_CHUNKS, -(-chunks // max(1, WG_BLOCKS // tiles)))
    return cps, -(-chunks // cps)


def wgrad_depth(q, cout, cin, accumulate=False):
    """cg_wgrad_kernel: one chain per split (1 product + WG_PIX accumulations per chunk, at most cps chunks);
    cg_wgrad_combine_kernel: `tot = tot + ws[...]` x (S - 1), `tot + *d` under accumulate."""
    cps, splits = wgrad_plan(q, cout, cin)
    return 1 + WG_PIX * min(cps, -(-q // WG_PIX)) + (splits - 1) + (1 if accumulate else 0) + EXTRA


# ===================================================================================================== float64 pieces
def _taps(hin, win, ho, wo, stride=2, pad=1):
    """every (ky, kx) with the output rows / columns whose tap lands inside the input, and where"""
    for ky in range(3):
        oy = np.array([o for o in range(ho) if 0 <= stride * o - pad + ky < hin], dtype=np.int64)
        for kx in range(3):
            ox = np.array([o for o in range(wo) if 0 <= stride * o - pad + kx < win], dtype=np.int64)
            if oy.size and ox.size:
                yield ky, kx, oy, ox, stride * oy - pad + ky, stride * ox - pad + kx


def dgrad_sum(g, w, hin, win, stride=2, pad=1):
    """gx[m, ci, iy, ix] = sum over (ky, kx, co) and the output pixels with stride o - pad + k = i, as index sums"""
    m, cout, ho, wo = g.shape
    gx = np.zeros((m, w.shape[1], hin, win))
    for ky, kx, oy, ox, iy, ix in _taps(hin, win, ho, wo, stride, pad):
        gx[:, :, iy[:, None], ix[None, :]] += np.einsum('mohw,oc->mchw', g[:, :, oy[:, None], ox[None, :]], w[:, :, ky, kx], optimize=True)
    return gx


def wgrad_sum(g, x, stride=2, pad=1):
    """dW[co, ci, ky, kx] = sum over (m, oy, ox) of g x[.., stride o - pad + k], zero outside the map"""
    m, cout, ho, wo = g.shape
    dw = np.zeros((cout, x.shape[1], 3, 3))
    for ky, kx, oy, ox, iy, ix in _taps(x.shape[2], x.shape[3], ho, wo, stride, pad):
        dw[:, :, ky, kx] = np.einsum('mohw,mchw->oc', g[:, :, oy[:, None], ox[None, :]], x[:, :, iy[:, None], ix[None, :]], optimize=True)
    return dw


def tap_count(hin, win):
    """taps of the chain of every input pixel: the parity class decides, a missing border tap still takes its steps"""
    ty = np.where(np.arange(hin) % 2 == 1, 2, 1)
    tx = np.where(np.arange(win) % 2 == 1, 2, 1)
    return ty[:, None] * tx[None, :]


def dgrad_ref(g, gb, w, hin, win):
    """-> (gx, bound) over (M, Cin, Hin, Win); gb: bound of g (scalar or array)"""
    g, w = f64(g), f64(w)
    gb = np.broadcast_to(np.asarray(gb, dtype=np.float64), g.shape)
    taps = tap_count(hin, win)
    gm = np.vectorize(lambda t: gamma(dgrad_depth(g.shape[1], int(t))))(taps)[None, None]
    with np.errstate(all='ignore'):
        ref = dgrad_sum(g, w, hin, win)
        b = gm * dgrad_sum(np.abs(g), np.abs(w), hin, win) + dgrad_sum(gb, np.abs(w), hin, win) * (1 + gm)
    return ref, b


def wgrad_ref(g, gb, x, xb=0.0, prev=None):
    """-> (dW, bound) over (Cout, Cin, 3, 3); gb, xb: bounds of g and of x; prev: the tensor the call accumulates into"""
    g, x = f64(g), f64(x)
    gb = np.broadcast_to(np.asarray(gb, dtype=np.float64), g.shape)
    xb = np.broadcast_to(np.asarray(xb, dtype=np.float64), x.shape)
    gm = gamma(wgrad_depth(g.shape[0] * g.shape[2] * g.shape[3], g.shape[1], x.shape[1], prev is not None))
    with np.errstate(all='ignore'):
        ref, sh = wgrad_sum(g, x), wgrad_sum(np.abs(g), np.abs(x))
        carried = wgrad_sum(gb, np.abs(x) + xb) + wgrad_sum(np.abs(g), xb)
        if prev is not None:
            ref, sh = ref + f64(prev), sh + np.abs(f64(prev))
    return ref, gm * sh + carried * (1 + gm)


# ============================================================================================================= cases
# (M, Cout, C0, C1, Hin, Win): every M in {1, 2, 3, 33}, Cout in {1, 31, 32, 33, 128}, (C0, C1) in {(1, 0), (3, 2), (32, 0),
# (33, 31), (128, 96)}, Hin x Win in {1x1, 2x2, 3x5, 5x3, 4x4, 8x8} several times, every pair of axes in several
# combinations; partial tiles of every kind (pixels of a parity class: 0, < 64, > 64; channels < 32, = 32, 33, 64, 224 =
# 128 + 96; output channels short of / past a chunk), more than one wgrad split (Q > 256: the 8x8 maps at M = 33)
CASES = [
    (1, 1, 1, 0, 1, 1), (2, 1, 1, 0, 2, 2), (3, 31, 3, 2, 3, 5), (33, 32, 3, 2, 5, 3), (1, 32, 32, 0, 4, 4),
    (2, 128, 32, 0, 8, 8), (3, 33, 33, 31, 8, 8), (1, 128, 128, 96, 4, 4), (2, 31, 128, 96, 3, 5), (33, 33, 33, 31, 2, 2),
    (3, 32, 1, 0, 5, 3), (2, 1, 33, 31, 1, 1), (33, 31, 32, 0, 8, 8), (1, 32, 3, 2, 2, 2), (3, 128, 1, 0, 1, 1),
    (2, 33, 128, 96, 5, 3), (33, 1, 3, 2, 4, 4), (1, 31, 33, 31, 8, 8), (2, 32, 128, 96, 2, 2), (3, 1, 32, 0, 3, 5),
    (33, 128, 1, 0, 3, 5), (1, 33, 1, 0, 5, 3), (2, 31, 1, 0, 4, 4), (3, 32, 33, 31, 1, 1), (33, 33, 32, 0, 1, 1),
    (1, 128, 3, 2, 2, 2), (2, 1, 128, 96, 8, 8), (3, 31, 32, 0, 2, 2), (33, 32, 128, 96, 4, 4), (1, 1, 33, 31, 3, 5),
    (33, 32, 3, 2, 8, 8),
]
LAYER0 = (2, 128, 128, 96, 32, 32)          # the shipped first layer, two samples
REGIMES = ['nominal', 'cancelling', 'offset', 'scaled']
SCALES = (40, 20)                            # powers of two on g and on the other operand
REGIME_CASES = [CASES[6], CASES[12], CASES[3], CASES[8]]


def conv_case(regime, m, cout, c0, c1, hin, win, seed=0):
    """g (M, Cout, Ho, Wo) cotangent, w (Cout, Cin, 3, 3), x (M, Cin, Hin, Win) post-ReLU activation; scale of the results"""
    cin, ho, wo = c0 + c1, out_size(hin), out_size(win)
    gen = torch.Generator().manual_seed(9100 + seed + m + 3 * cout + 7 * cin + 11 * hin + 13 * win)
    g = torch.randn((m, cout, ho, wo), generator=gen)
    w = torch.randn((cout, cin, 3, 3), generator=gen) * (9 * cout) ** -0.5
    x = torch.relu(torch.randn((m, cin, hin, win), generator=gen))
    if regime == 'cancelling':               # halves of the contraction cancel to 1e-4 of the shadow (dgrad: co, wgrad: m)
        h = cout // 2
        if h:
            g[:, h:2 * h] = g[:, :h]
            w[h:2 * h] = -w[:h] * (1 + 1e-4 * torch.randn(w[:h].shape, generator=gen))
        hm = m // 2
        if hm:
            x[hm:2 * hm] = x[:hm]
            g[hm:2 * hm] = -g[:hm] * (1 + 1e-4 * torch.randn(g[:hm].shape, generator=gen))
    if regime == 'offset':
        g, w, x = g + 2.0, w + 1.0, x + 4.0
    scale = 1.0
    if regime == 'scaled':
        g, w, x, scale = g * 2.0 ** SCALES[0], w * 2.0 ** SCALES[1], x * 2.0 ** SCALES[1], 2.0 ** (SCALES[0] + SCALES[1])
    return g.contiguous(), w.contiguous(), x.contiguous(), scale


# ================================================================================ fp32 emulations in the kernels' order
def fma(a, b, c):
    """fl(a b + c): the product of two fp32 is exact in float64, the sum is rounded to float64 first (2^-53: the double
    rounding changes a result only on a tie broken 2^-29 ulp away)"""
    return (a.double() * b.double() + c.double()).float()


def dgrad_fp32(g, w, hin, win, defect=None):
    """cg_dgrad_kernel: per parity class the taps in ascending (ky, kx), co ascending inside a tap, one fma chain from +0"""
    m, cout, ho, wo = g.shape
    cin = w.shape[1]
    if defect == 'ci_co_exchanged':
        w = w.reshape(cin, cout, 3, 3).permute(1, 0, 2, 3)           # the (Cout, Cin) buffer indexed [ci][co]
    if defect == 'tap_mirrored_y':
        w = w.flip(2)
    if defect == 'tap_mirrored_x':
        w = w.flip(3)
    gx = torch.zeros((m, cin, hin, win))
    for py in (0, 1):
        for px in (0, 1):
            hc, wc = (hin + 1 - py) // 2, (win + 1 - px) // 2
            if hc == 0 or wc == 0:
                continue
            acc = torch.zeros((m, cin, hc, wc))
            for ky in ((0, 2) if py else (1,)):
                for kx in ((0, 2) if px else (1,)):
                    oy = torch.arange(hc) + (1 if ky == 0 else 0)
                    ox = torch.arange(wc) + (1 if kx == 0 else 0)
                    lim_y = hin // 2 if defect == 'border_tap_dropped' else ho
                    lim_x = win // 2 if defect == 'border_tap_dropped' else wo
                    vy, vx = oy < lim_y, ox < lim_x
                    if defect == 'border_tap_kept':                    # the row past the map read as the last row
                        vy, vx = torch.ones_like(vy), torch.ones_like(vx)
                    gt = g[:, :, oy.clamp(max=ho - 1)][:, :, :, ox.clamp(max=wo - 1)] * (vy[:, None] & vx[None, :])
                    for co in range(cout):
                        acc = fma(gt[:, co, None], w[co, :, ky, kx][None, :, None, None], acc)
            gx[:, :, py::2, px::2] = acc
    return gx


def wgrad_fp32(g, x, prev=None, defect=None):
    """cg_wgrad_kernel + combine: per split one fma chain from +0 over its pixels (m, oy, ox) ascending; partial 0, +
    partial 1 ..., + the previous value last"""
    m, cout, ho, wo = g.shape
    cin, hin, win = x.shape[1:]
    q_all = m * ho * wo
    cps, splits = wgrad_plan(q_all, cout, cin)
    xp = torch.nn.functional.pad(x, (1, 1, 1, 1), mode='replicate' if defect == 'border_tap_kept' else 'constant')
    if defect == 'border_tap_kept':
        xp[:, :, 0], xp[:, :, :, 0] = 0.0, 0.0                     # the near border stays zero; the far one is read clamped
    if defect == 'wgrad_last_chunk_dropped':
        q_all = (q_all - 1) // WG_PIX * WG_PIX
    tot = None
    for s in range(splits):
        acc = torch.zeros((cout, cin, 3, 3))
        for q in range(s * cps * WG_PIX, min((s + 1) * cps * WG_PIX, q_all)):
            ox, oy, mm = q % wo, (q // wo) % ho, q // (wo * ho)
            acc = fma(g[mm, :, oy, ox][:, None, None, None], xp[mm, :, 2 * oy:2 * oy + 3, 2 * ox:2 * ox + 3][None], acc)
        tot = acc if tot is None else tot + acc
    if defect == 'tap_mirrored_y':
        tot = tot.flip(2)
    if defect == 'tap_mirrored_x':
        tot = tot.flip(3)
    if prev is None or defect == 'accumulate_overwrites':
        return tot
    return tot + prev


def other_geometry_fp32(g, w, x, stride, pad):
    """what a kernel with another stride or padding would return (no particular order: it only has to leave the bound)"""
    return (torch.from_numpy(dgrad_sum(f64(g), f64(w), x.shape[2], x.shape[3], stride, pad)).float(),
            torch.from_numpy(wgrad_sum(f64(g), f64(x), stride, pad)).float())


# ===================================================================================================== the self-checks
def test_symbols_are_declared_exported_and_bound():
    from scflow_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'scflow_hip.h')).read()
    for name in ('scf_conv_dgrad', 'scf_conv_wgrad', 'scf_conv_wgrad_workspace'):
        assert re.search(rf'\b{name}\s*\(', header), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    from scflow_amd import ops
    assert all(hasattr(ops, n) for n in ('conv_dgrad', 'conv_wgrad', 'conv_wgrad_workspace'))


def test_depths_and_plan_are_the_counts_of_the_source():
    from scflow_amd import _lib
    lib = _lib.load()
    assert (DG_CHUNK, DG_PIX, DG_CI, WG_TILE, WG_PIX, WG_MIN_CHUNKS, WG_BLOCKS) == (32, 64, 128, 64, 16, 16, 512)
    assert [dgrad_depth(c, t) for c, t in ((1, 1), (32, 4), (33, 2), (128, 4))] == [33, 129, 129, 513]
    assert wgrad_plan(256 * 256, 128, 224) == (64, 64) and wgrad_plan(256 * 16, 128, 128) == (16, 16)
    assert wgrad_plan(33 * 16, 31, 32) == (16, 3) and wgrad_plan(1, 1, 1) == (16, 1)
    assert wgrad_depth(33 * 16, 31, 32) == 1 + 256 + 2 and wgrad_depth(4, 1, 1, True) == 1 + 16 + 1
    for m, cout, c0, c1, hin, win in CASES + [LAYER0, (256, 128, 128, 96, 32, 32), (256, 128, 128, 0, 16, 16)]:
        ho, wo, cin = out_size(hin), out_size(win), c0 + c1
        assert lib.scf_conv_wgrad_workspace(m, cout, cin, ho, wo) == wgrad_plan(m * ho * wo, cout, cin)[1] * 9 * cout * cin
    assert lib.scf_conv_wgrad_workspace(0, 1, 1, 1, 1) < 0 and lib.scf_conv_wgrad_workspace(1, 1, 1, 0, 1) < 0


def test_cases_cover_every_value_of_every_axis():
    assert {c[0] for c in CASES} == {1, 2, 3, 33} and {c[1] for c in CASES} == {1, 31, 32, 33, 128}
    assert {c[2:4] for c in CASES} == {(1, 0), (3, 2), (32, 0), (33, 31), (128, 96)}
    assert {c[4:] for c in CASES} == {(1, 1), (2, 2), (3, 5), (5, 3), (4, 4), (8, 8)}
    assert len(CASES) <= 32 and any(wgrad_plan(c[0] * out_size(c[4]) * out_size(c[5]), c[1], c[2] + c[3])[1] > 1 for c in CASES)


def _torch_grads(g, w, x, stride=2, pad=1):
    wt = torch.tensor(f64(w), requires_grad=True)
    xt = torch.tensor(f64(x), requires_grad=True)
    y = torch.nn.functional.conv2d(xt, wt, stride=stride, padding=pad)
    (y * torch.tensor(f64(g))).sum().backward()
    return xt.grad.numpy(), wt.grad.numpy()


def test_index_sums_equal_float64_autograd():
    worst = 0.0
    for case in CASES:
        g, w, x, _ = conv_case('nominal', *case)
        gx, dw = _torch_grads(g, w, x)
        for got, want in ((dgrad_sum(f64(g), f64(w), *x.shape[2:]), gx), (wgrad_sum(f64(g), f64(x)), dw)):
            worst = max(worst, float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300)))
    measured('conv index sums - float64 autograd, relative to the largest entry', worst)
    assert worst <= 1e-14


def _emulation_inputs():
    for case in CASES:
        yield 'nominal', case
    for case in REGIME_CASES:
        for regime in REGIMES[1:]:
            yield regime, case


def _worst(defect=None):
    worst = {}

    def put(fam, got, ref_b):
        worst[fam] = max(worst.get(fam, 0.0), worst_ratio(got, *ref_b))

    for regime, case in _emulation_inputs():
        m, cout, c0, c1, hin, win = case
        g, w, x, _ = conv_case(regime, *case)
        if defect in (None, 'ci_co_exchanged', 'tap_mirrored_y', 'tap_mirrored_x', 'border_tap_kept', 'border_tap_dropped'):
            if defect == 'ci_co_exchanged' and cout != c0 + c1:
                continue
            put('dgrad ' + regime, dgrad_fp32(g, w, hin, win, defect), dgrad_ref(g, 0.0, w, hin, win))
        if defect in (None, 'tap_mirrored_y', 'tap_mirrored_x', 'border_tap_kept', 'wgrad_last_chunk_dropped'):
            if m * cout * (c0 + c1) > 33 * 33 * 64 and regime == 'nominal' and defect is not None:
                continue                                               # the defects do not need the heavy shapes
            put('wgrad ' + regime, wgrad_fp32(g, x, defect=defect), wgrad_ref(g, 0.0, x))
        if defect in ('pad0', 'pad2', 'stride1'):
            stride, pad = {'pad0': (2, 0), 'pad2': (2, 2), 'stride1': (1, 1)}[defect]
            gx, dw = other_geometry_fp32(g, w, x, stride, pad)
            put('dgrad ' + regime, gx, dgrad_ref(g, 0.0, w, hin, win))
            put('wgrad ' + regime, dw, wgrad_ref(g, 0.0, x))
        if defect == 'second_part_offset' and c1:
            gx = dgrad_fp32(g, w, hin, win)
            gx[:, c0:] = gx[:, :c1]                                    # the second part written from the first part's offset
            put('dgrad ' + regime, gx, dgrad_ref(g, 0.0, w, hin, win))
            xs = x.clone()
            xs[:, c0:] = x[:, :c1]                                     # ... read at the first part's offset
            put('wgrad ' + regime, wgrad_fp32(g, xs), wgrad_ref(g, 0.0, x))
        if defect == 'accumulate_overwrites':
            prev = torch.randn((cout, c0 + c1, 3, 3), generator=torch.Generator().manual_seed(3))
            put('wgrad ' + regime, wgrad_fp32(g, x, prev, defect), wgrad_ref(g, 0.0, x, prev=prev))
    return worst


def test_emulations_inside_the_bounds():
    for fam, v in _worst().items():
        measured(f'conv_grad fp32 emulation / bound, {fam}', v)
        assert v <= 1.0, fam


DEFECTS = ['ci_co_exchanged', 'tap_mirrored_y', 'tap_mirrored_x', 'pad0', 'pad2', 'stride1', 'border_tap_kept',
           'border_tap_dropped', 'second_part_offset', 'wgrad_last_chunk_dropped', 'accumulate_overwrites']


@pytest.mark.parametrize('defect', DEFECTS)
def test_planted_defects_outside(defect):
    worst = _worst(defect)
    assert worst, defect
    for fam, v in worst.items():
        measured(f'defect {defect} / bound, {fam} (worst case of the GPU lists)', v)
    assert max(worst.values()) > 1.0
    if defect in ('tap_mirrored_y', 'tap_mirrored_x', 'pad0', 'pad2', 'stride1', 'second_part_offset', 'border_tap_kept'):
        assert all(v > 1.0 for fam, v in worst.items() if fam.endswith('nominal')), worst     # both kernels notice


def test_accumulate_is_one_more_rounding():
    g, w, x, _ = conv_case('nominal', *CASES[12])
    prev = torch.randn(w.shape, generator=torch.Generator().manual_seed(1))
    dw = wgrad_fp32(g, x, prev)
    assert worst_ratio(dw, *wgrad_ref(g, 0.0, x, prev=prev)) <= 1.0
    assert torch.equal(dw, wgrad_fp32(g, x) + prev)


# ================================================================================================ the composed head
def conv_fwd64(x, w):
    """F.conv2d(stride=2, padding=1) as index sums"""
    m, cin, hin, win = x.shape
    ho, wo = out_size(hin), out_size(win)
    y = np.zeros((m, w.shape[0], ho, wo))
    for ky, kx, oy, ox, iy, ix in _taps(hin, win, ho, wo):
        y[:, :, oy[:, None], ox[None, :]] += np.einsum('mchw,oc->mohw', x[:, :, iy[:, None], ix[None, :]], w[:, :, ky, kx], optimize=True)
    return y


def gn64(y, gam, bet, groups):
    """GroupNorm + affine on (M, C, h, w) float64 -> (pre-activation u, xh, rstd) with the group axis flattened back"""
    m, c, h, w = y.shape
    yg = y.reshape(m, groups, -1)
    mean = yg.mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(((yg - mean) ** 2).mean(-1, keepdims=True) + float(np.float32(IN_EPS)))
    xh = ((yg - mean) * rstd).reshape(y.shape)
    return xh * gam[None, :, None, None] + bet[None, :, None, None], xh, rstd


def gn_grad64(y, g_a, mask, gam, groups):
    """backward of relu(GroupNorm(y)) given the mask -> (g_y, dgamma, dbeta)"""
    m, c, h, w = y.shape
    _, xh, rstd = gn64(y, gam, np.zeros_like(gam), groups)
    gu = g_a * mask
    t = (gu * gam[None, :, None, None]).reshape(m, groups, -1)
    xg = xh.reshape(m, groups, -1)
    g_y = (rstd * (t - t.mean(-1, keepdims=True) - xg * (t * xg).mean(-1, keepdims=True))).reshape(y.shape)
    return g_y, (gu * xh).sum((0, 2, 3)), gu.sum((0, 2, 3))


CONV_NAMES = ['conv_layers.0.conv.weight', 'conv_layers.0.gn.weight', 'conv_layers.0.gn.bias', 'conv_layers.1.conv.weight',
              'conv_layers.1.gn.weight', 'conv_layers.1.gn.bias', 'conv_layers.2.conv.weight']


def conv_stack_ref64(x, ys, p, g_y2, groups, masks=None, defect=None):
    """The three convolutions with GroupNorms 0 and 1, backward, in float64.  x (M, Cin, h, w); ys = (y0, y1): the raw
    outputs of the first two convolutions (None: computed here); p: float64 arrays keyed by CONV_NAMES; g_y2: the cotangent
    at the last convolution's raw output; masks = (a0 > 0, a1 > 0) or None: decided here.  -> dict of gradients and
    intermediates."""
    W0, W1, W2 = (p[f'conv_layers.{i}.conv.weight'] for i in range(3))
    gam0, bet0, gam1, bet1 = (p[f'conv_layers.{i}.gn.{k}'] for i in (0, 1) for k in ('weight', 'bias'))
    y0 = conv_fwd64(x, W0) if ys is None else ys[0]
    u0 = gn64(y0, gam0, bet0, groups)[0]
    m0 = (u0 > 0) if masks is None else masks[0]
    a0 = u0 * m0
    y1 = conv_fwd64(a0, W1) if ys is None else ys[1]
    u1 = gn64(y1, gam1, bet1, groups)[0]
    m1 = (u1 > 0) if masks is None else masks[1]
    a1 = u1 * m1
    y2 = conv_fwd64(a1, W2)
    dw2 = wgrad_sum(g_y2, a1)
    g_a1 = dgrad_sum(g_y2, W2, *a1.shape[2:])
    mk1 = m1
    if defect == 'gn_mask_from_layer0':                                # layer 0's mask, sub-sampled to layer 1's map
        mk1 = np.ascontiguousarray(m0[:, :, ::2, ::2][:, :, :m1.shape[2], :m1.shape[3]])
    g_y1, dg1, db1 = gn_grad64(a1 if defect == 'a_for_y' else y1, g_a1, mk1, gam1, groups)
    dw1 = wgrad_sum(g_y1, a0)
    g_a0 = dgrad_sum(g_y1, W1, *a0.shape[2:])
    g_y0, dg0, db0 = gn_grad64(y0, g_a0, m0, gam0, groups)
    dw0 = wgrad_sum(g_y0, x)
    g_x = dgrad_sum(g_y0, W0, *x.shape[2:])
    out = dict(zip(CONV_NAMES, (dw0, dg0, db0, dw1, dg1, db1, dw2)))
    out.update(g_x=g_x, y0=y0, y1=y1, y2=y2, a0=a0, a1=a1, g_a1=g_a1, g_y1=g_y1, g_a0=g_a0, g_y0=g_y0, m0=m0, m1=m1)
    return out


def conv_stack_bounds(ref, x, p, g_y2, b_gy2, groups, act_bounds=(0.0, 0.0)):
    """the composed bound around conv_stack_ref64's result: every stage's bound goes through the next stage's sum of
    magnitudes (dgrad_ref / wgrad_ref / test_fc_grad_host.gn_grad_ref with their carried terms); act_bounds = (a0b, a1b):
    bounds of the recomputed activations (0 when the reference was given the kernel's own a)."""
    a0b, a1b = act_bounds
    W0, W1, W2 = (p[f'conv_layers.{i}.conv.weight'] for i in range(3))
    m = x.shape[0]
    flat = lambda t: np.ascontiguousarray(t).reshape(m, -1)            # noqa: E731

    def norm(y, g_a, gb, mask, gam):
        c, hw = y.shape[1], y.shape[2] * y.shape[3]
        (_, b_gy), (_, b_dg), (_, b_db) = HF.gn_grad_ref(flat(y), flat(g_a), flat(np.broadcast_to(gb, g_a.shape)), flat(mask),
                                                         gam, c * hw // groups, hw)
        return b_gy.reshape(y.shape), b_dg, b_db

    _, bw2 = wgrad_ref(g_y2, b_gy2, ref['a1'], a1b)
    _, b_a1 = dgrad_ref(g_y2, b_gy2, W2, *ref['a1'].shape[2:])
    b_y1, bg1, bb1 = norm(ref['y1'], ref['g_a1'], b_a1, ref['m1'], p['conv_layers.1.gn.weight'])
    _, bw1 = wgrad_ref(ref['g_y1'], b_y1, ref['a0'], a0b)
    _, b_a0 = dgrad_ref(ref['g_y1'], b_y1, W1, *ref['a0'].shape[2:])
    b_y0, bg0, bb0 = norm(ref['y0'], ref['g_a0'], b_a0, ref['m0'], p['conv_layers.0.gn.weight'])
    _, bw0 = wgrad_ref(ref['g_y0'], b_y0, x, 0.0)
    _, b_x = dgrad_ref(ref['g_y0'], b_y0, W0, *x.shape[2:])
    out = dict(zip(CONV_NAMES, (bw0, bg0, bb0, bw1, bg1, bb1, bw2)))
    out['g_x'] = b_x
    return out


def stack_params(cin, c, seed=0):
    rs = np.random.RandomState(4321 + seed)
    r = lambda *s: rs.standard_normal(s)                               # noqa: E731
    p = {}
    for i, ci in enumerate((cin, c, c)):
        p[f'conv_layers.{i}.conv.weight'] = r(c, ci, 3, 3) * (9 * ci) ** -0.5
        if i < 2:
            p[f'conv_layers.{i}.gn.weight'] = 1.0 + 0.3 * r(c)
            p[f'conv_layers.{i}.gn.bias'] = 0.2 * r(c)
    return p


def _torch_stack(x, p, g_y2, groups):
    t = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in p.items()}
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    F = torch.nn.functional
    a = xt
    for i in range(3):
        a = F.conv2d(a, t[f'conv_layers.{i}.conv.weight'], stride=2, padding=1)
        if i < 2:
            a = torch.relu(F.group_norm(a, groups, t[f'conv_layers.{i}.gn.weight'], t[f'conv_layers.{i}.gn.bias'],
                                        float(np.float32(IN_EPS))))
    (a * torch.tensor(g_y2)).sum().backward()
    out = {k: v.grad.numpy() for k, v in t.items()}
    out['g_x'] = xt.grad.numpy()
    return out, a.detach().numpy()


@pytest.mark.parametrize('hw', [(8, 8), (12, 20), (5, 7)], ids=lambda v: f'{v[0]}x{v[1]}')
def test_composed_stack_equals_float64_autograd(hw):
    rs = np.random.RandomState(11)
    m, cin, c, groups = 3, 7, 8, 2
    p = stack_params(cin, c)
    x = rs.standard_normal((m, cin) + hw)
    h2 = (out_size(out_size(out_size(hw[0]))), out_size(out_size(out_size(hw[1]))))
    g_y2 = rs.standard_normal((m, c) + h2)
    got = conv_stack_ref64(x, None, p, g_y2, groups)
    want, y2 = _torch_stack(x, p, g_y2, groups)
    worst = float(np.abs(got['y2'] - y2).max() / np.abs(y2).max())
    for key, wv in want.items():
        worst = max(worst, float(np.abs(got[key] - wv).max() / np.abs(wv).max()))
    measured(f'composed convolution stack {hw} - float64 autograd, relative to the largest entry', worst)
    assert worst <= 1e-12


@pytest.mark.parametrize('mode', [0, 1])
def test_composed_head_equals_float64_autograd(mode):
    """convolutions, both GroupNorms and the tail of test_fc_grad_host.py, against one float64 autograd graph"""
    rs = np.random.RandomState(12)
    n, cin, c, groups, hw, nc = 3, 5, 8, 2, (8, 8), 3
    p = stack_params(cin, c, seed=1)
    tail = {k: f64(v) for k, v in HF.tail_params(c, 12, 10, nc, 1, seed=2).items()}           # 8x8 -> 1x1: K = c, hw = 1
    x = rs.standard_normal((n, cin) + hw)
    g_rot, g_tr = rs.standard_normal((n, 6)), rs.standard_normal((n, 3))
    cls = HF.clamp_class([2, 0, 1], n, n, nc, mode)
    fwd = conv_stack_ref64(x, None, p, np.zeros((n, c, 1, 1)), groups)
    tref = HF.tail_ref64(fwd['y2'].reshape(n, c), tail, cls, g_rot, g_tr, c // groups, 1)
    got = conv_stack_ref64(x, None, p, tref['g_y'].reshape(n, c, 1, 1), groups)
    # one autograd graph through everything
    F = torch.nn.functional
    t = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in {**p, **tail}.items()}
    xt = torch.tensor(x, requires_grad=True)
    a = xt
    for i in range(3):
        a = F.conv2d(a, t[f'conv_layers.{i}.conv.weight'], stride=2, padding=1)
        gw, gb = (t[f'conv_layers.{i}.gn.weight'], t[f'conv_layers.{i}.gn.bias']) if i < 2 else (t['gamma'], t['beta'])
        a = torch.relu(F.group_norm(a, groups, gw, gb, float(np.float32(IN_EPS))))
    a = torch.relu(a.reshape(n, c) @ t['W1'].T + t['b1'])
    a = torch.relu(a @ t['W2'].T + t['b2'])
    rot = (a @ t['Wr'].T + t['br']).reshape(n, nc, 6)[torch.arange(n), torch.from_numpy(cls)]
    tr = (a @ t['Wt'].T + t['bt']).reshape(n, nc, 3)[torch.arange(n), torch.from_numpy(cls)]
    ((rot * torch.tensor(g_rot)).sum() + (tr * torch.tensor(g_tr)).sum()).backward()
    worst = 0.0
    for key in CONV_NAMES + ['g_x']:
        want = (xt if key == 'g_x' else t[key]).grad.numpy()
        worst = max(worst, float(np.abs(got[key] - want).max() / max(np.abs(want).max(), 1e-300)))
    for key in tail:
        want = t[key].grad.numpy()
        worst = max(worst, float(np.abs(tref[key] - want).max() / max(np.abs(want).max(), 1e-300)))
    measured(f'composed float64 head - float64 autograd, label_mode {mode}', worst)
    assert worst <= 1e-12


@pytest.mark.parametrize('defect', ['gn_mask_from_layer0', 'a_for_y'])
def test_planted_stack_defects_outside(defect):
    """a defect between the stages: the float64 stack with the defect, rounded to fp32, against the composed bound"""
    rs = np.random.RandomState(13)
    m, cin, c, groups, hw = 3, 7, 8, 2, (8, 8)
    p = stack_params(cin, c)
    x = rs.standard_normal((m, cin) + hw)
    g_y2 = rs.standard_normal((m, c, 1, 1))
    ref = conv_stack_ref64(x, None, p, g_y2, groups)
    bounds = conv_stack_bounds(ref, x, p, g_y2, 0.0, groups)
    good = conv_stack_ref64(x, None, p, g_y2, groups)
    bad = conv_stack_ref64(x, None, p, g_y2, groups, defect=defect)
    f32 = lambda v: v.astype(np.float32)                               # noqa: E731
    keys = CONV_NAMES[:6] + ['g_x']
    assert max(worst_ratio(f32(good[k]), ref[k], bounds[k]) for k in keys) <= 1.0
    worst = max(worst_ratio(f32(bad[k]), ref[k], bounds[k]) for k in keys)
    measured(f'defect {defect} / composed bound', worst)
    assert worst > 1.0


# ============================================================================== the reference's own head (golden fixture)
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'pose_head_grads.npz')
GOLDEN_FEAT_SIZES = [(8, 8), (12, 20)]
GOLDEN_FC_SIZE = {(12, 20): (16, 24)}       # the declared feat_size only sizes fc1: 12 x 20 maps end as 128 x 2 x 3 = 768 features
GOLDEN_LABELS = [2, 0, 1]                   # differing: the reference selects label[0] = 2 for the whole batch
GOLDEN_X_CHANNELS = [0, 127, 128, 223]            # channels of d loss / d x that are stored
GOLDEN_W_ROWS = [0, 100]                         # output channels of the dW that are stored
GOLDEN_SEED = 20251
GROUPS = 32


def golden_case(fs):
    """-> (x, conv parameters, tail parameters, g_rot, g_trans) in float64 from the seeds, k0, hw of the tail"""
    tag = f'{fs[0]}x{fs[1]}'
    n = len(GOLDEN_LABELS)
    h3 = (out_size(out_size(out_size(fs[0]))), out_size(out_size(out_size(fs[1]))))
    k0 = 128 * h3[0] * h3[1]
    shapes = {'conv_layers.0.conv.weight': (128, 224, 3, 3), 'conv_layers.1.conv.weight': (128, 128, 3, 3),
              'conv_layers.2.conv.weight': (128, 128, 3, 3)}
    p = {name: f64(HF.golden_param(name, shapes.get(name, (128,)), GOLDEN_SEED)) for name in CONV_NAMES}
    tshape = {'W1': (1024, k0), 'b1': (1024,), 'W2': (256, 1024), 'b2': (256,), 'Wr': (18, 256), 'br': (18,), 'Wt': (9, 256),
              'bt': (9,), 'gamma': (128,), 'beta': (128,)}
    tail = {key: f64(HF.golden_param(name, tshape[key], GOLDEN_SEED)) for key, name in HF.TAIL_NAMES.items()}
    x = f64(HF.golden_param('input.' + tag, (n, 224, *fs), GOLDEN_SEED, scale=1.0))
    g_rot = f64(HF.golden_param('g_rot.' + tag, (n, 6), GOLDEN_SEED, scale=1.0))
    g_tr = f64(HF.golden_param('g_trans.' + tag, (n, 3), GOLDEN_SEED, scale=1.0))
    return tag, x, p, tail, g_rot, g_tr, k0, h3[0] * h3[1]


def golden_reference(fs):
    """The float64 backward on the fixture's inputs GIVEN the fp32 forward, and the room around it for an fp32 backward
    by torch -> (tag, reference dict, room dict).

    The forward (raw convolution outputs y0, y1, y2, activations a0, a1 and their masks) is recomputed here in fp32 by the
    operators the reference's ConvModules call (F.conv2d, F.group_norm, relu) and enters as given, the way the kernels'
    saved tensors enter tests/test_gpu_conv_grad.py.  The room is the kernels' composed bound (conv_stack_bounds, after
    test_fc_grad_host.tail_bounds) with EVERY depth raised by torch's longest fp32 chain (9 * 224, the tail's K, 1024), the
    activations' bounds doubled for torch's own group sums, as DESIGN 4.7 does.  A host whose fp32 convolution adds in
    another order than the fixture's differs in that forward by at most twice the forward's rounding bound; this term
    is NOT carried: through three 1152-term sums the worst-case bound of it is vacuous (it exceeds the group variances of
    the last GroupNorm).  The raised depths leave room for it: the test prints where the reference sits."""
    import test_fc_grad_host as hf
    import test_conv_grad_host as me
    from test_fc_host import fc_gn_ref, gemm_ref
    from test_stream_ops_host import group_norm_relu_ref
    F = torch.nn.functional
    tag, x, p, tail, g_rot, g_tr, k0, hw = golden_case(fs)
    n = x.shape[0]
    cls0 = HF.clamp_class(GOLDEN_LABELS, n, n, 3, 0)
    gsz = k0 // GROUPS
    t32 = lambda v: torch.from_numpy(np.asarray(v)).float()            # noqa: E731
    a, ys, acts = t32(x), [], []
    for i in range(3):
        y = F.conv2d(a, t32(p[f'conv_layers.{i}.conv.weight']), stride=2, padding=1)
        ys.append(y)
        if i < 2:
            a = torch.relu(F.group_norm(y, GROUPS, t32(p[f'conv_layers.{i}.gn.weight']), t32(p[f'conv_layers.{i}.gn.bias']),
                                        float(np.float32(IN_EPS))))
            acts.append(a)
    y2 = f64(ys[2]).reshape(n, k0)
    tref = HF.tail_ref64(y2, tail, cls0, g_rot, g_tr, gsz, hw)
    masks = tuple(tref[key] > 0 for key in ('x0', 'a1', 'a2'))
    longest = max(9 * 224, k0, 1024)
    gam_t, bet_t = t32(tail['gamma']), t32(tail['beta'])
    _, x0b = fc_gn_ref(y2, gsz, hw, gam_t, bet_t)
    x0b = 2.0 * x0b
    _, a1b = gemm_ref(tref['x0'], x0b, tail['W1'], tail['b1'], k0 + 1)
    _, a2b = gemm_ref(tref['a1'], a1b[0], tail['W2'], tail['b2'], 1024 + 1)
    abounds = []
    for i in (0, 1):
        c, hh, ww = ys[i].shape[1:]
        _, ab = group_norm_relu_ref(ys[i].reshape(1, n, c, hh * ww), t32(p[f'conv_layers.{i}.gn.weight']),
                                    t32(p[f'conv_layers.{i}.gn.bias']), GROUPS)
        abounds.append(2.0 * ab.reshape(n, c, hh, ww))
    old = hf.EXTRA, me.EXTRA
    hf.EXTRA = me.EXTRA = longest
    try:
        b_gy2 = HF.tail_bounds(tref, tail, y2, cls0, g_rot, g_tr, gsz, hw, masks, (x0b, a1b[0], a2b[0]))['g_y']
        g_y2 = tref['g_y'].reshape(ys[2].shape)
        ref = conv_stack_ref64(x, [f64(ys[0]), f64(ys[1])], p, g_y2, GROUPS, masks=[f64(v) > 0 for v in acts])
        room = conv_stack_bounds(ref, x, p, g_y2, b_gy2.reshape(g_y2.shape), GROUPS, abounds)
    finally:
        hf.EXTRA, me.EXTRA = old
    return tag, ref, room


def golden_pick(key, v):
    """the part of a full gradient the fixture stores"""
    if key == 'g_x':
        return v[:, GOLDEN_X_CHANNELS]
    return v[GOLDEN_W_ROWS] if key.endswith('conv.weight') else v


@pytest.mark.parametrize('fs', GOLDEN_FEAT_SIZES, ids=lambda v: f'{v[0]}x{v[1]}')
def test_reference_head_autograd_agrees_with_the_restatement(fs):
    """The reference's fp32 gradients against the float64 head.  The room is the kernels' composed bound PLUS torch's own
    fp32 terms (golden_reference); it is for the reference's fp32 alone and never granted to the kernels' own checks."""
    z = np.load(GOLDEN)
    tag, ref, room = golden_reference(fs)
    for key in CONV_NAMES + ['g_x']:
        v = worst_ratio(z[f'{tag}.{key}'], golden_pick(key, ref[key]), golden_pick(key, room[key]))
        measured(f'reference head autograd {tag} {key}, error / (kernels\' bound + torch fp32 terms)', v)
        assert v <= 1.0, key
        rel = float(np.abs(z[f'{tag}.{key}'] - golden_pick(key, ref[key])).max() / np.abs(golden_pick(key, ref[key])).max())
        measured(f'reference head autograd {tag} {key}, error relative to the largest entry', rel)
    assert os.path.getsize(GOLDEN) < 100 * 1024
