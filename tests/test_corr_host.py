"""CPU: the correlation pair -- corr_gemm.hip (all-pairs product, scale, pooling cascade) and corr_lookup.hip (windowed
bilinear lookup on every pyramid level) -- restated in float64, with a per-element error bound for any fp32 evaluation in
the kernels' operation order, the inputs tests/test_gpu_corr.py feeds the HIP kernels, a model of the two dispatches (which
route a shape takes), and the proof that the bounds are neither vacuous (planted defects fall outside) nor unreachable (an
fp32 replay of the kernel order and the fp32 oracle stay inside).

Bounds, from U = 2**-24 and magnitude shadows (the same computation on absolute values); gamma(k) = k U / (1 - k U):

* build, level 0: a chain of C multiply-adds (corr_gemm_kernel: v_mfma_f32_32x32x2_f32 over C / 2 steps; the convolution
  fallback: C fused multiply-adds in chunks) in any order is inside gamma(C) S, S = sum |f1| |f2| / sqrt(C).  The scale is
  a multiplication by a power of two when sqrt(C) is one (exact_scale, `v * p.scale`) or a division by 4, 8, 16 in the
  fallback (exact as well); otherwise `v / p.divisor` costs two roundings, fl32(sqrt C) and the division:
  bound_0 = gamma(C + c0) S, c0 = 0 | 2.
* build, level l: `(((a + b) + c) + d) * 0.25f` (corr_gemm_kernel's epilogue, scf_avgpool2x2_layout) on inputs that are
  off by bound_{l-1}: three additions, the product is exact: bound_l = mean(bound_{l-1}) + gamma(3) mean(|v| + bound_{l-1}).
* lookup, sharp: lk_centre takes tx = cx - floor(cx) and wx0 = (floor(cx) + 1) - cx (one rounding each; the integer sum
  is exact), the same for y, and four products (one rounding each); lk_blend is `fma(d, se, fma(c, sw, fma(b, ne, a nw)))`:
  the first term passes four roundings, the last one.  The worst term carries 2 + 1 + 4 = 7 factors (1 + d), |d| <= U:
  |got - ref| <= ((1 + U)**7 - 1) sum |w_i| |v_i|, K_LK = 7.  The centre fl32(x + f) is part of the operation (the
  reference and the kernels both add in fp32); its scaling by 2**-l is exact.
* lookup, loose -- for an evaluator that rounds c + delta and goes through [-1, 1] like the reference: the coordinate it
  samples at is off by e_c, which `coord_error` obtains by replaying the reference's six operations on an `EV`
  (~ U (6 |x| + size)): it grows with the map width.  The interpolant is continuous and piecewise linear, with slope at
  most the largest difference of neighbouring map values (zero padding included) in the cells within one pixel of the tap,
  G_x / G_y -- crossing an integer only changes which cell's slope applies: loose = sharp + 1.01 (e_x G_x + e_y G_y); the
  1 % covers the second-order terms.

fp32 underflow is outside the model (no input here comes near it).
"""
import math

import numpy as np
import pytest
import torch

import oracle
from scflow_amd import ops
from test_stream_ops_host import EV, U, f64, measured, worst_ratio  # noqa: E402

K_LK = 7
F32 = np.float32


def gamma(k):
    return k * U / (1.0 - k * U)


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ============================================================================================================== build
def _pool(v):
    """2x2 mean with floor sizes over the last two axes (float64: the order does not matter)"""
    lh, lw = v.shape[-2] // 2, v.shape[-1] // 2
    v = v[..., :2 * lh, :2 * lw]
    return 0.25 * (v[..., 0::2, 0::2] + v[..., 0::2, 1::2] + v[..., 1::2, 0::2] + v[..., 1::2, 1::2])


def build64(f1, f2, L):
    """-> (levels, shadows): float64 lists of (N h w, lh, lw).  Level 0 = sum_c f1 f2 / sqrt(C), the others 2x2 means with
    floor sizes; the shadows are the same on absolute values."""
    a, b = f64(f1), f64(f2)
    n, c, h, w = a.shape
    a, b = a.reshape(n, c, h * w).transpose(0, 2, 1), b.reshape(n, c, h * w)
    with np.errstate(all='ignore'):
        v = (np.matmul(a, b) / math.sqrt(c)).reshape(n * h * w, h, w)
        s = (np.matmul(np.abs(a), np.abs(b)) / math.sqrt(c)).reshape(n * h * w, h, w)
        lv, sh = [v], [s]
        for _ in range(L - 1):
            lv.append(_pool(lv[-1]))
            sh.append(_pool(sh[-1]))
    return lv, sh


def exact_scale(c):
    """corr_gemm_dispatch: sqrt(C) is a power of two"""
    return math.frexp(float(np.sqrt(F32(c))))[0] == 0.5


def build_bounds(levels, shadows, c):
    """per-element bounds of every level (module docstring)"""
    with np.errstate(all='ignore'):
        b = [gamma(c + (0 if exact_scale(c) else 2)) * shadows[0]]
        for l in range(1, len(levels)):
            b.append(_pool(b[-1]) + gamma(3) * (_pool(np.abs(levels[l - 1])) + _pool(b[-1])))
    return b


FEATURE_REGIMES = ['nominal', 'offset', 'cancelling', 'decades', 'onehot', 'zeros', 'exact']


def features(regime, shape, seed=0):
    """(feat1, feat2), fp32 (N, C, h, w)"""
    n, c, h, w = shape
    g = gen(1000 + seed)
    f1, f2 = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    if regime == 'offset':                      # mean 50, std 1: every product is ~2500, the sum loses 3-4 digits
        f1, f2 = f1 + 50., f2 + 50.
    elif regime == 'cancelling':                # channel pairs (g, g) x (h, -h + 1e-3 noise): |value| << S
        f1 = f1[:, :(c + 1) // 2].repeat_interleave(2, 1)[:, :c].contiguous()
        hh = f2[:, :(c + 1) // 2].repeat_interleave(2, 1)[:, :c]
        sign = torch.tensor([1., -1.]).repeat((c + 1) // 2)[:c].view(1, c, 1, 1)
        f2 = (hh * sign + 1e-3 * torch.randn(shape, generator=g)).contiguous()
    elif regime == 'decades':                   # channel magnitudes 0.1, 1, 10
        sc = 10.0 ** (torch.arange(c) % 3 - 1).float().view(1, c, 1, 1)
        f1, f2 = f1 * sc, f2 * sc
    elif regime == 'onehot':                    # one live channel per pixel
        p = torch.arange(h * w).view(1, 1, h, w)
        ch = torch.arange(c).view(1, c, 1, 1)
        f1 = ((p % c) == ch).float().expand(n, c, h, w).contiguous()
        f2 = (((p * 7 + 3) % c) == ch).float().expand(n, c, h, w).contiguous() * 3.
    elif regime == 'zeros':
        f1 = torch.zeros(shape)
    elif regime == 'exact':                     # integers in [-8, 8]: every product, sum (< 2**24), scale and pool is exact
        f1 = torch.randint(-8, 9, shape, generator=g).float()
        f2 = torch.randint(-8, 9, shape, generator=g).float()
    else:
        assert regime == 'nominal', regime
    return f1, f2


# (N, C, h, w, L, mask) and the launch it takes (corr_gemm_dispatch / scf_corr_build_ex).  GEMM iff C % 16 == 0, h w % 4 == 0,
# 16-byte aligned features and -- level 0 tiled -- w % 8 == 0, h % 4 == 0; the first pool is fused iff level 0 is tiled and
# L >= 2.  nchunk = C / 16: 1, 2, >= 3 chunks walk the three prologues of the staging ring.
BUILD_ROWMAJOR = [(2, 16, 12, 20, 4, 0),        # one chunk; hw = 240: the second 128-block is ragged (queries and targets)
                  (1, 32, 8, 8, 4, 0),          # two chunks, division scale (sqrt 32), one ragged block
                  (1, 48, 4, 8, 3, 0),          # three chunks, division scale, one 32-target fragment
                  (3, 256, 8, 16, 4, 0)]        # exact scale; 3 blocks: a grid that is no multiple of 8 (scf_xcd_remap's tail)
BUILD_TILED = [(1, 16, 4, 8, 1, 0b1),           # <true, false>: no level 1 to pool into
               (2, 64, 12, 24, 4, 0b0001),      # <true, true>, row-major level 1; 9 tiles: ragged in both block dimensions
               (2, 64, 12, 24, 4, 0b0011),      # <true, true>, tiled level 1: 6 x 12 padded to 8 x 16
               (1, 256, 32, 32, 4, None)]       # the layout ops.pyramid_layout picks (0b0001 at 32 x 32)
BUILD_FALLBACK = [(1, 6, 8, 16, 4, 0), (1, 6, 8, 16, 4, 1),       # C % 16 != 0: KC = 2
                  (1, 20, 8, 16, 4, 0), (1, 20, 8, 16, 4, 1),     # KC = 2 again (20 % 8 != 0), more than one chunk
                  (2, 16, 5, 7, 3, 0)]                            # hw % 4 != 0 (exact-regime C)
BUILD_MISALIGNED = (1, 16, 8, 8, 4, 0)          # features one float off 16-byte alignment


def build_route(c, h, w, L, mask, aligned=True):
    """-> ('gemm' | 'conv', level 0 tiled, first pool fused): corr_gemm_dispatch's conditions"""
    t0 = bool(mask & 1)
    gemm = c % 16 == 0 and (h * w) % 4 == 0 and aligned and (not t0 or (w % 8 == 0 and h % 4 == 0))
    fused = t0 and L >= 2
    if fused and (h < 2 or w < 2):
        gemm = False
    return ('gemm' if gemm else 'conv'), t0, bool(gemm and fused)


# ============================================================================================================= lookup
def tile_level(level, fill):
    """row-major (q, 1, lh, lw) -> 8x4-float tiles (q, 1, PH, PW), the padding set to `fill`: the inverse of
    ops.untile_level"""
    q, _, lh, lw = level.shape
    ph, pw = (lh + 3) // 4 * 4, (lw + 7) // 8 * 8
    pad = torch.full((q, 1, ph, pw), float(fill), dtype=level.dtype)
    pad[:, :, :lh, :lw] = level
    return pad.reshape(q, ph // 4, 4, pw // 8, 8).permute(0, 1, 3, 2, 4).reshape(q, 1, ph, pw).contiguous()


def tile_pyramid(pyr, mask, fill=float('nan')):
    return [tile_level(p, fill) if (mask >> l) & 1 else p for l, p in enumerate(pyr)]


def _maps(level):
    a = level.detach().cpu().numpy() if isinstance(level, torch.Tensor) else np.asarray(level)
    return a.reshape(a.shape[0], a.shape[-2], a.shape[-1])


def centres32(flow):
    """fl32(x + fx), fl32(y + fy) per query, as fp32 arrays (N h w,)"""
    fl = flow.detach().cpu().numpy().astype(F32)
    n, _, h, w = fl.shape
    ys, xs = np.meshgrid(np.arange(h, dtype=F32), np.arange(w, dtype=F32), indexing='ij')
    with np.errstate(all='ignore'):
        return (xs[None] + fl[:, 0]).reshape(-1), (ys[None] + fl[:, 1]).reshape(-1)


def _tap(mp, iy, ix, pin=True, edge_bug=False):
    """mp[q, iy, ix] with zero padding; along a size-1 axis every tap is index 0 (`pin`)"""
    q, lh, lw = mp.shape
    if pin and lw == 1:
        ix = np.zeros_like(ix)
    if pin and lh == 1:
        iy = np.zeros_like(iy)
    ok = (ix >= 0) & (ix < lw) & (iy >= 0) & (iy < lh)
    jx, jy = np.clip(ix, 0, lw - 1), np.clip(iy, 0, lh - 1)
    if edge_bug and lw > 1:
        jx = np.where(ix == lw - 1, lw - 2, jx)
    v = mp[np.arange(q).reshape(-1, 1, 1), jy, jx]
    return np.where(ok, v, np.zeros((), dtype=mp.dtype))


def _blend(mp, ix, iy, wx0, tx, wy0, ty, **kw):
    """lk_blend's order in the dtype of the operands: products and sums round one by one (an fma rounds less often)"""
    nw, ne, sw, se = wx0 * wy0, tx * wy0, wx0 * ty, tx * ty
    with np.errstate(all='ignore'):
        out = _tap(mp, iy, ix, **kw) * nw
        out = out + _tap(mp, iy, ix + 1, **kw) * ne
        out = out + _tap(mp, iy + 1, ix, **kw) * sw
        return out + _tap(mp, iy + 1, ix + 1, **kw) * se


def _channels(per_level, n, h, w):
    """[(Q, D, D) indexed (a, b)] per level -> (N, L D D, h, w), channel 81 l + 9 a + b"""
    out = [v.reshape(n, h, w, -1) for v in per_level]
    return np.ascontiguousarray(np.concatenate(out, axis=-1).transpose(0, 3, 1, 2))


def coord_error(c, off, size):
    """|coordinate the reference samples at - (c + off)|: its operations (corr_lookup.py:127, :64-65, grid_sample with
    align_corners) replayed on an EV.  (Q,) x (D,) -> (Q, D)."""
    if size == 1:                                                   # x 0: index 0 exactly
        return np.zeros((c.shape[0], off.shape[0]))
    x = EV(c[:, None]) + off[None, :].astype(np.float64)
    g = x * 2.0 / float(size - 1) - 1.0
    return ((g + 1.0) / 2.0 * float(size - 1)).e


class Look:
    """float64 lookup: `ref`, the shadow sum |w| |v|, and -- with_g -- per tap the slopes gx, gy and the reference's
    coordinate errors ex, ey, all (N, L D D, h, w)"""

    def sharp(self):
        return ((1.0 + U) ** K_LK - 1.0) * self.shadow

    def loose(self):
        return self.sharp() + 1.01 * (self.ex * self.gx + self.ey * self.gy)


def lookup64(pyramid, flow, r, with_g=False):
    """the lookup at the exact coordinate: centre fl32(x + f) scaled by 2**-l (exact), taps at floor(c) - r + i with the
    weights of c's own fraction, zero padding, size-1 axes pinned to index 0; everything after the centre in float64."""
    n, _, h, w = flow.shape
    cx32, cy32 = centres32(flow)
    D = 2 * r + 1
    off = np.arange(D) - r
    acc = {k: [] for k in ('ref', 'shadow', 'gx', 'gy', 'ex', 'ey')}
    for l, level in enumerate(pyramid):
        mp = _maps(level).astype(np.float64)
        _, lh, lw = mp.shape
        far = 2.0 ** 40                                             # beyond any map: all padding either way
        cx = np.clip(cx32.astype(np.float64) * 2.0 ** -l, -far, far) if lw > 1 else np.zeros(cx32.shape)
        cy = np.clip(cy32.astype(np.float64) * 2.0 ** -l, -far, far) if lh > 1 else np.zeros(cy32.shape)
        x0, y0 = np.floor(cx), np.floor(cy)
        tx, ty = (cx - x0).reshape(-1, 1, 1), (cy - y0).reshape(-1, 1, 1)
        ix = x0.astype(np.int64).reshape(-1, 1, 1) + off.reshape(1, D, 1)
        iy = y0.astype(np.int64).reshape(-1, 1, 1) + off.reshape(1, 1, D)
        ix, iy = np.broadcast_arrays(ix, iy)
        acc['ref'].append(_blend(mp, ix, iy, 1.0 - tx, tx, 1.0 - ty, ty))
        acc['shadow'].append(_blend(np.abs(mp), ix, iy, 1.0 - tx, tx, 1.0 - ty, ty))
        if with_g:
            gx, gy = np.zeros(ix.shape), np.zeros(ix.shape)
            for d1 in (-1, 0, 1, 2):                                # the cells within one pixel of the tap's own
                for d2 in (-1, 0, 1):
                    gx = np.maximum(gx, np.abs(_tap(mp, iy + d1, ix + d2 + 1) - _tap(mp, iy + d1, ix + d2)))
                    gy = np.maximum(gy, np.abs(_tap(mp, iy + d2 + 1, ix + d1) - _tap(mp, iy + d2, ix + d1)))
            acc['gx'].append(gx)
            acc['gy'].append(gy)
            acc['ex'].append(np.broadcast_to(coord_error(cx, off, lw)[:, :, None], ix.shape))
            acc['ey'].append(np.broadcast_to(coord_error(cy, off, lh)[:, None, :], ix.shape))
    out = Look()
    for k, v in acc.items():
        if v:
            setattr(out, k, _channels(v, n, h, w))
    return out


LOOKUP_DEFECTS = ['transposed', 'trunc', 'offset_before_scale', 'rounded_sum', 'lw_denorm', 'edge', 'unpinned']


def replay32(pyramid, flow, r, defect=None):
    """lk_centre / lk_blend in numpy fp32, every operation rounded on its own -- or the same with one planted defect:
    transposed (a / b swapped), trunc (truncation for floor), offset_before_scale ((c + delta) 2**-l), rounded_sum
    (weights from fl32(c + delta)), lw_denorm (normalised with lw, de-normalised with lw - 1), edge (the tap in the
    map's last column reads its left neighbour), unpinned (a size-1 axis treated like any other)."""
    n, _, h, w = flow.shape
    cx32, cy32 = centres32(flow)
    D = 2 * r + 1
    off = np.arange(D) - r
    pin = defect != 'unpinned'
    outs = []
    for l, level in enumerate(pyramid):
        mp = _maps(level).astype(F32)
        _, lh, lw = mp.shape
        inv = F32(2.0 ** -l)

        def axis(c32, size, shape):
            """-> first tap index (Q, D | 1 ...), weights wx0, tx in fp32, broadcastable to (Q, D, D)"""
            offs = off.reshape(shape).astype(F32)
            if defect in ('offset_before_scale', 'rounded_sum', 'lw_denorm'):      # per-tap coordinates
                if defect == 'offset_before_scale':
                    x = (c32.reshape(-1, 1, 1) + offs) * inv
                else:
                    x = c32.reshape(-1, 1, 1) * inv + offs
                if defect == 'lw_denorm' and size > 1:
                    x = x * F32(size - 1) / F32(size)
                if pin and size == 1:
                    x = np.zeros_like(x)
                x = np.clip(x, F32(-30000), F32(30000))
                x0 = np.floor(x)
                return x0.astype(np.int64), (x0 + F32(1)) - x, x - x0
            c = c32 * inv
            if pin and size == 1:
                c = np.full_like(c, F32(r))
            c = np.clip(c, F32(-30000), F32(30000)).reshape(-1, 1, 1)
            x0 = np.trunc(c) if defect == 'trunc' else np.floor(c)
            return x0.astype(np.int64) + off.reshape(shape), (x0 + F32(1)) - c, c - x0

        ix, wx0, tx = axis(cx32, lw, (1, D, 1))
        iy, wy0, ty = axis(cy32, lh, (1, 1, D))
        ix, iy = np.broadcast_arrays(ix, iy)
        v = _blend(mp, ix, iy, wx0, tx, wy0, ty, pin=pin, edge_bug=defect == 'edge')
        assert v.dtype == F32
        outs.append(v.transpose(0, 2, 1) if defect == 'transposed' else v)
    return _channels(outs, n, h, w)


VOLUME_REGIMES = ['nominal', 'offset', 'checker', 'decades', 'constant']
CONSTANT = 2.5


def volume(regime, n, h, w, L, seed=0):
    """a row-major pyramid [(N h w, 1, h >> l, w >> l)] of independent fp32 levels (the lookup does not care that they
    are not each other's means)"""
    g = gen(2000 + seed)
    pyr = []
    for l in range(L):
        sh = (n * h * w, 1, h >> l, w >> l)
        v = torch.randn(sh, generator=g)
        if regime == 'offset':
            v = v + 1e3
        elif regime == 'checker':               # +-1e4: a blend at a half-integer centre cancels completely
            yy, xx = torch.meshgrid(torch.arange(sh[2]), torch.arange(sh[3]), indexing='ij')
            v = (1e4 * (1 - 2 * ((yy + xx) % 2)).float()).expand(sh).contiguous()
        elif regime == 'decades':
            v = v * 10.0 ** torch.randint(-1, 2, sh, generator=g).float()
        elif regime == 'constant':
            v = torch.full(sh, CONSTANT)
        else:
            assert regime in ('nominal', 'offset'), regime
        pyr.append(v.contiguous())
    return pyr


def edge_items(r):
    """('f', flow) | ('c', centre at the level under test, relative: ('lo', d) = d, ('hi', d) = size + d)"""
    e = 2.0 ** -10
    return [('f', -0.0), ('f', -1e-10), ('f', 1.0 - 2.0 ** -24),
            ('c', ('lo', -1.)), ('c', ('lo', -r - 1.)), ('c', ('lo', -r - 1. + e)), ('c', ('lo', -r - 1. - e)),
            ('c', ('hi', -1.)), ('c', ('hi', -1. + e)), ('c', ('hi', float(r))),
            ('c', ('lo', 29999.)), ('c', ('lo', -29999.)), ('c', ('lo', 30001.)), ('c', ('lo', -30001.)), ('f', 1e9)]


FLOW_REGIMES = ['randn3', 'integer', 'edges']


def flows(regime, n, h, w, r=4, level=0, seed=0):
    """(N, 2, h, w) fp32.  'integer': every centre is a whole number at `level` (a multiple of 2**level within +-6 level
    pixels of the query), hence at all finer levels too: there the result is a map value or 0, bit for bit.  'edges': randn * 3
    with the edge list written to the first queries, alternately on x (with the width of `level`) and on y (with its
    height); a centre c at that level is the flow c 2**level - x, exact in fp32."""
    g = gen(3000 + seed)
    if regime == 'integer':
        s = 2 ** level
        ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing='ij')
        base = torch.stack([xs, ys])[None]
        d = torch.randint(-6 * s, 6 * s + 1, (n, 2, h, w), generator=g)
        return (torch.div(base + d, s, rounding_mode='floor') * s - base).float()
    fl = torch.randn((n, 2, h, w), generator=g) * 3
    if regime == 'edges':
        items = edge_items(r)
        for k in range(2 * len(items)):
            kind, val = items[k // 2]
            ax = k % 2
            q = k % (n * h * w)
            s, p = divmod(q, h * w)
            y, x = divmod(p, w)
            if kind == 'c':
                size = (w, h)[ax] >> level
                c = val[1] + (size if val[0] == 'hi' else 0)
                val = c * 2.0 ** level - (x, y)[ax]
                assert float(F32(val)) == val
            fl[s, ax, y, x] = val
    else:
        assert regime == 'randn3', regime
    return fl


# (N, h, w, r, L, mask, kinds) on the one-group kernel (lookup_pipe = 1); kinds = what each level is: 's' = row-major with
# lh <= 2r + 2 and lw <= 2r + 2 (staged whole), otherwise 'f' (row-major footprints) | 't' (tiled footprints)
LOOKUP_CASES = [(2, 8, 8, 4, 4, 0, 'ssss'),         # whole maps of exactly 64 floats (one full DMA), 16, 4, 1
                (1, 10, 10, 4, 2, 0, 'ss'),         # 100 floats: the second, masked DMA (msz in 65..100)
                (1, 9, 9, 4, 1, 0, 's'),            # 81 floats, odd row length
                (1, 8, 8, 3, 1, 0, 's'),            # r = 3: FW = 8, a whole map of 64 floats
                (1, 12, 20, 4, 3, 0, 'fss'),        # row-major footprints, 7.5 groups; 6 x 10 and 3 x 5 are staged whole
                (3, 5, 7, 4, 2, 0, 'ss'),           # odd sizes, 35-pixel maps: groups span samples
                (37, 4, 4, 2, 2, 0, 'ss'),          # hw = 16 < 32: the division branch, a group spans three samples
                (1, 3, 12, 4, 1, 0, 'f'),           # footprint level with fewer rows than the window
                (1, 1, 40, 4, 1, 0, 'f'),           # a flat y axis on a footprint level
                (1, 40, 1, 4, 1, 0, 'f'),           # a flat x axis on a footprint level
                (2, 12, 24, 4, 4, 0b0011, 'ttss'),  # tiled 12 x 24 and 6 x 12 (padded to 8 x 16); 3 x 6 and 1 x 3 staged whole
                (1, 16, 32, 4, 5, 0b00001, 'tfsss'),    # L = 5: wave 0 owns levels 0 and 4 (1 x 2)
                (1, 8, 16, 1, 3, 0b001, 'tfs'),     # r = 1
                (1, 8, 16, 2, 3, 0b001, 'tfs')]     # r = 2
LOOKUP_GENERIC = [(1, 8, 12, 5, 3, 0), (1, 8, 24, 6, 2, 0b01)]
LOOKUP_PACKED = (5, 12, 24, 4, 4)               # 1440 queries = 45 groups: >= 2 G for G = 2, 3; ragged under every packing
LOOKUP_OWN_CHOICE = (128, 16, 16, 4, 4, 0)      # 1024 groups = 4 x 256 CUs: the dispatch's own four-groups-per-block choice
LOOKUP_STORE = (2, 16, 16, 4, 4, 0)


def level_kinds(h, w, r, L, mask):
    fw = 2 * r + 2
    out = []
    for l in range(L):
        lh, lw = h >> l, w >> l
        out.append('t' if (mask >> l) & 1 else 's' if (lh <= fw and lw <= fw) else 'f')
    return ''.join(out)


def lookup_route(n, h, w, r, L, mask, pipe, cus):
    """the kernel lookup_launch (corr_lookup.hip) starts: 'generic', 'one' (one group per block), 'pipe2' / 'pipe3' (the
    pipelined kernel) or 'gpb2' / 'gpb3' / 'gpb4' (several groups per block) -- its conditions, restated"""
    fw, qb = 2 * r + 2, 32
    fsp = (fw * fw) | 1
    kinds = level_kinds(h, w, r, L, mask)
    fast = r <= 4
    msz, fl, cost = [], [], []
    for l in range(L):
        lh, lw = h >> l, w >> l
        m = ((lh + 3) // 4 * 4) * ((lw + 7) // 8 * 8) if kinds[l] == 't' else lh * lw
        fast = fast and m <= 32767
        msz.append(m)
        fl.append(qb * (m | 1) + lw if kinds[l] == 's' else qb * fsp + qb * fw)
        cost.append(qb * (2 if m > 64 else 1) if kinds[l] == 's' else qb * ((fw * fw + 63) // 64))
    al = lambda v: (v + 3) & ~3
    lds = 4 * sum(al(max([fl[l] for l in range(wv, L, 4)], default=0)) for wv in range(4))
    if not fast or lds > 64 * 1024 or 2 * L * (2 * r + 1) ** 2 * h * w * 4 > 0xffffffff:
        return 'generic'
    ngroups = -(-n * h * w // qb)
    per_cu = min(max((160 * 1024) // (lds + 512), 1), 4)
    G = pipe if pipe in (2, 3) else 0
    if G and r == 4 and L in (3, 4) and ngroups >= 2 * G:
        units = sorted([(l, gs) for l in range(L) for gs in range(G)], key=lambda u: -cost[u[0]])     # stable
        mine = [[], [], [], []]
        fits = True
        for i, u in enumerate(units):
            c = i & 3
            wv = 3 - c if (i >> 2) & 1 else c
            if len(mine[wv]) >= 3:
                fits = False
                break
            mine[wv].append(u)
        if fits:
            plds = 4 * sum(al(fl[l]) for wave in mine for (l, _) in wave)
            if max(len(m_) for m_ in mine) <= (2 if G == 2 else 3) and (160 * 1024) // (plds + 512) >= 1:
                return f'pipe{G}'
    gpb = {4: 2, 5: 4, 6: 3}.get(pipe, 1)
    if pipe == 0 and per_cu == 4 and ngroups >= 4 * cus:
        gpb = 4
    if gpb > 1 and r == 4 and gpb * lds + 512 <= 160 * 1024 and ngroups >= gpb:
        return f'gpb{gpb}'
    return 'one'


# =============================================================================================================== tests
def test_tile_level_inverts_untile_level():
    for (lh, lw) in ((6, 12), (4, 8), (3, 6), (1, 3), (12, 24), (5, 9)):
        x = torch.randn((7, 1, lh, lw), generator=gen(lh * 100 + lw))
        t = tile_level(x, float('nan'))
        assert tuple(t.shape[-2:]) == ((lh + 3) // 4 * 4, (lw + 7) // 8 * 8)
        assert torch.equal(ops.untile_level(t, lh, lw), x)
        assert int(torch.isnan(t).sum()) == 7 * (t.shape[-2] * t.shape[-1] - lh * lw)
        # the first tile holds rows 0..3 x columns 0..7, row by row
        assert torch.equal(t.reshape(7, -1)[:, :min(lw, 8)], x[:, 0, 0, :min(lw, 8)])


def test_route_models_on_known_shapes():
    assert build_route(16, 12, 20, 4, 0) == ('gemm', False, False)
    assert build_route(64, 12, 24, 4, 0b11) == ('gemm', True, True)
    assert build_route(16, 4, 8, 1, 1) == ('gemm', True, False)
    assert build_route(6, 8, 16, 4, 1)[0] == 'conv' and build_route(16, 5, 7, 3, 0)[0] == 'conv'
    assert build_route(16, 8, 8, 4, 0, aligned=False)[0] == 'conv'
    for case in LOOKUP_CASES:
        assert level_kinds(case[1], case[2], case[3], case[4], case[5]) == case[6], case
        assert lookup_route(*case[:6], 1, 256) == 'one', case
    for case in LOOKUP_GENERIC:
        assert lookup_route(*case, 0, 256) == 'generic', case
    for mask in (0, 0b0011):
        for pipe, want in ((1, 'one'), (2, 'pipe2'), (3, 'pipe3'), (4, 'gpb2'), (5, 'gpb4'), (6, 'gpb3'), (0, 'one')):
            assert lookup_route(*LOOKUP_PACKED, mask, pipe, 256) == want, (mask, pipe)
    assert lookup_route(*LOOKUP_OWN_CHOICE, 0, 256) == 'gpb4'
    assert lookup_route(*LOOKUP_STORE, 0, 256) == 'one'
    assert lookup_route(1, 192, 192, 4, 4, 0, 0, 256) == 'generic'          # 36864 floats per map: no u16 offsets


HOST_BUILD_SHAPES = [(2, 16, 12, 20, 4), (1, 48, 4, 8, 3), (1, 20, 8, 16, 4), (1, 64, 12, 24, 4)]


@pytest.mark.parametrize('regime', FEATURE_REGIMES)
def test_build_fp32_oracle_is_inside_the_bound(regime):
    worst = 0.0
    for (n, c, h, w, L) in HOST_BUILD_SHAPES:
        f1, f2 = features(regime, (n, c, h, w))
        lv, sh = build64(f1, f2, L)
        bd = build_bounds(lv, sh, c)
        got = oracle.correlation_pyramid(f1, f2, L)
        for l in range(L):
            ratio = worst_ratio(_maps(got[l]), lv[l], bd[l])
            measured(f'build oracle {regime} {(n, c, h, w)} level {l}, error / bound', ratio)
            worst = max(worst, ratio)
    assert worst <= 1.0
    if regime == 'zeros':
        assert all(float(np.abs(b).max()) == 0.0 for b in bd)


@pytest.mark.parametrize('c', [16, 64, 256])
def test_build_exact_regime_is_bit_equal_in_fp32(c):
    f1, f2 = features('exact', (1, c, 12, 24))
    lv, _ = build64(f1, f2, 4)
    got = oracle.correlation_pyramid(f1, f2, 4)
    for l in range(4):
        assert np.array_equal(_maps(got[l]).astype(np.float64), lv[l]), f'level {l}'
        assert np.array_equal(lv[l].astype(F32).astype(np.float64), lv[l])


def _build_defect(name, f1, f2, L):
    a, b = f64(f1), f64(f2)
    n, c, h, w = a.shape
    if name == 'last_chunk_dropped':
        lv0 = build64(f1[:, :c - 16], f2[:, :c - 16], 1)[0][0] * math.sqrt(c - 16) / math.sqrt(c)
    elif name == 'k_pair_twice':
        lv0 = build64(f1, f2, 1)[0][0] + build64(f1[:, :2], f2[:, :2], 1)[0][0] * math.sqrt(2) / math.sqrt(c)
    elif name == 'tile_shift':
        lv0 = np.roll(build64(f1, f2, 1)[0][0].reshape(n * h * w, h * w), 1, axis=1).reshape(n * h * w, h, w)
    else:
        lv0 = build64(f1, f2, 1)[0][0]
    lv = [lv0]
    for l in range(1, L):
        lv.append(_pool(lv[-1]))
    if name == 'pool_over_queries':             # level1[n, i, j1] = mean over the QUERY window j1 of corr[n, ., i]
        t = lv0.reshape(n, h, w, h * w)
        t = _pool(np.moveaxis(t, 3, 1)).reshape(n, h * w, (h // 2), (w // 2))
        lv[1] = t.reshape(n * h * w, h // 2, w // 2)
        for l in range(2, L):
            lv[l] = _pool(lv[l - 1])
    return lv


@pytest.mark.parametrize('name,first_level', [('last_chunk_dropped', 0), ('k_pair_twice', 0), ('tile_shift', 0),
                                              ('pool_over_queries', 1)])
def test_build_planted_defects_fall_outside(name, first_level):
    n, c, h, w, L = 2, 64, 12, 24, 4
    f1, f2 = features('nominal', (n, c, h, w))
    lv, sh = build64(f1, f2, L)
    bd = build_bounds(lv, sh, c)
    bad = _build_defect(name, f1, f2, L)
    for l in range(L):
        ratio = worst_ratio(bad[l], lv[l], bd[l])
        measured(f'build defect {name} level {l}, error / bound', ratio)
        if l >= first_level:
            assert ratio > 1.0, f'{name} is inside the bound at level {l}'
        else:
            assert ratio == 0.0


def test_build_equally_valid_orders():
    """0.25 applied per term is the same pool (x 0.25 is exact): it stays inside, in fact bit-identical.  1 / sqrt(C) as a
    rounded reciprocal multiply (three roundings against the division's two) at C = 48: the bound does NOT separate it --
    gamma(C + 2) S leaves room for C roundings of the chain that a real evaluation never uses up; the ratio is printed."""
    n, c, h, w, L = 1, 48, 12, 24, 3
    f1, f2 = features('nominal', (n, c, h, w))
    lv, sh = build64(f1, f2, L)
    bd = build_bounds(lv, sh, c)
    got = oracle.correlation_pyramid(f1, f2, L)
    v = _maps(got[0]).astype(F32)
    q = F32(0.25)
    per_term = ((v[:, 0::2, 0::2] * q + v[:, 0::2, 1::2] * q) + v[:, 1::2, 0::2] * q) + v[:, 1::2, 1::2] * q
    assert per_term.dtype == F32
    ratio = worst_ratio(per_term, lv[1], bd[1])
    measured('build pool with 0.25 per term, error / bound', ratio)
    assert ratio <= 1.0
    a = f1.reshape(n, c, h * w).transpose(1, 2)
    acc = torch.matmul(a, f2.reshape(n, c, h * w)).numpy().astype(F32)
    rcp = F32(1) / np.sqrt(F32(c))
    recip = (acc * rcp).reshape(n * h * w, h, w)
    assert recip.dtype == F32 and not np.array_equal(recip, _maps(got[0]))
    ratio = worst_ratio(recip, lv[0], bd[0])
    measured('build with a rounded reciprocal of sqrt(48), error / bound (not separated)', ratio)
    assert ratio <= 1.0


HOST_LOOKUP_SHAPES = [(1, 12, 20, 4, 3), (2, 8, 8, 4, 4), (1, 24, 32, 4, 4), (3, 4, 8, 2, 2)]


def flow_cases(n, h, w, r, L):
    """(name, level the flow is aimed at | None, flow): every regime, the level-dependent ones once per level"""
    yield 'randn3', None, flows('randn3', n, h, w, r)
    for l in range(L):
        yield f'integer@{l}', l, flows('integer', n, h, w, r, l)
        yield f'edges@{l}', l, flows('edges', n, h, w, r, l)


def integer_exact(name, level, got, ref, r):
    """an 'integer' flow aimed at `level`: the channels of levels 0..level are the float64 values bit for bit"""
    if not name.startswith('integer'):
        return True
    k = (level + 1) * (2 * r + 1) ** 2
    return np.array_equal(f64(got)[:, :k], ref.ref[:, :k])


@pytest.mark.parametrize('regime', VOLUME_REGIMES)
def test_lookup_kernel_order_replay_is_inside_the_sharp_bound(regime):
    worst = 0.0
    for (n, h, w, r, L) in HOST_LOOKUP_SHAPES:
        pyr = volume(regime, n, h, w, L)
        here = 0.0
        for name, lvl, fl in flow_cases(n, h, w, r, L):
            ref = lookup64(pyr, fl, r)
            got = replay32(pyr, fl, r)
            here = max(here, worst_ratio(got, ref.ref, ref.sharp()))
            assert integer_exact(name, lvl, got, ref, r), name      # weights 1 | 0: the map value or 0, bit for bit
        measured(f'lookup replay {regime} {(n, h, w, r, L)}, error / sharp bound', here)
        worst = max(worst, here)
    measured(f'lookup replay {regime}, worst error / sharp bound', worst)
    assert worst <= 1.0


@pytest.mark.parametrize('regime', VOLUME_REGIMES)
def test_lookup_fp32_oracle_is_inside_the_loose_bound(regime):
    worst = 0.0
    for (n, h, w, r, L) in HOST_LOOKUP_SHAPES:
        pyr = volume(regime, n, h, w, L)
        for name, _, fl in flow_cases(n, h, w, r, L):
            ref = lookup64(pyr, fl, r, with_g=True)
            got = oracle.corr_lookup(pyr, fl.clone(), r)
            worst = max(worst, worst_ratio(got, ref.ref, ref.loose()))
    measured(f'lookup oracle {regime}, worst error / loose bound', worst)
    assert worst <= 1.0


def test_sharp_bound_rejects_the_reference_coordinate():
    """the fp32 oracle samples at a coordinate that went through [-1, 1]: it must fall OUTSIDE the sharp bound, or the
    sharp test could not tell the exact coordinate from the reference's"""
    for (n, h, w, r, L) in HOST_LOOKUP_SHAPES:
        pyr = volume('nominal', n, h, w, L)
        fl = flows('randn3', n, h, w, r)
        ref = lookup64(pyr, fl, r)
        ratio = worst_ratio(oracle.corr_lookup(pyr, fl.clone(), r), ref.ref, ref.sharp())
        measured(f'lookup oracle nominal {(n, h, w, r, L)}, error / SHARP bound', ratio)
        assert ratio > 1.0


@pytest.mark.parametrize('defect', LOOKUP_DEFECTS)
def test_lookup_planted_defects_fall_outside(defect):
    n, h, w, r, L = (2, 8, 8, 4, 4) if defect == 'unpinned' else (1, 12, 20, 4, 3)      # 8 x 8, L = 4: a 1 x 1 level
    pyr = volume('nominal', n, h, w, L)
    worst = {}
    for name, _, fl in flow_cases(n, h, w, r, L):
        ref = lookup64(pyr, fl, r)
        worst[name] = worst_ratio(replay32(pyr, fl, r, defect), ref.ref, ref.sharp())
    measured(f'lookup defect {defect}, error / sharp bound on randn * 3 flows', worst['randn3'])
    measured(f'lookup defect {defect}, error / sharp bound on every flow regime', max(worst.values()))
    assert worst['randn3'] > 1.0                # caught without the help of the edge list


def test_zero_shadow_means_exactly_zero():
    """windows entirely in the padding have shadow 0: worst_ratio accepts only an exact 0 there"""
    n, h, w, r, L = 1, 12, 20, 4, 3
    pyr = volume('nominal', n, h, w, L)
    fl = flows('edges', n, h, w, r, 0)
    ref = lookup64(pyr, fl, r)
    zero = ref.shadow == 0
    assert zero.any() and bool((ref.ref[zero] == 0).all())
    got = replay32(pyr, fl, r)
    assert bool((got[zero] == 0).all())
    got[zero] = 1e-30
    assert worst_ratio(got, ref.ref, ref.sharp()) == np.inf
