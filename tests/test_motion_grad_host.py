"""CPU: backward of the motion encoder and of the correlation lookup with respect to the pyramid (corr_lookup_grad.hip,
MotionEncoder.backward, SCFlowDecoder.motion_backward) -- both restated in float64 with a per-element bound for any fp32
evaluation in the kernels' operation order, held against float64 autograd, with planted defects that must fall outside
the bounds, and against the reference's own modules (a fixture).

The lookup adjoint (the header comment of corr_lookup_grad.hip), with x0, y0, nw, ne, sw, se of lk_centre for (query, level,
iteration), i = jx - x0, k = jy - y0 and G[a, b] = mask g_corr of tap (a, b), +0 outside [0, 2r]^2:

    S_l[jy, jx] = sum_t  nw G[i, k] + ne G[i - 1, k] + sw G[i, k - 1] + se G[i - 1, k - 1]
    g_vol[q, jy, jx] = sum_l 4^-l S_l[jy >> l, jx >> l]      over the l with (jy >> l) < (h >> l) and (jx >> l) < (w >> l)

The weights are lk_centre's own fp32 values (restated here operation by operation, `lk_centre32`), so they enter as given.
Roundings on the way of one term w G into g_vol, U = 2^-24: the mask product (1, when there is a mask); the fma chain of
S_l, 4 T steps (times 2r + 1 per size-1 axis of the level: cell 0 takes every offset); the L - 1 steps of the fold (the
factor 4^-l is exact); the addition of the previous value (1, with accumulate).  So

    |fp32 - exact| <= sum_l gamma(d_l) 4^-l sum |w| |G|  [+ gamma(d) |previous|],   d_l = [mask] + 4 T n_a n_b + (L - 1) + [accumulate]

fp32 underflow is outside the model.  The encoder chain composes the convolution bounds of tests/test_head_grad_host.py
stage by stage, as tests/test_gru_grad_host.py does for the GRU.
"""
import os
import re

import numpy as np
import pytest
import torch

from test_stream_ops_host import f64, measured, worst_ratio  # noqa: E402
from test_fc_host import U, gamma  # noqa: E402
import test_corr_host as CH  # noqa: E402
from test_head_grad_host import NONE, RELU, act_grad_ref, dgrad_ref, wgrad_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = torch.nn.functional
F32 = np.float32


# ================================================================================================== the lookup adjoint
def lk_centre32(flow, l, lh, lw, r, defect=None):
    """lk_centre (lk_centre.h) in numpy fp32, every operation rounded on its own, for one iteration's flow (N, 2, h, w) at
    level l -> (x0, y0 int64 (Q,), dict of the fp32 weights nw, ne, sw, se (Q,), bad (Q,))"""
    cx32, cy32 = CH.centres32(flow)
    inv = F32(1.0) if defect == 'centre_not_scaled' else F32(2.0 ** -l)
    lim = F32(30000)
    with np.errstate(all='ignore'):
        cxu, cyu = cx32 * inv, cy32 * inv
        bad = ~(np.abs(cxu * F32(2)) < np.inf) | ~(np.abs(cyu * F32(2)) < np.inf)
        cx = np.full_like(cxu, F32(r)) if lw == 1 else cxu
        cy = np.full_like(cyu, F32(r)) if lh == 1 else cyu
        cx = np.where(bad, -lim, np.clip(cx, -lim, lim)).astype(F32)
        cy = np.where(bad, -lim, np.clip(cy, -lim, lim)).astype(F32)
        x0f, y0f = np.floor(cx), np.floor(cy)
        tx, ty = cx - x0f, cy - y0f
        wx0, wy0 = (x0f + F32(1)) - cx, (y0f + F32(1)) - cy
        wt = dict(nw=wx0 * wy0, ne=tx * wy0, sw=wx0 * ty, se=tx * ty)
    assert all(v.dtype == F32 for v in wt.values())
    return x0f.astype(np.int64) - r, y0f.astype(np.int64) - r, wt, bad


def fma32(a, b, c):
    """fl32(a b + c) (the product of two fp32 is exact in float64; see tests/test_conv_grad_host.py::fma)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


ADJOINT_DEFECTS = ['a_b_swapped', 'ne_sw_swapped', 'half_per_level', 'odd_not_dropped', 'centre_not_scaled',
                   'iteration_missing', 'mask_not_applied']


def lookup_adjoint(g_corr, flows, mask, r, L, mode='64', prev=None, defect=None, rows=None):
    """scf_corr_lookup_grad restated in the gather form.  g_corr (T, N, L D D, h, w), flows (T, N, 2, h, w), mask None or
    (T, N, 1, h, w), prev None or (N h w, h, w): what the call accumulates into.  mode '64': float64 -> (g_vol, bound);
    mode '32': fp32 in the header's order, every fma and product rounded once -> g_vol.  ``rows``: the queries (rows of
    g_vol) to restate, in that order; a query's row depends on that query alone."""
    g = g_corr.detach().cpu().numpy() if isinstance(g_corr, torch.Tensor) else np.asarray(g_corr)
    T, N, K, h, w = g.shape
    D = 2 * r + 1
    assert K == L * D * D
    sel = np.arange(N * h * w) if rows is None else np.asarray(rows, dtype=np.int64)
    assert sel.ndim == 1 and sel.size and 0 <= sel.min() and sel.max() < N * h * w
    full, Q = N * h * w, sel.size
    hi = mode == '64'
    dt = np.float64 if hi else F32
    S = [np.zeros((Q, h >> l, w >> l), dt) for l in range(L)]
    Sh = [np.zeros((Q, h >> l, w >> l)) for l in range(L)]
    qi = np.arange(Q).reshape(-1, 1, 1)
    with np.errstate(all='ignore'):
        for t in range(T):
            if defect == 'iteration_missing' and t == T - 1:
                continue
            G = np.ascontiguousarray(g[t].astype(F32).transpose(0, 2, 3, 1)).reshape(full, L, D, D)[sel]
            if mask is not None and defect != 'mask_not_applied':
                m = (mask[t].detach().cpu().numpy() if isinstance(mask, torch.Tensor) else np.asarray(mask[t])).astype(F32).reshape(full, 1, 1, 1)[sel]
                G = m.astype(np.float64) * G.astype(np.float64) if hi else m * G
            G = G.astype(dt)
            for l in range(L):
                lh, lw = h >> l, w >> l
                x0, y0, wt, bad = lk_centre32(flows[t], l, lh, lw, r, defect)
                x0, y0, bad, wt = x0[sel], y0[sel], bad[sel], {n_: v[sel] for n_, v in wt.items()}
                if defect == 'ne_sw_swapped':
                    wt = dict(wt, ne=wt['sw'], sw=wt['ne'])
                Gl = G[:, l].transpose(0, 2, 1) if defect == 'a_b_swapped' else G[:, l]
                Gp = np.zeros((Q, D + 2, D + 2), dt)
                Gp[:, 1:-1, 1:-1] = np.where(bad.reshape(-1, 1, 1), 0, Gl)         # a bad query contributes nothing
                fetch = lambda ia, kb: Gp[qi, np.clip(ia + 1, 0, D + 1)[:, None, :], np.clip(kb + 1, 0, D + 1)[:, :, None]]   # noqa: E731
                i = np.arange(lw)[None, :] - x0[:, None]                         # (Q, lw)
                k = np.arange(lh)[None, :] - y0[:, None]                         # (Q, lh)
                wv = {n_: np.where(bad, 0, v).astype(dt).reshape(-1, 1, 1) for n_, v in wt.items()}
                for a_ in range(D if lw == 1 else 1):
                    ia, ia1 = (np.full_like(i, a_),) * 2 if lw == 1 else (i, i - 1)
                    for b_ in range(D if lh == 1 else 1):
                        kb, kb1 = (np.full_like(k, b_),) * 2 if lh == 1 else (k, k - 1)
                        for n_, aa, bb in (('nw', ia, kb), ('ne', ia1, kb), ('sw', ia, kb1), ('se', ia1, kb1)):
                            gv = fetch(aa, bb)
                            if hi:
                                S[l] += wv[n_] * gv
                                Sh[l] += np.abs(wv[n_]) * np.abs(gv)
                            else:
                                S[l] = fma32(np.broadcast_to(wv[n_], gv.shape), gv, S[l])
        v, bound = S[0].copy(), None
        n_flat = [(D if (w >> l) == 1 else 1) * (D if (h >> l) == 1 else 1) for l in range(L)]
        d = [(mask is not None) + 4 * T * n_flat[l] + (L - 1) + (prev is not None) for l in range(L)]
        if hi:
            bound = gamma(d[0]) * Sh[0]
        for l in range(1, L):
            lh, lw = h >> l, w >> l
            scale = (0.5 if defect == 'half_per_level' else 0.25) ** l
            jy, jx = np.arange(h) >> l, np.arange(w) >> l
            valid = (jy < lh)[:, None] & (jx < lw)[None, :]
            if defect == 'odd_not_dropped':
                valid = np.ones_like(valid)
            iy, ix = np.minimum(jy, lh - 1)[:, None], np.minimum(jx, lw - 1)[None, :]
            if hi:
                v += np.where(valid, scale * S[l][:, iy, ix], 0.0)
                bound += np.where(valid, gamma(d[l]) * 0.25 ** l * Sh[l][:, iy, ix], 0.0)
            else:
                v = np.where(valid, fma32(np.full(v.shape, F32(scale)), S[l][:, iy, ix], v), v)
        if prev is not None:
            pv = prev.detach().cpu().numpy() if isinstance(prev, torch.Tensor) else np.asarray(prev)
            pv = pv.reshape(full, h, w)[sel]
            v = v + pv.astype(dt)
            if hi:
                bound += gamma(max(d)) * np.abs(pv.astype(np.float64))
    return (v, bound) if hi else v


def lookup_torch64(level0, flows, r, L):
    """the forward in plain float64 torch: avg_pool2d pyramid, grid_sample(bilinear, zeros, align_corners=True) at the
    reference's normalised coordinates (corr_lookup.py:127, :64-67), from the fp32 centre fl32(x + f) -> [corr_t (N, L D D, h, w)]"""
    T, N, _, h, w = flows.shape
    D = 2 * r + 1
    pyr = [level0]
    for _ in range(L - 1):
        pyr.append(F.avg_pool2d(pyr[-1], 2, 2))
    off = torch.arange(D, dtype=torch.float64) - r
    out = []
    for t in range(T):
        cx32, cy32 = CH.centres32(flows[t])
        cx, cy = torch.from_numpy(cx32.astype(np.float64)), torch.from_numpy(cy32.astype(np.float64))
        per = []
        for l, lv in enumerate(pyr):
            lh, lw = lv.shape[-2:]
            gx = 2.0 * (cx[:, None] / 2 ** l + off[None, :]) / max(lw - 1, 1) - 1.0
            gy = 2.0 * (cy[:, None] / 2 ** l + off[None, :]) / max(lh - 1, 1) - 1.0
            grid = torch.stack([gx[:, :, None].expand(-1, D, D), gy[:, None, :].expand(-1, D, D)], -1)      # [q, a, b] = (x(a), y(b))
            per.append(F.grid_sample(lv, grid, mode='bilinear', padding_mode='zeros', align_corners=True).reshape(-1, D * D))
        out.append(torch.cat(per, 1).reshape(N, h, w, L * D * D).permute(0, 3, 1, 2))
    return out


def gen(seed):
    return torch.Generator().manual_seed(seed)


FLOW_KINDS = ['in_range', 'overhang', 'far', 'integer', 'nonfinite']


def adjoint_case(n, T, h, w, r, L, with_mask=True, kinds=FLOW_KINDS, seed=0, dyadic=False):
    """-> (g_corr (T, N, K, h, w), flows (T, N, 2, h, w), mask | None) fp32.  The flows are randn * 3 (inside the map and
    overhanging its edges at 8 x 8 and 12 x 20) with, per iteration, queries written over: one overhanging each edge by
    more than the window, two far outside (every tap is padding: exact zeros), a band of whole-number coordinates, one NaN
    and one inf query.  ``dyadic``: multiples of 1 / 64, where lk_centre's fp32 weights are exact."""
    g = gen(7000 + seed + n + 3 * T + 5 * h + 7 * w)
    K = L * (2 * r + 1) ** 2
    g_corr = torch.randn((T, n, K, h, w), generator=g)
    fl = torch.randn((T, n, 2, h, w), generator=g) * 3
    if dyadic:
        fl = torch.round(fl * 64) / 64
    hw = h * w
    at = lambda t, q: (t, (q // hw) % n, slice(None), (q % hw) // w, q % w)       # noqa: E731
    for t in range(T):
        q = 3 * t
        if 'overhang' in kinds:
            for v in ((-(w + r + 0.5), 0.25), (w + r + 0.5, -0.25), (0.25, -(h + r + 0.5)), (-0.75, h + r + 0.5)):
                fl[at(t, q)] = torch.tensor(v)
                q += 5
        if 'far' in kinds:
            fl[at(t, q)] = torch.tensor((1e9, 2.0))
            fl[at(t, q + 1)] = torch.tensor((-3.0, -40000.0))
            q += 7
        if 'integer' in kinds:
            for j in range(6):
                fl[at(t, q + j)] = torch.tensor((float(j - 3), float(2 - j)))
            q += 11
        if 'nonfinite' in kinds:
            fl[at(t, q)] = torch.tensor((float('nan'), 1.0))
            fl[at(t, q + 2)] = torch.tensor((0.5, float('inf')))
    mask = torch.rand((T, n, 1, h, w), generator=g) if with_mask else None
    return g_corr, fl, mask


def exact_case(n, T, h, w, r, L, with_mask=True, seed=0):
    """operands on which every intermediate of the adjoint is an fp32 number, so that any order of evaluation and float64
    give the same bits: flows at multiples of 1 / 4 (whole numbers among them) reaching past every edge of the map,
    cotangents whole numbers in [-3, 3], masks in {0, 1 / 2, 1}.  A centre at level l is a multiple of 2^-(l + 2), a weight
    a multiple of 2^-(2 l + 4), a masked cotangent of 1 / 2, the fold's 4^-l exact: every term and partial sum of g_vol is a
    multiple of 2^-(4 l + 5), 2^-17 at l = 3.  The four weights of a pass sum to 1, so a pass adds at most 3 in magnitude and
    |g_vol| <= 3 T sum_l 4^-l (passes at l) < 2^5 for T <= 2 even with (2r + 1)^2 = 121 passes at l = 3: 22 bits.
    test_exact_operands_leave_no_rounding does not take this on trust, it compares the fp32 evaluation with float64's bit
    for bit."""
    g = gen(9100 + seed + n + 3 * T + 5 * h + 7 * w + 11 * r)
    K = L * (2 * r + 1) ** 2
    g_corr = torch.randint(-3, 4, (T, n, K, h, w), generator=g).float()
    reach = 4 * (r + 3)
    fl = torch.randint(-reach, reach + 1, (T, n, 2, h, w), generator=g).float() / 4
    mask = torch.randint(0, 3, (T, n, 1, h, w), generator=g).float() / 2 if with_mask else None
    return g_corr, fl, mask


# (N, T, h, w, r, L), the launches of corr_lookup_grad.hip that tests/test_gpu_motion_grad.py runs.  8 x 8: levels 8, 4, 2,
# 1 -- both axes flat at level 3; 12 x 20: 12 x 20, 6 x 10, 3 x 5, 1 x 2 -- a flat y axis, dropped rows and a dropped column; 16
# queries a block there.  32 x 32: a query's accumulators take 5.4 KB, so a block holds 8 queries.  r = 5: the plain route (one
# thread per element), which r <= 4 reaches only with maps whose accumulators exceed 64 KB a query.
KERNEL_SHAPES = [(2, 2, 8, 8, 4, 4), (1, 1, 8, 8, 4, 4), (2, 2, 12, 20, 4, 4), (1, 1, 12, 20, 4, 4), (2, 2, 8, 8, 3, 2),
                 (1, 1, 12, 20, 3, 2), (1, 1, 32, 32, 4, 4), (2, 2, 8, 8, 5, 2), (1, 2, 5, 7, 5, 3)]
# the other launch geometries (what ops.corr_lookup_grad_route must say of each, which test_lookup_route_coverage
# asserts): the radius 1 and 2 instances; 35 and 27 queries, a last block of 3 and of 11 whose other lanes serve no query,
# the second without a fold (L = 1); 8 queries a block because a thread holds at most 24 cotangents (L = 5), not for want of
# LDS; 4, 2 and 1 queries a block (a query's accumulators take 9.9, 18 and 33 KB); the plain route with a flat y axis and
# dropped rows
NEW_KERNEL_SHAPES = {(1, 1, 8, 8, 1, 4): dict(route='fast', radius=1, qb_log2=4, ragged=False),
                     (2, 2, 12, 20, 2, 3): dict(route='fast', radius=2, qb_log2=4, ragged=False),
                     (1, 2, 5, 7, 4, 3): dict(route='fast', radius=4, qb_log2=4, ragged=True),
                     (3, 1, 3, 3, 2, 1): dict(route='fast', radius=2, qb_log2=4, ragged=True),
                     (1, 1, 16, 16, 4, 5): dict(route='fast', radius=4, qb_log2=3, ragged=False),
                     (1, 1, 40, 40, 4, 4): dict(route='fast', radius=4, qb_log2=2, ragged=False),
                     (1, 1, 56, 56, 4, 4): dict(route='fast', radius=4, qb_log2=1, ragged=False),
                     (1, 1, 76, 78, 4, 4): dict(route='fast', radius=4, qb_log2=0, ragged=False),
                     (1, 1, 12, 20, 5, 4): dict(route='plain', radius=0, qb_log2=-1, ragged=False)}
KERNEL_SHAPES += list(NEW_KERNEL_SHAPES)
# one per route, and the fast route with a ragged last block
EXACT_SHAPES = [(2, 2, 12, 20, 4, 4), (1, 2, 5, 7, 4, 3), (1, 2, 5, 7, 5, 3)]


def shape_id(s):
    return 'N{}T{}-{}x{}-r{}L{}'.format(*s)


def kernel_rows(shape):
    """the queries of a kernel shape that are restated: all of them, or on the two largest maps a few hundred -- the first
    and the last 32 (at least a whole first and last block), adjoint_case's special queries (flat index below 3 T + 41) and
    every 23rd"""
    n, T, h, w, _, _ = shape
    q = n * h * w
    if q < 3000:
        return None
    return np.unique(np.concatenate([np.arange(max(32, 3 * T + 41)), np.arange(0, q, 23), np.arange(q - 32, q)]))


def test_lookup_route_coverage():
    """the library's own route decision (ops.corr_lookup_grad_route, a host call) over KERNEL_SHAPES: each added shape
    lands where it was put, and every radius instance, every block size, a ragged and a whole last block and the plain
    route are each reached"""
    from scflow_amd import _lib, ops
    route = lambda s: ops.corr_lookup_grad_route(s[0], s[2], s[3], s[4], s[5])        # noqa: E731
    for shape, want in NEW_KERNEL_SHAPES.items():
        assert shape in KERNEL_SHAPES and route(shape) == want, (shape, route(shape))
    seen = [route(s) for s in KERNEL_SHAPES]
    fast = [r for r in seen if r['route'] == 'fast']
    assert {r['radius'] for r in fast} == {1, 2, 3, 4} and {r['qb_log2'] for r in fast} == {0, 1, 2, 3, 4}
    assert {r['ragged'] for r in fast} == {True, False} and any(r['route'] == 'plain' for r in seen)
    assert any(r['route'] == 'plain' and s[5] == 4 and s[2] >> 3 == 1 for s, r in zip(KERNEL_SHAPES, seen))   # a flat y axis there
    assert any(s[5] == 1 and r['ragged'] for s, r in zip(KERNEL_SHAPES, seen))                               # no fold
    # 8 queries a block by the register cap: 16 of them would fit in LDS
    s = (1, 1, 16, 16, 4, 5)
    cells = sum((s[2] >> l) * (s[3] >> l) for l in range(5)) | 1
    assert (5 * 81 * 16 + cells * 16) * 4 + 5 * 16 * 32 <= 64 * 1024 and -(-5 * 81 * 16 // 256) > 24 >= -(-5 * 81 * 8 // 256)
    assert all(route(e)['route'] == want for e, want in zip(EXACT_SHAPES, ('fast', 'fast', 'plain'))) and route(EXACT_SHAPES[1])['ragged']
    # sizes the kernels do not take are the entry's own error codes
    for bad in ((0, 1, 8, 8, 4, 4), (1, 1, 8, 8, 0, 4), (1, 1, 8, 8, 4, 5), (1, 1, 8, 8, 4, _lib.MAX_LEVELS + 1)):
        with pytest.raises(_lib.ScflowHipError):
            route(bad)


@pytest.mark.parametrize('shape', KERNEL_SHAPES, ids=shape_id)
def test_adjoint_case_plants_two_nonfinite_queries_an_iteration(shape):
    n, T, h, w, r, L = shape
    _, fl, _ = adjoint_case(n, T, h, w, r, L)
    bad = ~torch.isfinite(fl).all(2)
    assert int(bad.sum()) == 2 * T and all(int(bad[t].sum()) == 2 for t in range(T))


@pytest.mark.parametrize('shape', list(NEW_KERNEL_SHAPES), ids=shape_id)
def test_fp32_in_the_stated_order_at_every_kernel_shape(shape):
    n, T, h, w, r, L = shape
    rows = kernel_rows(shape)
    g_corr, fl, mask = adjoint_case(n, T, h, w, r, L)
    ref, bound = lookup_adjoint(g_corr, fl, mask, r, L, rows=rows)
    got = lookup_adjoint(g_corr, fl, mask, r, L, mode='32', rows=rows)
    assert np.isfinite(ref).all() and np.isfinite(got).all() and ref.any()
    assert (rows is None) == (h < 50) and (rows is None or 200 <= len(rows) <= 400)
    v = worst_ratio(got, ref, bound)
    measured(f'lookup adjoint in fp32 {shape}: worst error / bound', v)
    assert v <= 1.0


def test_a_selection_of_rows_is_those_rows():
    n, T, h, w, r, L = 2, 2, 12, 20, 4, 4
    g_corr, fl, mask = adjoint_case(n, T, h, w, r, L)
    prev = torch.randn((n * h * w, h, w), generator=gen(5))
    rows = [479, 0, 38, 240, 17]
    for mode in ('64', '32'):
        whole = lookup_adjoint(g_corr, fl, mask, r, L, mode=mode, prev=prev)
        part = lookup_adjoint(g_corr, fl, mask, r, L, mode=mode, prev=prev, rows=rows)
        for a, b in zip(whole if mode == '64' else (whole,), part if mode == '64' else (part,)):
            assert b.shape == (5, h, w) and np.array_equal(a[rows], b, equal_nan=True)


@pytest.mark.parametrize('with_mask', [False, True], ids=['plain', 'masked'])
@pytest.mark.parametrize('shape', EXACT_SHAPES, ids=shape_id)
def test_exact_operands_leave_no_rounding(shape, with_mask):
    """on exact_case the fp32 evaluation in the header's order and float64 give the same numbers, bit for bit, with a zero
    error bound only where the value is zero: the kernel's result on these operands is then one set of bits, whatever
    order it sums in, and a wrong tap, level or query shows"""
    n, T, h, w, r, L = shape
    g_corr, fl, mask = exact_case(n, T, h, w, r, L, with_mask=with_mask)
    assert (fl * 4 == torch.round(fl * 4)).all() and (fl == torch.round(fl)).any() and (fl != torch.round(fl)).any()
    ref, _ = lookup_adjoint(g_corr, fl, mask, r, L)
    got = lookup_adjoint(g_corr, fl, mask, r, L, mode='32')
    assert got.dtype == F32 and np.array_equal(ref.astype(F32).astype(np.float64), ref)
    assert np.array_equal(ref.astype(F32).view(np.int32), got.view(np.int32))
    # the case is not degenerate: most cells of most rows are non-zero and take many distinct values, on every level
    assert (ref != 0).mean() > 0.2 and len(np.unique(ref)) > 100
    D = 2 * r + 1
    for l in range(L):
        only = g_corr.clone()
        only[:, :, :l * D * D], only[:, :, (l + 1) * D * D:] = 0, 0
        assert lookup_adjoint(only, fl, mask, r, L)[0].any(), l
    # and a defect of the indexing changes bits
    for defect in ('a_b_swapped', 'ne_sw_swapped', 'odd_not_dropped', 'iteration_missing'):
        if defect == 'odd_not_dropped' and all((h >> l) * 2 == (h >> (l - 1)) and (w >> l) * 2 == (w >> (l - 1)) for l in range(1, L)):
            continue
        bad = lookup_adjoint(g_corr, fl, mask, r, L, mode='32', defect=defect)
        assert not np.array_equal(bad, got), defect


def test_symbols_are_declared_exported_and_bound():
    import scflow_amd
    from scflow_amd import _lib, ops
    from scflow_amd.modules import MotionEncoder, SCFlowDecoder
    from scflow_amd.refiner import SCFlowRefiner
    text = open(os.path.join(ROOT, 'include', 'scflow_hip.h')).read()
    assert re.search(r'\bint\s+scf_corr_lookup_grad\s*\(', text)
    assert 'scf_corr_lookup_grad' in _lib.SIGNATURES and hasattr(_lib.load(), 'scf_corr_lookup_grad')
    assert len(_lib.SIGNATURES['scf_corr_lookup_grad'][1]) == 12
    assert re.search(r'\bint\s+scf_corr_lookup_grad_route\s*\(', text) and hasattr(_lib.load(), 'scf_corr_lookup_grad_route')
    assert callable(ops.corr_lookup_grad_route)
    assert callable(ops.corr_lookup_grad) and callable(MotionEncoder.backward) and callable(MotionEncoder.branches)
    assert callable(SCFlowDecoder.motion_backward) and callable(SCFlowRefiner.loss_and_motion_grads)
    dec = scflow_amd.build_refiner(scflow_amd.scflow_model_cfg(iters=2)).decoder
    assert dec.keep == 'none' and dec.detach_mask is True
    # lk_centre has ONE definition, shared by the forward and the adjoint
    csrc = os.path.join(ROOT, 'scflow_amd', 'csrc')
    for name in ('corr_lookup.hip', 'corr_lookup_grad.hip'):
        src = open(os.path.join(csrc, name)).read()
        assert '#include "lk_centre.h"' in src and 'struct LkCentre' not in src, name
    assert 'struct LkCentre' in open(os.path.join(csrc, 'lk_centre.h')).read()
    from scflow_amd.csrc import build
    assert 'corr_lookup_grad.hip' in build.SOURCES


def test_c_abi_rejections_on_the_host():
    """every rejection returns before anything touches a device: NULL pointers, sizes, the level and iteration limits"""
    from scflow_amd import _lib, ops
    lib = _lib.load()
    ok = [8, 8, None, 8, 0, 2, 1, 8, 8, 4, 4, None]       # fake non-null pointers: a rejected call dereferences nothing
    for at, v, code in ((0, None, -1), (1, None, -1), (3, None, -1), (5, 0, -1), (6, 0, -1), (7, 0, -1), (8, -2, -1), (9, 0, -1),
                        (10, 0, -1), (10, _lib.MAX_LEVELS + 1, -2), (5, ops.TAIL_MAX_T + 1, -2), (10, 5, -1)):     # 8 >> 4 = 0: an empty level
        bad = list(ok)
        bad[at] = v
        assert lib.scf_corr_lookup_grad(*bad) == code, (at, v)
    with pytest.raises(_lib.ScflowHipError):
        ops.corr_lookup_grad(torch.zeros(1, 1, 324, 8, 8), torch.zeros(1, 1, 2, 8, 8))       # CPU tensors


@pytest.mark.parametrize('shape', [(2, 2, 12, 20, 4, 4), (1, 2, 8, 8, 3, 2), (1, 1, 5, 7, 2, 3)], ids=str)
def test_gather_form_equals_float64_autograd(shape):
    """where lk_centre's fp32 weights are exact (flows on a 1 / 64 grid) the gather form IS the adjoint of grid_sample on
    the avg_pool2d pyramid"""
    n, T, h, w, r, L = shape
    g_corr, fl, mask = adjoint_case(n, T, h, w, r, L, kinds=['overhang', 'far', 'integer'], dyadic=True)
    v0 = torch.randn((n * h * w, 1, h, w), generator=gen(1), dtype=torch.float64).requires_grad_()
    corr = lookup_torch64(v0, fl, r, L)
    sum((c * (mask[t].double() * g_corr[t].double())).sum() for t, c in enumerate(corr)).backward()
    got, _ = lookup_adjoint(g_corr, fl, mask, r, L)
    want = f64(v0.grad).reshape(got.shape)
    rel = float(np.abs(got - want).max() / np.abs(want).max())
    measured(f'gather form against float64 autograd {shape}, relative to the largest entry', rel)
    assert rel <= 1e-13


CPU_CASE = (2, 2, 12, 20, 4, 4)          # levels 12 x 20, 6 x 10, 3 x 5, 1 x 2: a size-1 y axis, a dropped column and dropped rows


@pytest.mark.parametrize('with_mask, with_prev', [(True, False), (False, True)])
def test_fp32_in_the_stated_order_is_inside_the_bound(with_mask, with_prev):
    n, T, h, w, r, L = CPU_CASE
    g_corr, fl, mask = adjoint_case(n, T, h, w, r, L, with_mask=with_mask)
    prev = torch.randn((n * h * w, h, w), generator=gen(3)) if with_prev else None
    ref, bound = lookup_adjoint(g_corr, fl, mask, r, L, prev=prev)
    got = lookup_adjoint(g_corr, fl, mask, r, L, mode='32', prev=prev)
    assert got.dtype == F32 and np.isfinite(ref).all() and np.isfinite(got).all()
    v = worst_ratio(got, ref, bound)
    measured(f'lookup adjoint in fp32, mask {with_mask} accumulate {with_prev}: worst error / bound', v)
    assert 0.0 < v <= 1.0
    # the non-finite queries contribute nothing at their iteration; far-outside ones exact zeros -- on the levels without
    # a size-1 axis (the forward pins every tap of such an axis to index 0 wherever the centre is: level 3 here)
    D = 2 * r + 1
    m1 = None if mask is None else mask[:1]
    one = lookup_adjoint(g_corr[:1], fl[:1], m1, r, L)[0]
    three = lookup_adjoint(g_corr[:1, :, :3 * D * D], fl[:1], m1, r, 3)[0]
    q = 0 + 4 * 5 + 7 + 11            # adjoint_case: iteration 0's NaN query, the inf one two behind it
    assert not one[q].any() and not one[q + 2].any() and one[q + 1].any()
    assert not one[20].any() and one[21].any() and not three[20].any() and not three[21].any()


@pytest.mark.parametrize('defect', ADJOINT_DEFECTS)
def test_planted_adjoint_defects_fall_outside(defect):
    n, T, h, w, r, L = CPU_CASE
    g_corr, fl, mask = adjoint_case(n, T, h, w, r, L)
    ref, bound = lookup_adjoint(g_corr, fl, mask, r, L)
    bad = lookup_adjoint(g_corr, fl, mask, r, L, mode='32', defect=defect)
    v = worst_ratio(bad, ref, bound)
    measured(f'lookup adjoint defect {defect}: worst error / bound', v)
    assert v > 1.0


# ==================================================================================================== the encoder chain
ENC_LAYERS = ('corr_net.0', 'corr_net.1', 'flow_net.0', 'flow_net.1', 'out_net.0')
ENC_NAMES = [f'{m}.conv.{k}' for m in ENC_LAYERS for k in ('weight', 'bias')]
ENC_KERNELS = {'corr_net.0': (1, 1), 'corr_net.1': (3, 3), 'flow_net.0': (7, 7), 'flow_net.1': (3, 3), 'out_net.0': (3, 3)}
REAL_WIDTHS = dict(k=324, c1=256, cc=192, f1=128, cf=64, co=126)
SMALL_WIDTHS = dict(k=7, c1=6, cc=4, f1=5, cf=3, co=5)


def enc_shapes(wd):
    io = {'corr_net.0': (wd['c1'], wd['k']), 'corr_net.1': (wd['cc'], wd['c1']), 'flow_net.0': (wd['f1'], 2),
          'flow_net.1': (wd['cf'], wd['f1']), 'out_net.0': (wd['co'], wd['cc'] + wd['cf'])}
    return {m: io[m] + ENC_KERNELS[m] for m in ENC_LAYERS}


def enc_params(wd, seed=0):
    g = gen(6600 + seed)
    p = {}
    for m, s in enc_shapes(wd).items():
        p[f'{m}.conv.weight'] = f64(torch.randn(s, generator=g) * (s[1] * s[2] * s[3]) ** -0.5)
        p[f'{m}.conv.bias'] = f64(torch.randn(s[0], generator=g) * 0.1)
    return p


def enc_forward_torch(corr, flow, p, act):
    """the plain-torch encoder (raft_decoder.py:152-166) -> dict(c1, f1, cf, x), differentiable"""
    a_ = (lambda v: torch.relu(v)) if act == RELU else (lambda v: v)
    conv = lambda x, m: a_(F.conv2d(x, p[f'{m}.conv.weight'], p[f'{m}.conv.bias'], padding=(p[f'{m}.conv.weight'].shape[2] // 2,) * 2))  # noqa: E731
    c1, f1 = conv(corr, 'corr_net.0'), conv(flow, 'flow_net.0')
    cf = torch.cat([conv(c1, 'corr_net.1'), conv(f1, 'flow_net.1')], 1)
    return dict(c1=c1, f1=f1, cf=cf, x=torch.cat([conv(cf, 'out_net.0'), flow], 1))


ENC_DEFECTS = ['relu_mask_of_cf_dropped', 'passthrough_not_added', 'cf_split_at_wrong_column', 'bias_twice']


def encoder_ref64(saved, p, g_x, act, prev=None, defect=None, bounds=False, xbounds=None):
    """MotionEncoder.backward in float64 GIVEN the activations ``saved`` (corr, x, c1, f1, cf over the stacked samples) ->
    dict of g_corr, g_flow_in and the ten parameter gradients; with ``bounds`` a second dict, the composed per-element
    bounds (each stage's bound carried into the next; ``xbounds``: bounds of the activations as wgrad operands, by key)"""
    s = {k: f64(v) for k, v in saved.items()}
    p = {k: f64(v) for k, v in p.items()}
    g_x = f64(g_x)
    co, cc = p['out_net.0.conv.weight'].shape[0], p['corr_net.1.conv.weight'].shape[0]
    ref, bnd = {}, {}
    xb_of = lambda k, sl=slice(None): 0.0 if xbounds is None or k not in xbounds else f64(xbounds[k])[:, sl]      # noqa: E731
    a_ = lambda v: v if act != NONE else None                                                                    # noqa: E731

    def wgrad(name, g, gb, x, xb=0.0):
        kh, kw = p[f'{name}.conv.weight'].shape[2:]
        pv = None if prev is None else prev[f'{name}.conv.weight']
        pb = None if prev is None else prev[f'{name}.conv.bias']
        kw_, kb_ = f'{name}.conv.weight', f'{name}.conv.bias'
        ref[kw_], bnd[kw_], ref[kb_], bnd[kb_] = wgrad_ref(g, gb, x, kh, kw, xb=xb, prev=pv, prev_b=pb)

    u, ub = act_grad_ref(g_x[:, :co], 0.0, s['x'][:, :co], act)
    wgrad('out_net.0', u, ub, s['cf'], xb_of('cf'))
    if defect == 'relu_mask_of_cf_dropped':
        g_cf, b_cf = dgrad_ref(u, ub, p['out_net.0.conv.weight'])
    else:
        g_cf, b_cf = dgrad_ref(u, ub, p['out_net.0.conv.weight'], a=a_(s['cf']), act=act)
    wgrad('corr_net.1', g_cf[:, :cc], b_cf[:, :cc], s['c1'], xb_of('c1'))
    g_c1, b_c1 = dgrad_ref(g_cf[:, :cc], b_cf[:, :cc], p['corr_net.1.conv.weight'], a=a_(s['c1']), act=act)
    wgrad('corr_net.0', g_c1, b_c1, s['corr'], xb_of('corr'))
    ref['g_corr'], bnd['g_corr'] = dgrad_ref(g_c1, b_c1, p['corr_net.0.conv.weight'])
    fl = slice(0, g_cf.shape[1] - cc) if defect == 'cf_split_at_wrong_column' else slice(cc, None)
    wgrad('flow_net.1', g_cf[:, fl], b_cf[:, fl], s['f1'], xb_of('f1'))
    g_f1, b_f1 = dgrad_ref(g_cf[:, fl], b_cf[:, fl], p['flow_net.1.conv.weight'], a=a_(s['f1']), act=act)
    wgrad('flow_net.0', g_f1, b_f1, s['x'][:, co:])
    ref['g_flow_in'], bnd['g_flow_in'] = dgrad_ref(g_f1, b_f1, p['flow_net.0.conv.weight'],
                                                  add=None if defect == 'passthrough_not_added' else g_x[:, co:])
    if defect == 'bias_twice':
        ref['flow_net.1.conv.bias'] = 2.0 * ref['flow_net.1.conv.bias']
    return (ref, bnd) if bounds else ref


def enc_case(wd, m, h, w, seed=0):
    g = gen(8800 + seed + m + 3 * h + 5 * w)
    R = lambda *s: torch.randn(s, generator=g, dtype=torch.float64)       # noqa: E731
    return enc_params(wd, seed), R(m, wd['k'], h, w), R(m, 2, h, w) * 3, R(m, wd['co'] + 2, h, w)


@pytest.mark.parametrize('act', [RELU, NONE], ids=['relu', 'none'])
@pytest.mark.parametrize('hw', [(5, 7), (2, 3)], ids=lambda v: f'{v[0]}x{v[1]}')
def test_encoder_chain_equals_float64_autograd(hw, act):
    p, corr, flow, g_x = enc_case(SMALL_WIDTHS, 3, *hw)
    pt = {k: torch.from_numpy(v).requires_grad_() for k, v in p.items()}
    ct, ft = corr.clone().requires_grad_(), flow.clone().requires_grad_()
    fw = enc_forward_torch(ct, ft, pt, act)
    (fw['x'] * g_x).sum().backward()
    want = {k: v.grad for k, v in pt.items()}
    want.update(g_corr=ct.grad, g_flow_in=ft.grad)
    saved = {k: v.detach() for k, v in fw.items()}
    saved['corr'] = corr
    ref = encoder_ref64(saved, p, g_x, act)
    assert set(ref) == set(want) == set(ENC_NAMES) | {'g_corr', 'g_flow_in'}
    worst = max(float(np.abs(ref[k] - f64(want[k])).max() / np.abs(f64(want[k])).max()) for k in want)
    measured(f'encoder chain against float64 autograd {hw}, relative', worst)
    assert worst <= 1e-12


@pytest.mark.parametrize('defect', ENC_DEFECTS)
def test_planted_encoder_defects_fall_outside(defect):
    wd = dict(k=7, c1=6, cc=3, f1=5, cf=3, co=5)               # cc == cf: a split at the wrong column has the right shape
    p, corr, flow, g_x = enc_case(wd, 3, 5, 7)
    saved = {k: v.detach() for k, v in enc_forward_torch(corr, flow, {k: torch.from_numpy(v) for k, v in p.items()}, RELU).items()}
    saved['corr'] = corr
    ref, bnd = encoder_ref64(saved, p, g_x, RELU, bounds=True)
    bad = encoder_ref64(saved, p, g_x, RELU, defect=defect)
    worst = max(worst_ratio(bad[k], ref[k], bnd[k]) for k in ref)
    measured(f'encoder defect {defect} / composed bound', worst)
    assert worst > 1.0


# =================================================== the reference's own pyramid, lookup and motion encoder (a fixture)
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'motion_grads.npz')
GOLDEN_SHAPE = dict(n=1, T=2, h=12, w=20, r=4, L=4, c=32)
GOLDEN_SEED = 20253
GOLDEN_ROWS = list(range(0, 240, 7))             # queries (rows of g_vol) that are stored
GOLDEN_CORR_CHANNELS = [0, 40, 161, 242, 323]    # channels of d loss / d corr_t that are stored
GOLDEN_KEYS = ENC_NAMES + ['g_vol'] + [f'{k}.{t}' for t in range(GOLDEN_SHAPE['T']) for k in ('g_corr', 'g_flow_in')]
# float64 restatement - the reference's fp32 CPU autograd, relative to the largest entry of a key: measured 1.4e-6 at
# most (g_vol); asserted at a few times that
GOLDEN_MARGIN = 5e-6


def golden_case():
    """-> (the 10 parameters, feat1, feat2 (N, C, h, w), flows (T, N, 2, h, w), the cotangents c_t at x_t (T, N, 128, h, w))
    as float32 tensors, from the seeds"""
    from test_fc_grad_host import golden_param
    s = GOLDEN_SHAPE
    p = {}
    for m, sh in enc_shapes(REAL_WIDTHS).items():
        p[f'{m}.conv.weight'] = golden_param(f'{m}.conv.weight', sh, GOLDEN_SEED)
        p[f'{m}.conv.bias'] = golden_param(f'{m}.conv.bias', sh[:1], GOLDEN_SEED)
    x = lambda name, *shape, scale=1.0: golden_param(f'motion.{name}', shape, GOLDEN_SEED, scale=scale)      # noqa: E731
    feats = x('feat1', s['n'], s['c'], s['h'], s['w']), x('feat2', s['n'], s['c'], s['h'], s['w'])
    return p, feats[0], feats[1], x('flow', s['T'], s['n'], 2, s['h'], s['w'], scale=3.0), x('cot', s['T'], s['n'], 128, s['h'], s['w'])


def golden_pick(key, v):
    """the part of a full gradient the fixture stores"""
    if key == 'g_vol':
        return v[GOLDEN_ROWS]
    if key.startswith('g_corr'):
        return v[:, GOLDEN_CORR_CHANNELS]
    if v.ndim == 4 and v.size > 2048 and key.endswith('weight'):
        v = v[[0, v.shape[0] - 1]]
        if v.size > 2048:
            v = v[:, ::4]
    return v


def golden_reference():
    """the float64 backward on the fixture's inputs: the pyramid and the lookup of tests/test_corr_host.py (float64 from
    the fp32 centres), the encoder forward in float64 torch, then encoder_ref64 and lookup_adjoint -> dict by GOLDEN_KEYS"""
    s = GOLDEN_SHAPE
    p, f1, f2, flows, cots = golden_case()
    pyr, _ = CH.build64(f1, f2, s['L'])
    corr = torch.stack([torch.from_numpy(CH.lookup64(pyr, flows[t], s['r']).ref) for t in range(s['T'])])
    m = s['T'] * s['n']
    corr_, flow_ = corr.reshape(m, -1, s['h'], s['w']), flows.double().reshape(m, 2, s['h'], s['w'])
    with torch.no_grad():
        fw = enc_forward_torch(corr_, flow_, {k: v.double() for k, v in p.items()}, RELU)
    saved = dict(fw, corr=corr_)
    ref = encoder_ref64(saved, p, cots.reshape(m, 128, s['h'], s['w']), RELU)
    g_corr = ref['g_corr'].reshape(s['T'], s['n'], -1, s['h'], s['w'])
    out = {k: ref[k] for k in ENC_NAMES}
    out['g_vol'] = lookup_adjoint(g_corr, flows, None, s['r'], s['L'])[0]
    g_fl = ref['g_flow_in'].reshape(s['T'], s['n'], 2, s['h'], s['w'])
    for t in range(s['T']):
        out[f'g_corr.{t}'], out[f'g_flow_in.{t}'] = g_corr[t], g_fl[t]
    return out


def test_reference_autograd_agrees_with_the_restatement():
    """The reference's fp32 CPU autograd through its own CorrelationPyramid, CorrLookup and MotionEncoder (retain_grad on
    the pyramid's level 0 gives the folded volume cotangent) against the float64 restatement on the same seeds."""
    z = np.load(GOLDEN)
    ref = golden_reference()
    assert sorted(k for k in z.files if k != 'pinned_under') == sorted(GOLDEN_KEYS)
    for key in GOLDEN_KEYS:
        want = golden_pick(key, ref[key])
        assert z[key].shape == want.shape, key
        rel = float(np.abs(z[key] - want).max() / np.abs(want).max())
        measured(f'reference motion-stage autograd {key}, difference relative to the largest entry', rel)
        assert rel <= GOLDEN_MARGIN, key
    assert os.path.getsize(GOLDEN) < 200 * 1024
