"""GPU: the correlation pair -- ops.corr_build (corr_gemm.hip: MFMA GEMM with the fused first pool, the convolution
fallback, the pooling cascade) and ops.corr_lookup (corr_lookup.hip: whole-map and footprint routes, both layouts, every
packing, the generic kernel) -- against the float64 restatements and derived bounds of tests/test_corr_host.py, on every
launch route, at the smallest shapes that reach it.  The shape lists, the comments on which branch each shape takes and the
model of the two dispatches (build_route, lookup_route, level_kinds) live next to the restatements; every test asserts
from that model (and, for the fallback, from the convolution log) that its shape takes the route it names.

Every comparison is `error <= bound` (ratio <= 1) over ALL elements, or bit equality.  Lookup-only tests build the pyramid
on the host and tile it there with NaN in the padding: only the lookup is under test, and a read of the padding shows.

The measured error-to-bound ratios are recorded in DESIGN.md section 4.2.
"""
import contextlib
import functools

import numpy as np
import pytest
import torch

import oracle
from scflow_amd import ops
from test_corr_host import (BUILD_FALLBACK, BUILD_MISALIGNED, BUILD_ROWMAJOR, BUILD_TILED, CONSTANT, FEATURE_REGIMES,  # noqa: E402
                            LOOKUP_CASES, LOOKUP_GENERIC, LOOKUP_OWN_CHOICE, LOOKUP_PACKED, LOOKUP_STORE, VOLUME_REGIMES,
                            build64, build_bounds, build_route, features, flow_cases, flows, integer_exact, level_kinds,
                            lookup64, lookup_route, tile_pyramid, volume)
from test_stream_ops_host import f64, measured, worst_ratio  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAN = float('nan')


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@contextlib.contextmanager
def knob(key, value):
    prev = ops.tune(key, value)
    try:
        yield
    finally:
        ops.tune(key, prev)


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ============================================================================================================== build
def gpu_build(f1d, f2d, L, mask, route):
    """ops.corr_build into NaN-filled buffers -> row-major CPU levels (padding dropped).  `route` = 'gemm' | 'conv': the
    fallback is a launch of scf_conv2d and shows in the convolution log, the GEMM does not."""
    n, _, h, w = f1d.shape
    out = [torch.full((n * h * w, 1, *ops.level_storage_shape(h, w, l, bool((mask >> l) & 1))), NAN, device=DEV)
           for l in range(L)]
    with ops.record_conv_kernels() as ran:
        got = ops.corr_build(f1d, f2d, L, out=out, tiled_levels=mask)
    assert (len(ran) >= 1) == (route == 'conv'), f'expected the {route} route, the convolution log holds {ran}'
    return [(ops.untile_level(g, h >> l, w >> l) if (mask >> l) & 1 else g).cpu() for l, g in enumerate(got)]


def check_build(case, got, f1, f2, regime, what):
    n, c, h, w, L, mask = case
    lv, sh = build64(f1, f2, L)
    bd = build_bounds(lv, sh, c)
    worst = 0.0
    for l in range(L):
        g = got[l].reshape(lv[l].shape)
        assert bool(torch.isfinite(g).all()), f'{what} {regime} level {l}: an in-map element was not written'
        worst = max(worst, worst_ratio(g, lv[l], bd[l]))
        if regime == 'exact' and c in (16, 64, 256):
            assert np.array_equal(f64(g), lv[l]), f'{what} {regime} level {l}: not bit-equal to float64'
    measured(f'corr_build {what} {case} {regime}, error / bound', worst)
    assert worst <= 1.0
    return worst


def _build_case(case, what, place=lambda t: t.to(DEV), aligned=True):
    n, c, h, w, L, mask = case
    if mask is None:
        mask = ops.pyramid_layout(h, w, 4, L)
        assert mask & 1, 'the preferred layout tiles level 0 at this shape'
        case = (n, c, h, w, L, mask)
    route, t0, fused = build_route(c, h, w, L, mask, aligned)
    for regime in FEATURE_REGIMES:
        f1, f2 = features(regime, (n, c, h, w))
        f1d, f2d = place(f1), place(f2)
        got = gpu_build(f1d, f2d, L, mask, route)
        check_build(case, got, f1, f2, regime, what)
        if mask:                                                    # the same numbers as the row-major build, bit for bit
            plain = gpu_build(f1d, f2d, L, 0, build_route(c, h, w, L, 0, aligned)[0])
            for l in range(L):
                assert same_bits(got[l], plain[l]), f'{what} {regime}: level {l} differs from the row-major build'
    return route, t0, fused


@pytest.mark.parametrize('case', BUILD_ROWMAJOR, ids=str)
def test_build_rowmajor_gemm(case):
    assert _build_case(case, 'GEMM<false,false>') == ('gemm', False, False)


@pytest.mark.parametrize('case', BUILD_TILED, ids=str)
def test_build_tiled_gemm(case):
    route, t0, fused = _build_case(case, 'GEMM<true,*>')
    assert (route, t0) == ('gemm', True) and fused == (case[4] >= 2)


@pytest.mark.parametrize('case', BUILD_FALLBACK, ids=str)
def test_build_convolution_fallback(case):
    route, t0, _ = _build_case(case, 'conv fallback')
    assert route == 'conv' and t0 == bool(case[5] & 1)


@pytest.mark.parametrize('which', ['feat1', 'feat2', 'both'])
def test_build_misaligned_features_take_the_fallback(which):
    def place_for(name):
        def place(t):
            mis = which in (name, 'both')
            base = torch.zeros((t.numel() + 8,), device=DEV)
            o = 1 if mis else 4
            base[o:o + t.numel()] = t.flatten().to(DEV)
            v = base[o:o + t.numel()].view(t.shape)
            assert (v.data_ptr() % 16 != 0) == mis
            return v
        return place
    n, c, h, w, L, mask = BUILD_MISALIGNED
    assert build_route(c, h, w, L, mask, aligned=False)[0] == 'conv'
    for regime in FEATURE_REGIMES:
        f1, f2 = features(regime, (n, c, h, w))
        got = gpu_build(place_for('feat1')(f1), place_for('feat2')(f2), L, mask, 'conv')
        check_build(BUILD_MISALIGNED, got, f1, f2, regime, f'misaligned {which}')


@pytest.mark.parametrize('case', [BUILD_ROWMAJOR[0], BUILD_TILED[2], BUILD_FALLBACK[1]], ids=str)
def test_build_poison_stays_in_its_row_and_window(case):
    """a NaN at feat1[n, c, i] makes exactly query i of sample n NaN, at all targets and levels; one at feat2[n, c, j]
    exactly the targets whose pooling window holds j: the float64 pattern, and no other element moves a bit."""
    n, c, h, w, L, mask = case
    route = build_route(c, h, w, L, mask)[0]
    f1, f2 = features('nominal', (n, c, h, w))
    clean = gpu_build(f1.to(DEV), f2.to(DEV), L, mask, route)
    for name, pos in (('feat1', (n - 1, c - 1, h // 2, w // 3)), ('feat2', (0, 1, h - 1, w - 1)),
                      ('feat2', (n - 1, 0, 2, 5))):
        p1, p2 = f1.clone(), f2.clone()
        (p1 if name == 'feat1' else p2)[pos] = NAN
        got = gpu_build(p1.to(DEV), p2.to(DEV), L, mask, route)
        want, _ = build64(p1, p2, L)
        for l in range(L):
            g, bad = got[l].reshape(want[l].shape), torch.from_numpy(np.isnan(want[l]))
            assert torch.equal(torch.isnan(g), bad), f'{name}{pos} level {l}: NaN pattern differs from float64'
            keep = clean[l].reshape(want[l].shape)
            assert same_bits(torch.where(bad, torch.zeros(()), g), torch.where(bad, torch.zeros(()), keep)), \
                f'{name}{pos} level {l}: an element outside the pattern changed'
        if name == 'feat1':
            q = pos[0] * h * w + pos[2] * w + pos[3]
            assert int(torch.isnan(got[0].reshape(n * h * w, -1)).any(1).sum()) == 1
            assert bool(torch.isnan(got[0][q]).all())


# ============================================================================================================= lookup
def gpu_lookup(pyr, fl, r, mask):
    dev = [p.to(DEV) for p in tile_pyramid(pyr, mask, NAN)]
    return ops.corr_lookup(dev, fl.to(DEV), r, tiled_levels=mask).cpu()


@functools.lru_cache(maxsize=None)
def reference(regime, n, h, w, r, L):
    """[(flow name, level aimed at, flow, float64 lookup)] of one volume regime at one shape: computed once, shared by the
    tests that run the same inputs through several kernels"""
    pyr = volume(regime, n, h, w, L)
    return pyr, [(name, lvl, fl, lookup64(pyr, fl, r)) for name, lvl, fl in flow_cases(n, h, w, r, L)]


def check_lookup(n, h, w, r, L, mask, what, regimes=VOLUME_REGIMES):
    worst = 0.0
    for regime in regimes:
        pyr, cases = reference(regime, n, h, w, r, L)
        here = 0.0
        for name, lvl, fl, ref in cases:
            got = gpu_lookup(pyr, fl, r, mask)
            ratio = worst_ratio(got, ref.ref, ref.sharp())
            assert ratio <= 1.0, f'{what} {regime} {name}: error / sharp bound = {ratio:.3g}'
            assert integer_exact(name, lvl, got, ref, r), f'{what} {regime} {name}: not the map value bit for bit'
            here = max(here, ratio)
        measured(f'corr_lookup {what} {(n, h, w, r, L, mask)} {regime}, error / sharp bound', here)
        worst = max(worst, here)
    return worst


@pytest.mark.parametrize('case', LOOKUP_CASES, ids=str)
def test_lookup_one_group_per_block(case):
    n, h, w, r, L, mask, kinds = case
    assert level_kinds(h, w, r, L, mask) == kinds
    assert lookup_route(n, h, w, r, L, mask, 1, cus()) == 'one'
    with knob('lookup_pipe', 1):
        check_lookup(n, h, w, r, L, mask, 'one group per block')


@pytest.mark.parametrize('mask', [0, 0b0011])
@pytest.mark.parametrize('pipe,route', [(2, 'pipe2'), (3, 'pipe3'), (4, 'gpb2'), (5, 'gpb4'), (6, 'gpb3')])
def test_lookup_every_packing(pipe, route, mask):
    """each packing against float64 directly; 45 groups leave the last block ragged under all of them"""
    n, h, w, r, L = LOOKUP_PACKED
    assert lookup_route(n, h, w, r, L, mask, pipe, cus()) == route
    with knob('lookup_pipe', pipe):
        check_lookup(n, h, w, r, L, mask, route)


def test_lookup_dispatch_own_choice_of_four_groups():
    """lookup_pipe = 0 at >= 4 x CUs groups of four-per-CU blocks: the dispatch itself packs four groups per block"""
    n, h, w, r, L, mask = LOOKUP_OWN_CHOICE
    assert lookup_route(n, h, w, r, L, mask, 0, cus()) == 'gpb4', f'{cus()} CUs: this shape no longer reaches the route'
    pyr = volume('nominal', n, h, w, L)
    fl = flows('edges', n, h, w, r, 0)
    ref = lookup64(pyr, fl, r)
    with knob('lookup_pipe', 0):
        got = gpu_lookup(pyr, fl, r, mask)
    ratio = worst_ratio(got, ref.ref, ref.sharp())
    measured(f'corr_lookup own choice {LOOKUP_OWN_CHOICE}, error / sharp bound', ratio)
    assert ratio <= 1.0


def test_lookup_store_policies_are_bit_equal():
    n, h, w, r, L, mask = LOOKUP_STORE
    assert lookup_route(n, h, w, r, L, mask, 0, cus()) == 'one'         # the knob acts on the one-group r = 4 launch
    pyr, cases = reference('nominal', n, h, w, r, L)
    name, _, fl, ref = cases[-1]
    dev, fld = [p.to(DEV) for p in pyr], fl.to(DEV)
    with knob('lookup_pipe', 0), knob('lookup_store', 0):
        want = ops.corr_lookup(dev, fld, r)
        assert worst_ratio(want.cpu(), ref.ref, ref.sharp()) <= 1.0
        for policy in (1, 2, 3, 4, 5):
            ops.tune('lookup_store', policy)
            assert same_bits(ops.corr_lookup(dev, fld, r), want), f'lookup_store {policy}'


@pytest.mark.parametrize('case', LOOKUP_GENERIC, ids=str)
def test_lookup_generic_kernel(case):
    n, h, w, r, L, mask = case
    assert lookup_route(n, h, w, r, L, mask, 0, cus()) == 'generic'
    check_lookup(n, h, w, r, L, mask, 'generic')


def test_lookup_constant_volume_in_range_windows():
    """a constant volume under a window that lies fully inside the map: the constant, within the sharp bound"""
    n, h, w, r, L, mask = 2, 12, 24, 4, 4, 0b0011
    pyr, cases = reference('constant', n, h, w, r, L)
    seen = 0
    for name, _, fl, ref in cases:
        got = gpu_lookup(pyr, fl, r, mask).numpy().astype(np.float64)
        inside = np.abs(ref.shadow - CONSTANT) < 1e-12
        seen += int(inside.sum())
        assert bool((np.abs(got[inside] - CONSTANT) <= ref.sharp()[inside]).all()), name
    assert seen > 0


def _per_level(t, r, L):
    d = (2 * r + 1) ** 2
    return [t[:, l * d:(l + 1) * d] for l in range(L)]


@pytest.mark.parametrize('mask', [0, 0b011])
@pytest.mark.parametrize('r', [4, 5])
def test_lookup_non_finite_flow_like_the_reference(r, mask):
    """flow 3e38: the reference's normalisation overflows at level 0 only -- NaN there, zeros below; NaN, +-inf: NaN at
    every level; 1e30: zeros.  Per level the NaN pattern is the oracle's, every other query is inside the sharp bound."""
    n, h, w, L = 1, 16, 24, 3
    pyr = volume('nominal', n, h, w, L)
    fl = flows('randn3', n, h, w, r)
    special = {(2, 3): (NAN, 0.5), (4, 4): (1.0, NAN), (5, 5): (float('inf'), float('inf')), (6, 6): (0.0, float('-inf')),
               (7, 7): (1e30, 0.0), (8, 9): (3e38, 0.0), (9, 2): (0.0, -3e38)}
    clean = fl.clone()
    for (y, x), v in special.items():
        fl[0, :, y, x] = torch.tensor(v)
        clean[0, :, y, x] = 0.
    want = oracle.corr_lookup(pyr, fl.clone(), r)
    got = gpu_lookup(pyr, fl, r, mask)
    for l, (g, o) in enumerate(zip(_per_level(got, r, L), _per_level(want, r, L))):
        assert torch.equal(torch.isnan(g), torch.isnan(o)), f'level {l}'
    lv = _per_level(got, r, L)
    assert bool(torch.isnan(lv[0][0, :, 8, 9]).all()) and float(lv[1][0, :, 8, 9].abs().max()) == 0.0
    assert float(got[0, :, 7, 7].abs().max()) == 0.0
    ref = lookup64(pyr, clean, r)
    ok = np.ones((h, w), dtype=bool)
    for (y, x) in special:
        ok[y, x] = False
    assert worst_ratio(got.numpy()[:, :, ok], ref.ref[:, :, ok], ref.sharp()[:, :, ok]) <= 1.0


def _poisoned_volume(n, h, w, L):
    """a nominal pyramid with, in every level, +inf and NaN each in column 0, at an interior pixel and in the last row --
    six kinds on disjoint queries (query index mod 13 = 0..5; the other seven stay clean)"""
    pyr = volume('nominal', n, h, w, L, seed=7)
    for l, p in enumerate(pyr):
        lh, lw = p.shape[-2:]
        places = ((lh // 2, 0), (lh // 2, lw // 2), (lh - 1, lw // 3))
        for k, (y, x) in enumerate(places):
            p[2 * k::13, 0, y, x] = float('inf')
            p[2 * k + 1::13, 0, y, x] = NAN
    return pyr


@pytest.mark.parametrize('mask,kinds', [(0, 'ffs'), (0b011, 'tts')])
def test_lookup_non_finite_volume_like_the_reference(mask, kinds):
    """inf / NaN inside a map (column 0, an interior pixel, the last row) on a footprint, a tiled and a whole-map level:
    the output is non-finite exactly where the reference's is -- a window that hangs over the map's edge reads zeros there,
    it does not multiply the clamped column by a zero weight -- and the fast and the generic kernel agree."""
    n, h, w, r, L = 2, 12, 24, 4, 3
    assert level_kinds(h, w, r, L, mask) == kinds
    assert lookup_route(n, h, w, r, L, mask, 1, cus()) == 'one' and lookup_route(n, h, w, 5, L, mask, 1, cus()) == 'generic'
    pyr = _poisoned_volume(n, h, w, L)
    fl = flows('randn3', n, h, w, r)
    want = oracle.corr_lookup(pyr, fl.clone(), r)
    with knob('lookup_pipe', 1):
        got = gpu_lookup(pyr, fl, r, mask)
    gen = gpu_lookup(pyr, fl, 5, mask).reshape(n, L, 11, 11, h, w)[:, :, 1:10, 1:10].reshape(got.shape)
    for l, (g, o, e) in enumerate(zip(_per_level(got, r, L), _per_level(want, r, L), _per_level(gen, r, L))):
        assert torch.equal(torch.isnan(g), torch.isnan(o)), f'level {l} ({kinds[l]}): NaN pattern'
        assert torch.equal(torch.isinf(g), torch.isinf(o)), f'level {l} ({kinds[l]}): inf pattern'
        assert torch.equal(torch.isnan(g), torch.isnan(e)) and same_bits(torch.nan_to_num(g), torch.nan_to_num(e)), \
            f'level {l} ({kinds[l]}): fast and generic kernels differ'
    fin = torch.isfinite(want)
    assert float((got[fin] - want[fin]).abs().max()) <= 5e-5


@pytest.mark.parametrize('n,h,w,kind', [(1, 1, 40, 'f'), (8, 1, 8, 's')])
def test_lookup_flat_axis_with_inf_is_nan_pinned(n, h, w, kind):
    """pinned, not changed: along a size-1 axis both taps of a pair are index 0 with weights 1 and 0
    (lk_centre), so an inf there comes out as inf 1 + inf 0 = NaN; the reference skips the second tap (out of the map) and
    returns inf.  Non-finite in the same places either way, on a footprint level and on one that is staged whole (flat_y
    points every window row at row 0)."""
    r, L = 4, 1
    assert level_kinds(h, w, r, L, 0) == kind
    pyr = volume('nominal', n, h, w, L, seed=9)
    pyr[0][::3, 0, 0, w // 2] = float('inf')
    fl = flows('randn3', n, h, w, r)
    want = oracle.corr_lookup(pyr, fl.clone(), r)
    with knob('lookup_pipe', 1):
        got = gpu_lookup(pyr, fl, r, 0)
    assert bool(torch.isinf(want).any()) and not bool(torch.isnan(want).any())
    assert torch.equal(torch.isnan(got), torch.isinf(want)) and not bool(torch.isinf(got).any())


# =============================================================================================================== pair
@pytest.mark.parametrize('mask', [0, 0b0011])
def test_pair_build_then_lookup_from_features(mask):
    """corr_build then corr_lookup on the GPU against float64 from the features.  The looked-up pyramid is off by at most
    bound_l per element, which the blend passes on as sum |w_i| bound_l(v_i); the lookup adds its own sharp bound, taken
    on the float64 pyramid: the second-order term 7 U sum |w_i| bound_l(v_i) (the lookup's rounding of the build's error,
    ~1e-12 of the value here) is left out, as the composed bound is stated."""
    n, c, h, w, L, r = 2, 64, 12, 24, 4, 4
    for regime in ('nominal', 'offset', 'cancelling'):
        worst = 0.0
        f1, f2 = features(regime, (n, c, h, w))
        lv, sh = build64(f1, f2, L)
        bd = build_bounds(lv, sh, c)
        pyr = ops.corr_build(f1.to(DEV), f2.to(DEV), L, tiled_levels=mask)
        for name, _, fl in flow_cases(n, h, w, r, L):
            got = ops.corr_lookup(pyr, fl.to(DEV), r, tiled_levels=mask).cpu()
            ref = lookup64(lv, fl, r)
            bound = lookup64(bd, fl, r).shadow + ref.sharp()
            ratio = worst_ratio(got, ref.ref, bound)
            assert ratio <= 1.0, f'{regime} {name}: error / composed bound = {ratio:.3g}'
            worst = max(worst, ratio)
        measured(f'corr pair {(n, c, h, w)} mask {mask:#06b} {regime}, error / composed bound', worst)
