"""GPU: the split-fp16 convolution kernel (conv_f16x3.hip) against float64 across fp16's range.

tests/test_conv_f16x3_host.py holds the restatement ``f16x3_ref64`` (what the kernel is specified to compute), the two
per-element bounds B_acc (kernel against specification) and B_model (specification against the true convolution), the
operand regimes and the planted defects.  Here every row (the six f16-* rows of the route table, a <2, 1, 1> row with 48
output channels, a stride-2 row) is launched in every regime, seeds 0 and 1, with the plain, bias + ReLU, BN affine +
residual and two-segment epilogues, and per element, with no tensor-wide scale and no absolute floor:

    |got - f16x3_ref64| <= B_acc                    |got - conv64| <= B_acc + B_model

The kernel is held to its specification in EVERY regime: where ``PackedConv.from_weight`` refuses the layer (small_w,
subnormal_band, a weight beyond fp16's range) the split packing is attached by hand for that, and ``test_packer_policy``
checks what the refusal gives -- another kernel family, inside c_m 2^-22 sum|w||x| + B_acc.  subnormal_band against the
restatement with subnormals KEPT is the measurement of what v_cvt_f16_f32 and the fp16 MFMA operands do on gfx950: the
planted-defect factors of the host file (hi flushed: > 2e4 bounds; lo' flushed: 60 - 700) say which one flushed if it fails.

Sample n of every input repeats sample n % PERIOD: the outputs must repeat bit for bit (every block of a launch does the
same arithmetic), and the first PERIOD samples are compared with float64.  The instantiation that ran is taken from the
dry-run query as tests/test_gpu_conv_exact.py does; ``test_zz_route_coverage`` fails unless all five ran in every regime.
The worst ratios per regime are printed there and stand in DESIGN.md."""
import ctypes as C

import pytest
import torch

from scflow_amd import _lib, ops
import test_conv_exact_host as H
import test_conv_f16x3_host as X
from test_gru_host import epilogue_expected, epilogue_tol

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = 1.2345678e30
GUARD = 4

RAN = {}                            # regime -> {(WM, WN, NK)} of the launches that were compared
WORST = {}                          # regime -> [worst |got - ref| / B_acc, worst |got - true| / (B_acc + B_model)]
DONE = set()                        # (row id, regime) checked in this session
SM = slice(0, X.PERIOD)


def _cus():
    return int(torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count)


def _pack(row, case, spec, force=True):
    """-> (PackedConv, refused by the packer's criterion).  force: a refused layer gets the split packing all the same (made
    on the host, where the roundings are the restatement's)"""
    pc = H.packed_conv(row, case, spec, DEV)
    refused = pc.wp16 is None
    if refused and force:
        pc.wp16 = ops.pack_conv_weight_f16x3(case['w']).to(DEV)
    return pc, refused


def _launch(row, case, spec, pc, x, res, out=None, parts=None):
    """one launch -> (result, families, info of the dry run of the same descriptor)"""
    with H.route_knobs(row):
        x0, x1, kw = H.launch_args(row, case, spec, x, res)
        if parts is not None:
            x0, x1 = parts
        d, _ = ops.conv_desc(pc, x0, x1, **kw)
        info = (C.c_int32 * 4)()
        assert _lib.load().scf_conv2d_query(C.byref(d), info) == 0
        with ops.record_conv_kernels() as ran:
            got = ops.conv2d(pc, x0, x1, out, **kw)
        try:
            torch.cuda.synchronize()
        except RuntimeError as exc:         # a device fault: nothing more is launched on this GPU by this session
            pytest.exit(f'{row.id}: the device reported {exc!r}', returncode=3)
    return got, {k for _, k in ran}, tuple(info)


def _assert_route(row, fams, info, what):
    """the split-fp16 kernel ran, in the row's instantiation (pinned on 256 CUs) -> the instantiation"""
    if row.family != 'f16x3':
        assert 'f16x3' not in fams, (what, fams)
        return None
    assert fams == {'f16x3'}, (what, fams)
    inst = X.instantiation(row, info)
    if _cus() == 256:
        assert inst == X.instantiation(row) and info[:2] == tuple(row.info[:2]), (what, info)
    return inst


def _periodic(got, what):
    n = got.shape[0]
    if n > X.PERIOD:
        assert H.same_bits(got[X.PERIOD:], got[:n - X.PERIOD]), f'{what}: sample n differs from sample n - {X.PERIOD} on the same input'


def _ratio(err, lim):
    """worst err / lim over the elements; inf where an element is outside although the quotient is undefined (0 / 0 is inside)"""
    inside = err <= lim
    r = torch.where(inside & (lim == 0), torch.zeros_like(err), err / lim)
    r = torch.where(inside | torch.isfinite(r), r, torch.full_like(r, float('inf')))
    return float(r.max()), int((~inside).sum())


def _note(regime, r_acc, r_true):
    w = WORST.setdefault(regime, [0.0, 0.0])
    w[0], w[1] = max(w[0], r_acc), max(w[1], r_true)


def _dev(case):
    return case['x'].to(DEV), case['res'].to(DEV)


def _check(rid, regime):
    row = X.BY_ID[rid]
    for seed in X.SEEDS:
        if regime == 'over_range':
            _check_over_range(row, seed)
            continue
        case = X.operands(row, regime, seed)
        x, res = _dev(case)
        for name, spec in X.variants(row).items():
            pc, _ = _pack(row, case, spec)
            what = f'{rid} {regime}/{seed} [{name}]'
            got, fams, info = _launch(row, case, spec, pc, x, res)
            inst = _assert_route(row, fams, info, what)
            _periodic(got, what)
            g = got[SM].double().cpu()
            assert bool(torch.isfinite(g).all()), f'{what}: non-finite output in a finite regime'
            b = X.bounds(row, case, spec, SM)
            if inst is not None:
                r_acc, n_acc = _ratio((g - b['ref']).abs(), b['b_acc'])
                r_true, n_true = _ratio((g - b['true']).abs(), b['b_acc'] + b['b_model'])
                print(f'[measured] {what} <{inst}>: {r_acc:.3f} of B_acc, {r_true:.3f} of B_acc + B_model')
                assert n_acc == 0, f'{what}: {n_acc} elements outside B_acc of the specification, worst {r_acc:.3g}'
                assert n_true == 0, f'{what}: {n_true} elements outside B_acc + B_model of float64, worst {r_true:.3g}'
                _note(regime, r_acc, r_true)
                RAN.setdefault(regime, set()).add(inst)
            else:                           # the stride-2 row: an fp32 kernel, held to the fp32 bound
                r32, n32 = _ratio((g - b['true']).abs(), X.fp32_bound(row, case, spec, SM))
                print(f'[measured] {what} on {sorted(fams)}: {r32:.3f} of the fp32 bound')
                assert n32 == 0, f'{what}: {n32} elements outside the fp32 bound, worst {r32:.3g}'
            if name == 'plain':
                again, fams2, _ = _launch(row, case, spec, pc, x, res)
                assert fams2 == fams and H.same_bits(again, got), f'{what}: a second run gives other bits'
    DONE.add((rid, regime))


def _field(row, places):
    """(n, Ho, Wo) mask of the outputs whose receptive field holds one of ``places`` = rows of (n, c, i, j)"""
    (kh, kw), (ph, pw), s = row.k, row.pad, row.stride
    ho, wo = H.out_hw(row)
    oy, ox = torch.arange(ho).view(-1, 1), torch.arange(wo).view(1, -1)
    m = torch.zeros((row.n, ho, wo), dtype=torch.bool)
    for n, _, i, j in places.tolist():
        ky, kx = i + ph - oy * s, j + pw - ox * s
        m[n] |= (ky >= 0) & (ky < kh) & (kx >= 0) & (kx < kw)
    return m


def _check_over_range(row, seed):
    """seed 0, one activation of 1e5 per sample: every output of its receptive field, in every channel, is non-finite, and
    every other output has the bits of the run with 1.0 in its place.  seed 1, one weight of 1e5: the packer refuses the layer
    (test_packer_policy); nothing to launch on this route."""
    if seed != 0:
        return
    case = X.operands(row, 'over_range', 0)
    places = (case['x'] == X.OVER).nonzero()
    assert places.shape[0] == row.n
    field = _field(row, places)
    tame = dict(case, x=torch.where(case['x'] == X.OVER, torch.ones_like(case['x']), case['x']))
    x, res = _dev(case)
    xt = tame['x'].to(DEV)
    for name, spec in X.variants(row).items():
        what = f'{row.id} over_range/0 [{name}]'
        pc, refused = _pack(row, case, spec, force=False)
        assert not refused
        got, fams, info = _launch(row, case, spec, pc, x, res)
        clean, fams2, _ = _launch(row, tame, spec, pc, xt, res)
        inst = _assert_route(row, fams, info, what)
        assert fams2 == fams
        got, clean = got.cpu(), clean.cpu()
        assert bool(torch.isfinite(clean).all())
        out = ~field[:, None].expand_as(got)
        assert H.same_bits(got[out], clean[out]), f'{what}: an output outside the receptive field of the 1e5 differs from the run without it'
        inside = got[field[:, None].expand_as(got)]
        if inst is None:                    # the fp32 kernel: finite
            assert bool(torch.isfinite(inside).all()), what
            continue
        if spec['act'] == H.RELU:           # ReLU is compare + select: NaN -> 0, -inf -> 0
            assert bool((~torch.isfinite(inside) | (inside == 0)).all()), what
        else:
            assert bool((~torch.isfinite(inside)).all()), f'{what}: a finite output inside the receptive field of the 1e5'
        RAN.setdefault('over_range', set()).add(inst)
    WORST.setdefault('over_range', [0.0, 0.0])


@pytest.mark.parametrize('regime', X.REGIMES)
@pytest.mark.parametrize('rid', X.IDS)
def test_bounds(rid, regime):
    _check(rid, regime)


@pytest.mark.parametrize('rid', X.IDS)
def test_pow2_scaling_is_exact(rid):
    """conv(2^a x, 2^b w) == 2^(a + b) conv(x, w) bit for bit on operands whose halves, products and sums stay normal: no
    tolerance.  A conversion or an operand path that loses bits at one end of fp16's normal range breaks it."""
    row = X.BY_ID[rid]
    spec = X.variants(row)['plain']
    base = None
    for seed, (a, b) in enumerate(X.POW2_GRID):
        case = X.operands(row, 'pow2_scaled', seed)
        if base is None:
            c0 = dict(case, x=case['x'] * 2.0 ** -a, w=case['w'] * 2.0 ** -b)
            base, fams0, _ = _launch(row, c0, spec, _pack(row, c0, spec, force=False)[0], c0['x'].to(DEV), None)
        pc, refused = _pack(row, case, spec, force=False)
        assert not refused
        got, fams, info = _launch(row, case, spec, pc, case['x'].to(DEV), None)
        _assert_route(row, fams, info, f'{rid} 2^{a} x, 2^{b} w')
        want = base * 2.0 ** (a + b)
        assert bool(torch.isfinite(want).all())
        assert H.same_bits(got, want), f'{rid}: conv(2^{a} x, 2^{b} w) != 2^{a + b} conv(x, w)'


def _sentinel_intact(t):
    want = torch.full((1,), SENTINEL, dtype=torch.float32, device=t.device).view(torch.int32)
    return bool((t.contiguous().view(torch.int32) == want).all())


def _guarded_input(seg):
    n, c, h, w = seg.shape
    margin = (GUARD * h * w + 4096 + 3) // 4 * 4
    inner = n * (c + 2 * GUARD) * h * w
    buf = torch.full((margin + inner + margin,), float('nan'), dtype=torch.float32, device=seg.device)
    view = buf[margin:margin + inner].view(n, c + 2 * GUARD, h, w)[:, GUARD:GUARD + c]
    view.copy_(seg)
    return buf, view


@pytest.mark.parametrize('rid', X.IDS)
def test_guard_bands(rid):
    """on near_max operands (the largest finite halves): an output slice of a wider tensor leaves the sentinel around it alone,
    inputs as slices of NaN-filled tensors give the same bits -- one or two segments"""
    row = X.BY_ID[rid]
    case = X.operands(row, 'near_max', 0)
    x, res = _dev(case)
    vs = X.variants(row)
    spec = vs['bn_res']
    pc, _ = _pack(row, case, spec)
    whole, fams, _ = _launch(row, case, spec, pc, x, res)
    ho, wo = H.out_hw(row)
    wide = torch.full((row.n, row.cout + 2 * GUARD, ho, wo), SENTINEL, dtype=torch.float32, device=DEV)
    got, fams2, _ = _launch(row, case, spec, pc, x, res, out=wide[:, GUARD:GUARD + row.cout])
    assert fams2 == fams
    assert _sentinel_intact(wide[:, :GUARD]) and _sentinel_intact(wide[:, GUARD + row.cout:]), f'{rid}: sentinel overwritten'
    assert H.same_bits(got, whole), f'{rid}: other bits into a slice'
    buf, view = _guarded_input(x)
    got, _, _ = _launch(row, case, spec, pc, view, res)
    assert H.same_bits(got, whole), f'{rid}: other bits with the input inside NaN guard bands'
    if 'two' in vs:
        pc2, _ = _pack(row, case, vs['two'])
        want, _, _ = _launch(row, case, vs['two'], pc2, x, res)
        (b0, v0), (b1, v1) = _guarded_input(x[:, :row.c0]), _guarded_input(x[:, row.c0:])
        got, _, _ = _launch(row, case, vs['two'], pc2, x, res, parts=(v0, v1))
        assert H.same_bits(got, want), f'{rid}: other bits with two segments inside NaN guard bands'


def test_device_packing_keeps_subnormals():
    """``pack_conv_weight_f16x3`` on the device gives the bits of the host's packing, subnormal halves included"""
    row = X.BY_ID['f16-11-nk1']
    for regime in ('nominal', 'small_w', 'subnormal_band', 'near_max'):
        for seed in X.SEEDS:
            w = X.operands(row, regime, seed)['w']
            host, dev = ops.pack_conv_weight_f16x3(w), ops.pack_conv_weight_f16x3(w.to(DEV)).cpu()
            assert torch.equal(host.view(torch.int16), dev.view(torch.int16)), f'{regime}/{seed}: the device packs other fp16 bits'


@pytest.mark.parametrize('rid', ['f16-11-nk1', 'f16-21-nk2', 'f16-12'])
def test_packer_policy(rid):
    """what ``PackedConv.from_weight`` decides: layers whose weights lie in the split's domain take the route; small_w,
    subnormal_band and a weight of 1e5 keep wp16 = None, ``record_conv_kernels`` shows another family, and the result is
    inside c_m 2^-22 sum|w||x| + B_acc of float64 -- finite for the 1e5 weight, where the split would give an infinite half"""
    row = X.BY_ID[rid]
    spec = X.variants(row)['bias_relu']
    for regime, seed, refuse in (('nominal', 0, False), ('three_decades', 0, False), ('three_decades', 1, False),
                                 ('small_w', 0, True), ('small_w', 1, True), ('subnormal_band', 0, True), ('over_range', 1, True)):
        case = X.operands(row, regime, seed)
        pc, refused = _pack(row, case, spec, force=False)
        assert refused == refuse, (rid, regime, seed, ops.f16x3_weight_excess(case['w']))
        x, res = _dev(case)
        got, fams, info = _launch(row, case, spec, pc, x, res)
        assert ('f16x3' not in fams) if refuse else (fams == {'f16x3'}), (rid, regime, seed, fams)
        assert bool(torch.isfinite(got).all())
        if regime == 'over_range':
            # the per-element bound is the direct kernels': a Winograd kernel mixes the 1e5 into every product of its tile and
            # is bounded tile by tile only (761 x this bound measured on F(4, 5)); the fp32 routes are not this file's subject
            direct = row._replace(knobs=dict(row.knobs, wino=False))
            got, fams, info = _launch(direct, case, spec, pc, x, res)
            assert fams <= {'direct-dma', 'direct-mfma', 'direct-mfma-ksplit'}, fams
        g = got[SM].double().cpu()
        assert bool(torch.isfinite(g).all())
        if regime == 'over_range':
            lim = X.fp32_bound(row, case, spec, SM)
            true = X.epilogue64(case, X.conv64(row, case['x'][SM], case['w']), spec, SM)
        else:
            b = X.bounds(row, case, spec, SM)
            lim, true = X.C_M * 2.0 ** -22 * b['mag'] + b['b_acc'], b['true']
        r, nbad = _ratio((g - true).abs(), lim)
        print(f'[measured] {rid} {regime}/{seed} on {sorted(fams)}: {r:.3f} of c_m 2^-22 sum|w||x| + B_acc')
        assert nbad == 0, f'{rid} {regime}/{seed} on {sorted(fams)}: {nbad} elements outside the fp32-class bound, worst {r:.3g}'


# ------------------------------------------------------------------------------------------------------------ GRU launches
GRU_HC, GRU_CX = 64, 40
GRU_SHAPES = [(2, 8, 8), (1, 13, 21)]
GRU_REGIMES = [('nominal', 0), ('three_decades', 0), ('small_w', 1)]
PASSES = [((1, 5), (0, 2)), ((5, 1), (2, 0))]


def _gru_row(tag, n, h, w, cin, cout, k, pad, c0, info):
    return H.Row(tag, n, cin, cout, k, 1, pad, h, w, c0, dict(f16=True), 'f16x3', info, '')


def _gru_weights(regime, seed, k, g):
    hc, cin = GRU_HC, GRU_HC + GRU_CX
    def draw(cout):
        w = torch.randn((cout, cin, *k), generator=g) * (1.0 / (cin * 5)) ** 0.5
        if regime == 'three_decades':
            w = w * 10.0 ** (-3.0 * torch.rand(w.shape, generator=g))
        if regime == 'small_w':
            w = w * 1e-6
        return w
    return draw(2 * hc), draw(hc), torch.randn(2 * hc, generator=g) * 0.5, torch.randn(hc, generator=g) * 0.5


def _preact(tag, pc, x0, x1, k, pad, w, bias, forced):
    """the plain launch of a GRU layer: its fp32 pre-activation, held to the two bounds (split packing) or to the fp32 bound"""
    n, _, h, wd = x0.shape
    d, _ = ops.conv_desc(pc, x0, x1)
    info = (C.c_int32 * 4)()
    assert _lib.load().scf_conv2d_query(C.byref(d), info) == 0
    with ops.record_conv_kernels() as ran:
        v = ops.conv2d(pc, x0, x1)
    fams = {f for _, f in ran}
    xc = (x0 if x1 is None else torch.cat([x0, x1], 1)).cpu()
    split = pc.wp16 is not None
    assert fams == ({'f16x3'} if split else fams - {'f16x3'}), (tag, fams)
    row = _gru_row(tag, n, h, wd, xc.shape[1], w.shape[0], k, pad, 0 if x1 is None else x0.shape[1],
                   tuple(info) if split else (1, 1, 1, -1))
    if not split:
        row = row._replace(family='fp32')
    case = dict(x=xc, w=w, b=bias)
    spec = dict(X.variants(row)['plain'], bias=True)
    g = v.double().cpu()
    assert bool(torch.isfinite(g).all())
    if split:
        b = X.bounds(row, case, spec)
        r_acc, n_acc = _ratio((g - b['ref']).abs(), b['b_acc'])
        r_true, n_true = _ratio((g - b['true']).abs(), b['b_acc'] + b['b_model'])
        print(f'[measured] {tag} <{X.instantiation(row)}>{" (packing forced)" if forced else ""}: {r_acc:.3f} of B_acc, {r_true:.3f} of B_acc + B_model')
        assert n_acc == 0 and n_true == 0, (tag, r_acc, r_true)
    else:
        true = X.epilogue64(case, X.conv64(row, xc, w), spec)
        r32, n32 = _ratio((g - true).abs(), X.fp32_bound(row, case, spec))
        print(f'[measured] {tag} on {sorted(fams)}: {r32:.3f} of the fp32 bound')
        assert n32 == 0, (tag, r32)
    return v, fams


def _sharp(kind, got, v, **kw):
    err = (got.double() - epilogue_expected(kind, v, **kw)).abs()
    tol = epilogue_tol(kind, v, **kw)
    return int((~(err <= tol)).sum()), float((err / tol).max())


@pytest.mark.parametrize('regime,seed', GRU_REGIMES)
@pytest.mark.parametrize('shape', GRU_SHAPES, ids=str)
def test_gru_launches(shape, regime, seed):
    """CONV_GRU_ZR and CONV_GRU_Q under 'f16x3', 1x5 then 5x1: the pre-activation of each layer (its plain launch) inside
    the two bounds, the gate outputs inside the epilogue tolerances of tests/test_gru_host.py on that pre-activation, and
    ``sepconv_gru`` (the C entry with wp_zr_f16 / wp_q_f16) bit for bit the launch sequence.  small_w: the packer refuses the
    layers, the launches take another family and are held to the fp32 bound; then once more with the packing forced."""
    n, h, w = shape
    hc = GRU_HC
    g = torch.Generator().manual_seed(1000 * GRU_SHAPES.index(shape) + 10 * seed + len(regime))
    hx0 = torch.randn((n, hc + GRU_CX, h, w), generator=g)
    hx0[:, :hc] = torch.tanh(hx0[:, :hc])
    weights = [_gru_weights(regime, seed, k, g) for k, _ in PASSES]
    prev = ops.set_conv_precision('f16x3')
    try:
        for forced in ((False, True) if regime == 'small_w' else (False,)):
            packs = []
            for (k, pad), (wzr, wq, bzr, bq) in zip(PASSES, weights):
                pzr = ops.PackedConv.from_weight(wzr.to(DEV), bzr.to(DEV), padding=pad)
                pq = ops.PackedConv.from_weight(wq.to(DEV), bq.to(DEV), padding=pad)
                assert (pzr.wp16 is None) == (regime == 'small_w') and (pq.wp16 is None) == (regime == 'small_w')
                if forced:
                    pzr.wp16, pq.wp16 = ops.pack_conv_weight_f16x3(wzr).to(DEV), ops.pack_conv_weight_f16x3(wq).to(DEV)
                packs.append((pzr, pq))
            buf = hx0.to(DEV)
            hv, xv = buf[:, :hc], buf[:, hc:]
            z, rh = torch.empty((2, n, hc, h, w), device=DEV)
            for i, ((k, pad), (wzr, wq, bzr, bq), (pzr, pq)) in enumerate(zip(PASSES, weights, packs)):
                tag = f'gru {regime} {shape} {k[0]}x{k[1]}'
                h_old = hv.clone()
                v_zr, f_zr = _preact(tag + ' z|r', pzr, buf, None, k, pad, wzr, bzr, forced)
                with ops.record_conv_kernels() as ran:
                    ops.conv2d(pzr, buf, out=z, mode=ops.CONV_GRU_ZR, gru_h=hv, gru_aux=rh)
                assert {f for _, f in ran} == f_zr, (tag, ran)
                v_q, f_q = _preact(tag + ' q', pq, rh, xv, k, pad, wq, bq, forced)
                with ops.record_conv_kernels() as ran:
                    ops.conv2d(pq, rh, xv, out=hv, mode=ops.CONV_GRU_Q, gru_h=hv, gru_z=z)
                assert {f for _, f in ran} == f_q, (tag, ran)
                for kind, got, v, kw in (('z', z, v_zr[:, :hc], {}), ('rh', rh, v_zr[:, hc:], {'h': h_old}),
                                         ('h', hv, v_q, {'h': h_old, 'z': z})):
                    nbad, worst = _sharp(kind, got, v, **kw)
                    print(f'[measured] {tag} {kind}: {worst:.3f} of the epilogue tolerance')
                    assert nbad == 0, f'{tag}: {nbad} elements of {kind} outside the epilogue tolerance, worst {worst:.3g}'
            assert torch.equal(buf[:, hc:], hx0[:, hc:].to(DEV)), 'the launches wrote outside h'
            entry = hx0.to(DEV)
            z2, rh2 = torch.empty((2, n, hc, h, w), device=DEV)
            with ops.record_conv_kernels() as ran:
                ops.sepconv_gru(packs, entry, hc, z2, rh2)
            assert len(ran) == 4 and all((f == 'f16x3') == (regime != 'small_w' or forced) for _, f in ran), ran
            assert H.same_bits(entry, buf) and H.same_bits(z2, z) and H.same_bits(rh2, rh), f'{regime} {shape}: sepconv_gru differs from its launches'
    finally:
        ops.set_conv_precision(prev)


@pytest.mark.parametrize('regime,seed', GRU_REGIMES)
@pytest.mark.parametrize('shape', GRU_SHAPES, ids=str)
def test_conv2d_pair(shape, regime, seed):
    """two independent layers through ``conv2d_pair`` under 'f16x3': the bits of two ``conv2d`` calls, whose results are held
    to the bounds, on the family the packer's decision implies"""
    n, h, w = shape
    g = torch.Generator().manual_seed(77 + 1000 * GRU_SHAPES.index(shape) + seed)
    xa, xb = torch.randn((n, 36, h, w), generator=g), torch.randn((n, 36, h, w), generator=g)
    prev = ops.set_conv_precision('f16x3')
    try:
        layers = []
        for x, (k, pad) in ((xa, PASSES[0]), (xb, PASSES[1])):
            wzr, _, bzr, _ = _gru_weights(regime, seed, k, g)
            wt, b = wzr[:40, :36].contiguous(), bzr[:40].contiguous()
            pc = ops.PackedConv.from_weight(wt.to(DEV), b.to(DEV), padding=pad)
            v, fams = _preact(f'pair {regime} {shape} {k[0]}x{k[1]}', pc, x.to(DEV), None, k, pad, wt, b, False)
            layers.append((pc, x.to(DEV), v, fams))
        with ops.record_conv_kernels() as ran:
            oa, ob = ops.conv2d_pair((layers[0][0], layers[0][1]), (layers[1][0], layers[1][1]))
        assert {f for _, f in ran} == layers[0][3] | layers[1][3], ran
        assert H.same_bits(oa, layers[0][2]) and H.same_bits(ob, layers[1][2]), f'{regime} {shape}: the pair differs from two launches'
    finally:
        ops.set_conv_precision(prev)


def test_zz_route_coverage():
    """all five instantiations of conv_f16x3_kernel ran and were compared in every regime"""
    for row in X.ROWS:
        for regime in X.REGIMES:
            if (row.id, regime) not in DONE and row.family == 'f16x3':
                _check(row.id, regime)
    for regime in X.REGIMES:
        r_acc, r_true = WORST[regime]
        print(f'[measured] {regime}: worst {r_acc:.3f} of B_acc, {r_true:.3f} of B_acc + B_model; ran {sorted(RAN[regime])}')
    if _cus() != 256:
        pytest.skip(f'route table pinned on 256 CUs, this device has {_cus()}')
    for regime in X.REGIMES:
        assert RAN[regime] == set(X.INSTANTIATIONS), (regime, RAN[regime])
