"""GPU: every forward convolution route, bit for bit, on exact operands.

tests/test_conv_exact_host.py holds the route table (one row per kernel family and template instantiation a single
``scf_conv2d`` launch reaches), lattice operands on which every product and partial sum of every route is an fp32 number, the
certificate that proves it without a GPU result, and the float64 reference.  Here each row is launched and

a. ``record_conv_kernels`` names the expected family and ``scf_conv2d_query`` answers the pinned info (256 CUs);
b. plain, with bias, with bias + residual + ReLU, with the exact BN fold, with ``act_split`` on and off a 32-channel fragment
   boundary (ReLU below / above), and with two input segments, the output has the BITS of the float64 reference;
c. written into a channel slice of a wider tensor it leaves the sentinel around it alone and keeps its bits;
d. read from channel slices of wider tensors full of NaN (other channels, the floats before the first and after the last
   sample) it keeps its bits: a read outside the operand may happen, but must not reach an accumulator;
e. one NaN in the input makes exactly its receptive field NaN, in every output channel (Winograd: nothing beyond the
   transform window along a filter axis, nothing outside the receptive field on the other axis);
f. a second run gives the same bits.

The table is pinned for the 256-CU MI355X; on another CU count the family / info assertions and the coverage floor are
skipped with a message and every other check runs on whatever route the device takes."""
import contextlib
import ctypes as C

import pytest
import torch

from scflow_amd import _lib, ops
import test_conv_exact_host as H

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = 1.2345678e30
GUARD = 4                       # guard channels on each side: 4 * Ho * Wo floats keep every 16-byte alignment of the operand

_STATE = {}                     # row id -> the row's case on the device, its plain result, the families that ran
RAN, COMPARED = {}, {}          # row id -> family of the plain launch / number of variants compared bit for bit


def _cus():
    return int(torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count)


@contextlib.contextmanager
def _knobs(row):
    with H.route_knobs(row):
        ws = bool(row.knobs.get('workspace'))
        if ws:
            ops.register_conv_workspace(True)
        try:
            yield
        finally:
            if ws:
                ops.register_conv_workspace(False)


def _packed(st, spec):
    key = (spec['bias'], spec['bn'])
    if key not in st['packed']:
        st['packed'][key] = H.packed_conv(st['row'], st['case'], spec, DEV)
    return st['packed'][key]


def _finish(row, got):
    """explicit K slices: the raw partial tensors summed in slice order on the host in float64 (exact too), as fp32"""
    if row.knobs.get('kslices', 1) <= 1:
        return got
    total = got[0].double().cpu()
    for s in range(1, got.shape[0]):
        total = total + got[s].double().cpu()
    out = total.float()
    assert torch.equal(out.double()[~torch.isnan(total)], total[~torch.isnan(total)]), 'a sum of the slices is no fp32 number'
    return out.to(got.device)


def _run(st, spec, x=None, parts=None, out=None):
    """one launch of a variant -> (result, set of families that ran).  x: another input tensor; parts: (x0, x1) views."""
    row, case = st['row'], st['case']
    pc = _packed(st, spec)
    with _knobs(row):
        x0, x1, kw = H.launch_args(row, case, spec, st['x'] if x is None else x, st['res'])
        if parts is not None:
            x0, x1 = parts
        with ops.record_conv_kernels() as ran:
            got = ops.conv2d(pc, x0, x1, out, **kw)
        try:
            torch.cuda.synchronize()
        except RuntimeError as exc:         # a device fault: nothing more is launched on this GPU by this session
            pytest.exit(f'{row.id}: the device reported {exc!r}', returncode=3)
    return _finish(row, got), {k for _, k in ran}


def _state(row):
    if row.id not in _STATE:
        case = H.lattice_case(row)
        st = dict(row=row, case=case, packed={}, x=case['x'].to(DEV), res=case['res'].to(DEV))
        _STATE.clear()          # one row's tensors at a time on the device
        _STATE[row.id] = st
        st['plain'], st['families'] = _run(st, H.variants(row)['plain'])
        RAN[row.id] = st['families']
    return _STATE[row.id]


def _explain(got, want):
    g, w = got.detach().cpu(), want.detach().cpu()
    diff = g.view(torch.int32) != w.view(torch.int32)
    idx = tuple(int(v) for v in diff.nonzero()[0])
    return f'{int(diff.sum())} of {diff.numel()} elements differ, first at {idx}: got {float(g[idx])!r}, want {float(w[idx])!r}'


def _assert_bits(got, want, what):
    assert H.same_bits(got, want), f'{what}: {_explain(got, want)}'


def _check_variants(row):
    st = _state(row)
    case = st['case']
    certified = case['certificate']['ok'] and row.id not in H.UNCERTIFIED
    pinned = _cus() == 256
    n = 0
    for name, spec in H.variants(row).items():
        got, fams = (st['plain'], st['families']) if name == 'plain' else _run(st, spec)
        if pinned and not H.refused(row, spec):
            assert fams == {row.family}, (row.id, name, fams)
        if certified:
            ref = H.reference(row, case, spec)
            want = ref.float()
            assert torch.equal(want.double(), ref)
            _assert_bits(got, want, f'{row.id} [{name}] on {sorted(fams)}')
            n += 1
    COMPARED[row.id] = n
    return st


@pytest.mark.parametrize('rid', H.IDS)
def test_route_and_bits(rid):
    """a, b, f: the expected route ran, every epilogue has the float64 reference's bits, a second run repeats them"""
    row = H.BY_ID[rid]
    st = _check_variants(row)
    if _cus() == 256:
        spec = H.variants(row)['plain']
        with _knobs(row):
            x0, x1, kw = H.launch_args(row, st['case'], spec, st['x'], st['res'])
            d, _ = ops.conv_desc(_packed(st, spec), x0, x1, **kw)
            info = (C.c_int32 * 4)()
            assert _lib.load().scf_conv2d_query(C.byref(d), info) == 0
        assert tuple(info) == tuple(row.info), (rid, tuple(info))
    again, fams = _run(st, H.variants(row)['plain'])
    assert fams == st['families']
    _assert_bits(again, st['plain'], f'{rid}: second run')


def _sentinel_intact(t):
    want = torch.full((1,), SENTINEL, dtype=torch.float32, device=t.device).view(torch.int32)
    return bool((t.contiguous().view(torch.int32) == want).all())


def _guarded_input(seg):
    """seg as a channel slice of a wider tensor inside a larger allocation; everything else NaN"""
    n, c, h, w = seg.shape
    margin = (GUARD * h * w + 4096 + 3) // 4 * 4
    inner = n * (c + 2 * GUARD) * h * w
    buf = torch.full((margin + inner + margin,), float('nan'), dtype=torch.float32, device=seg.device)
    view = buf[margin:margin + inner].view(n, c + 2 * GUARD, h, w)[:, GUARD:GUARD + c]
    view.copy_(seg)
    return buf, view


@pytest.mark.parametrize('rid', H.IDS)
def test_guard_bands(rid):
    """c, d: nothing is written outside an output slice; nothing read outside an input slice reaches the result"""
    row = H.BY_ID[rid]
    st = _state(row)
    vs = H.variants(row)
    sliced = row.knobs.get('kslices', 1) > 1
    # c. the output as a channel slice (explicit K slices: the partial tensors inside a larger allocation)
    name = 'bias_res_relu' if 'bias_res_relu' in vs and not H.refused(row, vs['bias_res_relu']) else 'plain'
    whole, fams = _run(st, vs[name])
    ho, wo = H.out_hw(row)
    if sliced:
        s = row.knobs['kslices']
        numel, margin = s * row.n * row.cout * ho * wo, 4096
        buf = torch.full((numel + 2 * margin,), SENTINEL, dtype=torch.float32, device=DEV)
        got, fams2 = _run(st, vs[name], out=buf[margin:margin + numel].view(s, row.n, row.cout, ho, wo))
        assert _sentinel_intact(buf[:margin]) and _sentinel_intact(buf[margin + numel:])
    else:
        wide = torch.full((row.n, row.cout + 2 * GUARD, ho, wo), SENTINEL, dtype=torch.float32, device=DEV)
        got, fams2 = _run(st, vs[name], out=wide[:, GUARD:GUARD + row.cout])
        assert _sentinel_intact(wide[:, :GUARD]) and _sentinel_intact(wide[:, GUARD + row.cout:]), f'{rid}: sentinel overwritten'
    assert fams2 == fams, (rid, fams, fams2)
    _assert_bits(got, whole, f'{rid} [{name}] into a slice')
    # d. the inputs as channel slices of NaN-filled tensors
    buf, view = _guarded_input(st['x'])
    got, fams2 = _run(st, vs['plain'], x=view)
    assert fams2 == st['families'], (rid, st['families'], fams2)
    _assert_bits(got, st['plain'], f'{rid}: input inside NaN guard bands')
    if 'two' in vs:
        want, fams = _run(st, vs['two'])
        b0, v0 = _guarded_input(st['x'][:, :row.c0])
        b1, v1 = _guarded_input(st['x'][:, row.c0:])
        got, fams2 = _run(st, vs['two'], parts=(v0, v1))
        assert fams2 == fams, (rid, fams, fams2)
        _assert_bits(got, want, f'{rid}: two segments inside NaN guard bands')


def _nan_places(row):
    return [('corner', 0, 0, 0, 0),
            ('last row' + (' of an odd-height map' if row.H % 2 else ''), row.n // 2, row.cin // 2, row.H - 1, row.W // 2),
            ('last channel of the tail chunk', row.n - 1, row.cin - 1, row.H // 2, row.W - 1)]


@pytest.mark.parametrize('rid', H.IDS)
def test_one_nan_stays_in_its_receptive_field(rid):
    """e: NaN placement"""
    row = H.BY_ID[rid]
    st = _state(row)
    (kh, kw), (ph, pw), s = row.k, row.pad, row.stride
    ho, wo = H.out_hw(row)
    oy, ox = torch.arange(ho).view(-1, 1), torch.arange(wo).view(1, -1)
    clean = st['plain'].cpu()
    for what, n, c, i, j in _nan_places(row):
        x = st['x'].clone()
        x[n, c, i, j] = float('nan')
        got, fams = _run(st, H.variants(row)['plain'], x=x)
        got = got.cpu()
        ky, kx = i + ph - oy * s, j + pw - ox * s
        field = ((ky >= 0) & (ky < kh) & (kx >= 0) & (kx < kw)).expand(ho, wo)
        assert bool(field.any()), (rid, what)
        assert bool(torch.isnan(got[n][:, field]).all()), f'{rid}, NaN at the {what}: an output of its receptive field is finite'
        fam = next(iter(fams)) if len(fams) == 1 else None
        if fam in H.WINDOW:                 # nothing beyond the transform window along a filter axis
            win = H.WINDOW[fam]
            far_y = (oy - i).abs() > win if kh > 1 else oy != i
            far_x = (ox - j).abs() > win if kw > 1 else ox != j
            keep = (far_y | far_x).expand(ho, wo)
        else:
            keep = ~field
        others = [m for m in range(row.n) if m != n]
        _assert_bits(got[others], clean[others], f'{rid}, NaN at the {what}: another sample')
        _assert_bits(got[n][:, keep].contiguous(), clean[n][:, keep].contiguous(), f'{rid}, NaN at the {what}: outside the field')


def test_zz_route_coverage():
    """every KERNEL_NAMES family and every table row was launched and compared in this session, at least once each"""
    cus = _cus()
    for row in H.ROUTES:
        if row.id not in COMPARED:
            _check_variants(row)
    by_family = {}
    for row in H.ROUTES:
        for f in RAN[row.id]:
            by_family[f] = by_family.get(f, 0) + 1
    print(f'[measured] plain launches per family: {by_family}; rows compared: {sum(1 for v in COMPARED.values() if v)} of {len(H.ROUTES)}')
    if cus != 256:
        pytest.skip(f'route table pinned on 256 CUs, this device has {cus}')
    assert not [r.id for r in H.ROUTES if RAN[r.id] != {r.family}], {r.id: RAN[r.id] for r in H.ROUTES if RAN[r.id] != {r.family}}
    assert not [r.id for r in H.ROUTES if COMPARED[r.id] < 1 and r.id not in H.UNCERTIFIED]
    assert set(by_family) == set(_lib.KERNEL_NAMES.values()), by_family
