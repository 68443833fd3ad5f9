"""GPU: gru_grad.hip (scf_gru_gate_grad_q, scf_gru_gate_grad_r, scf_gru_carry, scf_gru_gate_state), ConvGRU.backward /
recompute_gates, SCFlowDecoder.keep = 'gru' / gru_backward and SCFlowRefiner.loss_and_gru_grads against the float64
restatement and the derived bounds of tests/test_gru_grad_host.py.  Every comparison is `error <= bound` over ALL
elements (ratio <= 1) or bit equality; there is no absolute tolerance.  The measured ratios are recorded in DESIGN.md
section 4.11."""
import json
import os

import numpy as np
import pytest
import torch

import scflow_amd
from scflow_amd import _lib, ops
from scflow_amd._lib import ScflowHipError
from scflow_amd.modules import ConvGRU
import test_gru_grad_host as GH
import test_gru_host as GF
import test_loss_host as HL
from test_stream_ops_host import f64, measured, same_bits, worst_ratio  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = -7777.25
GUARD = 64
EINVAL = -1                         # include/scflow_hip.h
SIGMOID, TANH = 2, 3
cpu = lambda t: t.detach().cpu()                                    # noqa: E731
KEYS = ('g', 'g_rh', 'h', 'z', 'r', 'q')


def D(t):
    return None if t is None else t.to(DEV).contiguous()


def sliced(t, before, after):
    """t (M, C, H, W) as a channel slice of a wider GPU tensor whose other channels hold the sentinel -> (wide, view)"""
    m, c, h, w = t.shape
    wide_ = torch.full((m, before + c + after, h, w), SENTINEL, dtype=torch.float32, device=DEV)
    wide_[:, before:before + c] = t.to(DEV)
    return wide_, wide_[:, before:before + c]


def slice_untouched(wide_, c, before):
    rest = torch.cat([wide_[:, :before], wide_[:, before + c:]], 1)
    return bool((rest == SENTINEL).all())


# ==================================================================================================== the gate kernels
# (C, H, W, slices as (before, after) or None): 33 * 5 * 7 = 1155 floats a row at a stride of 38 * 35 -- the scalar
# instantiation; 32 * 4 * 8 contiguous -- the 16-byte instantiation; 33 * 2 * 3 = 198 floats a row (no multiple of 4) in a
# 38-channel tensor from channel 4 on (stride 228, offset 96 bytes) -- the 16-byte instantiation with a scalar last quad
GATE_SHAPES = [(33, 5, 7, (3, 2)), (32, 4, 8, None), (33, 2, 3, (4, 1))]


def _run_gates(d, sl, sums=None, first=True):
    """both kernels on the case ``d`` -> dict u_q, u_z, u_r, g_h_direct (GPU tensors); operands and outputs as channel
    slices of sentinel-filled tensors when ``sl``; the u_z / u_r halves of one [u_z | u_r] tensor always"""
    m, c, h, w = d['g'].shape
    wides = {}

    def operand(k, t):
        if sl is None:
            return D(t)
        wides[k], v = sliced(t, *sl)
        return v

    o = {k: operand(k, d[k]) for k in KEYS}
    u_q = operand('u_q', torch.full((m, c, h, w), SENTINEL))
    u_zr = torch.full((m, 2 * c, h, w), SENTINEL, device=DEV)
    s_q, s_zr = (None, None) if sums is None else sums
    ops.gru_gate_grad_q(o['g'], o['h'], o['z'], o['q'], u_q=u_q, u_z=u_zr[:, :c], sum_q=s_q,
                        sum_z=None if s_zr is None else s_zr[:, :c], first=first)
    assert bool((u_zr[:, c:] == SENTINEL).all()), 'grad_q wrote the u_r rows'
    ur, gh = ops.gru_gate_grad_r(o['g'], o['z'], o['g_rh'], o['h'], o['r'], u_r=u_zr[:, c:],
                                 sum_r=None if s_zr is None else s_zr[:, c:], first=first)
    assert gh.data_ptr() == o['g_rh'].data_ptr(), 'g_h_direct is written in place over g_rh'
    for k in ('g', 'h', 'z', 'r', 'q'):                                # inputs unchanged, their surroundings untouched
        assert same_bits(o[k], D(d[k])), k
    for k, wd in wides.items():
        assert slice_untouched(wd, c, sl[0]), k
    return dict(u_q=u_q, u_z=u_zr[:, :c], u_r=u_zr[:, c:], g_h_direct=o['g_rh'])


@pytest.mark.parametrize('shape', GATE_SHAPES, ids=lambda s: f'{s[0]}x{s[1]}x{s[2]}' + ('' if s[3] is None else '-sliced'))
@pytest.mark.parametrize('m', [1, 3])
@pytest.mark.parametrize('regime', GH.GATE_REGIMES)
def test_gate_kernels_against_float64(regime, m, shape):
    c, h, w, sl = shape
    d = GH.gate_case(regime, m, c, h, w)
    ref = GH.gate_refs(d)
    got = _run_gates(d, sl)
    worst = max(worst_ratio(cpu(got[k]), ref[k].v, ref[k].b) for k in ref)
    measured(f'gate kernels {regime} M {m} {shape[:3]}, worst error / bound', worst)
    assert worst <= 1.0
    # the CPU evaluation in the stated order gives the same bits: the order IS the stated one
    emu = GH.gate_fp32(d)
    assert all(torch.equal(cpu(got[k]), emu[k]) for k in emu)
    if regime == 'zero_cotangent':
        assert all(not torch.signbit(cpu(v)).any() and not cpu(v).any() for v in got.values()), 'not +0 everywhere'
    if regime == 'h_equals_q':
        assert not cpu(got['u_z']).any()
    again = _run_gates(d, sl)
    assert all(same_bits(got[k], again[k]) for k in got), 'two runs differ'
    # the factors shared with the activation backward, bit for bit
    g, g_rh, hh, z, r, q = (D(d[k]) for k in KEYS)
    assert torch.equal(got['u_q'], ops.act_grad(g * z, q, TANH))
    assert torch.equal(got['u_z'], ops.act_grad(g * (q - hh), z, SIGMOID))
    assert torch.equal(got['u_r'], ops.act_grad(g_rh * hh, r, SIGMOID))
    if m == 3:                                              # a sample's result is the same alone and inside the batch
        one = _run_gates({k: v[1:2] for k, v in d.items()}, sl)
        assert all(same_bits(one[k], got[k][1:2]) for k in got)


@pytest.mark.parametrize('shape', GATE_SHAPES, ids=lambda s: f'{s[0]}x{s[1]}x{s[2]}')
def test_gate_kernels_keep_nan_and_inf_in_their_sample(shape):
    c, h, w, sl = shape
    d = GH.gate_case('nominal', 3, c, h, w)
    clean = _run_gates(d, sl)
    bad = {k: v.clone() for k, v in d.items()}
    bad['g'][1, 0, 0, 0], bad['g'][1, 1, 0, 1], bad['g_rh'][1, 2, 1, 0], bad['q'][1, 3, 1, 1] = float('nan'), float('inf'), float('-inf'), float('nan')
    got = _run_gates(bad, sl)
    for k in got:
        assert same_bits(got[k][0], clean[k][0]) and same_bits(got[k][2], clean[k][2]), k
    assert not torch.isfinite(got['u_q'][1, 0, 0, 0]) and not torch.isfinite(got['u_q'][1, 1, 0, 1])
    assert not torch.isfinite(got['u_r'][1, 2, 1, 0]) and not torch.isfinite(got['u_z'][1, 3, 1, 1])
    assert int((~torch.isfinite(got['u_q'][1])).sum()) == 3 and int((~torch.isfinite(got['g_h_direct'][1])).sum()) == 3


@pytest.mark.parametrize('shape', GATE_SHAPES, ids=lambda s: f'{s[0]}x{s[1]}x{s[2]}')
def test_gate_kernels_running_sums(shape):
    c, h, w, sl = shape
    a, b = GH.gate_case('nominal', 3, c, h, w), GH.gate_case('decades', 3, c, h, w, seed=1)
    wq, s_q = sliced(torch.full((3, c, h, w), SENTINEL), 4, 4)
    s_zr = torch.full((3, 2 * c, h, w), SENTINEL, device=DEV)
    ua = _run_gates(a, sl, (s_q, s_zr), first=True)                  # first call: the sum IS u, whatever it held
    assert same_bits(s_q, ua['u_q']) and same_bits(s_zr, torch.cat([ua['u_z'], ua['u_r']], 1))
    ub = _run_gates(b, sl, (s_q, s_zr), first=False)                 # then sum = sum + u, one fp32 addition
    assert same_bits(s_q, ua['u_q'] + ub['u_q']) and same_bits(s_zr, torch.cat([ua['u_z'] + ub['u_z'], ua['u_r'] + ub['u_r']], 1))
    assert slice_untouched(wq, c, 4)


def test_carry_and_state_kernels():
    for c, h, w, sl in GATE_SHAPES:
        d = GH.gate_case('nominal', 3, c, h, w)
        wide_, src = sliced(d['g'], 4, 4)
        out = ops.gru_carry(src, D(d['g_rh']))
        assert same_bits(out, D(d['g']) + D(d['g_rh'])) and same_bits(src, D(d['g']))
        out = ops.gru_carry(src, clear=True)
        assert same_bits(out, D(d['g'])) and not src.any() and not torch.signbit(src).any() and slice_untouched(wide_, c, 4)
        hh, z, q, r = (D(d[k]) for k in ('h', 'z', 'q', 'r'))
        assert same_bits(ops.gru_gate_state(hh, r), r * hh)
        assert torch.equal(cpu(ops.gru_gate_state(hh, z, q)), GH.fma(cpu(z), cpu(q), (1.0 - cpu(z)) * cpu(hh)))


def test_c_abi_rejections_leave_the_outputs_unwritten():
    lib = _lib.load()
    m, n = 2, 40
    buf = lambda: torch.full((m, n), SENTINEL, device=DEV)          # noqa: E731
    g, h, z, q, grh, r = (torch.rand((m, n), device=DEV) for _ in range(6))
    u_q, u_z, u_r, s_ = buf(), buf(), buf(), buf()
    P = lambda t: t.data_ptr()                                       # noqa: E731
    ok_q = [P(g), n, P(h), n, P(z), n, P(q), n, P(u_q), n, P(u_z), n, P(s_), n, None, 0, 1, m, n, None]
    ok_r = [P(g), n, P(z), n, P(grh), n, P(h), n, P(r), n, P(u_r), n, P(s_), n, 1, m, n, None]
    before = grh.clone()
    for fn, ok, ptrs, m_at in ((lib.scf_gru_gate_grad_q, ok_q, (0, 2, 4, 6, 8, 10), 17), (lib.scf_gru_gate_grad_r, ok_r, (0, 2, 4, 6, 8, 10), 15)):
        for i in ptrs:
            for at, v in ((i, None), (i + 1, n - 1)):
                bad = list(ok)
                bad[at] = v
                assert fn(*bad) == EINVAL, (fn.__name__, at)
        for at, v in ((m_at, 0), (m_at + 1, 0), (m_at + 1, -3), (13, n - 1)):
            bad = list(ok)
            bad[at] = v
            assert fn(*bad) == EINVAL, (fn.__name__, at)
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in (u_q, u_z, u_r, s_)) and same_bits(grh, before)
    d = GH.gate_case('nominal', 2, 4, 2, 5)
    with pytest.raises(ScflowHipError):
        ops.gru_gate_grad_q(D(d['g']), D(d['h']), D(d['z'])[:, :3], D(d['q']))
    with pytest.raises(ScflowHipError):
        ops.gru_gate_grad_r(D(d['g']), D(d['z']), D(d['g_rh']).permute(0, 1, 3, 2), D(d['h']), D(d['r']))
    with pytest.raises(ScflowHipError):
        ops.gru_gate_grad_q(d['g'], d['h'], d['z'], d['q'])           # CPU tensors


# ================================================================================================== ConvGRU.backward
HC = CC = CX = 128


def _gru(net, seed=0, params=None):
    gru = ConvGRU(HC, CC + CX, net)
    gen = torch.Generator().manual_seed(700 + seed)
    with torch.no_grad():
        for name, prm in gru.named_parameters():
            if params is not None:
                prm.copy_(params[name])
            else:
                fan = prm[0].numel() if prm.dim() > 1 else 1
                prm.copy_(torch.randn(prm.shape, generator=gen) * (2.0 * fan ** -0.5 if prm.dim() > 1 else 0.1))
    return gru.to(DEV)


def _forward(gru, h0, c, x):
    """the decoder's use of the GRU: one buffer [h | c | x'], the context hoisted, h updated in place -> saved"""
    T, n = x.shape[:2]
    hx = torch.cat([h0, c, x[0]], 1).contiguous()
    ctx = gru.context_terms(hx[:, HC:HC + CC])
    hv = torch.empty((T, n, HC) + tuple(h0.shape[2:]), device=DEV)
    for t in range(T):
        ops.copy_channels(x[t], hx[:, HC + CC:])
        hv[t].copy_(gru.forward_inplace(hx, ctx, CC))
    return dict(h0=h0.contiguous(), c=c.contiguous(), x=x.contiguous(), hv=hv)


def _case(net, T, hw, seed=0, n=2):
    gen = torch.Generator().manual_seed(800 + seed + T + 3 * hw[0] + 5 * hw[1])
    R = lambda *s: torch.randn(s, generator=gen)                     # noqa: E731
    gru = _gru(net, seed)
    saved = _forward(gru, D(torch.tanh(R(n, HC, *hw))), D(torch.relu(R(n, CC, *hw))), D(R(T, n, CX, *hw)))
    return gru, saved, [D(R(n, HC, *hw)) for _ in range(T)]


def _weights(gru):
    return [{g: cpu(getattr(gru, f'conv_{g}')[i].conv.weight) for g in 'zrq'} for i in range(len(gru.conv_z))]


def _check(gru, net, saved, gates, g_hs, got, prev=None):
    """worst error / composed bound per result against the float64 scan GIVEN the GPU's own recomputed gates"""
    gcpu = {k: [cpu(v) for v in gates[k]] for k in ('h_in', 'zr', 'rh', 'q')}
    ref = GH.gru_scan(GH.B64(), gcpu, _weights(gru), cpu(saved['c']), cpu(saved['x']), [cpu(g) for g in g_hs], prev=prev)
    g_h0, g_c, g_x, grads = got
    have = dict(g_h0=g_h0, g_c=g_c, **{f'g_x.{t}': v for t, v in enumerate(g_x)}, **{k: grads[k] for k in GH.param_names(net)})
    assert set(have) == set(ref)
    return {k: worst_ratio(cpu(have[k]), ref[k].v, ref[k].b) for k in ref}


def _check_launches(gru, net, saved, g_hs, got, im, prev=None):
    """The scan launch by launch: every launch against float64 GIVEN the GPU's own operands of that launch (no bound is
    carried from launch to launch, so none is amplified by the convolutions behind it), and every hand-over between
    launches bit for bit -> worst error / bound per kind of launch.  Together with the hand-overs this pins every output."""
    be, P, T = GH.B64(), len(gru.conv_z), len(g_hs)
    Vx = lambda t: GH.V(cpu(t))                                       # noqa: E731
    gates, u_zr, u_q = im['gates'], im['u_zr'], im['u_q']
    wts = _weights(gru)
    w_zr, w_q = [torch.cat([wp['z'], wp['r']], 0) for wp in wts], [wp['q'] for wp in wts]
    hx_cols = lambda wt: f64(torch.cat([wt[:, :HC], wt[:, HC + CC:]], 1))      # noqa: E731
    worst = {}

    def hold(kind, have, ref):
        worst[kind] = max(worst.get(kind, 0.0), worst_ratio(cpu(have), ref.v, ref.b))

    for t in reversed(range(T)):
        for p in reversed(range(P)):
            g, g_q, add, out = (im[k][(p, t)] for k in ('g', 'g_q', 'add', 'out'))
            if p == P - 1:
                assert same_bits(g, g_hs[t] if t == T - 1 else im['out'][(0, t + 1)][:, :HC] + g_hs[t]), 'the carried cotangent'
            else:
                assert same_bits(g, im['out'][(p + 1, t)][:, :HC]), 'the hand-over between the passes'
            h_in, z, r, q = (cpu(v) for v in (gates['h_in'][p][t], gates['zr'][p][t][:, :HC], gates['zr'][p][t][:, HC:], gates['q'][p][t]))
            uq, uz = be.gate_q(Vx(g), h_in, z, q)
            hold('gate_q', u_q[p][t], uq)
            hold('gate_q', u_zr[p][t][:, :HC], uz)
            prior = None if p == P - 1 else torch.cat([torch.zeros_like(g), im['out'][(p + 1, t)][:, HC:]], 1)
            hold('dgrad_q', g_q, be.dgrad(Vx(u_q[p][t]), hx_cols(w_q[p]), None if prior is None else Vx(prior)))
            ur, ghd = be.gate_r(Vx(g), z, Vx(g_q[:, :HC]), h_in, r)
            hold('gate_r', u_zr[p][t][:, HC:], ur)
            hold('gate_r', add[:, :HC], ghd)
            assert same_bits(add[:, HC:], g_q[:, HC:])
            hold('dgrad_zr', out, be.dgrad(Vx(u_zr[p][t]), hx_cols(w_zr[p]), Vx(add)))
    for p in range(P):                                                # the running sums: one fp32 addition a call, the scan's order
        for s_, u in ((im['s_zr'][p], u_zr[p]), (im['s_q'][p], u_q[p])):
            tot = u[T - 1]
            for t in reversed(range(T - 1)):
                tot = tot + u[t]
            assert same_bits(s_, tot), 'a running sum'
    g_h0, g_c, g_x, grads = got
    assert same_bits(g_h0, im['out'][(0, 0)][:, :HC]) and all(same_bits(g_x[t], im['out'][(0, t)][:, HC:]) for t in range(T))
    ref = None
    for p in range(P):                                                # the context columns: a chain through `add` alone
        ref = be.dgrad(Vx(im['s_zr'][p]), f64(w_zr[p][:, HC:HC + CC]), ref)
        ref = be.dgrad(Vx(im['s_q'][p]), f64(w_q[p][:, HC:HC + CC]), ref)
    hold('dgrad_c', g_c, ref)
    xs, cl = Vx(saved['x'].flatten(0, 1)), Vx(saved['c'])
    for p in range(P):
        k = tuple(w_q[p].shape[2:])
        for u, s_, state, mods in ((u_zr[p], im['s_zr'][p], gates['h_in'][p], 'zr'), (u_q[p], im['s_q'][p], gates['rh'][p], 'q')):
            names = [f'conv_{m_}.{p}.conv' for m_ in mods]
            pw = None if prev is None else torch.cat([prev[f'{n_}.weight'] for n_ in names], 0)
            pb = None if prev is None else torch.cat([prev[f'{n_}.bias'] for n_ in names], 0)
            have_w = torch.cat([cpu(grads[f'{n_}.weight']) for n_ in names], 0)
            have_b = torch.cat([cpu(grads[f'{n_}.bias']) for n_ in names], 0)
            for kind, uu, xx, cols, bias in (('wgrad_h', u.flatten(0, 1), Vx(state.flatten(0, 1)), slice(0, HC), True),
                                             ('wgrad_c', s_, cl, slice(HC, HC + CC), False), ('wgrad_x', u.flatten(0, 1), xs, slice(HC + CC, None), False)):
                dw, db = be.wgrad(Vx(uu), xx, k, None if pw is None else pw[:, cols], pb if bias else None)
                hold(kind, have_w[:, cols], dw)
                if bias:
                    hold('bias', have_b, db)
    return worst


def _forward_bound(gru, saved, gates, t):
    """worst |h - h64| / gru_bound (tests/test_gru_host.py, the forward's gate bound at the largest route budget, with the
    hoisted context term) of the recomputed and of the kept state of iteration t, from the kept input state"""
    passes = []
    for i in range(len(gru.conv_z)):
        blk = {g: getattr(gru, f'conv_{g}')[i].conv for g in 'zrq'}
        p = {'pad': tuple(blk['z'].padding)}
        for g in 'zrq':
            p['w' + g], p['b' + g] = blk[g].weight.detach().double(), blk[g].bias.detach().double()
        passes.append(p)
    hx = torch.cat([gates['h_in'][0][t], saved['c'], saved['x'][t]], 1).double()
    ref = GF.gru_reference(hx, passes, HC)
    c64 = saved['c'].double()
    cterm = [torch.cat([GF.conv_taps(c64, p['w' + g][:, HC:HC + CC], p['b' + g], p['pad']) for g in 'zrq'], 1) for p in passes]
    bound = GF.gru_bound(ref, passes, HC, max(GF.BUDGET.values()), cterm=cterm)
    return GF.bound_ratio(gates['h_out'][t], ref, bound)[0], GF.bound_ratio(saved['hv'][t], ref, bound)[0]


@pytest.mark.parametrize('net', GH.NETS)
@pytest.mark.parametrize('T', [1, 3])
@pytest.mark.parametrize('hw', [(8, 8), (5, 7), (12, 20)], ids=lambda v: f'{v[0]}x{v[1]}')
def test_gru_backward_against_float64_given_the_gates(hw, T, net):
    gru, saved, g_hs = _case(net, T, hw)
    n = 2
    gates = gru.recompute_gates(saved)
    again = gru.recompute_gates(saved)
    assert all(same_bits(a, b) for k in ('h_in', 'zr', 'rh', 'q') for a, b in zip(gates[k], again[k]))
    for t in range(T):                                              # the recomputed state against the kept one
        r_new, r_kept = _forward_bound(gru, saved, gates, t)
        ulps = float(((gates['h_out'][t] - saved['hv'][t]).abs() / GF.ulp32(saved['hv'][t].double()).float().clamp(min=2.0 ** -24)).max())
        measured(f'recomputed h_out {net} {hw} t {t}: error / forward bound {r_new:.3g} (kept hv {r_kept:.3g}), |h_out - hv| in ulps', ulps)
        measured(f'recomputed h_out {net} {hw} t {t}: max |h_out - hv|', float((gates['h_out'][t] - saved['hv'][t]).abs().max()))
        assert r_new <= 1.0 and r_kept <= 1.0
    got = gru.backward(saved, g_hs)
    g_h0, g_c, g_x, grads = got
    assert sorted(grads) == sorted(GH.param_names(net)) and len(g_x) == T
    assert g_h0.shape == (n, HC, *hw) and g_c.shape == (n, CC, *hw) and all(v.shape == (n, CX, *hw) for v in g_x)
    again = gru.backward(saved, g_hs)
    assert same_bits(g_h0, again[0]) and same_bits(g_c, again[1]) and all(same_bits(a, b) for a, b in zip(g_x, again[2]))
    assert all(same_bits(grads[k], again[3][k]) for k in grads), 'two runs differ'
    for key, v in _check(gru, net, saved, gates, g_hs, got).items():
        measured(f'ConvGRU.backward {net} {hw} T {T} {key}, error / composed bound', v)
        assert v <= 1.0, key
    # launch by launch, each given the GPU's own operands: the sharp form of the same statement
    im = {}
    seen = gru.backward(saved, g_hs, intermediates=im)
    assert same_bits(seen[0], g_h0) and same_bits(seen[1], g_c) and all(same_bits(seen[3][k], grads[k]) for k in grads)
    assert all(same_bits(a, b) for k in ('h_in', 'zr', 'rh', 'q') for a, b in zip(gates[k], im['gates'][k]))
    for kind, v in _check_launches(gru, net, saved, g_hs, seen, im).items():
        measured(f'ConvGRU.backward {net} {hw} T {T} launches of kind {kind}, error / bound', v)
        assert v <= 1.0, kind
    # accumulating into a dict passed in: previous + sum
    gen = torch.Generator().manual_seed(5)
    prev = {k: D(torch.randn(v.shape, generator=gen)) for k, v in grads.items()}
    into = {k: v.clone() for k, v in prev.items()}
    into['other'] = prev['conv_q.0.conv.bias']
    im = {}
    acc = gru.backward(saved, g_hs, param_grads=into, intermediates=im)
    assert acc[3] is into and set(into) == set(grads) | {'other'}
    assert all(same_bits(into[k], grads[k] + prev[k]) for k in grads)
    for key, v in _check(gru, net, saved, gates, g_hs, acc, prev={k: cpu(v) for k, v in prev.items()}).items():
        assert v <= 1.0, key
    for kind, v in _check_launches(gru, net, saved, g_hs, acc, im, prev={k: cpu(v) for k, v in prev.items()}).items():
        assert v <= 1.0, kind
    if T == 3:
        # iteration 2 of this call, whose carried cotangent is g_hs[2] itself, is a T = 1 call: the result does not depend on T
        one = gru.backward(dict(h0=saved['hv'][1].contiguous(), c=saved['c'], x=saved['x'][2:3].contiguous(), hv=saved['hv'][2:3].contiguous()),
                           g_hs[2:3])
        assert same_bits(one[2][0], g_x[2])
        name = GH.param_names(net)[0]
        with pytest.raises(ScflowHipError):
            gru.backward(saved, g_hs, param_grads={name: prev[name]})
        with pytest.raises(ScflowHipError):
            gru.backward(saved, [])
        with pytest.raises(ScflowHipError):
            gru.backward(saved, g_hs[:2])
        with pytest.raises(ScflowHipError):
            gru.backward({k: v for k, v in saved.items() if k != 'x'}, g_hs)
        with pytest.raises(ScflowHipError):
            gru.backward(dict(saved, c=saved['c'][:, :64]), g_hs)
        with pytest.raises(ScflowHipError):
            gru.backward(dict(saved, hv=saved['hv'].transpose(3, 4)), g_hs)


def test_gru_backward_refuses_more_iterations_than_the_tail():
    gru = _gru('Conv')
    T = ops.TAIL_MAX_T + 1
    z = lambda *s: torch.zeros(s, device=DEV)                        # noqa: E731
    saved = dict(h0=z(1, HC, 2, 2), c=z(1, CC, 2, 2), x=z(T, 1, CX, 2, 2), hv=z(T, 1, HC, 2, 2))
    with pytest.raises(ScflowHipError):
        gru.backward(saved, [z(1, HC, 2, 2)] * T)
    saved = {k: (v[:T - 1] if v.dim() == 5 else v) for k, v in saved.items()}
    assert len(gru.backward(saved, [z(1, HC, 2, 2)] * (T - 1))[2]) == T - 1       # the limit itself is accepted


# ======================================================================================== the reference's own ConvGRU
@pytest.mark.parametrize('net', GH.NETS)
@pytest.mark.parametrize('hw', GH.GOLDEN_MAPS, ids=lambda v: f'{v[0]}x{v[1]}')
def test_kernels_against_the_reference_fixture(net, hw):
    """ConvGRU.backward on the fixture's seeds against the reference's recorded autograd.  Both are fp32 evaluations around
    the float64 scan of tests/test_gru_grad_host.py::golden_reference, each inside its room, so they are at most two rooms
    apart (the GPU's gates come from its hardware-unit sigmoid / tanh, the fixture's from libm: the rooms are taken around
    the scan given each side's own gates); the kernels' own, tighter bounds are held by the tests above."""
    z = np.load(GH.GOLDEN)
    tag, p, h0, c, x, cots = GH.golden_case(net, hw)
    gru = _gru(net, params=p)
    saved = _forward(gru, D(h0), D(c), D(x))
    gates = gru.recompute_gates(saved)
    g_h0, g_c, g_x, grads = gru.backward(saved, [D(v) for v in cots])
    got = dict(g_h0=g_h0, g_c=g_c, **{f'g_x.{t}': v for t, v in enumerate(g_x)}, **grads)
    _, ref_gpu, room_gpu = GH.golden_reference(net, hw, {k: [cpu(v) for v in gates[k]] for k in ('h_in', 'zr', 'rh', 'q')})
    _, ref_cpu, room_cpu = GH.golden_reference(net, hw)
    for key in GH.golden_keys(net):
        pick = lambda v: GH.golden_pick(key, v)                      # noqa: E731
        v = worst_ratio(pick(cpu(got[key]).numpy()), pick(ref_gpu[key]), pick(room_gpu[key]))
        measured(f'kernels on the fixture\'s inputs {tag} {key}, error / room given the GPU\'s gates', v)
        assert v <= 1.0, key
        # the two float64 scans differ by what the gates differ; the recorded values against the GPU's through both
        gap = np.abs(pick(ref_gpu[key]) - pick(ref_cpu[key]))
        v = worst_ratio(pick(cpu(got[key]).numpy()), z[f'{tag}.{key}'], pick(room_gpu[key]) + pick(room_cpu[key]) + gap)
        measured(f'kernels - reference fixture {tag} {key}, difference / (two rooms + the gates\' gap)', v)
        assert v <= 1.0, key
        rel = float(np.abs(pick(cpu(got[key]).numpy()) - z[f'{tag}.{key}']).max() / np.abs(z[f'{tag}.{key}']).max())
        measured(f'kernels - reference fixture {tag} {key}, relative to the largest entry', rel)
        assert rel <= 1e-4, key          # gates 3e-7 apart (A_SIG / A_TANH of tests/test_gru_host.py) through <= 4 passes


# ================================================================================================= the refiner's entry
@pytest.fixture(scope='module')
def scflow_model(golden_dir):
    """the small random-weight refiner of tests/test_gpu_head_grad.py (64 x 64, two iterations)"""
    case = HL.refiner_loss_case()
    cfg = scflow_amd.scflow_model_cfg(iters=HL.REFINER_ITERS)
    cfg.update(HL.refiner_loss_cfgs(case))
    cfg['pose_loss_cfg'] = dict(type='SequenceLoss', gamma=0.7, loss_func_cfg=dict(type='RAFTLoss', loss_weight=0.3, max_flow=400.))
    m = scflow_amd.build_refiner(cfg)
    shapes = json.load(open(os.path.join(golden_dir, 'state_dict_keys.json')))['shapes']
    m.load_state_dict(scflow_amd.fill_state_dict(shapes, seed=0), strict=True)
    return m.to(DEV), case


def test_loss_and_gru_grads(scflow_model):
    m, case = scflow_model
    data = HL.refiner_data(case, DEV)
    base = m.loss_and_decoder_head_grads(None, data=data)
    loss, log_imgs, log_vars, seq_r, seq_t, grads = m.loss_and_gru_grads(None, data=data)
    assert same_bits(loss, base[0]) and list(log_vars.items()) == list(base[2].items()) and log_imgs is None
    assert sorted(grads) == sorted(list(base[5]) + ['gru'])
    dec = m.decoder
    gru_names = {'decoder.gru.' + k for k in dict(dec.gru.named_parameters())}
    assert set(grads['params']) == set(base[5]['params']) | gru_names and len(gru_names) == 12

    def same(a, b):
        if isinstance(a, dict):
            return sorted(a) == sorted(b) and all(same(a[k], b[k]) for k in a)
        if isinstance(a, (list, tuple)):
            return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
        return same_bits(a, b)
    for key, v in base[5].items():
        assert same({k: grads[key][k] for k in v} if key == 'params' else grads[key], v), key
    assert dec.keep == 'none'
    g = grads['gru']
    assert sorted(g) == ['context', 'initial_hidden', 'motion_features'] and len(g['motion_features']) == dec.iters
    saved = dec.kept
    assert sorted(saved) == ['c', 'd_flow', 'dm', 'h0', 'hv', 'mask', 'tail_inputs', 'x', 'y0', 'y1', 'y2']
    gates = dec.gru.recompute_gates(saved)
    got = (g['initial_hidden'], g['context'], g['motion_features'], {k: grads['params']['decoder.gru.' + k] for k in GH.param_names('SeqConv')})
    for key, v in _check(dec.gru, 'SeqConv', saved, gates, grads['decoder_heads']['hidden_states'], got).items():
        measured(f'loss_and_gru_grads {key}, error / composed bound', v)
        assert v <= 1.0, key
    for t in range(dec.iters):
        r_new, r_kept = _forward_bound(dec.gru, saved, gates, t)
        assert r_new <= 1.0 and r_kept <= 1.0
    with pytest.raises(ScflowHipError):
        dec.gru_backward({k: v for k, v in saved.items() if k != 'c'}, grads['decoder_heads']['hidden_states'])
    with pytest.raises(NotImplementedError, match='loss_and_gru_grads'):
        m.forward(data, return_loss=True)


def test_keeping_the_gru_inputs_changes_no_bit(scflow_model):
    m, case = scflow_model
    data = HL.refiner_data(case, DEV)
    dec = m.decoder
    get = lambda: m.get_pose(data['rendered_images'], data['real_images'], data['ref_rotations'], data['ref_translations'],   # noqa: E731
                             data['rendered_depths'], data['internel_k'], data['labels'])
    old = dec.c_iteration
    kept, tails = {}, {}
    try:
        for c_iteration in (True, False):
            dec.c_iteration = c_iteration
            dec.kept = {}
            off = get()
            assert dec.kept == {}
            dec.keep = 'gru'
            on = get()
            dec.keep = 'none'
            assert sorted(dec.kept) == ['c', 'd_flow', 'dm', 'h0', 'hv', 'mask', 'tail_inputs', 'x', 'y0', 'y1', 'y2']
            kept[c_iteration] = {k: v.clone() for k, v in dec.kept.items() if k != 'tail_inputs'}
            tails[c_iteration] = [t.clone() for t in dec.kept['tail_inputs']]
            for a, b in zip(off, on):
                assert all(same_bits(x, y) for x, y in zip(a, b)), f'c_iteration {c_iteration}'
    finally:
        dec.keep, dec.c_iteration = 'none', old
    sc, sp = kept[True], kept[False]
    assert sorted(sc) == sorted(sp) == ['c', 'd_flow', 'dm', 'h0', 'hv', 'mask', 'x', 'y0', 'y1', 'y2']
    n, (h, w) = sc['hv'].shape[1], sc['hv'].shape[3:]
    assert sc['h0'].shape == (n, 128, h, w) and sc['c'].shape == (n, 128, h, w) and sc['x'].shape == (dec.iters, n, 128, h, w)
    assert all(v.is_contiguous() for v in sc.values())
    assert all(same_bits(sc[k], sp[k]) for k in sc), 'the two loop forms keep different tensors'
    assert len(tails[True]) == len(tails[False]) == dec.iters and all(same_bits(a, b) for a, b in zip(tails[True], tails[False]))
    assert not same_bits(sc['x'][0], sc['x'][1]) and not same_bits(sc['h0'], sc['hv'][0])
    # the kept tensors are the forward's own: the GRU run again from them gives the kept states
    again = _forward(dec.gru, sc['h0'], sc['c'], sc['x'])
    assert same_bits(again['hv'], sc['hv'])
