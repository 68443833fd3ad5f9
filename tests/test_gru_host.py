"""CPU: the ConvGRU cell (decoder/raft_decoder.py:235-253) restated in torch float64, an elementwise error bound for
any fp32 evaluation of it, the regimes a trained cell lives in, and the checks that tests/test_gpu_gru.py applies to
the HIP gate epilogues -- shown here to accept a plain fp32 torch cell and to reject subtly wrong ones.

Per pass (SeqConv: a 1x5 pass, then a 5x1 pass; Conv: one 3x3 pass), on hx = [h | x]:

    z = sigmoid(conv_z[h | x])        r = sigmoid(conv_r[h | x])
    q = tanh(conv_q[r h | x])         h' = (1 - z) h + z q

Two nets of different mesh:

* ``gru_bound``: a first-order (mean-value, with the second-order cross terms kept) bound on |h_fp32 - h_fp64|
  for an evaluation whose convolutions err by <= B eps sum|w||x| (B: the budgets tests/test_gpu_ops.py asserts per
  kernel family), whose activations err by A_SIG / A_TANH absolutely and whose products / blend round once per
  operation.  It grows with sum|w||x|, so it is a gross-error net: it must hold in every regime, but an epilogue that
  is wrong by 1e-5 stays inside it (test_bound_alone_misses_the_small_sigmoid_mutant).
* ``epilogue_expected`` / ``epilogue_tol``: one fused epilogue given ITS OWN fp32 pre-activation.  The convolution's
  rounding is out of the comparison, the tolerance is ~1e-7 in every regime, and an operand taken from the wrong
  pixel or a constant that is off in the sixth digit shows.
"""
import math

import pytest
import torch
import torch.nn.functional as F

EPS = 2.0 ** -24
A_SIG, A_TANH = 3e-7, 1.5e-7          # absolute activation errors claimed next to scf_fast_sigmoid / scf_fast_tanh
# budgets in units of eps sum|w||x| that tests/test_gpu_ops.py asserts per kernel family (_winograd_stress)
BUDGET = {'direct': 24.0, 'F(2,5)': 60.0, 'F(4,5)': 60.0, 'F(2x2,3x3)': 12.0}
REGIMES = ['nominal', 'saturated', 'keep', 'replace', 'cancelling', 'h_edge']
_KERNEL = {'Conv': [((3, 3), (1, 1))], 'SeqConv': [((1, 5), (0, 2)), ((5, 1), (2, 0))]}


def _rnd(shape, g, scale=1.0):
    return torch.randn(shape, generator=g) * scale


def conv_taps(x, w, b, padding):
    """the float64 paths' convolution: F.conv2d on the CPU; on a device, whose convolution library may have no float64
    kernels, one channel contraction per tap (einsum -> GEMM) of a 'same' stride-1 convolution"""
    if not x.is_cuda:
        return F.conv2d(x, w, b, padding=padding)
    n, c, hh, ww = x.shape
    kh, kw = w.shape[2:]
    xp = F.pad(x, (padding[1], padding[1], padding[0], padding[0]))
    out = None
    for ky in range(kh):
        for kx in range(kw):
            t = torch.einsum('oc,nchw->nohw', w[:, :, ky, kx], xp[:, :, ky:ky + hh, kx:kx + ww])
            out = t if out is None else out + t
    return out if b is None else out + b.view(1, -1, 1, 1)


# ------------------------------------------------------------------------------------------------ regimes
def bias_bands(hc, rot):
    """(first channel, last channel + 1, value) of the saturated regime's 16-channel bias bands of ONE gate: bands at
    24 + 32 k straddle the 32-channel fragment boundaries, the halves at both ends of the gate make one band across
    the Cout / 2 boundary of the stacked z | r bias.  ``rot`` rotates the values so that every gate and pass sees
    each of them somewhere."""
    vals = [100.0, -100.0, 30.0, -30.0]
    out, k = [], 0
    while 24 + 32 * k + 16 <= hc - 8:
        out.append((24 + 32 * k, 40 + 32 * k, vals[(k + rot) % 4]))
        k += 1
    out += [(0, 8, vals[(k + rot) % 4]), (hc - 8, hc, vals[(k + rot) % 4])]
    return out


def gru_case(regime, n, h, w, kind='SeqConv', seed=0, hc=128, cc=128, xc=128):
    """inputs of one ConvGRU: ``hx`` = [h | c | x'] (fp32), per pass the six parameter tensors over all hc + cc + xc
    input channels, and the sizes.  ``gru_motion(case, it)`` draws the x' of a later iteration by the same recipe."""
    assert regime in REGIMES, regime
    g = torch.Generator().manual_seed(1000 * REGIMES.index(regime) + seed)
    cin = hc + cc + xc
    hx = _rnd((n, cin, h, w), g)
    hx[:, :hc] = torch.tanh(hx[:, :hc])
    if regime == 'cancelling':                  # post-ReLU features on a DC offset: every product has one sign per weight
        hx[:, hc:] = hx[:, hc:].abs() + 20.0
    if regime == 'h_edge':                      # exactly +-1, +-0, denormals, the smallest denormal: one value per pixel column
        edge = torch.tensor([1.0, -1.0, 0.0, -0.0, 1e-40, -1e-40, 1.4e-45, -1.4e-45])
        idx = (torch.arange(h * w).reshape(h, w) + torch.arange(hc).reshape(hc, 1, 1)) % 11
        hv = hx[:, :hc]
        for k in range(8):
            hv[:] = torch.where(idx == k, edge[k], hv)
    passes = []
    for i, (k, pad) in enumerate(_KERNEL[kind]):
        fan = cin * k[0] * k[1]
        p = {'pad': pad}
        for j, gate in enumerate('zrq'):
            if regime == 'cancelling':          # magnitudes log-uniform over three decades (the wide_weights stress recipe)
                wt = _rnd((hc, cin, *k), g, (1.0 / fan) ** 0.5)
                wt = wt * torch.pow(10.0, torch.rand((hc, cin, *k), generator=g) * 3.0 - 1.5)
            else:
                wt = _rnd((hc, cin, *k), g, 1.5 * (1.6 / fan) ** 0.5)
            b = _rnd((hc,), g, 0.1)
            if regime == 'saturated':
                wt = wt * 12.0
                for lo, hi, v in bias_bands(hc, i + j):
                    b[lo:hi] += v
            if gate == 'z' and regime in ('keep', 'replace'):
                b += -30.0 if regime == 'keep' else 30.0
            p['w' + gate], p['b' + gate] = wt, b
        passes.append(p)
    return {'regime': regime, 'kind': kind, 'hx': hx, 'passes': passes, 'hc': hc, 'cc': cc, 'xc': xc, 'seed': seed}


def gru_motion(case, it):
    g = torch.Generator().manual_seed(77777 + 1000 * REGIMES.index(case['regime']) + 13 * case['seed'] + it)
    n, _, h, w = case['hx'].shape
    x = _rnd((n, case['xc'], h, w), g)
    return x.abs() + 20.0 if case['regime'] == 'cancelling' else x


def split_context(case, dtype=torch.float64):
    """the hoisted form of a case: per pass the parameters over [h | x'] only, and the context terms
    conv_c(c) + bias for z | r | q, (N, 3 hc, H, W), evaluated in ``dtype``."""
    hc, cc = case['hc'], case['cc']
    c = case['hx'][:, hc:hc + cc].to(dtype)
    passes, ctx = [], []
    for p in case['passes']:
        q = {'pad': p['pad']}
        terms = []
        for gate in 'zrq':
            wt = p['w' + gate]
            q['w' + gate] = torch.cat([wt[:, :hc], wt[:, hc + cc:]], 1)
            q['b' + gate] = torch.zeros_like(p['b' + gate])
            conv = F.conv2d if dtype == torch.float32 else conv_taps
            terms.append(conv(c, wt[:, hc:hc + cc].to(c), p['b' + gate].to(c), padding=p['pad']))
        passes.append(q)
        ctx.append(torch.cat(terms, 1))
    return passes, ctx


# ------------------------------------------------------------------------------------------------ the cell
class Exact:
    """the operations of the cell as the formula states them; mutants override one of them"""
    sigmoid = staticmethod(torch.sigmoid)
    tanh = staticmethod(torch.tanh)

    @staticmethod
    def blend(z, h, rh, q):
        return (1 - z) * h + z * q


def _cell(hx, passes, hc, dtype, ctx, iters, motion, ops_):
    hx = hx.to(dtype)
    conv = F.conv2d if dtype == torch.float32 else conv_taps
    h = hx[:, :hc]
    skip = hx.shape[1] - passes[0]['wz'].shape[1]          # context channels the passes do not convolve (hoisted form)
    assert (skip > 0) == (ctx is not None)
    x = hx[:, hc + skip:]
    trace = []
    for it in range(iters):
        if motion is not None:
            m = motion[it].to(hx)
            x = torch.cat([x[:, :x.shape[1] - m.shape[1]], m], 1)
        steps = []
        for i, p in enumerate(passes):
            cv = lambda inp, gate: conv(inp, p['w' + gate].to(hx), p['b' + gate].to(hx), padding=p['pad'])  # noqa: E731
            hin = torch.cat([h, x], 1)
            v_z, v_r = cv(hin, 'z'), cv(hin, 'r')
            if ctx is not None:
                v_z, v_r = v_z + ctx[i][:, :hc].to(hx), v_r + ctx[i][:, hc:2 * hc].to(hx)
            z, r = ops_.sigmoid(v_z), ops_.sigmoid(v_r)
            rh = r * h
            v_q = cv(torch.cat([rh, x], 1), 'q')
            if ctx is not None:
                v_q = v_q + ctx[i][:, 2 * hc:].to(hx)
            q = ops_.tanh(v_q)
            hn = ops_.blend(z, h, rh, q)
            steps.append({'h_in': h, 'x': x, 'v_z': v_z, 'v_r': v_r, 'v_q': v_q, 'z': z, 'r': r, 'rh': rh, 'q': q, 'h': hn})
            h = hn
        trace.append(steps)
    return {'h': h, 'trace': trace}


def gru_reference(hx, passes, h_channels, ctx=None, iters=1, motion=None):
    """the cell in float64.  ``passes``: per pass {'wz', 'wr', 'wq', 'bz', 'br', 'bq', 'pad'}; with ``ctx`` (one
    (N, 3 hc, H, W) pre-activation term per pass) the weights cover [h | x'] and hx = [h | c | x'].  ``motion``: one x'
    per iteration (the last channels of x).  Returns {'h': final state, 'trace': [iteration][pass] -> every
    intermediate (h_in, x, v_z, v_r, v_q, z, r, rh, q, h)}."""
    return _cell(hx, passes, h_channels, torch.float64, ctx, iters, motion, Exact)


def gru_fp32(hx, passes, h_channels, ctx=None, iters=1, motion=None, ops_=Exact):
    """the same cell in torch fp32 on the CPU: the evaluation the GPU's error is compared with, and the subject the
    mutants are made from."""
    return _cell(hx, passes, h_channels, torch.float32, ctx, iters, motion, ops_)


# ------------------------------------------------------------------------------------------------ sharp epilogue check
def ulp32(v):
    """distance from |v| to the next fp32 above it (fp64 tensor)"""
    a = v.float().abs()
    return (torch.nextafter(a, torch.full_like(a, math.inf)).double() - a.double())


def epilogue_expected(kind, v, h=None, z=None):
    """float64 value of one fused epilogue given its pre-activation: 'z' sigmoid(v); 'rh' sigmoid(v) h;
    'h' (1 - z) h + z tanh(v) with the z the epilogue read."""
    v = v.double()
    if kind == 'z':
        return torch.sigmoid(v)
    if kind == 'rh':
        return torch.sigmoid(v) * h.double()
    assert kind == 'h'
    return (1 - z.double()) * h.double() + z.double() * torch.tanh(v.double())


def epilogue_tol(kind, v, h=None, z=None):
    """(a_act + |act'(v)| 2 ulp(v)) s + 3 eps (|h| + 1), s = 1 ('z'), |h| ('rh'), z ('h'): the activation's claimed
    absolute error, two ulps of the pre-activation (acc + bias + res is added in another order on some routes), and three
    roundings of the product / blend."""
    v = v.double()
    if kind == 'h':
        a, d, s = A_TANH, 1 - torch.tanh(v) ** 2, z.double()
    else:
        sg = torch.sigmoid(v)
        a, d, s = A_SIG, sg * (1 - sg), (1.0 if kind == 'z' else h.double().abs())
    habs = 0.0 if h is None else h.double().abs()
    return (a + d * 2 * ulp32(v)) * s + 3 * EPS * (habs + 1)


def sharp_ratios(step):
    """worst |got - expected| / tolerance of the three epilogue outputs of one pass, each against ITS OWN fp32
    pre-activation (``step``: fp32 tensors v_z, v_r, v_q, h_in, z, rh, h)."""
    out = {}
    for kind, v, got, kw in (('z', step['v_z'], step['z'], {}),
                             ('rh', step['v_r'], step['rh'], {'h': step['h_in']}),
                             ('h', step['v_q'], step['h'], {'h': step['h_in'], 'z': step['z']})):
        err = (got.double() - epilogue_expected(kind, v, **kw)).abs()
        ratio = err / epilogue_tol(kind, v, **kw)
        ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, math.inf))
        out[kind] = float(ratio.max())
    return out


# ------------------------------------------------------------------------------------------------ the bound
def _dsig(v, dv):       # max of sigmoid' over [v - dv, v + dv]
    s = torch.sigmoid((v.abs() - dv).clamp(min=0))
    return s * (1 - s)


def _dtanh(v, dv):
    return 1 - torch.tanh((v.abs() - dv).clamp(min=0)) ** 2


def gru_bound(ref, passes, h_channels, budget=BUDGET['direct'], cterm=None):
    """elementwise bound on |h_fp32 - h_fp64| along ``ref`` (a ``gru_reference`` result computed with the same
    ``passes``): [iteration][pass] -> {'dv_z', 'dz', 'z_ub', 'drh', 'dv_q', 'dq', 'dh'}.
    Convolutions err by <= budget eps sum|w||x| (bias and context term counted as terms of the sum) and carry the
    error of their inputs through |w|; ``cterm`` (the float64 context terms of the hoisted form) adds what hoisting can
    cost: the term's own convolution error (it is part of sum|w||x| already: 4 eps more for the extra additions) and,
    on the F(4, 5) kernel, its passage through the transform domain together with its neighbours of the same 4-pixel
    tile (budget eps max|term| over the 7 pixels around)."""
    hc = h_channels
    out, dh = [], torch.zeros_like(ref['trace'][0][0]['h_in'])
    for steps in ref['trace']:
        row = []
        for i, (p, s) in enumerate(zip(passes, steps)):
            h, x = s['h_in'], s['x']
            aw = {g_: p['w' + g_].to(h).abs() for g_ in 'zrq'}
            ab = {g_: p['b' + g_].to(h).abs() for g_ in 'zrq'}
            zero_x = torch.zeros_like(x)
            extra = {g_: 0.0 for g_ in 'zrq'}
            if cterm is not None:
                kh, kw = p['wz'].shape[2:]
                win = (7, 1) if kh > 1 and kw == 1 else (1, 7) if kw > 1 and kh == 1 else (1, 1)
                t = cterm[i].to(h).abs()
                tm = F.max_pool2d(t, win, stride=1, padding=(win[0] // 2, win[1] // 2))
                for j, g_ in enumerate('zrq'):
                    extra[g_] = t[:, j * hc:(j + 1) * hc], tm[:, j * hc:(j + 1) * hc]

            def conv_err(gate, inp_abs, inp_err):
                ssum = conv_taps(inp_abs, aw[gate], ab[gate], p['pad'])
                dv = conv_taps(inp_err, aw[gate], None, p['pad'])
                if cterm is not None:
                    t_, tm_ = extra[gate]
                    return (budget + 4) * EPS * (ssum + t_) + budget * EPS * tm_ + dv
                return budget * EPS * ssum + dv

            hin_abs, hin_err = torch.cat([h.abs() + dh, x.abs()], 1), torch.cat([dh, zero_x], 1)
            dv_z, dv_r = conv_err('z', hin_abs, hin_err), conv_err('r', hin_abs, hin_err)
            dz = _dsig(s['v_z'], dv_z) * dv_z + A_SIG
            dr = _dsig(s['v_r'], dv_r) * dv_r + A_SIG
            drh = dr * (h.abs() + dh) + s['r'] * dh
            drh = drh + EPS * (s['rh'].abs() + drh)
            dv_q = conv_err('q', torch.cat([s['rh'].abs() + drh, x.abs()], 1), torch.cat([drh, zero_x], 1))
            dq = _dtanh(s['v_q'], dv_q) * dv_q + A_TANH
            dhn = (dz * (s['q'] - h).abs() + (1 - s['z']) * dh + s['z'] * dq + dz * (dh + dq)
                   + 3 * EPS * (h.abs() + dh + 1))
            row.append({'dv_z': dv_z, 'dz': dz, 'z_ub': (torch.sigmoid(s['v_z'] + dv_z) + A_SIG).clamp(max=1.0),
                        'drh': drh, 'dv_q': dv_q, 'dq': dq, 'dh': dhn})
            dh = dhn
        out.append(row)
    return out


def bound_ratio(got_h, ref, bound):
    """worst |h - h_64| / bound of the final state, and the worst absolute error"""
    err = (got_h.to(ref['h']) - ref['h']).abs()
    return float((err / bound[-1][-1]['dh']).max()), float(err.max())


# ------------------------------------------------------------------------------------------------ mutants
class SigmoidOff1e5(Exact):
    @staticmethod
    def sigmoid(v):
        z = torch.sigmoid(v)
        return z + 1e-5 * 4 * z * (1 - z)


class TanhScaled(Exact):
    @staticmethod
    def tanh(v):
        return torch.tanh(v) * (1 + 3e-6)


class BlendSwapsH(Exact):
    @staticmethod
    def blend(z, h, rh, q):
        return (1 - z) * rh + z * q


class BlendNeighbourZ(Exact):
    @staticmethod
    def blend(z, h, rh, q):
        zn = torch.roll(z, 1, dims=-1)
        return (1 - zn) * h + zn * q


class HardTanh(Exact):
    @staticmethod
    def tanh(v):
        return v.clamp(-1, 1)


# mutant -> the check that must reject it: 'sharp:<output>' (epilogue_expected / epilogue_tol) or 'bound' (gru_bound)
MUTANTS = {'sigmoid+1e-5': (SigmoidOff1e5, 'sharp:z'), 'tanh*(1+3e-6)': (TanhScaled, 'sharp:h'),
           'blend takes r*h for h': (BlendSwapsH, 'sharp:h'), 'blend takes z of pixel x-1': (BlendNeighbourZ, 'sharp:h'),
           'hard-tanh': (HardTanh, 'bound')}

SMALL = dict(hc=64, cc=32, xc=32)       # CPU-sized cases: 64-channel gates still hold one fragment boundary and the z | r split


# ------------------------------------------------------------------------------------------------ tests: closed forms
def _one_pass(hc, cin, k, pad, fill=0.0):
    p = {'pad': pad}
    for gate in 'zrq':
        p['w' + gate] = torch.full((hc, cin, *k), fill)
        p['b' + gate] = torch.zeros(hc)
    return p


@pytest.mark.parametrize('kind', ['SeqConv', 'Conv'])
def test_reference_zero_weights_closed_form(kind):
    """all-zero weights: every pass is h' = (1 - sigmoid(b_z)) h + sigmoid(b_z) tanh(b_q), whatever r is"""
    g = torch.Generator().manual_seed(3)
    hc, cx = 8, 6
    hx = _rnd((2, hc + cx, 5, 7), g)
    passes = [_one_pass(hc, hc + cx, k, pad) for k, pad in _KERNEL[kind]]
    for p in passes:
        p['bz'], p['br'], p['bq'] = _rnd((hc,), g, 2.0), _rnd((hc,), g, 50.0), _rnd((hc,), g, 2.0)
    ref = gru_reference(hx, passes, hc)
    want = hx[:, :hc].double()
    for p in passes:
        z = torch.sigmoid(p['bz'].double()).view(1, hc, 1, 1)
        want = (1 - z) * want + z * torch.tanh(p['bq'].double()).view(1, hc, 1, 1)
    assert len(ref['trace']) == 1 and len(ref['trace'][0]) == len(passes)
    torch.testing.assert_close(ref['h'], want, rtol=0, atol=1e-15)


def test_reference_z_bias_limits():
    """z bias -> -inf keeps the state exactly, -> +inf replaces it by q exactly; r bias -> -inf removes h from q"""
    case = gru_case('nominal', 1, 6, 9, 'SeqConv', seed=1, hc=8, cc=4, xc=4)
    for p in case['passes']:
        p['bz'] = torch.full((8,), -math.inf)
    ref = gru_reference(case['hx'], case['passes'], 8)
    assert torch.equal(ref['h'], case['hx'][:, :8].double())
    for p in case['passes']:
        p['bz'] = torch.full((8,), math.inf)
        p['br'] = torch.full((8,), -math.inf)
    ref = gru_reference(case['hx'], case['passes'], 8)
    last = ref['trace'][0][-1]
    assert torch.equal(ref['h'], last['q']) and float(last['rh'].abs().max()) == 0.0
    p = case['passes'][-1]
    x = torch.cat([torch.zeros(1, 8, 6, 9, dtype=torch.float64), case['hx'][:, 8:].double()], 1)
    want = torch.tanh(F.conv2d(x, p['wq'].double(), p['bq'].double(), padding=p['pad']))
    torch.testing.assert_close(ref['h'], want, rtol=0, atol=1e-15)


@pytest.mark.parametrize('pass_index,tap,dy,dx', [(0, 3, 0, 1), (0, 0, 0, -2), (1, 3, 1, 0), (1, 0, -2, 0)])
def test_reference_one_hot_weight_pins_orientation_and_padding(pass_index, tap, dy, dx):
    """a one-hot q weight at tap t of the 1x5 (5x1) pass reads the input t - 2 pixels to the right (below), zeros
    outside the image: v_q[y, x] = x_in[y + dy, x + dx]"""
    hc, cx, H, W = 4, 4, 6, 7
    g = torch.Generator().manual_seed(5)
    hx = _rnd((1, hc + cx, H, W), g)
    k, pad = _KERNEL['SeqConv'][pass_index]
    p = _one_pass(hc, hc + cx, k, pad)
    for o in range(hc):
        if pass_index == 0:
            p['wq'][o, hc + o, 0, tap] = 1.0
        else:
            p['wq'][o, hc + o, tap, 0] = 1.0
    p['bz'] = torch.full((hc,), math.inf)               # z = 1: h' = tanh(v_q)
    ref = gru_reference(hx, [p], hc)
    xin = hx[:, hc:].double()
    want = torch.zeros_like(xin)
    for y in range(H):
        for xx in range(W):
            if 0 <= y + dy < H and 0 <= xx + dx < W:
                want[:, :, y, xx] = xin[:, :, y + dy, xx + dx]
    assert torch.equal(ref['trace'][0][0]['v_q'], want)
    assert torch.equal(ref['h'], torch.tanh(want))


def test_reference_hoisted_form_is_the_same_cell():
    case = gru_case('saturated', 2, 7, 9, 'SeqConv', seed=2, hc=16, cc=8, xc=8)
    full = gru_reference(case['hx'], case['passes'], 16, iters=2, motion=[gru_motion(case, i) for i in range(2)])
    passes, ctx = split_context(case)
    hoist = gru_reference(case['hx'], passes, 16, ctx=ctx, iters=2, motion=[gru_motion(case, i) for i in range(2)])
    torch.testing.assert_close(hoist['h'], full['h'], rtol=0, atol=1e-12)


# ------------------------------------------------------------------------------------------------ tests: regimes
def test_regimes_are_what_they_claim():
    """the recipes reach the conditions they are named after (figures of the 128-channel cell at (2, 16, 20))"""
    sat = gru_case('saturated', 2, 16, 20, seed=0)
    ref = gru_reference(sat['hx'], sat['passes'], 128)
    vz = ref['trace'][0][0]['v_z']
    assert float(vz.abs().max()) > 100 and float((vz.abs() > 20).double().mean()) > 0.4
    b = torch.cat([sat['passes'][0]['bz'], sat['passes'][0]['br']])
    big = (b.abs() > 20).nonzero().flatten().tolist()
    assert {31, 32, 127, 128, 128 + 31, 128 + 32} <= set(big)          # bands across fragment boundaries and the z | r split
    can = gru_case('cancelling', 2, 16, 20, seed=0)
    ref = gru_reference(can['hx'], can['passes'], 128)
    s = ref['trace'][0][0]
    p = can['passes'][0]
    ssum = F.conv2d(torch.cat([s['h_in'], s['x']], 1).abs(), p['wz'].double().abs(), p['bz'].double().abs(), padding=p['pad'])
    trans = s['v_z'].abs() < 5
    assert float(s['v_z'].abs().max()) > 300 and bool(trans.any())
    assert float((ssum / s['v_z'].abs().clamp(min=1e-3))[trans].min()) > 50       # small sums of large cancelling terms
    for regime, lim in (('keep', 1e-9), ('replace', 1 - 1e-9)):
        c = gru_case(regime, 1, 8, 8, seed=0, **SMALL)
        z = gru_reference(c['hx'], c['passes'], 64)['trace'][0][0]['z']
        assert bool((z < lim).all()) if regime == 'keep' else bool((z > lim).all())
    he = gru_case('h_edge', 1, 8, 8, seed=0, **SMALL)['hx'][:, :64]
    for v in (1.0, -1.0, 1e-40, -1e-40, 1.4e-45):
        assert bool((he == torch.tensor(v)).any()), v
    assert bool(((he == 0) & torch.signbit(he)).any()) and bool(((he == 0) & ~torch.signbit(he)).any())


@pytest.mark.parametrize('kind', ['SeqConv', 'Conv'])
@pytest.mark.parametrize('regime', REGIMES)
def test_fp32_cell_inside_bound_and_sharp(regime, kind):
    """the unmutated fp32 torch cell is accepted by both nets in every regime, plain and hoisted, two iterations"""
    case = gru_case(regime, 2, 16, 20, kind, seed=0, **SMALL)
    motion = [gru_motion(case, i) for i in range(2)]
    ref = gru_reference(case['hx'], case['passes'], 64, iters=2, motion=motion)
    got = gru_fp32(case['hx'], case['passes'], 64, iters=2, motion=motion)
    bound = gru_bound(ref, case['passes'], 64)
    ratio, err = bound_ratio(got['h'], ref, bound)
    sharp = [sharp_ratios(s) for steps in got['trace'] for s in steps]
    worst = {k: max(s[k] for s in sharp) for k in ('z', 'rh', 'h')}
    print(f'[measured] fp32 torch cell, {regime} {kind}: max |h - h64| {err:.2e} = {ratio:.3f} of the bound; '
          f'sharp epilogue error / tolerance {worst}')
    assert torch.isfinite(got['h']).all() and ratio <= 1.0, (ratio, err)
    assert max(worst.values()) <= 1.0, worst
    # hoisted form: context terms evaluated in fp32, the cell on [h | x'] + terms
    passes_h, ctx64 = split_context(case)
    ctx32 = split_context(case, torch.float32)[1]
    got_h = gru_fp32(case['hx'], passes_h, 64, ctx=ctx32, iters=2, motion=motion)
    bound_h = gru_bound(ref, case['passes'], 64, cterm=ctx64)
    ratio_h, _ = bound_ratio(got_h['h'], ref, bound_h)
    assert ratio_h <= 1.0, ratio_h


# ------------------------------------------------------------------------------------------------ tests: non-vacuity
def _mutant_verdicts(regime, ops_):
    case = gru_case(regime, 2, 16, 20, 'SeqConv', seed=0, **SMALL)
    ref = gru_reference(case['hx'], case['passes'], 64)
    got = gru_fp32(case['hx'], case['passes'], 64, ops_=ops_)
    ratio, _ = bound_ratio(got['h'], ref, gru_bound(ref, case['passes'], 64))
    sharp = [sharp_ratios(s) for steps in got['trace'] for s in steps]
    return ratio, {k: max(s[k] for s in sharp) for k in ('z', 'rh', 'h')}


@pytest.mark.parametrize('name', list(MUTANTS))
def test_mutants_are_rejected_by_the_named_check(name):
    ops_, check = MUTANTS[name]
    for regime in ('nominal', 'saturated'):
        ratio, sharp = _mutant_verdicts(regime, ops_)
        print(f'[measured] mutant {name!r}, {regime}: error / bound {ratio:.2f}, sharp error / tolerance {sharp}')
        if check == 'bound':
            assert ratio > 1.0, (name, regime, ratio)
        else:
            assert sharp[check.split(':')[1]] > 1.0, (name, regime, sharp)
    ratio, sharp = _mutant_verdicts('nominal', Exact)
    assert ratio <= 1.0 and max(sharp.values()) <= 1.0


def test_bound_alone_misses_the_small_sigmoid_mutant():
    """why the sharp checks exist: a sigmoid that is off by 1e-5 stays inside gru_bound where sum|w||x| is large, and
    the sharp check on z rejects it there too"""
    ratio, sharp = _mutant_verdicts('saturated', SigmoidOff1e5)
    assert ratio <= 1.0 and sharp['z'] > 10.0, (ratio, sharp)
