"""CPU: backward of the InstanceNorm feature encoder (instance_norm_grad.hip, RAFTEncoder.in_backward) -- the three forms
of the InstanceNorm derivative and the whole layer walk restated in float64, a per-element bound for any fp32 evaluation
in the kernel's operation order, float64 autograd through ``oracle.raft_encoder(x, sd, prefix, 'IN')`` as the truth,
planted defects that must fall outside the bound, and the reference's own module (a fixture).

The bound, U = 2^-24, gamma(d) = d U / (1 - d U), D = in_depth(HW) of tests/test_stream_ops_host.py (the longest chain of
additions of a plane sum: the backward's two sums take the forward's tree, instance_norm_grad.hip).  Per plane of HW
elements, u the raw convolution output, g' the (masked, hence exact) cotangent:

  mean, rstd, xhat   norm_core's model of the forward, which this kernel repeats operation for operation:
                     |d mean| <= (D + 1) U mean|u|; the cancellation in u - mean enters as em = rstd |d mean|;
                     rstd relative rho = ((D + 4) U + em^2) / 2 + 3 U (+ 2 U, kept from norm_core, for slack);
                     |d xhat_i| <= (em + |xhat_i| rho)(1 + rho_lin) =: xb_i
  S1 = sum g'        gamma(D) sum |g'|
  S2 = sum g' xhat   p_i = g'_i xhat_i carries |g'_i| xb_i and its own rounding; the sum gamma(D) on top of all of it
  m1, m2             one rounding each (the division by HW, exact in float64 up to that rounding)
  du                 ((g' - m1) - xhat m2) rstd with running errors (EV): every operation hands on the errors of its
                     operands to first and second order and adds one rounding U (|value| + error).

It is derived, not measured: nothing in it comes from a run of the kernel.  The normalised shortcut's dr is the same
expression with r's statistics and its own S2; g' and S1 are shared.  fp32 underflow is outside the model.
"""
import os

import numpy as np
import pytest
import torch

from test_stream_ops_host import EV, IN_EPS, f64, in_depth, measured, worst_ratio  # noqa: E402
from test_fc_host import U, gamma  # noqa: E402
import test_context_grad_host as CH  # noqa: E402
from test_context_grad_host import BLOCKS, half  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, 'scflow_amd', 'csrc', 'instance_norm_grad.hip')).read()
HEADER = open(os.path.join(ROOT, 'include', 'scflow_hip.h')).read()
F = torch.nn.functional
EPS = float(np.float32(IN_EPS))
SYMBOLS = ['scf_instance_norm_grad', 'scf_instance_norm_res_norm_grad']
FORMS = ['mid', 'tail', 'tail_ds']

# plane sizes (H, W): every boundary of the kernel's dispatch and one float4 beyond it, the unaligned sizes of the
# encoder's own maps at the fixture's images, and the smallest planes.  Register forms: HW % 4 == 0 and HW / 4 <= 256 ->
# one float4 a thread, <= 1024 -> 4, <= 4096 -> 16; then 1024-thread sweeps up to HW / 4 = 20480; else 256-thread sweeps.
GRAD_SHAPES = [(1, 1), (1, 2), (2, 3), (5, 7), (9, 13), (2, 2), (32, 32), (4, 257), (64, 64), (4, 1025), (128, 128),
               (4, 4097), (256, 320), (4, 20481)]
assert {h * w for h, w in GRAD_SHAPES} >= {1, 2, 6, 35, 117, 1024, 1028, 4096, 4100, 16384, 16388, 81920, 81924}


# ============================================================================================ the three forms, float64
def stats64(u, eps=EPS, unbiased=False, eps_outside=False):
    """u (P, HW) float64 -> mean, rstd, xhat"""
    hw = u.shape[-1]
    with np.errstate(all='ignore'):
        mean = u.mean(-1, keepdims=True)
        var = ((u - mean) ** 2).sum(-1, keepdims=True) / (max(hw - 1, 1) if unbiased else hw)
        rstd = 1.0 / (np.sqrt(var) + eps) if eps_outside else 1.0 / np.sqrt(var + eps)
    return mean, rstd, (u - mean) * rstd


def du64(gp, xhat, rstd, drop=None):
    hw = gp.shape[-1]
    with np.errstate(all='ignore'):
        m1 = 0.0 if drop == 'mean' else gp.sum(-1, keepdims=True) / hw
        m2 = 0.0 if drop == 'xhat' else (gp * xhat).sum(-1, keepdims=True) / hw
        return ((gp - m1) - xhat * m2) * rstd


def _planes(t):
    t = f64(t)
    return t.reshape(t.shape[0] * t.shape[1], -1)


def in_grad64(g, u, y=None, r=None, defect=None):
    """the three forms in float64 on (N, C, H, W) operands -> dict of the kernel's outputs (gp, du, dr) where the form has
    them.  ``defect``: one planted mistake (PLANTED)."""
    shape = np.shape(g)
    G, Uu = _planes(g), _planes(u)
    with np.errstate(all='ignore'):
        if y is None:
            gp = G
        else:
            mask = (Uu if defect == 'mask_from_u' else _planes(y)) > 0
            gp = np.where(mask, G, 0.0)
        _, rstd, xhat = stats64(Uu, unbiased=defect == 'unbiased', eps_outside=defect == 'eps_outside')
        out = dict(du=du64(gp, xhat, rstd, drop={'mean_dropped': 'mean', 'xhat_dropped': 'xhat'}.get(defect)))
        if y is not None and r is None:
            out['gp'] = G if defect == 'gp_unmasked' else gp
        if r is not None:
            if defect == 'dr_with_u_stats':
                mean, _, _ = stats64(_planes(r))
                out['dr'] = du64(gp, (_planes(r) - mean) * rstd, rstd)
            else:
                _, rr, rhat = stats64(_planes(r))
                out['dr'] = du64(gp, rhat, rr)
    return {k: v.reshape(shape) for k, v in out.items()}


# ================================================================================================ the derived bound
def _operand_ev(u, depth):
    """(EV of xhat, EV of rstd) of one operand (P, HW) for the forward's two-pass fp32 evaluation at chain depth `depth`:
    test_stream_ops_host.norm_core's model, with rstd's own part kept apart"""
    with np.errstate(all='ignore'):
        _, rstd, xhat = stats64(u)
        em = (depth + 1) * U * np.abs(u).mean(-1, keepdims=True) * rstd
        rho_lin = 0.5 * (depth + 4) * U + 3 * U + 2 * U
        rho = rho_lin + 0.5 * em * em
        return EV(xhat, (em + np.abs(xhat) * rho) * (1 + rho_lin)), EV(rstd, rstd * rho * (1 + rho_lin))


def _sum_ev(t, depth):
    """a plane sum of the EV `t` (P, HW) in a tree of chain depth `depth`"""
    with np.errstate(all='ignore'):
        e = t.e.sum(-1, keepdims=True)
        return EV(t.v.sum(-1, keepdims=True), e + gamma(depth) * ((np.abs(t.v)).sum(-1, keepdims=True) + e))


def _du_ev(gp, X, RS, S1, depth):
    hw = gp.v.shape[-1]
    S2 = _sum_ev(gp * X, depth)
    m1, m2 = S1 / EV(float(hw)), S2 / EV(float(hw))
    # EV's quotient of two exact values is exact: S1 / HW rounds once all the same
    m1.e, m2.e = m1.e + U * np.abs(m1.v), m2.e + U * np.abs(m2.v)
    return ((gp - m1) - X * m2) * RS


def in_grad_ref(g, u, y=None, r=None, aligned=True, depth=None):
    """-> {output: (float64 value, per-element bound)} of the form the operands select, for an fp32 evaluation in the
    kernel's order (``depth``: another chain depth, for an evaluation in another order)"""
    shape = np.shape(g)
    hw = shape[2] * shape[3]
    d = in_depth(hw, aligned) if depth is None else depth
    val = in_grad64(g, u, y, r)
    G, Uu = _planes(g), _planes(u)
    gp = EV(G if y is None else np.where(_planes(y) > 0, G, 0.0))
    S1 = _sum_ev(gp, d)
    out = {}
    X, RS = _operand_ev(Uu, d)
    with np.errstate(all='ignore'):
        out['du'] = _du_ev(gp, X, RS, S1, d).e
        if r is not None:
            X, RS = _operand_ev(_planes(r), d)
            out['dr'] = _du_ev(gp, X, RS, S1, d).e
    if 'gp' in val:
        out['gp'] = np.zeros_like(gp.v)                              # a select: exact
    return {k: (val[k], np.asarray(out[k]).reshape(shape)) for k in val}


def _rand(shape, seed, scale=1.0):
    return torch.from_numpy(np.asarray(CH._rand(shape, seed, scale), dtype=np.float32))


def inorm(t):
    """F.instance_norm; a plane of one element, which torch refuses, is normalised by the same expression"""
    if t.shape[2] * t.shape[3] > 1:
        return F.instance_norm(t, eps=EPS)
    mean = t.mean((2, 3), keepdim=True)
    return (t - mean) / torch.sqrt(((t - mean) ** 2).mean((2, 3), keepdim=True) + EPS)


def grad_case(form, planes, hw, seed=0, regime='nominal'):
    """operands (1, planes, H, W) float32 of one form -> dict(g, u[, y][, r]); y is what an fp32 forward gives"""
    h, w = hw
    shape = (1, planes, h, w)
    s = 9000 + 17 * seed + 1000 * FORMS.index(form)
    u, g = 0.5 + 2.0 * _rand(shape, s), _rand(shape, s + 1)
    if regime == 'constant':
        u = torch.full(shape, 3.7)
    elif regime == 'offset':
        u = 1e4 + _rand(shape, s)
    case = dict(g=g, u=u)
    if form == 'mid':
        if regime == 'all_masked':
            case['g'] = torch.zeros(shape)
        else:                                                       # the consumer's epilogue has masked g already
            case['g'] = torch.where(inorm(u.double()) > 0, g.double(), 0.0).float()
        return case
    r = _rand(shape, s + 2)
    xh = inorm(u.double())
    if form == 'tail':
        y = torch.relu(xh + r.double()).float()
    else:
        r = 0.3 + 1.5 * r
        case['r'] = r
        y = torch.relu(xh + inorm(r.double())).float()
    case['y'] = torch.zeros(shape) if regime == 'all_masked' else y
    return case


# ===================================================================================================== the self-checks
def test_symbols_are_declared_exported_and_bound():
    from scflow_amd import _lib
    for name in SYMBOLS:
        assert f'int {name}(' in HEADER and f'extern "C" int {name}(' in SRC and name in _lib.SIGNATURES, name
    assert 'atomic' not in SRC.split('#include')[1]                 # no atomics: one summation order
    build = open(os.path.join(ROOT, 'scflow_amd', 'csrc', 'build.py')).read()
    assert "'instance_norm_grad.hip'" in build


def test_c_abi_rejects_bad_arguments_before_any_launch():
    """every refusal returns before the stream is touched, so this runs without a GPU"""
    from scflow_amd import _lib
    import ctypes as C
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    E, EUNSUP = -1, -2                          # scflow_hip.h: SCF_EINVAL, SCF_EUNSUPPORTED
    mid = lambda g=p, y=None, u=p, gp=None, du=p, n=2, hw=8: lib.scf_instance_norm_grad(g, y, u, gp, du, n, hw, 1e-5, None)  # noqa: E731
    ds = lambda g=p, y=p, u=p, r=p, du=p, dr=p, n=2, hw=8: lib.scf_instance_norm_res_norm_grad(g, y, u, r, du, dr, n, hw, 1e-5, None)  # noqa: E731
    for bad in (dict(g=None), dict(u=None), dict(du=None), dict(n=0), dict(n=-1), dict(hw=0), dict(y=p), dict(gp=p)):
        assert mid(**bad) == E, bad
    for bad in (dict(g=None), dict(y=None), dict(u=None), dict(r=None), dict(du=None), dict(dr=None), dict(n=0), dict(hw=-3)):
        assert ds(**bad) == E, bad
    assert mid(n=2 ** 31) == EUNSUP and ds(n=2 ** 31) == EUNSUP
    assert not any(buf)


def _autograd(case, dtype):
    """torch autograd of the forward expression the form belongs to -> dict(du[, dr][, gp])"""
    u = case['u'].to(dtype).requires_grad_(True)
    xh = inorm(u)
    g = case['g'].to(dtype)
    if 'y' not in case:
        (xh * g).sum().backward()
        return dict(du=u.grad)
    r = case.get('r', None)
    if r is None:                                    # the identity shortcut: its cotangent is G [y > 0]
        res = torch.zeros_like(u).requires_grad_(True)
        gp = torch.where(case['y'] > 0, g, torch.zeros_like(g))
        ((xh + res) * gp).sum().backward()
        return dict(du=u.grad, gp=res.grad)
    r = r.to(dtype).requires_grad_(True)
    gp = torch.where(case['y'] > 0, g, torch.zeros_like(g))
    ((xh + inorm(r)) * gp).sum().backward()
    return dict(du=u.grad, dr=r.grad)


HOST_SHAPES = [(1, 1), (1, 2), (2, 3), (5, 7), (9, 13), (32, 32), (4, 257)]


@pytest.mark.parametrize('form', FORMS)
def test_forms_equal_float64_autograd_and_fp32_torch_falls_inside(form):
    """the restated forms are float64 autograd of F.instance_norm; fp32 autograd of the same expression lies inside the
    bound taken at depth HW - 1 + D, which covers torch's own summation order whatever it is (any order of n terms is
    within gamma(n - 1) sum |terms|)"""
    worst = 0.0
    for hw in HOST_SHAPES:
        case = grad_case(form, 3, hw)
        want = _autograd(case, torch.float64)
        n = hw[0] * hw[1]
        ref = in_grad_ref(**case, depth=n - 1 + in_depth(n))
        got = _autograd(case, torch.float32)
        assert sorted(ref) == sorted(want)
        for k in want:
            scale = max(float(want[k].abs().max()), 1e-300)
            assert float(np.abs(ref[k][0] - f64(want[k])).max()) <= 1e-12 * max(scale, 1.0), (form, hw, k)
            assert np.isfinite(ref[k][1]).all() and (ref[k][1] >= 0).all()
            worst = max(worst, worst_ratio(got[k], *ref[k]))
        if n == 1:
            assert not ref['du'][0].any()
    measured(f'fp32 torch autograd of F.instance_norm, form {form}: worst error / bound', worst)
    assert worst <= 1


PLANTED = {'mid': ['mean_dropped', 'xhat_dropped', 'unbiased', 'eps_outside'],
           'tail': ['mask_from_u', 'gp_unmasked'],
           'tail_ds': ['dr_with_u_stats']}


@pytest.mark.parametrize('form,defect', [(f, d) for f, ds in PLANTED.items() for d in ds])
def test_planted_defects_outside(form, defect):
    """each at its own launch, against that launch's bound at the kernel's own depth; planes of 117 elements with a
    spread of 0.1 (eps is then 1e-3 of the variance, and Bessel's correction 1 / 116)"""
    case = grad_case(form, 4, (9, 13), seed=3)
    case['u'] = 0.1 * case['u']
    if form == 'mid':
        case = dict(case, g=torch.where(inorm(case['u'].double()) > 0, _rand(case['g'].shape, 77).double(), 0.0).float())
    ref = in_grad_ref(**case, aligned=False)
    bad = in_grad64(**case, defect=defect)
    key = {'gp_unmasked': 'gp', 'dr_with_u_stats': 'dr'}.get(defect, 'du')
    worst = worst_ratio(bad[key], *ref[key])
    measured(f'planted defect {defect} ({form}), error / bound', worst)
    assert worst >= 10


# ========================================================================================= the encoder, restated
OUT_CHANNELS = 256


def param_shapes(cin=3):
    """the 32 parameters of the InstanceNorm encoder in named_parameters() order (InstanceNorm2d has none)"""
    p = {}

    def conv(key, co, ci, k):
        p[f'{key}.weight'], p[f'{key}.bias'] = (co, ci, k, k), (co,)

    conv('conv1', 64, cin, 7)
    for key, ci, co, stride in BLOCKS:
        conv(f'{key}.conv1', co, ci, 3)
        conv(f'{key}.conv2', co, co, 3)
        if stride != 1:
            conv(f'{key}.downsample.0', co, ci, 1)
    conv('conv2', OUT_CHANNELS, 128, 1)
    return p


PARAM_SHAPES = param_shapes()
PARAM_NAMES = list(PARAM_SHAPES)
# the biases in front of an InstanceNorm: gradient 0 in exact arithmetic
ZERO_BIASES = [n for n in PARAM_NAMES if n.endswith('.bias') and n != 'conv2.bias']


def encoder_params(seed, prefix=''):
    from test_fc_grad_host import golden_param
    return {prefix + name: golden_param('feat.' + name, shape, seed) for name, shape in PARAM_SHAPES.items()}


def encoder_inputs(seed, n, h, w, tag=''):
    """-> (images (n, 3, h, w), cotangent (n, 256, h', w') at the head's output), float32"""
    from test_fc_grad_host import golden_param
    ho, wo = half(half(half(h))), half(half(half(w)))
    x = golden_param(f'feat.image{tag}.{n}.{h}x{w}', (n, 3, h, w), seed, scale=1.0)
    g = golden_param(f'feat.cot{tag}.{n}.{h}x{w}', (n, OUT_CHANNELS, ho, wo), seed, scale=1.0)
    return x, g


def oracle_grads(x, sd, g_out, prefix='', dtype=torch.float64):
    """autograd through oracle.raft_encoder(kind='IN') -> (out, dict of the 32 gradients)"""
    import sys
    sys.path.insert(0, ROOT)
    from oracle import scflow_oracle as oracle
    sdx = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    out = oracle.raft_encoder(x.to(dtype), sdx, prefix, 'IN')
    (out * g_out.to(dtype)).sum().backward()
    return out.detach(), {k[len(prefix):]: v.grad for k, v in sdx.items()}


TIE_FACTOR = 64


def forward64(x, sd, prefix='', relu=None, ties=None):
    """the forward with everything the backward reads, float64 torch (differentiable where ``sd`` requires grad) -> dict
    x, stem, u_stem, t{i}, y{i}, u1_{i}, u2_{i}, r{i}, out.

    ``relu``: {stem | t{i} | y{i}: the decisions (bool) of an fp32 forward}; a unit whose float64 pre-activation lies within
    what an fp32 forward may deviate there takes the given decision, as tests/test_context_grad_host.py::forward64 does.
    The deviation allowed of IN(u): TIE_FACTOR (K + 8) U rstd (1 + |xhat|) (m + mean m), m = sum |w| |x| + |b| of the
    unit's own convolution with K terms (its error, the error of the plane mean, and rstd's relative one)."""
    p = {k[len(prefix):]: v.double() for k, v in sd.items()}

    def layer(v, ckey, stride, pad):
        w, b = p[f'{ckey}.weight'], p[f'{ckey}.bias']
        u = F.conv2d(v, w, b, stride=stride, padding=pad)
        xh = F.instance_norm(u, eps=EPS)
        with torch.no_grad():
            m = (w[0].numel() + 8) * F.conv2d(v.abs(), w.abs(), b.abs(), stride=stride, padding=pad)
            rstd = 1.0 / torch.sqrt(u.var((2, 3), unbiased=False, keepdim=True) + EPS)
            mag = rstd * (1 + xh.abs()) * (m + m.mean((2, 3), keepdim=True))
        return u, xh, mag

    def gate(key, pre, mag):
        if relu is None:
            return torch.relu(pre)
        with torch.no_grad():
            own = pre > 0
            allowed = TIE_FACTOR * U * mag
            tied = (own != torch.as_tensor(relu[key]).reshape(own.shape)) & (pre.abs() <= allowed)
            g = torch.where(tied, ~own, own).to(pre.dtype)
        if ties is not None and bool(tied.any()):
            ties.append((key, int(tied.sum()), float((pre.detach().abs() / allowed)[tied].max())))
        return pre * g

    acts = dict(x=x.double())
    acts['u_stem'], xh, mag = layer(acts['x'], 'conv1', 2, 3)
    v = acts['stem'] = gate('stem', xh, mag)
    for i, (key, _, _, stride) in enumerate(BLOCKS):
        acts[f'u1_{i}'], xh, mag = layer(v, f'{key}.conv1', stride, 1)
        t = acts[f't{i}'] = gate(f't{i}', xh, mag)
        if stride != 1:
            acts[f'r{i}'], idt, imag = layer(v, f'{key}.downsample.0', stride, 0)
        else:
            idt, imag = v, v.detach().abs()
        acts[f'u2_{i}'], xh, mag = layer(t, f'{key}.conv2', 1, 1)
        v = acts[f'y{i}'] = gate(f'y{i}', xh + idt, mag + imag)
    acts['out'] = F.conv2d(v, p['conv2.weight'], p['conv2.bias'])
    return acts


MASK_KEYS = ['stem'] + [f'{k}{i}' for i in range(len(BLOCKS)) for k in 'ty']


def relu_decisions(kept):
    """the ReLU decisions of a forward from the activations it kept (RAFTEncoder.kept, or forward64's dict)"""
    return {k: (kept[k] > 0).cpu() for k in MASK_KEYS}


def truth64(x, sd, g_out, prefix='', relu=None, ties=None):
    """float64 autograd through forward64 -> (its activations, detached; dict of the 32 gradients)"""
    sd64 = {k: v.detach().cpu().double().clone().requires_grad_(True) for k, v in sd.items()}
    acts = forward64(x.detach().cpu(), sd64, prefix, relu, ties)
    (acts['out'] * g_out.detach().cpu().double()).sum().backward()
    return {k: v.detach() for k, v in acts.items()}, {k[len(prefix):]: v.grad for k, v in sd64.items()}


def backward_ref64(acts, sd, g_out, prefix='', launches=None):
    """RAFTEncoder.in_backward restated in float64 on the activations ``acts``: the convolution gradients by
    torch.nn.grad on float64 tensors, the InstanceNorm derivative by in_grad64 -> dict name -> gradient (numpy).
    ``launches``: a dict that receives the maps the walk passes on, keyed as in_backward's ``intermediates``."""
    from torch.nn import grad as TG
    p = {k[len(prefix):]: v.detach().double() for k, v in sd.items()}
    a = {k: v.detach().double() for k, v in acts.items()}
    rec = {} if launches is None else launches
    out = {}
    T = lambda v: torch.from_numpy(np.ascontiguousarray(v))         # noqa: E731

    def wgrad(key, g, x, stride, pad):
        w = p[f'{key}.weight']
        out[f'{key}.weight'] = TG.conv2d_weight(x, w.shape, g, stride=stride, padding=pad).numpy()
        out[f'{key}.bias'] = g.sum((0, 2, 3)).numpy()

    def dgrad(key, g, x, stride, pad):
        return TG.conv2d_input(x.shape, p[f'{key}.weight'], g, stride=stride, padding=pad)

    nb = len(BLOCKS)
    g = g_out.detach().double()
    wgrad('conv2', g, a[f'y{nb - 1}'], 1, 0)
    G = dgrad('conv2', g, a[f'y{nb - 1}'], 1, 0)
    for i in reversed(range(nb)):
        key, _, _, stride = BLOCKS[i]
        x_in, t, y = a[f'y{i - 1}' if i else 'stem'], a[f't{i}'], a[f'y{i}']
        if stride == 1:
            res = in_grad64(G, a[f'u2_{i}'], y=y)
            g_sc, du2 = T(res['gp']), T(res['du'])
        else:
            res = in_grad64(G, a[f'u2_{i}'], y=y, r=a[f'r{i}'])
            du2, dr = T(res['du']), T(res['dr'])
        rec[f'{key}.in2'] = {k: v for k, v in res.items()}
        wgrad(f'{key}.conv2', du2, t, 1, 1)
        g_t = dgrad(f'{key}.conv2', du2, t, 1, 1) * (t > 0)
        du1 = T(in_grad64(g_t, a[f'u1_{i}'])['du'])
        rec[f'{key}.in1'] = dict(du=du1.numpy())
        wgrad(f'{key}.conv1', du1, x_in, stride, 1)
        G = dgrad(f'{key}.conv1', du1, x_in, stride, 1)
        if stride == 1:
            G = G + g_sc
        else:
            wgrad(f'{key}.downsample.0', dr, x_in, stride, 0)
            G = G + dgrad(f'{key}.downsample.0', dr, x_in, stride, 0)
        if i == 0:
            G = G * (x_in > 0)
    du = T(in_grad64(G, a['u_stem'])['du'])
    rec['in1'] = dict(du=du.numpy())
    wgrad('conv1', du, a['x'], 2, 3)
    return out


CASE_SEED = 20261


def small_case(n=4, h=18, w=26, seed=CASE_SEED):
    """2N = 4 stacked samples, as the shared encoder sees the render and the real images"""
    sd = encoder_params(seed)
    x, g = encoder_inputs(seed, n, h, w)
    return sd, x, g


# Room of the composed gradients, |g - g64| <= ROOM x the largest entry of that gradient's float64 value.  The argument of
# tests/test_context_grad_host.py::test_reference_autograd_agrees_with_float64, re-derived for this encoder on 2N = 4
# samples: 14 convolution layers there and back, the longest sums 1152 products (3x3, 128 channels) or 2N h w <= 468
# pixels (a weight gradient), so sqrt(1152) is still the longest random walk: 14 sqrt(1152) U ~ 3e-5.  The 15 InstanceNorm
# layers add per plane (D + 4) U / 2 + 5 U < 1e-6 relative each way (the bound above at em ~ 0: these planes have |mean|
# ~ spread), below the convolutions' share; the statistics of the smallest planes (6 and 12 pixels) are no worse
# conditioned in relative terms, they only make d xhat / d u larger, which both evaluations share.  Topped by 3: 1e-4.
GOLDEN_ROOM = 1e-4
# A bias in front of an InstanceNorm: the exact gradient is 0 and an fp32 evaluation leaves the rounding of sum du over
# 2N planes of its channel.  Each du carries the same first-order relative error as above (<= GOLDEN_ROOM of the layer's
# typical |du|) and the sum adds gamma(2N h w) <= 468 U = 3e-5 of sum |du|: |db| <= GOLDEN_ROOM x sum |du| of the channel.
ZERO_BIAS_ROOM = GOLDEN_ROOM


def zero_bias_scales(launches):
    """name -> per-channel sum |du| of the layer in front of that bias, from backward_ref64's ``launches``"""
    s = {'conv1.bias': np.abs(launches['in1']['du']).sum((0, 2, 3))}
    for key, _, _, stride in BLOCKS:
        s[f'{key}.conv1.bias'] = np.abs(launches[f'{key}.in1']['du']).sum((0, 2, 3))
        s[f'{key}.conv2.bias'] = np.abs(launches[f'{key}.in2']['du']).sum((0, 2, 3))
        if stride != 1:
            s[f'{key}.downsample.0.bias'] = np.abs(launches[f'{key}.in2']['dr']).sum((0, 2, 3))
    return s


def composed_error(got, truth, scales, pick=None):
    """-> (worst |got - g64| / (largest |g64| entry) over the weights and the head's bias, worst |got| / sum |du| over the
    biases in front of an InstanceNorm); ``pick``: the thinning applied to ``got`` already (golden_pick)"""
    worst, worst0 = 0.0, 0.0
    for name in PARAM_NAMES:
        want = f64(truth[name])
        have = f64(got[name])
        if pick is not None:
            want_p = pick(name, want)
        else:
            want_p = want
        assert have.shape == want_p.shape, name
        if name in ZERO_BIASES:
            assert np.abs(want).max() <= 1e-9 * scales[name].max(), name            # float64: zero up to its own rounding
            worst0 = max(worst0, float((np.abs(have) / scales[name]).max()))
        else:
            assert np.abs(want).max() > 0, name
            worst = max(worst, float(np.abs(have - want_p).max() / np.abs(want).max()))
    return worst, worst0


@pytest.mark.parametrize('hw', [(18, 26), (16, 24)], ids=lambda v: f'{v[0]}x{v[1]}')
def test_restated_walk_equals_float64_autograd(hw):
    sd, x, g = small_case(4, *hw)
    out, truth = oracle_grads(x, sd, g)
    acts = forward64(x, sd)
    # the oracle's eps is the double 1e-5, the kernel's (and this file's) the fp32 number next to it, 2.5e-8 of eps away:
    # the two graphs agree to ~1e-13 / var a layer, not bit for bit; the restated walk is held to this file's own graph
    close = lambda a, b, tol: float((a - b).abs().max()) <= tol * max(float(b.abs().max()), 1.0)      # noqa: E731
    assert close(acts['out'], out, 1e-9)
    acts2, own = truth64(x, sd, g, relu=relu_decisions(acts))
    assert all(close(acts2[k], acts[k], 1e-12) for k in acts)
    launches = {}
    got = backward_ref64(acts, sd, g, launches=launches)
    assert sorted(got) == sorted(PARAM_NAMES) and len(got) == 32
    scales = zero_bias_scales(launches)
    for name in PARAM_NAMES:
        want = own[name].numpy()
        scale = scales[name].max() if name in ZERO_BIASES else np.abs(want).max()
        assert scale > 0, name
        assert np.abs(truth[name].numpy() - want).max() <= 1e-8 * scale, name
        assert np.abs(got[name] - want).max() <= 1e-11 * scale, name


def test_fp32_autograd_inside_the_room():
    """torch's own fp32 autograd of the oracle graph (CPU) meets the rooms that the GPU chain is held to"""
    sd, x, g = small_case(4, 18, 26)
    acts = forward64(x, sd)
    launches = {}
    backward_ref64(acts, sd, g, launches=launches)
    _, truth = truth64(x, sd, g)
    _, got = oracle_grads(x, sd, g, dtype=torch.float32)
    worst, worst0 = composed_error(got, truth, zero_bias_scales(launches))
    measured('fp32 torch autograd of the IN encoder: worst max error / largest float64 entry', worst)
    measured('fp32 torch autograd of the IN encoder: worst |zero bias gradient| / sum |du|', worst0)
    assert worst <= GOLDEN_ROOM and worst0 <= ZERO_BIAS_ROOM


# ======================================================================================================== the fixture
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'feature_grads.npz')
GOLDEN_SIZES = CH.GOLDEN_SIZES
GOLDEN_N, GOLDEN_SEED = CH.GOLDEN_N, CH.GOLDEN_SEED
golden_pick = CH.golden_pick


def golden_case(hw):
    """-> (tag, float32 state dict, the 2N = 4 stacked images, cotangent at the head's output)"""
    sd = encoder_params(GOLDEN_SEED)
    x, g = encoder_inputs(GOLDEN_SEED, 2 * GOLDEN_N, *hw, tag='.golden')
    return f'{hw[0]}x{hw[1]}', sd, x, g


@pytest.mark.parametrize('hw', GOLDEN_SIZES, ids=lambda v: f'{v[0]}x{v[1]}')
def test_reference_autograd_agrees_with_float64(hw):
    """The reference's own RAFTEncoder (``encoder`` of configs/refine_models/scflow.py: norm_cfg IN; fp32 autograd on the
    CPU, loss <cotangent, output>) against float64 autograd of the oracle on the same seeds, inside GOLDEN_ROOM and
    ZERO_BIAS_ROOM (derived above).  What the fixture pins is that the reference module computes what the oracle
    computes: a wrong term moves a gradient by its own size."""
    z = np.load(GOLDEN)
    tag, sd, x, g = golden_case(hw)
    acts, truth = truth64(x, sd, g)
    launches = {}
    backward_ref64(acts, sd, g, launches=launches)
    got = {name: z[f'{tag}.{name}'] for name in PARAM_NAMES}
    assert all(v.dtype == np.float32 for v in got.values())
    worst, worst0 = composed_error(got, truth, zero_bias_scales(launches), pick=golden_pick)
    measured(f'reference IN RAFTEncoder autograd {tag}: |fixture - float64| / largest entry', worst)
    measured(f'reference IN RAFTEncoder autograd {tag}: worst |zero bias gradient| / sum |du|', worst0)
    assert worst <= GOLDEN_ROOM and worst0 <= ZERO_BIAS_ROOM
    assert os.path.getsize(GOLDEN) < 200 * 1024
