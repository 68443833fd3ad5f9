"""CPU: BatchNorm on the statistics of the batch (batch_norm_train.hip, ops.batch_norm_train / batch_norm_train_grad) -- the
three forms, forward and backward, and the running update restated in float64; a per-element bound for any fp32 evaluation
in the kernel's operation order; torch's own fp32 ``F.batch_norm(training=True)`` and its autograd inside that bound;
planted defects outside it; the C ABI's refusals; the additive Python surface (``network_parameters``,
``build_optimizer(network=True)``) with ``train_step``'s refusal still in place.

The bound, U = 2^-24, gamma(d) = d U / (1 - d U).  Per channel of M = N HW values x, with the kernel's sums (a plane or a
16384-element chunk per workgroup, P = N K partials per channel):

  D      the longest chain of additions of a chunk sum: a thread's float4s ((a + b) + (c + d): 2, then one chain add each),
         the wave's 6 levels and the workgroup's 2 (``bn_depths``); without float4 the thread's scalar chain.
  L      levels of the Chan combination: 6 in a group of 64 partials plus one fold per group.  A level computes
         mean = mean_a + d f and m2 = (m2_a + m2_b) + (d d)(na f) in 4 and 5 roundings of quantities bounded by max|x|
         and by m2.
  mean   |d mean| <= (D + 1) U mean|x| + 4 L U max|x| =: ea;  em = ea rstd is what the cancellation in x - mean costs.
  rstd   relative rho = ((D + 4 + 5 L) U + em^2) / 2 + 2 em + 5 U: the sum of squares about an inexact centre is off by
         n d^2 (the em^2 term, as for InstanceNorm), a level's d d carries 2 |d| ea, at most 4 em of the variance in all (the
         2 em term; InstanceNorm has no such term), and the division, the addition of eps, root and reciprocal are the 5 U.
  xhat   |d xhat_i| <= (em + |xhat_i| rho)(1 + rho_lin)
  y, du  running errors (EV of tests/test_stream_ops_host.py) through the expressions as the kernels write them; a sum of the
         backward takes D plus the apply pass's chain (one add per 64 partials) and its 6 levels.
  running statistics: EV through (1 - m) r + m b with b's error from above; the variance's relative error is 2 rho + 2 U.

It is derived, not measured: nothing in it comes from a run of the kernel.  For torch's fp32 evaluation, whose order this
file does not know, D is replaced by M - 1 + D: any order of n terms is within gamma(n - 1) sum |terms|.
fp32 underflow is outside the model."""
import math
import os

import numpy as np
import pytest
import torch

from test_stream_ops_host import EV, f64, measured, worst_ratio
from test_fc_host import U, gamma

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, 'scflow_amd', 'csrc', 'batch_norm_train.hip')).read()
HEADER = open(os.path.join(ROOT, 'include', 'scflow_hip.h')).read()
F = torch.nn.functional
EPS = float(np.float32(1e-5))
MOMENTUM = 0.1
SYMBOLS = ['scf_batch_norm_train_workspace', 'scf_batch_norm_train', 'scf_batch_norm_train_grad', 'scf_batch_norm_train_route']
FORMS = ['mid', 'tail', 'tail_ds']
CHUNK = 16384

# (N, C, H, W): the scalar route (HW = 6, the encoder's coarsest planes at small sizes); N = 1; a plain vector plane; many
# blocks on the vector route; a plane beyond one chunk (two chunks, the second a partial one); more partials than a
# butterfly's first level pairs up, odd N
SHAPES = [(3, 5, 2, 3), (1, 2, 4, 4), (2, 3, 8, 12), (4, 64, 16, 16), (2, 2, 136, 132), (33, 2, 4, 4)]
# every launch geometry of batch_norm_train.hip (ROUTE_WHY: what ops.batch_norm_train_route must say of each, which
# test_route_coverage asserts): HW 1040 / 4096, the two ends of the 4-float4 statistics kernel, 4096 one full apply block;
# HW 4100, the bottom of the 16-float4 kernel, a second apply block of 4 elements; HW 16384, one whole chunk, 4 full apply
# blocks; HW 16388, a second chunk of 4 elements (one float4); HW 16389 / 16386, the looped kernel with a second chunk of 5 /
# of 2 elements, 5 scalar apply blocks; P = N K = 65, 128, 129 partials: a second group of 64 with one entry, full, and a
# third with one entry (HW 2: the scalar route); M = 2, the smallest count that has an unbiased variance
SHAPES += [(2, 3, 20, 52), (1, 2, 64, 64), (2, 2, 25, 164), (1, 2, 128, 128), (1, 2, 4, 4097), (2, 2, 3, 5463), (1, 2, 1, 16386),
           (65, 2, 2, 2), (128, 2, 1, 2), (129, 1, 1, 2), (1, 2, 1, 2)]
ROUTE_WHY = {(2, 3, 20, 52): dict(stats=4, vec=True, K=1, bpp=1, groups=1),
             (1, 2, 64, 64): dict(stats=4, vec=True, K=1, bpp=1, groups=1),
             (2, 2, 25, 164): dict(stats=16, vec=True, K=1, bpp=2, groups=1),
             (1, 2, 128, 128): dict(stats=16, vec=True, K=1, bpp=4, groups=1),
             (1, 2, 4, 4097): dict(stats=16, vec=True, K=2, bpp=5, groups=1),
             (2, 2, 3, 5463): dict(stats='loop', vec=False, K=2, bpp=5, groups=1),
             (1, 2, 1, 16386): dict(stats='loop', vec=False, K=2, bpp=5, groups=1),
             (65, 2, 2, 2): dict(stats=1, vec=True, K=1, bpp=1, groups=2),
             (128, 2, 1, 2): dict(stats='loop', vec=False, K=1, bpp=1, groups=2),
             (129, 1, 1, 2): dict(stats='loop', vec=False, K=1, bpp=1, groups=3),
             (1, 2, 1, 2): dict(stats='loop', vec=False, K=1, bpp=1, groups=1),
             (3, 2, 4, 4097): dict(stats=16, vec=True, K=2, bpp=5, groups=1)}
REGIMES = ['nominal', 'offset', 'constant', 'channel_masked', 'gamma_zero']
REGIME_SHAPE = (2, 3, 8, 12)
# every regime again where a channel's moments are combined across chunks (K = 2, P = 6) and across groups (P = 65)
REGIME_SHAPES = [REGIME_SHAPE, (3, 2, 4, 4097), (65, 2, 2, 2)]
# planes that take the vector route, run again with every map 4 bytes off a 16-byte boundary: one scalar block; two scalar
# apply blocks; the looped statistics kernel over two chunks
UNALIGNED_SHAPES = [(2, 3, 8, 12), (2, 2, 25, 164), (1, 2, 4, 4097)]


# ============================================================================================ layout and the float64 forms
def chan(t):
    """(N, C, H, W) -> (C, N H W) float64"""
    t = f64(t)
    return np.moveaxis(t, 1, 0).reshape(t.shape[1], -1)


def unchan(v, shape):
    n, c, h, w = shape
    return np.ascontiguousarray(np.moveaxis(np.asarray(v).reshape(c, n, h, w), 0, 1))


def col(v):
    return f64(v).reshape(-1, 1)


def stats64(x, eps=EPS, unbiased=False):
    """x (C, M) -> mean, biased variance, rstd, xhat"""
    m = x.shape[-1]
    with np.errstate(all='ignore'):
        mean = x.mean(-1, keepdims=True)
        var = ((x - mean) ** 2).sum(-1, keepdims=True) / m
        rstd = 1.0 / np.sqrt((var * m / (m - 1) if unbiased else var) + eps)
    return mean, var, rstd, (x - mean) * rstd


def running64(run_mean, run_var, mean, var, m, momentum, defect=None):
    keep, take = (momentum, 1.0 - momentum) if defect == 'momentum_swapped' else (1.0 - momentum, momentum)
    b = var if defect == 'running_biased' else var * m / (m - 1)
    return keep * col(run_mean) + take * mean, keep * col(run_var) + take * b


def bn_forward64(u, gamma_, beta, run_mean, run_var, momentum=MOMENTUM, eps=EPS, res=None, relu=False, res_bn=None,
                 defect=None):
    """the three forms in float64 -> dict(y, saved, running_mean, running_var[, saved_r, running_mean_r, running_var_r])"""
    shape = tuple(np.shape(u))
    x = chan(u)
    m = x.shape[-1]
    mean, var, rstd, xhat = stats64(x, eps, unbiased=defect == 'xhat_unbiased')
    out = {}
    v = xhat * col(gamma_) + col(beta)
    rm, rv = running64(run_mean, run_var, mean, var, m, momentum, defect)
    out.update(saved=np.stack([mean[:, 0], rstd[:, 0]]), running_mean=rm[:, 0], running_var=rv[:, 0])
    if res_bn is not None:
        g2, b2, rm2, rv2 = res_bn
        mean2, var2, rstd2, rhat = stats64(chan(res), eps, unbiased=defect == 'xhat_unbiased')
        v = v + (rhat * col(g2) + col(b2))
        rm2, rv2 = running64(rm2, rv2, mean2, var2, m, momentum, defect)
        out.update(saved_r=np.stack([mean2[:, 0], rstd2[:, 0]]), running_mean_r=rm2[:, 0], running_var_r=rv2[:, 0])
    elif res is not None:
        v = v + chan(res)
    out['y'] = unchan(np.maximum(v, 0.0) if relu else v, shape)
    return out


def bn_grad64(g, u, gamma_, eps=EPS, y=None, r=None, gamma_r=None, defect=None, pre=None):
    """the three backward forms in float64 -> dict(du, dgamma, dbeta[, gp][, dr, dgamma_r, dbeta_r]).  ``defect``: one
    planted mistake; 'mask_from_xhat' masks with ``pre`` (a recomputed pre-activation) where the kernel reads the kept y."""
    shape = tuple(np.shape(g))
    G, X = chan(g), chan(u)
    m = X.shape[-1]
    with np.errstate(all='ignore'):
        if y is None:
            gp = G
        else:
            gp = np.where((chan(pre) if defect == 'mask_from_xhat' else chan(y)) > 0, G, 0.0)
        _, _, rstd, xhat = stats64(X, eps, unbiased=defect == 'xhat_unbiased')
        s1 = gp.sum(-1, keepdims=True)
        s2 = (gp * xhat).sum(-1, keepdims=True)
        if r is not None:
            _, _, rstd_r, rhat = stats64(chan(r), eps, unbiased=defect == 'xhat_unbiased')
            s2r = (gp * rhat).sum(-1, keepdims=True)
            if defect == 'S2_swapped':
                s2, s2r = s2r, s2

        def du(xh, rs, s, gam):
            t = (gp - s1 / m) - (0.0 if defect == 'S2_dropped' else xh * (s / m))
            return t * (rs if defect == 'gamma_missing' else col(gam) * rs)

        out = dict(du=unchan(du(xhat, rstd, s2, gamma_), shape), dgamma=s2[:, 0], dbeta=s1[:, 0])
        if y is not None and r is None:
            out['gp'] = unchan(gp, shape)
        if r is not None:
            out.update(dr=unchan(du(rhat, rstd_r, s2r, gamma_r), shape), dgamma_r=s2r[:, 0], dbeta_r=s1[:, 0])
    return out


# ================================================================================================ the derived bound
def bn_depths(n, hw, aligned=True):
    """(D, L, D of a backward sum) of the kernels' order for planes of ``hw`` elements in a batch of ``n``"""
    cnt, k = min(hw, CHUNK), -(-hw // CHUNK)
    per = -(-cnt // (4 * 256)) + 2 if aligned and hw % 4 == 0 else -(-cnt // 256)
    d = per + 6 + 2
    groups = -(-(n * k) // 64)
    return d, 6 + groups, d + groups + 6


def torch_depths(n, hw):
    d, _, dg = bn_depths(n, hw)
    return n * hw - 1 + d, 0, n * hw - 1 + dg


def _operand_ev(x, d, levels, eps=EPS):
    """x (C, M) -> EV of mean, of the biased variance's relative error (a plain array), of rstd and of xhat"""
    with np.errstate(all='ignore'):
        mean, var, rstd, xhat = stats64(x, eps)
        ea = (d + 1) * U * np.abs(x).mean(-1, keepdims=True) + 4 * levels * U * np.abs(x).max(-1, keepdims=True)
        em = ea * rstd
        rho_lin = 0.5 * (d + 4 + 5 * levels) * U + 5 * U
        rho = rho_lin + 0.5 * em * em + 2 * em
        return (EV(mean, ea), 2 * rho + 2 * U, EV(rstd, rstd * rho * (1 + rho_lin)),
                EV(xhat, (em + np.abs(xhat) * rho) * (1 + rho_lin)))


def _running_ev(run_mean, run_var, mean, var_rel, x, momentum):
    m = x.shape[-1]
    _, var, _, _ = stats64(x)
    unb = var * m / (m - 1)
    keep = EV(1.0) - EV(float(np.float32(momentum)))
    take = EV(float(np.float32(momentum)))
    rm = keep * EV(col(run_mean)) + take * mean
    rv = keep * EV(col(run_var)) + take * EV(unb, unb * var_rel)
    return rm, rv


def _f32(v):
    return f64(np.asarray(v, dtype=np.float32))


def bn_forward_ref(u, gamma_, beta, run_mean, run_var, momentum=MOMENTUM, eps=EPS, res=None, relu=False, res_bn=None,
                   depths=None):
    """-> {output: (float64 value, bound)} for an fp32 evaluation in the kernel's order (``depths``: another order's)"""
    shape = tuple(np.shape(u))
    n, _, h, w = shape
    d, levels, _ = bn_depths(n, h * w) if depths is None else depths
    # the float64 truth normalises with the fp32 number momentum is handed over as
    val = bn_forward64(u, gamma_, beta, run_mean, run_var, float(np.float32(momentum)), eps, res, relu, res_bn)
    x = chan(u)
    mean, var_rel, rs, xh = _operand_ev(x, d, levels, eps)
    v = xh * EV(col(gamma_)) + EV(col(beta))
    rm, rv = _running_ev(run_mean, run_var, mean, var_rel, x, momentum)
    bound = dict(saved=np.stack([mean.e[:, 0], rs.e[:, 0]]), running_mean=rm.e[:, 0], running_var=rv.e[:, 0])
    if res_bn is not None:
        g2, b2, rm2, rv2 = res_bn
        xr = chan(res)
        mean2, var_rel2, rs2, rh = _operand_ev(xr, d, levels, eps)
        v = v + (rh * EV(col(g2)) + EV(col(b2)))
        rm2, rv2 = _running_ev(rm2, rv2, mean2, var_rel2, xr, momentum)
        bound.update(saved_r=np.stack([mean2.e[:, 0], rs2.e[:, 0]]), running_mean_r=rm2.e[:, 0], running_var_r=rv2.e[:, 0])
    elif res is not None:
        v = v + EV(chan(res))
    bound['y'] = unchan(v.e, shape)                               # max(., 0) does not widen it
    return {k: (val[k], bound[k]) for k in val}


def _sum_ev(t, depth):
    with np.errstate(all='ignore'):
        e = t.e.sum(-1, keepdims=True)
        return EV(t.v.sum(-1, keepdims=True), e + gamma(depth) * (np.abs(t.v).sum(-1, keepdims=True) + e))


def bn_grad_ref(g, u, gamma_, eps=EPS, y=None, r=None, gamma_r=None, depths=None):
    """-> {output: (float64 value, bound)} of the backward form the operands select"""
    shape = tuple(np.shape(g))
    n, _, h, w = shape
    d, levels, dg = bn_depths(n, h * w) if depths is None else depths
    val = bn_grad64(g, u, gamma_, eps, y, r, gamma_r)
    G = chan(g)
    m = float(G.shape[-1])
    gp = EV(G if y is None else np.where(chan(y) > 0, G, 0.0))
    s1 = _sum_ev(gp, dg)

    def operand(x, gam):
        _, _, rs, xh = _operand_ev(chan(x), d, levels, eps)
        s2 = _sum_ev(gp * xh, dg)
        m1, m2 = s1 / EV(m), s2 / EV(m)
        m1.e, m2.e = m1.e + U * np.abs(m1.v), m2.e + U * np.abs(m2.v)         # EV's quotient of exact values is exact
        return ((gp - m1) - xh * m2) * (EV(col(gam)) * rs), s2

    with np.errstate(all='ignore'):
        du, s2 = operand(u, gamma_)
        bound = dict(du=unchan(du.e, shape), dgamma=s2.e[:, 0], dbeta=s1.e[:, 0])
        if 'gp' in val:
            bound['gp'] = np.zeros(shape)                           # a select: exact
        if r is not None:
            dr, s2r = operand(r, gamma_r)
            bound.update(dr=unchan(dr.e, shape), dgamma_r=s2r.e[:, 0], dbeta_r=s1.e[:, 0])
    return {k: (val[k], bound[k]) for k in val}


# ======================================================================================================= the cases
def _rand(shape, seed, scale=1.0):
    return torch.from_numpy((np.random.RandomState(seed).standard_normal(shape) * scale).astype(np.float32))


def bn_case(form, shape, seed=0, regime='nominal'):
    """fp32 operands of one form -> dict(u, gamma, beta, running_mean, running_var[, res][, res_bn], g, y): ``y`` is what
    an fp32 forward in float64's order gives, ``g`` the cotangent the backward of the form receives (the mid form's
    masked as its consumer's epilogue masks it)"""
    n, c, h, w = shape
    s = 4000 + 31 * seed + 1000 * FORMS.index(form) + 7 * (n * c * h * w % 1009)
    u = 0.5 + 2.0 * _rand(shape, s)
    if regime == 'offset':
        u = 1e3 + _rand(shape, s)
    elif regime == 'constant':
        u = torch.full(shape, 3.7)
    vec = lambda k, lo, sc: (lo + sc * _rand((c,), s + k)).contiguous()      # noqa: E731
    case = dict(u=u, gamma=vec(1, 1.0, 0.3), beta=vec(2, 0.1, 0.5), running_mean=vec(3, 0.0, 0.5),
                running_var=(1.0 + 0.3 * _rand((c,), s + 4)).abs() + 0.1)
    if regime == 'gamma_zero':
        case['gamma'] = torch.zeros(c)
    if regime == 'channel_masked':                                  # channel 0 far below zero: every y of it is 0
        case['beta'][0] = -50.0
    if form == 'tail':
        case['res'] = _rand(shape, s + 5)
    if form == 'tail_ds':
        case['res'] = 0.3 + 1.5 * _rand(shape, s + 5)
        case['res_bn'] = (vec(6, 1.0, 0.3), vec(7, -0.1, 0.5), vec(8, 0.0, 0.5), (1.0 + 0.3 * _rand((c,), s + 9)).abs() + 0.1)
        if regime == 'gamma_zero':
            case['res_bn'] = (torch.zeros(c),) + case['res_bn'][1:]
        if regime == 'channel_masked':
            case['res_bn'][1][0] = -50.0
    case['y'] = torch.from_numpy(bn_forward64(**forward_args(case), relu=True)['y'].astype(np.float32))
    g = _rand(shape, s + 10)
    case['g'] = torch.where(case['y'] > 0, g, torch.zeros(())) if form == 'mid' else g
    return case


def forward_args(case):
    """(``gamma_``: this file's ``gamma`` is the rounding-error function)"""
    named = dict(u='u', gamma='gamma_', beta='beta', running_mean='run_mean', running_var='run_var', res='res', res_bn='res_bn')
    return {arg: case[k] for k, arg in named.items() if k in case}


def grad_args(case):
    """the operands of the backward form: the mid form takes no y (its g is masked already)"""
    a = dict(g=case['g'], u=case['u'], gamma_=case['gamma'])
    if 'res' in case:
        a['y'] = case['y']
    if 'res_bn' in case:
        a.update(r=case['res'], gamma_r=case['res_bn'][0])
    return a


ALL_CASES = ([(form, shape, 'nominal') for form in FORMS for shape in SHAPES]
             + [(form, shape, regime) for shape in REGIME_SHAPES for form in FORMS for regime in REGIMES
                if regime != 'nominal' or shape not in SHAPES])


def case_id(v):
    form, shape, regime = v
    return f'{form}-{"x".join(map(str, shape))}-{regime}'


# ===================================================================================================== torch, fp32 and fp64
def torch_bn(case, dtype):
    """F.batch_norm(training=True) forward and autograd of the form -> (forward dict, backward dict), keyed as the refs"""
    t = lambda v: v.detach().clone().to(dtype)                     # noqa: E731
    u = t(case['u']).requires_grad_(True)
    ga, be = t(case['gamma']).requires_grad_(True), t(case['beta']).requires_grad_(True)
    rm, rv = t(case['running_mean']), t(case['running_var'])
    v = F.batch_norm(u, rm, rv, ga, be, True, MOMENTUM, EPS)
    fwd = dict(running_mean=rm, running_var=rv)
    leaves = dict(du=u, dgamma=ga, dbeta=be)
    if 'res_bn' in case:
        r = t(case['res']).requires_grad_(True)
        g2, b2 = t(case['res_bn'][0]).requires_grad_(True), t(case['res_bn'][1]).requires_grad_(True)
        rm2, rv2 = t(case['res_bn'][2]), t(case['res_bn'][3])
        v = v + F.batch_norm(r, rm2, rv2, g2, b2, True, MOMENTUM, EPS)
        fwd.update(running_mean_r=rm2, running_var_r=rv2)
        leaves.update(dr=r, dgamma_r=g2, dbeta_r=b2)
    elif 'res' in case:
        res = t(case['res']).requires_grad_(True)
        v = v + res
        leaves['gp'] = res
    fwd['y'] = torch.relu(v).detach()
    g = t(case['g'])
    gp = g if 'res' not in case else torch.where(case['y'] > 0, g, torch.zeros_like(g))
    (v * gp).sum().backward()                                       # the ReLU decisions are the kept y's, as the kernel's
    return fwd, {k: leaf.grad for k, leaf in leaves.items()}


@pytest.mark.parametrize('case', ALL_CASES, ids=case_id)
def test_forms_equal_float64_torch_and_fp32_torch_falls_inside(case):
    form, shape, regime = case
    c = bn_case(form, shape, regime=regime)
    n, _, h, w = shape
    depths = torch_depths(n, h * w)
    fref = bn_forward_ref(**forward_args(c), relu=True, depths=depths)
    gref = bn_grad_ref(**grad_args(c), depths=depths)
    f64_, g64_ = torch_bn(c, torch.float64)
    f32_, g32_ = torch_bn(c, torch.float32)
    assert sorted(g64_) == sorted(gref)
    worst = 0.0
    # the restatement is torch's float64 result; torch's momentum is the double 0.1, the kernel's (and the bound's centre)
    # the fp32 number next to it, so the running statistics are compared at the double
    own = dict(bn_forward64(**forward_args(c), momentum=MOMENTUM, relu=True), **{k: v[0] for k, v in gref.items()})
    for ref, want, got in ((fref, f64_, f32_), (gref, g64_, g32_)):
        for k in want:
            scale = max(float(want[k].abs().max()), 1.0)
            tol = 1e-9 if regime != 'constant' else 1e-6
            assert float(np.abs(own[k] - f64(want[k])).max()) <= tol * scale, (case, k)
            assert np.isfinite(ref[k][1]).all() and (ref[k][1] >= 0).all(), (case, k)
            worst = max(worst, worst_ratio(got[k], *ref[k]))
    measured(f'fp32 torch batch_norm(training=True) and autograd, {case_id(case)}: worst error / bound', worst)
    assert worst <= 1


# ============================================================================= fp32 in the kernels' own operation order
F32 = np.float32


def _chain(terms):
    """(B, n) fp32 -> (B, 256): thread t of the workgroup adds terms t, t + 256, ... to one chain from +0"""
    b, n = terms.shape
    its = -(-n // 256)
    pad = np.zeros((b, its * 256), F32)
    pad[:, :n] = terms
    acc = np.zeros((b, 256), F32)
    for i in range(its):
        acc = acc + pad[:, i * 256:(i + 1) * 256]
    return acc


def _wave(v):
    """(B, 64) -> (B,): v[l] += v[l ^ off] for off = 32, ..., 1 (bnt_wave_sum); every lane ends with the same bits"""
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lanes ^ off]
    return v[:, 0]


def _block(v):
    """(B, 256) -> (B,): the four waves, then (w0 + w1) + (w2 + w3) (bnt_block_sum)"""
    w = _wave(v.reshape(-1, 64)).reshape(-1, 4)
    return (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])


def _quad(t):
    """(B, 4 m) -> (B, m): a float4's terms as (a + b) + (c + d)"""
    q = t.reshape(t.shape[0], -1, 4)
    return (q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3])


def _chunk_sum(terms, vec):
    return _block(_chain(_quad(terms) if vec else terms))


def _chan32(a, b):
    """bnt_chan on (..., 3) arrays of (count, mean, m2); a holds the lower partial indices"""
    with np.errstate(all='ignore'):
        n = a[..., 0] + b[..., 0]
        d = b[..., 1] - a[..., 1]
        f = b[..., 0] / n
        r = np.stack([n, a[..., 1] + d * f, (a[..., 2] + b[..., 2]) + (d * d) * (a[..., 0] * f)], -1)
    r = np.where((a[..., :1] == 0), b, r)
    return np.where((b[..., :1] == 0), a, r).astype(F32)


def _moments32(ws):
    """ws (N, C, K, 3) -> (C, 3): bnt_channel_moments, groups of 64 partials p = n K + k in a tree whose lower lane is the
    left operand at every level, the groups folded in ascending order"""
    n, c, k, _ = ws.shape
    part = np.moveaxis(ws, 1, 0).reshape(c, n * k, 3)
    acc = np.zeros((c, 3), F32)
    for p0 in range(0, n * k, 64):
        m = np.zeros((c, 64, 3), F32)
        m[:, :min(64, n * k - p0)] = part[:, p0:p0 + 64]
        while m.shape[1] > 1:
            m = _chan32(m[:, 0::2], m[:, 1::2])
        acc = _chan32(acc, m[:, 0])
    return acc


def _stats32(x, vec, K):
    """x (N, C, HW) fp32 -> the workspace (N, C, K, 3) of the statistics pass: per chunk the count, the mean, then the sum of
    the squared differences from it"""
    n, c, hw = x.shape
    planes = x.reshape(n * c, hw)
    ws = np.zeros((n * c, K, 3), F32)
    for k in range(K):
        ch = planes[:, k * CHUNK:(k + 1) * CHUNK]
        cnt = F32(ch.shape[1])
        mean = _chunk_sum(ch, vec) / cnt
        a = ch - mean[:, None]
        ws[:, k] = np.stack([np.full_like(mean, cnt), mean, _chunk_sum(a * a, vec)], -1)
    return ws.reshape(n, c, K, 3)


def _np32(t):
    return np.ascontiguousarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, dtype=F32)


def bn_forward32(case, vec, K, momentum=MOMENTUM, eps=EPS):
    """batch_norm_train.hip's forward with relu in numpy fp32, every operation rounded on its own, in the order of the
    route (``vec``, ``K`` chunks per plane) -> dict keyed as bn_forward64"""
    shape = tuple(case['u'].shape)
    n, c, h, w = shape
    mom, eps = F32(momentum), F32(eps)
    one = F32(1)

    def operand(x, gam, bet, rm, rv):
        x = _np32(x).reshape(n, c, h * w)
        m = _moments32(_stats32(x, vec, K))
        mean = m[:, 1]
        rstd = one / np.sqrt(m[:, 2] / m[:, 0] + eps)
        keep, unb = one - mom, m[:, 2] / (m[:, 0] - one)
        B = lambda v: _np32(v).reshape(1, c, 1)                    # noqa: E731
        v = ((x - B(mean)) * B(rstd)) * B(gam) + B(bet)
        return v, np.stack([mean, rstd]), keep * _np32(rm) + mom * mean, keep * _np32(rv) + mom * unb

    with np.errstate(all='ignore'):
        v, saved, rm, rv = operand(case['u'], case['gamma'], case['beta'], case['running_mean'], case['running_var'])
        out = dict(saved=saved, running_mean=rm, running_var=rv)
        if 'res_bn' in case:
            v2, saved_r, rm2, rv2 = operand(case['res'], *case['res_bn'])
            v = v + v2
            out.update(saved_r=saved_r, running_mean_r=rm2, running_var_r=rv2)
        elif 'res' in case:
            v = v + _np32(case['res']).reshape(n, c, h * w)
        out['y'] = np.where(v > 0, v, F32(0)).reshape(shape)
    assert all(v.dtype == F32 for v in out.values())
    return out


def bn_grad32(case, fwd, vec, K):
    """batch_norm_train.hip's backward in numpy fp32 on the forward ``fwd`` (its saved statistics; the mask is read from
    ``case['y']``) -> dict keyed as bn_grad64"""
    shape = tuple(case['u'].shape)
    n, c, h, w = shape
    hw = h * w
    flat = lambda v: _np32(v).reshape(n, c, hw)                    # noqa: E731
    B = lambda v: _np32(v).reshape(1, c, 1)                        # noqa: E731
    g, u = flat(case['g']), flat(case['u'])
    tail, ds = 'res' in case, 'res_bn' in case
    with np.errstate(all='ignore'):
        gm = np.where(flat(case['y']) > 0, g, F32(0)) if tail else g
        ops_ = [(u, fwd['saved'], case['gamma'])] + ([(flat(case['res']), fwd['saved_r'], case['res_bn'][0])] if ds else [])
        xh = [(x - B(sv[0])) * B(sv[1]) for x, sv, _ in ops_]
        ws = np.zeros((n * c, K, 3), F32)
        for k in range(K):
            sl = slice(k * CHUNK, (k + 1) * CHUNK)
            terms = [gm[..., sl]] + [gm[..., sl] * t[..., sl] for t in xh]
            for j, t in enumerate(terms):
                ws[:, k, j] = _chunk_sum(t.reshape(n * c, -1), vec)
        part = np.moveaxis(ws.reshape(n, c, K, 3), 1, 0).reshape(c, n * K, 3)
        its = -(-(n * K) // 64)
        pad = np.zeros((c, its * 64, 3), F32)
        pad[:, :n * K] = part
        acc = np.zeros((c, 64, 3), F32)
        for i in range(its):                                        # lane l adds p = l, l + 64, ... to one chain from +0
            acc = acc + pad[:, i * 64:(i + 1) * 64]
        s = np.stack([_wave(acc[..., j]) for j in range(3)], -1)    # (C, 3)
        M = F32(n * hw)
        m1 = s[:, 0] / M

        def grad(x_hat, sv, gam, s2):
            return ((gm - B(m1)) - x_hat * B(s2 / M)) * B(_np32(gam) * sv[1])

        out = dict(du=grad(xh[0], fwd['saved'], case['gamma'], s[:, 1]).reshape(shape), dgamma=s[:, 1], dbeta=s[:, 0])
        if tail and not ds:
            out['gp'] = gm.reshape(shape)
        if ds:
            out.update(dr=grad(xh[1], fwd['saved_r'], case['res_bn'][0], s[:, 2]).reshape(shape), dgamma_r=s[:, 2], dbeta_r=s[:, 0])
    assert all(v.dtype == F32 for v in out.values())
    return out


def kernel_order_case(case, form, vec, K):
    """``case`` with y, and the mid form's mask, taken from the fp32 forward in the kernel's order, as the encoder has them
    -> (case, that forward)"""
    fwd = bn_forward32(case, vec, K)
    case = dict(case, y=torch.from_numpy(fwd['y']))
    if form == 'mid':
        case['g'] = torch.where(case['y'] > 0, _rand(tuple(case['u'].shape), 99), torch.zeros(()))
    return case, fwd


ORDER_CASES = [(c, True) for c in ALL_CASES] + [((form, shape, 'nominal'), False) for form in FORMS for shape in UNALIGNED_SHAPES]


@pytest.mark.parametrize('case, aligned', ORDER_CASES, ids=lambda v: case_id(v) if isinstance(v, tuple) else ('aligned' if v else 'off16'))
def test_fp32_in_the_kernels_order_is_inside_the_bound(case, aligned):
    """the forward and the backward restated in fp32 in the order of the route the library itself names for the shape
    (ops.batch_norm_train_route, a host call), against float64 and the bound at that route's depth"""
    from scflow_amd import ops
    form, shape, regime = case
    n, ch, h, w = shape
    route = ops.batch_norm_train_route(n, ch, h * w, aligned)
    assert route['vec'] == (aligned and h * w % 4 == 0) and route['K'] == -(-h * w // CHUNK) and route['groups'] == -(-n * route['K'] // 64)
    c, fwd = kernel_order_case(bn_case(form, shape, regime=regime), form, route['vec'], route['K'])
    got = bn_grad32(c, fwd, route['vec'], route['K'])
    depths = bn_depths(n, h * w, aligned)
    fref = bn_forward_ref(**forward_args(c), relu=True, depths=depths)
    gref = bn_grad_ref(**grad_args(c), depths=depths)
    assert sorted(fwd) == sorted(fref) and sorted(got) == sorted(gref)
    worst = {k: worst_ratio(have[k], *ref[k]) for have, ref in ((fwd, fref), (got, gref)) for k in ref}
    measured(f'fp32 in the kernel\'s order, {case_id(case)} {"aligned" if aligned else "4 bytes off"}: worst error / bound',
             max(worst.values()))
    assert max(worst.values()) <= 1, worst
    assert all(np.isfinite(v).all() for v in list(fwd.values()) + list(got.values()))


def test_route_coverage():
    """the library's own route decision over every case the kernel tests run (tests/test_gpu_bn_train.py runs ALL_CASES
    aligned and UNALIGNED_SHAPES 4 bytes off): each added shape lands where it was put, and every statistics kernel, float4
    and scalar sweeps, one and several chunks per plane, one and several apply blocks per plane, one and several groups of
    partials are each reached by a case of each form"""
    from scflow_amd import ops
    route = lambda shape, aligned=True: ops.batch_norm_train_route(shape[0], shape[1], shape[2] * shape[3], aligned)   # noqa: E731
    for shape, want in ROUTE_WHY.items():
        assert shape in [s for _, s, _ in ALL_CASES] and route(shape) == want, (shape, route(shape))
    assert [route(s, False) for s in UNALIGNED_SHAPES] == [dict(stats='loop', vec=False, K=1, bpp=1, groups=1),
                                                          dict(stats='loop', vec=False, K=1, bpp=2, groups=1),
                                                          dict(stats='loop', vec=False, K=2, bpp=5, groups=1)]
    for form in FORMS:
        seen = [route(s) for f, s, _ in ALL_CASES if f == form] + [route(s, False) for s in UNALIGNED_SHAPES]
        for key, values in (('stats', (1, 4, 16, 'loop')), ('vec', (True, False))):
            assert {r[key] for r in seen} == set(values), (form, key)
        for key in ('K', 'bpp', 'groups'):
            assert {min(r[key], 2) for r in seen} == {1, 2}, (form, key)
        # the combinations a single property does not pin down
        has = lambda **kw: any(all(r[k] == v if k in ('stats', 'vec') else (r[k] > 1) == v for k, v in kw.items()) for r in seen)  # noqa: E731
        assert has(vec=False, bpp=True) and has(vec=True, bpp=True) and has(stats='loop', K=True) and has(stats=16, K=True)
        assert has(vec=False, groups=True) and has(vec=True, groups=True)
    # the regimes meet the combination across chunks and across groups
    for regime in REGIMES:
        seen = [route(s) for _, s, r in ALL_CASES if r == regime]
        assert any(r['K'] > 1 for r in seen) and any(r['groups'] > 1 for r in seen), regime
    # a size the kernels do not take is the entries' own error code
    from scflow_amd._lib import ScflowHipError
    for bad in ((1, 1, 1, 1), (0, 1, 2, 2), (2 ** 10, 1, 1, 2 ** 15)):
        with pytest.raises(ScflowHipError):
            route(bad)


def test_bound_is_tight_where_it_matters():
    """nominal data: a few hundred U of the output's scale at the kernel's own depth, so a defect of first order cannot hide"""
    c = bn_case('tail_ds', (4, 64, 16, 16))
    f = bn_forward_ref(**forward_args(c), relu=True)
    g = bn_grad_ref(**grad_args(c))
    assert float(f['y'][1].max()) <= 2000 * U * float(np.abs(f['y'][0]).max())
    assert float(g['du'][1].max()) <= 2000 * U * float(np.abs(g['du'][0]).max())
    assert float(f['running_var'][1].max()) <= 2000 * U


# ================================================================================================ planted defects
PLANTED = [('running_biased', 'mid', 'running_var'), ('xhat_unbiased', 'mid', 'y'), ('xhat_unbiased', 'mid', 'du'),
           ('momentum_swapped', 'mid', 'running_mean'), ('S2_dropped', 'mid', 'du'), ('gamma_missing', 'tail', 'du'),
           ('mask_from_xhat', 'tail', 'gp'), ('mask_from_xhat', 'tail', 'du'), ('S2_swapped', 'tail_ds', 'du'),
           ('S2_swapped', 'tail_ds', 'dr'), ('S2_swapped', 'tail_ds', 'dgamma')]


def disagreeing_cell(case):
    """the kept y of ``case`` with the smallest positive pre-activation's cell set to 0 -- an fp32 forward that rounded it
    the other way -- and the float64 pre-activation that a recomputed mask would read"""
    pre = bn_forward64(**forward_args(case), relu=False)['y']
    y = case['y'].clone()
    flat = np.where(pre > 0, pre, np.inf).reshape(-1)
    cell = int(flat.argmin())
    y.view(-1)[cell] = 0.0
    assert pre.reshape(-1)[cell] > 0 and case['g'].view(-1)[cell] != 0
    return y, pre


@pytest.mark.parametrize('defect,form,key', PLANTED, ids=lambda v: str(v))
def test_planted_defects_outside(defect, form, key):
    """each against the bound at the kernel's own depth, at (3, 5, 2, 3): 18 values a channel, Bessel's correction 1 / 17"""
    c = bn_case(form, (3, 5, 2, 3), seed=3)
    pre = None
    if defect == 'mask_from_xhat':
        c['y'], pre = disagreeing_cell(c)
    if key in ('y', 'running_mean', 'running_var'):
        ref = bn_forward_ref(**forward_args(c), relu=True)
        bad = bn_forward64(**forward_args(c), momentum=float(np.float32(MOMENTUM)), relu=True, defect=defect)
    else:
        ref = bn_grad_ref(**grad_args(c))
        bad = bn_grad64(**grad_args(c), defect=defect, pre=pre)
    worst = worst_ratio(bad[key], *ref[key])
    measured(f'planted defect {defect} ({form}), {key}: error / bound', worst)
    assert worst >= 10


# ====================================================================================================== the C ABI
def test_symbols_are_declared_exported_and_bound():
    from scflow_amd import _lib
    for name in SYMBOLS:
        assert f'{name}(' in HEADER and f'extern "C" int{"64_t" if name.endswith("workspace") else ""} {name}(' in SRC, name
        assert name in _lib.SIGNATURES, name
    body = SRC.split('#include')[1]
    assert 'atomic' not in body and '#pragma clang fp contract(off)' in body
    assert "'batch_norm_train.hip'" in open(os.path.join(ROOT, 'scflow_amd', 'csrc', 'build.py')).read()
    assert 'scf_batch_norm_train' in open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    import re
    assert re.search(r'#define SCF_VERSION \(SCF_ABI_MAJOR \* 100 \+ 3\)', HEADER)          # no bump


def test_c_abi_rejects_bad_arguments_before_any_launch():
    """every refusal returns before the stream is touched, so this runs without a GPU"""
    from scflow_amd import _lib
    import ctypes as C
    lib = _lib.load()
    buf = (C.c_float * 256)()
    p = C.cast(buf, C.c_void_p)
    odd = C.c_void_p(p.value + 2)                                   # not 4-byte aligned
    E, EUNSUP = -1, -2                          # scflow_hip.h: SCF_EINVAL, SCF_EUNSUPPORTED
    ws = lib.scf_batch_norm_train_workspace
    assert ws(2, 3, 8) == 6 * 6 and ws(2, 3, CHUNK + 4) == 6 * 12 and ws(1, 2, 16) == 12
    assert ws(0, 3, 8) == E and ws(2, 0, 8) == E and ws(2, 3, -1) == E and ws(1, 4, 1) == E and ws(2, 4, 1) == 6 * 8
    assert ws(2 ** 10, 1, 2 ** 15) == EUNSUP

    def fwd(u=p, gamma_=p, beta=p, rm=p, rv=p, res=None, g2=None, b2=None, rm2=None, rv2=None, y=p, saved=p, saved_r=None,
            w=p, wf=256, n=2, c=3, hw=8):
        return lib.scf_batch_norm_train(u, gamma_, beta, rm, rv, res, g2, b2, rm2, rv2, 1, 0.1, 1e-5, y, saved, saved_r, w, wf,
                                        n, c, hw, None)

    for bad in (dict(u=None), dict(gamma_=None), dict(beta=None), dict(y=None), dict(saved=None), dict(w=None), dict(rm=None),
                dict(rv=None), dict(n=0), dict(c=-1), dict(hw=0), dict(n=1, hw=1), dict(wf=35), dict(u=odd), dict(y=odd),
                dict(saved=odd), dict(b2=p), dict(saved_r=p), dict(rm2=p),
                dict(g2=p), dict(g2=p, res=p, b2=p), dict(g2=p, res=p, saved_r=p), dict(g2=p, res=p, b2=p, saved_r=p, rm2=p)):
        assert fwd(**bad) == E, bad
    assert fwd(n=2 ** 10, c=1, hw=2 ** 15) == EUNSUP

    def bwd(g=p, y=None, u=p, r=None, saved=p, saved_r=None, gamma_=p, gamma_r=None, gp=None, du=p, dr=None, dg=p, db=p,
            dg2=None, db2=None, w=p, wf=256, n=2, c=3, hw=8):
        return lib.scf_batch_norm_train_grad(g, y, u, r, saved, saved_r, gamma_, gamma_r, gp, du, dr, dg, db, dg2, db2, 0, w, wf,
                                             n, c, hw, None)

    ds = dict(y=p, r=p, saved_r=p, gamma_r=p, dr=p, dg2=p, db2=p)
    for bad in (dict(g=None), dict(u=None), dict(saved=None), dict(gamma_=None), dict(du=None), dict(dg=None), dict(db=None),
                dict(w=None), dict(y=p), dict(gp=p), dict(saved_r=p), dict(dr=p), dict(dg2=p), dict(n=0), dict(hw=-3),
                dict(n=1, hw=1), dict(wf=35), dict(g=odd), dict(du=odd), dict(ds, gp=p), dict(ds, y=None),
                dict(ds, saved_r=None), dict(ds, gamma_r=None), dict(ds, dr=None), dict(ds, db2=None)):
        assert bwd(**bad) == E, bad
    assert bwd(n=2 ** 10, c=1, hw=2 ** 15) == EUNSUP
    assert not any(buf)


# ============================================================================================= the Python surface
def _model(**over):
    import scflow_amd
    cfg = scflow_amd.scflow_model_cfg(iters=2)
    cfg.update(over)
    return scflow_amd.build_refiner(cfg)


def test_network_parameters_and_build_optimizer():
    from scflow_amd import optim
    m = _model()                                                    # the shipped flags
    assert m.freeze_encoder is False and m.freeze_bn is False
    named = m.network_parameters()
    assert [n for n, _ in named] == [n for n, _ in m.named_parameters()] and len(named) == 149
    assert sum(n.startswith('context.') for n, _ in named) == 62 and sum(n.startswith('render_encoder.') for n, _ in named) == 32
    frozen = _model(freeze_encoder=True)
    assert [n for n, _ in frozen.network_parameters()] == [n for n, _ in frozen.trainable_parameters()]
    assert len(frozen.network_parameters()) == 117
    cfgs = (dict(type='AdamW', lr=4e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4), dict(grad_clip=dict(max_norm=10.)))
    opt = optim.build_optimizer(m, *cfgs, network=True)
    assert opt.names == [n for n, _ in named] and all(a is b for a, (_, b) in zip(opt.params, named))
    assert optim.build_optimizer(m, *cfgs).names == [n for n, _ in m.trainable_parameters()]        # the default stays
    with pytest.raises(ValueError, match='network_parameters'):
        m.train_step_network(None, optim.build_optimizer(m, *cfgs), data={})
    with pytest.raises(TypeError, match='scflow_amd.optim.AdamW'):
        m.train_step_network(None, torch.optim.AdamW(m.parameters()), data={})


def test_switches_are_off_by_default_and_refuse_by_name():
    m = _model()
    ctx, feat = m.context, m.render_encoder
    assert ctx.batch is False and feat.batch is False
    with m.batch_norm_training() as inside:
        assert inside is m and ctx.batch is True and feat.batch is False
        with ctx.batch_stats():
            assert ctx.batch is True
        assert ctx.batch is True                                    # a setting of the caller's stays
    assert ctx.batch is False
    with pytest.raises(NotImplementedError, match='InstanceNorm encoder has no batch statistics'):
        with feat.batch_stats():
            pass
    with pytest.raises(NotImplementedError, match='InstanceNorm encoder takes RAFTEncoder.in_backward'):
        feat.bn_backward({}, torch.zeros(1))
    from scflow_amd import ops
    with pytest.raises(NotImplementedError, match='momentum=None'):
        ops.batch_norm_train(torch.zeros(2, 1, 2, 2), torch.ones(1), torch.zeros(1), None, None, momentum=None)


def test_kept_keys_of_the_three_norm_kinds():
    """what a keeping forward leaves and a backward reads, per norm kind: the sets as tests/test_gpu_context_grad.py,
    tests/test_gpu_feature_grad.py (KEPT_KEYS) and tests/test_gpu_bn_train.py (KEPT_KEYS) assert them on the GPU, stated
    here again and not taken from the module"""
    from scflow_amd import modules
    from scflow_amd.modules import RAFTEncoder
    walk = ['x', 'stem', 'out'] + [f'{k}{i}' for i in range(6) for k in ('t', 'y')]
    raw = ['u_stem', 'r2', 'r4'] + [f'{k}{i}' for i in range(6) for k in ('u1_', 'u2_')]
    stats = ['s_stem', 'sr2', 'sr4'] + [f'{k}{i}' for i in range(6) for k in ('s1_', 's2_')]
    assert len(walk) == 15 and len(raw) == 15 and len(stats) == 15
    ctx, feat = (RAFTEncoder(3, 8, norm_cfg=dict(type=kind)) for kind in ('BN', 'IN'))
    for enc, norm, want in ((ctx, modules._FoldedBN, walk), (feat, modules._RawIN, walk + raw),
                            (ctx, modules._BatchBN, walk + raw + stats)):
        keys = modules._kept_keys(norm, enc._blocks())
        assert sorted(keys) == sorted(want) and len(set(keys)) == len(keys), norm.__name__
        # a backward whose caller passes the head's output reads the rest
        assert modules._kept_keys(norm, enc._blocks(), out=False) == [k for k in keys if k != 'out']
    # the kind a forward runs follows the encoder's norm and its batch_stats() switch
    assert feat._norm() is modules._RawIN and ctx._norm() is modules._FoldedBN
    with ctx.batch_stats():
        assert ctx._norm() is modules._BatchBN
    assert ctx._norm() is modules._FoldedBN
    # the shortcut keys follow the blocks that have a shortcut convolution
    assert [i for i, blk in enumerate(ctx._blocks()) if blk.downsample is not None] == [2, 4]
    # the error of a backward names exactly these keys
    from scflow_amd._lib import ScflowHipError
    for enc, back, norm, out in ((ctx, ctx.backward, modules._FoldedBN, True), (ctx, ctx.bn_backward, modules._BatchBN, True),
                                 (feat, feat.in_backward, modules._RawIN, False)):
        with pytest.raises(ScflowHipError) as err:
            back({}, torch.zeros(1))
        assert f"saved holds {', '.join(modules._kept_keys(norm, enc._blocks(), out=out))}: RAFTEncoder.kept" in str(err.value)


def test_train_step_still_refuses_freeze_bn_false():
    """the additive contract: the old entry point and its words are as they were"""
    from scflow_amd import optim
    opt = optim.AdamW([('w', torch.zeros(3))])
    with pytest.raises(NotImplementedError, match='freeze_bn=False needs BatchNorm on batch statistics, forward and backward'):
        _model(freeze_encoder=True, freeze_bn=False).train_step(None, opt, data={})
    m = _model(freeze_encoder=True, freeze_bn=True)
    assert [n for n, _ in m.trainable_parameters()] == [n for n, _ in m.named_parameters()
                                                        if n.startswith(('decoder.', 'context.'))]
