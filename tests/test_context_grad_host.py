"""CPU: backward of the context encoder (encoder_grad.hip, RAFTEncoder.backward) -- every new kernel and the whole layer walk
restated in float64 with a per-element bound for any fp32 evaluation in the kernels' operation order, held against float64
autograd through ``oracle.raft_encoder(x, sd, 'context.', 'BN')`` followed by the split tanh | relu, with planted defects
that must fall outside the bounds, and against the reference's own module (a fixture).

Bounds, U = 2^-24, gamma(d) = d U / (1 - d U) (a chain of d roundings), in the manner of tests/test_conv_grad_host.py and
tests/test_head_grad_host.py: a sum evaluated as the header of encoder_grad.hip states is within gamma(d) sum |terms| of
the exact sum, d = 1 (the product) + the additions of the longest chain + (S - 1) (the combine) + 1 (accumulate); operands
that are themselves computed carry their bound in linearly (first order in their error, times 1 + gamma(d)).

  stem wgrad     d = 1 + EW_PIX min(cps, chunks) + (S - 1) [+ 1]
  ds wgrad       the same with its own plan
  ds dgrad       d = 1 + 32 ceil(Cout / 32), then one rounding for `+ add`, then the activation factor
  channel sum    d = ceil(min(per, Q) / 256) + log2(256) + (S - 1) [+ 1]
  fold           s = gamma / sqrt(var + eps): eps as an fp32 number, the sum, the root, the quotient: 4 roundings; W' one
                 more (5); b' = fma(s, b - mean, beta): the difference and the fma on top (6)
  unfold         dW = s dW', db = s db': gamma(5) (|s| |dW'|) + |s| bound(dW'); dbeta = db' as given;
                 dgamma = fma(b - mean, db', <W, dW'>) / sd: the lane's chain ceil(K / 64), 6 tree levels, the product,
                 the difference, the fma, sd (3) and the quotient: D = ceil(K / 64) + 13,
                 gamma(D) (sum |W| |dW'| + |b - mean| |db'|) / sd + (sum |W| bound(dW') + |b - mean| bound(db')) / sd

fp32 underflow is outside the model.
"""
import os
import re

import numpy as np
import pytest
import torch

from test_stream_ops_host import f64, measured, worst_ratio  # noqa: E402
from test_fc_host import U, gamma  # noqa: E402
import test_conv_grad_host as CG  # noqa: E402
import test_head_grad_host as S1  # noqa: E402
from test_head_grad_host import NONE, RELU, TANH, act_factor, act_grad_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, 'scflow_amd', 'csrc', 'encoder_grad.hip')).read()
HEADER = open(os.path.join(ROOT, 'include', 'scflow_hip.h')).read()
F = torch.nn.functional
EPS = 1e-5
SYMBOLS = ['scf_conv_stem_wgrad_workspace', 'scf_conv_stem_wgrad', 'scf_conv_ds_dgrad', 'scf_conv_ds_wgrad_workspace',
           'scf_conv_ds_wgrad', 'scf_channel_sum_workspace', 'scf_channel_sum', 'scf_bn_fold', 'scf_bn_unfold']


def _define(name):
    return int(re.search(rf'#define\s+{name}\s+(\d+)', SRC).group(1))


EW_PIX, ST_MIN_CHUNKS, ST_SPLITS, ED_CHUNK = (_define(k) for k in ('EW_PIX', 'ST_MIN_CHUNKS', 'ST_SPLITS', 'ED_CHUNK'))
EW_TILE, EW_MIN_CHUNKS, EW_BLOCKS, CS_MIN, CS_BLOCKS, EG_THREADS = (_define(k) for k in (
    'EW_TILE', 'EW_MIN_CHUNKS', 'EW_BLOCKS', 'CS_MIN', 'CS_BLOCKS', 'EG_THREADS'))
EXTRA = 0                           # added to every depth: 0 for the kernels; raised for torch's own fp32 order


def half(n):
    return (n - 1) // 2 + 1


def cdiv(a, b):
    return -(-a // b)


# ================================================================================================ depths, from the source
def stem_plan(m, ho, wo):
    """eg_stem_cps -> (chunks per split, splits)"""
    chunks = m * ho * cdiv(wo, EW_PIX)
    cps = max(ST_MIN_CHUNKS, cdiv(chunks, ST_SPLITS))
    return cps, cdiv(chunks, cps)


def stem_depth(m, ho, wo, accumulate=False):
    cps, splits = stem_plan(m, ho, wo)
    return 1 + EW_PIX * min(cps, m * ho * cdiv(wo, EW_PIX)) + (splits - 1) + (1 if accumulate else 0) + EXTRA


def ds_plan(m, cout, cin, ho, wo):
    """eg_ds_cps -> (chunks per split, splits)"""
    chunks = m * ho * cdiv(wo, EW_PIX)
    tiles = cdiv(cout, EW_TILE) * cdiv(cin, EW_TILE)
    cps = max(EW_MIN_CHUNKS, cdiv(chunks, max(1, EW_BLOCKS // tiles)))
    return cps, cdiv(chunks, cps)


def ds_wgrad_depth(m, cout, cin, ho, wo, accumulate=False):
    cps, splits = ds_plan(m, cout, cin, ho, wo)
    return 1 + EW_PIX * min(cps, m * ho * cdiv(wo, EW_PIX)) + (splits - 1) + (1 if accumulate else 0) + EXTRA


def ds_dgrad_depth(cout):
    return 1 + ED_CHUNK * cdiv(cout, ED_CHUNK) + EXTRA


def cs_plan(q, c):
    per = max(CS_MIN, cdiv(q, max(1, CS_BLOCKS // c)))
    per = cdiv(per, EG_THREADS) * EG_THREADS
    return per, cdiv(q, per)


def cs_depth(q, c, accumulate=False):
    per, splits = cs_plan(q, c)
    return cdiv(min(per, q), EG_THREADS) + EG_THREADS.bit_length() - 1 + (splits - 1) + (1 if accumulate else 0) + EXTRA


S_ROUNDINGS, WF_ROUNDINGS, BF_ROUNDINGS = 4, 5, 6


def unfold_depth(k):
    return cdiv(k, 64) + 13 + EXTRA


# ===================================================================================================== float64 pieces
def _b(v, like):
    return np.broadcast_to(np.asarray(v, dtype=np.float64), like.shape)


def patches(x, k, pad, ho, wo):
    """x (M, C, H, W) -> (M, C, k, k, ho, wo): x[m, c, 2 oy - pad + ky, 2 ox - pad + kx], zero outside the map"""
    m, c, h, w = x.shape
    xp = np.zeros((m, c, 2 * ho + k + pad, 2 * wo + k + pad))
    xp[:, :, pad:pad + h, pad:pad + w] = x
    out = np.empty((m, c, k, k, ho, wo))
    for ky in range(k):
        for kx in range(k):
            out[:, :, ky, kx] = xp[:, :, ky:ky + 2 * ho:2, kx:kx + 2 * wo:2]
    return out


def stem_wgrad_sum(g, x, pad=3):
    return np.einsum('mohw,mckjhw->ockj', g, patches(x, 7, pad, g.shape[2], g.shape[3]), optimize=True)


def stem_wgrad_ref(g, gb, x, xb=0.0, prev=None, prev_b=None, pad=3):
    """-> (dW, its bound, db, its bound); gb, xb: bounds of g and x; prev / prev_b: what the call accumulates into"""
    g, x = f64(g), f64(x)
    gb, xb = _b(gb, g), _b(xb, x)
    m, _, ho, wo = g.shape
    gm = gamma(stem_depth(m, ho, wo, prev is not None))
    with np.errstate(all='ignore'):
        ref, sh = stem_wgrad_sum(g, x, pad), stem_wgrad_sum(np.abs(g), np.abs(x), pad)
        carried = stem_wgrad_sum(gb, np.abs(x) + xb, pad) + stem_wgrad_sum(np.abs(g), xb, pad)
        db, dsh, dcar = g.sum((0, 2, 3)), np.abs(g).sum((0, 2, 3)), gb.sum((0, 2, 3))
        if prev is not None:
            ref, sh = ref + f64(prev), sh + np.abs(f64(prev))
        if prev_b is not None:
            db, dsh = db + f64(prev_b), dsh + np.abs(f64(prev_b))
    return ref, gm * sh + carried * (1 + gm), db, gm * dsh + dcar * (1 + gm)


def ds_wgrad_sum(g, x):
    return np.einsum('mohw,mchw->oc', g, x[:, :, ::2, ::2], optimize=True)[:, :, None, None]


def ds_wgrad_ref(g, gb, x, xb=0.0, prev=None, prev_b=None):
    g, x = f64(g), f64(x)
    gb, xb = _b(gb, g), _b(xb, x)
    m, cout, ho, wo = g.shape
    gm = gamma(ds_wgrad_depth(m, cout, x.shape[1], ho, wo, prev is not None))
    with np.errstate(all='ignore'):
        ref, sh = ds_wgrad_sum(g, x), ds_wgrad_sum(np.abs(g), np.abs(x))
        carried = ds_wgrad_sum(gb, np.abs(x) + xb) + ds_wgrad_sum(np.abs(g), xb)
        db, dsh, dcar = g.sum((0, 2, 3)), np.abs(g).sum((0, 2, 3)), gb.sum((0, 2, 3))
        if prev is not None:
            ref, sh = ref + f64(prev), sh + np.abs(f64(prev))
        if prev_b is not None:
            db, dsh = db + f64(prev_b), dsh + np.abs(f64(prev_b))
    return ref, gm * sh + carried * (1 + gm), db, gm * dsh + dcar * (1 + gm)


def ds_dgrad_sum(g, w, hin, win, odd=False):
    """the shortcut's input gradient: non-zero at the even pixels (odd=True, a defect: scattered to the odd ones)"""
    gx = np.zeros((g.shape[0], w.shape[1], hin, win))
    v = np.einsum('mohw,oc->mchw', g, w.reshape(w.shape[0], w.shape[1]), optimize=True)
    if odd:
        gx[:, :, 1::2, 1::2] = v[:, :, :hin // 2, :win // 2]
    else:
        gx[:, :, 0::2, 0::2] = v
    return gx


def ds_dgrad_ref(g, gb, w, hin, win, wb=0.0, add=None, addb=0.0, a=None, act=NONE):
    """-> (gx, bound) over (M, Cin, Hin, Win); gb, wb, addb: bounds of g, w and add"""
    g, w = f64(g), f64(w)
    gb, wb = _b(gb, g), _b(wb, w)
    gm = gamma(ds_dgrad_depth(g.shape[1]))
    with np.errstate(all='ignore'):
        ref = ds_dgrad_sum(g, w, hin, win)
        b = gm * ds_dgrad_sum(np.abs(g), np.abs(w), hin, win) + (
            ds_dgrad_sum(gb, np.abs(w) + wb, hin, win) + ds_dgrad_sum(np.abs(g), wb, hin, win)) * (1 + gm)
        if add is not None:
            add = f64(add)
            b = b + _b(addb, add)
            b = b + U * (np.abs(ref) + np.abs(add) + b)
            ref = ref + add
        return act_grad_ref(ref, b, a, act)


def channel_sum_ref(g, gb=0.0, prev=None):
    g = f64(g)
    gb = _b(gb, g)
    m, c, h, w = g.shape
    gm = gamma(cs_depth(m * h * w, c, prev is not None))
    ref, sh = g.sum((0, 2, 3)), np.abs(g).sum((0, 2, 3))
    if prev is not None:
        ref, sh = ref + f64(prev), sh + np.abs(f64(prev))
    return ref, gm * sh + gb.sum((0, 2, 3)) * (1 + gm)


def bn_scale(gam, var, eps=EPS):
    sd = np.sqrt(f64(var) + eps)
    return f64(gam) / sd, sd


def fold_ref(w, b, gam, beta, mean, var, eps=EPS):
    """-> (W', its bound, b', its bound)"""
    w, b, beta, mean = f64(w), f64(b), f64(beta), f64(mean)
    s, _ = bn_scale(gam, var, eps)
    sw = s.reshape(-1, *([1] * (w.ndim - 1)))
    wf, bf = sw * w, beta + s * (b - mean)
    return wf, gamma(WF_ROUNDINGS) * np.abs(wf), bf, gamma(BF_ROUNDINGS) * (np.abs(s * (b - mean)) + np.abs(beta))


UNFOLD_DEFECTS = ['no_bias_term', 's_twice']


def unfold_ref(w, b, gam, mean, var, dwf, dwfb, dbf, dbfb, eps=EPS, prev=None, defect=None):
    """-> dict of (value, bound) for dw, db, dgamma, dbeta; dwfb, dbfb: the bounds of dW', db'; prev: the four previous
    values under accumulate"""
    w, b, mean, dwf, dbf = f64(w), f64(b), f64(mean), f64(dwf), f64(dbf)
    dwfb, dbfb = _b(dwfb, dwf), _b(dbfb, dbf)
    s, sd = bn_scale(gam, var, eps)
    sw = s.reshape(-1, *([1] * (w.ndim - 1)))
    k = w[0].size
    ax = tuple(range(1, w.ndim))
    g5, gd = gamma(WF_ROUNDINGS + (prev is not None)), gamma(unfold_depth(k) + (prev is not None))
    d = b - mean
    with np.errstate(all='ignore'):
        dot, dsh = (w * dwf).sum(ax), (np.abs(w) * np.abs(dwf)).sum(ax)
        bias_term = 0.0 if defect == 'no_bias_term' else d * dbf
        out = dict(dw=(sw * dwf * (sw if defect == 's_twice' else 1.0), g5 * np.abs(sw * dwf) + np.abs(sw) * dwfb * (1 + g5)),
                   db=(s * dbf, g5 * np.abs(s * dbf) + np.abs(s) * dbfb * (1 + g5)),
                   dgamma=((dot + bias_term) / sd, (gd * (dsh + np.abs(d * dbf)) + ((np.abs(w) * dwfb).sum(ax) + np.abs(d) * dbfb) * (1 + gd)) / sd),
                   dbeta=(dbf + 0.0, dbfb + 0.0))
        if prev is not None:
            for key, pv in zip(('dw', 'db', 'dgamma', 'dbeta'), prev):
                v, bd = out[key]
                out[key] = (v + f64(pv), bd + (gd if key == 'dgamma' else g5 if key != 'dbeta' else U) * np.abs(f64(pv)) + (
                    U * np.abs(v) if key == 'dbeta' else 0.0))
    return out


# ============================================================================================== the encoder, restated
BLOCKS = [('res_layer1.0', 64, 64, 1), ('res_layer1.1', 64, 64, 1), ('res_layer2.0', 64, 96, 2), ('res_layer2.1', 96, 96, 1),
          ('res_layer3.0', 96, 128, 2), ('res_layer3.1', 128, 128, 1)]
OUT_CHANNELS, SPLIT = 256, 128


def param_shapes(cin=3):
    """the 62 parameters of the context encoder in named_parameters() order, then its 30 running statistics"""
    p, stats = {}, {}

    def conv(key, co, ci, k):
        p[f'{key}.weight'], p[f'{key}.bias'] = (co, ci, k, k), (co,)

    def bn(key, c):
        p[f'{key}.weight'], p[f'{key}.bias'] = (c,), (c,)
        stats[f'{key}.running_mean'], stats[f'{key}.running_var'] = (c,), (c,)

    conv('conv1', 64, cin, 7)
    bn('bn1', 64)
    for key, ci, co, stride in BLOCKS:
        conv(f'{key}.conv1', co, ci, 3)
        bn(f'{key}.bn1', co)
        conv(f'{key}.conv2', co, co, 3)
        bn(f'{key}.bn2', co)
        if stride != 1:
            conv(f'{key}.downsample.0', co, ci, 1)
            bn(f'{key}.downsample.1', co)
    conv('conv2', OUT_CHANNELS, 128, 1)
    return p, stats


PARAM_SHAPES, STAT_SHAPES = param_shapes()
PARAM_NAMES = list(PARAM_SHAPES)
LAYERS = [('conv1', 'conv1', 'bn1')] + [lay for key, _, _, stride in BLOCKS for lay in (
    [(f'{key}.conv1', f'{key}.conv1', f'{key}.bn1'), (f'{key}.conv2', f'{key}.conv2', f'{key}.bn2')] + (
        [(f'{key}.downsample', f'{key}.downsample.0', f'{key}.downsample.1')] if stride != 1 else []))]


def encoder_params(seed, prefix='context.'):
    """weights N(0, 0.05^2), biases N(0, 0.1^2), BatchNorm weights 1 + N(0, 0.1^2), running means N(0, 0.3^2) and running
    variances 0.5 + U-shaped |N(0, 1)|: statistics away from (0, 1); a pure function of the seed -> float32 state dict"""
    from test_fc_grad_host import golden_param
    sd = {}
    for name, shape in PARAM_SHAPES.items():
        v = golden_param('ctx.' + name, shape, seed)
        if re.search(r'(bn\d|downsample\.1)\.weight$', name):
            v = v + 1.0
        sd[prefix + name] = v
    for name, shape in STAT_SHAPES.items():
        v = golden_param('ctx.' + name, shape, seed, scale=1.0)
        sd[prefix + name] = (0.3 * v if name.endswith('mean') else 0.5 + v.abs()).float()
    return sd


def encoder_inputs(seed, n, h, w, tag=''):
    """-> (image (n, 3, h, w), cotangent (n, 256, h', w') at the head's post-activation output), float32"""
    from test_fc_grad_host import golden_param
    ho, wo = half(half(half(h))), half(half(half(w)))
    x = golden_param(f'ctx.image{tag}.{n}.{h}x{w}', (n, 3, h, w), seed, scale=1.0)
    g = golden_param(f'ctx.cot{tag}.{n}.{h}x{w}', (n, OUT_CHANNELS, ho, wo), seed, scale=1.0)
    return x, g


def head_act64(y):
    return torch.cat([torch.tanh(y[:, :SPLIT]), torch.relu(y[:, SPLIT:])], 1)


def oracle_grads(x, sd, g_out, prefix='context.'):
    """float64 autograd through oracle.raft_encoder and the split activation -> (out, dict of the 62 gradients)"""
    import sys
    sys.path.insert(0, ROOT)
    from oracle import scflow_oracle as oracle
    sd64 = {k: v.double().clone().requires_grad_(k[len(prefix):] in PARAM_SHAPES) for k, v in sd.items()}
    out = head_act64(oracle.raft_encoder(x.double(), sd64, prefix, 'BN'))
    (out * g_out.double()).sum().backward()
    return out.detach(), {k[len(prefix):]: v.grad for k, v in sd64.items() if v.grad is not None}


TIE_FACTOR = 64


def forward64(x, sd, prefix='context.', relu=None, ties=None):
    """the forward with every activation the backward reads, float64 torch (differentiable where ``sd`` requires grad)
    -> dict x, stem, t0 .. t5, y0 .. y5, out.

    ``relu``: {activation key: the decisions (bool) of an fp32 forward}.  A ReLU unit whose float64 pre-activation lies
    within the deviation an fp32 forward can have there has no derivative the inputs determine.  The deviation allowed:
    TIE_FACTOR (K + 8) U (|s| sum |w| |x| + |b'| + |identity|), K the terms of the unit's own sums, (K + 8) U for one
    evaluation of them with the folded BatchNorm, TIE_FACTOR = 64 for the deviation the up to 13 layers in front hand
    on and the transform-domain forward's constants.  There, and only there, the unit takes the given decision (as
    tests/test_chain_grad_host.py::chain_ref64 does); ``ties`` receives (key, units, worst |pre| / allowed)."""
    p = {k[len(prefix):]: v.double() for k, v in sd.items()}

    def layer(v, ckey, bkey, stride, pad):
        w, b = p[f'{ckey}.weight'], p[f'{ckey}.bias']
        y = F.batch_norm(F.conv2d(v, w, b, stride=stride, padding=pad), p[f'{bkey}.running_mean'], p[f'{bkey}.running_var'],
                         p[f'{bkey}.weight'], p[f'{bkey}.bias'], training=False, eps=EPS)
        with torch.no_grad():
            s = (p[f'{bkey}.weight'] / torch.sqrt(p[f'{bkey}.running_var'] + EPS)).abs().view(1, -1, 1, 1)
            mag = s * F.conv2d(v.abs(), w.abs(), (b - p[f'{bkey}.running_mean']).abs(), stride=stride, padding=pad)
            mag = (w[0].numel() + 8) * (mag + p[f'{bkey}.bias'].abs().view(1, -1, 1, 1))
        return y, mag

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
    v = acts['stem'] = gate('stem', *layer(acts['x'], 'conv1', 'bn1', 2, 3))
    for i, (key, _, _, stride) in enumerate(BLOCKS):
        t = acts[f't{i}'] = gate(f't{i}', *layer(v, f'{key}.conv1', f'{key}.bn1', stride, 1))
        idt, imag = layer(v, f'{key}.downsample.0', f'{key}.downsample.1', stride, 0) if stride != 1 else (v, v.detach().abs())
        pre, mag = layer(t, f'{key}.conv2', f'{key}.bn2', 1, 1)
        v = acts[f'y{i}'] = gate(f'y{i}', pre + idt, mag + imag)
    w, b = p['conv2.weight'], p['conv2.bias']
    y = F.conv2d(v, w, b)
    with torch.no_grad():
        mag = (w[0].numel() + 8) * F.conv2d(v.abs(), w.abs(), b.abs())
    acts['out'] = torch.cat([torch.tanh(y[:, :SPLIT]), gate('out', y[:, SPLIT:], mag[:, SPLIT:])], 1)
    return acts


def relu_decisions(kept):
    """the ReLU decisions of a forward from the activations it kept (RAFTEncoder.kept, or forward32's dict)"""
    d = {k: (v > 0).cpu() for k, v in kept.items() if k not in ('x', 'out')}
    d['out'] = (kept['out'][:, SPLIT:] > 0).cpu()
    return d


def truth64(x, sd, g_out, prefix='context.', relu=None, ties=None):
    """float64 autograd through forward64 -> (its activations, detached; dict of the 62 gradients): oracle_grads' graph
    (test_restated_walk_equals_float64_autograd holds the two against each other), with the ReLU decisions ``relu``"""
    sd64 = {k: v.detach().cpu().double().clone().requires_grad_(k[len(prefix):] in PARAM_SHAPES) for k, v in sd.items()}
    acts = forward64(x.detach().cpu(), sd64, prefix, relu, ties)
    (acts['out'] * g_out.detach().cpu().double()).sum().backward()
    return ({k: v.detach() for k, v in acts.items()},
            {k[len(prefix):]: v.grad for k, v in sd64.items() if k[len(prefix):] in PARAM_SHAPES})


def s1_dgrad(g, gb, w, wb, add=None, addb=0.0, a=None, act=NONE):
    """tests/test_head_grad_host.py's dgrad_ref with a bound on the weight: first order in wb, through the same index sum
    (the (1 + gamma(d)) (1 + U) on top of it is below 1.001 for every d of this file)"""
    ref, b = S1.dgrad_ref(g, gb, w, add, addb, a, act)
    extra = 1.001 * S1.dgrad_sum(np.abs(f64(g)) + _b(gb, f64(g)), _b(wb, f64(w)))
    return ref, b + (extra if act == NONE else extra * np.abs(act_factor(a, act)))


def cg_dgrad(g, gb, w, wb, hin, win):
    ref, b = CG.dgrad_ref(g, gb, w, hin, win)
    return ref, b + 1.001 * CG.dgrad_sum(np.abs(f64(g)) + _b(gb, f64(g)), _b(wb, f64(w)), hin, win)


def backward_ref64(acts, sd, g_out, xb=None, prefix='context.', launches=None):
    """RAFTEncoder.backward restated: the layer walk in float64 on the activations ``acts`` (taken as given up to the
    bounds ``xb``, a dict of the same keys; None: exact), every stage's bound carried into the next.
    -> dict name -> (gradient, bound) of the 62 parameters.  ``launches``: a dict that receives (value, bound) of the
    maps the walk passes on, keyed as RAFTEncoder.backward's ``intermediates``."""
    p = {k[len(prefix):]: f64(v) for k, v in sd.items()}
    a = {k: f64(v) for k, v in acts.items()}
    xb = {k: (0.0 if xb is None else f64(xb[k])) for k in a}
    rec = {} if launches is None else launches
    out = {}

    def folded(ckey, bkey):
        return fold_ref(p[f'{ckey}.weight'], p[f'{ckey}.bias'], p[f'{bkey}.weight'], p[f'{bkey}.bias'],
                        p[f'{bkey}.running_mean'], p[f'{bkey}.running_var'])[:2]

    def unfold(ckey, bkey, dwf, dwfb, dbf, dbfb):
        res = unfold_ref(p[f'{ckey}.weight'], p[f'{ckey}.bias'], p[f'{bkey}.weight'], p[f'{bkey}.running_mean'],
                         p[f'{bkey}.running_var'], dwf, dwfb, dbf, dbfb)
        out[f'{ckey}.weight'], out[f'{ckey}.bias'] = res['dw'], res['db']
        out[f'{bkey}.weight'], out[f'{bkey}.bias'] = res['dgamma'], res['dbeta']

    # head: the activation factors read `out` (bound xb['out']): tanh' = 1 - a^2 moves by at most (2 |a| + e) e
    g = f64(g_out)
    o, ob = a['out'], _b(xb['out'], a['out'])
    u, ub = np.empty_like(g), np.empty_like(g)
    u[:, :SPLIT], ub[:, :SPLIT] = act_grad_ref(g[:, :SPLIT], 0.0, o[:, :SPLIT], TANH)
    ub[:, :SPLIT] += np.abs(g[:, :SPLIT]) * (2 * np.abs(o[:, :SPLIT]) + ob[:, :SPLIT]) * ob[:, :SPLIT]
    u[:, SPLIT:], ub[:, SPLIT:] = act_grad_ref(g[:, SPLIT:], 0.0, o[:, SPLIT:], RELU)
    nb = len(BLOCKS)
    y = a[f'y{nb - 1}']
    dw, dwb, db, dbb = S1.wgrad_ref(u, ub, y, 1, 1, xb[f'y{nb - 1}'])
    out['conv2.weight'], out['conv2.bias'] = (dw, dwb), (db, dbb)
    G, Gb = S1.dgrad_ref(u, ub, p['conv2.weight'], a=y, act=RELU)
    rec['head'] = (G, Gb)
    for i in reversed(range(nb)):
        key, _, _, stride = BLOCKS[i]
        xk = f'y{i - 1}' if i else 'stem'
        x_in, t = a[xk], a[f't{i}']
        w2, w2b = folded(f'{key}.conv2', f'{key}.bn2')
        dwf, dwfb, dbf, dbfb = S1.wgrad_ref(G, Gb, t, 3, 3, xb[f't{i}'])
        g_t, g_tb = s1_dgrad(G, Gb, w2, w2b, a=t, act=RELU)
        unfold(f'{key}.conv2', f'{key}.bn2', dwf, dwfb, dbf, dbfb)
        rec[f'{key}.conv2'] = (g_t, g_tb)
        w1, w1b = folded(f'{key}.conv1', f'{key}.bn1')
        if stride == 1:
            dwf, dwfb, dbf, dbfb = S1.wgrad_ref(g_t, g_tb, x_in, 3, 3, xb[xk])
            g_prev, g_prevb = s1_dgrad(g_t, g_tb, w1, w1b, add=G, addb=Gb, a=x_in, act=RELU)
            unfold(f'{key}.conv1', f'{key}.bn1', dwf, dwfb, dbf, dbfb)
            rec[f'{key}.conv1'] = (g_prev, g_prevb)
        else:
            hin, win = x_in.shape[2:]
            dwf, dwfb = CG.wgrad_ref(g_t, g_tb, x_in, xb[xk])
            dbf, dbfb = channel_sum_ref(g_t, g_tb)
            gx1, gx1b = cg_dgrad(g_t, g_tb, w1, w1b, hin, win)
            unfold(f'{key}.conv1', f'{key}.bn1', dwf, dwfb, dbf, dbfb)
            rec[f'{key}.conv1'] = (gx1, gx1b)
            wd, wdb = folded(f'{key}.downsample.0', f'{key}.downsample.1')
            dwf, dwfb, dbf, dbfb = ds_wgrad_ref(G, Gb, x_in, xb[xk])
            g_prev, g_prevb = ds_dgrad_ref(G, Gb, wd, hin, win, wdb, add=gx1, addb=gx1b, a=x_in, act=RELU)
            unfold(f'{key}.downsample.0', f'{key}.downsample.1', dwf, dwfb, dbf, dbfb)
            rec[f'{key}.downsample'] = (g_prev, g_prevb)
        G, Gb = g_prev, g_prevb
    dwf, dwfb, dbf, dbfb = stem_wgrad_ref(G, Gb, a['x'], xb['x'])
    unfold('conv1', 'bn1', dwf, dwfb, dbf, dbfb)
    return out


# ===================================================================================================== the self-checks
def test_symbols_are_declared_exported_and_bound():
    from scflow_amd import _lib
    from scflow_amd.csrc import build
    assert 'encoder_grad.hip' in build.SOURCES
    for name in SYMBOLS:
        assert re.search(rf'\b{name}\(', HEADER), f'{name} is not declared in scflow_hip.h'
        assert re.search(rf'extern "C" \w+ {name}\(', SRC), f'{name} is not defined in encoder_grad.hip'
        assert name in _lib.SIGNATURES, f'{name} has no ctypes signature'
        proto = re.search(rf'^int(?:64_t)? {name}\(([^;]*)\);', HEADER, re.M).group(1)
        assert len(_lib.SIGNATURES[name][1]) == len(proto.split(',')), f'{name}: argument count'
    assert 'the presence of scf_conv_stem_wgrad marks' in re.sub(r'\s*\n \* ', ' ', HEADER)


def test_plans_are_the_counts_of_the_source():
    """the plans restated above against the library's own workspace queries (host code, no GPU)"""
    from scflow_amd import _lib
    lib = _lib.load()
    for m, cout, cin, ho, wo in [(1, 64, 3, 4, 5), (3, 64, 3, 9, 13), (2, 64, 4, 8, 12), (32, 64, 3, 128, 128), (5, 70, 1, 40, 33)]:
        _, s = stem_plan(m, ho, wo)
        assert lib.scf_conv_stem_wgrad_workspace(m, cout, cin, ho, wo) == s * (cout * cin * 49 + cout)
    for m, cout, cin, ho, wo in [(1, 96, 64, 5, 7), (3, 128, 96, 4, 6), (3, 72, 40, 5, 7), (32, 96, 64, 32, 32), (40, 300, 200, 16, 17)]:
        _, s = ds_plan(m, cout, cin, ho, wo)
        assert lib.scf_conv_ds_wgrad_workspace(m, cout, cin, ho, wo) == s * (cout * cin + cout)
    for m, c, n in [(1, 96, 35), (3, 128, 12), (32, 96, 1024), (7, 3000, 5000), (2, 1, 100000)]:
        _, s = cs_plan(m * n, c)
        assert lib.scf_channel_sum_workspace(m, c, n) == s * c
    assert stem_plan(3, 9, 13)[1] >= 2 and ds_plan(32, 96, 64, 32, 32)[1] >= 2 and cs_plan(32 * 1024, 96)[1] >= 2


def test_c_abi_rejects_bad_arguments_before_any_launch():
    """null pointers, non-positive sizes, maps that do not belong together, unknown activations, short strides and short
    workspaces: SCF_EINVAL; geometries that are not built: SCF_EUNSUPPORTED.  CPU pointers suffice: nothing is launched."""
    import ctypes as C
    from scflow_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 4096)()
    p = C.cast(buf, C.c_void_p)
    EINVAL, EUNSUP = -1, -2                     # scflow_hip.h: SCF_EINVAL, SCF_EUNSUPPORTED
    big = 1 << 40

    def stem(g=p, x=p, dw=p, ws=p, wsf=big, m=1, cout=64, cin=3, ho=4, wo=5, hin=7, win=9, k=7, stride=2, pad=3, gs=None, xs=None):
        return lib.scf_conv_stem_wgrad(g, cout * ho * wo if gs is None else gs, x, cin * hin * win if xs is None else xs, dw,
                                       p, 0, ws, wsf, m, cout, cin, ho, wo, hin, win, k, k, stride, pad, None)

    for kw in (dict(g=None), dict(x=None), dict(dw=None), dict(ws=None), dict(m=0), dict(cout=0), dict(cin=0), dict(ho=0),
               dict(ho=5), dict(wo=4), dict(wsf=10), dict(gs=3), dict(xs=3), dict(k=0), dict(stride=0), dict(pad=-1)):
        assert stem(**kw) == EINVAL, kw
    for kw in (dict(stride=1, ho=7, wo=9), dict(k=3), dict(pad=2), dict(cin=5), dict(k=5)):
        assert stem(**kw) == EUNSUP, kw

    def dsd(g=p, w=p, add=p, a=p, act=RELU, gx=p, m=1, cout=96, cin=64, ho=5, wo=7, hin=9, win=13, s=None):
        s = cin * hin * win if s is None else s
        return lib.scf_conv_ds_dgrad(g, cout * ho * wo, w, add, s, a, s, act, gx, s, m, cout, cin, ho, wo, hin, win, None)

    for kw in (dict(g=None), dict(w=None), dict(gx=None), dict(a=None), dict(act=7), dict(act=-1), dict(m=0), dict(cout=0),
               dict(cin=0), dict(ho=4), dict(wo=6), dict(hin=0), dict(s=5)):
        assert dsd(**kw) == EINVAL, kw

    def dsw(g=p, x=p, dw=p, ws=p, wsf=big, m=1, cout=96, cin=64, ho=5, wo=7, hin=9, win=13, gs=None):
        return lib.scf_conv_ds_wgrad(g, cout * ho * wo if gs is None else gs, x, cin * hin * win, dw, p, 0, ws, wsf, m, cout,
                                     cin, ho, wo, hin, win, None)

    for kw in (dict(g=None), dict(x=None), dict(dw=None), dict(ws=None), dict(wsf=100), dict(m=0), dict(cout=-1), dict(cin=0),
               dict(ho=6), dict(win=15), dict(gs=1)):
        assert dsw(**kw) == EINVAL, kw
    cs = lambda g=p, out=p, ws=p, wsf=big, m=2, c=5, n=12, gs=60: lib.scf_channel_sum(g, gs, out, 0, ws, wsf, m, c, n, None)  # noqa: E731
    for kw in (dict(g=None), dict(out=None), dict(ws=None), dict(wsf=4), dict(m=0), dict(c=0), dict(n=0), dict(gs=59)):
        assert cs(**kw) == EINVAL, kw
    assert cs(c=70000, gs=70000 * 12) == EUNSUP
    fold = lambda w=p, b=p, var=p, wf=p, eps=1e-5, c=4, k=9: lib.scf_bn_fold(w, b, p, p, p, var, eps, wf, p, c, k, None)  # noqa: E731
    for kw in (dict(w=None), dict(b=None), dict(var=None), dict(wf=None), dict(c=0), dict(k=0), dict(eps=-1.0), dict(eps=float('nan'))):
        assert fold(**kw) == EINVAL, kw
    unf = lambda w=p, dwf=p, dg=p, eps=1e-5, c=4, k=9: lib.scf_bn_unfold(w, p, p, p, p, eps, dwf, p, p, p, dg, p, 0, c, k, None)  # noqa: E731
    for kw in (dict(w=None), dict(dwf=None), dict(dg=None), dict(c=0), dict(k=-3), dict(eps=-1.0)):
        assert unf(**kw) == EINVAL, kw
    for name, args in (('scf_conv_stem_wgrad_workspace', (0, 64, 3, 4, 5)), ('scf_conv_stem_wgrad_workspace', (1, 64, 5, 4, 5)),
                       ('scf_conv_ds_wgrad_workspace', (1, 0, 3, 4, 5)), ('scf_channel_sum_workspace', (1, 2, 0))):
        assert getattr(lib, name)(*args) == -1, name
    assert not any(buf), 'a rejected call wrote'


def _rand(shape, seed, scale=1.0):
    return (np.random.RandomState(seed).standard_normal(shape) * scale).astype(np.float32)


STEM_CASES = [(1, 7, 9), (3, 18, 26), (2, 16, 24), (1, 1, 1), (2, 5, 40)]
DS_CASES = [(1, 64, 96, 9, 13), (3, 96, 128, 8, 12), (3, 40, 72, 9, 13), (1, 40, 72, 8, 12)]


def test_index_sums_equal_float64_autograd():
    """the index sums the bounds are built on are the gradients of the layers (float64 torch autograd)"""
    for m, h, w in STEM_CASES:
        x = torch.from_numpy(_rand((m, 3, h, w), 1)).double()
        wt = torch.from_numpy(_rand((8, 3, 7, 7), 2)).double().requires_grad_()
        b = torch.zeros(8, dtype=torch.float64, requires_grad=True)
        y = F.conv2d(x, wt, b, stride=2, padding=3)
        assert y.shape[2:] == (half(h), half(w))
        g = torch.from_numpy(_rand(tuple(y.shape), 3)).double()
        (y * g).sum().backward()
        ref = stem_wgrad_ref(g, 0.0, x)
        np.testing.assert_allclose(ref[0], wt.grad.numpy(), rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(ref[2], b.grad.numpy(), rtol=1e-12, atol=1e-12)
    for m, cin, cout, h, w in DS_CASES:
        x = torch.from_numpy(_rand((m, cin, h, w), 4)).double().requires_grad_()
        wt = torch.from_numpy(_rand((cout, cin, 1, 1), 5)).double().requires_grad_()
        b = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
        y = F.conv2d(x, wt, b, stride=2)
        g = torch.from_numpy(_rand(tuple(y.shape), 6)).double()
        (y * g).sum().backward()
        ref = ds_wgrad_ref(g, 0.0, x.detach())
        np.testing.assert_allclose(ref[0], wt.grad.numpy(), rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(ref[2], b.grad.numpy(), rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(ds_dgrad_ref(g, 0.0, wt.detach(), h, w)[0], x.grad.numpy(), rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(channel_sum_ref(g)[0], b.grad.numpy(), rtol=1e-12, atol=1e-12)


def _bn_case(c, k, seed):
    w, b = _rand((c, k), seed, 0.05), _rand((c,), seed + 1, 0.1)
    gam, beta = 1 + _rand((c,), seed + 2, 0.1), _rand((c,), seed + 3, 0.1)
    mean, var = _rand((c,), seed + 4, 0.3), 0.5 + np.abs(_rand((c,), seed + 5))
    return w, b, gam, beta, mean, var


def test_fold_and_unfold_equal_float64_autograd_and_fp32_torch_falls_inside():
    for c, k in ((5, 27), (64, 147), (96, 576)):
        w, b, gam, beta, mean, var = _bn_case(c, k, 10 + c)
        dwf, dbf = _rand((c, k), 20 + c), _rand((c,), 21 + c)
        t = [torch.from_numpy(v).double().requires_grad_() for v in (w, b, gam, beta)]
        s = t[2] / torch.sqrt(torch.from_numpy(var).double() + EPS)
        wf, bf = s[:, None] * t[0], t[3] + s * (t[1] - torch.from_numpy(mean).double())
        ref = fold_ref(w, b, gam, beta, mean, var)
        np.testing.assert_allclose(ref[0], wf.detach().numpy(), rtol=1e-13)
        np.testing.assert_allclose(ref[2], bf.detach().numpy(), rtol=1e-13)
        ((wf * torch.from_numpy(dwf).double()).sum() + (bf * torch.from_numpy(dbf).double()).sum()).backward()
        un = unfold_ref(w, b, gam, mean, var, dwf, 0.0, dbf, 0.0)
        for key, tt in zip(('dw', 'db', 'dgamma', 'dbeta'), t):
            np.testing.assert_allclose(un[key][0], tt.grad.numpy(), rtol=1e-11, atol=1e-13)
        # fp32 torch, an order of its own
        s32 = torch.from_numpy(gam) / torch.sqrt(torch.from_numpy(var) + np.float32(EPS))
        assert worst_ratio(s32[:, None] * torch.from_numpy(w), ref[0], ref[1]) <= 1
        assert worst_ratio(torch.from_numpy(beta) + s32 * torch.from_numpy(b - mean), ref[2], ref[3]) <= 1
        dg32 = ((torch.from_numpy(w) * torch.from_numpy(dwf)).sum(1) + torch.from_numpy(b - mean) * torch.from_numpy(dbf)) / torch.sqrt(
            torch.from_numpy(var) + np.float32(EPS))
        r = max(worst_ratio(dg32, *un['dgamma']), worst_ratio(s32[:, None] * torch.from_numpy(dwf), *un['dw']),
                worst_ratio(s32 * torch.from_numpy(dbf), *un['db']))
        measured(f'fp32 torch unfold {c}x{k}, error / bound', r)
        assert r <= 1


def test_fp32_torch_falls_inside_the_launch_bounds():
    """torch's own fp32 gradients of the layers (an order of its own, so the depths are raised by its longest chain) against
    the float64 sums"""
    global EXTRA
    worst = 0.0
    for m, h, w in STEM_CASES:
        x, g = _rand((m, 3, h, w), 31), _rand((m, 64, half(h), half(w)), 32)
        EXTRA = m * half(h) * half(w)
        try:
            ref = stem_wgrad_ref(g, 0.0, x)
        finally:
            EXTRA = 0
        dw = torch.nn.grad.conv2d_weight(torch.from_numpy(x), (64, 3, 7, 7), torch.from_numpy(g), stride=2, padding=3)
        worst = max(worst, worst_ratio(dw, ref[0], ref[1]), worst_ratio(torch.from_numpy(g).sum((0, 2, 3)), ref[2], ref[3]))
    for m, cin, cout, h, w in DS_CASES:
        x, g, wt = _rand((m, cin, h, w), 33), _rand((m, cout, half(h), half(w)), 34), _rand((cout, cin, 1, 1), 35, 0.05)
        add, a = _rand((m, cin, h, w), 36), _rand((m, cin, h, w), 37)
        EXTRA = max(m * half(h) * half(w), cout)
        try:
            ref = ds_wgrad_ref(g, 0.0, x)
            dref = ds_dgrad_ref(g, 0.0, wt, h, w, add=add, a=a, act=RELU)
        finally:
            EXTRA = 0
        dw = torch.nn.grad.conv2d_weight(torch.from_numpy(x), (cout, cin, 1, 1), torch.from_numpy(g), stride=2)
        gx = torch.nn.grad.conv2d_input((m, cin, h, w), torch.from_numpy(wt), torch.from_numpy(g), stride=2)
        gx = (gx + torch.from_numpy(add)) * (torch.from_numpy(a) > 0)
        worst = max(worst, worst_ratio(dw, ref[0], ref[1]), worst_ratio(gx, *dref))
    measured('fp32 torch layer gradients, error / bound', worst)
    assert worst <= 1


CASE_SEED = 20254


def small_case(n=2, h=18, w=26, seed=CASE_SEED):
    sd = encoder_params(seed)
    x, g = encoder_inputs(seed, n, h, w)
    return sd, x, g


@pytest.mark.parametrize('hw', [(18, 26), (16, 24)], ids=lambda v: f'{v[0]}x{v[1]}')
def test_restated_walk_equals_float64_autograd(hw):
    sd, x, g = small_case(2, *hw)
    out, truth = oracle_grads(x, sd, g)
    acts = forward64(x, sd)
    assert torch.equal(acts['out'], out)
    acts2, own = truth64(x, sd, g, relu=relu_decisions(acts))
    assert all(torch.equal(acts2[k], acts[k]) for k in acts)
    for name in PARAM_NAMES:
        assert (own[name] - truth[name]).abs().max() <= 1e-12 * truth[name].abs().max(), name
    got = backward_ref64(acts, sd, g)
    assert sorted(got) == sorted(PARAM_NAMES) and len(got) == 62
    for name in PARAM_NAMES:
        want = truth[name].numpy()
        scale = np.abs(want).max()
        assert scale > 0, name
        assert np.abs(got[name][0] - want).max() <= 1e-11 * scale, name
        assert (got[name][1] >= 0).all() and np.isfinite(got[name][1]).all(), name


def fp32_walk(sd, x, g):
    """the whole backward in fp32 by torch autograd (CPU) -> dict of the 62 gradients"""
    import sys
    sys.path.insert(0, ROOT)
    from oracle import scflow_oracle as oracle
    prefix = 'context.'
    sd32 = {k: v.clone().requires_grad_(k[len(prefix):] in PARAM_SHAPES) for k, v in sd.items()}
    out = head_act64(oracle.raft_encoder(x, sd32, prefix, 'BN'))
    (out * g).sum().backward()
    return {k[len(prefix):]: v.grad for k, v in sd32.items() if v.grad is not None}


TORCH_LONGEST = 9 * 128 + 2 * 9 * 13            # torch's fp32 chains: a 3x3 layer's 1152 products, a weight gradient's pixels


def composed_room(sd, x, g):
    """(float64 walk with its bounds at torch's depths, the forward's activations) for an fp32 evaluation of the whole
    encoder: the activations of an fp32 forward differ from float64 ones, which enters as xb"""
    global EXTRA
    acts = forward64(x, sd)
    f32 = forward32(x, sd)                    # the deviation of an fp32 forward, measured on torch's own (not under test)
    xb = {k: (acts[k] - f32[k].double()).abs().numpy() for k in acts}
    old = (S1.EXTRA, CG.EXTRA)
    S1.EXTRA = CG.EXTRA = EXTRA = TORCH_LONGEST
    try:
        return backward_ref64(acts, sd, g, xb=xb), acts, f32
    finally:
        S1.EXTRA, CG.EXTRA = old
        EXTRA = 0


def forward32(x, sd, prefix='context.'):
    """forward64's activations from an fp32 torch forward"""
    p = {k[len(prefix):]: v.float() for k, v in sd.items()}

    def layer(v, ckey, bkey, stride, pad):
        v = F.conv2d(v, p[f'{ckey}.weight'], p[f'{ckey}.bias'], stride=stride, padding=pad)
        return F.batch_norm(v, p[f'{bkey}.running_mean'], p[f'{bkey}.running_var'], p[f'{bkey}.weight'], p[f'{bkey}.bias'],
                            training=False, eps=EPS)

    acts = dict(x=x.float())
    v = acts['stem'] = torch.relu(layer(acts['x'], 'conv1', 'bn1', 2, 3))
    for i, (key, _, _, stride) in enumerate(BLOCKS):
        t = acts[f't{i}'] = torch.relu(layer(v, f'{key}.conv1', f'{key}.bn1', stride, 1))
        idt = layer(v, f'{key}.downsample.0', f'{key}.downsample.1', stride, 0) if stride != 1 else v
        v = acts[f'y{i}'] = torch.relu(layer(t, f'{key}.conv2', f'{key}.bn2', 1, 1) + idt)
    acts['out'] = head_act64(F.conv2d(v, p['conv2.weight'], p['conv2.bias']))
    return acts


def masks_agree(acts, other):
    """no ReLU of the walk decides differently in the two forwards (the bounds take the masks as given)"""
    return all(bool(((acts[k] > 0) == (other[k] > 0)).all()) for k in acts if k not in ('x', 'out')) and bool(
        ((acts['out'][:, SPLIT:] > 0) == (other['out'][:, SPLIT:] > 0)).all())


def test_fp32_walk_inside_the_composed_bounds():
    sd, x, g = small_case(2, 18, 26)
    ref, acts, f32 = composed_room(sd, x, g)
    assert masks_agree(acts, f32), 'a ReLU decides differently in fp32: choose another seed'
    got = fp32_walk(sd, x, g)
    worst = max(worst_ratio(got[name], *ref[name]) for name in PARAM_NAMES)
    measured('fp32 torch autograd of the whole encoder, error / composed bound', worst)
    assert worst <= 1


# Planted defects, each at the launch it belongs to and against that launch's own bound (operands as given): through the
# whole walk the worst-case bounds grow by a layer's sum |w| per layer while the signal grows by its norm, so only the
# launch's bound is sharp enough to tell.  The margins are the measured worst |defective - float64| / bound, rounded down.
# (measured: 1.01e5, inf -- a masked element has bound 0 --, 5.22e4, 1.98e6, 1.51e11, 1.4e5)
DEFECT_MARGINS = {'shortcut_dropped': 1e5, 'mask_of_wrong_activation': 1e9, 'no_bias_term': 5e4, 's_twice': 1e6,
                  'shortcut_to_odd_pixels': 1e11, 'stem_pad_off_by_one': 1e5}


def planted(defect):
    """-> (the defective value, the float64 value, its bound) of the launch the defect sits in"""
    if defect in UNFOLD_DEFECTS:
        w, b, gam, _, mean, var = _bn_case(96, 576, 50)
        dwf, dbf = _rand((96, 576), 51), _rand((96,), 52)
        key = 'dgamma' if defect == 'no_bias_term' else 'dw'
        return (unfold_ref(w, b, gam, mean, var, dwf, 0.0, dbf, 0.0, defect=defect)[key][0],
                *unfold_ref(w, b, gam, mean, var, dwf, 0.0, dbf, 0.0)[key])
    if defect == 'stem_pad_off_by_one':
        x, g = _rand((3, 3, 18, 26), 53), _rand((3, 64, 9, 13), 54)
        ref = stem_wgrad_ref(g, 0.0, x)
        return stem_wgrad_ref(g, 0.0, x, pad=2)[0], ref[0], ref[1]
    m, cin, cout, h, w = 3, 64, 96, 9, 13
    g, wt = _rand((m, cout, half(h), half(w)), 55), _rand((cout, cin, 1, 1), 56, 0.05)
    add, a, other = _rand((m, cin, h, w), 57), _rand((m, cin, h, w), 58), _rand((m, cin, h, w), 59)
    ref = ds_dgrad_ref(g, 0.0, wt, h, w, add=add, a=a, act=RELU)
    ds = ds_dgrad_sum(f64(g), f64(wt), h, w, odd=defect == 'shortcut_to_odd_pixels')
    if defect == 'shortcut_dropped':
        ds = 0.0
    mask = act_factor(other if defect == 'mask_of_wrong_activation' else a, RELU)
    return (ds + f64(add)) * mask, ref[0], ref[1]


PLANTED_DEFECTS = ['shortcut_dropped', 'mask_of_wrong_activation', 'shortcut_to_odd_pixels', 'stem_pad_off_by_one'] + UNFOLD_DEFECTS


@pytest.mark.parametrize('defect', PLANTED_DEFECTS)
def test_planted_defects_outside(defect):
    bad, ref, bound = planted(defect)
    worst = worst_ratio(bad, ref, bound)
    measured(f'planted defect {defect}, error / bound', worst)
    assert worst >= DEFECT_MARGINS[defect] >= 10


# ======================================================================================================== the fixture
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'context_grads.npz')
GOLDEN_SIZES = [(18, 26), (16, 24)]
GOLDEN_N, GOLDEN_SEED = 2, 20255
GOLDEN_ROOM = 1e-4                    # see test_reference_autograd_agrees_with_float64


def golden_case(hw):
    """-> (tag, float32 state dict behind 'context.', image, cotangent at the post-activation output)"""
    sd = encoder_params(GOLDEN_SEED)
    x, g = encoder_inputs(GOLDEN_SEED, GOLDEN_N, *hw, tag='.golden')
    return f'{hw[0]}x{hw[1]}', sd, x, g


def golden_pick(key, v):
    """the part of a gradient the fixture stores: of a weight the first and the last output channel and every fourth input
    channel of those; vectors whole"""
    v = np.asarray(v)
    return v[[0, v.shape[0] - 1]][:, ::4] if v.ndim == 4 else v


@pytest.mark.parametrize('hw', GOLDEN_SIZES, ids=lambda v: f'{v[0]}x{v[1]}')
def test_reference_autograd_agrees_with_float64(hw):
    """The reference's own RAFTEncoder (cxt_encoder of configs/refine_models/scflow.py, .eval(), fp32 autograd on the CPU,
    loss <cotangent, tanh | relu of its output>) against float64 autograd of the oracle on the same seeds.  The room:
    |fixture - float64| <= GOLDEN_ROOM x the largest entry of that gradient.  An fp32 forward and backward through 14
    layers whose longest sums hold 1152 products (3x3, 128 channels) or N h w <= 234 pixels: first-order errors of about
    14 (layers, there and back) x sqrt(1152) U ~ 3e-5 of a gradient's scale when roundings add like a random walk, which
    the room tops by 3; the worst case gamma(1152) = 7e-5 per layer is not reached by random data.  What the fixture
    pins is that the reference module computes what the oracle computes: a wrong term moves a gradient by its own size."""
    z = np.load(GOLDEN)
    tag, sd, x, g = golden_case(hw)
    _, truth = oracle_grads(x, sd, g)
    worst = 0.0
    for name in PARAM_NAMES:
        want = golden_pick(name, truth[name].numpy())
        got = z[f'{tag}.{name}']
        assert got.shape == want.shape and got.dtype == np.float32, name
        worst = max(worst, float(np.abs(got - want).max() / np.abs(truth[name].numpy()).max()))
    measured(f'reference RAFTEncoder autograd {tag}, |fixture - float64| / largest entry', worst)
    assert worst <= GOLDEN_ROOM
    assert os.path.getsize(GOLDEN) < 200 * 1024
