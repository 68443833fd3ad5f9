"""GPU: BatchNorm on the statistics of the batch -- ops.batch_norm_train / batch_norm_train_grad against the float64
restatement and the derived bound of tests/test_bn_train_host.py on every route of batch_norm_train.hip;
RAFTEncoder.batch_stats() / bn_backward against float64 autograd of a plain-torch restatement written here;
SCFlowRefiner.batch_norm_training() and train_step_network on the shipped flags."""
import contextlib
import json
import os

import numpy as np
import pytest
import torch

import scflow_amd
from scflow_amd import modules, ops, optim
from scflow_amd._lib import ScflowHipError
from scflow_amd.modules import RAFTEncoder, _bn_step
from scflow_amd.ops import ACT_RELU
import test_bn_train_host as BH
import test_context_grad_host as CH
import test_feature_grad_host as FH
import test_loss_host as HL
from test_stream_ops_host import f64, measured, same_bits, worst_ratio

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 1234.5
F = torch.nn.functional
cpu = lambda t: t.detach().cpu()                                    # noqa: E731


def D(t):
    return None if t is None else (torch.from_numpy(t) if isinstance(t, np.ndarray) else t).to(DEV).contiguous()


class Guarded:
    """destinations inside larger buffers filled with GUARD, 1 KiB either side (16-byte alignment is kept)"""

    def __init__(self):
        self.bufs = []

    def __call__(self, shape):
        n = int(np.prod(shape))
        b = torch.full((n + 512,), GUARD, device=DEV)
        self.bufs.append((b, n))
        return b[256:256 + n].view(shape)

    def check(self):
        for b, n in self.bufs:
            assert bool((b[:256] == GUARD).all()) and bool((b[256 + n:] == GUARD).all()), 'a guard value was overwritten'


def run_forward(case, guard=None):
    """ops.batch_norm_train on a host case (the running statistics are copies) -> dict keyed as BH.bn_forward64"""
    n, c, h, w = case['u'].shape
    dev = {k: D(v) for k, v in case.items() if k != 'res_bn'}
    rm, rv = dev['running_mean'].clone(), dev['running_var'].clone()
    res_bn = None
    if 'res_bn' in case:
        res_bn = [D(v).clone() for v in case['res_bn']]
    ws = None
    if guard is not None:
        ws = guard((ops.batch_norm_train_workspace(n, c, h * w),))
    out = guard(case['u'].shape) if guard is not None else None
    res = ops.batch_norm_train(dev['u'], dev['gamma'], dev['beta'], rm, rv, BH.MOMENTUM, BH.EPS, res=dev.get('res'), relu=True,
                               res_bn=res_bn, out=out, workspace=ws)
    got = dict(y=res[0], saved=res[1], running_mean=rm, running_var=rv)
    if res_bn is not None:
        got.update(saved_r=res[2], running_mean_r=res_bn[2], running_var_r=res_bn[3])
    return got


def run_grad(case, fwd, guard=None, out=None, accumulate=False):
    """ops.batch_norm_train_grad on the kernel's own forward ``fwd`` (its y and saved) -> dict keyed as BH.bn_grad64"""
    n, c, h, w = case['u'].shape
    form = 'tail_ds' if 'res_bn' in case else ('tail' if 'res' in case else 'mid')
    names = dict(mid=['du'], tail=['gp', 'du'], tail_ds=['du', 'dr'])[form] + ['dgamma', 'dbeta'] + (
        ['dgamma_r', 'dbeta_r'] if form == 'tail_ds' else [])
    ws = None
    if guard is not None:
        out = [guard(case['u'].shape if k in ('du', 'gp', 'dr') else (c,)) for k in names]
        ws = guard((ops.batch_norm_train_workspace(n, c, h * w),))
    kw = {}
    if form != 'mid':
        kw['y'] = fwd['y']
    if form == 'tail_ds':
        kw.update(r=D(case['res']), saved_r=fwd['saved_r'], gamma_r=D(case['res_bn'][0]))
    res = ops.batch_norm_train_grad(D(case['g']), D(case['u']), fwd['saved'], D(case['gamma']), out=out, accumulate=accumulate,
                                    workspace=ws, **kw)
    return dict(zip(names, res))


def kernel_case(form, shape, regime):
    """the host case with ``y`` and the mid form's mask taken from the kernel's own forward, as the encoder has them"""
    case = BH.bn_case(form, shape, regime=regime)
    fwd = run_forward(case)
    case['y'] = cpu(fwd['y'])
    if form == 'mid':
        g = BH._rand(shape, 99)
        case['g'] = torch.where(case['y'] > 0, g, torch.zeros(()))
    return case


def check_case(case, tag, aligned=True):
    n, _, h, w = case['u'].shape
    depths = BH.bn_depths(n, h * w, aligned)
    guard = Guarded()
    fwd = run_forward(case, guard)
    got = run_grad(case, fwd, guard)
    guard.check()
    fref = BH.bn_forward_ref(**BH.forward_args(case), relu=True, depths=depths)
    gref = BH.bn_grad_ref(**BH.grad_args(case), depths=depths)
    assert sorted(fwd) == sorted(fref) and sorted(got) == sorted(gref)
    worst = {}
    for have, ref in ((fwd, fref), (got, gref)):
        for k in ref:
            worst[k] = worst_ratio(cpu(have[k]), *ref[k])
    for k, v in worst.items():
        measured(f'batch_norm_train {tag}, {k}: error / bound', v)
    return fwd, got, worst


# ============================================================================================================ kernels
@pytest.mark.parametrize('case', BH.ALL_CASES, ids=BH.case_id)
def test_forms_against_float64(case):
    form, shape, regime = case
    c = kernel_case(form, shape, regime)
    fwd, got, worst = check_case(c, BH.case_id(case))
    assert max(worst.values()) <= 1.0, worst
    assert all(bool(torch.isfinite(v).all()) for v in list(fwd.values()) + list(got.values()))
    if 'gp' in got:                                                 # the residual's cotangent: g where y > 0, +0 elsewhere
        assert same_bits(got['gp'], torch.where(fwd['y'] > 0, D(c['g']), torch.zeros((), device=DEV)))
    if regime == 'constant':                                        # variance 0: rstd = 1 / sqrt(eps)
        want = 1.0 / np.sqrt(np.float32(BH.EPS))
        assert float((fwd['saved'][1] - float(want)).abs().max()) <= 16 * BH.U * float(want)
    if regime == 'channel_masked':
        assert not bool(fwd['y'][:, 0].any())
        if form != 'mid':                                           # nothing comes back through an all-masked channel
            assert not bool(got['du'][:, 0].any()) and float(got['dbeta'][0]) == 0 and float(got['dgamma'][0]) == 0
    if regime == 'gamma_zero':
        assert not bool(got['du'].any())
    # two more runs: the same bits
    for _ in range(2):
        f2 = run_forward(c)
        g2 = run_grad(c, f2)
        assert all(same_bits(f2[k], fwd[k]) for k in fwd) and all(same_bits(g2[k], got[k]) for k in got), 'two runs differ'
    # accumulate=True adds the parameter gradients to what the destinations hold, and leaves the maps as they are
    vec = [k for k in got if k.startswith(('dgamma', 'dbeta'))]
    base = {k: D(BH._rand(tuple(got[k].shape), 5 + i)) for i, k in enumerate(vec)}
    into = [None if k not in base else base[k].clone() for k in got]
    acc = run_grad(c, fwd, out=into, accumulate=True)
    assert all(same_bits(acc[k], got[k] + base[k]) for k in vec) and all(same_bits(acc[k], got[k]) for k in got if k not in vec)


def unaligned_case(form, shape):
    """a plane size that would take the vector route, every map 4 bytes off a 16-byte boundary -> worst error / bound"""
    assert ops.batch_norm_train_route(shape[0], shape[1], shape[2] * shape[3], True)['vec']
    assert not ops.batch_norm_train_route(shape[0], shape[1], shape[2] * shape[3], False)['vec']
    case = kernel_case(form, shape, 'nominal')
    off = lambda v: torch.empty((v.numel() + 1,), device=DEV)[1:].view(v.shape).copy_(v)      # noqa: E731
    u, g = off(case['u']), off(case['g'])
    assert u.data_ptr() % 16 == 4
    res = None if 'res' not in case else off(case['res'])
    rm, rv = D(case['running_mean']).clone(), D(case['running_var']).clone()
    res_bn = None if 'res_bn' not in case else [D(v).clone() for v in case['res_bn']]
    out = ops.batch_norm_train(u, D(case['gamma']), D(case['beta']), rm, rv, BH.MOMENTUM, BH.EPS, res=res, relu=True,
                               res_bn=res_bn)
    depths = BH.bn_depths(shape[0], shape[2] * shape[3], aligned=False)
    fref = BH.bn_forward_ref(**BH.forward_args(case), relu=True, depths=depths)
    worst = max(worst_ratio(cpu(out[0]), *fref['y']), worst_ratio(cpu(rv), *fref['running_var']))
    kw = {} if form == 'mid' else dict(y=off(cpu(out[0])))
    if form == 'tail_ds':
        kw.update(r=res, saved_r=out[2], gamma_r=res_bn[0])
    got = ops.batch_norm_train_grad(g if form != 'mid' else off(torch.where(cpu(out[0]) > 0, case['g'], torch.zeros(()))), u,
                                    out[1], D(case['gamma']), **kw)
    case = dict(case, y=cpu(out[0]), g=case['g'] if form != 'mid' else torch.where(cpu(out[0]) > 0, case['g'], torch.zeros(())))
    gref = BH.bn_grad_ref(**BH.grad_args(case), depths=depths)
    names = dict(mid=['du'], tail=['gp', 'du'], tail_ds=['du', 'dr'])[form] + ['dgamma', 'dbeta']
    worst = max([worst] + [worst_ratio(cpu(v), *gref[k]) for k, v in zip(names, got)])
    measured(f'batch_norm_train {form} {shape[2]}x{shape[3]} unaligned: worst error / bound', worst)
    return worst


@pytest.mark.parametrize('form', BH.FORMS)
def test_unaligned_pointers_take_the_scalar_route(form):
    assert unaligned_case(form, (2, 3, 8, 12)) <= 1.0


@pytest.mark.parametrize('form', BH.FORMS)
@pytest.mark.parametrize('shape', BH.UNALIGNED_SHAPES[1:], ids=lambda s: 'x'.join(map(str, s)))
def test_unaligned_pointers_at_two_apply_blocks_and_two_chunks(shape, form):
    """HW 4100: two scalar apply blocks, the second of 4 elements; HW 16388: the looped statistics kernel over two chunks,
    the second of 4 elements"""
    assert unaligned_case(form, shape) <= 1.0


def test_running_statistics_after_two_forwards_match_torch():
    """nn.BatchNorm2d in train() mode, float64 on the CPU, two batches: each kernel step inside its bound from the state
    before it, the end state next to torch's own fp32 module, num_batches_tracked == 2"""
    shape = (3, 5, 6, 10)
    bn = torch.nn.BatchNorm2d(5).to(DEV)
    t32, t64 = torch.nn.BatchNorm2d(5), torch.nn.BatchNorm2d(5).double()
    start = BH.bn_case('mid', shape, seed=7)
    for m in (bn, t32, t64):
        with torch.no_grad():
            m.weight.copy_(start['gamma']), m.bias.copy_(start['beta'])
            m.running_mean.copy_(start['running_mean']), m.running_var.copy_(start['running_var'])
        m.train()
    total = 0.0
    for step in range(2):
        u = BH.bn_case('mid', shape, seed=8 + step)['u']
        before = dict(start, u=u, running_mean=cpu(bn.running_mean).clone(), running_var=cpu(bn.running_var).clone())
        ref = BH.bn_forward_ref(**BH.forward_args(before), relu=True)
        y, _ = _bn_step(bn, D(u), relu=True)
        t32(u), t64(u.double())
        for k, have in (('running_mean', bn.running_mean), ('running_var', bn.running_var), ('y', y)):
            assert worst_ratio(cpu(have), *ref[k]) <= 1.0, (step, k)
        total = 0.9 * total + float(max(ref['running_mean'][1].max(), ref['running_var'][1].max()))
    assert int(bn.num_batches_tracked) == int(t32.num_batches_tracked) == 2
    for k in ('running_mean', 'running_var'):
        # both are fp32 evaluations of the float64 module's state: torch's own distance from it, plus this chain's bound
        room = float((getattr(t32, k).double() - getattr(t64, k)).abs().max()) + 2 * total
        assert float((cpu(getattr(bn, k)).double() - getattr(t64, k)).abs().max()) <= room, k


def test_ops_refusals():
    g = D(BH._rand((2, 2, 4, 4), 1))
    v, s = D(torch.ones(2)), D(torch.zeros(2, 2))
    with pytest.raises(NotImplementedError, match='momentum=None'):
        ops.batch_norm_train(g, v, v, None, None, momentum=None)
    with pytest.raises(ScflowHipError, match='no batch statistics'):
        ops.batch_norm_train(g[:1, :, :1, :1].contiguous(), v, v, None, None)
    with pytest.raises(ScflowHipError, match='comes with res'):
        ops.batch_norm_train(g, v, v, None, None, res_bn=(v, v, None, None))
    with pytest.raises(ScflowHipError, match='come together'):
        ops.batch_norm_train(g, v, v, v.clone(), None)
    with pytest.raises(ScflowHipError, match='must not alias'):
        ops.batch_norm_train(g, v, v, None, None, out=g)
    with pytest.raises(ScflowHipError, match='must be'):
        ops.batch_norm_train(g, v[:1].contiguous(), v, None, None)
    with pytest.raises(ScflowHipError, match='comes with y'):
        ops.batch_norm_train_grad(g, g, s, v, r=g, saved_r=s, gamma_r=v)
    with pytest.raises(ScflowHipError, match='come together'):
        ops.batch_norm_train_grad(g, g, s, v, y=g, r=g)
    with pytest.raises(ScflowHipError, match='destinations'):
        ops.batch_norm_train_grad(g, g, s, v, out=[None])
    with pytest.raises(ScflowHipError, match=r'\(2, 2\)'):
        ops.batch_norm_train_grad(g, g, s[:1].contiguous(), v)
    with pytest.raises(ScflowHipError, match='accumulate needs'):
        ops.batch_norm_train_grad(g, g, s, v, accumulate=True)
    with pytest.raises(ScflowHipError):
        ops.batch_norm_train(g.cpu(), v, v, None, None)
    y, saved = ops.batch_norm_train(g, v, v, None, None, relu=True)        # no running statistics: none are kept
    assert tuple(saved.shape) == (2, 2) and bool((y >= 0).all())


# ============================================================================================================ the encoder
ENC_N, ENC_HW = 3, (16, 24)
BN_KEYS = [b for _, _, b in CH.LAYERS]
# the biases in front of a BatchNorm: gradient 0 in exact arithmetic
ZERO_BIASES = [f'{c}.bias' for _, c, _ in CH.LAYERS]
KEPT_KEYS = sorted(['x', 'stem', 'u_stem', 's_stem', 'out', 'r2', 'r4', 'sr2', 'sr4']
                   + [f'{k}{i}' for i in range(6) for k in ('t', 'y', 'u1_', 'u2_', 's1_', 's2_')])


def build_encoder(sd):
    enc = RAFTEncoder(3, CH.OUT_CHANNELS, norm_cfg=dict(type='BN')).to(DEV)
    enc.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=False)
    return enc


def encoder_case():
    sd = CH.encoder_params(FH.CASE_SEED, prefix='')
    x, g = CH.encoder_inputs(FH.CASE_SEED, ENC_N, *ENC_HW, tag='.bn_train')
    return sd, x, g


def train_forward64(x, sd, relu):
    """the encoder in train() mode as plain torch, float64, differentiable where ``sd`` requires grad -> (activations with
    the raw outputs' gradients retained, the 30 updated running statistics, the worst |pre-activation| at a ReLU unit the
    kernel's forward decided the other way).  ``relu``: the decisions of the kernel's forward, which this graph takes."""
    p = {k: v for k, v in sd.items()}
    stats, acts, tie = {}, dict(x=x.double()), [0.0]

    def layer(v, ckey, bkey, stride, pad, ukey):
        u = F.conv2d(v, p[f'{ckey}.weight'], p[f'{ckey}.bias'], stride=stride, padding=pad)
        u.retain_grad()
        acts[ukey] = u
        rm, rv = p[f'{bkey}.running_mean'].detach().clone(), p[f'{bkey}.running_var'].detach().clone()
        out = F.batch_norm(u, rm, rv, p[f'{bkey}.weight'], p[f'{bkey}.bias'], True, 0.1, BH.EPS)
        stats[f'{bkey}.running_mean'], stats[f'{bkey}.running_var'] = rm, rv
        return out

    def gate(key, pre):
        mask = relu[key].to(pre.device)
        with torch.no_grad():
            wrong = (pre > 0) != mask
            if bool(wrong.any()):
                tie[0] = max(tie[0], float(pre.abs()[wrong].max()))
        acts[key] = pre * mask.to(pre.dtype)
        return acts[key]

    v = gate('stem', layer(acts['x'], 'conv1', 'bn1', 2, 3, 'u_stem'))
    for i, (key, _, _, stride) in enumerate(CH.BLOCKS):
        t = gate(f't{i}', layer(v, f'{key}.conv1', f'{key}.bn1', stride, 1, f'u1_{i}'))
        idt = v if stride == 1 else layer(v, f'{key}.downsample.0', f'{key}.downsample.1', stride, 0, f'r{i}')
        v = gate(f'y{i}', layer(t, f'{key}.conv2', f'{key}.bn2', 1, 1, f'u2_{i}') + idt)
    acts['out'] = F.conv2d(v, p['conv2.weight'], p['conv2.bias'])
    return acts, stats, tie[0]


@pytest.fixture(scope='module')
def encoder_run():
    """one forward under batch_stats() + keeping() and its bn_backward, and float64 autograd of the restatement on the
    kernel's ReLU decisions: computed once, shared and left unchanged"""
    sd, x, g = encoder_case()
    enc = build_encoder(sd)
    eval_before = enc(D(x)).clone()
    with enc.batch_stats(), enc.keeping():
        y = enc(D(x))
        saved = dict(enc.kept)
    im = {}
    grads = enc.bn_backward(saved, D(g), intermediates=im)
    sd64 = {k: v.double().clone().requires_grad_(v.dtype.is_floating_point and 'running' not in k) for k, v in sd.items()}
    relu = {k: cpu(saved[k] > 0) for k in FH.MASK_KEYS}
    acts, stats, tie = train_forward64(x, sd64, relu)
    (acts['out'] * g.double()).sum().backward()
    return dict(sd=sd, x=x, g=g, enc=enc, y=y, saved=saved, grads=grads, im=im, acts=acts, stats=stats, tie=tie,
                truth={k: v.grad for k, v in sd64.items() if v.requires_grad}, eval_before=eval_before)


def test_encoder_forward_on_batch_statistics(encoder_run):
    r = encoder_run
    enc, acts = r['enc'], r['acts']
    assert sorted(r['saved']) == KEPT_KEYS
    # the ReLU decisions taken from the kernel differ from float64's own only at units within rounding of zero
    measured('RAFTEncoder.batch_stats: worst |pre-activation| at a ReLU unit decided otherwise by float64', r['tie'])
    assert r['tie'] <= FH.GOLDEN_ROOM * max(float(acts[k].detach().abs().max()) for k in FH.MASK_KEYS)
    # FH.GOLDEN_ROOM: the argument of tests/test_feature_grad_host.py for 14 convolution layers there and back, the norms'
    # share below the convolutions'; a BatchNorm's sums are longer (N h w >= 18 values) and no worse conditioned
    for k in ['out', 'stem', 'y2', 'y5', 'u2_3']:
        want = acts[k].detach()
        err = float((cpu(r['saved'][k] if k != 'out' else r['y']).double() - want).abs().max()) / float(want.abs().max())
        measured(f'RAFTEncoder.batch_stats {k}: max error / largest float64 entry', err)
        assert err <= FH.GOLDEN_ROOM, k
    # the 30 running statistics moved to torch's, and the 15 batch counts
    now = enc.state_dict()
    for k, want in r['stats'].items():
        assert not same_bits(now[k], D(r['sd'][k])), k
        scale = max(float(want.abs().max()), 1.0)
        assert float((cpu(now[k]).double() - want).abs().max()) <= FH.GOLDEN_ROOM * scale, k
    assert all(int(now[f'{b}.num_batches_tracked']) == 1 for b in BN_KEYS) and len(BN_KEYS) == 15
    # the kept statistics are the forward's: normalising the kept raw output again gives the kept activation's bits
    bn1 = enc.bn1
    again, s = ops.batch_norm_train(r['saved']['u_stem'], bn1.weight, bn1.bias, None, None, bn1.momentum, bn1.eps, relu=True)
    assert same_bits(again, r['saved']['stem']) and same_bits(s, r['saved']['s_stem'])


def test_bn_backward_against_float64_autograd(encoder_run):
    r = encoder_run
    enc, grads, truth = r['enc'], r['grads'], r['truth']
    names = [k for k, _ in enc.named_parameters()]
    assert sorted(grads) == sorted(names) == sorted(truth) and len(grads) == 62
    assert all(grads[k].shape == v.shape for k, v in enc.named_parameters())
    worst = worst0 = 0.0
    du_key = {'conv1.bias': 'u_stem'}
    for i, (key, _, _, stride) in enumerate(CH.BLOCKS):
        du_key.update({f'{key}.conv1.bias': f'u1_{i}', f'{key}.conv2.bias': f'u2_{i}'})
        if stride != 1:
            du_key[f'{key}.downsample.0.bias'] = f'r{i}'
    assert sorted(du_key) == sorted(ZERO_BIASES)
    for k in names:
        want, have = f64(truth[k]), f64(grads[k])
        if k in ZERO_BIASES:
            scale = f64(r['acts'][du_key[k]].grad.abs().sum((0, 2, 3)))
            assert np.abs(want).max() <= 1e-9 * scale.max(), k     # float64: zero up to its own rounding
            worst0 = max(worst0, float((np.abs(have) / scale).max()))
        else:
            assert np.abs(want).max() > 0, k
            worst = max(worst, float(np.abs(have - want).max() / np.abs(want).max()))
    measured('RAFTEncoder.bn_backward 16x24 N 3, composed: worst max error / largest float64 entry', worst)
    measured('RAFTEncoder.bn_backward 16x24 N 3, composed: worst |zero bias gradient| / sum |du|', worst0)
    assert worst <= FH.GOLDEN_ROOM and worst0 <= FH.ZERO_BIAS_ROOM
    assert any(bool(grads[k].any()) for k in ZERO_BIASES)          # computed, not hard-wired
    # every launch of the new kernel in the walk, given its own operands, against the derived bound
    launches = 0
    for key, rec in r['im'].items():
        if not key.endswith(('bn1', 'bn2')):
            continue
        launches += 1
        bn = enc.get_submodule(key)
        case = dict(g=cpu(rec['g']), u=cpu(rec['u']), gamma_=cpu(bn.weight))
        if 'y' in rec:
            case['y'] = cpu(rec['y'])
        if 'r' in rec:
            case.update(r=cpu(rec['r']), gamma_r=cpu(enc.get_submodule(key[:-3] + 'downsample.1').weight))
        ref = BH.bn_grad_ref(**case)
        for k in ('du', 'dr', 'gp'):
            if k in rec:
                assert worst_ratio(cpu(rec[k]), *ref[k]) <= 1.0, (key, k)
    assert launches == 13
    # a second run: the same bits; accumulation doubles them
    again = enc.bn_backward(r['saved'], D(r['g']))
    assert all(same_bits(again[k], grads[k]) for k in grads)
    into = {k: v.clone() for k, v in grads.items()}
    assert enc.bn_backward(r['saved'], D(r['g']), param_grads=into) is into
    assert all(same_bits(into[k], grads[k] + grads[k]) for k in grads)
    with pytest.raises(ScflowHipError, match=r'under batch_stats\(\)'):
        enc.bn_backward({k: v for k, v in r['saved'].items() if k != 's2_3'}, D(r['g']))


def folded_forward(enc, x):
    """the eval forward as the parent commit launches it: ops.conv2d on the folded packs, layer by layer"""
    y = ops.conv2d(enc.packed['stem'], x, act=ACT_RELU)
    for name in enc.res_layers:
        for blk in getattr(enc, name):
            p = blk.packed
            if 'ds' in p:
                t, idt = ops.conv2d_pair((p['c1'], y, dict(act=ACT_RELU)), (p['ds'], y))
            else:
                t, idt = ops.conv2d(p['c1'], y, act=ACT_RELU), y
            y = ops.conv2d(p['c2'], t, res=idt, act=ACT_RELU)
    return ops.conv2d(enc.packed['head'], y)


def raw_packs(enc):
    """every convolution of the encoder packed without the norm behind it, keyed by the nn.Conv2d"""
    convs = [enc.conv1, enc.conv2] + [m for name in enc.res_layers for blk in getattr(enc, name)
                                      for m in (blk.conv1, blk.conv2) + (() if blk.downsample is None else (blk.downsample[0],))]
    return {c: ops.PackedConv.from_weight(c.weight, c.bias, c.stride[0], c.padding) for c in convs}


def batch_stats_forward(enc, p, x):
    """the forward under batch_stats() and keeping() as the parent commit launches it: ops.conv2d / conv2d_pair on the raw
    packs ``p``, ops.batch_norm_train behind each, layer by layer -> (the head's output, what the forward keeps)"""
    def norm(bn, u, **form):
        res = ops.batch_norm_train(u, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.momentum, bn.eps, **form)
        bn.num_batches_tracked += 1
        return res

    kept = dict(x=x, u_stem=ops.conv2d(p[enc.conv1], x))
    kept['stem'], kept['s_stem'] = norm(enc.bn1, kept['u_stem'], relu=True)
    y = kept['stem']
    for i, blk in enumerate(blk for name in enc.res_layers for blk in getattr(enc, name)):
        if blk.downsample is not None:
            u1, r = ops.conv2d_pair((p[blk.conv1], y), (p[blk.downsample[0]], y))
        else:
            u1, r = ops.conv2d(p[blk.conv1], y), None
        t, s1 = norm(blk.bn1, u1, relu=True)
        u2 = ops.conv2d(p[blk.conv2], t)
        if r is None:
            y, s2 = norm(blk.bn2, u2, res=y, relu=True)
        else:
            d = blk.downsample[1]
            y, s2, sr = norm(blk.bn2, u2, res=r, relu=True, res_bn=(d.weight, d.bias, d.running_mean, d.running_var))
            d.num_batches_tracked += 1
            kept[f'r{i}'], kept[f'sr{i}'] = r, sr
        kept.update({f't{i}': t, f'y{i}': y, f'u1_{i}': u1, f'u2_{i}': u2, f's1_{i}': s1, f's2_{i}': s2})
    kept['out'] = ops.conv2d(p[enc.conv2], y)
    return kept['out'], kept


def recorded(fn):
    """fn() -> (its result, (ran, paired, variants) of ops.record_conv_kernels around it)"""
    rec = ops.record_conv_kernels()
    with rec:
        res = fn()
    return res, (rec.ran, rec.paired, rec.variants)


def no_shared_storage(kept):
    ptrs = [v.data_ptr() for v in kept.values()]
    return len(set(ptrs)) == len(ptrs)


@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('hw', [(18, 26), (16, 24)], ids=lambda v: f'{v[0]}x{v[1]}')
def test_forward_modes_launch_what_the_lists_do(hw, n):
    """the BatchNorm encoder's four forward modes against the launch lists above: the bits of the output and of every kept
    tensor, the convolution routes, the moved statistics; 18 x 26 has 3 x 4 planes at the coarsest level (HW % 4 != 0)"""
    sd = CH.encoder_params(FH.CASE_SEED, prefix='')
    x = D(CH.encoder_inputs(FH.CASE_SEED, n, *hw, tag='.bn_train')[0])
    folded_keys = sorted(['x', 'stem', 'out'] + [f'{k}{i}' for i in range(6) for k in ('t', 'y')])

    def forward(enc, keep, batch):
        with (enc.batch_stats() if batch else contextlib.nullcontext()), (enc.keeping() if keep else contextlib.nullcontext()):
            return enc(x), dict(enc.kept)

    # folded on the running statistics, plain and keeping
    enc = build_encoder(sd)
    want, routes = recorded(lambda: folded_forward(enc, x))
    for keep in (False, True):
        (y, kept), ran = recorded(lambda: forward(enc, keep, False))
        assert same_bits(y, want) and ran == routes, keep
        assert sorted(kept) == (folded_keys if keep else [])
        assert not keep or sorted(kept) == sorted(modules._kept_keys(modules._FoldedBN, enc._blocks()))
        if keep:
            assert kept['x'] is x and kept['out'] is y and no_shared_storage(kept)
            assert same_bits(ops.conv2d(enc.packed['head'], kept['y5']), want)
    assert all(int(v) == 0 for k, v in enc.state_dict().items() if k.endswith('num_batches_tracked'))
    # on the statistics of the batch, plain and keeping: each against the list run on a second module of the same state
    for keep in (False, True):
        enc, ref = build_encoder(sd), build_encoder(sd)
        packs = raw_packs(ref)
        (want, want_kept), routes = recorded(lambda: batch_stats_forward(ref, packs, x))
        (y, kept), ran = recorded(lambda: forward(enc, keep, True))
        assert same_bits(y, want) and ran == routes, keep
        assert sorted(kept) == (KEPT_KEYS if keep else [])
        assert not keep or sorted(kept) == sorted(modules._kept_keys(modules._BatchBN, enc._blocks()))
        assert all(same_bits(kept[k], want_kept[k]) for k in kept)
        if keep:
            assert kept['x'] is x and kept['out'] is y and no_shared_storage(kept)
        now, ref_now = enc.state_dict(), ref.state_dict()
        stats = [k for k in now if 'running_' in k]
        counts = [k for k in now if k.endswith('num_batches_tracked')]
        assert len(stats) == 30 and len(counts) == 15 and len(now) == len(stats) + len(counts) + 62
        assert all(same_bits(now[k], ref_now[k]) and not same_bits(now[k], D(sd[k])) for k in stats)
        assert all(int(now[k]) == int(ref_now[k]) == 1 for k in counts)
        assert all(same_bits(now[k], D(sd[k])) for k in now if k not in stats and k not in counts)
    # a caller-owned destination: the kept output is a copy of it
    guard = Guarded()
    dest = guard(tuple(want.shape))
    with enc.batch_stats(), enc.keeping():
        y = enc(x, out=dest)
    guard.check()
    assert y.data_ptr() == dest.data_ptr() and enc.kept['out'].data_ptr() != y.data_ptr()
    assert same_bits(enc.kept['out'], y) and no_shared_storage(enc.kept)


def test_eval_forward_is_unchanged_and_follows_the_moved_statistics(encoder_run):
    r = encoder_run
    sd, x = r['sd'], D(r['x'])
    fresh = build_encoder(sd)
    assert fresh.batch is False
    assert same_bits(fresh(x), folded_forward(fresh, x)) and same_bits(fresh(x), r['eval_before'])
    assert fresh.kept == {} and all(int(v) == 0 for k, v in fresh.state_dict().items() if k.endswith('num_batches_tracked'))
    # after the forward on batch statistics the eval forward of the same module runs on the moved statistics: the bits of
    # a module built from its state dict, not the bits from before
    enc = r['enc']
    after = enc(x)
    moved = build_encoder({k: cpu(v) for k, v in enc.state_dict().items()})
    assert same_bits(after, moved(x)) and same_bits(after, folded_forward(enc, x))
    assert not same_bits(after, r['eval_before'])
    feat = RAFTEncoder(3, 256, norm_cfg=dict(type='IN')).to(DEV)
    with pytest.raises(NotImplementedError, match='InstanceNorm encoder has no batch statistics'):
        with feat.batch_stats():
            pass


# ====================================================================================================== the training step
# 256 x 256 is the one image size the network takes: the pose head's first fully connected layer has 2048 = 128 x 4 x 4
# inputs, which fixes the maps behind three stride-2 convolutions at 32 x 32 (a 64 x 64 crop gives 128 features and raises)
STEP_N, STEP_HW, STEP_ITERS = 2, 256, 2
HP = dict(type='AdamW', lr=4e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4)


def step_case(input_seed=7, case_seed=5):
    """HL.refiner_loss_case at N = 2"""
    from scflow_amd.synthetic import make_inputs
    n, f32 = STEP_N, np.float32
    inp = make_inputs(n, STEP_HW, STEP_HW, seed=input_seed)
    rng = np.random.RandomState(case_seed)
    gt_r = np.stack([HL.rand_rot(rng, 0.04) @ inp['ref_rotation'][i].numpy() for i in range(n)]).astype(f32)
    gt_t = (inp['ref_translation'].numpy() + rng.randn(n, 3) * [3, 3, 12]).astype(f32)
    gt_masks = (inp['depth'] > 0).clone()
    gt_masks[:, :100, :110] = False
    labels = [int(v) for v in inp['label']]
    return dict(inp=inp, gt_r=gt_r, gt_t=gt_t, gt_masks=gt_masks, labels=labels, symmetry_types={f'cls_{labels[0] + 1}': {}},
                diameter=[float(f32(90 + 7.7 * c)) for c in range(21)],
                init_add_error=torch.from_numpy(rng.uniform(5, 40, size=n).astype(f32)),
                scale=rng.uniform(0.8, 1.6, size=n).astype(f32))


@pytest.fixture(scope='module')
def step_start(golden_dir):
    shapes = json.load(open(os.path.join(golden_dir, 'state_dict_keys.json')))['shapes']
    return scflow_amd.fill_state_dict(shapes, seed=0), step_case()


def build(start, **over):
    sd, case = start
    cfg = scflow_amd.scflow_model_cfg(iters=STEP_ITERS)
    cfg.update(HL.refiner_loss_cfgs(case))
    cfg['pose_loss_cfg'] = dict(type='SequenceLoss', gamma=0.7, loss_func_cfg=dict(type='RAFTLoss', loss_weight=0.3, max_flow=400.))
    cfg.update(over)
    m = scflow_amd.build_refiner(cfg)
    m.load_state_dict(sd, strict=True)
    return m.to(DEV)


def optimizer(m):
    return optim.build_optimizer(m, HP, dict(grad_clip=dict(max_norm=10.)), network=True)


def same(a, b):
    return same_bits(a, b) if a.dtype == torch.float32 else torch.equal(a, b)


def snapshot(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def pose(m, data):
    return m.get_pose(data['rendered_images'], data['real_images'], data['ref_rotations'], data['ref_translations'],
                      data['rendered_depths'], data['internel_k'], data['labels'])


def test_train_step_network_on_the_shipped_flags(step_start):
    data = HL.refiner_data(step_start[1], DEV)
    m = build(step_start)
    assert m.freeze_encoder is False and m.freeze_bn is False
    before = snapshot(m)
    eval_before = pose(m, data)
    out = m.train_step_network(None, optimizer(m), data=data)
    assert sorted(out) == ['log_imgs', 'log_vars', 'loss', 'num_samples'] and out['num_samples'] == STEP_N
    assert list(out['log_vars'])[-2:] == ['grad_norm', 'lr'] and np.isfinite(list(out['log_vars'].values())).all()
    after = snapshot(m)
    names = [n for n, _ in m.named_parameters()]
    assert len(names) == 149 and all(not same_bits(before[n], after[n]) for n in names), 'every tensor moves'
    stats = [k for k in before if 'running_' in k]
    assert len(stats) == 30 and all(not same_bits(before[k], after[k]) for k in stats)
    assert all(int(after[k]) == 1 for k in before if k.endswith('num_batches_tracked'))
    assert m.context.batch is False and m.context.kept == {}
    # the same bits as the rung inside the switch followed by the optimizer's step
    ref = build(step_start)
    opt = optimizer(ref)
    with ref.batch_norm_training():
        want = ref.loss_and_network_grads(None, data=data)
    assert sorted(want[5]['params']) == sorted(names)
    opt.step(want[5]['params'])
    assert same_bits(out['loss'], want[0])
    state = snapshot(ref)
    assert all(same(after[k], state[k]) for k in after)
    # the next eval forward runs on the new weights and statistics: the bits of a model built from the state dict
    fresh = build((({k: v.cpu() for k, v in after.items()}), step_start[1]))
    a, b = pose(m, data), pose(fresh, data)
    assert all(same_bits(x, y) for sa, sb in zip(a, b) for x, y in zip(sa, sb))
    assert not all(same_bits(x, y) for sa, sb in zip(a, eval_before) for x, y in zip(sa, sb))
    # the loss rungs outside the switch are the parent's: eval statistics, nothing moves
    mid = snapshot(m)
    m.loss_and_context_grads(None, data=data)
    assert all(same(v, mid[k]) for k, v in m.state_dict().items())


@pytest.mark.parametrize('flag', ['freeze_bn', 'freeze_encoder'])
def test_train_step_network_leaves_what_is_frozen(step_start, flag):
    data = HL.refiner_data(step_start[1], DEV)
    m = build(step_start, **{flag: True})
    before = snapshot(m)
    m.train_step_network(None, optimizer(m), data=data)
    after = snapshot(m)
    if flag == 'freeze_bn':
        frozen = [k for k in before if 'running_' in k or k.endswith('num_batches_tracked')]
        assert len(frozen) == 45
    else:
        frozen = [k for k in before if k.startswith(('render_encoder.', 'real_encoder.'))]
        assert len(frozen) >= 32 and any('running_' in k and not same_bits(before[k], after[k]) for k in before)
    assert all(same(before[k], after[k]) for k in frozen)
    moved = [n for n, _ in m.network_parameters()]
    assert all(not same_bits(before[n], after[n]) for n in moved) and len(moved) == (149 if flag == 'freeze_bn' else 117)
    with pytest.raises(ValueError, match='network_parameters'):
        m.train_step_network(None, optim.build_optimizer(build(step_start), HP, network=True), data=data)


# ================================================================================================ the reference fixture
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'bn_train_grads.npz')


def test_network_grads_on_batch_statistics_against_the_reference_fixture(step_start):
    """``loss_and_network_grads()`` inside ``batch_norm_training()`` at the fixture's case (tests/golden/
    make_golden_bn_train.py: the reference's own ``.backward()`` in ``train()`` mode, fp32 on the CPU) -- the loss, the
    62 ``context.*`` and 32 ``render_encoder.*`` gradients and the 30 moved running statistics, each within 3 x the distance
    between the reference's fp32 and float64 evaluations of that graph, which the generator measured on the CPU and stored:
    loss 2.0e-7, context 1.11e-2, render_encoder 1.05e-2 of a tensor's largest entry, running statistics 9.8e-8."""
    import test_chain_grad_host as CG
    z = np.load(GOLDEN)
    assert {k: int(z[k]) for k in CG.FIXTURE_SEEDS} == CG.FIXTURE_SEEDS and int(z['iters']) == HL.REFINER_ITERS
    assert os.path.getsize(GOLDEN) < 256 * 1024
    case = HL.refiner_loss_case(CG.FIXTURE_SEEDS['input_seed'], CG.FIXTURE_SEEDS['case_seed'])
    sd, _ = step_start
    cfg = scflow_amd.scflow_model_cfg(iters=HL.REFINER_ITERS)
    cfg.update(HL.refiner_loss_cfgs(case))
    cfg['pose_loss_cfg'] = dict(CG.RAFT_POSE_LOSS)
    m = scflow_amd.build_refiner(cfg)
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV)
    with m.batch_norm_training():
        loss, _, _, _, _, grads = m.loss_and_network_grads(None, data=HL.refiner_data(case, DEV))
    dist = {g: float(z[f'distance.{g}']) for g in ('loss', 'context', 'render_encoder', 'running')}
    want = float(z['loss'].reshape(-1)[0])
    worst = dict(loss=abs(float(loss) - want) / abs(want) / dist['loss'])
    state = m.context.state_dict()
    for k in z.files:
        group, _, name = k.partition('.')
        if group not in ('context', 'render_encoder', 'running'):
            continue
        scale = float(z[f'scale.{k}'])
        top = max(float(z[f'scale.{q}']) for q in z.files if q.startswith(group + '.'))
        if scale <= 1e-6 * top:                                     # a bias in front of a norm: exact gradient 0, left out
            continue
        have = state[name] if group == 'running' else grads['params'][k]
        err = float(np.abs(CH.golden_pick(k, f64(have)) - f64(z[k])).max()) / scale
        worst[group] = max(worst.get(group, 0.0), err / dist[group])
    for g, v in worst.items():
        measured(f'batch-statistics network gradients against the reference fixture, {g}: distance / the fp32-float64 distance', v)
    assert max(worst.values()) <= 3.0, worst
