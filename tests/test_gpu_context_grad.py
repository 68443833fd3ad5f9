"""GPU: encoder_grad.hip (scf_conv_stem_wgrad, scf_conv_ds_dgrad, scf_conv_ds_wgrad, scf_channel_sum, scf_bn_fold,
scf_bn_unfold), RAFTEncoder.keeping / backward and SCFlowRefiner.loss_and_context_grads against the float64 restatements
and the derived bounds of tests/test_context_grad_host.py.  Every launch is compared as `error <= bound` over ALL elements
(ratio <= 1) given its own operands, or by bit equality.  The composed gradients are held to float64 autograd of the whole
encoder in the measure of tests/test_gpu_chain_grad.py, max |g - g64| / max |g64| per tensor, inside CH.GOLDEN_ROOM (the
room of an fp32 evaluation, derived at test_reference_autograd_agrees_with_float64), and to the reference module's fixture
inside twice that (two fp32 evaluations around one float64 value).  The measured ratios are recorded in DESIGN.md section
4.15."""
import numpy as np
import pytest
import torch

from scflow_amd import ops
from scflow_amd._lib import ScflowHipError
from scflow_amd.modules import RAFTEncoder
import test_context_grad_host as CH
import test_conv_grad_host as CG
import test_head_grad_host as S1
import test_loss_host as HL
from test_head_grad_host import NONE, RELU, TANH
from test_stream_ops_host import f64, measured, same_bits, worst_ratio  # noqa: E402
from test_gpu_gru_grad import scflow_model  # noqa: F401  (the small random-weight refiner, a module-scoped fixture)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
cpu = lambda t: t.detach().cpu()                                    # noqa: E731


def D(t):
    return None if t is None else (torch.from_numpy(t) if isinstance(t, np.ndarray) else t).to(DEV).contiguous()


def R(shape, seed, scale=1.0):
    return CH._rand(shape, seed, scale)


# ============================================================================================================ kernels
# (M, H, W): odd and even maps, a map smaller than the kernel, contractions that are no multiple of the 16-pixel chunk,
# 1 split (1, 7, 9), several splits of ST_MIN_CHUNKS chunks, and (16, 128, 130): 5120 chunks, 1024 splits of 5
STEM_SHAPES = [(1, 7, 9, 3), (3, 18, 26, 3), (2, 16, 24, 3), (2, 16, 24, 1), (2, 16, 24, 2), (2, 16, 24, 4), (1, 1, 1, 3),
               (16, 128, 130, 3)]


@pytest.mark.parametrize('shape', STEM_SHAPES, ids=lambda s: 'M{}-{}x{}-C{}'.format(*s))
def test_stem_wgrad_against_float64(shape):
    m, h, w, cin = shape
    ho, wo = CH.half(h), CH.half(w)
    x, g = R((m, cin, h, w), 1), R((m, 64, ho, wo), 2)
    if shape == STEM_SHAPES[1]:
        assert CH.stem_plan(m, ho, wo)[1] >= 2
    if shape == STEM_SHAPES[-1]:
        assert CH.stem_plan(m, ho, wo) == (5, 1024)
    dw, db = ops.conv_stem_wgrad(D(g), D(x))
    ref = CH.stem_wgrad_ref(g, 0.0, x)
    v = max(worst_ratio(cpu(dw), ref[0], ref[1]), worst_ratio(cpu(db), ref[2], ref[3]))
    measured(f'conv_stem_wgrad {shape}, worst error / bound', v)
    assert v <= 1.0 and bool(torch.isfinite(dw).all())
    dw2, db2 = ops.conv_stem_wgrad(D(g), D(x))
    assert same_bits(dw, dw2) and same_bits(db, db2), 'two runs differ'
    pw, pb = D(R((64, cin, 7, 7), 3)), D(R((64,), 4))
    aw, ab = ops.conv_stem_wgrad(D(g), D(x), dw=pw.clone(), db=pb.clone(), accumulate=True)
    assert same_bits(aw, dw + pw) and same_bits(ab, db + pb), 'accumulate adds the previous value last'
    assert ops.conv_stem_wgrad(D(g), D(x), bias=False)[1] is None
    # channel slices of wider tensors are operands
    wide_g, wide_x = D(R((m, 70, ho, wo), 5)), D(R((m, cin + 2, h, w), 6))
    wide_g[:, 3:67], wide_x[:, 1:1 + cin] = D(g), D(x)
    sw, sb = ops.conv_stem_wgrad(wide_g[:, 3:67], wide_x[:, 1:1 + cin])
    assert same_bits(sw, dw) and same_bits(sb, db)


DS_CHANNELS = [(64, 96), (96, 128), (40, 72)]
DS_MAPS = [(9, 13), (8, 12)]


@pytest.mark.parametrize('hw', DS_MAPS, ids=lambda v: f'{v[0]}x{v[1]}')
@pytest.mark.parametrize('ch', DS_CHANNELS, ids=lambda v: f'{v[0]}to{v[1]}')
def test_shortcut_dgrad_against_float64(ch, hw):
    cin, cout = ch
    h, w = hw
    ho, wo = CH.half(h), CH.half(w)
    worst = 0.0
    for m in (1, 3):
        g, wt = R((m, cout, ho, wo), 11), R((cout, cin, 1, 1), 12, 0.05)
        add, a = R((m, cin, h, w), 13), R((m, cin, h, w), 14)
        for with_add in (False, True):
            for act in (NONE, RELU):
                got = ops.conv_ds_dgrad(D(g), D(wt), (h, w), add=D(add) if with_add else None, a=D(a) if act else None, act=act)
                ref, bound = CH.ds_dgrad_ref(g, 0.0, wt, h, w, add=add if with_add else None, a=a if act else None, act=act)
                worst = max(worst, worst_ratio(cpu(got), ref, bound))
                if not with_add:                            # the odd pixels hold +0
                    assert not bool(got[:, :, 1::2].any()) and not bool(got[:, :, :, 1::2].any())
                assert same_bits(got, ops.conv_ds_dgrad(D(g), D(wt), (h, w), add=D(add) if with_add else None,
                                                        a=D(a) if act else None, act=act)), 'two runs differ'
    measured(f'conv_ds_dgrad {ch} {hw}, worst error / bound', worst)
    assert worst <= 1.0
    # a sample's input gradient depends on that sample alone: sample 1 of M = 3 alone gives the same bits
    g, wt, add, a = D(R((3, cout, ho, wo), 11)), D(R((cout, cin, 1, 1), 12, 0.05)), D(R((3, cin, h, w), 13)), D(R((3, cin, h, w), 14))
    all3 = ops.conv_ds_dgrad(g, wt, (h, w), add=add, a=a, act=RELU)
    one = ops.conv_ds_dgrad(g[1:2], wt, (h, w), add=add[1:2], a=a[1:2], act=RELU)
    assert same_bits(all3[1:2], one)
    # the other activation factors are scf_act_grad's
    for act in (S1.SIGMOID, TANH):
        got = ops.conv_ds_dgrad(g, wt, (h, w), add=add, a=a, act=act)
        assert same_bits(got, ops.act_grad(ops.conv_ds_dgrad(g, wt, (h, w), add=add), a, act))


@pytest.mark.parametrize('hw', DS_MAPS, ids=lambda v: f'{v[0]}x{v[1]}')
@pytest.mark.parametrize('ch', DS_CHANNELS, ids=lambda v: f'{v[0]}to{v[1]}')
def test_shortcut_wgrad_against_float64(ch, hw):
    cin, cout = ch
    h, w = hw
    ho, wo = CH.half(h), CH.half(w)
    worst = 0.0
    for m in (1, 3, 40):                        # 40: 200 chunks, more than one split
        g, x = R((m, cout, ho, wo), 21), R((m, cin, h, w), 22)
        dw, db = ops.conv_ds_wgrad(D(g), D(x))
        ref = CH.ds_wgrad_ref(g, 0.0, x)
        worst = max(worst, worst_ratio(cpu(dw), ref[0], ref[1]), worst_ratio(cpu(db), ref[2], ref[3]))
        dw2, db2 = ops.conv_ds_wgrad(D(g), D(x))
        assert same_bits(dw, dw2) and same_bits(db, db2), 'two runs differ'
        pw, pb = D(R((cout, cin, 1, 1), 23)), D(R((cout,), 24))
        aw, ab = ops.conv_ds_wgrad(D(g), D(x), dw=pw.clone(), db=pb.clone(), accumulate=True)
        assert same_bits(aw, dw + pw) and same_bits(ab, db + pb)
    assert CH.ds_plan(40, cout, cin, ho, wo)[1] >= 2
    measured(f'conv_ds_wgrad {ch} {hw}, worst error / bound', worst)
    assert worst <= 1.0


def test_channel_sum():
    worst = 0.0
    for m, c, h, w in [(1, 96, 5, 7), (3, 128, 4, 6), (2, 5, 1, 1), (32, 96, 32, 32)]:
        g = R((m, c, h, w), 31)
        got = ops.channel_sum(D(g))
        worst = max(worst, worst_ratio(cpu(got), *CH.channel_sum_ref(g)))
        assert same_bits(got, ops.channel_sum(D(g)))
        prev = D(R((c,), 32))
        assert same_bits(ops.channel_sum(D(g), out=prev.clone(), accumulate=True), got + prev)
        wide = D(R((m, c + 3, h, w), 33))
        wide[:, 2:2 + c] = D(g)
        assert same_bits(ops.channel_sum(wide[:, 2:2 + c]), got)
        # integer operands: every partial sum is exact, so any order gives these bits
        gi = torch.randint(-8, 9, (m, c, h, w), generator=torch.Generator().manual_seed(34)).float()
        assert same_bits(ops.channel_sum(D(gi)), D(gi.sum((0, 2, 3))))
    assert CH.cs_plan(32 * 1024, 96)[1] >= 2
    measured('channel_sum, worst error / bound', worst)
    assert worst <= 1.0


def _bn_operands(c, k, seed):
    return [D(v) for v in CH._bn_case(c, k, seed)]


def test_fold_and_unfold():
    worst = 0.0
    for c, k in [(5, 27), (64, 147), (96, 576), (128, 1152), (96, 64)]:
        w, b, gam, beta, mean, var = ops_in = _bn_operands(c, k, 40 + c)
        wf, bf = ops.bn_fold(w, b, gam, beta, mean, var, CH.EPS)
        ref = CH.fold_ref(*[cpu(t) for t in ops_in])
        worst = max(worst, worst_ratio(cpu(wf), ref[0], ref[1]), worst_ratio(cpu(bf), ref[2], ref[3]))
        dwf, dbf = D(R((c, k), 41)), D(R((c,), 42))
        got = ops.bn_unfold(w, b, gam, mean, var, CH.EPS, dwf, dbf)
        un = CH.unfold_ref(cpu(w), cpu(b), cpu(gam), cpu(mean), cpu(var), cpu(dwf), 0.0, cpu(dbf), 0.0)
        for key, t in zip(('dw', 'db', 'dgamma', 'dbeta'), got):
            worst = max(worst, worst_ratio(cpu(t), *un[key]))
        assert same_bits(got[3], dbf)
        again = ops.bn_unfold(w, b, gam, mean, var, CH.EPS, dwf, dbf)
        assert all(same_bits(a, b_) for a, b_ in zip(got, again)), 'two runs differ'
        prev = [D(R(tuple(t.shape), 43 + i)) for i, t in enumerate(got)]
        acc = ops.bn_unfold(w, b, gam, mean, var, CH.EPS, dwf, dbf, out=[t.clone() for t in prev], accumulate=True)
        assert all(same_bits(a, t + pv) for a, t, pv in zip(acc, got, prev)), 'accumulate adds the previous value last'
    measured('bn_fold / bn_unfold, worst error / bound', worst)
    assert worst <= 1.0


def test_fold_and_unfold_edges():
    c, k = 6, 18
    gen = torch.Generator().manual_seed(50)
    ints = lambda *s: torch.randint(-4, 5, s, generator=gen).float()        # noqa: E731
    # integer operands with var + eps = 4 exactly (eps = 0): s = gamma / 2, every product and sum exact -> bit equality
    w, b, gam, beta, mean, dwf, dbf = ints(c, k), ints(c), 2 * ints(c), ints(c), ints(c), ints(c, k), ints(c)
    gam[2] = 0.0                                                             # a gamma = 0 channel
    var = torch.full((c,), 4.0)
    wf, bf = ops.bn_fold(D(w), D(b), D(gam), D(beta), D(mean), D(var), 0.0)
    s = gam / 2
    assert same_bits(wf, D(s[:, None] * w)) and same_bits(bf, D(beta + s * (b - mean)))
    assert not bool(wf[2].any()) and float(bf[2]) == float(beta[2])
    dw, db, dg, dbeta = ops.bn_unfold(D(w), D(b), D(gam), D(mean), D(var), 0.0, D(dwf), D(dbf))
    assert same_bits(dw, D(s[:, None] * dwf)) and same_bits(db, D(s * dbf)) and same_bits(dbeta, D(dbf))
    assert same_bits(dg, D(((w * dwf).sum(1) + (b - mean) * dbf) / 2))
    assert not bool(dw[2].any()) and float(db[2]) == 0.0
    # var = 0 is finite with eps
    zero = torch.zeros(c)
    wf, bf = ops.bn_fold(D(w), D(b), D(gam), D(beta), D(mean), D(zero), CH.EPS)
    res = ops.bn_unfold(D(w), D(b), D(gam), D(mean), D(zero), CH.EPS, D(dwf), D(dbf))
    assert all(bool(torch.isfinite(t).all()) for t in (wf, bf) + tuple(res))
    ref = CH.unfold_ref(w, b, gam, mean, zero, dwf, 0.0, dbf, 0.0)
    assert max(worst_ratio(cpu(t), *ref[key]) for key, t in zip(('dw', 'db', 'dgamma', 'dbeta'), res)) <= 1.0
    # non-finite values in one channel stay in that channel
    clean = ops.bn_unfold(D(w), D(b), D(gam), D(mean), D(var), CH.EPS, D(dwf), D(dbf))
    clean_f = ops.bn_fold(D(w), D(b), D(gam), D(beta), D(mean), D(var), CH.EPS)
    for poison in (float('nan'), float('inf')):
        w2, dwf2, var2, dbf2 = w.clone(), dwf.clone(), var.clone(), dbf.clone()
        w2[3, 5], dwf2[3, 7], var2[3], dbf2[3] = poison, poison, poison, poison
        bad = ops.bn_unfold(D(w2), D(b), D(gam), D(mean), D(var2), CH.EPS, D(dwf2), D(dbf2))
        bad_f = ops.bn_fold(D(w2), D(b), D(gam), D(beta), D(mean), D(var2), CH.EPS)
        keep = [i for i in range(c) if i != 3]
        assert all(same_bits(a[keep], b_[keep]) for a, b_ in zip(bad + bad_f, clean + clean_f))
        assert not bool(torch.isfinite(bad[2][3]))


def test_wrappers_refuse_what_the_kernels_cannot_take():
    g, x = D(R((2, 64, 4, 6), 1)), D(R((2, 3, 8, 12), 2))
    for call in (lambda: ops.conv_stem_wgrad(g.cpu(), x), lambda: ops.conv_stem_wgrad(g, x[:, :, :7]),
                 lambda: ops.conv_stem_wgrad(g, D(R((2, 5, 8, 12), 3))), lambda: ops.conv_stem_wgrad(g, x, stride=1),
                 lambda: ops.conv_stem_wgrad(g, x, accumulate=True), lambda: ops.conv_stem_wgrad(g, x, workspace=D(R((8,), 4))),
                 lambda: ops.conv_ds_dgrad(g, D(R((64, 32, 3, 3), 5)), (8, 12)),
                 lambda: ops.conv_ds_dgrad(g, D(R((64, 32, 1, 1), 5)), (9, 12)),
                 lambda: ops.conv_ds_dgrad(g, D(R((64, 32, 1, 1), 5)), (8, 12), act=RELU),
                 lambda: ops.conv_ds_dgrad(g, D(R((64, 32, 1, 1), 5)), (8, 12), add=D(R((2, 32, 8, 11), 6))),
                 lambda: ops.conv_ds_wgrad(g, x[:1]), lambda: ops.conv_ds_wgrad(g, x.double()),
                 lambda: ops.channel_sum(g[:, :, :, ::2]), lambda: ops.channel_sum(g, out=D(R((3,), 7))),
                 lambda: ops.bn_fold(D(R((4, 9), 8)), *[D(R((5,), 9))] * 5, 1e-5),
                 lambda: ops.bn_unfold(D(R((4, 9), 8)), *[D(R((4,), 9))] * 4, 1e-5, D(R((4, 8), 8)), D(R((4,), 9)))):
        with pytest.raises(ScflowHipError):
            call()


# ======================================================================================================= the encoder
def build_encoder(sd, kind='BN'):
    enc = RAFTEncoder(3, CH.OUT_CHANNELS, norm_cfg=dict(type=kind))
    if kind == 'BN':
        missing, unexpected = enc.load_state_dict({k[len('context.'):]: v for k, v in sd.items()}, strict=False)
        assert not unexpected and all(k.endswith('num_batches_tracked') for k in missing)
    return enc.to(DEV)


def keep_forward(enc, x):
    with enc.keeping():
        y = enc(D(x), head_act=ops.ACT_TANH, head_act2=ops.ACT_RELU, head_split=CH.SPLIT)
    saved = enc.kept
    assert same_bits(saved['out'], y)
    return y, saved


HEAD = dict(head_act=ops.ACT_TANH, head_act2=ops.ACT_RELU, head_split=CH.SPLIT)


def check_launches(enc, im, grads, prefix=''):
    """every launch of RAFTEncoder.backward against its float64 restatement GIVEN its own operands (``intermediates``)
    -> {kind: worst error / bound}"""
    p = {k: cpu(v) for k, v in enc.state_dict().items()}
    worst = {}

    def note(kind, got, ref, bound):
        worst[kind] = max(worst.get(kind, 0.0), worst_ratio(cpu(got), ref, bound))

    def bn_layer(key, ckey, bkey, fold=True):
        rec = im[key]
        args = [p[f'{ckey}.weight'], p[f'{ckey}.bias'], p[f'{bkey}.weight'], p[f'{bkey}.bias'], p[f'{bkey}.running_mean'],
                p[f'{bkey}.running_var']]
        if fold:
            ref = CH.fold_ref(*args)
            note('fold', rec['wf'], ref[0], ref[1])
            note('fold', rec['bf'], ref[2], ref[3])
        un = CH.unfold_ref(args[0], args[1], args[2], args[4], args[5], cpu(rec['dwf']), 0.0, cpu(rec['dbf']), 0.0)
        for kind, name in (('dw', f'{ckey}.weight'), ('db', f'{ckey}.bias'), ('dgamma', f'{bkey}.weight'), ('dbeta', f'{bkey}.bias')):
            note('unfold', grads[prefix + name], *un[kind])
        return rec

    rec = im['head']
    ref = S1.wgrad_ref(cpu(rec['g']), 0.0, cpu(rec['x']), 1, 1)
    note('head wgrad', grads[prefix + 'conv2.weight'], ref[0], ref[1])
    note('head wgrad', grads[prefix + 'conv2.bias'], ref[2], ref[3])
    note('head dgrad', rec['gx'], *S1.dgrad_ref(cpu(rec['g']), 0.0, p['conv2.weight'], a=cpu(rec['x']), act=RELU))
    for key, _, _, stride in CH.BLOCKS:
        rec = bn_layer(f'{key}.conv2', f'{key}.conv2', f'{key}.bn2')
        g, x = cpu(rec['g']), cpu(rec['x'])
        ref = S1.wgrad_ref(g, 0.0, x, 3, 3)
        note('3x3 wgrad', rec['dwf'], ref[0], ref[1])
        note('3x3 wgrad', rec['dbf'], ref[2], ref[3])
        note('3x3 dgrad', rec['gx'], *S1.dgrad_ref(g, 0.0, cpu(rec['wf']), a=x, act=RELU))
        rec = bn_layer(f'{key}.conv1', f'{key}.conv1', f'{key}.bn1')
        g, x = cpu(rec['g']), cpu(rec['x'])
        if stride == 1:
            ref = S1.wgrad_ref(g, 0.0, x, 3, 3)
            note('3x3 wgrad', rec['dwf'], ref[0], ref[1])
            note('3x3 wgrad', rec['dbf'], ref[2], ref[3])
            note('3x3 dgrad', rec['gx'], *S1.dgrad_ref(g, 0.0, cpu(rec['wf']), add=cpu(rec['add']), a=x, act=RELU))
        else:
            hin, win = x.shape[2:]
            note('3x3 s2 wgrad', rec['dwf'], *CG.wgrad_ref(g, 0.0, x))
            note('channel sum', rec['dbf'], *CH.channel_sum_ref(g))
            note('3x3 s2 dgrad', rec['gx'], *CG.dgrad_ref(g, 0.0, cpu(rec['wf']), hin, win))
            rec = bn_layer(f'{key}.downsample', f'{key}.downsample.0', f'{key}.downsample.1')
            g = cpu(rec['g'])
            ref = CH.ds_wgrad_ref(g, 0.0, x)
            note('shortcut wgrad', rec['dwf'], ref[0], ref[1])
            note('shortcut wgrad', rec['dbf'], ref[2], ref[3])
            note('shortcut dgrad', rec['gx'], *CH.ds_dgrad_ref(g, 0.0, cpu(rec['wf']), hin, win, add=cpu(rec['add']), a=x, act=RELU))
    rec = bn_layer('conv1', 'conv1', 'bn1', fold=False)
    ref = CH.stem_wgrad_ref(cpu(rec['g']), 0.0, cpu(rec['x']))
    note('stem wgrad', rec['dwf'], ref[0], ref[1])
    note('stem wgrad', rec['dbf'], ref[2], ref[3])
    return worst


def compare_composed(tag, grads, saved, x, sd, g_out, prefix=''):
    """the 62 gradients against float64 autograd of the whole encoder (the oracle's graph, with the GPU forward's ReLU
    decisions at units within fp32 rounding of zero) -> worst max |g - g64| / max |g64|"""
    ties = []
    _, truth = CH.truth64(x, sd, g_out, relu=CH.relu_decisions(saved), ties=ties)
    for key, count, v in ties:
        measured(f'{tag}: ReLU units of {key} within fp32 rounding of zero and decided otherwise by the GPU forward: {count}; '
                 'worst |pre-activation| / allowed', v)
    worst = 0.0
    for name in CH.PARAM_NAMES:
        want = truth[name].numpy()
        assert np.abs(want).max() > 0, name
        worst = max(worst, float(np.abs(f64(grads[prefix + name]) - want).max() / np.abs(want).max()))
    return worst


@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('hw', [(18, 26), (16, 24)], ids=lambda v: f'{v[0]}x{v[1]}')
def test_encoder_backward_launch_by_launch(hw, n):
    sd = CH.encoder_params(CH.CASE_SEED)
    x, g = CH.encoder_inputs(CH.CASE_SEED, n, *hw)
    enc = build_encoder(sd)
    plain = enc(D(x), **HEAD)
    assert enc.kept == {}
    y, saved = keep_forward(enc, x)
    assert same_bits(y, plain), 'keeping changes the forward'
    assert sorted(saved) == sorted(['x', 'stem', 'out'] + [f'{k}{i}' for i in range(6) for k in 'ty'])
    im = {}
    grads = enc.backward(saved, D(g), **HEAD, intermediates=im)
    assert list(grads) and sorted(grads) == sorted(dict(enc.named_parameters())) and len(grads) == 62
    assert all(grads[k].shape == v.shape for k, v in enc.named_parameters())
    # the records come in launch order: the head, the blocks last to first (conv2, conv1, the shortcut), the stem
    assert list(im) == ['head'] + [f'res_layer{L}.{j}.{c}' for L in (3, 2, 1) for j in (1, 0)
                                   for c in ('conv2', 'conv1') + (('downsample',) if j == 0 and L > 1 else ())] + ['conv1']
    for kind, v in sorted(check_launches(enc, im, grads).items()):
        measured(f'RAFTEncoder.backward {hw} N {n}, {kind}: worst error / bound', v)
        assert v <= 1.0, kind
    v = compare_composed(f'{hw} N {n}', grads, saved, x, sd, g)
    measured(f'RAFTEncoder.backward {hw} N {n}, composed: worst max error / largest float64 entry', v)
    assert v <= CH.GOLDEN_ROOM
    # the cotangent as two channel slices, the head's output handed in: the same bits; a second run too
    again = enc.backward({k: v for k, v in saved.items() if k != 'out'}, (D(g[:, :CH.SPLIT]), D(g[:, CH.SPLIT:])),
                         out=saved['out'], **HEAD)
    assert all(same_bits(again[k], grads[k]) for k in grads)
    # accumulation doubles the bits
    into = {k: v.clone() for k, v in grads.items()}
    assert enc.backward(saved, D(g), **HEAD, param_grads=into) is into
    assert all(same_bits(into[k], grads[k] + grads[k]) for k in grads)
    pre = {'context.' + k: v.clone() for k, v in grads.items()}
    pre['other'] = D(R((3,), 1))
    enc.backward(saved, D(g), **HEAD, param_grads=pre, prefix='context.')
    assert all(same_bits(pre['context.' + k], grads[k] + grads[k]) for k in grads) and len(pre) == 63


def test_encoder_backward_against_the_reference_fixture():
    z = np.load(CH.GOLDEN)
    for hw in CH.GOLDEN_SIZES:
        tag, sd, x, g = CH.golden_case(hw)
        enc = build_encoder(sd)
        _, saved = keep_forward(enc, x)
        grads = enc.backward(saved, D(g), **HEAD)
        worst = 0.0
        for name in CH.PARAM_NAMES:
            got = CH.golden_pick(name, cpu(grads[name]).numpy())
            worst = max(worst, float(np.abs(f64(got) - f64(z[f'{tag}.{name}'])).max() / float(grads[name].abs().max())))
        measured(f'RAFTEncoder.backward against the reference module {tag}: worst max error / largest entry', worst)
        assert worst <= 2 * CH.GOLDEN_ROOM


def test_encoder_backward_errors():
    sd = CH.encoder_params(CH.CASE_SEED)
    x, g = CH.encoder_inputs(CH.CASE_SEED, 1, 16, 24)
    enc = build_encoder(sd)
    _, saved = keep_forward(enc, x)
    g = D(g)
    for key in ('x', 'stem', 't3', 'y5', 'out'):
        with pytest.raises(ScflowHipError, match='keeping'):
            enc.backward({k: v for k, v in saved.items() if k != key}, g, **HEAD)
    with pytest.raises(ScflowHipError, match='keeping'):
        enc.backward(None, g, **HEAD)
    for bad in ((g[:, :CH.SPLIT],), (g[:, :CH.SPLIT], g[:, CH.SPLIT:], g[:, :1]), (g[:, :100], g[:, 100:]), g[:, :, :1],
                (g[:, :CH.SPLIT, :1], g[:, CH.SPLIT:])):
        with pytest.raises(ScflowHipError, match='g_out'):
            enc.backward(saved, bad, **HEAD)
    with pytest.raises(ScflowHipError, match='out must be'):
        enc.backward(saved, g, out=saved['out'][:, :, :1], **HEAD)
    grads = enc.backward(saved, g, **HEAD)
    with pytest.raises(ScflowHipError, match='but not all'):
        enc.backward(saved, g, **HEAD, param_grads={'conv2.bias': grads['conv2.bias']})
    feat = build_encoder(None, kind='IN')
    with feat.keeping():
        feat(D(x))
    with pytest.raises(NotImplementedError, match='correlation-build backward'):
        feat.backward(feat.kept, g)
    enc(D(x))
    assert enc.kept == {} and not enc.keep


# ================================================================================================= the refiner's entry
def _get_pose(m, data):
    return m.get_pose(data['rendered_images'], data['real_images'], data['ref_rotations'], data['ref_translations'],
                      data['rendered_depths'], data['internel_k'], data['labels'])


def _same(a, b):
    if isinstance(a, dict):
        return sorted(a) == sorted(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return (a is None and b is None) or same_bits(a, b)


def test_loss_and_context_grads(scflow_model):  # noqa: F811
    m, case = scflow_model
    data = HL.refiner_data(case, DEV)
    before = _get_pose(m, data)
    loss_before = m.loss(None, data=data)
    base = m.loss_and_motion_grads(None, data=data)
    loss, log_imgs, log_vars, seq_r, seq_t, grads = m.loss_and_context_grads(None, data=data)
    assert same_bits(loss, base[0]) and list(log_vars.items()) == list(base[2].items()) and log_imgs is None
    assert _same(seq_r, base[3]) and _same(seq_t, base[4])
    assert sorted(grads) == sorted(base[5])
    ctx_names = {'context.' + k for k in dict(m.context.named_parameters())}
    assert set(grads['params']) == set(base[5]['params']) | ctx_names and len(ctx_names) == 62
    assert not ctx_names & set(base[5]['params'])
    for key, v in base[5].items():
        assert _same({k: grads[key][k] for k in v} if key == 'params' else grads[key], v), key
    assert m.context.kept == {} and not m.context.keep and m.decoder.keep == 'none'
    # the encoder's stage again, from the same cotangents: the same bits (test_encoder_backward_launch_by_launch holds every
    # launch of the stage to its bound, at sizes whose float64 restatements take seconds)
    rend = data['rendered_images'].contiguous()
    with m.context.keeping():
        y = m.context(rend, **HEAD)
    saved = m.context.kept
    kept = m.decoder.kept
    assert same_bits(y[:, :CH.SPLIT], kept['h0']) and same_bits(y[:, CH.SPLIT:], kept['c']), 'not the forward the decoder read'
    g_out = (grads['gru']['initial_hidden'], grads['gru']['context'])
    stage = m.context.backward(saved, g_out, **HEAD, prefix='context.')
    assert all(same_bits(stage[k], grads['params'][k]) for k in ctx_names) and len(stage) == 62
    # decoder + loss + context encoder as one float64 graph: the float64 chain of tests/test_chain_grad_host.py gives
    # d loss / d (h0, c) of decoder + loss from the decoder inputs of this forward; oracle.raft_encoder's graph (CH.truth64)
    # carries exactly those cotangents on, which is what one backward pass through the joined graph does at that cut
    import test_chain_grad_host as CC
    from test_gpu_chain_grad import relu_decisions
    feats = [t.clone() for t in m.extract_feat(data['rendered_images'], data['real_images'])]
    assert same_bits(feats[2], kept['h0']) and same_bits(feats[3], kept['c'])
    hdata = dict(CC.chain_data(case), gt_flow=m._supervision(data, True).cpu())
    res = CC.chain_ref64([f.cpu() for f in feats], CC.decoder_sd64(m.state_dict()), hdata, CC.chain_cfgs(case, 'raft'),
                         dict(CC.shipped_flags(), relu=relu_decisions(m)), iters=m.decoder.iters, variant='raft')
    g64 = torch.from_numpy(np.concatenate([res['initial_hidden'], res['context']], 1))
    sd = {k: v for k, v in m.state_dict().items() if k.startswith('context.') and not k.endswith('num_batches_tracked')}
    ties = []
    _, truth = CH.truth64(rend, sd, g64, relu=CH.relu_decisions(saved), ties=ties)
    for key, count, v in ties:
        measured(f'loss_and_context_grads: ReLU units of {key} within fp32 rounding of zero decided otherwise: {count}; '
                 'worst |pre-activation| / allowed', v)
    worst = 0.0
    for name in CH.PARAM_NAMES:
        want = truth[name].numpy()
        assert np.abs(want).max() > 0 and bool(grads['params']['context.' + name].any()), name
        worst = max(worst, float(np.abs(f64(grads['params']['context.' + name]) - want).max() / np.abs(want).max()))
    measured('loss_and_context_grads against the joined float64 graph: worst max error / largest float64 entry', worst)
    # the cotangents at (h0, c) are themselves inside 2 x the chain's room for that group (tests/test_gpu_chain_grad.py),
    # and the encoder adds its own GOLDEN_ROOM
    assert worst <= 2 * CC.ROOM['raft'][CC.group_of('initial_hidden')] + CH.GOLDEN_ROOM
    # plain calls before and after: the same bits, nothing kept
    after = _get_pose(m, data)
    assert _same(list(before), list(after)) and _same(loss_before[0], m.loss(None, data=data)[0])
    assert m.context.kept == {}
    with pytest.raises(NotImplementedError, match='loss_and_context_grads'):
        m.forward(data, return_loss=True)
    with pytest.raises(NotImplementedError, match='loss_and_motion_grads'):
        m.forward(data, return_loss=True)
