"""GPU: `SCFlowRefiner.loss_and_network_grads()` -- the rung that carries `loss_and_context_grads()` through the correlation
build (`SCFlowDecoder.corr_backward`) and the feature encoder(s) (`RAFTEncoder.in_backward`), so that `grads['params']`
covers all of `named_parameters()`.

* every key `loss_and_context_grads()` returns keeps its key and its bits; loss and log_vars are `loss()`'s;
* `features` and the encoder gradients are, bit for bit, the pieces called by hand: the context rung, `ops.corr_build_grad`,
  `feature_grads`;
* `features` against float64: the float64 chain of tests/test_chain_grad_host.py from the GPU's own decoder inputs, its
  volume cotangent carried through `corr_build_grad64` (the join tests/test_corr_grad_host.py holds to one-graph autograd),
  max |g - g64| / max |g64| within 2 x KH.ROOM; from the FIXTURE's decoder inputs also within 3 x KH.ROOM of the
  reference's own backward (network_grads.npz), the factors and their reason being tests/test_chain_grad_host.py's;
* the encoder gradients, at both cases, against float64 autograd of the encoder (FH.truth64, the GPU forward's ReLU
  decisions at units within fp32 rounding of zero, as everywhere) FROM THE FLOAT64 JOIN'S COTANGENT, end to end, inside
  DESIGN.md 4.17's composed room (FH.GOLDEN_ROOM, FH.ZERO_BIAS_ROOM); at the fixture case also within 3 x KH.ROOM of the
  reference's own backward through the whole network (network_grads.npz)."""
import numpy as np
import pytest
import torch

import scflow_amd
from scflow_amd import ops
from scflow_amd.optim import AdamW
import test_chain_grad_host as CH
import test_corr_grad_host as KH
import test_feature_grad_host as FH
import test_loss_host as HL
from test_gpu_chain_grad import FC1_IN_B, H_B, N_B, SEEDS_B, T_B, W_B, build, relu_decisions
from test_stream_ops_host import f64, measured, same_bits

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
cpu = lambda t: t.detach().cpu()                                    # noqa: E731


def _same(a, b):
    if isinstance(a, dict):
        return sorted(a) == sorted(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, torch.Tensor):
        return same_bits(a, b)
    return a == b


def _cases():
    small = CH.chain_case(N_B, H_B, W_B, **SEEDS_B)
    return {'small': (T_B, dict(fc1_in=FC1_IN_B, case=small)), 'fixture': (HL.REFINER_ITERS, {})}


@pytest.fixture(scope='module')
def runs():
    """(case name, variant) -> dict(m, case, data, net, ctx): the model and one call of each rung, computed once"""
    done = {}

    def get(name, variant='shipped'):
        if (name, variant) not in done:
            iters, kw = _cases()[name]
            m, case = build(variant, iters, **kw)
            data = HL.refiner_data(case, DEV)
            net = m.loss_and_network_grads(None, data=data)
            assert m.render_encoder.kept == {} and m.context.kept == {} and not m.render_encoder.keep
            ctx = m.loss_and_context_grads(None, data=data)
            done[name, variant] = dict(m=m, case=case, data=data, net=net, ctx=ctx)
        return done[name, variant]
    return get


def by_hand(m, data, g_vol):
    """the pieces of the rung called by hand -> (feats of a keeping forward, (g_render, g_real), the kept activations'
    ReLU decisions, the encoder gradients)"""
    fe = m.render_encoder
    with fe.keeping():
        feats = m.extract_feat(data['rendered_images'].contiguous(), data['real_images'].contiguous())
    decisions = FH.relu_decisions(fe.kept)
    g = ops.corr_build_grad(g_vol, feats[0], feats[1])
    return feats, g, decisions, m.feature_grads(*g)


@pytest.mark.parametrize('name', ['small', 'fixture'])
def test_shared_keys_keep_their_bits_and_the_rest_is_the_pieces_by_hand(runs, name):
    r = runs(name)
    m, net, ctx = r['m'], r['net'], r['ctx']
    assert len(net) == 6 and net[1] is None
    plain = m.loss(None, data=r['data'])
    assert same_bits(net[0], plain[0]) and net[2] == plain[2] and _same(net[3], plain[3]) and _same(net[4], plain[4])
    assert all(_same(a, b) for a, b in zip(net[:5], ctx[:5]))
    g_net, g_ctx = net[5], ctx[5]
    assert sorted(set(g_net) - set(g_ctx)) == ['features'] and sorted(g_net['features']) == ['real', 'render']
    for k in g_ctx:
        if k == 'params':
            assert all(same_bits(g_net[k][p], v) for p, v in g_ctx[k].items())
        else:
            assert _same(g_net[k], g_ctx[k]), k
    named = dict(m.named_parameters())
    assert sorted(g_net['params']) == sorted(named) and len(named) == len(g_ctx['params']) + 32
    assert all(g_net['params'][k].shape == v.shape for k, v in named.items())
    feats, g, _, enc = by_hand(m, r['data'], g_ctx['motion']['correlation'])
    assert same_bits(g[0], g_net['features']['render']) and same_bits(g[1], g_net['features']['real'])
    assert sorted(enc) == sorted(set(g_net['params']) - set(g_ctx['params']))
    assert all(same_bits(g_net['params'][k], v) for k, v in enc.items())
    assert tuple(g[0].shape) == tuple(feats[0].shape) and all(bool(torch.isfinite(v).all()) for v in g)
    again = m.loss_and_network_grads(None, data=r['data'])
    assert same_bits(again[0], net[0]) and _same(again[5], g_net), 'two calls differ'


def chain_from(m, case, variant, feats, data):
    """the float64 chain from the decoder inputs ``feats`` with the ReLU decisions of the forward m.decoder.kept is from"""
    hdata = dict(CH.chain_data(case), gt_flow=m._supervision(data, True).cpu())
    res = CH.chain_ref64([cpu(f) for f in feats], CH.decoder_sd64(m.state_dict()), hdata, CH.chain_cfgs(case, variant),
                         dict(CH.shipped_flags(), relu=relu_decisions(m)), iters=m.decoder.iters, variant=variant)
    for layer, t, count, worst in res['ties']:
        measured(f'{variant} loss: ReLU units of {layer}, iteration {t}, within fp32 rounding of zero and decided otherwise '
                 f'by the GPU forward: {count}; worst |pre-activation| / rounding bound', worst)
    return res


def against_float64(tag, r, variant='shipped'):
    """one case of `runs`: features within 2 x ROOM of the float64 join from the GPU's own decoder inputs; the encoder
    gradients inside 4.17's room of float64 autograd from that float64 cotangent -> (the GPU's 32 gradients as float64
    arrays, the float64 ones)"""
    m, case, data, grads = r['m'], r['case'], r['data'], r['net'][5]
    feats, _, decisions, _ = by_hand(m, data, grads['motion']['correlation'])
    assert same_bits(m.decoder.kept['h0'], feats[2]) and same_bits(m.decoder.kept['c'], feats[3])
    res = chain_from(m, case, variant, feats, data)
    want = KH.join64(res, [cpu(f) for f in feats[:2]])
    got = (grads['features']['render'], grads['features']['real'])
    v = max(CH.rel(f64(a), b) for a, b in zip(got, want))
    measured(f'{tag}: features, max error / largest float64 entry, in rooms {v / KH.ROOM[variant]["features"]:.3g}; value', v)
    assert v <= 2.0 * KH.ROOM[variant]['features']
    params = {k[len('render_encoder.'):]: f64(p) for k, p in grads['params'].items() if k.startswith('render_encoder.')}
    assert sorted(params) == sorted(FH.PARAM_NAMES)
    ties = []
    truth, scales = KH.encoder_truth64((data['rendered_images'], data['real_images']), cpu_sd(m), want, relu=decisions, ties=ties)
    for key, count, w in ties:
        measured(f'{tag}: ReLU units of {key} within fp32 rounding of zero and decided otherwise by the GPU forward: {count}; '
                 'worst |pre-activation| / allowed', w)
    worst = KH.network_measures(KH.network_flat(got, params), KH.network_flat(want, truth), scales)
    measured(f'{tag}: encoder gradients from the float64 join, worst max error / largest float64 entry', worst['render_encoder'])
    measured(f'{tag}: encoder gradients from the float64 join, worst |zero bias gradient| / sum |du|', worst['zero_bias'])
    assert worst['render_encoder'] <= FH.GOLDEN_ROOM and worst['zero_bias'] <= FH.ZERO_BIAS_ROOM
    return params, truth, scales


def test_small_case_against_float64(runs):
    against_float64('12 x 20, N 2, T 2', runs('small'))


def test_fixture_case_against_float64_and_the_reference(runs):
    """the fixture case from the GPU's OWN encoders: features and encoder gradients against float64 as at the small case,
    and the encoder gradients against the reference's own backward through the whole network (network_grads.npz, through
    the fixture's pick): 3 x KH.ROOM, two fp32 evaluations around one float64 value"""
    variant = 'shipped'
    params, _, scales = against_float64('fixture case 32 x 32, N 3, T 3', runs('fixture'), variant)
    z = np.load(KH.GOLDEN)
    worst, worst0 = 0.0, 0.0
    for name in FH.PARAM_NAMES:
        have, want = FH.golden_pick(name, params[name]), f64(z[f'{variant}.render_encoder.{name}'])
        assert have.shape == want.shape, name
        if name in FH.ZERO_BIASES:
            worst0 = max(worst0, float((np.abs(have - want) / scales[name]).max()))
        else:
            worst = max(worst, float(np.abs(have - want).max() / np.abs(params[name]).max()))
    room = KH.ROOM[variant]
    measured(f'fixture case: encoder gradients vs the reference\'s backward, in rooms {worst / room["render_encoder"]:.3g}; value', worst)
    measured(f'fixture case: zero-bias gradients vs the reference\'s backward / sum |du|, in rooms {worst0 / room["zero_bias"]:.3g}; value', worst0)
    assert worst <= 3.0 * room['render_encoder'] and worst0 <= 3.0 * room['zero_bias']


def cpu_sd(m):
    return {k: cpu(v) for k, v in m.state_dict().items()}


@pytest.mark.parametrize('variant', CH.VARIANTS)
def test_features_from_the_fixture_inputs_against_float64_and_the_reference(variant):
    """the GPU's decoder handed the FIXTURE's decoder inputs (as tests/test_gpu_chain_grad.py does), the context rung, then
    `corr_backward` on those same feature maps: two rooms of float64, three of the reference's own backward, less the
    float64 effect of the ReLU units the GPU forward decided otherwise (zero when there is none)"""
    m, case = build(variant, HL.REFINER_ITERS)
    data = HL.refiner_data(case, DEV)
    feats = [t.detach().to(DEV).contiguous() for t in CH.fixture_decoder_inputs()]
    m.extract_feat = lambda render_images, real_images: tuple(t.clone() for t in feats)
    try:
        out = m.loss_and_motion_grads(None, data=data)
    finally:
        del m.extract_feat
    got = m.decoder.corr_backward(feats[0], feats[1], out[5]['motion']['correlation'])
    res = chain_from(m, case, variant, feats, data)
    want = KH.join64(res, [cpu(f) for f in feats[:2]])
    v = max(CH.rel(f64(a), b) for a, b in zip(got, want))
    room = KH.ROOM[variant]['features']
    measured(f'fixture\'s decoder inputs, {variant}: features vs float64, in rooms {v / room:.3g}; value', v)
    assert v <= 2.0 * room
    z = np.load(KH.GOLDEN)
    units = sum(t[2] for t in res['ties'])
    own = KH.fixture_truth(variant)[0] if units else want
    for name, a, b, c in zip(('render', 'real'), got, want, own):
        d = CH.rel(KH.feature_pick(f64(a) - (b - c)), z[f'{variant}.features.{name}'])
        measured(f'fixture\'s decoder inputs, {variant}: features.{name} vs the reference\'s backward, less the float64 effect '
                 f'of {units} ReLU units, in rooms {d / room:.3g}; value', d)
        assert d <= 3.0 * room


def test_separate_encoders_give_both_prefixes(runs):
    case = runs('small')['case']
    cfg = scflow_amd.scflow_model_cfg(iters=T_B)
    cfg.update(CH.chain_cfgs(case, 'raft'))
    cfg['seperate_encoder'] = True
    cfg['decoder']['pose_head_cfg']['feat_size'] = (16, 24)
    torch.manual_seed(11)
    m = scflow_amd.build_refiner(cfg).to(DEV)
    assert m.render_encoder is not m.real_encoder
    data = HL.refiner_data(case, DEV)
    out = m.loss_and_network_grads(None, data=data)
    params = out[5]['params']
    named = dict(m.named_parameters())
    assert len(params) == 181 and sorted(params) == sorted(named)
    assert sum(k.startswith('render_encoder.') for k in params) == 32 and sum(k.startswith('real_encoder.') for k in params) == 32
    assert m.render_encoder.kept == {} and m.real_encoder.kept == {} and m.context.kept == {}
    # by hand: two passes from the two cotangents
    fe, re_ = m.render_encoder, m.real_encoder
    with fe.keeping(), re_.keeping():
        feats = m.extract_feat(data['rendered_images'].contiguous(), data['real_images'].contiguous())
    g = ops.corr_build_grad(out[5]['motion']['correlation'], feats[0], feats[1])
    assert same_bits(g[0], out[5]['features']['render']) and same_bits(g[1], out[5]['features']['real'])
    enc = m.feature_grads(*g)
    assert len(enc) == 64 and all(same_bits(params[k], v) for k, v in enc.items())
    assert all(bool(v.any()) for k, v in enc.items() if k.endswith('.weight'))


def test_refusals_are_the_motion_rungs_and_nothing_stays_kept():
    case = CH.chain_case(N_B, H_B, W_B, **SEEDS_B)
    for over in (dict(detach_flow=False), dict(mask_flow=True, detach_mask=False)):
        m, _ = build('shipped', T_B, over, fc1_in=FC1_IN_B, case=case)
        data = HL.refiner_data(case, DEV)
        with pytest.raises(NotImplementedError):
            m.loss_and_motion_grads(None, data=data)
        with pytest.raises(NotImplementedError):
            m.loss_and_network_grads(None, data=data)
        assert m.render_encoder.kept == {} and m.context.kept == {} and not m.render_encoder.keep


def test_one_adamw_step_over_all_named_parameters(runs):
    """a hand-made optimizer step over the whole network: every feature-encoder tensor moves and the next forward runs"""
    case = runs('small')['case']
    m, _ = build('shipped', T_B, fc1_in=FC1_IN_B, case=case)
    data = HL.refiner_data(case, DEV)
    named = list(m.named_parameters())
    before = {k: p.detach().clone() for k, p in named}
    opt = AdamW(named, lr=1e-3)
    out = m.loss_and_network_grads(None, data=data)
    opt.step(out[5]['params'])
    m.invalidate_packed()
    moved = [k for k, p in named if not same_bits(p, before[k])]
    assert sorted(k for k in moved if k.startswith('render_encoder.')) == sorted(k for k, _ in named if k.startswith('render_encoder.'))
    assert len(moved) == len(named)
    after = m.loss(None, data=data)
    assert bool(torch.isfinite(after[0])) and not same_bits(after[0], out[0])
