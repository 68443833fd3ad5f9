"""GPU: `SCFlowRefiner.loss_and_motion_grads()` as a WHOLE against d(loss)/d(everything) of decoder + loss as one float64
graph (`chain_ref64` of tests/test_chain_grad_host.py) and against the reference's own backward (chain_grads.npz).

The stage tests hold every backward stage to float64 given the GPU's own cotangent at the stage's output; a wrong join
between two stages (a cotangent handed to the wrong iteration, a dropped branch into hv, a wrong sequence weight, a
detach in the wrong place, parameter gradients not summed over the iterations) passes all of them.  Here the float64
chain starts from the decoder's four inputs as the GPU's forward produced them -- the encoders' fp32 rounding does not
enter -- and everything after is float64, so every key of `grads` has one independent truth.

Measure: max |g - g64| / max |g64| over all elements of a tensor (`CH.rel`).  Rooms: `CH.ROOM`, the same measure of the
reference's fp32 CPU autograd against the float64 chain, per loss variant and tensor group; the kernels are held to
2 x ROOM against float64.  Case B (12 x 20 maps, N = 2, T = 2) uses the same table, the shipped loss's; its sums are
shorter.  Measured values: DESIGN.md 4.13.

Against the fixture (3 x ROOM) the GPU's decoder is handed the FIXTURE's decoder inputs -- the fp32 CPU encoders' outputs
in place of its own encoders', the decoder, the loss and the whole backward unchanged -- so that the reference's fp32
backward and the kernels are two fp32 evaluations around one float64 value, and the GPU's result goes through the
fixture's pick as it is.

ReLU units within fp32 rounding of zero: the GPU's forward decides one or two of the fixture case's ~5e6 units otherwise
than float64 (measured: pre-activations of 5e-8 against sums of magnitude ~4), and one such unit alone puts the
cotangents behind it ~5e-3 of their largest entry away from the float64 chain -- no stage's or join's error.  The chain
is therefore given the GPU forward's decisions (`relu_decisions`) and takes them at exactly those units
(`chain_ref64`, which prints how many); every element stays compared, at the unchanged rooms.  The reference's forward
decided every unit as float64 does, so against the fixture the float64 effect of exactly those units (the chain with
them minus the chain without, same inputs) is taken off the GPU's result; with no such unit nothing is taken off."""
import numpy as np
import pytest
import torch

import scflow_amd
from scflow_amd import ops
import test_chain_grad_host as CH
import test_loss_host as HL
from test_stream_ops_host import measured, same_bits  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def gpu_view(grads):
    """the refiner's `grads` under the keys of a chain result (`CH.flat` reads both): what each depth returns, where it
    returns it"""
    seq = lambda v: [host(t) for t in v]                                         # noqa: E731
    out = dict(params={k: host(v) for k, v in grads.get('params', {}).items()})
    for key in ('sequence_flow_from_pred', 'sequence_masks', 'seq_rotations', 'seq_translations', 'sequence_flow_from_pose',
                'delta_rotation_preds', 'delta_translation_preds'):
        if key in grads:
            out[key] = seq(grads[key])
    if 'delta_flow_preds' in grads:             # the top-level pair is the tail's part: through the up-sampled outputs alone
        out['delta_flow_tail'], out['masks_tail'] = seq(grads['delta_flow_preds']), seq(grads['masks'])
    if 'decoder_heads' in grads:
        dh = grads['decoder_heads']
        out.update(hidden_states=seq(dh['hidden_states']), delta_flow_preds=seq(dh['delta_flow_preds']),
                   mask_logits=seq(dh['mask_logits']))
    if 'gru' in grads:
        out.update(initial_hidden=host(grads['gru']['initial_hidden']), context=host(grads['gru']['context']),
                   motion_features=seq(grads['gru']['motion_features']))
    if 'motion' in grads:
        out.update(correlation=host(grads['motion']['correlation']), flow_inputs=seq(grads['motion']['flow_inputs']))
    return out


def flat_gpu(view):
    out = dict(view['params'])
    out.update((k, view[k]) for k in CH.INPUT_KEYS if k in view)
    for k in CH.ITER_KEYS:
        if k in view:
            out.update((f'{k}.{t}', v.reshape(-1, *v.shape[1:])) for t, v in enumerate(view[k]))
    return out


def build(variant, iters, decoder=None, shapes_file='state_dict_keys.json', fc1_in=None, case=None, label_mode=0):
    case = HL.refiner_loss_case() if case is None else case
    cfg = scflow_amd.scflow_model_cfg(iters=iters)
    cfg.update(CH.chain_cfgs(case, variant))
    cfg['decoder'].update(decoder or {})
    if fc1_in is not None:
        cfg['decoder']['pose_head_cfg']['feat_size'] = FEAT_SIZE_B
    m = scflow_amd.build_refiner(cfg)
    m.load_state_dict(CH.state_dict(CH.FIXTURE_SEEDS['weight_seed'], shapes_file, fc1_in), strict=True)
    m = m.to(DEV)
    if variant == 'shipped':
        m._build_loss_funcs()
        m.pose_loss_func.loss_func.meshes = [torch.from_numpy(v) for v in case['verts']]
    m.decoder.pose_pred.label_mode = label_mode
    return m, case


def relu_decisions(m):
    """the ReLU decisions of the GPU's forward, layer by layer and iteration by iteration, from what the forward kept
    (`decoder.kept` at keep level 'motion') and the FORWARD's own modules run again on it; nothing of the backward
    is read -> {(oracle layer prefix, t): bool}.  The float64 chain reads them only at units whose float64
    pre-activation lies within fp32 rounding of zero (`chain_ref64`).  The pose head's GroupNorm + ReLU and fully
    connected ReLUs are not handed over."""
    dec = m.decoder
    enc, kept = dec.encoder, dec.kept
    ch, cdf = dec.flow_pred.layers[0].conv.out_channels, dec.delta_flow_encoder[1].conv.out_channels
    out = {}
    for t in range(dec.iters):
        heads = ops.conv2d(dec.packed, kept['hv'][t].contiguous(), act=ops.ACT_RELU)
        out['decoder.flow_pred.layers.0', t], out['decoder.mask_pred.layers.0', t] = heads[:, :ch] > 0, heads[:, ch:] > 0
        out['decoder.delta_flow_encoder.1', t], out['decoder.mask_encoder.1', t] = kept['dm'][t][:, :cdf] > 0, kept['dm'][t][:, cdf:] > 0
        out['decoder.delta_flow_encoder.0', t] = dec.delta_flow_encoder[0](kept['d_flow'][t].contiguous()) > 0
        out['decoder.mask_encoder.0', t] = dec.mask_encoder[0](kept['mask'][t].contiguous()) > 0
        out['decoder.encoder.out_net.0', t] = kept['x'][t][:, :126] > 0
        corr = ops.corr_lookup(kept['pyramid'], kept['flow_lr'][t], dec.radius, tiled_levels=kept['tiled'])
        if dec.mask_corr:
            corr = ops.mul_mask(corr, torch.ones_like(kept['mask'][0]) if t == 0 else kept['mask'][t - 1])
        c1 = enc.corr_net[0](corr)
        f1 = enc.flow_net[0](kept['x'][t][:, 126:].contiguous())
        out['decoder.encoder.corr_net.0', t], out['decoder.encoder.flow_net.0', t] = c1 > 0, f1 > 0
        out['decoder.encoder.corr_net.1', t], out['decoder.encoder.flow_net.1', t] = enc.corr_net[1](c1) > 0, enc.flow_net[1](f1) > 0
    return {k: v.cpu() for k, v in out.items()}


def run(m, case, variant, flags, feats=None):
    """one call of loss_and_motion_grads() and the float64 chain from the same decoder inputs -> (the entry's tuple, the
    chain result).  ``feats`` None: the decoder inputs of the GPU's own encoders.  Else the four (host) tensors the GPU's
    decoder is handed in their place: `extract_feat`, the one call get_pose makes before the decoder, returns them."""
    data = HL.refiner_data(case, DEV)
    if feats is None:
        # the same encoder call get_pose makes; the decoder consumes get_pose's own buffers, not these
        feats = [t.clone() for t in m.extract_feat(data['rendered_images'], data['real_images'])]
        out = m.loss_and_motion_grads(None, data=data)
    else:
        feats = [t.detach().to(DEV).contiguous() for t in feats]
        m.extract_feat = lambda render_images, real_images: tuple(t.clone() for t in feats)
        try:
            out = m.loss_and_motion_grads(None, data=data)
        finally:
            del m.extract_feat
    kept = m.decoder.kept
    assert same_bits(kept['h0'], feats[2]) and same_bits(kept['c'], feats[3]), 'the decoder did not start from these inputs'
    hdata = dict(CH.chain_data(case), gt_flow=m._supervision(data, True).cpu())
    res = CH.chain_ref64([f.cpu() for f in feats], CH.decoder_sd64(m.state_dict()), hdata, CH.chain_cfgs(case, variant),
                         dict(flags, relu=relu_decisions(m)), iters=m.decoder.iters, variant=variant)
    for layer, t, count, worst in res['ties']:
        measured(f'{variant} loss: ReLU units of {layer}, iteration {t}, within fp32 rounding of zero and decided otherwise '
                 f'by the GPU forward: {count}; worst |pre-activation| / rounding bound', worst)
    return out, res


def compare(tag, variant, grads, res, factor=2.0):
    """every key the GPU returned against the float64 chain -> the compared keys; asserts measure <= factor x ROOM"""
    got, want = flat_gpu(gpu_view(grads)), CH.flat(res)
    assert set(got) <= set(want), sorted(set(got) - set(want))
    worst, over = {}, []
    for k, g in got.items():
        v = CH.rel(g.reshape(want[k].shape), want[k])
        group = CH.group_of(k)
        if v >= worst.get(group, (-1.0, ''))[0]:
            worst[group] = (v, k)
        if not v <= factor * CH.ROOM[variant][group]:
            over.append((k, v, CH.ROOM[variant][group]))
    for group, (v, k) in sorted(worst.items()):
        measured(f'{tag}, {variant} loss, {group}: worst max error / largest float64 entry ({k}), in rooms '
                 f'{v / CH.ROOM[variant][group]:.3g}; value', v)
    assert not over, over
    return set(got)


# ====================================================================================================== case A: the fixture's
@pytest.fixture(scope='module')
def case_a():
    """variant -> (model, case, loss_and_motion_grads()'s tuple, float64 chain), computed once per variant"""
    runs = {}

    def get(variant):
        if variant not in runs:
            m, case = build(variant, HL.REFINER_ITERS)
            runs[variant] = (m, case) + run(m, case, variant, CH.shipped_flags())
        return runs[variant]
    return get


@pytest.mark.parametrize('variant', CH.VARIANTS)
def test_fixture_case_against_the_float64_chain(case_a, variant):
    m, case, out, res = case_a(variant)
    loss, log_imgs, log_vars, seq_r, seq_t, grads = out
    assert abs(float(loss) - res['loss']) <= 1e-4 * abs(res['loss'])
    if variant == 'shipped':                    # the GPU's neighbours are the float64 forward's: the same constants
        pl = m.pose_loss_func.loss_func
        data = HL.refiner_data(case, DEV)
        nn = pl.sequence(seq_r, seq_t, data['gt_rotations'], data['gt_translations'], data['labels'],
                         scale_factors=data['scale_factors'], return_nn=True)[3].cpu().numpy()
        want = res['nn']
        assert all(np.array_equal(nn[t, n][:int((want[t, n] >= 0).sum())], want[t, n][want[t, n] >= 0])
                   for t in range(want.shape[0]) for n in range(want.shape[1]))
    keys = compare('fixture case 32 x 32, N 3, T 3', variant, grads, res)
    dec = m.decoder
    names = {'decoder.' + k for k in dict(dec.named_parameters())}
    assert {k for k in keys if k.startswith('decoder.')} == names, 'a decoder parameter is not compared'
    T = dec.iters
    per_iter = ['hidden_states', 'motion_features', 'flow_inputs', 'delta_flow_preds', 'mask_logits', 'delta_flow_tail',
                'masks_tail', 'delta_rotation_preds', 'delta_translation_preds']
    assert keys >= set(CH.INPUT_KEYS) | {f'{k}.{t}' for k in per_iter for t in range(T)}


@pytest.mark.parametrize('variant', CH.VARIANTS)
def test_fixture_case_against_the_reference_backward(case_a, variant):
    """the kernels against the reference's own fp32 backward (chain_grads.npz) through the fixture's pick, three rooms.
    The GPU's decoder starts from the fixture's decoder inputs (`run` with ``feats``), so both are fp32 evaluations of ONE
    function at ONE point.  The only thing taken off the GPU's result is the float64 effect of the ReLU units within
    rounding of zero that its forward decides otherwise than float64 and the reference (module docstring): zero when there
    is none.  The same run is also held to the float64 chain at these inputs, two rooms."""
    m, case = case_a(variant)[:2]
    out, res = run(m, case, variant, CH.shipped_flags(), feats=CH.fixture_decoder_inputs())
    compare('fixture case from the fixture\'s decoder inputs', variant, out[5], res)
    z = np.load(CH.GOLDEN)
    got, want = flat_gpu(gpu_view(out[5])), CH.flat(res)
    units = sum(t[2] for t in res['ties'])
    own = CH.flat(CH.fixture_case(variant)[1]) if units else want            # the chain at the same inputs, its own decisions
    worst, raw, seen = {}, {}, 0
    for k in CH.golden_keys(res):
        if k not in got:                        # the complete hidden-state cotangent stays inside gru_backward
            assert k.startswith('hidden_total.'), k
            continue
        seen += 1
        g = got[k].reshape(want[k].shape)
        group = CH.group_of(k)
        worst[group] = max(worst.get(group, 0.0), CH.rel(CH.golden_pick(k, g - (want[k] - own[k])), z[f'{variant}.{k}']))
        as_it_is = CH.rel(CH.golden_pick(k, g), z[f'{variant}.{k}'])
        raw[group] = max(raw.get(group, 0.0), as_it_is)
        # what no handed-over ReLU layer lies behind -- the pose head's parameters and the cotangents at its outputs -- is
        # held as it is, whatever the forward decided elsewhere
        if k.startswith('decoder.pose_pred.') or k.split('.')[0] in ('delta_rotation_preds', 'delta_translation_preds'):
            assert as_it_is <= 3.0 * CH.ROOM[variant][group], (k, as_it_is)
    assert abs(float(out[0]) - float(z[f'{variant}.loss'])) <= 1e-4 * abs(float(z[f'{variant}.loss']))
    for group, v in sorted(worst.items()):
        measured(f'kernels - reference fixture, {variant} loss, {group}: as it is, max distance / largest entry', raw[group])
        measured(f'kernels - reference fixture, {variant} loss, {group}: less the float64 effect of {units} ReLU units, in '
                 f'rooms {v / CH.ROOM[variant][group]:.3g}; value', v)
    for group, v in sorted(worst.items()):
        assert v <= 3.0 * CH.ROOM[variant][group], group
        assert units or raw[group] == v
    assert sorted(worst) == sorted(CH.ROOM[variant]) and seen >= len(dict(m.decoder.named_parameters())) + 3


# ====================================================================================================== case C: consistency
def _same(a, b):
    if isinstance(a, dict):
        return sorted(a) == sorted(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return same_bits(a, b)


def test_the_chain_keeps_its_bits_across_calls_and_loop_forms(case_a):
    m, case, out, _ = case_a('shipped')
    data = HL.refiner_data(case, DEV)
    dec = m.decoder
    old = dec.c_iteration
    assert old is True
    try:
        again = m.loss_and_motion_grads(None, data=data)
        assert same_bits(again[0], out[0]) and _same(again[5], out[5]), 'two calls differ'
        dec.c_iteration = False
        plain = m.loss_and_motion_grads(None, data=data)
        assert same_bits(plain[0], out[0]) and _same(plain[5], out[5]), 'the two loop forms differ'
    finally:
        dec.c_iteration = old


# ====================================================================================================== case B: small, non-square
H_B, W_B, N_B, T_B = 96, 160, 2, 2             # maps 12 x 20; levels 12 x 20, 6 x 10, 3 x 5, 1 x 2
FEAT_SIZE_B = (16, 24)                          # pose_head.py sizes fc1 by int(int(int(h w / 4) / 4) / 4): 12 x 20 maps end as
FC1_IN_B = 128 * 2 * 3                          # 128 x 2 x 3 = 768 features, which a (16, 24) declaration gives
SEEDS_B = dict(input_seed=3, case_seed=4)
# name -> (decoder config, chain flags, state-dict shapes, label_mode); all under the shipped loss and its rooms
CASES_B = {
    'shipped': ({}, {}, 'state_dict_keys.json', 0),
    'masked': (dict(mask_flow=True, mask_corr=True, detach_mask=True), dict(mask_flow=True, mask_corr=True),
               'state_dict_keys.json', 0),
    'conv_gru_r3': (dict(gru_type='Conv', radius=3), dict(radius=3), 'state_dict_keys_conv_gru_r3.json', 0),
    'linear_depth': (dict(depth_transform='linear', detach_depth_for_xy=True), dict(depth_transform='linear'),
                     'state_dict_keys.json', 0),
    'label_per_sample': ({}, dict(label_mode=1), 'state_dict_keys.json', 1),
}


@pytest.mark.parametrize('name', list(CASES_B))
def test_small_non_square_case_against_the_float64_chain(name):
    """loss_and_motion_grads() refuses none of these configurations (a refusal fails the test by its name)"""
    variant = 'shipped'
    dec_cfg, flags, shapes_file, label_mode = CASES_B[name]
    case = CH.chain_case(N_B, H_B, W_B, **SEEDS_B)
    assert len(set(case['labels'])) == N_B, 'the labels must differ across the batch'
    m, _ = build(variant, T_B, dec_cfg, shapes_file, FC1_IN_B, case, label_mode)
    out, res = run(m, case, variant, CH.shipped_flags(**flags))
    assert abs(float(out[0]) - res['loss']) <= 1e-4 * abs(res['loss'])
    keys = compare(f'12 x 20, N 2, T 2, {name}', variant, out[5], res)
    assert {k for k in keys if k.startswith('decoder.')} == {'decoder.' + k for k in dict(m.decoder.named_parameters())}
    assert keys >= set(CH.INPUT_KEYS)
