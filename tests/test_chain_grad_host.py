"""CPU: the joined decoder backward as ONE float64 graph -- `chain_ref64`: oracle.scflow_decoder (with its autograd-only
detach flags) in float64 from the decoder's four inputs, under a float64 torch statement of the refiner's loss wiring
(`torch_wiring_total` of tests/test_loss_grad_host.py), differentiated by one `torch.autograd.grad` call.  It returns what
`SCFlowRefiner.loss_and_motion_grads()` returns under the same keys: every decoder parameter gradient, the cotangents at
h0, at the context and at level 0 of the correlation pyramid, and per iteration the cotangents at the hidden state, the
motion features, the encoder's flow input and the head outputs.  The stage tests hold every stage to float64 GIVEN the
GPU's own cotangent at the stage's output; this holds the JOINS: which cotangent is handed to which stage, for which
iteration, with which sequence weight, and where the detach flags cut the graph.

The measure of a tensor g against its float64 value g64 is max |g - g64| / max |g64| over ALL elements (`rel`).  The room
of a tensor group (`ROOM`) is that measure of the REFERENCE's own fp32 CPU autograd (tests/golden/chain_grads.npz:
`.backward()` on the total its `SCFlowRefiner.loss` returns, make_golden_chain_grad.py) against the float64 chain at the
fixture's inputs: it is measured by `test_chain_equals_the_reference_autograd`, written down in `ROOM`, and that test
then holds the reference to 1.5 x the recorded value (regeneration noise across BLAS thread counts).  The GPU tests
(tests/test_gpu_chain_grad.py) hold the kernels to 2 x ROOM against float64 and, from the fixture's decoder inputs, to
3 x ROOM against the fixture.  A planted
join defect must leave at least one tensor 10 x its room away (`test_planted_join_defects_leave_the_room`), so the factor
2 stays five times below every defect.

One thing an fp32 forward does not inherit from the float64 one: the derivative of a ReLU whose pre-activation lies
within fp32 rounding of zero.  Of the fixture case's ~5e6 ReLU units about one per run is decided otherwise by an fp32
evaluation, and one such unit moves the cotangents behind it by ~5e-3 of their largest entry, a thousand rooms.
`chain_ref64` therefore accepts the decisions of the fp32 forward under test (`flags['relu']`) and differentiates at
them where, and only where, the float64 pre-activation is inside the rounding bound of its own fp32 sum; every other
unit, and so every element of every tensor, is held to the float64 decision and the unchanged room.  The host tests
pass no decisions: the reference's fp32 forward decided every unit of the fixture case as float64 does.
"""
import json
import os
from functools import lru_cache

import numpy as np
import pytest
import torch

import oracle
import test_loss_grad_host as HG
import test_loss_host as H
from test_stream_ops_host import measured

GOLDEN = os.path.join(H.GOLDEN, 'chain_grads.npz')
VARIANTS = ('shipped', 'raft')
# the pose loss of the `scflow_model` fixtures of the gradient tests (tests/test_gpu_gru_grad.py)
RAFT_POSE_LOSS = dict(type='SequenceLoss', gamma=0.7, loss_func_cfg=dict(type='RAFTLoss', loss_weight=0.3, max_flow=400.))
FIXTURE_SEEDS = dict(input_seed=7, case_seed=5, weight_seed=0)              # refiner_loss.npz's: the first triple tried

# ROOM[variant][group]: the measure of the reference's fp32 CPU autograd against the float64 chain at the fixture's inputs,
# as test_chain_equals_the_reference_autograd printed it when the fixture was recorded.  The two fp32
# forwards differ from the float64 one in the last bits of every pose, hence by ~1e-4 pixel in the flow re-projected from it;
# the cotangents are taken at these different forwards, which is most of every entry: the motion encoder's flow branch
# and its 1 x 1 correlation layer read exactly these inputs, and under the 'raft' pose loss every sign(prediction - target)
# of a re-projected flow is a decision.
ROOM = {
    'shipped': {'pose_pred': 1.42e-06, 'heads': 1.7e-06, 'gru': 3.13e-06, 'encoder': 0.000945, 'inputs': 2.44e-06,
                'iteration': 3.37e-06},
    'raft': {'pose_pred': 3.32e-05, 'heads': 2.84e-05, 'gru': 4.45e-05, 'encoder': 0.0012, 'inputs': 4.09e-05,
             'iteration': 0.000177},
}
PARAM_GROUPS = (('decoder.pose_pred.', 'pose_pred'), ('decoder.flow_pred.', 'heads'), ('decoder.mask_pred.', 'heads'),
                ('decoder.delta_flow_encoder.', 'heads'), ('decoder.mask_encoder.', 'heads'), ('decoder.gru.', 'gru'),
                ('decoder.encoder.', 'encoder'))
INPUT_KEYS = ('initial_hidden', 'context', 'correlation')
# per-iteration lists of a chain result; the first block is what loss_and_motion_grads() returns (see `gpu_view`)
ITER_KEYS = ('hidden_states', 'motion_features', 'flow_inputs', 'delta_flow_preds', 'mask_logits', 'delta_flow_tail',
             'masks_tail', 'delta_rotation_preds', 'delta_translation_preds', 'sequence_flow_from_pred', 'sequence_masks',
             'seq_rotations', 'seq_translations', 'sequence_flow_from_pose', 'hidden_total')
DEFECTS = ('pose_to_hv_dropped', 'mask_head_dropped', 'carry_dropped', 'lists_reversed', 'gamma_reversed',
           'params_last_iteration', 'detach_pose_ignored', 'detach_flow_ignored')


def group_of(key):
    """compared key ('decoder.gru....', 'context', 'motion_features.1', ...) -> its ROOM group"""
    for prefix, group in PARAM_GROUPS:
        if key.startswith(prefix):
            return group
    if key in INPUT_KEYS:
        return 'inputs'
    assert key.split('.')[0] in ITER_KEYS, key
    return 'iteration'


def rel(got, ref):
    """max |got - ref| / max |ref| over all elements; inf when got is not finite or ref is identically zero and got is not"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if not np.isfinite(got).all():
        return float('inf')
    err, top = float(np.abs(got - ref).max()), float(np.abs(ref).max())
    return 0.0 if err == 0 else (err / top if top else float('inf'))


# ============================================================================================================ cases
def shipped_flags(**over):
    """the decoder options `chain_ref64` hands to oracle.scflow_decoder: the shipped values of scflow_model_cfg()"""
    import scflow_amd
    d = scflow_amd.scflow_model_cfg()['decoder']
    flags = {k: d[k] for k in ('detach_flow', 'detach_mask', 'detach_pose', 'detach_depth_for_xy', 'mask_flow', 'mask_corr',
                               'radius', 'num_levels')}
    flags.update(depth_transform=d.get('depth_transform', 'exp'), label_mode=0)
    flags.update(over)
    return flags


def chain_case(n=H.REFINER_N, height=256, width=256, input_seed=7, case_seed=5):
    """`refiner_loss_case` of tests/test_loss_host.py at any batch and image size (the same draws in the same order: at
    3 x 256 x 256 it IS that case)."""
    from scflow_amd.synthetic import make_inputs
    f32 = np.float32
    inp = make_inputs(n, height, width, seed=input_seed)
    rng = np.random.RandomState(case_seed)
    gt_r = np.stack([H.rand_rot(rng, 0.04) @ inp['ref_rotation'][i].numpy() for i in range(n)]).astype(f32)
    gt_t = (inp['ref_translation'].numpy() + rng.randn(n, 3) * [3, 3, 12]).astype(f32)
    gt_masks = (inp['depth'] > 0).clone()
    gt_masks[:, :height * 100 // 256, :width * 110 // 256] = False
    verts = [(rng.randn(40 + 5 * c, 3) * 35).astype(f32) for c in range(21)]
    labels = [int(x) for x in inp['label']]
    symmetry_types = {f'cls_{labels[0] + 1}': {}}
    diameter = [float(f32(90 + 7.7 * c)) for c in range(21)]
    init_add_error = torch.from_numpy(rng.uniform(5, 40, size=n).astype(f32))
    scale = rng.uniform(0.8, 1.6, size=n).astype(f32)
    return dict(inp=inp, gt_r=gt_r, gt_t=gt_t, gt_masks=gt_masks, verts=verts, labels=labels, symmetry_types=symmetry_types,
                diameter=diameter, init_add_error=init_add_error, scale=scale)


def chain_cfgs(case, variant):
    """the three loss configs of a variant: 'shipped' = configs/refine_models/scflow.py (disentangled point matching, the
    first sample's class symmetric), 'raft' = the same with the RAFTLoss pose loss of the gradient tests' `scflow_model`"""
    cfgs = H.refiner_loss_cfgs(case)
    if variant == 'raft':
        cfgs['pose_loss_cfg'] = json.loads(json.dumps(RAFT_POSE_LOSS))
    else:
        assert variant == 'shipped', variant
    return cfgs


def chain_data(case, device='cpu'):
    """`refiner_data` plus what the pose loss reads from its meshes: the class vertex sets (host arrays)"""
    return dict(H.refiner_data(case, device), verts=case['verts'])


def decoder_sd64(sd):
    """a state dict -> its 'decoder.*' entries as float64 leaves that require a gradient"""
    return {k: v.detach().cpu().double().requires_grad_() for k, v in sd.items() if k.startswith('decoder.')}


def state_dict(weight_seed=0, shapes_file='state_dict_keys.json', fc1_in=None):
    from scflow_amd.weights import fill_state_dict
    shapes = dict(json.load(open(os.path.join(H.GOLDEN, shapes_file)))['shapes'])
    if fc1_in is not None:                     # the pose head on another map size: fc1 reads 128 * (h / 8) * (w / 8) features
        shapes['decoder.pose_pred.fc_layers.0.0.weight'] = [shapes['decoder.pose_pred.fc_layers.0.0.weight'][0], fc1_in]
    return fill_state_dict(shapes, seed=weight_seed)


# ============================================================================================================ the chain
_ALIASED = ('hv_flow', 'hv_mask', 'hv_pose', 'd_flow_tail', 'mask_tail', 'flow_in')       # the cotangent of ONE use
_RECORDED = ('x', 'hv', 'd_flow', 'mask_logit', 'd_rot', 'd_trans', 'flow_pred', 'up_mask', 'rotation', 'translation',
             'flow_from_pose')
_DROPPED = dict(pose_to_hv_dropped='hv_pose', mask_head_dropped='hv_mask')


def chain_ref64(decoder_inputs, sd, data, cfgs, flags, *, iters, variant):
    """d(loss) / d(everything) of decoder + loss as one float64 graph.

    decoder_inputs: (feat_render, feat_real, h0, context), any float dtype, taken as given and converted to float64; sd:
    `decoder_sd64`'s float64 leaves; data: `chain_data` (host tensors; an entry 'gt_flow', when present, is the ground-truth
    flow to take the fp32 validity decisions from -- else it is oracle.flow_from_delta_pose_and_depth +
    filter_flow_by_mask in fp32, as `test_wiring_reproduces_the_reference_log_vars` builds it); cfgs: `chain_cfgs`; flags:
    `shipped_flags`, optionally with 'defect' (one of DEFECTS: a planted join defect, applied to THIS graph) and 'nn' (the
    neighbour indices to differentiate at, [t][n] -> array or None, instead of the float64 forward's own) and 'relu' (the
    ReLU decisions of an fp32 forward, see `conv_act` below: they count only at units whose derivative the inputs do not
    determine).

    -> dict: 'loss' (float), 'log' (wiring_ref's OrderedDict of the float64 forward's values), 'nn' ((T, N, Vmax) int32,
    -1 where a sample's class is not symmetric; None for the 'raft' variant), 'params' {name: array}, 'initial_hidden',
    'context', 'correlation' (N h w, h, w), and a list over the iterations for every key of ITER_KEYS: 'hidden_states' is
    d loss / d hv_t through iteration t's OWN heads (what the GRU backward adds the carry to), 'hidden_total' the complete
    one; 'delta_flow_preds' / 'mask_logits' are complete, 'delta_flow_tail' / 'masks_tail' the part that arrives through
    the up-sampled outputs alone (the refiner's top-level 'delta_flow_preds' / 'masks').  The nearest-neighbour index of a
    symmetric class is a constant of the differentiation, taken from the float64 forward."""
    flags = dict(flags)
    defect, nn_given, relu = flags.pop('defect', None), flags.pop('nn', None), flags.pop('relu', None)
    assert defect is None or defect in DEFECTS, defect
    if defect == 'detach_pose_ignored':
        flags['detach_pose'] = False
    if defect == 'detach_flow_ignored':
        flags['detach_flow'] = False
    D = lambda t: (torch.from_numpy(t) if isinstance(t, np.ndarray) else t).detach().cpu().double()       # noqa: E731
    fr, fl, h0, ctx = (D(t).clone().requires_grad_() for t in decoder_inputs)
    rec = {}

    def tap(name, t, v):
        if name == 'pyramid':
            rec['pyramid0'] = v[0]
        elif name == 'sd':
            rec['t'] = t
            if defect == 'params_last_iteration' and t < iters - 1:
                return {k: w.detach() for k, w in v.items()}
        elif name == 'h_in':
            if defect == 'carry_dropped' and t > 0:
                return v.detach()
        elif name in _ALIASED:
            a = v.view_as(v) if v.requires_grad else v.detach().requires_grad_()
            rec[name, t] = a
            return v.detach() if _DROPPED.get(defect) == name else a
        elif name in _RECORDED:
            rec[name, t] = v
        return v

    depth = D(data['rendered_depths'])
    n, height, width = depth.shape
    labels = data['labels'].detach().cpu().long()
    ties = []
    plain_conv_act = oracle.conv_act

    def conv_act(x, w, prefix, *, stride=1, padding=0, act='relu'):
        """`relu`: {(layer prefix, t): the fp32 evaluation's decisions (bool, the layer's output shape)}.  A ReLU unit
        whose float64 pre-activation lies within the rounding bound of an fp32 evaluation of its own sum -- (K + 2) U
        (sum |w| |x| + |b|), K the terms of the sum -- has no derivative the inputs determine: 0 and 1 are both an fp32
        evaluation's.  There, and only there, the chain differentiates at the given decision; everywhere else at its own."""
        given = None if relu is None or act != 'relu' else relu.get((prefix, rec.get('t')))
        if given is None:
            return plain_conv_act(x, w, prefix, stride=stride, padding=padding, act=act)
        pre = plain_conv_act(x, w, prefix, stride=stride, padding=padding, act=None)
        wt, b = w[prefix + '.conv.weight'], w.get(prefix + '.conv.bias')
        with torch.no_grad():
            mag = torch.nn.functional.conv2d(x.abs(), wt.abs(), None if b is None else b.abs(), stride=stride, padding=padding)
            bound = (wt[0].numel() + 2) * 2.0 ** -24 * mag
            own = pre > 0
            tied = (own != torch.as_tensor(given).reshape(own.shape)) & (pre.abs() <= bound)
            gate = torch.where(tied, ~own, own).to(pre.dtype)
        if bool(tied.any()):
            ties.append((prefix, rec.get('t'), int(tied.sum()), float((pre.detach().abs() / bound)[tied].max())))
        return pre * gate

    outs = oracle.scflow_decoder(fr, fl, h0, ctx, D(data['ref_rotations']), D(data['ref_translations']), depth,
                                 D(data['internel_k']), labels, torch.zeros((n, 2, height, width), dtype=torch.float64), sd,
                                 iters=iters, invalid_flow_num=0., tap=tap, conv=conv_act, **flags)
    F32 = lambda t: t.detach().cpu().float()                                                    # noqa: E731
    valid = F32(data['rendered_masks'])
    if 'gt_flow' in data:
        gt_flow = F32(data['gt_flow'])
    else:
        with torch.no_grad():
            gt_flow = oracle.flow_from_delta_pose_and_depth(F32(data['ref_rotations']), F32(data['ref_translations']),
                                                            F32(data['gt_rotations']), F32(data['gt_translations']),
                                                            F32(data['rendered_depths']), F32(data['internel_k']), 400.)
            gt_flow = oracle.filter_flow_by_mask(gt_flow, data['gt_masks'].cpu(), 400.)
    seqs = [outs[0], outs[1], outs[2], outs[3], [m[:, 0] for m in outs[4]]]
    lp = cfgs['pose_loss_cfg']['loss_func_cfg']
    assert (lp['type'] == 'RAFTLoss') == (variant == 'raft'), (lp['type'], variant)
    pose, nn_arr = None, None
    if variant != 'raft':
        lab = [int(x) for x in labels]
        sym = [f'cls_{c + 1}' in lp['symmetry_types'] for c in range(len(data['verts']))]
        pose = dict(verts=data['verts'], labels=lab, symmetric=sym, diameter=lp['mesh_diameter'],
                    gt_r=H.a64(data['gt_rotations']), gt_t=H.a64(data['gt_translations']), scale=H.a64(data['scale_factors']))
        nn = nn_given
        if nn is None:
            opt = dict(lp, cls=lp['type'])
            q = H.pm_ref(pose['verts'], lab, sym, pose['diameter'], [H.a64(r) for r in outs[2]], [H.a64(t) for t in outs[3]],
                         pose['gt_r'], pose['gt_t'], scale=pose['scale'], mode=H.PM_MODES[lp['type']],
                         loss_type=int(lp.get('loss_type', 'l2')[-1]), flags=H.pm_flags(opt), sdf=lp.get('scale_depth_factor', 1.),
                         reduction=lp.get('reduction', 'mean'), weight=lp.get('loss_weight', 1.))
            nn = q['nn']
        vmax = max(len(v) for v in data['verts'])
        nn_arr = np.full((iters, n, vmax), -1, dtype=np.int32)
        for t in range(iters):
            for i in range(n):
                if nn[t][i] is not None:
                    k = len(data['verts'][lab[i]])
                    nn_arr[t, i, :k] = np.asarray(nn[t][i])[:k]
        nn_list = [[None if nn[t][i] is None else np.asarray(nn[t][i])[:len(data['verts'][lab[i]])] for i in range(n)]
                   for t in range(iters)]
        pose['nn'], pose['nn_idx'] = nn_list, nn_list
    with torch.no_grad():
        log = H.wiring_ref('scflow', [[s.detach() for s in q_] for q_ in seqs], gt_flow, valid, cfgs, pose=pose)
    wired = seqs
    if defect == 'gamma_reversed':              # gamma ** i on iteration i: the weights of the reversed sequences
        wired = [s[::-1] for s in seqs]
        if pose is not None:
            pose = dict(pose, nn=pose['nn'][::-1])
    total = HG.torch_wiring_total('scflow', wired, gt_flow, valid, cfgs, pose=pose)
    if defect == 'lists_reversed':
        # every list of loss cotangents handed on in reversed iteration order: iteration t's outputs take the cotangents
        # the loss has for iteration T - 1 - t
        names = ['flow_pred', 'up_mask'] + (['flow_from_pose'] if variant == 'raft' else ['rotation', 'translation'])
        outs_ = [rec[name, t] for name in names for t in range(iters)]
        cots = torch.autograd.grad(total, outs_, retain_graph=True)
        total = 0.
        for j, name in enumerate(names):
            for t in range(iters):
                total = total + (cots[j * iters + (iters - 1 - t)] * rec[name, t]).sum()
    names = sorted(sd)
    per_iter = [(k, t) for k in _ALIASED + _RECORDED for t in range(iters)]
    targets = [sd[k] for k in names] + [h0, ctx, rec['pyramid0']] + [rec[k] for k in per_iter]
    got = torch.autograd.grad(total, targets, allow_unused=True)
    got = [torch.zeros_like(t) if g is None else g for g, t in zip(got, targets)]
    A = lambda g: g.detach().numpy()                                                            # noqa: E731
    res = dict(loss=float(log['loss'].v), log=log, nn=nn_arr, params={k: A(g) for k, g in zip(names, got)})
    res['ties'] = ties                         # (layer, t, units differentiated at the given decision, worst |pre| / bound)
    res['forward'] = {k: [A(rec[k, t]) for t in range(iters)] for k in _RECORDED}       # the float64 forward's values
    res['initial_hidden'], res['context'] = A(got[len(names)]), A(got[len(names) + 1])
    h, w = rec['pyramid0'].shape[-2:]
    res['correlation'] = A(got[len(names) + 2]).reshape(-1, h, w)
    it = {k: A(g) for k, g in zip(per_iter, got[len(names) + 3:])}
    seq = lambda name: [it[name, t] for t in range(iters)]                                      # noqa: E731
    res.update(hidden_states=[it['hv_flow', t] + it['hv_mask', t] + it['hv_pose', t] for t in range(iters)],
               hidden_total=seq('hv'), motion_features=seq('x'), flow_inputs=seq('flow_in'), delta_flow_preds=seq('d_flow'),
               mask_logits=seq('mask_logit'), delta_flow_tail=seq('d_flow_tail'), masks_tail=seq('mask_tail'),
               delta_rotation_preds=seq('d_rot'), delta_translation_preds=seq('d_trans'),
               sequence_flow_from_pred=seq('flow_pred'), sequence_masks=seq('up_mask'), seq_rotations=seq('rotation'),
               seq_translations=seq('translation'), sequence_flow_from_pose=seq('flow_from_pose'))
    return res


def flat(res):
    """a chain result (or `gpu_view` of the refiner's grads) -> {compared key: array}: parameter names, INPUT_KEYS and
    '<ITER_KEY>.<t>'"""
    out = dict(res['params'])
    out.update((k, res[k]) for k in INPUT_KEYS)
    for k in ITER_KEYS:
        if k in res:
            out.update((f'{k}.{t}', v) for t, v in enumerate(res[k]))
    return out


# ============================================================================================================ fixture
GOLDEN_ROWS = slice(37, None, 768)             # every 768th query map of the volume cotangent, from query 37
GOLDEN_ITER_KEYS = ('motion_features', 'hidden_total', 'delta_flow_preds', 'mask_logits', 'delta_rotation_preds',
                    'delta_translation_preds')


def golden_pick(key, v):
    """the part of a full gradient chain_grads.npz stores"""
    if key == 'correlation':
        return v[GOLDEN_ROWS]
    if key in ('initial_hidden', 'context'):
        return v[:, [5, 77], ::4]
    name = key.split('.')[0]
    if name == 'motion_features':
        return v[:, [3, 127], ::8]
    if name == 'hidden_total':
        return v[:, [9], ::4]
    if name == 'delta_flow_preds':
        return v[:, :, ::8]
    if name == 'mask_logits':
        return v[:, :, ::4]
    if name in ITER_KEYS:
        return v
    if v.ndim == 1:
        return v[::4] if v.size > 256 else v
    if v.ndim == 2 and v.size > 2048:
        if 'fc_layers' in key:                 # rows spread over the units: a dead ReLU unit's row is all zero
            return v[::v.shape[0] // 4, ::8]
        return v[:, ::32]                       # rotation_pred / translation_pred: only one class's rows are not zero
    if v.ndim == 4 and v.size > 256:            # of a large weight the first and the last output channel ...
        v = v[[0, v.shape[0] - 1]]
        while v.size > 256 and v.shape[1] > 1:  # ... and of those every 2nd, 4th, ... input channel
            v = v[:, ::2]
    return v


def golden_keys(res):
    keep = set(GOLDEN_ITER_KEYS)
    return [k for k in flat(res) if k.split('.')[0] not in ITER_KEYS or k.split('.')[0] in keep]


@lru_cache(maxsize=None)
def fixture_case(variant, defect=None):
    """the float64 chain at the fixture's own inputs: the seeded case and weights, the decoder's four inputs from the fp32
    CPU encoders (oracle.extract_feat), shipped flags, T = 3 -> (case, chain result).  Results are shared: do not write."""
    case = H.refiner_loss_case(FIXTURE_SEEDS['input_seed'], FIXTURE_SEEDS['case_seed'])
    return case, _fixture_chain(variant, defect)


@lru_cache(maxsize=None)
def _fixture_inputs():
    case = H.refiner_loss_case(FIXTURE_SEEDS['input_seed'], FIXTURE_SEEDS['case_seed'])
    sd = state_dict(FIXTURE_SEEDS['weight_seed'])
    with torch.no_grad():
        feats = oracle.extract_feat(case['inp']['render_images'], case['inp']['real_images'], sd)
    return case, sd, feats


def fixture_decoder_inputs():
    """the decoder's four inputs at the fixture case: the fp32 CPU encoders' outputs (what `fixture_case` starts from and,
    up to the host's fp32 sums, what the reference's decoder was handed when chain_grads.npz was recorded)"""
    return _fixture_inputs()[2]


def _fixture_chain(variant, defect):
    case, sd, feats = _fixture_inputs()
    flags = shipped_flags() if defect is None else shipped_flags(defect=defect)
    return chain_ref64(feats, decoder_sd64(sd), chain_data(case), chain_cfgs(case, variant), flags, iters=H.REFINER_ITERS,
                       variant=variant)


# ============================================================================================================ the tests
def test_oracle_flags_change_no_forward_bit():
    """the detach flags and an identity tap are autograd only: a small decoder run gives the same bits under every setting"""
    case = chain_case(2, 96, 160, input_seed=3, case_seed=4)
    sd = state_dict(0, fc1_in=768)
    inp = case['inp']
    with torch.no_grad():
        feats = oracle.extract_feat(inp['render_images'], inp['real_images'], sd)
        run = lambda **kw: oracle.scflow_decoder(*feats, inp['ref_rotation'], inp['ref_translation'], inp['depth'],      # noqa: E731
                                                 inp['internel_k'], inp['label'], torch.zeros((2, 2, 96, 160)), sd, iters=2, **kw)
        base = run()
        for kw in (dict(detach_flow=False, detach_mask=False, detach_pose=False, detach_depth_for_xy=False),
                   dict(tap=lambda name, t, v: v)):
            for a, b in zip(base, run(**kw)):
                assert all(torch.equal(x, y) for x, y in zip(a, b)), kw
    assert all(v.dtype == torch.float32 for seq in base for v in seq)


def test_chain_case_is_the_refiner_loss_case():
    """`chain_case` restates `refiner_loss_case` draw for draw: at 3 x 256 x 256 the two are the same case"""
    a, b = chain_case(), H.refiner_loss_case()
    assert sorted(a) == sorted(b) and a['labels'] == b['labels'] and a['symmetry_types'] == b['symmetry_types']
    assert a['diameter'] == b['diameter'] and all(torch.equal(a['inp'][k], b['inp'][k]) for k in b['inp'])
    assert all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in ('gt_r', 'gt_t', 'gt_masks', 'init_add_error', 'scale'))
    assert all(np.array_equal(x, y) for x, y in zip(a['verts'], b['verts']))


def test_relu_decisions_count_only_inside_the_rounding_bound():
    """`flags['relu']`: handed decisions that contradict float64 at EVERY active unit of a layer (all off), the chain
    honours the contradiction at the units whose pre-activation is inside the fp32 rounding bound of their own sum and
    at no other: the result has the bits of a chain handed float64's own decisions flipped at exactly those units, it is
    not the plain chain, and the units are the ones an independent evaluation of the bound names."""
    import torch.nn.functional as F
    case = chain_case(2, 96, 160, input_seed=3, case_seed=4)
    sd = state_dict(0, fc1_in=768)
    with torch.no_grad():
        feats = oracle.extract_feat(case['inp']['render_images'], case['inp']['real_images'], sd)
    layer, t = 'decoder.flow_pred.layers.0', 1
    run = lambda **kw: chain_ref64(feats, decoder_sd64(sd), chain_data(case), chain_cfgs(case, 'shipped'),      # noqa: E731
                                   shipped_flags(**kw), iters=2, variant='shipped')
    plain = run()
    assert plain['ties'] == []
    w, b = sd[layer + '.conv.weight'].double(), sd[layer + '.conv.bias'].double()
    hv = torch.from_numpy(plain['forward']['hv'][t])
    pre = F.conv2d(hv, w, b, padding=1)
    bound = (w[0].numel() + 2) * 2.0 ** -24 * F.conv2d(hv.abs(), w.abs(), b.abs(), padding=1)
    own = pre > 0
    inside = own & (pre.abs() <= bound)
    count = int(inside.sum())
    measured(f'{layer}, iteration {t}: active units inside the rounding bound, of {own.numel()} ({int(own.sum())} active)', count)
    assert 1 <= count < 1e-3 * own.numel() and float(bound.max()) < 1e-2 * float(pre.abs().max())
    all_off = run(relu={(layer, t): torch.zeros_like(own)})
    assert [(k[0], k[1], k[2]) for k in all_off['ties']] == [(layer, t, count)] and all_off['ties'][0][3] <= 1.0
    exact = run(relu={(layer, t): own & ~inside})                   # float64's own decisions, flipped at the inside units only
    a, b_, p_ = flat(all_off), flat(exact), flat(plain)
    assert all(np.array_equal(a[k], b_[k]) for k in a), 'a contradiction outside the bound was honoured'
    moved = rel(a[f'hidden_states.{t}'], p_[f'hidden_states.{t}'])
    measured(f'{count} units decided otherwise move hidden_states.{t} by, of its largest entry', moved)
    assert moved > 10 * ROOM['shipped']['iteration']
    # outside the bound a handed decision changes nothing: one active unit far from zero, handed as off
    far = own & (pre == pre.max())
    assert run(relu={(layer, t): own & ~far})['ties'] == []


def test_chain_value_is_the_refiner_loss(golden_dir):
    """the float64 chain's loss values reproduce the reference's log_vars (refiner_loss.npz) within the room
    test_wiring_reproduces_the_reference_log_vars uses: the oracle's network tolerance propagated to each value plus the
    restatement's own bound"""
    g = np.load(os.path.join(golden_dir, 'refiner_loss.npz'))
    assert {k: int(g[k]) for k in FIXTURE_SEEDS} == FIXTURE_SEEDS and int(g['iters']) == H.REFINER_ITERS
    case, res = fixture_case('shipped')
    cfgs = chain_cfgs(case, 'shipped')
    log = res['log']
    want_keys = [str(k) for k in g['keys']]
    assert ['init_add_mean', 'init_add_std'] + list(log.keys()) == want_keys
    worst = 0.0
    for k, want in zip(want_keys[2:], g['values'][2:]):
        ev = log[k]
        room = float(ev.e) + H.propagated_tolerance(k, cfgs, H.ORACLE_TOL, case)
        r = abs(float(want) - float(ev.v)) / room
        worst = max(worst, r)
        assert r <= 1.0, (k, float(want), float(ev.v), room)
    measured('reference log_vars vs the float64 chain: worst error / propagated tolerance', worst)
    assert res['loss'] == float(log['loss'].v)


@pytest.mark.parametrize('variant', VARIANTS)
def test_chain_equals_the_reference_autograd(variant):
    """the reference's own fp32 CPU backward (chain_grads.npz) against the float64 chain at the fixture's inputs: this pins
    the oracle's detach flags and the chain's loss wiring to the reference's real graph, and it is where ROOM is measured"""
    z = np.load(GOLDEN)
    assert {k: int(z[k]) for k in FIXTURE_SEEDS} == FIXTURE_SEEDS and int(z['iters']) == H.REFINER_ITERS
    assert os.path.getsize(GOLDEN) < 256 * 1024
    assert all(z[k].dtype in (np.float32, np.int32, np.int64) or z[k].dtype.kind == 'U' for k in z.files)
    case, res = fixture_case(variant)
    got = flat(res)
    keys = golden_keys(res)
    assert sorted(f'{variant}.{k}' for k in keys) == sorted(k for k in z.files if k.startswith(variant + '.') and
                                                            k not in (f'{variant}.loss', f'{variant}.nn'))
    assert abs(float(z[f'{variant}.loss']) - res['loss']) <= 1e-4 * abs(res['loss'])
    if variant == 'shipped':                    # the neighbours the reference differentiated at are the float64 forward's
        assert np.array_equal(z['shipped.nn'], res['nn']) and (res['nn'][:, 0] >= 0).any()
    worst = {}
    for k in keys:
        v = rel(z[f'{variant}.{k}'], golden_pick(k, got[k]))
        worst[group_of(k)] = max(worst.get(group_of(k), 0.0), v)
    for group, v in sorted(worst.items()):
        measured(f'reference fp32 autograd vs float64 chain, {variant}, {group}: max error / largest entry', v)
        assert v <= 1.5 * ROOM[variant][group], (group, v)
    assert sorted(worst) == sorted(ROOM[variant])


@pytest.mark.parametrize('defect', DEFECTS)
def test_planted_join_defects_leave_the_room(defect):
    """every join defect, planted into the float64 chain, moves at least one compared tensor 10 rooms away from the
    undamaged chain: the GPU tests' 2 x ROOM would see it five times over.  A condition on the inputs (FIXTURE_SEEDS)."""
    for variant in VARIANTS:
        good, bad = flat(fixture_case(variant)[1]), flat(fixture_case(variant, defect)[1])
        ratios = {k: rel(bad[k], good[k]) / ROOM[variant][group_of(k)] for k in good if np.abs(good[k]).max() > 0}
        k = max(ratios, key=ratios.get)
        measured(f'planted {defect}, {variant}: largest deviation / room ({k})', ratios[k])
        assert ratios[k] >= 10.0, (variant, k, ratios[k])


@pytest.mark.parametrize('variant', VARIANTS)
def test_no_dead_path(variant):
    """no parameter gradient and no input cotangent of the float64 chain is identically zero, and no compared tensor's
    largest entry is below 1e-30: the relative measure is never empty"""
    _, res = fixture_case(variant)
    got = flat(res)
    silent = {'shipped': ('sequence_flow_from_pose',), 'raft': ()}[variant]     # flow_from_pose feeds no shipped loss term
    for k, v in got.items():
        if k.split('.')[0] in silent:
            assert not v.any(), k
            continue
        assert np.isfinite(v).all() and np.abs(v).max() >= 1e-30, k
    assert set(res['params']) == {k for k in state_dict(0) if k.startswith('decoder.')}
