"""GPU: what every keep level of SCFlowDecoder leaves in `kept`, that a caller's own level survives the refiner's entries,
and that `SCFlowDecoder.backward()` is the stages in order: called directly it returns the bits of
`SCFlowRefiner.loss_and_motion_grads()`, and at every shallower depth the bits of that result's entries.  Bit equality
only; the stages' numerics are held by the stage tests and tests/test_gpu_chain_grad.py."""
import pytest

from scflow_amd.modules import KEEP_LEVELS
import test_loss_host as HL
from test_gpu_gru_grad import scflow_model  # noqa: F401  (3 samples of 256 x 256, 3 iterations, 32 x 32 maps; module-scoped)
from test_stream_ops_host import same_bits  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# written out, not read from the code's table: the keys a forward at each level leaves in `kept`
LEVEL_KEYS = {
    'pose_tail': {'tail_inputs'},
    'pose_head': {'tail_inputs', 'hv', 'dm', 'y0', 'y1', 'y2'},
    'decoder_heads': {'tail_inputs', 'hv', 'dm', 'y0', 'y1', 'y2', 'd_flow', 'mask'},
    'gru': {'tail_inputs', 'hv', 'dm', 'y0', 'y1', 'y2', 'd_flow', 'mask', 'h0', 'c', 'x'},
    'motion': {'tail_inputs', 'hv', 'dm', 'y0', 'y1', 'y2', 'd_flow', 'mask', 'h0', 'c', 'x', 'flow_lr', 'pyramid', 'tiled'},
}
HEAD_KEYS = {'delta_flow_preds', 'masks', 'delta_rotation_preds', 'delta_translation_preds'}
# the keys of the returned gradients at each depth of the chain
DEPTH_KEYS = {
    'head': HEAD_KEYS,
    'pose_tail': HEAD_KEYS | {'pose_tail_inputs', 'params'},
    'pose_head': HEAD_KEYS | {'pose_tail_inputs', 'params', 'pose_head_inputs'},
    'decoder_heads': HEAD_KEYS | {'pose_tail_inputs', 'params', 'pose_head_inputs', 'decoder_heads'},
    'gru': HEAD_KEYS | {'pose_tail_inputs', 'params', 'pose_head_inputs', 'decoder_heads', 'gru'},
    'motion': HEAD_KEYS | {'pose_tail_inputs', 'params', 'pose_head_inputs', 'decoder_heads', 'gru', 'motion'},
}


def _get_pose(m, data):
    return m.get_pose(data['rendered_images'], data['real_images'], data['ref_rotations'], data['ref_translations'],
                      data['rendered_depths'], data['internel_k'], data['labels'])


def _same(a, b):
    if isinstance(a, dict):
        return sorted(a) == sorted(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return same_bits(a, b)


@pytest.mark.parametrize('level', KEEP_LEVELS[1:])
def test_a_level_keeps_exactly_its_keys(scflow_model, level):  # noqa: F811
    assert list(LEVEL_KEYS) == list(KEEP_LEVELS[1:])
    m, case = scflow_model
    data = HL.refiner_data(case, DEV)
    dec = m.decoder
    assert dec.keep == 'none'
    dec.kept = dict(stale=None)                     # a forward above 'none' REPLACES the store
    try:
        dec.keep = level
        _get_pose(m, data)
    finally:
        dec.keep = 'none'
    assert set(dec.kept) == LEVEL_KEYS[level]
    before = KEEP_LEVELS[KEEP_LEVELS.index(level) - 1]
    assert set(dec.kept) >= LEVEL_KEYS.get(before, set())
    assert len(dec.kept['tail_inputs']) == dec.iters
    assert all(v.shape[0] == dec.iters for k, v in dec.kept.items() if k in ('hv', 'dm', 'd_flow', 'mask', 'x', 'flow_lr'))
    assert all(dec.kept[k].shape[1] == dec.iters for k in ('y0', 'y1', 'y2') if k in dec.kept)
    dec.kept = {}


def test_a_level_the_caller_set_survives_the_refiner(scflow_model):  # noqa: F811
    m, case = scflow_model
    data = HL.refiner_data(case, DEV)
    dec = m.decoder
    try:
        dec.keep = 'motion'
        m.loss_and_pose_tail_grads(None, data=data)
        assert dec.keep == 'motion' and set(dec.kept) == LEVEL_KEYS['motion']
        dec.keep = 'none'
        m.loss_and_pose_tail_grads(None, data=data)
        assert dec.keep == 'none' and set(dec.kept) == LEVEL_KEYS['pose_tail']
    finally:
        dec.keep, dec.kept = 'none', {}


def test_the_chain_is_the_stages(scflow_model):  # noqa: F811
    m, case = scflow_model
    data = HL.refiner_data(case, DEV)
    dec = m.decoder
    want = m.loss_and_motion_grads(None, data=data)[5]
    assert set(want) == DEPTH_KEYS['motion']
    # the outputs and the loss gradients of a loss_and_grads() call under keeping('motion'): get_pose's tuple is caught on its way
    caught, get_pose = [], m.get_pose
    m.get_pose = lambda *a, **k: caught.append(get_pose(*a, **k)) or caught[-1]
    try:
        with dec.keeping('motion'):
            base = m.loss_and_grads(None, data=data)
    finally:
        del m.get_pose
    assert dec.keep == 'none' and len(caught) == 1 and set(dec.kept) == LEVEL_KEYS['motion']
    args = (data['labels'], data['ref_rotations'], data['ref_translations'], data['rendered_depths'].contiguous(),
            data['internel_k'].contiguous())
    for depth in reversed(list(DEPTH_KEYS)):
        got = dec.backward(depth, caught[0], dict(base[5]), *args)
        assert set(got) == DEPTH_KEYS[depth], depth
        for key, v in got.items():
            if key == 'params':         # relative to the decoder; the refiner prefixes them once
                assert depth != 'motion' or len(v) == len(want['params'])
                assert all(same_bits(g, want['params']['decoder.' + k]) for k, g in v.items()), (depth, key)
            else:
                assert _same(v, want[key]), (depth, key)
    with pytest.raises(ValueError):
        dec.backward('outputs', caught[0], dict(base[5]), *args)
    dec.kept = {}
