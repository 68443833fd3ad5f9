"""Host: the one keep level of SCFlowDecoder (`keep`, `keeping()`) and the refusals of `check_backward()`, on a CPU-built
decoder.  Nothing here launches: what the levels keep and what the chain returns is held on the GPU by
tests/test_gpu_keep_levels.py."""
import pytest
import torch

import scflow_amd
from scflow_amd.modules import KEEP_LEVELS
from scflow_amd.refiner import _GRAD_DEPTHS


@pytest.fixture(scope='module')
def dec():
    return scflow_amd.build_refiner(scflow_amd.scflow_model_cfg(iters=2)).decoder


def test_the_keep_levels_are_the_grad_depths():
    assert KEEP_LEVELS[0] == 'none' and KEEP_LEVELS[1:] == _GRAD_DEPTHS[3:]
    assert _GRAD_DEPTHS[:3] == ('none', 'outputs', 'head') and _GRAD_DEPTHS[-1] == 'motion'


def test_keeping_raises_the_level_and_never_lowers_it(dec):
    assert dec.keep == 'none' and dec.kept == {}
    for outer in KEEP_LEVELS:
        dec.keep = outer
        for inner in KEEP_LEVELS:
            with dec.keeping(inner):
                assert dec.keep == max(outer, inner, key=KEEP_LEVELS.index), (outer, inner)
            assert dec.keep == outer, (outer, inner)
    dec.keep = 'none'
    with dec.keeping('pose_head'):
        with dec.keeping('pose_tail'):
            assert dec.keep == 'pose_head'
        with dec.keeping('motion'):
            assert dec.keep == 'motion'
        assert dec.keep == 'pose_head'
    assert dec.keep == 'none'


@pytest.mark.parametrize('outer', ['none', 'decoder_heads'])
def test_keeping_restores_the_level_after_an_exception(dec, outer):
    dec.keep = outer
    try:
        with pytest.raises(RuntimeError, match='in the body'):
            with dec.keeping('gru'):
                assert dec.keep == 'gru'
                raise RuntimeError('in the body')
        assert dec.keep == outer
        with pytest.raises(ValueError):
            with dec.keeping('everything'):
                pass
        assert dec.keep == outer
    finally:
        dec.keep = 'none'


def test_an_unknown_keep_name_is_refused_before_anything_touches_a_device(dec):
    """CPU tensors: a forward that got as far as its first launch would raise the library's device error instead"""
    n, H, W = 1, 64, 64
    h, w = H // 8, W // 8
    args = (torch.zeros(n, 256, h, w), torch.zeros(n, 256, h, w), torch.zeros(n, 128, h, w), torch.zeros(n, 128, h, w),
            torch.eye(3).repeat(n, 1, 1), torch.ones(n, 3), torch.ones(n, H, W), torch.eye(3).repeat(n, 1, 1))
    kw = dict(label=torch.zeros(n, dtype=torch.int64), init_flow=torch.zeros(n, 2, H, W), invalid_flow_num=0.)
    dec.keep = 'pose'
    try:
        with pytest.raises(ValueError, match='KEEP_LEVELS') as err:
            dec(*args, **kw)
        assert all(name in str(err.value) for name in KEEP_LEVELS) and "'pose'" in str(err.value)
        assert dec.kept == {}
    finally:
        dec.keep = 'none'
    from scflow_amd._lib import ScflowHipError
    with pytest.raises(ScflowHipError):           # at a valid level the same call reaches the library, which refuses CPU tensors
        dec(*args, **kw)


# the three configurations tests/test_gpu_motion_grad.py::test_loss_and_motion_grads lists: (flags, what the refusal names)
REFUSED = [(dict(detach_flow=False), 'detach_flow'),
           (dict(detach_flow=True, detach_mask=False, mask_flow=True), 'detach_mask'),
           (dict(detach_flow=True, detach_mask=False, mask_flow=False, mask_corr=True), 'detach_mask')]


@pytest.mark.parametrize('flags,names', REFUSED, ids=[n + str(i) for i, (_, n) in enumerate(REFUSED)])
def test_check_backward_refuses_at_motion_only(dec, flags, names):
    shipped = {k: getattr(dec, k) for k in ('detach_flow', 'detach_mask', 'mask_flow', 'mask_corr')}
    assert shipped == dict(detach_flow=True, detach_mask=True, mask_flow=False, mask_corr=False)
    for depth in _GRAD_DEPTHS:
        dec.check_backward(depth)                  # the shipped configuration: nothing is refused at any depth
    try:
        for k, v in flags.items():
            setattr(dec, k, v)
        with pytest.raises(NotImplementedError, match=names) as err:
            dec.check_backward('motion')
        assert 'loss_and_motion_grads' in str(err.value)
        for depth in _GRAD_DEPTHS[:-1]:
            dec.check_backward(depth)              # 'gru' and every depth before it refuse nothing, as before
    finally:
        for k, v in shipped.items():
            setattr(dec, k, v)
    with pytest.raises(ValueError):
        dec.check_backward('everything')
