"""GPU: the pose head's fully connected tail -- scf_fc_splitk (fc.hip) and scf_linear / scf_linear_pair (norm.hip) --
against the float64 restatements and derived bounds of tests/test_fc_host.py: every tile layout with and without
zero-filled columns, partial tiles in N and O, every count of parts around the rounds of four, the unrolled and the
generic folded GroupNorm, two heads in one launch, both paths and both tails of linear_kernel, and the regimes where a
fixed tolerance says nothing (offset operands, constant groups, cancelling parts and k ranges, operands scaled by
2**+-60).  The case lists and the comments on which branch each case takes live next to the restatements.

Every comparison is `error <= bound` over ALL elements (ratio <= 1) or bit equality; there is no absolute tolerance.
Every launch is made twice and must give the same bits, and the last row of every batch must equal the N = 1 launch of
that sample bit for bit.

The ReLU of the tail and NaN.  fc_splitk's operand load and folded GroupNorm use fmaxf(v, 0), scf_apply_act uses
v > 0 ? v : 0: both return 0 for NaN, where torch.relu returns NaN.  A NaN (or -inf) partial sum under x_relu is
therefore 0 in the consumer's operand and the consumer's outputs are finite; a finished ReLU output of a NaN
pre-activation is 0.  The tests below assert what the kernels do (test_relu_*), the fused and the unfused head agree
on it, and DESIGN.md section 4.6 describes it.  Without a ReLU in between NaN and inf propagate as IEEE arithmetic says:
to exactly the rows and columns they belong to.

The measured error-to-bound ratios are recorded in DESIGN.md section 4.6.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from scflow_amd import _lib, ops
from scflow_amd._lib import ScflowHipError
from test_fc_host import (ACT_NONE, ACT_RELU, ACT_TANH, ACTS, FC_FINISHED, FC_GN, FC_GN_REGIMES,  # noqa: E402
                          FC_HEAD_GEOMETRY, FC_PARTIAL, FC_PARTS, FC_PARTS_K, FC_TWO_HEADS, KERNEL_RELU_OF_NAN,
                          LINEAR_PAIR_KN, LINEAR_PAIRS, LINEAR_REGIMES, LINEAR_SINGLE, SCALES, Case, fc_case, fc_depth,
                          fc_fp32, fc_gn_ref, fc_operand, fc_ref, fc_shape, gemm_ref, linear_case, linear_ref,
                          linear_ref_core, linear_shape, nonfinite_case, nonfinite_pattern, parts_ref)
from test_stream_ops_host import (IN_EPS, f64, group_norm_relu_ref, measured, same_bits, worst_ratio)  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = -7777.25
GUARD = 64                          # floats on either side of a guarded output: a multiple of 4, so alignment is kept
EINVAL, EUNSUPPORTED = -1, -2       # include/scflow_hip.h


def D(t):
    return None if t is None else t.to(DEV)


def guarded(shape):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    return buf, buf[GUARD:GUARD + n].view(shape)


def guard_untouched(buf, shape):
    n = int(np.prod(shape))
    want = torch.full_like(buf, SENTINEL)
    return same_bits(buf[:GUARD], want[:GUARD]) and same_bits(buf[GUARD + n:], want[GUARD + n:])


# ============================================================================================================ running
def fc_launch(c):
    gn = None if c.gn is None else (c.k // c.gn[0], c.gn[1], D(c.gamma), D(c.beta), IN_EPS)
    x = D(c.x) if c.parts > 1 else D(c.x[0])                        # one part: the (N, K) form of the entry point
    out = ops.fc_splitk(x, D(c.w), D(c.bias), x_bias=D(c.x_bias), x_relu=c.x_relu, gn=gn, weight2=D(c.w2),
                        bias2=D(c.bias2), act=c.act, slices=c.slices)
    return (torch.cat(out, 1) if isinstance(out, tuple) else out).cpu()


def rows_of(c, r):
    """the case of sample r alone"""
    return Case(c, n=1, x=c.x[:, r:r + 1].contiguous())


def fc_run(c):
    """the launch, made twice (same bits), and -- for a batch -- its last row as a launch of its own (same bits)"""
    got = fc_launch(c)
    assert same_bits(got, fc_launch(c)), 'two runs differ'
    if c.n > 1:
        assert same_bits(got[..., c.n - 1:c.n, :], fc_launch(rows_of(c, c.n - 1))), 'a row depends on its batch'
    return got


def fc_check(regime, shape):
    c = fc_case(regime, shape)
    return worst_ratio(fc_run(c), *fc_ref(c))


def linear_launch(c):
    if c.w2 is None:
        return ops.linear(D(c.x), D(c.w), D(c.bias), c.act).cpu()
    return torch.cat(ops.linear_pair(D(c.x), D(c.w), D(c.bias), D(c.w2), D(c.bias2), c.act), 1).cpu()


def linear_run(c):
    got = linear_launch(c)
    assert same_bits(got, linear_launch(c)), 'two runs differ'
    if c.n > 1:
        assert same_bits(got[c.n - 1:], linear_launch(Case(c, n=1, x=c.x[c.n - 1:].contiguous()))), 'a row depends on its batch'
    return got


# ================================================================================================ 2a: finished outputs
@pytest.mark.parametrize('n, o, k, act, bias', FC_FINISHED)
def test_fc_finished_tiles_layouts_activations(n, o, k, act, bias):
    worst = fc_check('nominal', fc_shape(n, k, o, act=act, bias=bias))
    measured(f'fc_splitk finished N {n} O {o} K {k} act {act} bias {bias}, error / bound', worst)
    assert worst <= 1.0


@pytest.mark.parametrize('regime', ['offset', 'cancelling_k', 'scaled_up', 'scaled_down'])
def test_fc_finished_regimes(regime):
    worst = max(fc_check(regime, fc_shape(n, k, o, act=act, bias=bias)) for n, o, k, act, bias in FC_FINISHED[::5])
    measured(f'fc_splitk finished {regime}, error / bound', worst)
    assert worst <= 1.0


# ============================================================================= 2b: partial outputs and their consumption
@pytest.mark.parametrize('slices, ks', FC_PARTIAL)
def test_fc_partial_outputs_slice_by_slice_and_consumed(slices, ks):
    """(slices, 33, 40) partial sums, each slice against its own reference and bound; then the tensor the kernel wrote
    goes through a second launch's load (in-order sum + x_bias + ReLU): the reference of that launch starts from the
    partial sums as they are, so it is exact about the order."""
    worst = 0.0
    for regime in ('nominal', 'cancelling_k'):
        c = fc_case(regime, fc_shape(33, slices * ks, 40, slices=slices))
        got = fc_run(c)
        assert got.shape == (slices, 33, 40)
        worst = max(worst, worst_ratio(got, *fc_ref(c)))
        nxt = fc_case('nominal', fc_shape(33, 40, 33, parts=slices, x_bias=True, x_relu=True, act=ACT_RELU), seed=slices)
        nxt = Case(nxt, x=got.contiguous())
        worst = max(worst, worst_ratio(fc_run(nxt), *fc_ref(nxt)))
    measured(f'fc_splitk partial slices {slices} Ks {ks} + consumer, error / bound', worst)
    assert worst <= 1.0


@pytest.mark.parametrize('parts', FC_PARTS)
def test_fc_parts_in_order(parts):
    """(parts, 33, 40) inputs built directly.  `cancelling_parts`: part 0 = -1e3 part 1 + small, so the in-order sum is
    the only right answer: the result is inside the bound of the in-order reference, and the emulation that adds the
    parts last to first is not (for 2 parts the two orders are the same sum)."""
    shape = fc_shape(33, FC_PARTS_K, 33, parts=parts, x_bias=True, x_relu=True, act=ACT_RELU)
    worst = fc_check('nominal', shape)
    c = fc_case('cancelling_parts', shape)
    ref, bound = fc_ref(c)
    got = fc_run(c)
    worst = max(worst, worst_ratio(got, ref, bound))
    measured(f'fc_splitk x_parts {parts}, error / bound', worst)
    assert worst <= 1.0
    if parts > 2:
        rev = fc_fp32(c, 'slices_reversed')
        assert worst_ratio(rev, ref, bound) > 1.0
        assert worst_ratio(got, f64(rev), bound) > 1.0, 'the result fits the reversed sum'


# ================================================================================================ 2c: folded GroupNorm
@pytest.mark.parametrize('gs, hw, slices, k', FC_GN + list(FC_HEAD_GEOMETRY.values()), ids=lambda v: str(v))
def test_fc_group_norm_folded(gs, hw, slices, k):
    worst = {}
    for regime in FC_GN_REGIMES:
        worst[regime] = fc_check(regime, fc_shape(33, k, 33, slices=slices, gn=(gs, hw)))
    measured(f'fc_splitk GroupNorm group {gs} hw {hw} slices {slices} K {k}, error / bound', max(worst.values()))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize('gs, hw, slices, k', [(64, 16, 8, 2048), (8, 3, 8, 64), (16, 4, 2, 96)])
def test_fc_group_norm_of_four_parts(gs, hw, slices, k):
    """the K-sliced convolution feeding fc1: four partial tensors added before the statistics"""
    worst = fc_check('nominal', fc_shape(33, k, 33, slices=slices, parts=4, gn=(gs, hw)))
    measured(f'fc_splitk GroupNorm of 4 parts, group {gs} hw {hw}, error / bound', worst)
    assert worst <= 1.0


def _head(feat_size, seed=5):
    import scflow_amd
    from scflow_amd.registry import HEAD, build_from_cfg
    cfg = dict(scflow_amd.scflow_model_cfg()['decoder']['pose_head_cfg'], feat_size=feat_size)
    head = build_from_cfg(cfg, HEAD)
    g = torch.Generator().manual_seed(seed)
    for prm in head.parameters():
        prm.data.copy_(torch.randn(prm.shape, generator=g) * (0.05 if prm.dim() > 1 else 0.1))
    with torch.no_grad():
        head.conv_layers[2].gn.weight.add_(1.0)
    return head.to(DEV)


def _last_conv(head, x):
    """the (parts, N, C h w) output of the head's last convolution, as features() computes it"""
    y = head.conv_layers[1](head.conv_layers[0](x))
    last = head.conv_layers[2]
    ks = ops.conv_kslices_for(last.packed, y)
    y = ops.conv2d(last.packed, y, kslices=ks)
    hw = y.shape[-2] * y.shape[-1]
    return y.reshape(ks if ks > 1 else 1, x.shape[0], -1).cpu(), hw


def _head_ref(head, parts, hw, fused):
    """float64 GroupNorm -> fc1 -> fc2 -> heads of the read-back convolution output with the composed bound: each
    stage's bound goes through the next stage's sum |W|."""
    last, fc1, fc2 = head.conv_layers[2], head.fc_layers[0][0], head.fc_layers[1][0]
    cpu = lambda t: t.detach().cpu()
    heads = ((cpu(head.rotation_pred.weight), cpu(head.rotation_pred.bias)),
             (cpu(head.translation_pred.weight), cpu(head.translation_pred.bias)))
    n, k = parts.shape[1:]
    if fused:
        s1, s2 = head.fc_plan()
        v, vb = fc_gn_ref(f64(fc_operand(parts)), k // last.groups, hw, cpu(last.gn.weight), cpu(last.gn.bias))
        r, b = gemm_ref(v, vb, f64(cpu(fc1.weight)), None, fc_depth(k // s1, False), s1)
        v, vb = parts_ref(r, b, cpu(fc1.bias), True)
        r, b = gemm_ref(v, vb, f64(cpu(fc2.weight)), None, fc_depth(v.shape[1] // s2, False), s2)
        v, vb = parts_ref(r, b, cpu(fc2.bias), True)
        out = [gemm_ref(v, vb, f64(w), f64(bb), fc_depth(v.shape[1], True)) for w, bb in heads]
        return np.concatenate([r[0] for r, _ in out], 1), np.concatenate([e[0] for _, e in out], 1)
    c = k // hw
    v, vb = group_norm_relu_ref(parts.view(parts.shape[0], n, c, hw), cpu(last.gn.weight), cpu(last.gn.bias), last.groups)
    v, vb = v.reshape(n, k), vb.reshape(n, k)
    for fc in (fc1, fc2):
        v, vb = linear_ref_core(v, vb, cpu(fc.weight), cpu(fc.bias), ACT_RELU)
    out = [linear_ref_core(v, vb, w, bb, ACT_NONE) for w, bb in heads]
    return np.concatenate([r for r, _ in out], 1), np.concatenate([e for _, e in out], 1)


@pytest.mark.parametrize('feat_size', list(FC_HEAD_GEOMETRY), ids=lambda v: f'{v[0]}x{v[1]}')
def test_pose_head_tail_against_float64_of_the_read_back_map(feat_size):
    head = _head(feat_size)
    gs, hw_want, s1, k = FC_HEAD_GEOMETRY[feat_size]
    g = torch.Generator().manual_seed(181)
    x = torch.randn((3, 224, *feat_size), generator=g).to(DEV)
    assert head.fc_plan() == (s1, 4) and head.fc_layers[0][0].in_features == k
    parts, hw = _last_conv(head, x)
    assert hw == hw_want and k // head.conv_layers[2].groups == gs
    for fused in (True, False):
        head.fused_fc = fused
        assert (head.fc_plan() != (0, 0)) == fused
        got = torch.cat(head.features(x), 1).cpu()
        assert same_bits(got, torch.cat(head.features(x), 1))
        worst = worst_ratio(got, *_head_ref(head, parts, hw, fused))
        measured(f'pose head tail feat_size {feat_size} fused_fc {fused}, error / composed bound', worst)
        assert worst <= 1.0


@pytest.mark.parametrize('feat_size, kslices', [((8, 8), True), ((8, 24), True), ((8, 8), False)],
                         ids=['8x8', '8x24', '8x8-unsliced'])
def test_pose_head_stages_make_the_written_out_launches(feat_size, kslices):
    """The head's launch list written out with ops calls only, against its two stages and what is composed of them:
    bit equality throughout.  (8, 8): 128 features, the fused route, the last convolution in 4 K-slices (the parts path)
    or unsliced; (8, 24): 384 features, which ``fc_plan()`` refuses, so the linear route whatever ``fused_fc`` says."""
    head = _head(feat_size)
    g = torch.Generator().manual_seed(29)
    n = 2
    x0, x1 = (torch.randn((n, c, *feat_size), generator=g).to(DEV) for c in (128, 96))
    last, fc1, fc2 = head.conv_layers[2], head.fc_layers[0][0], head.fc_layers[1][0]
    rot, trans = head.rotation_pred, head.translation_pred
    prev = ops.set_conv_kslices(kslices)
    try:
        ys, x, xb = [], x0, x1
        for i, blk in enumerate(head.conv_layers):
            ys.append(ops.conv2d(blk.packed, x, xb, kslices=ops.conv_kslices_for(blk.packed, x, xb)))
            if i < 2:
                x, xb = ops.group_norm_relu(ys[-1], blk.gn.weight, blk.gn.bias, blk.groups, blk.gn.eps), None
        y = ys[2]
        if not kslices:
            assert all(v.dim() == 4 for v in ys)
        elif feat_size == (8, 8):
            assert y.dim() == 5 and y.shape[0] == 4
        hw = y.shape[-2] * y.shape[-1]
        feat = y.shape[-3] * hw
        assert feat == fc1.in_features
        for got, want in zip(head._conv_outputs(x0, x1), ys):
            assert got.shape == want.shape and same_bits(got, want)
        assert same_bits(head.tail_input(x0, x1), y)
        for fused in (True, False):
            head.fused_fc = fused
            s1, s2 = head.fc_plan()
            assert (s1 > 0) == (fused and feat_size == (8, 8))
            if s1:
                gn = (last.groups, hw, last.gn.weight, last.gn.bias, last.gn.eps)
                yv = y.view(y.shape[0], n, feat) if y.dim() == 5 else y.view(n, feat)
                p1 = ops.fc_splitk(yv, fc1.weight, gn=gn, slices=s1)
                p2 = ops.fc_splitk(p1, fc2.weight, x_bias=fc1.bias, x_relu=True, slices=s2)
                want = ops.fc_splitk(p2, rot.weight, rot.bias, x_bias=fc2.bias, x_relu=True, weight2=trans.weight,
                                     bias2=trans.bias)
                acts = (ops.fc_operand(yv, gn=gn), ops.fc_operand(p1, x_bias=fc1.bias, x_relu=True),
                        ops.fc_operand(p2, x_bias=fc2.bias, x_relu=True))
            else:
                a0 = ops.group_norm_relu(y, last.gn.weight, last.gn.bias, last.groups, last.gn.eps).view(n, feat)
                a1 = ops.linear(a0, fc1.weight, fc1.bias, ACT_RELU)
                a2 = ops.linear(a1, fc2.weight, fc2.bias, ACT_RELU)
                want = ops.linear_pair(a2, rot.weight, rot.bias, trans.weight, trans.bias)
                acts = (a0, a1, a2)
            for name, got in (('features', head.features(x0, x1)), ('_tail', head._tail(head.tail_input(x0, x1)))):
                assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]), (name, fused)
            # the (parts, M, C, h, w) form tail_backward hands over: one part for an unsliced convolution
            got = head._tail(y if y.dim() == 5 else y.unsqueeze(0), activations=True)
            assert len(got) == 3
            for a, b in zip(got, acts):
                assert a.shape == b.shape and torch.equal(a > 0, b > 0) and same_bits(a, b), fused
    finally:
        ops.set_conv_kslices(prev)


# ================================================================================================== 2d: two heads
@pytest.mark.parametrize('n', [1, 33])
@pytest.mark.parametrize('o, o2', FC_TWO_HEADS)
def test_fc_two_heads_in_one_launch(o, o2, n):
    worst = [0.0, 0.0]
    for shape in (fc_shape(n, 72, o, o2=o2, parts=2, x_bias=True, x_relu=True), fc_shape(n, 256, o, o2=o2, act=ACT_TANH)):
        c = fc_case('nominal', shape)
        got = fc_run(c)
        ref, bound = fc_ref(c)
        worst = [max(worst[0], worst_ratio(got[:, :o], ref[:, :o], bound[:, :o])),
                 max(worst[1], worst_ratio(got[:, o:], ref[:, o:], bound[:, o:]))]
        one = fc_launch(Case(c, o2=0, w2=None, bias2=None))
        two = fc_launch(Case(c, o=o2, o2=0, w=c.w2, bias=c.bias2, w2=None, bias2=None))
        assert same_bits(got, torch.cat([one, two], 1)), 'a pair launch differs from two single launches'
    measured(f'fc_splitk two heads ({o}, {o2}) N {n}, error / bound (y, y2)', max(worst))
    assert worst[0] <= 1.0 and worst[1] <= 1.0


# ============================================================================================ 2e: linear / linear_pair
@pytest.mark.parametrize('k, n, o, act, bias', LINEAR_SINGLE)
def test_linear_paths_tails_and_blocks(k, n, o, act, bias):
    worst = {}
    for regime in LINEAR_REGIMES:
        c = linear_case(regime, linear_shape(n, k, o, act=act, bias=bias))
        worst[regime] = worst_ratio(linear_run(c), *linear_ref(c))
    measured(f'linear K {k} N {n} O {o} act {act} bias {bias}, error / bound', max(worst.values()))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize('pair, kn', list(zip(LINEAR_PAIRS, LINEAR_PAIR_KN)), ids=lambda v: str(v))
def test_linear_pair_is_two_linear_launches(pair, kn):
    (o, o2), (k, n) = pair, kn
    worst = 0.0
    for regime, act in [('nominal', a) for a in ACTS] + [('cancelling_k', ACT_NONE)]:
        c = linear_case(regime, linear_shape(n, k, o, o2=o2, act=act))
        got = linear_run(c)
        ref, bound = linear_ref(c)
        assert worst_ratio(got[:, :o], ref[:, :o], bound[:, :o]) <= 1.0 and worst_ratio(got[:, o:], ref[:, o:], bound[:, o:]) <= 1.0
        worst = max(worst, worst_ratio(got, ref, bound))
        one = linear_launch(Case(c, o2=0, w2=None, bias2=None))
        two = linear_launch(Case(c, o=o2, o2=0, w=c.w2, bias=c.bias2, w2=None, bias2=None))
        assert same_bits(got, torch.cat([one, two], 1)), 'linear_pair differs from two linear launches'
    measured(f'linear_pair ({o}, {o2}) K {k} N {n}, error / bound', worst)


# ============================================================================================= 2f: bit-level properties
def test_batch_invariance_of_every_mode_at_65_rows():
    """row n of an N = 65 launch (three row tiles, the last with one row) is the N = 1 launch of that sample"""
    shapes = [fc_shape(65, 136, 33, act=a) for a in ACTS]
    shapes += [fc_shape(65, 3 * 72, 40, slices=3), fc_shape(65, 40, 33, parts=5, x_bias=True, x_relu=True, act=ACT_RELU),
               fc_shape(65, 256, 33, slices=2, gn=(64, 16)), fc_shape(65, 96, 33, slices=2, gn=(16, 4)),
               fc_shape(65, 72, 33, o2=31, parts=2, x_bias=True, x_relu=True)]
    for shape in shapes:
        c = fc_case('nominal', shape)
        got = fc_launch(c)
        for r in (0, 31, 32, 63, 64):
            assert same_bits(got[..., r:r + 1, :], fc_launch(rows_of(c, r))), (shape, r)
    for k, o2 in ((1028, 0), (65, 0), (256, 63)):
        c = linear_case('nominal', linear_shape(65, k, 5, o2=o2, act=ACT_RELU))
        got = linear_launch(c)
        for r in (0, 7, 8, 63, 64):
            assert same_bits(got[r:r + 1], linear_launch(Case(c, n=1, x=c.x[r:r + 1].contiguous()))), (k, r)


def test_power_of_two_scaling_is_exact():
    for n, o, k, act, bias in FC_FINISHED[::5]:
        shape = fc_shape(n, k, o, act=act if act == ACT_RELU else ACT_NONE, bias=False)
        base = fc_launch(fc_case('nominal', shape))
        for regime in SCALES:
            c = fc_case(regime, shape)
            assert same_bits(fc_launch(c), base * c.scale), (regime, shape)
    c0 = fc_case('nominal', fc_shape(33, 2 * 72, 40, slices=2, bias=False))
    for regime in SCALES:
        c = fc_case(regime, fc_shape(33, 2 * 72, 40, slices=2, bias=False))
        assert same_bits(fc_launch(c), fc_launch(c0) * c.scale)
    for k, n, o, act, bias in LINEAR_SINGLE[::4]:
        shape = linear_shape(n, k, o, act=act if act == ACT_RELU else ACT_NONE, bias=False)
        base = linear_launch(linear_case('nominal', shape))
        for regime in SCALES:
            c = linear_case(regime, shape)
            assert same_bits(linear_launch(c), base * c.scale), (regime, shape)


def _codes(t):
    t = f64(t)
    return np.where(np.isnan(t), 1, np.where(np.isinf(t), 2, 0))


def test_row_and_column_isolation():
    """one NaN in x[1, 5], one +inf in W[2, 9] with x[3, 9] == 0 (nonfinite_case): NaN in exactly row 1 of every output,
    both heads, and of the slice that holds k = 5; column 2 of the first head +-inf with (3, 2) NaN, as in torch; every
    other element finite and inside its bound."""
    c = nonfinite_case()
    want = np.concatenate([nonfinite_pattern(c), np.where(np.arange(4)[:, None] == 1, 1, 0) * np.ones((1, 3), dtype=np.int64)], 1)
    clean = want == 0
    ref, bound = fc_ref(c)
    lin = Case(c, x=c.x[0])
    for name, got in (('fc_splitk', fc_run(c)), ('linear_pair', linear_run(lin))):
        assert np.array_equal(_codes(got), want), name
        assert bool((got[[0, 2], 2] == float('inf')).all()), name
        r, b = (ref, bound) if name == 'fc_splitk' else linear_ref(lin)
        assert worst_ratio(got.numpy()[clean], r[clean], b[clean]) <= 1.0, name
    p = Case(c, slices=2, o2=0, w2=None, bias2=None, bias=None)     # slice 0: k 0..7 (the NaN), slice 1: k 8..15 (the inf)
    got = fc_run(p)
    want0, want1 = np.zeros((4, 6), dtype=np.int64), nonfinite_pattern(c).copy()
    want0[1, :] = 1
    want1[1, :] = 0
    want1[1, 2] = 2
    assert np.array_equal(_codes(got[0]), want0) and np.array_equal(_codes(got[1]), want1)
    ref, bound = fc_ref(p)
    clean = np.stack([want0, want1]) == 0
    assert worst_ratio(got.numpy()[clean], ref[clean], bound[clean]) <= 1.0


def test_relu_of_a_nonfinite_partial_sum_is_zero_in_the_consumer():
    """THE DIVERGENCE FROM torch.relu (module docstring): a NaN and a -inf partial sum under x_relu are 0 in the
    consumer's operand (fmaxf), so its outputs are finite -- the same as with partial sums of -1e30 there -- where
    torch.relu(NaN) is NaN and would poison row 1."""
    shape = fc_shape(4, 40, 33, o2=5, parts=3, x_bias=True, x_relu=True)
    c, z = fc_case('nominal', shape), fc_case('nominal', shape)
    c.x[1, 1, 7], c.x[2, 2, 30] = float('nan'), float('-inf')
    z.x[1, 1, 7], z.x[2, 2, 30] = -1e30, -1e30
    assert bool(torch.isnan(fc_operand(c.x, c.x_bias, True)[1, 7]))             # what torch.relu makes of it
    got = fc_run(c)
    assert bool(torch.isfinite(got).all())
    assert same_bits(got, fc_launch(z))
    assert worst_ratio(got, *fc_ref(z)) <= 1.0


def test_relu_of_a_nan_preactivation_is_zero_in_both_kernels():
    """a finished ReLU output of a NaN pre-activation is KERNEL_RELU_OF_NAN = 0 (v > 0 ? v : 0) in fc_splitk and in
    linear; every other row is inside its bound.  torch.relu would return NaN in row 1."""
    c = fc_case('nominal', fc_shape(4, 72, 33, act=ACT_RELU))
    c.x[0, 1, 70] = float('nan')
    lin = Case(c, x=c.x[0], o2=0)
    rows = [0, 2, 3]
    for name, got, (ref, bound) in (('fc_splitk', fc_run(c), fc_ref(c)), ('linear', linear_run(lin), linear_ref(lin))):
        assert bool((got[1] == KERNEL_RELU_OF_NAN).all()), name
        assert worst_ratio(got[rows], ref[rows], bound[rows]) <= 1.0, name


def test_relu_divergence_fused_and_unfused_head_agree():
    """a NaN weight makes feature 3 of fc1 NaN for every sample.  Both tails turn it into 0 (the fused one in fc2's
    operand load, the unfused one in scf_linear's ReLU) and return a finite pose: bit for bit the pose of a head whose
    fc1 feature 3 is 0 (zero weights, bias -1)."""
    head, zero = _head((8, 8)), _head((8, 8))
    with torch.no_grad():
        head.fc_layers[0][0].weight[3, 17] = float('nan')
        zero.fc_layers[0][0].weight[3, :] = 0.0
        zero.fc_layers[0][0].bias[3] = -1.0
    x = torch.randn((3, 224, 8, 8), generator=torch.Generator().manual_seed(7)).to(DEV)
    for fused in (True, False):
        head.fused_fc = zero.fused_fc = fused
        got, want = torch.cat(head.features(x), 1), torch.cat(zero.features(x), 1)
        assert bool(torch.isfinite(got).all()) and same_bits(got, want), fused


# ----------------------------------------------------------------------------------------------------- raw C-ABI calls
def fc_desc(x, w, y, n, k, o, **over):
    d = _lib.FcDesc()
    d.x, d.x_parts, d.x_part_stride, d.N, d.K = x.data_ptr(), 1, n * k, n, k
    d.W, d.y, d.O, d.act, d.slices = w.data_ptr(), y.data_ptr(), o, ACT_NONE, 1
    for name, v in over.items():
        setattr(d, name, v.data_ptr() if isinstance(v, torch.Tensor) else v)
    return d


def fc_raw(d):
    code = _lib.load().scf_fc_splitk(C.byref(d), ops._stream())
    torch.cuda.synchronize()
    return code


@pytest.mark.parametrize('n', [1, 33])
@pytest.mark.parametrize('o, o2', [(1, 0), (33, 0), (126, 63), (33, 1)])
def test_no_stray_writes(n, o, o2):
    """y, y2 and the (slices, N, O) partial tensor as interior views of sentinel-filled buffers"""
    c = fc_case('nominal', fc_shape(n, 72, o, o2=o2))
    xd, wd, bd = D(c.x[0]), D(c.w), D(c.bias)
    buf, y = guarded((n, o))
    over = dict(bias=bd)
    if o2:
        buf2, y2 = guarded((n, o2))
        w2d, b2d = D(c.w2), D(c.bias2)
        over.update(W2=w2d, bias2=b2d, y2=y2, O2=o2)
    assert fc_raw(fc_desc(xd, wd, y, n, 72, o, **over)) == 0
    assert guard_untouched(buf, (n, o)) and (not o2 or guard_untouched(buf2, (n, o2)))
    got = torch.cat([y, y2], 1) if o2 else y
    assert same_bits(got, fc_launch(c))
    if not o2:
        bufp, yp = guarded((3, n, o))
        assert fc_raw(fc_desc(xd, wd, yp, n, 72, o, slices=3)) == 0
        assert guard_untouched(bufp, (3, n, o))
        assert same_bits(yp, fc_launch(fc_case('nominal', fc_shape(n, 72, o, slices=3))))


def test_fc_rejections_through_the_c_abi():
    """each returns its documented code and launches nothing (the sentinel-filled output stays as it is)"""
    n, o = 4, 8
    big = torch.zeros((4 * 2048 + 64,), device=DEV)
    w = torch.zeros((8 * 2048 + 64,), device=DEV)
    ones = torch.ones((2048,), device=DEV)
    y = torch.full((8, n, o), SENTINEL, device=DEV)
    y2 = torch.full((n, o), SENTINEL, device=DEV)

    def code(k, x=big, wt=w, **over):
        return fc_raw(fc_desc(x, wt, y, n, k, o, **over))

    assert code(264) == EUNSUPPORTED                                # Ks = 264 > 256
    assert code(12) == EUNSUPPORTED and code(2 * 60, slices=2) == EUNSUPPORTED          # Ks % 8 != 0
    assert code(64, slices=3) == EUNSUPPORTED                       # K % slices != 0
    assert code(64, x=big[1:]) == EUNSUPPORTED and code(64, wt=w[1:]) == EUNSUPPORTED   # pointers 4 bytes off
    assert code(64, W2=w[1:], y2=y2, O2=o) == EUNSUPPORTED and code(64, x_bias=ones[1:]) == EUNSUPPORTED
    assert code(64, x_parts=2, x_part_stride=n * 64 + 2) == EUNSUPPORTED
    gn = dict(gn_gamma=ones, gn_beta=ones, gn_hw=1, gn_eps=IN_EPS)
    assert code(96, slices=2, gn_groups=3, **gn) == EUNSUPPORTED   # groups of 32 in slices of 48
    assert code(72, gn_groups=8, **gn) == EUNSUPPORTED              # groups of 9
    assert code(128, slices=2, W2=w, y2=y2, O2=o) == EUNSUPPORTED   # two heads: finished outputs only
    assert code(64, y2=y2, O2=o) == EINVAL and code(64, W2=w, O2=o) == EINVAL
    assert code(64, gn_groups=4, gn_hw=1) == EINVAL                 # GroupNorm without gamma / beta
    assert bool((y == SENTINEL).all()) and bool((y2 == SENTINEL).all())
    assert code(64, W2=w, y2=y2, O2=o) == 0 and code(128, slices=2) == 0    # the accepted neighbours of the above
    assert bool((y[:2] == 0).all()) and bool((y2 == 0).all()) and bool((y[2:] == SENTINEL).all())


def test_linear_alignment_rule():
    """a pointer that is not 16-byte aligned: refused with K % 4 == 0 (the float4 path would fault or read shifted
    data), and run -- correctly -- on the scalar path with K % 4 != 0"""
    lib = _lib.load()
    for k, ok in ((64, False), (63, True)):
        c = linear_case('nominal', linear_shape(9, k, 5))
        base = torch.zeros((9 * k + 8,), device=DEV)
        base[1:1 + 9 * k] = D(c.x).flatten()
        x = base[1:1 + 9 * k]
        assert x.data_ptr() % 16 == 4
        buf, y = guarded((9, 5))
        wd, bd = D(c.w), D(c.bias)
        code = lib.scf_linear(x.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.data_ptr(), 9, k, 5, ACT_NONE, ops._stream())
        torch.cuda.synchronize()
        assert guard_untouched(buf, (9, 5))
        if ok:
            assert code == 0 and worst_ratio(y.cpu(), *linear_ref(c)) <= 1.0
            assert same_bits(y, linear_launch(c))
        else:
            assert code == EUNSUPPORTED and bool((y == SENTINEL).all())


# ======================================================================================= 3: the Python entry points
def test_python_entry_points_check_vector_lengths_and_weight_rank():
    """a short bias / x_bias / gamma / beta, or a weight that is not 2-D, was read past its end: now ScflowHipError"""
    x, w, b = torch.zeros((4, 64), device=DEV), torch.zeros((8, 64), device=DEV), torch.zeros((8,), device=DEV)
    w2, b2 = torch.zeros((5, 64), device=DEV), torch.zeros((5,), device=DEV)
    gam = torch.ones((16,), device=DEV)                             # hw = 4: 16 channels
    bad = [lambda: ops.linear(x, w, b[:7]), lambda: ops.linear(x, w, torch.zeros((9,), device=DEV)),
           lambda: ops.linear(x, w.view(8, 8, 8), b), lambda: ops.linear(x, w.flatten(), b),
           lambda: ops.linear_pair(x, w, b[:7], w2, b2), lambda: ops.linear_pair(x, w, b, w2, b2[:4]),
           lambda: ops.linear_pair(x, w, b, w2.view(5, 8, 8), b2), lambda: ops.linear_pair(x, w[:, :60], b, w2, b2),
           lambda: ops.fc_splitk(x, w, b[:7]), lambda: ops.fc_splitk(x, w, b, x_bias=torch.zeros((63,), device=DEV)),
           lambda: ops.fc_splitk(x, w, b, weight2=w2, bias2=b2[:4]),
           lambda: ops.fc_splitk(x, w, b, weight2=w2.view(5, 8, 8), bias2=b2),
           lambda: ops.fc_splitk(x, w.view(8, 8, 8), b),
           lambda: ops.fc_splitk(x, w, b, gn=(4, 4, gam[:15], gam, IN_EPS)),
           lambda: ops.fc_splitk(x, w, b, gn=(4, 4, gam, gam[:15], IN_EPS)),
           lambda: ops.fc_splitk(x, w, b, gn=(4, 3, gam, gam, IN_EPS)),            # hw = 3: ceil(64 / 3) = 22 channels
           lambda: ops.fc_splitk(x, w, b, gn=(4, 0, gam, gam, IN_EPS))]
    for i, call in enumerate(bad):
        with pytest.raises(ScflowHipError):
            call()
            pytest.fail(f'call {i} was accepted')
    # the accepted neighbours
    ops.linear(x, w, b), ops.linear_pair(x, w, b, w2, b2), ops.fc_splitk(x, w, b, weight2=w2, bias2=b2)
    ops.fc_splitk(x, w, b, x_bias=torch.zeros((64,), device=DEV), gn=(4, 4, gam, gam, IN_EPS))
    ops.fc_splitk(x, w, b, gn=(4, 3, torch.ones((22,), device=DEV), torch.ones((22,), device=DEV), IN_EPS))
    torch.cuda.synchronize()
