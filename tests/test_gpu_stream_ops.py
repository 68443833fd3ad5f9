"""GPU: norm.hip (scf_instance_norm, scf_group_norm_relu[_parts]), resample.hip (scf_resize_bilinear, scf_avgpool2x2,
scf_mul_mask, scf_copy_strided, scf_convex_upsample) and pose.hip (scf_pose_update, scf_reproject_flow,
scf_unproject_depth, scf_filter_flow_by_mask) against the float64 restatements and derived bounds of
tests/test_stream_ops_host.py -- on every launch route of each entry point, at the smallest shapes that reach it, and in
the regimes where a normalisation, a softmax or a projection goes wrong (offset means, constant planes, saturated and
tied logits, qz near 0, degenerate 6-D rotations, non-finite inputs).  The shape lists and the comments on which branch
each shape takes live next to the restatements (IN_SHAPES, GN_HW, RESIZE_SIZES, ...); this file adds what only a launch
has: alignment, aliasing, strides and guard bands.

Every comparison is `error <= bound` (ratio <= 1) or bit equality.  Elements are left out only where the restatement
itself says there is no bound -- |qz| < 64 U S_qz in the re-projection, a sampled mask inside 0.9 +- margin in the
filter -- and each such case asserts that they are at most 1 % of what it compares.

Left out on purpose: the merged launches of scf_scflow_iteration (pose update inside the re-projection launch, the
two-job resize and its second destination).  test_c_iteration_is_bit_identical (tests/test_gpu_refiner.py) holds them
bit-identical to the stand-alone entry points tested here.

The measured error-to-bound ratios are recorded in DESIGN.md section 4.
"""
import numpy as np
import pytest
import torch

from scflow_amd import _lib, ops
from test_stream_ops_host import (CONVEX_NONFINITE, CONVEX_REGIMES, CONVEX_SIZES, FILTER_INVALID,  # noqa: E402
                                  FILTER_SIZES, GEOM_POSES, GEOM_SIZES, GN_G, GN_HW, GN_PARTS, GN_REGIMES, IN_EPS,
                                  IN_REGIME_SHAPES, IN_REGIMES, IN_SHAPES, NUM_CLASS, POOL_SIZES, POSE_N, POSE_REGIMES,
                                  RESIZE_SIZES, avgpool_ref, check_left_out, convex_case, convex_ref, f64, filter_agrees,
                                  filter_case, filter_ref, geom_case, gn_case, group_norm_relu_ref, in_case,
                                  instance_norm_ref, measured, orthonormality_bound, pose_case, pose_update_ref,
                                  reproject_ref, resize_case, resize_ref, same_bits, same_nan_pattern,
                                  torch_instance_norm, unproject_ref, worst_ratio)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = -7777.25
GUARD = 64                          # floats on either side of a guarded output: a multiple of 4, so alignment is kept


def guarded(shape, off=0):
    """a sentinel-filled buffer and a contiguous view of `shape` GUARD + off floats into it."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD + off,), SENTINEL, dtype=torch.float32, device=DEV)
    return buf, buf[GUARD + off:GUARD + off + n].view(shape)


def guard_untouched(buf, shape, off=0):
    n = int(np.prod(shape))
    want = torch.full_like(buf, SENTINEL)
    return same_bits(buf[:GUARD + off], want[:GUARD + off]) and same_bits(buf[GUARD + off + n:], want[GUARD + off + n:])


def raw(name, *args):
    return getattr(_lib.load(), name)(*args, ops._stream())


# ======================================================================================================= InstanceNorm
def _in_variants(x, res, aligned=True, off=0):
    """(name, got, reference, bound) of one input through every calling form: res None / given, ReLU off / on,
    out-of-place into a guarded buffer, in place (out is x), and with the residual aliasing the output."""
    xd, rd = x.to(DEV), res.to(DEV)
    for r, rdev in ((None, None), (res, rd)):
        for relu in (False, True):
            ref, bound = instance_norm_ref(x, r, relu, aligned)
            buf, out = guarded(x.shape, off)
            ops.instance_norm(xd, rdev, relu, out=out)
            assert guard_untouched(buf, x.shape, off), 'guard band written'
            yield f'res={r is not None} relu={relu}', out.cpu(), ref, bound
            xin = xd.clone()
            ops.instance_norm(xin, rdev, relu, out=xin)
            assert same_bits(xin, out), 'in place (out is x) differs from out of place'
            if r is not None:
                alias = rd.clone()
                ops.instance_norm(xd, alias, relu, out=alias)
                assert same_bits(alias, out), 'res aliasing out differs from out of place'


@pytest.mark.parametrize('shape', IN_SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_instance_norm_every_route(shape):
    x, res = in_case('nominal', shape)
    worst = max(worst_ratio(got, ref, bound) for _, got, ref, bound in _in_variants(x, res))
    measured(f'instance_norm {shape} nominal, error / bound', worst)
    assert worst <= 1.0


@pytest.mark.parametrize('which', ['x', 'out', 'res', 'all'])
def test_instance_norm_misaligned_pointer_takes_the_generic_kernel(which):
    """a (32, 32) plane set one float into a larger buffer: HW % 4 == 0 but a pointer is not 16-byte aligned, so the launch
    must fall back to the generic kernel (a float4 access there would fault or read shifted data)."""
    shape = (2, 3, 32, 32)
    x, res = in_case('nominal', (32, 32))
    n = x.numel()

    def place(t, mis):                                              # 4 floats into a fresh allocation: aligned; 1 float: not
        base = torch.zeros((n + 8,), device=DEV)
        o = 1 if mis else 4
        base[o:o + n] = t.flatten().to(DEV)
        return base[o:o + n].view(shape)

    xd, rd = place(x, which in ('x', 'all')), place(res, which in ('res', 'all'))
    assert (xd.data_ptr() % 16 != 0) == (which in ('x', 'all')) and (rd.data_ptr() % 16 != 0) == (which in ('res', 'all'))
    off = 1 if which in ('out', 'all') else 0
    buf, out = guarded(shape, off)
    assert (out.data_ptr() % 16 != 0) == bool(off)
    ops.instance_norm(xd, rd, True, out=out)
    assert guard_untouched(buf, shape, off)
    ref, bound = instance_norm_ref(x, res, True, aligned=False)
    worst = worst_ratio(out.cpu(), ref, bound)
    measured(f'instance_norm (32, 32) misaligned {which}, error / bound', worst)
    assert worst <= 1.0


@pytest.mark.parametrize('shape', IN_REGIME_SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
@pytest.mark.parametrize('regime', IN_REGIMES[1:])
def test_instance_norm_regimes(regime, shape):
    x, res = in_case(regime, shape)
    worst = max(worst_ratio(got, ref, bound) for _, got, ref, bound in _in_variants(x, res))
    measured(f'instance_norm {shape} {regime}, error / bound', worst)
    assert worst <= 1.0


@pytest.mark.parametrize('shape', IN_REGIME_SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_instance_norm_poisoned_planes(shape):
    """one NaN in plane (0, 1), one +inf in plane (1, 0).  Every other plane is unaffected and inside its bound.  Without
    ReLU the poisoned planes are NaN throughout, as in torch; with ReLU they are 0 throughout -- the kernel's ReLU is
    v_max (NaN -> 0, its comment), where torch.relu keeps the NaN."""
    x, res = in_case('nominal', shape)
    x[0, 1, shape[0] // 2, shape[1] // 3] = float('nan')
    x[1, 0, 0, 0] = float('inf')
    bad = torch.tensor([[False, True, False], [True, False, False]])
    for r in (None, res):
        for relu in (False, True):
            got = ops.instance_norm(x.to(DEV), None if r is None else r.to(DEV), relu).cpu()
            ref, bound = instance_norm_ref(x, r, relu)
            assert worst_ratio(got[~bad], ref[~bad.numpy()], bound[~bad.numpy()]) <= 1.0
            if relu:
                assert bool((got[bad] == 0).all())
            else:
                assert bool(torch.isnan(got[bad]).all())
                assert same_nan_pattern(got, torch_instance_norm(x, r, False))


# ========================================================================================================== GroupNorm
def _gn_run(p, gamma, beta, groups, hw_shape, pad=0):
    """parts (S, N, C, HW) -> the kernel's output (N, C, HW); pad > 0 puts the parts `pad` floats further apart than
    N C HW (part_stride larger than a part)."""
    s, n, c, hw = p.shape
    store = torch.full((s, n * c * hw + pad), SENTINEL, dtype=torch.float32, device=DEV)
    store[:, :n * c * hw] = p.reshape(s, -1).to(DEV)
    buf, out = guarded((n, c, hw))
    gd, bd = gamma.to(DEV), beta.to(DEV)
    code = raw('scf_group_norm_relu_parts', store.data_ptr(), s, store.stride(0), gd.data_ptr(), bd.data_ptr(),
               out.data_ptr(), n, c, hw, groups, IN_EPS)
    _lib.check(code, 'scf_group_norm_relu_parts')
    assert guard_untouched(buf, (n, c, hw))
    if pad == 0 and s > 1:                                          # the python entry takes the same parts as a 5-D tensor
        via = ops.group_norm_relu(p.to(DEV).view(s, n, c, *hw_shape), gd, bd, groups)
        assert same_bits(via.view(n, c, hw), out)
    return out.cpu()


def _hw_shape(hw):
    return (23, 23) if hw == 529 else (1, hw)


@pytest.mark.parametrize('parts', GN_PARTS)
@pytest.mark.parametrize('hw', GN_HW)
def test_group_norm_relu_sizes_and_parts(hw, parts):
    p, gamma, beta = gn_case('nominal', hw, parts)
    ref, bound = group_norm_relu_ref(p, gamma, beta, GN_G)
    worst = worst_ratio(_gn_run(p, gamma, beta, GN_G, _hw_shape(hw)), ref, bound)
    measured(f'group_norm_relu HW {hw} parts {parts}, error / bound', worst)
    assert worst <= 1.0


@pytest.mark.parametrize('hw, parts', [(16, 1), (512, 3), (513, 5)])
@pytest.mark.parametrize('regime', GN_REGIMES[1:])
def test_group_norm_relu_regimes(regime, hw, parts):
    """`cancelling`: part0 = -part1 + small.  The reference adds the parts IN ORDER and rounds every partial sum to fp32
    (gn_sum_parts): that sum is the function the kernel computes, any other order is another function."""
    p, gamma, beta = gn_case(regime, hw, parts)
    ref, bound = group_norm_relu_ref(p, gamma, beta, GN_G)
    worst = worst_ratio(_gn_run(p, gamma, beta, GN_G, _hw_shape(hw)), ref, bound)
    measured(f'group_norm_relu HW {hw} parts {parts} {regime}, error / bound', worst)
    assert worst <= 1.0


def test_group_norm_relu_part_stride_larger_than_a_part():
    p, gamma, beta = gn_case('nominal', 513, 5)
    ref, bound = group_norm_relu_ref(p, gamma, beta, GN_G)
    assert worst_ratio(_gn_run(p, gamma, beta, GN_G, (1, 513), pad=52), ref, bound) <= 1.0
    p, gamma, beta = gn_case('nominal', 16, 3)
    ref, bound = group_norm_relu_ref(p, gamma, beta, GN_G)
    assert worst_ratio(_gn_run(p, gamma, beta, GN_G, (1, 16), pad=3), ref, bound) <= 1.0


@pytest.mark.parametrize('hw', [16, 256])
def test_group_norm_relu_pose_head_shape(hw):
    """C = 128, G = 32 at 4 x 4 and 16 x 16: the groups the pose head normalises."""
    p, gamma, beta = gn_case('nominal', hw, 1, c=128, groups=32)
    ref, bound = group_norm_relu_ref(p, gamma, beta, 32)
    got = ops.group_norm_relu(p[0].to(DEV).view(2, 128, int(hw ** 0.5), -1), gamma.to(DEV), beta.to(DEV), 32)
    worst = worst_ratio(got.cpu().view(2, 128, hw), ref, bound)
    measured(f'group_norm_relu C 128 G 32 HW {hw}, error / bound', worst)
    assert worst <= 1.0


def test_group_norm_relu_rejections():
    x = torch.zeros((3, 2, 8, 16), device=DEV)
    g = torch.ones((8,), device=DEV)
    out = torch.empty((2, 8, 16), device=DEV)
    assert raw('scf_group_norm_relu_parts', x.data_ptr(), 1, 0, g.data_ptr(), g.data_ptr(), out.data_ptr(), 2, 8, 16, 3,
               IN_EPS) != 0                                         # C % G != 0
    assert raw('scf_group_norm_relu_parts', x.data_ptr(), 3, 2 * 8 * 16 - 1, g.data_ptr(), g.data_ptr(), out.data_ptr(),
               2, 8, 16, 2, IN_EPS) != 0                            # parts > 1 with a stride shorter than a part
    assert raw('scf_group_norm_relu_parts', x.data_ptr(), 3, 2 * 8 * 16, g.data_ptr(), g.data_ptr(), out.data_ptr(),
               2, 8, 16, 2, IN_EPS) == 0


# ============================================================================================================= resize
def _resize_check(planes, in_hw, out_hw, off=0):
    worst = {}
    for kind in ('nominal', 'checker'):
        a, b = resize_case(kind, planes, in_hw)
        ad, bd = a.to(DEV).view(-1, 10 if planes % 10 == 0 else 1, *in_hw), b.to(DEV).view(-1, 10 if planes % 10 == 0 else 1, *in_hw)
        for mul in (1.0, 0.125):
            for bb, bdev in ((None, None), (b, bd)):
                shape = (*ad.shape[:2], *out_hw)
                buf, out = guarded(shape, off)
                ops.resize_bilinear(ad, out_hw, mul, bdev, out=out)
                assert guard_untouched(buf, shape, off), 'guard band written'
                got = out.cpu().view(planes, *out_hw)
                for coords in ('exact', 'fp32'):
                    ref, bound = resize_ref(a, out_hw, mul, bb, coords)
                    worst[coords] = max(worst.get(coords, 0.0), worst_ratio(got, ref, bound))
    return worst


@pytest.mark.parametrize('planes, in_hw, out_hw', RESIZE_SIZES, ids=lambda v: str(v).replace(' ', ''))
def test_resize_bilinear_sizes(planes, in_hw, out_hw):
    """inside the bound against exact coordinates (continuity covers a rounded coordinate on the other side of an
    integer) AND inside the sharp bound against the coordinates as fp32 defines them (no coordinate term at all)."""
    worst = _resize_check(planes, in_hw, out_hw)
    for coords, v in worst.items():
        measured(f'resize_bilinear {in_hw}->{out_hw} x{planes}, {coords} coordinates, error / bound', v)
        assert v <= 1.0, coords


def test_resize_bilinear_misaligned_out_takes_scalar_stores():
    """Wout % 4 == 0 but `out` one float off 16-byte alignment: the scalar-store form must be chosen."""
    worst = _resize_check(4, (3, 3), (5, 8), off=1)
    assert max(worst.values()) <= 1.0


# ================================================================================================== pool, mask, copy
@pytest.mark.parametrize('hw', POOL_SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_avgpool2x2_sizes(hw):
    x = torch.randn((2, 3, *hw), generator=torch.Generator().manual_seed(hw[0] * 100 + hw[1])) * 3 + 1
    ref, bound = avgpool_ref(x.view(6, *hw))
    got = ops.avgpool2x2(x.to(DEV)).cpu()
    assert got.shape == (2, 3, hw[0] // 2, hw[1] // 2)
    worst = worst_ratio(got.view(6, hw[0] // 2, hw[1] // 2), ref, bound)
    measured(f'avgpool2x2 {hw}, error / bound', worst)
    assert worst <= 1.0


def test_avgpool2x2_rejects_sizes_below_two():
    out = torch.empty((8,), device=DEV)
    for hw in ((1, 4), (4, 1), (1, 1)):
        x = torch.zeros((2, *hw), device=DEV)
        assert raw('scf_avgpool2x2', x.data_ptr(), out.data_ptr(), 2, hw[0], hw[1]) != 0


def test_mul_mask_dense_and_channel_slices():
    """bit-equal to the fp32 product; with x and out channel slices of wider tensors the neighbouring channels of out
    keep their bits."""
    g = torch.Generator().manual_seed(23)
    x, mask = torch.randn((3, 5, 6, 7), generator=g), torch.randn((3, 1, 6, 7), generator=g)
    assert same_bits(ops.mul_mask(x.to(DEV), mask.to(DEV)), x * mask)
    wide_x = torch.randn((3, 9, 6, 7), generator=g)
    wide_out = torch.full((3, 8, 6, 7), SENTINEL, device=DEV)
    ops.mul_mask(wide_x.to(DEV)[:, 2:7], mask.to(DEV), out=wide_out[:, 1:6])
    assert same_bits(wide_out[:, 1:6], wide_x[:, 2:7] * mask)
    keep = torch.full((3, 8, 6, 7), SENTINEL)
    assert same_bits(wide_out[:, :1], keep[:, :1]) and same_bits(wide_out[:, 6:], keep[:, 6:])


@pytest.mark.parametrize('count, sns, dns, soff, doff, n', [
    (64, 80, 96, 0, 0, 3),             # VEC: count, strides and pointers all multiples of 4 floats
    (63, 80, 96, 0, 0, 3),             # count % 4: scalar
    (64, 81, 96, 0, 0, 3),             # source stride % 4: scalar
    (64, 80, 98, 0, 0, 3),             # destination stride % 4: scalar
    (64, 80, 96, 1, 0, 3),             # source pointer one float off: scalar
    (64, 80, 96, 0, 1, 3),             # destination pointer one float off: scalar
    (1100000, 1100008, 1100012, 0, 0, 2),      # 550 000 float4 units > 8 x 256 CUs x 256 threads: the VEC grid-stride loop
    (300001, 300001, 300004, 0, 0, 2),         # 600 002 scalar units: the scalar grid-stride loop
])
def test_copy_strided_forms(count, sns, dns, soff, doff, n):
    g = torch.Generator().manual_seed(count + sns)
    src = torch.randn((n * sns + 8,), generator=g).to(DEV)
    buf = torch.full((n * dns + 2 * GUARD + 8,), SENTINEL, device=DEV)
    dst = buf[GUARD + doff:]
    assert src.data_ptr() % 16 == 0 and buf.data_ptr() % 16 == 0
    _lib.check(raw('scf_copy_strided', src[soff:].data_ptr(), sns, dst.data_ptr(), dns, n, count), 'scf_copy_strided')
    want = torch.full_like(buf, SENTINEL)
    for i in range(n):
        want[GUARD + doff + i * dns:GUARD + doff + i * dns + count] = src[soff + i * sns:soff + i * sns + count]
    assert same_bits(buf, want)


# ==================================================================================================== convex upsample
@pytest.mark.parametrize('size', CONVEX_SIZES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('regime', CONVEX_REGIMES)
def test_convex_upsample_regimes(regime, size):
    x, m, x_mul, mask_mul = convex_case(regime, size)
    ref, bound = convex_ref(x, m, x_mul, mask_mul)
    n, c, h, w = size
    buf, out = guarded((n, c, 8 * h, 8 * w))
    ops.convex_upsample(x.to(DEV), m.to(DEV), 8, x_mul, mask_mul, out=out)
    assert guard_untouched(buf, (n, c, 8 * h, 8 * w))
    worst = worst_ratio(out.cpu(), ref, bound)
    measured(f'convex_upsample {size} {regime}, error / bound', worst)
    assert worst <= 1.0


@pytest.mark.parametrize('regime', CONVEX_NONFINITE)
def test_convex_upsample_nonfinite_logits_like_softmax(regime):
    """the NaN pattern of the float64 softmax restatement (recorded against torch in the host file): a NaN or +inf logit
    -> its sub-pixel NaN; one -inf -> weight 0; all nine -inf -> NaN; finite outputs inside the bound."""
    x, m, x_mul, mask_mul = convex_case(regime, (2, 2, 3, 33))
    ref, bound = convex_ref(x, m, x_mul, mask_mul)
    got = ops.convex_upsample(x.to(DEV), m.to(DEV), 8, x_mul, mask_mul).cpu()
    assert same_nan_pattern(got, ref)
    ok = ~np.isnan(ref)
    assert worst_ratio(got.numpy()[ok], ref[ok], bound[ok]) <= 1.0


def test_convex_upsample_rejections():
    x9, m9 = torch.zeros((1, 9, 2, 2), device=DEV), torch.zeros((1, 576, 2, 2), device=DEV)
    with pytest.raises(_lib.ScflowHipError):                        # C = 9: 72 KiB of LDS
        ops.convex_upsample(x9, m9)
    with pytest.raises(_lib.ScflowHipError):                        # scale != 8
        ops.convex_upsample(x9[:, :2].contiguous(), torch.zeros((1, 144, 2, 2), device=DEV), scale=4)


# ======================================================================================================== pose update
def _pose_check(regime, n, mode):
    case = pose_case(regime, n)
    d_rot, d_trans, (rv, re), (tv, te) = pose_update_ref(*case, mode)
    dev = [t.to(DEV) for t in case]
    got = [t.cpu() for t in ops.pose_update(dev[0], dev[1], dev[2], NUM_CLASS, dev[3], dev[4], mode)]
    assert same_bits(got[0], d_rot) and same_bits(got[1], d_trans), 'class select is not bit-exact'
    ok = np.isfinite(re).all((1, 2))                                # a || b, a = 0: no bound on R'
    if regime not in ('zero_a', 'parallel'):
        assert ok.all()
        dev_i = np.abs(f64(got[2]) @ f64(got[2]).transpose(0, 2, 1) - np.eye(3))
        assert (dev_i <= orthonormality_bound(rv, re)).all(), 'R\' R\'^T - I outside the bound'
    assert torch.isfinite(got[2]).all() and torch.isfinite(got[3]).all()
    return worst_ratio(got[2], rv, re), worst_ratio(got[3], tv, te)


@pytest.mark.parametrize('mode', [0, 1, 2, 3])
@pytest.mark.parametrize('n', POSE_N)
def test_pose_update_sizes_and_label_modes(n, mode):
    rr, rt = _pose_check('nominal', n, mode)
    measured(f'pose_update N {n} mode {mode}, error / bound (R\', t\')', max(rr, rt))
    assert rr <= 1.0 and rt <= 1.0


@pytest.mark.parametrize('regime', POSE_REGIMES[1:])
def test_pose_update_regimes(regime):
    for mode in (1, 3):
        rr, rt = _pose_check(regime, 3, mode)
        measured(f'pose_update {regime} mode {mode}, error / bound (R\', t\')', max(rr, rt))
        assert rr <= 1.0 and rt <= 1.0


def test_pose_update_rejects_label_mode_4():
    dev = [t.to(DEV) for t in pose_case('nominal', 3)]
    with pytest.raises(_lib.ScflowHipError):
        ops.pose_update(dev[0], dev[1], dev[2], NUM_CLASS, dev[3], dev[4], 4)


# ==================================================================================== re-projection and un-projection
@pytest.mark.parametrize('size', GEOM_SIZES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('pose', GEOM_POSES)
def test_reproject_and_unproject(pose, size):
    skew = size[1] % 2 == 1
    for invalid in (0.0, 400.0):
        case = geom_case(pose, size, skew)
        dev = [t.to(DEV) for t in case]
        ref, bound, left = reproject_ref(*case, invalid)
        fg = f64(case[0]) > 0
        check_left_out(left, fg)
        buf, out = guarded((size[0], 2, *size[1:]))
        ops.reproject_flow(*dev, invalid_num=invalid, out=out)
        assert guard_untouched(buf, (size[0], 2, *size[1:]))
        got = out.cpu().numpy()
        keep = ~left[:, None].repeat(2, 1)
        worst = worst_ratio(got[keep], ref[keep], bound[keep])      # background: bound 0, exactly invalid_num
        measured(f'reproject_flow {pose} {size} invalid {invalid}, error / bound', worst)
        assert worst <= 1.0
        if pose == 'through_camera' and size == (3, 12, 20):        # the case that exists to produce left-out pixels
            assert 0 < left.sum() < 8 and left[0, 1, :8].sum() == left.sum()
            assert np.isfinite(bound[keep]).all()
    pref, pbound = unproject_ref(*case[:4])
    worst = worst_ratio(ops.unproject_depth(*dev[:4]).cpu(), pref, pbound)
    measured(f'unproject_depth {pose} {size}, error / bound', worst)
    assert worst <= 1.0


# ================================================================================================ filter_flow_by_mask
@pytest.mark.parametrize('size', FILTER_SIZES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('kind', ['binary', 'smooth'])
@pytest.mark.parametrize('align_corners', [False, True])
def test_filter_flow_by_mask_decisions(align_corners, kind, size):
    """every vector whose decision is certain is bit-equal to the input flow or to invalid_num, as the restatement says --
    border and one-pixel-outside end points, invalid_num in one / both components, +-1e9 and the non-finite ones."""
    flow, mask = filter_case(kind, size)
    expect, certain = filter_ref(flow, mask, FILTER_INVALID, align_corners)
    share = check_left_out(~certain, np.ones_like(certain))
    got = ops.filter_flow_by_mask_(flow.to(DEV), mask.to(DEV), FILTER_INVALID, align_corners).cpu()
    measured(f'filter_flow_by_mask {size} {kind} ac {align_corners}, share inside 0.9 +- margin', share)
    assert filter_agrees(got, expect, certain)
    unc = torch.from_numpy(~certain)[:, None].expand_as(flow)       # an uncertain vector is still one of the two
    assert bool(((got[unc] == flow[unc]) | (got[unc] == FILTER_INVALID)).all())


def test_filter_flow_nonfinite_end_point_is_kept_like_grid_sample():
    """the divergence this file found first: a NaN, +-inf or overflowing component gives grid_sample a non-finite
    coordinate, the sampled mask is NaN and `NaN < 0.9` is false -- the reference KEEPS the vector (unless both
    components are >= invalid_num).  The kernel used to take its out-of-range path (sample 0) and overwrite it."""
    import oracle
    inf, nan = float('inf'), float('nan')
    vecs = [(nan, 0.0), (0.0, nan), (inf, 0.0), (0.0, inf), (-inf, 0.0), (0.0, -inf), (3e38, 0.0), (0.0, -3e38),
            (nan, nan), (inf, 500.0), (inf, inf), (1e9, 0.0), (0.0, -1e9)]
    for ac in (False, True):
        flow = torch.zeros((1, 2, 3, 5))
        for i, v in enumerate(vecs):
            flow[0, 0, i // 5, i % 5], flow[0, 1, i // 5, i % 5] = v
        mask = torch.ones((1, 3, 5))
        want = oracle.filter_flow_by_mask(flow, mask, FILTER_INVALID, align_corners=ac)
        got = ops.filter_flow_by_mask_(flow.to(DEV), mask.to(DEV), FILTER_INVALID, ac)
        assert same_bits(got, want)
        assert same_bits(want[0, :, 0, :4], flow[0, :, 0, :4])      # kept
        assert bool((want[0, :, 1, 4] == FILTER_INVALID).all())     # (inf, 500): both >= invalid_num
