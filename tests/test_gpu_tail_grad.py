"""GPU: tail_grad.hip (scf_resize_bilinear_grad, scf_reproject_flow_grad, scf_pose_tail_grad), SCFlowDecoder.tail_backward
and SCFlowRefiner.loss_and_head_grads against the float64 definition and the derived bounds of
tests/test_tail_grad_host.py.  Every comparison is `error <= bound` (ratio <= 1), bit equality, or -- for the degenerate
6-D rotations, where only the pattern is defined -- the same zeros and the same non-finite entries as float64 autograd.
The measured ratios are recorded in DESIGN.md section 4.5."""
import itertools
import json
import os

import numpy as np
import pytest
import torch

import scflow_amd
from scflow_amd import losses as L
from scflow_amd import ops
import test_loss_grad_host as HG
import test_loss_host as HL
import test_tail_grad_host as HT
from test_stream_ops_host import GEOM_SIZES, POSE_REGIMES, RESIZE_SIZES, f64, geom_case, measured, same_bits, worst_ratio

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def dev(x):
    return [dev(t) for t in x] if isinstance(x, (list, tuple)) else (None if x is None else x.to(DEV).contiguous())


def host(x):
    return x.detach().cpu().numpy()


def planes4(t):
    """(P, H, W) -> the (1, P, H, W) tensor the binding takes."""
    return t[None].contiguous()


# ====================================================================================================== resize adjoint
def _resize_variants(planes, in_hw, out_hw, off=0):
    """every calling form of one geometry: T = 1 / 3, one / two jobs, mul != 1, accumulate off / on -> worst ratio."""
    worst = 0.0
    for T, two, acc in itertools.product((1, 3), (False, True), (False, True)):
        gs = [HT.resize_grad_case(planes, out_hw, seed=10 * t) for t in range(T)]
        g2 = [HT.resize_grad_case(2, out_hw, seed=10 * t + 5) for t in range(T)]
        dst = [HT.resize_grad_case(planes, in_hw, seed=10 * t + 7) for t in range(T)]
        if off:                                                     # every source one float off 16-byte alignment
            buf = [torch.zeros((g.numel() + 4,), device=DEV) for g in gs]
            dg = [b[off:off + g.numel()].view(1, *g.shape).copy_(g[None]) for b, g in zip(buf, gs)]
            assert all(d.data_ptr() % 16 for d in dg)
        else:
            dg = [dev(planes4(g)) for g in gs]
        kw = dict(mul=-3.7)
        if acc:
            out = [dev(planes4(d)) for d in dst]
            kw.update(out=out, accumulate=True)
        if two:
            kw.update(second=([dev(planes4(g)) for g in g2], 0.125))
        got = ops.resize_bilinear_grad(dg, in_hw, **kw)
        got, got2 = got if two else (got, None)
        for t in range(T):
            ref, bound = HT.resize_grad_ref(gs[t], in_hw, -3.7, dst=dst[t] if acc else None)
            worst = max(worst, worst_ratio(host(got[t])[0], ref, bound))
            if two:
                ref, bound = HT.resize_grad_ref(g2[t], in_hw, 0.125)
                worst = max(worst, worst_ratio(host(got2[t])[0], ref, bound))
    return worst


@pytest.mark.parametrize('planes,in_hw,out_hw', RESIZE_SIZES)
def test_resize_adjoint_vs_float64(planes, in_hw, out_hw):
    r = _resize_variants(planes, in_hw, out_hw)
    measured(f'resize adjoint {in_hw} <- {out_hw}, {planes} planes', r)
    assert r <= 1.0


def test_resize_adjoint_misaligned_and_hot_route():
    r = _resize_variants(4, (3, 3), (5, 8), off=1)
    measured('resize adjoint (3, 3) <- (5, 8), sources one float off', r)
    assert r <= 1.0
    g = HT.resize_grad_case(6, (256, 256))
    got = ops.resize_bilinear_grad(dev(planes4(g)), (32, 32), mul=8.0)
    ref, bound = HT.resize_grad_ref(g, (32, 32), 8.0)
    r = worst_ratio(host(got)[0], ref, bound)
    measured('resize adjoint (32, 32) <- (256, 256), 6 planes, plane-walk route', r)
    assert r <= 1.0


@pytest.mark.parametrize('in_hw,out_hw', [((4, 4), (32, 32)), ((3, 5), (20, 24)), ((32, 32), (256, 256))])
def test_resize_adjoint_routes_and_replay_give_the_same_bits(in_hw, out_hw):
    """aligned sources take the plane-walk kernel, sources one float off the gather kernel: one summation order, so the
    same bits -- and the bits of the numpy replay of that order."""
    g = HT.resize_grad_case(3, out_hw, seed=3)
    a = ops.resize_bilinear_grad(dev(planes4(g)), in_hw, mul=8.0)
    buf = torch.zeros((g.numel() + 4,), device=DEV)
    off = buf[1:1 + g.numel()].view(1, *g.shape).copy_(g[None])
    b = ops.resize_bilinear_grad(off, in_hw, mul=8.0)
    assert same_bits(a, b)
    assert same_bits(a, torch.from_numpy(HT.resize_grad_fp32(g.numpy(), in_hw, 8.0))[None])


def test_resize_adjoint_exact_cases():
    g = HT.resize_grad_case(4, (8, 8), seed=1)
    got = ops.resize_bilinear_grad(dev(planes4(g)), (8, 8), mul=0.25)                 # identity: mul * g
    assert same_bits(got, (0.25 * g)[None])
    for in_hw, out_hw in (((5, 9), (9, 17)), ((1, 1), (3, 5))):                        # weights 0, 1/2, 1 on small integers
        g = HT.resize_grad_case(4, out_hw, seed=2, small_int=True)
        got = ops.resize_bilinear_grad(dev(planes4(g)), in_hw)
        ref, _ = HT.resize_grad_ref(g, in_hw)
        assert same_bits(got, torch.from_numpy(ref.astype(np.float32))[None])
    assert np.array_equal(ref[:, 0, 0], f64(g).sum((1, 2)))                            # (1, 1): the sum of the plane


@pytest.mark.parametrize('in_hw,out_hw', [((5, 9), (9, 17)), ((17, 25), (3, 4)), ((4, 4), (32, 32))])
def test_resize_adjoint_is_the_adjoint_of_the_forward_kernel(in_hw, out_hw):
    from test_stream_ops_host import resize_ref
    a, g = HT.resize_grad_case(4, in_hw, seed=4), HT.resize_grad_case(4, out_hw, seed=6)
    fwd = host(ops.resize_bilinear(dev(planes4(a)), out_hw, mul=2.0))[0].astype(np.float64)
    adj = host(ops.resize_bilinear_grad(dev(planes4(g)), in_hw, mul=2.0))[0].astype(np.float64)
    _, fb = resize_ref(a, out_hw, 2.0, coords='fp32')
    _, ab = HT.resize_grad_ref(g, in_hw, 2.0)
    room = (fb * np.abs(f64(g))).sum() + (ab * np.abs(f64(a))).sum()
    assert abs((fwd * f64(g)).sum() - (f64(a) * adj).sum()) <= room * (1 + 1e-9)


def test_resize_adjoint_is_deterministic_and_independent_of_t():
    gs = [dev(planes4(HT.resize_grad_case(6, (64, 64), seed=t))) for t in range(3)]
    ms = [dev(planes4(HT.resize_grad_case(3, (64, 64), seed=t + 50))) for t in range(3)]
    a, a2 = ops.resize_bilinear_grad(gs, (8, 8), mul=8.0, second=(ms, 1.0))
    b, b2 = ops.resize_bilinear_grad(gs, (8, 8), mul=8.0, second=(ms, 1.0))
    for t in range(3):
        one, one2 = ops.resize_bilinear_grad(gs[t], (8, 8), mul=8.0, second=(ms[t], 1.0))
        assert same_bits(a[t], b[t]) and same_bits(a2[t], b2[t]) and same_bits(a[t], one) and same_bits(a2[t], one2)
    ups = [dev(planes4(HT.resize_grad_case(2, (8, 8), seed=t))) for t in range(3)]       # the D^T direction (gather kernel)
    c = ops.resize_bilinear_grad(ups, (64, 64), mul=0.125)
    assert all(same_bits(c[t], ops.resize_bilinear_grad(ups[t], (64, 64), mul=0.125)) for t in range(3))


# ======================================================================================================= re-projection
def _reproject_sums(case_list, depth, k, rot0, trans0):
    """case_list: [(rot, trans, g | None)] per iteration -> (T, N, 12) float64, the tiles added in ascending order."""
    ws = ops.reproject_flow_grad([dev(c[2]) for c in case_list], dev(depth), dev(k), dev(rot0), dev(trans0),
                                 [dev(c[0]) for c in case_list], [dev(c[1]) for c in case_list])
    ws = host(ws)
    out = np.zeros(ws.shape[:2] + (12,))
    for tile in range(ws.shape[2]):
        out = out + ws[:, :, tile]
    return out


@pytest.mark.parametrize('T', [1, 3])
@pytest.mark.parametrize('skew', [True, False])
@pytest.mark.parametrize('pose', ['identity', 'large_rotation'])
@pytest.mark.parametrize('size', GEOM_SIZES)
def test_reprojection_sums_vs_float64(size, pose, skew, T):
    depth, k, rot0, trans0, rot, trans, g = HT.reproject_grad_case(pose, size, skew)
    if size[0] > 1:
        depth = depth.clone()
        depth[-1] = 0.0                                             # an all-background sample
    its = [(rot, trans, g)]
    if T == 3:
        _, _, _, _, rot2, trans2 = geom_case('large_rotation', size, skew, seed=3)
        its += [(rot2, trans2, None), (rot2, trans2, HT.reproject_grad_case(pose, size, skew, seed=9)[6])]      # a NULL cotangent
    got = _reproject_sums(its, depth, k, rot0, trans0)
    worst = 0.0
    for t, (r_, t_, g_) in enumerate(its):
        ref, bound = HT.reproject_grad_ref(depth, k, rot0, trans0, r_, t_, g_)
        assert np.isfinite(bound).all()                             # no sample is left out
        worst = max(worst, worst_ratio(got[t], ref, bound))
        if g_ is None:
            assert not got[t].any()
    if size[0] > 1:
        assert not got[:, -1].any()
    measured(f'reprojection sums {pose} {size} skew={skew} T={T}', worst)
    assert worst <= 1.0


def test_reprojection_sums_through_the_camera():
    case = HT.reproject_grad_case('through_camera', (3, 12, 20), True)
    got = _reproject_sums([(case[4], case[5], case[6])], *case[:4])[0]
    ref, bound = HT.reproject_grad_ref(*case)
    finite = np.isfinite(bound).all(1)
    assert finite.tolist() == [False, True, True]                   # the planted sample, and no other
    r = worst_ratio(got[finite], ref[finite], bound[finite])
    measured('reprojection sums through_camera (3, 12, 20), samples 1 and 2', r)
    assert r <= 1.0


# =========================================================================================================== pose scan
SUM_HW = (40, 40)       # 1600 pixels: two tiles of partial sums per (iteration, sample)


@pytest.mark.parametrize('T', [1, 4])
@pytest.mark.parametrize('n', [1, 5, 70])
@pytest.mark.parametrize('regime', POSE_REGIMES)
def test_pose_scan_vs_float64(regime, n, T):
    worst = 0.0
    for linear, with_sums in itertools.product((False, True), (False, True)):
        d_rots, d_transs, rot0, trans0, g_rot, g_trans = HT.scan_case(regime, n, T, with_sums=with_sums)
        rots, transs = HT.pose_forward64(d_rots, d_transs, rot0, trans0, linear)
        sums, total_r, total_t = None, g_rot.double().numpy(), g_trans.double().numpy()
        if with_sums:
            gen = torch.Generator().manual_seed(29000 + n + T)
            sums = torch.randn((T, n, 2, 12), generator=gen, dtype=torch.float64) * 20.0
            folded = (sums[:, :, 0] + sums[:, :, 1]).numpy()
            total_r, total_t = total_r + folded[..., :9].reshape(T, n, 3, 3), total_t + folded[..., 9:]
        for detach_pose, detach_depth in itertools.product((False, True), repeat=2):
            got_r, got_t = ops.pose_update_grad(dev(d_rots), dev(d_transs), dev(rot0), dev(trans0), dev(rots), dev(transs),
                                                g_rots=dev(list(g_rot)), g_transs=dev(list(g_trans)),
                                                reproject_sums=None if sums is None else sums.to(DEV), image_hw=SUM_HW,
                                                detach_pose=detach_pose, detach_depth_for_xy=detach_depth,
                                                label_mode=2 if linear else 0)
            got_r, got_t = np.stack([host(g) for g in got_r]), np.stack([host(g) for g in got_t])
            (rr, rb), (tr, tb) = HT.scan_ref(torch.stack(d_rots), torch.stack(d_transs), rot0, trans0, torch.stack(rots),
                                             torch.stack(transs), total_r, total_t, detach_pose, detach_depth, linear)
            if regime in ('zero_a', 'parallel'):                    # the pattern float64 autograd shows (host file)
                assert np.array_equal(np.isfinite(got_r), np.isfinite(rr)) and np.array_equal(got_r == 0, rr == 0)
            else:
                worst = max(worst, worst_ratio(got_r, rr, rb))
            worst = max(worst, worst_ratio(got_t, tr, tb))
    measured(f'pose scan {regime} N={n} T={T}', worst)
    assert worst <= 1.0


# ======================================================================================================= tail_backward
@pytest.fixture(scope='module')
def scflow_model(golden_dir):
    """the small random-weight refiner of tests/test_gpu_loss_grad.py, its pose loss a SequenceLoss over RAFTLoss so
    that every part of the tail (re-projection included) carries a gradient."""
    case = HL.refiner_loss_case()
    cfg = scflow_amd.scflow_model_cfg(iters=HL.REFINER_ITERS)
    cfg.update(HL.refiner_loss_cfgs(case))
    cfg['pose_loss_cfg'] = dict(type='SequenceLoss', gamma=0.7, loss_func_cfg=dict(type='RAFTLoss', loss_weight=0.3, max_flow=400.))
    m = scflow_amd.build_refiner(cfg)
    shapes = json.load(open(os.path.join(golden_dir, 'state_dict_keys.json')))['shapes']
    m.load_state_dict(scflow_amd.fill_state_dict(shapes, seed=0), strict=True)
    return m.to(DEV), case, cfg


class _Flags:
    """the decoder with other autograd switches for the duration of a block."""

    def __init__(self, decoder, flags, depth_transform):
        self.d, self.new = decoder, (*flags, depth_transform)

    def __enter__(self):
        d = self.d
        self.old = (d.detach_flow, d.detach_pose, d.detach_depth_for_xy, d.depth_transform)
        d.detach_flow, d.detach_pose, d.detach_depth_for_xy, d.depth_transform = self.new
        return d

    def __exit__(self, *exc):
        d = self.d
        d.detach_flow, d.detach_pose, d.detach_depth_for_xy, d.depth_transform = self.old


GRAD_KEYS = dict(flow_from_pose='sequence_flow_from_pose', flow_from_pred='sequence_flow_from_pred', rotation_preds='seq_rotations',
                 translation_preds='seq_translations', mask_preds='sequence_masks')


def _tail_backward(decoder, heads, consts, cots, poses, extra=None):
    outs = (None, None, dev(poses[0]), dev(poses[1]), None, dev(heads['delta_rotation_preds']), dev(heads['delta_translation_preds']))
    grads = {GRAD_KEYS[key]: dev(val) for key, val in cots.items()}
    got = decoder.tail_backward(outs, grads, dev(consts[0]), dev(consts[1]), dev(consts[2]), dev(consts[3]),
                                extra_flow_lr=None if extra is None else dev(extra))
    assert sorted(got) == sorted(HT.HEAD_KEYS)
    return {key: [host(g) for g in got[key]] for key in HT.HEAD_KEYS}


def _tail_ratio(got, ref, bound):
    return max(worst_ratio(g.reshape(r.shape), r, b) for key in HT.HEAD_KEYS for g, r, b in zip(got[key], ref[key], bound[key]))


@pytest.mark.parametrize('depth_transform', ['exp', 'linear'])
@pytest.mark.parametrize('tag,flags', [('shipped', (True, True, False)), ('free', (False, False, False))])
def test_tail_backward_on_the_golden_fixture(scflow_model, tag, flags, depth_transform):
    z = np.load(HT.GOLDEN)
    heads, consts, cots, _ = HT.tail_case()
    poses = ([torch.from_numpy(a) for a in z[f'{tag}_{depth_transform}_rot']],
             [torch.from_numpy(a) for a in z[f'{tag}_{depth_transform}_trans']])
    ref, bound = HT.tail_closed_form(heads, consts, cots, flags, depth_transform, poses, with_bounds=True)
    with _Flags(scflow_model[0].decoder, flags, depth_transform) as dec:
        got = _tail_backward(dec, heads, consts, cots, poses)
    r = _tail_ratio(got, ref, bound)
    measured(f'tail_backward, golden fixture, {tag} {depth_transform}', r)
    assert r <= 1.0


@pytest.mark.parametrize('depth_transform', ['exp', 'linear'])
@pytest.mark.parametrize('flags', HT.FLAG_COMBOS)
def test_tail_backward_random_sequences(scflow_model, flags, depth_transform):
    heads, consts, cots, extra = HT.tail_case(n=2, hw=(64, 64), T=3, seed=1)
    poses = HT.stored_poses(heads, consts, flags, depth_transform)
    ref, bound = HT.tail_closed_form(heads, consts, cots, flags, depth_transform, poses, with_bounds=True)
    with _Flags(scflow_model[0].decoder, flags, depth_transform) as dec:
        got = _tail_backward(dec, heads, consts, cots, poses)
        r = _tail_ratio(got, ref, bound)
        measured(f'tail_backward, 64 x 64, flags {flags} {depth_transform}', r)
        assert r <= 1.0
        if flags == (False, False, False):
            # extra_flow_lr: the result is the sum of this call's contributions and those of a call with the extra
            # cotangents alone (the tail is linear in its cotangents), inside the bounds of the two
            both = _tail_backward(dec, heads, consts, cots, poses, extra=extra)
            alone = _tail_backward(dec, heads, consts, {}, poses, extra=extra)
            ref2, bound2 = HT.tail_closed_form(heads, consts, {}, flags, depth_transform, poses, extra=extra, with_bounds=True)
            ref12, bound12 = HT.tail_closed_form(heads, consts, cots, flags, depth_transform, poses, extra=extra, with_bounds=True)
            assert _tail_ratio(alone, ref2, bound2) <= 1.0 and _tail_ratio(both, ref12, bound12) <= 1.0
            for key in HT.HEAD_KEYS:
                for a, b, c, b1, b2, b3 in zip(both[key], got[key], alone[key], bound12[key], bound[key], bound2[key]):
                    assert worst_ratio(a.reshape(b1.shape), (f64(b) + f64(c)).reshape(b1.shape), b1 + b2 + b3) <= 1.0


# ================================================================================================= loss_and_head_grads
def test_scflow_refiner_loss_and_head_grads(scflow_model, monkeypatch):
    from test_gpu_loss import TransferCount
    m, case, cfg = scflow_model
    data = HL.refiner_data(case, DEV)
    plain = m.loss(None, data=data)
    count = TransferCount(monkeypatch)
    loss, log_imgs, log_vars, seq_r, seq_t, grads = m.loss_and_head_grads(None, data=data)
    assert (count.helper, count.raw) == (1, 1)                      # still ONE device-to-host copy
    monkeypatch.undo()
    assert same_bits(loss, plain[0]) and list(log_vars.items()) == list(plain[2].items()) and log_imgs is None
    assert sorted(grads) == sorted(HT.HEAD_KEYS)
    base = m.loss_and_grads(None, data=data)[5]
    get = lambda: m.get_pose(data['rendered_images'], data['real_images'], data['ref_rotations'], data['ref_translations'],   # noqa: E731
                             data['rendered_depths'], data['internel_k'], data['labels'])
    outs = get()
    consts_dev = (data['ref_rotations'], data['ref_translations'], data['rendered_depths'].contiguous(), data['internel_k'].contiguous())
    again = m.decoder.tail_backward(outs, base, *consts_dev)
    for key in HT.HEAD_KEYS:
        assert all(same_bits(a, b) for a, b in zip(grads[key], again[key])), key
    # float64 autograd of loss restatement o tail restatement on the sequences the GPU produced
    T = len(outs[0])
    n, H, W = data['rendered_depths'].shape
    cpu = lambda seq: [s.detach().cpu() for s in seq]               # noqa: E731
    heads = {'delta_flow_preds': [torch.zeros((n, 2, H // 8, W // 8))] * T, 'masks': [torch.zeros((n, 1, H // 8, W // 8))] * T,
             'delta_rotation_preds': cpu(outs[5]), 'delta_translation_preds': cpu(outs[6])}
    consts = tuple(t.cpu() for t in consts_dev) + (torch.zeros((n, 2, H, W)), 0.0)
    stored = dict(zip(HT.COT_KEYS, (cpu(outs[0]), cpu(outs[1]), cpu(outs[2]), cpu(outs[3]), cpu(outs[4]))))
    d = m.decoder
    flags = (d.detach_flow, d.detach_pose, d.detach_depth_for_xy)
    leaves = {key: [t.double().clone().requires_grad_() for t in heads[key]] for key in HT.HEAD_KEYS}
    out = HT.tail_restatement(leaves['delta_flow_preds'], leaves['masks'], leaves['delta_rotation_preds'],
                              leaves['delta_translation_preds'], *consts, flags, d.depth_transform, stored=stored)
    gt_flow, valid = m._supervision(data, True).cpu(), data['rendered_masks'].cpu()
    seqs64 = [out['flow_from_pose'], out['flow_from_pred'], None, None, [s[:, 0] for s in out['mask_preds']]]
    HG.torch_wiring_total('scflow', seqs64, gt_flow, valid, cfg).backward()
    # the loss gradients in float64 at the same sequences: the cotangents of the exact chain
    fpose, fp, mk = ([s.detach().cpu().double().requires_grad_() for s in seq] for seq in (outs[0], outs[1], [s[:, 0] for s in outs[4]]))
    HG.torch_wiring_total('scflow', [fpose, fp, None, None, mk], gt_flow, valid, cfg).backward()
    exact = dict(flow_from_pose=[t.grad for t in fpose], flow_from_pred=[t.grad for t in fp], mask_preds=[t.grad[:, None] for t in mk])
    gpu = dict(flow_from_pose=cpu(base['sequence_flow_from_pose']), flow_from_pred=cpu(base['sequence_flow_from_pred']),
               mask_preds=cpu(base['sequence_masks']))
    poses = (cpu(outs[2]), cpu(outs[3]))
    ref, bound = HT.tail_closed_form(heads, consts, gpu, flags, d.depth_transform, poses, with_bounds=True)
    chain = HT.tail_closed_form(heads, consts, exact, flags, d.depth_transform, poses)
    worst = 0.0
    for key in HT.HEAD_KEYS:
        for i in range(T):
            auto = leaves[key][i].grad
            auto = np.zeros(chain[key][i].shape) if auto is None else auto.numpy().reshape(chain[key][i].shape)
            # the chain rule in float64: tail closed form of the exact loss gradients IS autograd of the composition
            assert np.abs(auto - chain[key][i]).max() <= 1e-12 * max(np.abs(auto).max(), 1e-300), key
            # composed bound: the tail's bound at the GPU's own cotangents + the tail (linear) applied to the loss
            # gradients' own error, which tests/test_gpu_loss_grad.py holds inside its bound
            room = bound[key][i] + np.abs(ref[key][i] - chain[key][i])
            worst = max(worst, worst_ratio(host(grads[key][i]).reshape(auto.shape), auto, room))
    measured('loss_and_head_grads against float64 autograd of loss o tail', worst)
    assert worst <= 1.0
    with pytest.raises(NotImplementedError, match='loss_and_head_grads'):
        m.forward(data, return_loss=True)
