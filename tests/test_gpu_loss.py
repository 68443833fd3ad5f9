"""GPU: the loss kernels (loss.hip), the public loss classes and the refiners' loss() against the float64 restatements
and bounds of tests/test_loss_host.py: error <= bound on every output, decisions and exact cases bit for bit."""
import json
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

import scflow_amd
from scflow_amd import _lib, losses as L
from scflow_amd.mesh import MeshRenderer, MeshStore

import test_loss_host as H
from test_loss_host import EV, U, f32, measured, ratio
from test_render_host import SHIPPED, colored_icosphere, intrinsics, look_at_pose

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def dev(x):
    if isinstance(x, (list, tuple)):
        return [dev(v) for v in x]
    return (torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x).to(DEV)


def host(x):
    return x.detach().cpu().numpy()


def bits(x):
    return host(x).view(np.uint32)


# ================================================================================================== pixel kernel
PIX_SHAPES = [(1, 1, 1), (2, 3, 5), (1, 8, 8), (2, 64, 64), (1, 65, 63), (1, 17, 241), (3, 60, 80)]
WEIGHTS, EPS, GAMMAS = (.1, 2.5, 10.), (1e-10, 1e-6, 0.), (0.8, 0.5, 0.9)


def run_pixel(case, use_valid=True, two=True, with_mask=True, max_flow=400.):
    return L.seq_pixel_loss(dev(case['gt']), dev(case['valid']) if use_valid else None, flow_a=dev(case['flow_a']),
                            flow_b=dev(case['flow_b']) if two else None, masks=dev(case['masks']) if with_mask else None,
                            max_flow=max_flow, loss_weight=WEIGHTS, eps=EPS, gamma=GAMMAS)


def ref_pixel(case, use_valid=True, two=True, with_mask=True, max_flow=400.):
    """pixel_ref takes weight / eps / gamma by the kernel's row: 0 and 1 for the flow sequences, 2 for the mask."""
    return H.pixel_ref(case['gt'], case['valid'] if use_valid else None, flows=[case['flow_a']] + ([case['flow_b']] if two else []),
                       masks=case['masks'] if with_mask else None, max_flow=max_flow, weights=WEIGHTS, eps=EPS, gammas=GAMMAS)


def check_pixel(case, **variant):
    per_iter, totals = run_pixel(case, **variant)
    again = run_pixel(case, **variant)
    assert np.array_equal(bits(per_iter), bits(again[0])) and np.array_equal(bits(totals), bits(again[1]))     # run to run
    ref = ref_pixel(case, **variant)
    rows = [0] + ([1] if variant.get('two', True) else []) + ([2] if variant.get('with_mask', True) else [])
    worst = 0.0
    got_i, got_t = host(per_iter), host(totals)
    for vals, total, row in zip(ref['per_iter'], ref['totals'], rows):
        for t, v in enumerate(vals):
            worst = max(worst, ratio(got_i[row, t], v))
        worst = max(worst, ratio(got_t[row], total))
        # the gamma total is the fp32 recombination of the RETURNED values, bit for bit
        assert f32(got_t[row]).view(np.uint32) == H.fp32_recombine(got_i[row], GAMMAS[row]).view(np.uint32)
    for row in set(range(3)) - set(rows):
        assert not got_i[row].any() and got_t[row] == 0
    return worst


@pytest.mark.parametrize('T', [1, 8, 12, 33])
@pytest.mark.parametrize('shape', PIX_SHAPES)
def test_pixel_kernel_vs_float64(shape, T):
    case = H.pixel_case(shape, T, 'nominal', seed=1)
    worst = 0.0
    for variant in (dict(), dict(use_valid=False), dict(two=False), dict(with_mask=False), dict(use_valid=False, two=False)):
        worst = max(worst, check_pixel(case, **variant))
    measured(f'pixel kernel {shape} T={T}: worst error / bound', worst)
    assert worst <= 1.0


@pytest.mark.parametrize('shape', [(1, 8, 8), (1, 65, 63), (2, 64, 64)])
@pytest.mark.parametrize('regime', ['boundary', 'valid_half', 'all_background'])
def test_pixel_kernel_decisions(shape, regime):
    """cells whose magnitude straddles max_flow by one ulp (a contracted evaluation decides differently), mag == max_flow,
    valid == 0.5 and its predecessor, the quirk cells (300, 200) and (-500, 100), a ground truth that is all background:
    one flipped decision moves a value by ~1 / count, far outside the bound."""
    case = H.pixel_case(shape, 3, regime, seed=2)
    v, occ = H.pixel_decisions(case['gt'], case['valid'], 400.)
    if regime == 'boundary':
        assert 0 < v.sum() < v.size and 0 < occ.sum() < occ.size
    worst = max(check_pixel(case), check_pixel(case, use_valid=False))
    measured(f'pixel kernel {regime} {shape}: worst error / bound', worst)
    assert worst <= 1.0


def test_pixel_kernel_all_invalid_is_zero_and_nan_propagates():
    case = H.pixel_case((2, 3, 5), 2, 'all_invalid', seed=3)
    per_iter, totals = run_pixel(case)
    got = host(per_iter)
    assert not got[:2].any() and not host(totals)[:2].any()                       # 0 / (0 + eps) = 0, not NaN
    assert np.isfinite(got[2]).all() and (got[2] > 0).all()                       # the mask loss ignores valid
    # NaN in a prediction at an INVALID pixel: valid[:, None] * loss = 0 * NaN = NaN, as in the reference
    case = H.pixel_case((1, 8, 8), 2, 'nominal', seed=4)
    case['valid'][0, 0, 0] = 0.
    case['flow_a'][1][0, 0, 0, 0] = float('nan')
    per_iter, totals = run_pixel(case)
    got = host(per_iter)
    assert np.isfinite(got[0, 0]) and np.isnan(got[0, 1]) and np.isnan(host(totals)[0])
    assert np.isfinite(got[1]).all() and np.isfinite(got[2]).all()
    # ... and at a valid one
    case = H.pixel_case((1, 8, 8), 2, 'nominal', seed=4)
    case['valid'][0, 1, 1] = 1.
    case['gt'][0, :, 1, 1] = 1.
    case['flow_b'][0][0, 1, 1, 1] = float('nan')
    got = host(run_pixel(case)[0])
    assert np.isnan(got[1, 0]) and np.isfinite(got[1, 1]) and np.isfinite(got[0]).all()


def test_pixel_kernel_unaligned_views_take_the_scalar_route():
    """a prediction whose storage is not 16-byte aligned (a view at an odd offset): same values as its aligned copy."""
    case = H.pixel_case((2, 64, 64), 2, 'nominal', seed=5)
    want = run_pixel(case)
    n = case['gt'].numel()
    buf = torch.zeros(n + 1, device=DEV)
    buf[1:] = dev(case['flow_a'][0]).reshape(-1)
    fa = [buf[1:].view_as(case['gt']), dev(case['flow_a'][1])]
    assert fa[0].data_ptr() % 16 != 0
    got = L.seq_pixel_loss(dev(case['gt']), dev(case['valid']), flow_a=fa, flow_b=dev(case['flow_b']), masks=dev(case['masks']),
                           loss_weight=WEIGHTS, eps=EPS, gamma=GAMMAS)
    ref = ref_pixel(case)
    assert max(ratio(host(got[0])[0, t], ref['per_iter'][0][t]) for t in range(2)) <= 1.0
    assert np.allclose(host(got[0]), host(want[0]), rtol=1e-6)


# ================================================================================================== point matching
SYM = [False, True]
PM_VARIANTS = H.PM_VARIANTS


def run_pm(case, symmetric, mode, loss_type=2, flags=0, sdf=1., reduction='mean', weight=1., gamma=0.8):
    counts = [len(v) for v in case['verts']]
    verts = dev(np.concatenate(case['verts']).astype(np.float32))
    offsets = dev(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32))
    lab = dev(np.asarray(case['labels'], dtype=np.int32))
    return L.point_matching_loss(verts, offsets, lab, lab, dev(np.asarray(symmetric, dtype=np.int32)),
                                 dev(np.asarray(case['diameter'], dtype=np.float32)), dev(case['seq_r']), dev(case['seq_t']),
                                 dev(case['gt_r']), dev(case['gt_t']), dev(case['scale']), max(counts), mode, loss_type, flags,
                                 sdf, reduction, weight, gamma, return_nn=True)


def check_pm(case, symmetric, mode, decided, **opt):
    loss_i, per_iter, total, nn_idx = run_pm(case, symmetric, mode, **opt)
    nn = host(nn_idx)
    kw = dict(mode=mode, loss_type=opt.get('loss_type', 2), flags=opt.get('flags', 0), sdf=opt.get('sdf', 1.),
              reduction=opt.get('reduction', 'mean'), weight=opt.get('weight', 1.), gamma=opt.get('gamma', 0.8))
    args = (case['verts'], case['labels'], symmetric, case['diameter'], case['seq_r'], case['seq_t'], case['gt_r'], case['gt_t'])
    free = H.pm_ref(*args, scale=case['scale'], want_d=True, **kw)                # the fp64 neighbours and distances
    T, N = len(case['seq_r']), len(case['labels'])
    for t in range(T):
        for n in range(N):
            V = len(case['verts'][int(case['labels'][n])])
            assert (nn[t, n, V:] == -1).all()
            D = free['dist'][t][n]
            if D is None:
                assert np.array_equal(nn[t, n, :V], np.arange(V))                 # a non-symmetric class keeps its own index
                continue
            r, best, got = np.arange(V), free['nn'][t][n], nn[t, n, :V]
            assert ((got >= 0) & (got < V)).all()
            # the returned neighbour is the nearest within the fp32 slack of the two distances compared ...
            assert (D.v[r, got] <= D.v[r, best] + D.e[r, got] + D.e[r, best]).all()
            if decided:                                                           # ... and THE nearest where the gaps decide it
                assert np.array_equal(got, best)
    ref = H.pm_ref(*args, scale=case['scale'], nn_idx=nn, **kw)                   # the value at the returned neighbours
    worst = max(ratio(host(loss_i)[t, n], ref['loss_i'][t][n]) for t in range(T) for n in range(N))
    worst = max([worst, ratio(host(total)[0], ref['total'])] + [ratio(host(per_iter)[t], ref['per_iter'][t]) for t in range(T)])
    assert f32(host(total)[0]).view(np.uint32) == H.fp32_recombine(host(per_iter), kw['gamma']).view(np.uint32)
    again = run_pm(case, symmetric, mode, **opt)
    assert all(np.array_equal(host(a).view(np.uint32), host(b).view(np.uint32)) for a, b in zip((loss_i, per_iter, total), again[:3]))
    assert np.array_equal(nn, host(again[3]))
    return worst


@pytest.mark.parametrize('mode', [H.PM_FULL, H.PM_DISENTANGLE, H.PM_ROT])
@pytest.mark.parametrize('T', [1, 3])
@pytest.mark.parametrize('counts', H.PM_GPU_COUNTS)
def test_point_matching_kernel_vs_float64(counts, T, mode):
    seed, _ = H.pm_gpu_case(counts, T, mode)         # gap-checked under every translation scaling of the mode's options
    case = H.pm_case(list(counts), H.PM_GPU_LABELS, T, seed=seed)
    worst = max(check_pm(case, SYM, mode, True, **opt) for opt in PM_VARIANTS[mode])
    measured(f'point matching V={counts} T={T} mode={mode}: worst error / bound', worst)
    assert worst <= 1.0


@pytest.mark.parametrize('counts,mode', [(c, m) for c in H.PM_GPU_LARGE for m in H.PM_LARGE_VARIANTS])
def test_point_matching_kernel_beyond_one_tile(counts, mode):
    """vertex sets of more than 1024 points: several blocks per sample and several LDS chunks per block, neighbours in
    every chunk, a smaller class in the same batch whose later tiles return early, the sum over tiles in the combine."""
    seed, _ = H.pm_gpu_case(counts, 1, mode, True)
    case = H.pm_case(list(counts), H.PM_GPU_LARGE_LABELS, 1, seed=seed, layout='lattice')
    worst = max(check_pm(case, SYM, mode, True, **opt) for opt in H.PM_LARGE_VARIANTS[mode])
    measured(f'point matching V={counts} mode={mode}: worst error / bound', worst)
    assert worst <= 1.0


def test_point_matching_kernel_33_iterations():
    """more iterations than one launch carries (32): the second launch writes at its own offset."""
    seed, _ = H.pm_gpu_case((64, 65), 33, H.PM_FULL)
    case = H.pm_case([64, 65], H.PM_GPU_LABELS, 33, seed=seed)
    worst = check_pm(case, SYM, H.PM_FULL, True, loss_type=2)
    measured('point matching T=33: worst error / bound', worst)
    assert worst <= 1.0


def test_point_matching_both_classes_symmetric_and_swapped():
    case = H.pm_case([257, 600], (0, 1, 1, 0), 1, seed=9)
    assert check_pm(case, [True, True], H.PM_FULL, False, loss_type=1) <= 1.0
    assert check_pm(case, [True, False], H.PM_DISENTANGLE, False, loss_type=2, flags=H.PM_DISENTANGLE_Z) <= 1.0


def _lattice():
    r = np.arange(-2, 3)
    return np.stack(np.meshgrid(r, r, r, indexing='ij'), -1).reshape(-1, 3).astype(np.float32)         # 125 points


RZ = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], dtype=np.float32)
RX = np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0]], dtype=np.float32)


def test_point_matching_exact_lattice_cases():
    """integer lattice vertices, rotations with 0 / +-1 entries, integer translations: every operation is exact.  The
    predicted pose differs from the ground truth by a symmetry of the lattice."""
    P = _lattice()
    gt_r = np.stack([RZ, RX @ RZ])
    S = [RX, RZ @ RZ]                                                             # lattice symmetries
    pred_r = np.stack([gt_r[0] @ S[0], gt_r[1] @ S[1]]).astype(np.float32)
    gt_t = np.array([[3, -4, 700], [0, 9, 650]], dtype=np.float32)
    case = dict(verts=[P], labels=np.array([0, 0]), gt_r=gt_r, gt_t=gt_t, seq_r=[pred_r], seq_t=[gt_t.copy()],
                scale=np.ones(2, np.float32), diameter=[64.0])
    for lt in (1, 2):
        loss_i, per_iter, total, nn = run_pm(case, [True], H.PM_FULL, loss_type=lt)
        assert not host(loss_i).any() and host(total)[0] == 0                     # flagged symmetric: exactly 0
        for n in range(2):                                                        # and the neighbour is THE matching vertex
            want = [int(np.nonzero((P == (S[n].T @ p)).all(1))[0][0]) for p in P]
            assert host(nn)[0, n].tolist() == want
    # without the flag: mean_p |S p - p|_1 / 64, summed in integers
    loss_i, per_iter, total, _ = run_pm(case, [False], H.PM_FULL, loss_type=1, reduction='sum', weight=2.)
    hand = [f32(f32(f32(np.abs(P @ s.T - P).sum()) / f32(125)) / f32(64)) for s in S]
    assert host(loss_i)[0].tolist() == [float(h) for h in hand]
    assert host(per_iter)[0] == f32(f32(2.) * f32(hand[0] + hand[1])) and host(total)[0] == host(per_iter)[0]
    # a shifted prediction: the 25 targets of one face find their neighbour at distance 1, all others at 0
    case['seq_t'] = [gt_t + gt_r[:, :, 0]]                                        # R_gt (1, 0, 0): a shift along the model's x
    case['seq_r'] = [gt_r.copy()]
    loss_i, _, _, nn = run_pm(case, [True], H.PM_FULL, loss_type=2)
    want = f32(f32(f32(25.) / f32(125.)) / f32(64.))
    assert host(loss_i)[0].tolist() == [float(want)] * 2
    # duplicated vertices: the lowest index wins, the value is unchanged
    case['verts'] = [np.concatenate([P, P])]
    loss_d, _, _, nn_d = run_pm(case, [True], H.PM_FULL, loss_type=2)
    assert host(loss_d)[0].tolist() == [float(want)] * 2
    assert (host(nn_d)[0] < 125).all() and np.array_equal(host(nn_d)[0][:, :125], host(nn)[0][:, :125])
    assert np.array_equal(host(nn_d)[0][:, 125:], host(nn_d)[0][:, :125])


def test_point_matching_duplicated_lattice_across_chunks():
    """11^3 = 1331 lattice points, twice: 2662 predicted points in three LDS chunks, 2662 targets in three tiles.  Every
    target's exact neighbour exists at index j and at j + 1331 -- in different chunks for most j: the lower one wins."""
    r = np.arange(-5, 6)
    P = np.stack(np.meshgrid(r, r, r, indexing='ij'), -1).reshape(-1, 3).astype(np.float32)
    gt_r = np.stack([RZ, RX @ RZ])
    gt_t = np.array([[3, -4, 700], [0, 9, 650]], dtype=np.float32)
    case = dict(verts=[np.concatenate([P, P])], labels=np.array([0, 0]), gt_r=gt_r, gt_t=gt_t, seq_r=[gt_r.copy()],
                seq_t=[gt_t + gt_r[:, :, 0]], scale=np.ones(2, np.float32), diameter=[64.0])
    loss_i, _, _, nn = run_pm(case, [True], H.PM_FULL, loss_type=2)
    nn = host(nn)[0]
    # predicted vertex q sits at R (q + e_x) + t: target p finds q = p - e_x at distance 0, or, on the face x = -5, q = p at 1
    want = np.array([int(np.nonzero((P == (p - [1, 0, 0] if p[0] > -5 else p)).all(1))[0][0]) for p in P])
    assert np.array_equal(nn[:, :1331], np.stack([want, want])) and np.array_equal(nn[:, 1331:], nn[:, :1331])
    assert (nn < 1331).all() and (want >= 1024).any()
    hand = f32(f32(f32(242.) / f32(2662.)) / f32(64.))                           # 2 x 121 face points at distance 1
    assert host(loss_i)[0].tolist() == [float(hand)] * 2


def test_point_matching_out_of_range_label_is_nan_not_a_fault():
    case = H.pm_case([64, 65], (1, 0, 1), 1, seed=1)
    case['labels'] = np.array([1, 7, -1])
    loss_i, per_iter, _, _ = run_pm(case, SYM, H.PM_FULL)
    got = host(loss_i)[0]
    assert np.isfinite(got[0]) and np.isnan(got[1]) and np.isnan(got[2]) and np.isnan(host(per_iter)[0])


# ================================================================================================== public classes
@pytest.fixture(scope='module')
def fix():
    d = np.load(os.path.join(H.GOLDEN, 'losses.npz'))
    return d


def test_fixture_values_through_the_public_classes(fix):
    """losses.npz (the reference's own classes) through LOSSES / build_loss: the reference's fp32 value lies within the
    kernel bound plus torch's summation term around the float64 restatement (host test), the kernel's within the kernel
    bound; so they differ by at most the sum of the two."""
    d = fix
    px = dict(gt=torch.from_numpy(d['gt']), valid=torch.from_numpy(d['valid']), flow_a=list(torch.from_numpy(d['flow_a'])),
              flow_b=list(torch.from_numpy(d['flow_b'])), masks=list(torch.from_numpy(d['masks'])))
    pm = dict(verts=[d['verts0'], d['verts1']], labels=d['labels'], gt_r=d['gt_r'], gt_t=d['gt_t'], seq_r=list(d['seq_r']),
              seq_t=list(d['seq_t']), scale=d['scale'], diameter=[float(x) for x in d['diameter']])
    worst_k = worst_r = 0.0

    def compare(total, lst, ref_iter, ref_total, wide_iter, wide_total, key):
        nonlocal worst_k, worst_r
        assert total.dim() == 0 and total.is_cuda and all(v.dim() == 0 for v in lst)
        for t in range(3):
            worst_k = max(worst_k, ratio(float(lst[t]), ref_iter[t]))
            worst_r = max(worst_r, abs(float(lst[t]) - float(d[f'{key}_list'][t])) / float(ref_iter[t].e + wide_iter[t].e))
        worst_k = max(worst_k, ratio(float(total), ref_total))
        worst_r = max(worst_r, abs(float(total) - float(d[f'{key}_total'])) / float(ref_total.e + wide_total.e))

    for i, opt in enumerate(H.PIXEL_OPTIONS):
        valid = dev(px['valid']) if opt['valid'] else None
        if opt['cls'] == 'RAFTLoss':
            f = scflow_amd.build_loss(dict(type='SequenceLoss', gamma=opt['gamma'], loss_func_cfg=dict(
                type='RAFTLoss', loss_weight=opt['loss_weight'], max_flow=opt['max_flow'])))
            total, lst = f(dev(px['flow_a']), gt_flow=dev(px['gt']), valid=valid)
            single = f.loss_func(dev(px['flow_a'][1]), dev(px['gt']), valid)
        else:
            f = scflow_amd.build_loss(dict(type='SequenceLoss', gamma=opt['gamma'],
                                           loss_func_cfg=dict(type='L1Loss', loss_weight=opt['loss_weight'])))
            total, lst = f(dev(px['masks']), gt_mask=dev(d['gt_occ']), valid=valid)
            single = f.loss_func(dev(px['masks'][1]), dev(d['gt_occ']), valid)
        assert float(single) == float(lst[1])                                     # one iteration alone: the same bits
        compare(total, lst, *H.pixel_ref_for(opt, px), *H.pixel_ref_for(opt, px, torch_sums=True), f'pixel_{i}')
    for i, opt in enumerate(H.PM_OPTIONS):
        cfg = {k: v for k, v in opt.items() if k != 'cls'}
        f = scflow_amd.build_loss(dict(type='SequenceLoss', gamma=0.8, loss_func_cfg=dict(
            type=opt['cls'], symmetry_types=H.FIX_SYMMETRY, mesh_diameter=pm['diameter'], mesh_path='no/such/dir', **cfg)))
        f.loss_func.meshes = [torch.from_numpy(v) for v in pm['verts']]
        lab = dev(pm['labels'])
        if opt['cls'] == 'RotPointMatchingLoss':
            total, lst = f(dev(pm['seq_r']), gt_r=dev(pm['gt_r']), labels=lab)
            single = f.loss_func(dev(pm['seq_r'][2]), dev(pm['gt_r']), lab)
        else:
            total, lst = f(dev(pm['seq_r']), dev(pm['seq_t']), gt_r=dev(pm['gt_r']), gt_t=dev(pm['gt_t']), labels=lab,
                           scale_factors=dev(pm['scale']))
            single = f.loss_func(dev(pm['seq_r'][2]), dev(pm['seq_t'][2]), dev(pm['gt_r']), dev(pm['gt_t']), lab,
                                 scale_factors=dev(pm['scale']))
        assert float(single) == float(lst[2])
        ref, wide = H.pm_ref_for(opt, pm, SYM), H.pm_ref_for(opt, pm, SYM, torch_sums=True)
        compare(total, lst, ref['per_iter'], ref['total'], wide['per_iter'], wide['total'], f'pm_{i}')
    measured('public classes vs float64: worst error / kernel bound', worst_k)
    measured('public classes vs the reference values: worst error / (kernel bound + reference bound)', worst_r)
    assert worst_k <= 1.0 and worst_r <= 1.0


def test_sequence_loss_generic_loop_and_perspective_points():
    """a class registered in LOSSES that is none of the built ones takes the reference's per-iteration loop;
    use_perspective_shape takes per-sample point lists."""
    if 'HalfRAFT' not in L.LOSSES:
        @L.LOSSES.register_module()
        class HalfRAFT(L.RAFTLoss):
            def forward(self, pred_flow, gt_flow, valid=None):
                return 0.5 * super().forward(pred_flow, gt_flow, valid)
            __call__ = forward
    case = H.pixel_case((2, 3, 5), 3, 'nominal', seed=6)
    f = scflow_amd.build_loss(dict(type='SequenceLoss', gamma=0.8, loss_func_cfg=dict(type='HalfRAFT', loss_weight=2.)))
    g = scflow_amd.build_loss(dict(type='SequenceLoss', gamma=0.8, loss_func_cfg=dict(type='RAFTLoss', loss_weight=1.)))
    total, lst = f(dev(case['flow_a']), gt_flow=dev(case['gt']), valid=dev(case['valid']))
    want_total, want = g(dev(case['flow_a']), gt_flow=dev(case['gt']), valid=dev(case['valid']))
    assert [float(v) for v in lst] == [float(v) for v in want]                    # 0.5 * 2 w = w: exact
    assert float(total) == float(want_total)
    pm = H.pm_case([65, 300], (1, 0, 1), 2, seed=3)
    a = scflow_amd.PointMatchingLoss(H.FIX_SYMMETRY, pm['diameter'], use_perspective_shape=True, loss_type='l1')
    b = scflow_amd.PointMatchingLoss(H.FIX_SYMMETRY, pm['diameter'], loss_type='l1')
    b.meshes = [torch.from_numpy(v) for v in pm['verts']]
    args = (dev(pm['seq_r'][0]), dev(pm['seq_t'][0]), dev(pm['gt_r']), dev(pm['gt_t']), dev(pm['labels']))
    assert float(a(*args, points_list=[dev(pm['verts'][c]) for c in (1, 0, 1)])) == float(b(*args))


# ================================================================================================== refiners
GPU_TOL = dict(flow_from_pose=1e-3, flow_from_pred=1e-3, rotation=6e-7, translation=1e-3, mask=6e-6)   # stated 1e-3 px; the
# rotation / translation / mask figures are the tolerances of test_gpu_refiner.py::test_full_refiner_golden


class TransferCount:
    """device-to-host transfers: calls of losses.to_host, and of Tensor.cpu / item / tolist / numpy / float() / int() /
    bool() on GPU tensors and of Tensor.to with a CPU result."""

    def __init__(self, monkeypatch):
        self.helper, self.raw = 0, 0
        real = L.to_host

        def to_host(vec):
            self.helper += 1
            return real(vec)
        monkeypatch.setattr(L, 'to_host', to_host)
        for name in ('cpu', 'item', 'tolist', 'numpy', '__float__', '__int__', '__bool__'):
            orig = getattr(torch.Tensor, name)

            def wrapped(t, *a, _orig=orig, **k):
                self.raw += int(t.is_cuda)
                return _orig(t, *a, **k)
            monkeypatch.setattr(torch.Tensor, name, wrapped)
        to = torch.Tensor.to

        def to_wrapped(t, *a, **k):
            out = to(t, *a, **k)
            self.raw += int(t.is_cuda and not out.is_cuda)                        # .to('cpu'), .to(a CPU tensor)
            return out
        monkeypatch.setattr(torch.Tensor, 'to', to_wrapped)


@pytest.fixture(scope='module')
def scflow_model(golden_dir):
    case = H.refiner_loss_case()
    cfg = scflow_amd.scflow_model_cfg(iters=H.REFINER_ITERS)
    cfg.update(H.refiner_loss_cfgs(case))
    m = scflow_amd.build_refiner(cfg)
    shapes = json.load(open(os.path.join(golden_dir, 'state_dict_keys.json')))['shapes']
    m.load_state_dict(scflow_amd.fill_state_dict(shapes, seed=0), strict=True)
    m = m.to(DEV)
    m._build_loss_funcs()
    m.pose_loss_func.loss_func.meshes = [torch.from_numpy(v) for v in case['verts']]
    return m, case, cfg


def test_scflow_refiner_loss(scflow_model, golden_dir, monkeypatch):
    m, case, cfg = scflow_model
    data = H.refiner_data(case, DEV)
    m.loss(None, data=data)                                                       # first use: mesh tables, constants
    count = TransferCount(monkeypatch)
    loss, log_imgs, log_vars, seq_r, seq_t = m.loss(None, data=data)
    assert (count.helper, count.raw) == (1, 1)                                    # ONE device-to-host copy
    monkeypatch.undo()
    assert log_imgs is None and loss.dim() == 0 and loss.is_cuda and not loss.requires_grad
    assert len(seq_r) == len(seq_t) == H.REFINER_ITERS
    g = np.load(os.path.join(golden_dir, 'refiner_loss.npz'))
    keys = [str(k) for k in g['keys']]
    assert isinstance(log_vars, OrderedDict) and list(log_vars) == keys           # the reference's keys, in its order
    assert float(loss) == log_vars['loss']
    # 1. wiring: the model's OWN sequences through the float64 restatement, inside the kernel bounds
    outs = m.get_pose(data['rendered_images'], data['real_images'], data['ref_rotations'], data['ref_translations'],
                      data['rendered_depths'], data['internel_k'], data['labels'])
    assert all(torch.equal(a, b) for a, b in zip(outs[2], seq_r))                 # get_pose is deterministic
    gt_flow = m._supervision(data, True)
    pl = m.pose_loss_func.loss_func
    _, _, _, nn = pl.sequence(outs[2], outs[3], data['gt_rotations'], data['gt_translations'], data['labels'],
                              scale_factors=data['scale_factors'], return_nn=True)
    sym = [f'cls_{c + 1}' in case['symmetry_types'] for c in range(21)]
    sd_, mn_ = torch.std_mean(case['init_add_error'], unbiased=False)
    cpu = lambda seq: [s.cpu() for s in seq]
    log = H.wiring_ref('scflow', [cpu(outs[0]), cpu(outs[1]), cpu(outs[2]), cpu(outs[3]), [s[:, 0].cpu() for s in outs[4]]],
                       gt_flow.cpu(), data['rendered_masks'].cpu(), cfg,
                       pose=dict(verts=case['verts'], labels=case['labels'], symmetric=sym, diameter=case['diameter'],
                                 gt_r=case['gt_r'], gt_t=case['gt_t'], scale=case['scale'], nn_idx=host(nn)),
                       init=(EV(float(mn_)), EV(float(sd_))))
    assert list(log) == keys
    worst = max(ratio(log_vars[k], log[k]) for k in keys)
    measured('SCFlowRefiner.loss vs float64 wiring on its own sequences: worst error / bound', worst)
    assert worst <= 1.0
    # 2. against the reference's log_vars within the network tolerance propagated to each value
    worst = 0.0
    for k, want in zip(keys, g['values']):
        room = H.propagated_tolerance(k, cfg, GPU_TOL, case) + 2 * float(log[k].e)
        r = abs(log_vars[k] - float(want)) / room if room else float(log_vars[k] != float(want))
        worst = max(worst, r)
        assert r <= 1.0, (k, log_vars[k], float(want), room)
    measured('SCFlowRefiner.loss vs the reference log_vars: worst error / propagated tolerance', worst)


def test_scflow_refiner_loss_with_a_flow_pose_loss(scflow_model):
    """pose_loss_cfg over RAFTLoss (scflow_refiner.py:222-225): all three losses in one fused launch."""
    m0, case, cfg = scflow_model
    cfg = dict(cfg, pose_loss_cfg=dict(type='SequenceLoss', gamma=0.7, loss_func_cfg=dict(type='RAFTLoss', loss_weight=0.3,
                                                                                          max_flow=400.)))
    m = scflow_amd.build_refiner(cfg)
    m.load_state_dict(m0.state_dict(), strict=True)
    m = m.to(DEV)
    data = H.refiner_data(case, DEV)
    loss, _, log_vars, _, _ = m.loss(None, data=data)
    outs = m.get_pose(data['rendered_images'], data['real_images'], data['ref_rotations'], data['ref_translations'],
                      data['rendered_depths'], data['internel_k'], data['labels'])
    cpu = lambda seq: [s.cpu() for s in seq]
    sd_, mn_ = torch.std_mean(case['init_add_error'], unbiased=False)
    log = H.wiring_ref('scflow', [cpu(outs[0]), cpu(outs[1]), None, None, [s[:, 0].cpu() for s in outs[4]]],
                       m._supervision(data, True).cpu(), data['rendered_masks'].cpu(), cfg,
                       init=(EV(float(mn_)), EV(float(sd_))))
    assert list(log_vars) == list(log)
    assert max(ratio(log_vars[k], log[k]) for k in log) <= 1.0


@pytest.mark.parametrize('kind', ['RAFTRefinerFlowMask', 'RAFTRefinerFlow'])
def test_raft_refiner_loss(kind):
    cfg = scflow_amd.raft_model_cfg(iters=2)
    cfg.update(scflow_amd.raft_loss_cfgs())
    if kind == 'RAFTRefinerFlow':
        cfg.update(type='RAFTRefinerFlow', decoder=dict(cfg['decoder'], type='RAFTDecoder'))
    m = scflow_amd.build_refiner(cfg)
    m.load_state_dict(scflow_amd.fill_state_dict({k: v.shape for k, v in m.state_dict().items()}, seed=9), strict=True)
    m = m.to(DEV)
    case = H.refiner_loss_case(input_seed=11)
    data = H.refiner_data(case, DEV)
    loss, log_imgs, log_vars = m.loss(None, data=data)
    assert log_imgs is None and loss.dim() == 0 and float(loss) == log_vars['loss']
    out = m.get_flow(data['rendered_images'], data['real_images'])
    gt_flow = m._supervision(data, True).cpu()
    cpu = lambda seq: [s.cpu() for s in seq]
    if kind == 'RAFTRefinerFlowMask':
        log = H.wiring_ref('flow_mask', [cpu(out[0]), [s[:, 0].cpu() for s in out[1]]], gt_flow, data['rendered_masks'].cpu(), cfg)
        assert list(log_vars) == ['seq_0_flow_loss', 'seq_0_occ_loss', 'seq_1_flow_loss', 'seq_1_occ_loss', 'loss_occ',
                                  'loss_flow', 'loss']
    else:
        log = H.wiring_ref('flow', [cpu(out)], gt_flow, data['rendered_masks'].cpu(), dict(loss_cfg=cfg['flow_loss_cfg']))
        assert list(log_vars) == ['seq_0_loss', 'seq_1_loss', 'loss']
    assert list(log_vars) == list(log)
    worst = max(ratio(log_vars[k], log[k]) for k in log)
    measured(f'{kind}.loss vs float64 wiring: worst error / bound', worst)
    assert worst <= 1.0


def test_loss_end_to_end_with_a_renderer():
    """loss(data_batch) on an attached MeshRenderer (icosphere classes) runs and equals loss(None, data=
    format_data_train_sup(data_batch)) bit for bit."""
    Hh = W = 256
    store = MeshStore({0: colored_icosphere(3, 60.0), 1: colored_icosphere(2, 70.0)})
    renderer = MeshRenderer(store, (Hh, W), **SHIPPED)
    g = np.random.default_rng(5)
    n = 3
    poses = [look_at_pose(*g.uniform(-0.4, 0.4, 3), g.uniform(450, 550), *g.uniform(-10, 10, 2)) for _ in range(n)]
    R = torch.tensor(np.stack([p[0] for p in poses]), device=DEV)
    t = torch.tensor(np.stack([p[1] for p in poses]), device=DEV)
    Rg = torch.tensor(np.stack([H.rand_rot(np.random.RandomState(i), 0.05) for i in range(n)]), device=DEV) @ R
    tg = t + torch.tensor([[2., -3., 10.]], device=DEV)
    K = torch.tensor(np.stack([intrinsics(320.0, Hh, W)] * n), device=DEV)
    labels = torch.tensor([0, 1, 0], device=DEV)
    real = torch.rand((n, 3, Hh, W), generator=torch.Generator().manual_seed(3)).to(DEV)
    norm = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375])
    sp = lambda x: [x[:2], x[2:]]
    batch = dict(img=sp(real), annots=dict(ref_rotations=sp(R), ref_translations=sp(t), gt_rotations=sp(Rg), gt_translations=sp(tg),
                                           labels=sp(labels), k=sp(K), gt_masks=sp(torch.ones((n, Hh, W), device=DEV)),
                                           init_add_error=torch.tensor([11., 7., 23.], device=DEV),
                                           init_rot_error=torch.tensor([1., 2., 3.], device=DEV),
                                           init_trans_error=torch.tensor([4., 5., 6.], device=DEV)),
                 img_metas=[dict(img_norm_cfg=norm, scale_factor=np.full((2, 4), 1.25, np.float32)),
                            dict(img_norm_cfg=norm, scale_factor=np.full((1, 4), 0.8, np.float32))])
    cfg = scflow_amd.scflow_model_cfg(iters=2)
    cfg.update(scflow_amd.scflow_loss_cfgs())
    cfg['pose_loss_cfg']['loss_func_cfg'].update(symmetry_types={'cls_2': {}}, scale_xy=True)
    m = scflow_amd.build_refiner(cfg)
    shapes = json.load(open(os.path.join(H.GOLDEN, 'state_dict_keys.json')))['shapes']
    m.load_state_dict(scflow_amd.fill_state_dict(shapes, seed=0), strict=True)
    m = m.to(DEV).attach_renderer(renderer)
    m._build_loss_funcs()
    m.pose_loss_func.loss_func.meshes = store                                    # the renderer's MeshStore serves the loss too
    loss, _, log_vars, _, _ = m.loss(batch)
    data = m.format_data_train_sup(batch)
    assert float(data['init_add_error_mean']) == pytest.approx(41 / 3, rel=1e-6) and 'init_trans_error_std' in data
    loss2, _, log_vars2, _, _ = m.loss(batch, data=data)
    assert np.isfinite(float(loss)) and float(loss) > 0
    assert list(log_vars.items()) == list(log_vars2.items()) and float(loss) == float(loss2)
    assert list(log_vars)[:2] == ['init_add_mean', 'init_add_std'] and log_vars['seq_1_pose_loss'] > 0


# ================================================================================================== refusals
def test_refusals(scflow_model):
    m, case, _ = scflow_model
    opaque = scflow_amd.build_refiner(scflow_amd.scflow_model_cfg(iters=2)).to(DEV)
    with pytest.raises(ValueError, match='loss_func_cfg'):
        opaque.loss(None, data=H.refiner_data(case, DEV))
    with pytest.raises(_lib.ScflowHipError):
        m.loss(None, data=H.refiner_data(case, 'cpu'))
    px = H.pixel_case((1, 8, 8), 1, 'nominal')
    with pytest.raises(_lib.ScflowHipError):
        scflow_amd.RAFTLoss()(px['flow_a'][0], px['gt'])
    with pytest.raises(_lib.ScflowHipError):
        scflow_amd.L1Loss()(px['masks'][0], px['masks'][0])
    pm = H.pm_case([5, 6], (0, 1), 1)
    f = scflow_amd.PointMatchingLoss({}, pm['diameter'])
    f.meshes = [torch.from_numpy(v) for v in pm['verts']]
    with pytest.raises(_lib.ScflowHipError):
        f(*[torch.from_numpy(np.asarray(pm[k][0] if k.startswith('seq') else pm[k])) for k in ('seq_r', 'seq_t', 'gt_r', 'gt_t', 'labels')])
    with pytest.raises(NotImplementedError):
        m.forward(H.refiner_data(case, DEV), return_loss=True)
    m.render_augmentations = [dict(type='RandomGaussianBlur')]
    try:
        with pytest.raises(NotImplementedError, match='render_augmentations'):
            m.loss(dict(img=[], annots={}, img_metas=[]))
    finally:
        m.render_augmentations = None
    r = scflow_amd.raft_model_cfg(iters=2)
    r.update(scflow_amd.raft_loss_cfgs(), filter_invalid_flow_by_depth=True)
    with pytest.raises(NotImplementedError, match='filter_invalid_flow_by_depth'):
        scflow_amd.build_refiner(r).loss(None, data=H.refiner_data(case, DEV))
