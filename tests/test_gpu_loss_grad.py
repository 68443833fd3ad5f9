"""GPU: the value-and-gradient entries of loss.hip (scf_seq_pixel_loss_grad, scf_point_matching_loss_grad), the public
classes on top of them (value_and_grad, autograd) and the refiners' loss_and_grads() against the float64 restatements and
bounds of tests/test_loss_grad_host.py: the values bit for bit those of the forward entries, the decisions (zero and NaN
patterns) exactly, every gradient inside its derived bound, the exact cases bit for bit."""
import json
import os

import numpy as np
import pytest
import torch

import scflow_amd
from scflow_amd import _lib, losses as L

import test_loss_grad_host as HG
import test_loss_host as H
from test_loss_grad_host import grad_ratio
from test_loss_host import f32, measured

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SYM = [False, True]


def dev(x):
    if isinstance(x, (list, tuple)):
        return [dev(v) for v in x]
    return (torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x).to(DEV)


def host(x):
    return x.detach().cpu().numpy()


def bits(x):
    return host(x).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ================================================================================================== pixel kernel
WEIGHTS, EPS, GAMMAS = (.1, 2.5, 10.), (1e-10, 1e-6, 0.), (0.8, 0.5, 0.9)
UPSTREAM = (1.7, 0.25, 3.)


def pixel_args(case, use_valid=True, two=True, with_mask=True, weights=WEIGHTS, eps=EPS):
    return (dev(case['gt']), dev(case['valid']) if use_valid else None), dict(
        flow_a=dev(case['flow_a']), flow_b=dev(case['flow_b']) if two else None, masks=dev(case['masks']) if with_mask else None,
        max_flow=400., loss_weight=weights, eps=eps, gamma=GAMMAS)


def check_pixel(case, use_valid=True, two=True, with_mask=True, want=(True, True, True), upstream=None):
    """values == the forward entry's bits; gradients: run to run, the zero / NaN pattern of the restatement exactly, the
    coefficient inside its bound -> worst error / bound."""
    a, kw = pixel_args(case, use_valid, two, with_mask)
    fwd = L.seq_pixel_loss(*a, **kw)
    up = None if upstream is None else torch.tensor(upstream, device=DEV)
    got = L.seq_pixel_loss_grad(*a, **kw, upstream=up, want=want)
    assert same_bits(fwd[0], got[0]) and same_bits(fwd[1], got[1])
    again = L.seq_pixel_loss_grad(*a, **kw, upstream=up, want=want)
    ref = HG.pixel_grad_ref(case['gt'], case['valid'] if use_valid else None, flows=[case['flow_a']] + ([case['flow_b']] if two else []),
                            masks=case['masks'] if with_mask else None, weights=WEIGHTS, eps=EPS, gammas=GAMMAS,
                            upstream=upstream or (1., 1., 1.))
    rows = [0] + ([1] if two else []) + ([2] if with_mask else [])
    worst = 0.0
    for row, ref_row in zip(rows, ref['grads']):
        if not want[row]:
            assert got[2][row] is None
            continue
        for t, r in enumerate(ref_row):
            g = got[2][row][t]
            assert g.shape == case['masks' if row == 2 else 'flow_a'][t].shape and same_bits(g, again[2][row][t])
            assert np.array_equal(host(g) == 0, r.v == 0)                        # the decisions, exactly
            worst = max(worst, grad_ratio(host(g), r))
    for row in set(range(3)) - set(rows):
        assert got[2][row] is None
    return worst


@pytest.mark.parametrize('T', [1, 8, 33])
@pytest.mark.parametrize('shape', [(1, 1, 1), (2, 3, 5), (1, 65, 63), (2, 64, 64), (1, 17, 241)])
def test_pixel_grad_vs_float64(shape, T):
    case = H.pixel_case(shape, T, 'nominal', seed=1)
    worst = 0.0
    for variant in (dict(), dict(use_valid=False, upstream=UPSTREAM), dict(two=False), dict(with_mask=False, upstream=UPSTREAM),
                    dict(use_valid=False, two=False), dict(want=(True, False, True)), dict(want=(False, True, False)),
                    dict(want=(False, False, False))):
        worst = max(worst, check_pixel(case, **variant))
    measured(f'pixel gradients {shape} T={T}: worst error / bound', worst)
    assert worst <= 1.0


@pytest.mark.parametrize('shape', [(1, 65, 63), (2, 64, 64)])
@pytest.mark.parametrize('regime', ['boundary', 'valid_half', 'all_background', 'all_invalid'])
def test_pixel_grad_decisions(shape, regime):
    """the regimes of `pixel_case`: cells one ulp around max_flow (a contracted magnitude decides differently), valid == 0.5
    and its predecessor, an all-background and an all-invalid ground truth (count = 0, eps > 0: zeros).  The zero pattern
    of every gradient is `pixel_decisions`' v (times sgn), exactly."""
    case = H.pixel_case(shape, 3, regime, seed=2)
    v, _ = H.pixel_decisions(case['gt'], case['valid'], 400.)
    for t in range(3):                                                           # and cells with p == g: sgn(0) = 0
        case['flow_a'][t] = case['flow_a'][t].clone()
        case['flow_a'][t][0, :, 0, ::3] = case['gt'][0, :, 0, ::3]
        case['masks'][t][0, 0, 1::2] = 1.0
    worst = max(check_pixel(case), check_pixel(case, use_valid=False))
    a, kw = pixel_args(case)
    g = host(L.seq_pixel_loss_grad(*a, **kw)[2][0][1])
    assert not g[0, :, 0, ::3].any()
    if regime in ('all_background', 'all_invalid'):
        assert not v.any() and not g.any()
    measured(f'pixel gradients {regime} {shape}: worst error / bound', worst)
    assert worst <= 1.0


def test_pixel_grad_count_zero_and_nan():
    # count(v) = 0 with eps = 0: autograd's 0 * inf = NaN everywhere in that row; eps > 0 next to it: zeros
    case = H.pixel_case((2, 3, 5), 2, 'all_invalid', seed=3)
    a, kw = pixel_args(case, eps=(0., 1e-10, 0.))
    _, _, grads = L.seq_pixel_loss_grad(*a, **kw)
    assert all(np.isnan(host(g)).all() for g in grads[0]) and not any(host(g).any() for g in grads[1])
    assert all(np.isfinite(host(g)).all() and host(g).any() for g in grads[2])    # the mask gradient ignores valid
    # NaN in a prediction at an INVALID pixel: 0 * sgn(NaN) = NaN there, and only there; and at a valid one
    case = H.pixel_case((1, 8, 8), 2, 'nominal', seed=4)
    case['valid'][0, 0, 0] = 0.
    case['flow_a'][1][0, 0, 0, 0] = float('nan')
    case['valid'][0, 1, 1] = 1.
    case['gt'][0, :, 1, 1] = 1.
    case['flow_b'][0][0, 1, 1, 1] = float('nan')
    case['masks'][1][0, 2, 2] = float('nan')
    case['flow_a'][0][0, 0, 3, 3], case['flow_a'][0][0, 1, 3, 3] = float('inf'), float('-inf')
    case['valid'][0, 3, 3] = 1.
    case['gt'][0, :, 3, 3] = 2.
    assert check_pixel(case) <= 1.0                                               # grad_ratio demands equal NaN patterns
    a, kw = pixel_args(case)
    _, _, grads = L.seq_pixel_loss_grad(*a, **kw)
    ga, gb, gm = host(grads[0][1]), host(grads[1][0]), host(grads[2][1])
    assert np.isnan(ga[0, 0, 0, 0]) and np.isnan(ga).sum() == 1 and np.isnan(gb[0, 1, 1, 1]) and np.isnan(gb).sum() == 1
    assert np.isnan(gm[0, 2, 2]) and np.isnan(gm).sum() == 1
    g0 = host(grads[0][0])
    assert g0[0, 0, 3, 3] > 0 and g0[0, 1, 3, 3] == -g0[0, 0, 3, 3]               # +-inf: +-1


def test_pixel_grad_unaligned_views_take_the_scalar_route():
    """a gradient tensor whose storage is not 16-byte aligned is written by the dword stores, a prediction that is not is
    read by the dword loads: the same gradient bits either way, and values equal to the forward entry's on the same inputs."""
    case = H.pixel_case((2, 64, 64), 2, 'nominal', seed=5)
    a, kw = pixel_args(case)
    want = L.seq_pixel_loss_grad(*a, **kw)
    n = case['gt'].numel()
    buf = torch.full((n + 1,), float('nan'), device=DEV)
    ga = [buf[1:].view_as(case['gt']), torch.empty_like(a[0])]
    assert ga[0].data_ptr() % 16 != 0
    got = L.seq_pixel_loss_grad(*a, **kw, grad_out=(ga, None, None))
    assert got[2][0][0] is ga[0] and bool(torch.isnan(buf[0]))                    # written in place, nothing before it touched
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
    assert all(same_bits(x, y) for r in range(3) for x, y in zip(got[2][r], want[2][r]))
    pbuf = torch.zeros(n + 1, device=DEV)
    pbuf[1:] = kw['flow_a'][0].reshape(-1)
    kw2 = dict(kw, flow_a=[pbuf[1:].view_as(case['gt']), kw['flow_a'][1]])
    got = L.seq_pixel_loss_grad(*a, **kw2)
    fwd = L.seq_pixel_loss(*a, **kw2)
    assert same_bits(got[0], fwd[0]) and same_bits(got[1], fwd[1])
    assert all(same_bits(x, y) for r in range(3) for x, y in zip(got[2][r], want[2][r]))


# ================================================================================================== point matching
def pm_args(case, symmetric, mode, loss_type=2, flags=0, sdf=1., reduction='mean', weight=1., gamma=0.8):
    counts = [len(v) for v in case['verts']]
    verts = dev(np.concatenate(case['verts']).astype(np.float32))
    offsets = dev(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32))
    lab = dev(np.asarray(case['labels'], dtype=np.int32))
    return (verts, offsets, lab, lab, dev(np.asarray(symmetric, dtype=np.int32)), dev(np.asarray(case['diameter'], dtype=np.float32)),
            dev(case['seq_r']), dev(case['seq_t']), dev(case['gt_r']), dev(case['gt_t']), dev(case['scale']), max(counts), mode,
            loss_type, flags, sdf, reduction, weight, gamma)


def run_pm_grad(case, symmetric, mode, upstream=None, **opt):
    up = None if upstream is None else torch.tensor([upstream], device=DEV)
    return L.point_matching_loss_grad(*pm_args(case, symmetric, mode, **opt), return_nn=True, upstream=up)


def check_pm(case, symmetric, mode, upstream=None, **opt):
    """values and neighbours == the forward entry's bits; gradients run to run and inside the bound of the restatement
    at the returned neighbours -> (worst error / bound, undecided L1 components -- their swing is part of the bound)."""
    fwd = L.point_matching_loss(*pm_args(case, symmetric, mode, **opt), return_nn=True)
    got = run_pm_grad(case, symmetric, mode, upstream, **opt)
    assert all(same_bits(a, b) for a, b in zip(fwd[:3], got[:3])) and torch.equal(fwd[3], got[3])
    again = run_pm_grad(case, symmetric, mode, upstream, **opt)
    ref = HG.pm_grads_of(case, symmetric, mode, nn_idx=host(got[3]), upstream=1. if upstream is None else upstream,
                         **HG.pm_kwargs(opt))
    worst = 0.0
    for t in range(len(case['seq_r'])):
        assert same_bits(got[4][t], again[4][t])
        worst = max(worst, grad_ratio(host(got[4][t]), ref['grad_r'][t]))
        if mode != H.PM_ROT:
            assert same_bits(got[5][t], again[5][t])
            worst = max(worst, grad_ratio(host(got[5][t]), ref['grad_t'][t]))
    assert (got[5] is None) == (mode == H.PM_ROT)
    return worst, ref['undecided']


@pytest.mark.parametrize('mode', [H.PM_FULL, H.PM_DISENTANGLE, H.PM_ROT])
@pytest.mark.parametrize('T', [1, 3])
@pytest.mark.parametrize('counts', H.PM_GPU_COUNTS)
def test_point_matching_grad_vs_float64(counts, T, mode):
    seed, _ = HG.pm_grad_gpu_case(counts, T, mode)     # neighbours AND L1 signs decided under every scaling of the mode
    case = H.pm_case(list(counts), H.PM_GPU_LABELS, T, seed=seed)
    worst = 0.0
    for i, opt in enumerate(H.PM_VARIANTS[mode]):
        w, und = check_pm(case, SYM, mode, upstream=0.37 if i % 2 else None, **opt)
        assert und == 0
        worst = max(worst, w)
    measured(f'point-matching gradients V={counts} T={T} mode={mode}: worst error / bound', worst)
    assert worst <= 1.0


@pytest.mark.parametrize('mode', list(H.PM_LARGE_VARIANTS))
def test_point_matching_grad_beyond_one_tile(mode):
    """1023 and 1025 vertices: two blocks per sample whose gradient sums meet in the combine, two LDS chunks, a class
    whose second tile holds ONE point; at most 4 L1 components undecided, their swing in the bound."""
    seed, _ = HG.pm_grad_gpu_case((1023, 1025), 1, mode, True, 4)
    case = H.pm_case([1023, 1025], H.PM_GPU_LARGE_LABELS, 1, seed=seed, layout='lattice')
    worst = 0.0
    for opt in H.PM_LARGE_VARIANTS[mode]:
        w, und = check_pm(case, SYM, mode, **opt)
        assert und <= 4
        worst = max(worst, w)
    measured(f'point-matching gradients V=(1023, 1025) mode={mode}: worst error / bound', worst)
    assert worst <= 1.0


def test_point_matching_grad_33_iterations():
    """more iterations than one launch carries (32): the partial sums and the gradient pointers of the second chunk."""
    seed, _ = H.pm_gpu_case((64, 65), 33, H.PM_FULL)
    case = H.pm_case([64, 65], H.PM_GPU_LABELS, 33, seed=seed)
    worst, _ = check_pm(case, SYM, H.PM_FULL, loss_type=2)
    measured('point-matching gradients T=33: worst error / bound', worst)
    assert worst <= 1.0


def test_point_matching_grad_both_classes_symmetric():
    case = H.pm_case([257, 600], (0, 1, 1, 0), 1, seed=9)
    assert check_pm(case, [True, True], H.PM_FULL, loss_type=1)[0] <= 1.0
    assert check_pm(case, [True, False], H.PM_DISENTANGLE, loss_type=2, flags=H.PM_DISENTANGLE_Z)[0] <= 1.0


@pytest.mark.parametrize('kind', ['l1', 'l2'])
def test_point_matching_grad_exact_lattice_cases(kind):
    """every operation exact: the gradients ARE the float64 values (rounded once: unchanged), zeros for the sample whose
    pose equals the ground truth, and an upstream of 1/4 scales them exactly."""
    case = HG.pm_exact_case(kind)
    for mode, opt in HG.EXACT_VARIANTS[kind]:
        got = run_pm_grad(case, SYM, mode, **opt)
        quarter = run_pm_grad(case, SYM, mode, upstream=0.25, **opt)
        ref = HG.pm_grads_of(case, SYM, mode, **opt)
        for t in range(2):
            assert np.array_equal(host(got[4][t]), ref['grad_r'][t].v.astype(np.float32)) and not host(got[4][t])[3].any()
            assert np.array_equal(host(quarter[4][t]), f32(0.25) * host(got[4][t]))
            if mode != H.PM_ROT:
                assert np.array_equal(host(got[5][t]), ref['grad_t'][t].v.astype(np.float32)) and not host(got[5][t])[3].any()
                assert np.array_equal(host(quarter[5][t]), f32(0.25) * host(got[5][t]))
        assert np.isfinite(host(got[4][0])).all()


def test_point_matching_grad_out_of_range_label_is_nan_not_a_fault():
    case = H.pm_case([64, 65], (1, 0, 1), 1, seed=1)
    case['labels'] = np.array([1, 7, -1])
    got = run_pm_grad(case, SYM, H.PM_FULL)
    gr, gt = host(got[4][0]), host(got[5][0])
    assert np.isfinite(gr[0]).all() and gr[0].any() and np.isnan(gr[1:]).all()
    assert np.isfinite(gt[0]).all() and np.isnan(gt[1:]).all() and np.isnan(host(got[0])[0, 1:]).all()


# ================================================================================================== public classes
@pytest.fixture(scope='module')
def fix():
    d = np.load(HG.GOLDEN_FILE)
    px, pm = HG.grad_fixture_inputs()
    return d, px, pm


def leaves(seq):
    return [dev(np.asarray(t) if not isinstance(t, torch.Tensor) else t).requires_grad_() for t in seq]


def test_fixture_gradients_through_the_public_classes(fix):
    """loss_grads.npz (autograd on the reference's own classes) through LOSSES / build_loss, two ways: `.backward()` on
    GPU predictions that require a gradient, and `value_and_grad` -- the same bits; inside the kernel bound around the
    float64 restatement; within the two bounds of the reference's fp32 gradients (where a symmetric sample's neighbours
    are the recorded ones: a near tie of the fixture is decided by the summation order)."""
    d, px, pm = fix
    worst_k = worst_r = 0.0
    occ = HG.gt_occ_of(px)
    for i, opt in enumerate(H.PIXEL_OPTIONS):
        valid = dev(px['valid']) if opt['valid'] else None
        if opt['cls'] == 'RAFTLoss':
            f = scflow_amd.build_loss(dict(type='SequenceLoss', gamma=opt['gamma'], loss_func_cfg=dict(
                type='RAFTLoss', loss_weight=opt['loss_weight'], max_flow=opt['max_flow'])))
            preds, kw = leaves(px['flow_a']), dict(gt_flow=dev(px['gt']), valid=valid)
        else:
            f = scflow_amd.build_loss(dict(type='SequenceLoss', gamma=opt['gamma'],
                                           loss_func_cfg=dict(type='L1Loss', loss_weight=opt['loss_weight'])))
            preds, kw = leaves(px['masks']), dict(gt_mask=dev(occ), valid=valid)
        plain, _ = f([p.detach() for p in preds], **kw)
        total, lst = f(preds, **kw)
        assert total.requires_grad and not plain.requires_grad and not any(v.requires_grad for v in lst)
        total.backward()
        total2, lst2, (grads,) = f.value_and_grad(preds, **kw)
        assert not total2.requires_grad and float(total2) == float(total) == float(plain)
        assert [float(v) for v in lst] == [float(v) for v in lst2]
        assert all(same_bits(p.grad, g) for p, g in zip(preds, grads))
        ref, _ = HG.pixel_grad_ref_for(opt, px, occ)
        for t, r in enumerate(ref):
            worst_k = max(worst_k, grad_ratio(host(grads[t]), r))
            worst_r = max(worst_r, grad_ratio(d[f'pixel_{i}_grad'][t], HG.EV(host(grads[t]).astype(np.float64), 2 * r.e)))
        # one iteration alone: the value carries the graph
        one = leaves([px['flow_a'][1] if opt['cls'] == 'RAFTLoss' else px['masks'][1]])[0]
        single = f.loss_func(one, *(kw.values()))
        assert single.requires_grad
        single.backward()
        assert np.array_equal(one.grad.cpu().numpy() == 0, host(grads[1]) == 0)
    for i, opt in enumerate(H.PM_OPTIONS):
        cfg = {k: v for k, v in opt.items() if k != 'cls'}
        f = scflow_amd.build_loss(dict(type='SequenceLoss', gamma=0.8, loss_func_cfg=dict(
            type=opt['cls'], symmetry_types=H.FIX_SYMMETRY, mesh_diameter=pm['diameter'], mesh_path='no/such/dir', **cfg)))
        f.loss_func.meshes = [torch.from_numpy(v) for v in pm['verts']]
        lab, rot = dev(pm['labels']), opt['cls'] == 'RotPointMatchingLoss'
        sr, st = leaves(pm['seq_r']), leaves(pm['seq_t'])
        if rot:
            preds, kw = (sr,), dict(gt_r=dev(pm['gt_r']), labels=lab)
            nn = f.loss_func.sequence(dev(pm['seq_r']), None, kw['gt_r'], None, lab, return_nn=True)[3]
        else:
            preds, kw = (sr, st), dict(gt_r=dev(pm['gt_r']), gt_t=dev(pm['gt_t']), labels=lab, scale_factors=dev(pm['scale']))
            nn = f.loss_func.sequence(dev(pm['seq_r']), dev(pm['seq_t']), kw['gt_r'], kw['gt_t'], lab,
                                      scale_factors=kw['scale_factors'], return_nn=True)[3]
        total, lst = f(*preds, **kw)
        assert total.requires_grad and not any(v.requires_grad for v in lst)
        total.backward()
        total2, lst2, grads = f.value_and_grad(*preds, **kw)
        assert float(total2) == float(total) and [float(v) for v in lst] == [float(v) for v in lst2] and len(grads) == len(preds)
        assert all(same_bits(p.grad, g) for seq, gs in zip(preds, grads) for p, g in zip(seq, gs))
        nn = host(nn)
        ref = HG.pm_grad_ref_for(opt, pm, SYM, nn_idx=nn)
        wide = HG.pm_grad_ref_for(opt, pm, SYM, nn_idx=nn, torch_sums=True)
        same_nn = [[bool((nn[t, n] == d[f'pm_{i}_nn'][t, n]).all()) or not SYM[int(c)] for n, c in enumerate(pm['labels'])]
                   for t in range(4)]
        assert sum(map(sum, same_nn)) >= 11                                      # at most the one near tie of the fixture
        for key, gs in zip(('grad_r', 'grad_t'), grads):
            for t in range(4):
                worst_k = max(worst_k, grad_ratio(host(gs[t]), ref[key][t]))
                keep = np.asarray(same_nn[t])
                room = HG.EV(host(gs[t]).astype(np.float64)[keep], (ref[key][t].e + wide[key][t].e)[keep])
                worst_r = max(worst_r, grad_ratio(d[f'pm_{i}_{key}'][t][keep], room))
        assert not host(grads[0][3])[:2].any()                                    # pose == ground truth: zeros
    measured('public classes, gradients vs float64: worst error / kernel bound', worst_k)
    measured('public classes, gradients vs the reference: worst error / (kernel bound + reference bound)', worst_r)
    assert worst_k <= 1.0 and worst_r <= 1.0


def test_value_and_grad_refuses_other_classes_and_backward_scales():
    if 'HalfRAFTGrad' not in L.LOSSES:
        @L.LOSSES.register_module()
        class HalfRAFTGrad(L.RAFTLoss):
            def forward(self, pred_flow, gt_flow, valid=None):
                return 0.5 * super().forward(pred_flow, gt_flow, valid)
            __call__ = forward
    case = H.pixel_case((2, 3, 5), 3, 'nominal', seed=6)
    f = scflow_amd.build_loss(dict(type='SequenceLoss', gamma=0.8, loss_func_cfg=dict(type='HalfRAFTGrad', loss_weight=2.)))
    with pytest.raises(NotImplementedError, match='HalfRAFTGrad'):
        f.value_and_grad(dev(case['flow_a']), gt_flow=dev(case['gt']), valid=dev(case['valid']))
    # a grad_output other than 1 scales the gradients (2 is exact); without grad mode there is no graph
    g = scflow_amd.build_loss(dict(type='SequenceLoss', gamma=0.8, loss_func_cfg=dict(type='RAFTLoss', loss_weight=1.)))
    preds = leaves(case['flow_a'])
    kw = dict(gt_flow=dev(case['gt']), valid=dev(case['valid']))
    (2. * g(preds, **kw)[0]).backward()
    _, _, (grads,) = g.value_and_grad(preds, **kw)
    assert all(np.array_equal(host(p.grad), 2 * host(x)) for p, x in zip(preds, grads))
    with torch.no_grad():
        assert not g(preds, **kw)[0].requires_grad


# ================================================================================================== refiners
@pytest.fixture(scope='module')
def scflow_model(golden_dir):
    """the set-up of tests/test_gpu_loss.py::scflow_model, restated."""
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


def lead64(seq):
    return [s.detach().cpu().double().requires_grad_() for s in seq]


def compare_autograd(name, got, leaves64, bounds):
    """GPU gradients against float64 autograd: the closed forms with their bounds (`bounds`: EV per iteration) must BE
    autograd's (1e-12), and the GPU's lie inside -> worst error / bound."""
    worst = 0.0
    for g, leaf, b in zip(got, leaves64, bounds):
        want = leaf.grad.numpy().reshape(b.v.shape)
        assert np.abs(want - b.v).max() <= 1e-12 * max(np.abs(want).max(), 1e-300), name
        worst = max(worst, grad_ratio(host(g).reshape(b.v.shape), b))
    measured(f'{name}: worst error / bound', worst)
    return worst


def test_scflow_refiner_loss_and_grads(scflow_model, monkeypatch):
    from test_gpu_loss import TransferCount
    m, case, cfg = scflow_model
    data = H.refiner_data(case, DEV)
    plain = m.loss(None, data=data)
    count = TransferCount(monkeypatch)
    loss, log_imgs, log_vars, seq_r, seq_t, grads = m.loss_and_grads(None, data=data)
    assert (count.helper, count.raw) == (1, 1)                                    # still ONE device-to-host copy
    monkeypatch.undo()
    assert not plain[0].requires_grad and not loss.requires_grad and float(loss) == float(plain[0])
    assert list(log_vars.items()) == list(plain[2].items()) and log_imgs is None
    assert sorted(grads) == ['seq_rotations', 'seq_translations', 'sequence_flow_from_pred', 'sequence_masks']
    outs = m.get_pose(data['rendered_images'], data['real_images'], data['ref_rotations'], data['ref_translations'],
                      data['rendered_depths'], data['internel_k'], data['labels'])
    assert all(g.shape == o.shape for key, idx in (('sequence_flow_from_pred', 1), ('seq_rotations', 2), ('seq_translations', 3),
                                                   ('sequence_masks', 4)) for g, o in zip(grads[key], outs[idx]))
    gt_flow = m._supervision(data, True).cpu()
    valid = data['rendered_masks'].cpu()
    pl = m.pose_loss_func.loss_func
    nn = host(pl.sequence(outs[2], outs[3], data['gt_rotations'], data['gt_translations'], data['labels'],
                          scale_factors=data['scale_factors'], return_nn=True)[3])
    sym = [f'cls_{c + 1}' in case['symmetry_types'] for c in range(21)]
    nn_list = [[nn[t, n] if sym[case['labels'][n]] else None for n in range(H.REFINER_N)] for t in range(H.REFINER_ITERS)]
    fp, rr, tt, mk = lead64(outs[1]), lead64(outs[2]), lead64(outs[3]), lead64([s[:, 0] for s in outs[4]])
    pose = dict(verts=case['verts'], labels=case['labels'], diameter=case['diameter'], gt_r=case['gt_r'], gt_t=case['gt_t'],
                scale=case['scale'], nn=[[None if x is None else x[:len(case['verts'][case['labels'][n]])] for n, x in enumerate(row)]
                                         for row in nn_list])
    HG.torch_wiring_total('scflow', [None, fp, rr, tt, mk], gt_flow, valid, cfg, pose=pose).backward()
    lf, lm, lp = (cfg[k]['loss_func_cfg'] for k in ('flow_loss_cfg', 'mask_loss_cfg', 'pose_loss_cfg'))
    gam = lambda k: cfg[k].get('gamma', 0.8)
    cpu = lambda seq: [s.cpu() for s in seq]
    pref = HG.pixel_grad_ref(gt_flow, valid, flows=[cpu(outs[1])], masks=[s[:, 0].cpu() for s in outs[4]],
                             weights=(lf.get('loss_weight', 1.), 1, lm.get('loss_weight', 1.)), eps=(lf.get('eps', 1e-10),) * 2,
                             gammas=(gam('flow_loss_cfg'), 1, gam('mask_loss_cfg')))
    opt = dict(lp, cls=lp['type'])
    mref = HG.pm_grad_ref(case['verts'], case['labels'], sym, case['diameter'], cpu(outs[2]), cpu(outs[3]), case['gt_r'], case['gt_t'],
                          scale=case['scale'], mode=H.PM_MODES[lp['type']], loss_type=int(lp.get('loss_type', 'l2')[-1]),
                          flags=H.pm_flags(opt), sdf=lp.get('scale_depth_factor', 1.), reduction=lp.get('reduction', 'mean'),
                          weight=lp.get('loss_weight', 1.), gamma=gam('pose_loss_cfg'), nn_idx=nn)
    worst = max(compare_autograd('loss_and_grads, flow', grads['sequence_flow_from_pred'], fp, pref['grads'][0]),
                compare_autograd('loss_and_grads, mask', grads['sequence_masks'], mk, pref['grads'][1]),
                compare_autograd('loss_and_grads, rotations', grads['seq_rotations'], rr, mref['grad_r']),
                compare_autograd('loss_and_grads, translations', grads['seq_translations'], tt, mref['grad_t']))
    assert worst <= 1.0


def test_scflow_refiner_loss_and_grads_with_a_flow_pose_loss(scflow_model):
    """pose_loss_cfg over RAFTLoss: all three rows, values and gradients, from ONE fused launch."""
    m0, case, cfg = scflow_model
    cfg = dict(cfg, pose_loss_cfg=dict(type='SequenceLoss', gamma=0.7, loss_func_cfg=dict(type='RAFTLoss', loss_weight=0.3,
                                                                                          max_flow=400.)))
    m = scflow_amd.build_refiner(cfg)
    m.load_state_dict(m0.state_dict(), strict=True)
    m = m.to(DEV)
    data = H.refiner_data(case, DEV)
    plain = m.loss(None, data=data)
    calls = []
    real = L.seq_pixel_loss_grad
    L.seq_pixel_loss_grad = lambda *a, **k: calls.append(1) or real(*a, **k)
    try:
        loss, _, log_vars, _, _, grads = m.loss_and_grads(None, data=data)
    finally:
        L.seq_pixel_loss_grad = real
    assert len(calls) == 1 and float(loss) == float(plain[0]) and list(log_vars.items()) == list(plain[2].items())
    assert sorted(grads) == ['sequence_flow_from_pose', 'sequence_flow_from_pred', 'sequence_masks']
    outs = m.get_pose(data['rendered_images'], data['real_images'], data['ref_rotations'], data['ref_translations'],
                      data['rendered_depths'], data['internel_k'], data['labels'])
    gt_flow, valid = m._supervision(data, True).cpu(), data['rendered_masks'].cpu()
    fpose, fp, mk = lead64(outs[0]), lead64(outs[1]), lead64([s[:, 0] for s in outs[4]])
    HG.torch_wiring_total('scflow', [fpose, fp, None, None, mk], gt_flow, valid, cfg).backward()
    lf, lm = cfg['flow_loss_cfg']['loss_func_cfg'], cfg['mask_loss_cfg']['loss_func_cfg']
    cpu = lambda seq: [s.cpu() for s in seq]
    ref = HG.pixel_grad_ref(gt_flow, valid, flows=[cpu(outs[1]), cpu(outs[0])], masks=[s[:, 0].cpu() for s in outs[4]],
                            weights=(lf.get('loss_weight', 1.), 0.3, lm.get('loss_weight', 1.)), eps=(lf.get('eps', 1e-10), 1e-10),
                            gammas=(cfg['flow_loss_cfg'].get('gamma', 0.8), 0.7, cfg['mask_loss_cfg'].get('gamma', 0.8)))
    worst = max(compare_autograd('fused loss_and_grads, flow', grads['sequence_flow_from_pred'], fp, ref['grads'][0]),
                compare_autograd('fused loss_and_grads, pose flow', grads['sequence_flow_from_pose'], fpose, ref['grads'][1]),
                compare_autograd('fused loss_and_grads, mask', grads['sequence_masks'], mk, ref['grads'][2]))
    assert worst <= 1.0


@pytest.mark.parametrize('kind', ['RAFTRefinerFlowMask', 'RAFTRefinerFlow'])
def test_raft_refiner_loss_and_grads(kind):
    cfg = scflow_amd.raft_model_cfg(iters=2)
    cfg.update(scflow_amd.raft_loss_cfgs())
    if kind == 'RAFTRefinerFlow':
        cfg.update(type='RAFTRefinerFlow', decoder=dict(cfg['decoder'], type='RAFTDecoder'))
    m = scflow_amd.build_refiner(cfg)
    m.load_state_dict(scflow_amd.fill_state_dict({k: v.shape for k, v in m.state_dict().items()}, seed=9), strict=True)
    m = m.to(DEV)
    case = H.refiner_loss_case(input_seed=11)
    data = H.refiner_data(case, DEV)
    plain = m.loss(None, data=data)
    loss, log_imgs, log_vars, grads = m.loss_and_grads(None, data=data)
    assert not plain[0].requires_grad and float(loss) == float(plain[0]) and list(log_vars.items()) == list(plain[2].items())
    out = m.get_flow(data['rendered_images'], data['real_images'])
    gt_flow, valid = m._supervision(data, True).cpu(), data['rendered_masks'].cpu()
    cpu = lambda seq: [s.cpu() for s in seq]
    if kind == 'RAFTRefinerFlowMask':
        assert sorted(grads) == ['sequence_flow_from_pred', 'sequence_masks']
        fl, oc = lead64(out[0]), lead64([s[:, 0] for s in out[1]])
        HG.torch_wiring_total('flow_mask', [fl, oc], gt_flow, valid, cfg).backward()
        lf, lm = cfg['flow_loss_cfg']['loss_func_cfg'], cfg['occlusion_loss_cfg']['loss_func_cfg']
        ref = HG.pixel_grad_ref(gt_flow, valid, flows=[cpu(out[0])], masks=[s[:, 0].cpu() for s in out[1]],
                                weights=(lf.get('loss_weight', 1.), 1, lm.get('loss_weight', 1.)), eps=(lf.get('eps', 1e-10),) * 2,
                                gammas=(cfg['flow_loss_cfg'].get('gamma', 0.8), 1, cfg['occlusion_loss_cfg'].get('gamma', 0.8)))
        worst = max(compare_autograd(f'{kind}, flow', grads['sequence_flow_from_pred'], fl, ref['grads'][0]),
                    compare_autograd(f'{kind}, occlusion', grads['sequence_masks'], oc, ref['grads'][1]))
        assert all(g.shape == o.shape for g, o in zip(grads['sequence_masks'], out[1]))
    else:
        assert sorted(grads) == ['sequence_flow_from_pred']
        fl = lead64(out)
        HG.torch_wiring_total('flow', [fl], gt_flow, valid, dict(loss_cfg=cfg['flow_loss_cfg'])).backward()
        lf = cfg['flow_loss_cfg']['loss_func_cfg']
        ref = HG.pixel_grad_ref(gt_flow, valid, flows=[cpu(out)], max_flow=lf.get('max_flow', 400), weights=(lf.get('loss_weight', 1.), 1, 1),
                                eps=(lf.get('eps', 1e-10),) * 2, gammas=(cfg['flow_loss_cfg'].get('gamma', 0.8),) * 3)
        worst = compare_autograd(f'{kind}, flow', grads['sequence_flow_from_pred'], fl, ref['grads'][0])
    assert worst <= 1.0
    with pytest.raises(NotImplementedError, match='loss_and_grads'):
        m.forward(data, return_loss=True)
