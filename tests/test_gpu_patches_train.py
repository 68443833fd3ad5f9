"""GPU: the train patch pipeline (scflow_amd/csrc/patch_train.hip) against the restatement of test_patches_train_host.py --
the jitter within 4 fp32 ulp with equal decisions, the draws, crop rectangles, patches and masks bit for bit on both
routes, the noise up to the transcendental part of its normal draw -- batch invariance, and the whole front end:
TrainPatchPipeline -> format_data_train_sup -> SCFlowRefiner.loss."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import scflow_amd
from scflow_amd import ops
from scflow_amd.mesh import MeshRenderer, MeshStore
from scflow_amd.patches import TrainPatchPipeline

from test_patches_host import _cfg, box_reference, crop_edges
from test_patches_train_host import (_aug, draws_reference, jitter_reference, noise_reference, patch_train_reference)
from test_render_host import SHIPPED as RENDER_SHIPPED, colored_icosphere, look_at_pose

pytestmark = pytest.mark.gpu
DEV = 'cuda'
HF, WF = 96, 128
EDGE_MARGIN = 1e-2          # px between a float64 crop edge and the integers, against the fp32 box (test_gpu_patches.py)

# class 1 is empty; class 0 spans several reduction chunks of the jitter's ADD sum (642 vertices, 256 threads)
MESHES = {0: colored_icosphere(3, 30.0), 2: colored_icosphere(1, 18.0), 3: colored_icosphere(2, 24.0)}
VERTS = {l: m.verts for l, m in MESHES.items()}
DIAM = [60.0, 1.0, 36.0, 48.0]
K0 = np.array([[600., 0, WF / 2 + 0.37], [0, 588., HF / 2 - 0.21], [0, 0, 1]], np.float32)
SIZES = [((32, 32), 32), ((17, 23), 17)]       # 17 x 23: the odd-width scalar stores


def dev(a, dt=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(DEV)


def _params(cfg):
    return ops.patch_params(cfg['size'], cfg['img_scale'], **{k: v for k, v in cfg.items() if k not in ('size', 'img_scale')})


def _pick_ids(aug, wants):
    """sample ids whose draws are what each entry of ``wants`` asks: dict(k=..., a/b/c = +1 (gain >= 1) or -1)."""
    d = draws_reference(aug, np.arange(1, 4000))
    ids, used = [], set()
    for w in wants:
        ok = np.ones(len(d['k']), bool)
        if 'k' in w:
            ok &= d['k'] == w['k']
        for g in 'abc':
            if g in w:
                ok &= (d[g] >= 1) == (w[g] > 0)
        pick = next(int(i) + 1 for i in np.flatnonzero(ok) if int(i) + 1 not in used)
        used.add(pick)
        ids.append(pick)
    return np.array(ids, np.int64)


@functools.lru_cache(maxsize=None)
def _scene():
    g = np.random.default_rng(21)
    frames = g.integers(0, 256, (2, HF, WF, 3), dtype=np.uint8)
    yy, xx = np.mgrid[:HF, :WF]
    return frames, yy, xx


def _masks(centres):
    _, yy, xx = _scene()
    return np.stack([(((xx - cx) ** 2 + (yy - cy) ** 2) < rad ** 2).astype(np.uint8) * (1 + 37 * i % 255)
                     for i, (cx, cy, rad) in enumerate(centres)])


# (name, label, z, x and y offset of the centre in frame widths / heights, expected valid)
CASES = [('inside', 0, 600.0, 0.0, 0.0, 1), ('partly_outside', 3, 420.0, 0.45, 0.1, 1), ('outside', 2, 500.0, 1.5, 0.2, 1),
         ('behind', 0, -500.0, 0.0, 0.0, 0), ('other_frame', 2, 260.0, -0.2, 0.15, 1)]


def _poses(cfg, ratios, seed):
    """poses for CASES, re-drawn until every float64 crop edge (at that object's drawn ratio) keeps EDGE_MARGIN from the
    integers, so that the fp32 box cannot move a truncation.  No case is dropped."""
    g = np.random.default_rng(seed)
    Rs, ts, labels = [], [], []
    for (name, label, z, ox, oy, want_valid), ratio in zip(CASES, ratios):
        for _ in range(1000):
            R, _t = look_at_pose(*g.uniform(-0.6, 0.6, 3), 1.0)
            zz = z * g.uniform(0.97, 1.03)
            t = np.array([(ox * WF + g.uniform(-4, 4)) * zz / 600.0, (oy * HF + g.uniform(-4, 4)) * zz / 588.0, zz], np.float32)
            box, ok = box_reference(VERTS[label], R, t, K0, cfg['vertex_stride'])
            assert ok == bool(want_valid), name
            if not ok:
                break
            e = crop_edges(box.astype(np.float32), (HF, WF), dict(cfg, size_ratio=float(ratio)), clip=False)
            if (np.abs(e - np.rint(e)) >= EDGE_MARGIN).all():
                break
        else:
            raise AssertionError(f'{name}: no draw kept its crop edges {EDGE_MARGIN} px from the integers')
        Rs.append(R)
        ts.append(t)
        labels.append(label)
    return np.stack(Rs), np.stack(ts), np.array(labels)


def _run(frames, frame_index, K, cfg, aug, ids, masks=None, labels=None, R=None, t=None, crop_rects=None, store=None):
    params, ap = _params(cfg), ops.patch_aug_params(**aug)
    sid = dev(ids, torch.int64)
    if crop_rects is None:
        box = ops.patch_boxes_train(store.on(DEV), dev(labels), dev(R), dev(t), dev(K), frames.shape[1:3], params, ap,
                                    sample_ids=sid)
    else:
        box = ops.patch_boxes_train(None, None, None, None, dev(K), frames.shape[1:3], params, ap, sample_ids=sid,
                                    crop_rects=dev(crop_rects))
    img, mask = ops.extract_patches_train(dev(frames), dev(frame_index, torch.int32), box['records'], params, ap,
                                          masks=None if masks is None else dev(masks))
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in box.items() if k != 'records'}
    out.update(img=img.cpu().numpy(), mask=None if mask is None else mask.cpu().numpy())
    return out


def _check_draws(got, want):
    d = want['draws']
    cols = [d['ratio'], d['a'].astype(np.float64), d['b'].astype(np.float64), d['c'].astype(np.float64), d['sigma'],
            d['k'].astype(np.float64), d['hsv_on'].astype(np.float64), d['noise_on'].astype(np.float64)]
    assert np.array_equal(got['draws'], np.stack(cols, 1))          # integers and uniforms: bit for bit


def _check_pixels(got, want, names):
    assert got['valid'].tolist() == want['valid'].tolist()
    for i, name in enumerate(names):
        assert got['crop'][i].tolist() == list(want['crop'][i]), name
        same = got['img'][i] == want['img'][i]
        assert same.all(), f'{name}: {int((~same).sum())} of {same.size} image values differ'
        if want.get('mask') is not None and len(want['mask']):
            same = got['mask'][i] == want['mask'][i]
            assert same.all(), f'{name}: {int((~same).sum())} of {same.size} mask values differ'


def _routes(want, k):
    out = []
    for (x1, y1, x2, y2), v, s, kk in zip(want['crop'], want['valid'], want['scale'], k):
        if v:
            pw, ph = x2 - x1 + 1, y2 - y1 + 1
            out.append(ops.patch_train_route(ph, pw, int(ph * s + 0.5), int(pw * s + 0.5), int(kk)))
    return out


# ====================================================================================================== jitter
def _ulps(got32, want64, floor=0.0):
    """|got - float32(want)| in float32 ulp of max(|want|, floor)."""
    want32 = want64.astype(np.float32)
    unit = np.spacing(np.maximum(np.abs(want32), np.float32(floor)).astype(np.float32)).astype(np.float64)
    return np.abs(got32.astype(np.float64) - want32.astype(np.float64)) / unit


@pytest.mark.parametrize('stride', [1, 3])
def test_pose_jitter_vs_reference(stride):
    """fp64 on both sides.  The device's sin / cos / log / sqrt / acos are within a few fp64 ulp (2.2e-16) of numpy's; the
    conditioning of everything computed here (acos at angles of degrees, a mean of norms) is below 1e3, so the two float64
    values differ by < 1e-12 relative, 2e-5 of an fp32 ulp: rounding once to fp32 gives the same number unless the pair
    straddles a rounding boundary (1 ulp).  4 ulp of the value itself is asserted.  A matrix entry is a sum of O(1) products
    and carries their absolute error (~1e-15): the argument holds for it while it is larger than 1e-6 in magnitude, which is
    asserted of the restatement's entries on the CPU side.  Decisions: every limit comparison of the restatement is asserted to be more than
    1e-9 (relative) from its limit, 1e3 times the error above, so ``tries`` and ``ok`` must be equal."""
    from scipy.spatial.transform import Rotation
    n = 7
    g = np.random.default_rng(3)
    R = Rotation.random(n, random_state=4).as_matrix().astype(np.float32)
    t = np.stack([g.uniform(-80, 80, n), g.uniform(-60, 60, n), g.uniform(300, 900, n)], 1).astype(np.float32)
    labels = np.array([0, 3, 2, 0, 3, 1, 9])                       # ..., an empty class, a label out of range
    aug = _aug(seed=11, angle_limit=20.0, translation_limit=60.0, add_limit=0.5)      # tight: several tries per object
    ids = np.array([3, 1000, 17, 2 ** 40 + 5, 8, 9, 10], np.int64)
    want = jitter_reference(R, t, labels, aug, ids, VERTS, DIAM, stride)
    assert want['ok'].tolist() == [1, 1, 1, 1, 1, 0, 0] and want['tries'][:5].max() > 1
    assert want['margin'][:5].min() > 1e-9, want['margin']
    assert np.abs(want['rot']).min() > 1e-6
    store = MeshStore(MESHES)
    got = ops.pose_jitter(store.on(DEV), dev(np.array(DIAM, np.float32)), dev(labels), dev(R), dev(t),
                          ops.patch_aug_params(**aug), vertex_stride=stride, sample_ids=dev(ids, torch.int64))
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in got.items()}
    assert got['ok'].tolist() == want['ok'].tolist() and got['tries'].tolist() == want['tries'].tolist()
    worst = dict(rot=_ulps(got['rot'], want['rot']).max(), trans=_ulps(got['trans'], want['trans']).max(),
                 add=_ulps(got['add_error'], want['add_error']).max(), rot_error=_ulps(got['rot_error'], want['rot_error']).max(),
                 trans_error=_ulps(got['trans_error'], want['trans_error']).max())
    print(f'pose jitter, stride {stride}: worst fp32 ulp {worst}, tries {got["tries"].tolist()}')
    assert max(worst.values()) <= 4
    # the failed objects: the gt pose bit for bit, zero errors
    assert np.array_equal(got['rot'][5:], R[5:]) and np.array_equal(got['trans'][5:], t[5:])
    assert (got['rot_error'][5:] == 0).all() and (got['add_error'][5:] == 0).all()
    # the swap quirk: fixed, the two error arrays change places
    fixed = ops.pose_jitter(store.on(DEV), dev(np.array(DIAM, np.float32)), dev(labels), dev(R), dev(t),
                            ops.patch_aug_params(**dict(aug, fix_error_swap_quirk=True)), vertex_stride=stride,
                            sample_ids=dev(ids, torch.int64))
    assert np.array_equal(fixed['rot_error'].cpu().numpy(), got['trans_error'])
    assert np.array_equal(fixed['trans_error'].cpu().numpy(), got['rot_error'])
    assert not np.array_equal(got['rot_error'][:5], got['trans_error'][:5])


def test_pose_jitter_impossible_limit_and_no_mesh():
    from scipy.spatial.transform import Rotation
    n = 3
    R = Rotation.random(n, random_state=1).as_matrix().astype(np.float32)
    t = np.array([[0, 0, 500.], [10, 20, 600.], [-5, 3, 700.]], np.float32)
    got = ops.pose_jitter(None, None, None, dev(R), dev(t),
                          ops.patch_aug_params(angle_limit=0.0, add_limit=None, max_tries=7), id_base=50)
    assert got['ok'].tolist() == [0, 0, 0] and got['tries'].tolist() == [7, 7, 7]
    assert torch.equal(got['rot'], dev(R)) and torch.equal(got['trans'], dev(t))
    assert (got['rot_error'] == 0).all() and (got['trans_error'] == 0).all() and (got['add_error'] == 0).all()
    # no mesh, no add_limit: accepted, add_error NaN; id_base + n is the sample id
    aug = _aug(add_limit=None, seed=2)
    free = ops.pose_jitter(None, None, None, dev(R), dev(t), ops.patch_aug_params(**aug), id_base=50)
    want = jitter_reference(R, t, None, aug, np.arange(50, 53))
    assert free['ok'].tolist() == [1, 1, 1] and bool(torch.isnan(free['add_error']).all())
    assert free['tries'].tolist() == want['tries'].tolist()
    assert np.abs(want['rot']).min() > 1e-6 and _ulps(free['rot'].cpu().numpy(), want['rot']).max() <= 4


# ===================================================================================================== extract
@pytest.mark.parametrize('size,scale', SIZES)
@pytest.mark.parametrize('hsv', [1.0, 0.0])
def test_extract_on_projected_boxes_vs_reference(size, scale, hsv):
    """noise off: image and mask bit for bit, k in {1, 3, 5}, gains on both sides of 1, objects partly and wholly outside
    the frame and behind the camera; the LDS route (asserted from the model)."""
    frames = _scene()[0]
    cfg = _cfg(size=size, img_scale=scale, vertex_stride=1 if hsv else 3, crop_pad_val=(10, 200, 90), pad_val=(5, 6, 7))
    aug = _aug(seed=6, noise_p=0.0, hsv_p=hsv, mask_pad_val=0 if hsv else 1)
    ids = _pick_ids(aug, [dict(k=5, a=1, b=-1, c=1), dict(k=3, a=-1, b=1, c=-1), dict(k=1), dict(k=5), dict(k=3, b=1, c=1)])
    draws = draws_reference(aug, ids)
    R, t, labels = _poses(cfg, draws['ratio'], seed=size[1] + int(hsv))
    K = np.stack([K0] * len(ids))
    frame_index = np.array([0, 0, 0, 0, 1])
    masks = _masks([(64, 48, 30), (118, 55, 28), (20, 20, 10), (64, 48, 5), (40, 62, 45)])
    want = patch_train_reference(frames, frame_index, K, cfg, aug, ids, masks=masks, meshes=VERTS, labels=labels, R=R, t=t)
    got = _run(frames, frame_index, K, cfg, aug, ids, masks=masks, labels=labels, R=R, t=t, store=MeshStore(MESHES))
    assert want['valid'].tolist() == [c[5] for c in CASES]
    _check_draws(got, want)
    _check_pixels(got, want, [c[0] for c in CASES])
    routes = _routes(want, draws['k'])
    print(f'routes at {size}: {routes}')
    # 32 x 32 from ~70 px crops: every object runs from LDS; 17 x 17 from the same crops is a 4-6 x down-scaling, whose
    # footprint at k = 5 does not fit: both routes in one launch
    assert set(routes) == ({'lds'} if scale == 32 else {'lds', 'direct'})
    # the cases are what they claim: the outside object's patch is all crop fill, its mask empty; the invalid one all pad
    fill = (np.asarray(cfg['crop_pad_val'][::-1], np.float32)) * np.float32(1 / 255.)
    if not hsv and scale == 32:
        assert (got['img'][2] == fill[:, None, None]).all()
    assert got['mask'][0].any() and not got['mask'][0].all()
    if not aug['mask_pad_val']:
        assert not got['mask'][2].any()
    assert (got['mask'][3] == bool(aug['mask_pad_val'])).all()
    assert (got['img'][3] == (np.asarray(cfg['pad_val'][::-1], np.float32) * np.float32(1 / 255.))[:, None, None]).all()


RECTS = np.array([[10, 12, 70, 60], [-8, 30, 40, 95], [100, -20, 131, 40], [60, 5, 60, 34], [5, 50, 34, 50],
                  [300, 300, 340, 350], [20, 20, 51, 51], [9, 9, 3, 12]], np.int32)
RECT_NAMES = ['inside', 'left_edge', 'top_right', 'one_pixel_wide', 'one_pixel_high', 'wholly_outside', 'one_to_one', 'empty']


@pytest.mark.parametrize('size,scale', SIZES)
def test_extract_on_caller_rectangles_vs_reference(size, scale):
    frames = _scene()[0]
    cfg = _cfg(size=size, img_scale=scale, to_rgb=False, mean=(123.675, 116.28, 103.53), std=(58.395, 57.12, 57.375),
               center=scale == 32)
    aug = _aug(seed=8, noise_p=0.0)
    ids = _pick_ids(aug, [dict(k=5), dict(k=3, c=1), dict(k=1, b=1), dict(k=5, a=1), dict(k=5, c=-1), dict(k=3), dict(k=3, a=-1),
                          dict(k=1)])
    n = len(RECTS)
    K = np.stack([K0] * n)
    frame_index = np.arange(n) % 2
    masks = _masks([(40 + 5 * i, 40, 25) for i in range(n)])
    want = patch_train_reference(frames, frame_index, K, cfg, aug, ids, masks=masks, crop_rects=RECTS)
    got = _run(frames, frame_index, K, cfg, aug, ids, masks=masks, crop_rects=RECTS)
    assert want['valid'].tolist() == [1, 1, 1, 1, 1, 1, 1, 0]
    _check_draws(got, want)
    _check_pixels(got, want, RECT_NAMES)
    routes = _routes(want, want['draws']['k'])
    print(f'routes at {size}: {routes}')
    assert set(routes) == {'lds'}


def test_wide_output_tiles_beyond_the_first_column():
    """80 x 80 outputs: two tile columns (64 + 16) and five tile rows, so the LDS route's column origin, the staging origin
    fx0 - r and the tile's destination range are exercised for tx > 0.  1:1, up-scaled and down-scaled, k in {1, 5}."""
    frames = _scene()[0]
    cfg = _cfg(size=(80, 80), img_scale=80)
    rects = np.array([[20, 10, 99, 89], [20, 10, 99, 89], [40, 30, 79, 59], [-8, -10, 135, 100], [-8, -10, 135, 100]], np.int32)
    n = len(rects)
    aug = _aug(seed=10, noise_p=0.0)
    ids = _pick_ids(aug, [dict(k=1), dict(k=5, c=1), dict(k=5, b=1), dict(k=5, a=-1), dict(k=1, c=-1)])
    masks = _masks([(60 + 3 * i, 50, 30) for i in range(n)])
    K = np.stack([K0] * n)
    want = patch_train_reference(frames, np.arange(n) % 2, K, cfg, aug, ids, masks=masks, crop_rects=rects)
    assert want['valid'].all() and want['draws']['k'].tolist() == [1, 5, 5, 5, 1]
    assert [int(80 * s + 0.5) for s in want['scale'][:2]] == [80, 80] and want['scale'][2] == 2.0 and want['scale'][3] < 0.6
    assert _routes(want, want['draws']['k']) == ['lds'] * n
    got = _run(frames, np.arange(n) % 2, K, cfg, aug, ids, masks=masks, crop_rects=rects)
    _check_draws(got, want)
    _check_pixels(got, want, ['one_to_one_k1', 'one_to_one_k5', 'up2_k5', 'down_k5', 'down_k1'])


def test_direct_route_gives_the_same_bits():
    """a 16 x 16 output from a 411 x 411 crop patch: the footprint of a tile does not fit the LDS budget, each thread
    evaluates its taps' k x k neighbourhoods itself.  Same restatement, same bits, k in {1, 3, 5}, HSV on and off."""
    frames = _scene()[0]
    cfg = _cfg(size=(16, 16), img_scale=16)
    rects = np.array([[-150, -160, 260, 250], [-40, -300, 370, 110], [-200, -100, 210, 310], [-150, -160, 260, 250]], np.int32)
    masks = _masks([(64, 48, 40), (30, 30, 25), (100, 60, 30), (64, 48, 40)])
    K = np.stack([K0] * 4)
    for hsv in (1.0, 0.0):
        aug = _aug(seed=9, noise_p=0.0, hsv_p=hsv)
        ids = _pick_ids(aug, [dict(k=1, c=1), dict(k=3, b=1), dict(k=5, a=1, b=-1), dict(k=5, c=-1)])
        want = patch_train_reference(frames, [0, 1, 0, 1], K, cfg, aug, ids, masks=masks, crop_rects=rects)
        assert _routes(want, want['draws']['k']) == ['direct'] * 4
        got = _run(frames, [0, 1, 0, 1], K, cfg, aug, ids, masks=masks, crop_rects=rects)
        _check_draws(got, want)
        _check_pixels(got, want, ['k1', 'k3', 'k5', 'k5b'])
        assert got['mask'].any()


@pytest.mark.parametrize('size,scale', SIZES)
def test_all_augmentations_off_is_extract_patches(size, scale):
    frames = _scene()[0]
    cfg = _cfg(size=size, img_scale=scale)
    aug = _aug(hsv_p=0.0, noise_p=0.0, smooth_p=0.0, size_range=(1.1, 1.1))
    params, ap = _params(cfg), ops.patch_aug_params(**aug)
    n = len(RECTS)
    fi = dev(np.arange(n) % 2, torch.int32)
    box = ops.patch_boxes_train(None, None, None, None, dev(np.stack([K0] * n)), (HF, WF), params, ap, crop_rects=dev(RECTS))
    img, mask = ops.extract_patches_train(dev(frames), fi, box['records'], params, ap)
    assert mask is None
    plain_box = ops.patch_boxes(None, None, None, None, dev(np.stack([K0] * n)), (HF, WF), params, crop_rects=dev(RECTS))
    plain = ops.extract_patches(dev(frames), fi, plain_box['records'], params)
    assert torch.equal(img, plain)
    # the head of the train workspace is the record extract_patches reads
    assert torch.equal(box['records'][:64 * n], plain_box['records'])
    assert torch.equal(ops.extract_patches(dev(frames), fi, box['records'][:64 * n].clone(), params), plain)
    # NaN-filled outputs are fully overwritten (image), and so is a mask of either fill
    masks = dev(_masks([(40 + 5 * i, 40, 25) for i in range(n)]))
    full = _aug(seed=3, noise_p=0.0)
    fp = ops.patch_aug_params(**full)
    box = ops.patch_boxes_train(None, None, None, None, dev(np.stack([K0] * n)), (HF, WF), params, fp, crop_rects=dev(RECTS))
    ref_img, ref_mask = ops.extract_patches_train(dev(frames), fi, box['records'], params, fp, masks=masks)
    for fill in (False, True):
        out = torch.full_like(ref_img, float('nan'))
        mo = torch.full_like(ref_mask, fill)
        ops.extract_patches_train(dev(frames), fi, box['records'], params, fp, masks=masks, out=out, mask_out=mo)
        assert torch.equal(out, ref_img) and torch.equal(mo, ref_mask)
    assert ref_mask.dtype == torch.bool and set(ref_mask.view(torch.uint8).unique().tolist()) <= {0, 1}


# ======================================================================================================= noise
# The device's normal draw z = sqrtf(-2 logf(u1)) cosf(2 pi u2) against numpy's float32 evaluation of the same expression:
# u1 >= 2^-25 so -2 ln u1 <= 34.7; logf, sqrtf and cosf are within 2 ulp on either side.  |d(-2 ln u1)| <= 4 ulp(34.7) =
# 1.5e-5, so the radius (<= 5.9, d sqrt = d / (2 sqrt)) moves by <= 1.5e-5 / 2 + 2 ulp(5.9) = 8.5e-6 for radii >= 1 (below 1
# the product with the sigma is smaller still); the cosine's argument is one fp32 product (both sides the same bits), its
# value differs by <= 4 ulp(1) = 4.8e-7, times the radius 2.8e-6; z therefore by <= 1.2e-5 + a product rounding (3e-7).
# Times s255 <= 25.5 grey levels and the final sum's rounding (ulp(255) / 2 = 7.6e-6): <= 3.3e-4 at the largest sigma,
# 1.6e-4 at sigma 255 = 12.75.  (The issue's estimate is 3e-5.)  The margin is 1e-3 grey levels around an integer.
NOISE_MARGIN = 1e-3


def _noise_case(noise_ratio, sample_id, side):
    frames = _scene()[0].copy()
    cfg = _cfg(size=(side, side), img_scale=side, to_rgb=False)
    aug = _aug(seed=13, hsv_p=0.0, smooth_p=0.0, noise_ratio=noise_ratio)
    rect = np.array([[20, 20, 20 + side - 1, 20 + side - 1]], np.int32)          # 1:1, inside the frame
    return frames, cfg, aug, rect, np.array([sample_id], np.int64)


def test_noise_vs_reference_up_to_the_transcendentals():
    frames, cfg, aug, rect, ids = _noise_case(0.1, 77, 32)
    got = _run(frames, [0], K0[None], cfg, aug, ids, crop_rects=rect)
    d = draws_reference(aug, ids)
    assert got['draws'][0, 7] == 1 and got['draws'][0, 5] == 1 and d['s255'][0] > 5
    src = frames[0, 20:52, 20:52]
    want, pre = noise_reference(src, aug['seed'], ids[0], d['s255'][0])
    out = np.rint(got['img'][0].transpose(1, 2, 0) * 255).astype(np.int64)       # (v - 0) * float32(1 / 255): v back exactly
    assert np.array_equal((out.astype(np.float32) * np.float32(1 / 255.)), got['img'][0].transpose(1, 2, 0))
    unclipped = (pre > 0) & (pre < 255)
    near = unclipped & (np.abs(pre - np.rint(pre)) < NOISE_MARGIN)
    frac = near.sum() / unclipped.sum()
    diff = np.abs(out - want.astype(np.int64))
    print(f'noise: {int(near.sum())} of {int(unclipped.sum())} unclipped values within {NOISE_MARGIN} of an integer '
          f'({100 * frac:.3f} %), mismatches there {int((diff[near] != 0).sum())}, elsewhere {int((diff[~near] != 0).sum())}')
    assert frac <= 0.01                                    # a continuous value lands there with probability 2e-3
    assert (diff[~near] == 0).all()
    assert diff[near].max(initial=0) <= 1
    assert (want != src).mean() > 0.9                      # the noise is there


def test_noise_moments_on_a_constant_frame():
    """constant 128, s = sigma 255 ~ 12.75 (10 sigma from the clip: nothing is clipped).  byte = trunc(128 + s z): mean
    128 - 1/2 (truncation bias), variance s^2 + 1/12 (truncation).  n = 3 * 64 * 64 samples: the mean's standard error is
    sqrt(var / n), the standard deviation's sqrt(var / (2 n)); five standard errors each."""
    side = 64
    u = draws_reference(_aug(seed=13, noise_ratio=1.0), np.array([5]))['sigma'][0]      # sigma = u noise_ratio
    frames, cfg, aug, rect, ids = _noise_case(0.05 / u, 5, side)
    frames[:] = 128
    d = draws_reference(aug, ids)
    s = float(d['s255'][0])
    assert abs(s - 12.75) < 1e-5
    got = _run(frames, [0], K0[None], cfg, aug, ids, crop_rects=rect)
    v = np.rint(got['img'][0] * 255).astype(np.float64).ravel()
    n, var = v.size, s * s + 1 / 12
    print(f'noise moments: mean {v.mean():.4f} (want {127.5}), std {v.std():.4f} (want {np.sqrt(var):.4f}), n = {n}')
    assert n == 3 * side * side and v.min() > 0 and v.max() < 255
    assert abs(v.mean() - 127.5) <= 5 * np.sqrt(var / n)
    assert abs(v.std() - np.sqrt(var)) <= 5 * np.sqrt(var / (2 * n))


# ======================================================================================== invariance and wiring
def _pipeline_inputs(n_per=(3, 2)):
    g = np.random.default_rng(31)
    Rs, ts, labels = [], [], []
    for i, label in enumerate([0, 3, 2, 0, 2]):
        R, _ = look_at_pose(*g.uniform(-0.5, 0.5, 3), 1.0)
        z = g.uniform(450, 700)
        Rs.append(R)
        ts.append(np.array([g.uniform(-30, 30) * z / 600, g.uniform(-20, 20) * z / 588, z], np.float32))
        labels.append(label)
    masks = _masks([(64, 48, 30), (50, 40, 20), (80, 60, 25), (30, 30, 18), (100, 50, 22)])
    return dict(frames=dev(_scene()[0]), gt_rotations=dev(np.stack(Rs)), gt_translations=dev(np.stack(ts)),
                k=dev(np.stack([K0] * 5)), labels=dev(np.array(labels)), masks=dev(masks)), list(n_per)


FLAT_KEYS = ('img', 'gt_masks', 'k', 'transform_matrix', 'crop', 'scale', 'valid', 'draws', 'ref_rotations',
             'ref_translations', 'init_add_error', 'init_rot_error', 'init_trans_error', 'jitter_ok', 'jitter_tries')


def _pipe(**kw):
    return TrainPatchPipeline(MeshStore(MESHES), DIAM, seed=5, size=(32, 32), img_scale=32, **kw)


def test_an_object_alone_equals_the_object_in_its_batch():
    a, counts = _pipeline_inputs()
    pipe = _pipe()
    ids = dev(np.array([40, 7, 2 ** 33, 12, 9], np.int64))
    batch = pipe(a['frames'], counts, a['gt_rotations'], a['gt_translations'], a['k'], a['labels'], a['masks'], sample_ids=ids)
    assert pipe.id_base == 0                                  # explicit ids do not advance the counter
    assert batch['flat']['jitter_ok'].tolist() == [1] * 5 and batch['valid'].tolist() == [1] * 5
    assert bool(batch['flat']['gt_masks'].any())
    for j in (0, 3, 4):
        f = 0 if j < counts[0] else 1
        one = pipe(a['frames'][f:f + 1], [1], a['gt_rotations'][j:j + 1], a['gt_translations'][j:j + 1], a['k'][j:j + 1],
                   a['labels'][j:j + 1], a['masks'][j:j + 1].contiguous(), sample_ids=ids[j:j + 1].contiguous())
        for key in FLAT_KEYS:
            assert torch.equal(one['flat'][key][0], batch['flat'][key][j]), (j, key)
    # ... and at another position, next to other objects
    perm = [4, 0, 3]
    sub = pipe(a['frames'], [0, 3], *(a[k][perm].contiguous() for k in ('gt_rotations', 'gt_translations', 'k', 'labels')),
               a['masks'][perm].contiguous(), sample_ids=ids[perm].contiguous())
    # object 0 comes from frame 0 in the batch and from frame 1 here: everything but its image must agree
    assert torch.equal(sub['flat']['img'][[0, 2]], batch['flat']['img'][[4, 3]])
    assert not torch.equal(sub['flat']['img'][1], batch['flat']['img'][0])
    for key in FLAT_KEYS[1:]:
        assert torch.equal(sub['flat'][key], batch['flat'][key][perm]), key


def test_calls_advance_the_sample_ids_and_reset_repeats():
    a, counts = _pipeline_inputs()
    pipe = _pipe()
    args = (a['frames'], counts, a['gt_rotations'], a['gt_translations'], a['k'], a['labels'], a['masks'])
    first = pipe(*args)
    assert pipe.id_base == 5
    second = pipe(*args)
    assert pipe.id_base == 10
    assert not torch.equal(first['flat']['img'], second['flat']['img'])
    assert not torch.equal(first['flat']['ref_rotations'], second['flat']['ref_rotations'])
    assert not torch.equal(first['flat']['draws'], second['flat']['draws'])
    again = pipe.reset(0)(*args)
    later = pipe(*args)
    for key in FLAT_KEYS:
        assert torch.equal(again['flat'][key], first['flat'][key]), key
        assert torch.equal(later['flat'][key], second['flat'][key]), key
    # the counter is the sample id: ids 5..9 by hand give the second call
    by_hand = pipe(*args, sample_ids=dev(np.arange(5, 10, dtype=np.int64)))
    assert torch.equal(by_hand['flat']['img'], second['flat']['img'])
    # the data_batch's layout
    ann = first['annots']
    assert set(ann) == {'ref_rotations', 'ref_translations', 'gt_rotations', 'gt_translations', 'gt_masks', 'init_add_error',
                        'init_rot_error', 'init_trans_error', 'k', 'labels'}
    assert [len(x) for x in ann['gt_masks']] == counts and ann['gt_masks'][0].dtype == torch.bool
    assert [tuple(x.shape) for x in first['img']] == [(3, 3, 32, 32), (2, 3, 32, 32)]
    meta = first['img_metas'][1]
    assert set(meta) >= {'img_norm_cfg', 'scale_factor', 'transform_matrix', 'ori_k', 'img_shape'}
    assert meta['img_shape'] == [(32, 32, 3)] * 2 and torch.equal(meta['ori_k'], a['k'][3])
    assert torch.equal(meta['transform_matrix'], first['flat']['transform_matrix'][3:])
    # the reference's swapped names by default: init_rot_error is the translation norm
    d = (first['flat']['ref_translations'] - a['gt_translations']).double().norm(dim=1)
    assert torch.allclose(first['flat']['init_rot_error'].double(), d, rtol=1e-5)


def test_pipeline_to_loss_on_the_device():
    """frames + gt poses + masks -> TrainPatchPipeline -> SCFlowRefiner.loss(data_batch) on the synthetic SCFlow model;
    finite, and bit-equal to loss(None, data=...) on a dict formatted by hand from the pipeline's flat tensors."""
    a, counts = _pipeline_inputs()
    store = MeshStore(MESHES)
    pipe = TrainPatchPipeline(store, DIAM, seed=2)                       # the shipped 256 x 256 patches
    batch = pipe(a['frames'], counts, a['gt_rotations'], a['gt_translations'], a['k'], a['labels'], a['masks'])
    flat = batch['flat']
    assert flat['valid'].tolist() == [1] * 5 and flat['jitter_ok'].tolist() == [1] * 5
    renderer = MeshRenderer(store, (256, 256), **RENDER_SHIPPED)
    cfg = scflow_amd.scflow_model_cfg(iters=2)
    cfg.update(scflow_amd.scflow_loss_cfgs())
    cfg['pose_loss_cfg']['loss_func_cfg'].update(symmetry_types={'cls_2': {}}, scale_xy=True)
    m = scflow_amd.build_refiner(cfg)
    here = os.path.dirname(os.path.abspath(__file__))
    shapes = json.load(open(os.path.join(here, 'golden', 'state_dict_keys.json')))['shapes']
    m.load_state_dict(scflow_amd.fill_state_dict(shapes, seed=0), strict=True)
    m = m.to(DEV).attach_renderer(renderer)
    m._build_loss_funcs()
    m.pose_loss_func.loss_func.meshes = store
    loss, _, log_vars, _, _ = m.loss(batch)
    assert np.isfinite(float(loss)) and all(np.isfinite(float(v)) for v in log_vars.values())
    assert 'init_add_mean' in log_vars
    # by hand, from the flat tensors
    norm = pipe.img_norm_cfg
    mean = (torch.tensor(norm['mean'], dtype=torch.float32) / 255.).tolist()
    std = (torch.tensor(norm['std'], dtype=torch.float32) / 255.).tolist()
    rgb, depth, mask = renderer.render_normalized(flat['ref_rotations'], flat['ref_translations'], flat['k'], a['labels'], mean, std)
    data = dict(ref_rotations=flat['ref_rotations'], ref_translations=flat['ref_translations'],
                gt_rotations=a['gt_rotations'], gt_translations=a['gt_translations'], labels=a['labels'],
                internel_k=flat['k'], rendered_images=rgb, real_images=flat['img'], rendered_masks=mask,
                rendered_depths=depth, gt_masks=flat['gt_masks'], scale_factors=flat['scale'])
    for name in ('add', 'rot', 'trans'):
        sd, mn = torch.std_mean(flat[f'init_{name}_error'], unbiased=False)
        data[f'init_{name}_error_mean'], data[f'init_{name}_error_std'] = mn, sd
    loss2, _, log_vars2, _, _ = m.loss(None, data=data)
    assert float(loss) == float(loss2) and list(log_vars.items()) == list(log_vars2.items())
