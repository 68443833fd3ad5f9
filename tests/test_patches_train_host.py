"""CPU: the train patch pipeline's host side -- TrainPatchPipeline.from_cfg and its refusals, the option checks, the C
entries' argument checks, the route model -- and ``patch_train_reference``, a numpy restatement of the semantics
patch_train.hip states (integers for the pixels and the draws, float64 for the jitter, float32 operation by operation for
HSV -> BGR and the noise), proven here on closed forms and used by test_gpu_patches_train.py as the yardstick.  cv2 and mmcv
are not installed: the restatement is the reference, cv2 bit parity is not claimed."""
import ctypes as C

import numpy as np
import pytest
import torch

import scflow_amd
from scflow_amd import _lib, ops
from scflow_amd.mesh import MeshStore, icosphere, make_mesh
from scflow_amd.patches import PatchPipeline, TrainPatchPipeline

from test_patches_host import (_cfg, box_reference, crop_reference, geometry_reference, resize_float64, resize_reference)

# stream numbers of scf_rng.h
JITTER, CROP, HSV, SIGMA, NOISE, SMOOTH, GATE_HSV, GATE_NOISE, GATE_SMOOTH = range(1, 10)

# the shipped train_pipeline's augmentation settings (ops.patch_aug_params' defaults)
AUG = dict(seed=0, jitter_angle_dis=(0., 15.), jitter_x_dis=(0., 15.), jitter_y_dis=(0., 15.), jitter_z_dis=(0., 50.),
           angle_limit=45., translation_limit=200., add_limit=1., max_tries=64, size_range=(1.0, 1.25), h_ratio=0.2,
           s_ratio=0.5, v_ratio=0.5, hsv_p=1.0, noise_ratio=0.1, noise_p=1.0, max_kernel_size=5, smooth_p=1.0,
           fix_error_swap_quirk=False, mask_pad_val=0)


def _aug(**kw):
    a = dict(AUG)
    a.update(kw)
    return a


# ---------------------------------------------------------------------------------------------- random numbers
def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def rng_mix(z):
    with np.errstate(over='ignore'):
        z = _u64(z) + _u64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> _u64(30))) * _u64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _u64(27))) * _u64(0x94D049BB133111EB)
        return z ^ (z >> _u64(31))


def rng_hash(seed, sample_id, stream, counter):
    return rng_mix(rng_mix(rng_mix(rng_mix(_u64(seed)) ^ _u64(sample_id)) ^ _u64(stream)) ^ _u64(counter))


def rng_u1(h):
    return ((h >> _u64(40)).astype(np.float64) + 0.5) * 2.0 ** -24


def rng_u2(h):
    return (((h >> _u64(16)) & _u64(0xFFFFFF)).astype(np.float64) + 0.5) * 2.0 ** -24


def rng_uniform(seed, sample_id, stream, counter=0):
    return rng_u1(rng_hash(seed, sample_id, stream, counter))


def rng_normal64(seed, sample_id, stream, counter):
    h = rng_hash(seed, sample_id, stream, counter)
    return np.sqrt(-2.0 * np.log(rng_u1(h))) * np.cos(2.0 * np.pi * rng_u2(h))


# ------------------------------------------------------------------------------------------------------ jitter
def euler_zyx(a0, a1, a2, order='contract'):
    """Rx(a2) Ry(a1) Rz(a0), angles in radians (``order='wrong'``: Rz(a0) Ry(a1) Rx(a2), the planted defect)."""
    cz, sz, cy, sy, cx, sx = np.cos(a0), np.sin(a0), np.cos(a1), np.sin(a1), np.cos(a2), np.sin(a2)
    rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    return rx @ ry @ rz if order == 'contract' else rz @ ry @ rx


def jitter_reference(R_gt, t_gt, labels, aug, sample_ids, meshes=None, diameters=None, stride=1, order='contract'):
    """item B of patch_train.hip in float64 from the fp32 inputs.  -> dict(rot, trans float64, add_error, rot_error,
    trans_error (as the kernel names them: swapped unless the quirk is fixed), ok, tries, margin: the smallest relative
    distance |value - limit| / limit over every limit comparison made)."""
    out = dict(rot=[], trans=[], add_error=[], rot_error=[], trans_error=[], ok=[], tries=[], margin=[])
    lim = {k: (-1.0 if aug[k] is None else float(aug[k])) for k in ('angle_limit', 'translation_limit', 'add_limit')}
    for n in range(len(R_gt)):
        R = np.asarray(R_gt[n], np.float32).astype(np.float64).reshape(3, 3)
        t = np.asarray(t_gt[n], np.float32).astype(np.float64).reshape(3)
        usable, verts, d = True, None, 1.0
        if meshes is not None:
            lab = int(labels[n])
            if 0 <= lab < len(diameters):
                verts = np.asarray(meshes.get(lab, np.zeros((0, 3), np.float32)), np.float32)[::stride].astype(np.float64)
                d = float(np.float32(diameters[lab]))
            else:
                usable = False
            if (verts is None or len(verts) == 0) and lim['add_limit'] >= 0:
                usable = False
        with_add = verts is not None and len(verts) > 0
        found, tries, margin = False, 0, np.inf
        Rr, tr, e_rot, e_trans, e_add = R, t, 0.0, 0.0, 0.0
        for tr_i in range(aug['max_tries'] if usable else 0):
            tries = tr_i + 1
            z = [float(rng_normal64(aug['seed'], sample_ids[n], JITTER, tr_i * 8 + i)) for i in range(6)]
            a = [np.deg2rad(aug['jitter_angle_dis'][0] + aug['jitter_angle_dis'][1] * z[i]) for i in range(3)]
            noise = np.array([aug['jitter_x_dis'][0] + aug['jitter_x_dis'][1] * z[3],
                              aug['jitter_y_dis'][0] + aug['jitter_y_dis'][1] * z[4],
                              aug['jitter_z_dis'][0] + aug['jitter_z_dis'][1] * z[5]])
            Rr = euler_zyx(a[0], a[1], a[2], order) @ R
            e_rot = float(np.rad2deg(np.arccos(np.clip((np.trace(Rr @ R.T) - 1) / 2, -1, 1))))
            e_trans = float(np.linalg.norm(noise))
            tr = t + noise
            rej = False
            for val, key in ((e_rot, 'angle_limit'), (e_trans, 'translation_limit')):
                if lim[key] >= 0 and not rej:
                    margin = min(margin, abs(val - lim[key]) / max(lim[key], 1e-300))
                    rej = val > lim[key]
            if not rej and with_add:
                diff = verts @ (R - Rr).T + (t - tr)
                e_add = float(np.linalg.norm(diff, axis=1).mean() / d)
                if lim['add_limit'] >= 0:
                    margin = min(margin, abs(e_add - lim['add_limit']) / max(lim['add_limit'], 1e-300))
                    rej = e_add > lim['add_limit']
            if not rej:
                found = True
                break
        if not found:
            Rr, tr, e_rot, e_trans, e_add = R, t, 0.0, 0.0, 0.0
        elif not with_add:
            e_add = np.nan
        swap = not aug['fix_error_swap_quirk']
        out['rot'].append(Rr)
        out['trans'].append(tr)
        out['add_error'].append(e_add)
        out['rot_error'].append(e_trans if swap else e_rot)
        out['trans_error'].append(e_rot if swap else e_trans)
        out['ok'].append(int(found))
        out['tries'].append(tries)
        out['margin'].append(margin)
    return {k: np.asarray(v) for k, v in out.items()}


# ------------------------------------------------------------------------------------------------------- draws
def draws_reference(aug, sample_ids):
    """item C: per object (ratio float64, a, b, c float32, sigma float64, s255 float32, k, hsv_on, noise_on)."""
    sid, seed = _u64(sample_ids), aug['seed']
    lo, hi = aug['size_range']
    ratio = lo + (hi - lo) * rng_uniform(seed, sid, CROP)
    gains = [((2.0 * rng_uniform(seed, sid, HSV, i) - 1.0) * aug[key] + 1.0).astype(np.float32)
             for i, key in enumerate(('h_ratio', 's_ratio', 'v_ratio'))]
    sigma = rng_uniform(seed, sid, SIGMA) * aug['noise_ratio']
    kinds = int(aug['max_kernel_size']) // 2 + 1
    idx = np.minimum((rng_uniform(seed, sid, SMOOTH) * kinds).astype(np.int64), kinds - 1)
    smooth_on = rng_uniform(seed, sid, GATE_SMOOTH) <= aug['smooth_p']
    return dict(ratio=ratio, a=gains[0], b=gains[1], c=gains[2], sigma=sigma, s255=(sigma * 255.0).astype(np.float32),
                k=np.where(smooth_on, 2 * idx + 1, 1), hsv_on=rng_uniform(seed, sid, GATE_HSV) <= aug['hsv_p'],
                noise_on=rng_uniform(seed, sid, GATE_NOISE) <= aug['noise_p'])


# --------------------------------------------------------------------------------------------------------- HSV
_I = np.arange(1, 256, dtype=np.float64)
SDIV = np.concatenate([[0], np.rint((255 << 12) / _I)]).astype(np.int64)
HDIV = np.concatenate([[0], np.rint((180 << 12) / (6.0 * _I))]).astype(np.int64)
SECTOR = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])


def bgr_to_hsv(img):
    """item D.b, integers: (..., 3) uint8 BGR -> h in [0, 180), s, v int64 arrays."""
    b, g, r = (img[..., i].astype(np.int64) for i in range(3))
    v = np.maximum(b, np.maximum(g, r))
    d = v - np.minimum(b, np.minimum(g, r))
    s = (d * SDIV[v] + 2048) >> 12
    h = np.where(v == r, g - b, np.where(v == g, b - r + 2 * d, r - g + 4 * d))
    h = (h * HDIV[d] + 2048) >> 12
    return h + np.where(h < 0, 180, 0), s, v


def hsv_gain(x, gain, top, inverted=False):
    """channel times gain in float32, clipped to ``top`` ONLY when the gain is >= 1 (the reference's rule), truncated and
    stored as a byte.  Under the rule nothing exceeds ``top``.  ``inverted``: the planted defect, the clip applied when the
    gain is below 1 instead -- a gain >= 1 then wraps in the byte."""
    y = x.astype(np.float32) * np.float32(gain)
    if (np.float32(gain) >= 1) != inverted:
        y = np.minimum(y, np.float32(top))
    return np.trunc(y).astype(np.int64) & 255


def hsv_to_bgr(h, s, v):
    """item D.b, float32 operation by operation -> (..., 3) uint8 BGR."""
    one = np.float32(1)
    sf = s.astype(np.float32) * (one / np.float32(255))
    vf = v.astype(np.float32) * (one / np.float32(255))
    hh = h.astype(np.float32) * (np.float32(6) / np.float32(180))
    fl = np.floor(hh)
    sector = fl.astype(np.int64)
    f = (hh - fl).astype(np.float32)
    bad = (sector < 0) | (sector >= 6)
    sector, f = np.where(bad, 0, sector), np.where(bad, np.float32(0), f)
    tab = np.stack([vf, vf * (one - sf), vf * (one - sf * f), vf * (one - sf * (one - f))], -1).astype(np.float32)
    x = np.take_along_axis(tab, SECTOR[sector], -1)
    return np.clip(np.rint(np.float32(255) * x), 0, 255).astype(np.uint8)


def hsv_reference(img, a, b, c, inverted=False):
    h, s, v = bgr_to_hsv(img)
    return hsv_to_bgr(hsv_gain(h, a, 179, inverted), hsv_gain(s, b, 255, inverted), hsv_gain(v, c, 255, inverted))


# ------------------------------------------------------------------------------------------------ noise, smooth
def noise_reference(patch, seed, sample_id, s255):
    """item D.c -> (uint8 patch, float32 values before the truncation, clipped to [0, 255])."""
    ph, pw = patch.shape[:2]
    key = (np.arange(ph * pw * 3, dtype=np.uint64)).reshape(ph, pw, 3)
    h = rng_hash(seed, sample_id, NOISE, key)
    u1, u2 = rng_u1(h).astype(np.float32), rng_u2(h).astype(np.float32)
    z = np.sqrt(np.float32(-2) * np.log(u1)) * np.cos(np.float32(6.2831855) * u2)
    x = np.clip(patch.astype(np.float32) + z.astype(np.float32) * np.float32(s255), np.float32(0), np.float32(255))
    return np.trunc(x).astype(np.uint8), x.astype(np.float32)


def reflect101(i, n):
    if n == 1:
        return 0
    while i < 0 or i >= n:
        i = -i if i < 0 else 2 * n - 2 - i
    return i


def smooth_reference(patch, k, border='reflect101'):
    """item D.d: k x k box mean, integer sum, rounded to nearest (``border='replicate'``: the planted defect)."""
    if k == 1:
        return patch
    ph, pw = patch.shape[:2]
    r = k // 2
    if border == 'reflect101':
        ys = np.array([[reflect101(y + d, ph) for d in range(-r, r + 1)] for y in range(ph)])
        xs = np.array([[reflect101(x + d, pw) for d in range(-r, r + 1)] for x in range(pw)])
    else:
        ys = np.clip(np.arange(ph)[:, None] + np.arange(-r, r + 1), 0, ph - 1)
        xs = np.clip(np.arange(pw)[:, None] + np.arange(-r, r + 1), 0, pw - 1)
    P = patch.astype(np.int64)
    S = P[ys].sum(1)                      # (ph, pw, 3): vertical sums
    S = S[:, xs].sum(2)                   # horizontal
    return ((S + (k * k) // 2) // (k * k)).astype(np.uint8)


def augment_reference(patch, seed, sample_id, d, defect=None):
    """steps b-d on one crop patch; ``d``: this object's draws (scalars)."""
    if defect == 'blur_before_noise':
        patch = smooth_reference(patch, int(d['k']))
    if d['hsv_on']:
        patch = hsv_reference(patch, d['a'], d['b'], d['c'], inverted=defect == 'clip_inverted')
    if d['noise_on']:
        patch = noise_reference(patch, seed, sample_id, d['s255'])[0]
    if defect != 'blur_before_noise':
        patch = smooth_reference(patch, int(d['k']), border='replicate' if defect == 'replicate' else 'reflect101')
    return patch


# -------------------------------------------------------------------------------------------------------- mask
def mask_reference(mask, geo, cfg, pad, bilinear=False):
    """item D.f for one object -> (H, W) bool."""
    H, W = cfg['size']
    out = np.full((H, W), bool(pad))
    if not geo['valid'] or mask is None:
        return out
    x1, y1, x2, y2 = geo['crop']
    m = crop_reference(np.repeat((mask != 0).astype(np.uint8)[..., None], 3, -1), geo['crop'], (0, 0, 0))[..., 0]
    ph, pw = m.shape
    if bilinear:                                          # the planted defect: the image's interpolation, thresholded
        small = resize_float64(np.repeat(m[..., None], 3, -1) * 255, geo['new_h'], geo['new_w'])[..., 0] >= 127.5
    else:
        sy = np.minimum(np.floor(np.arange(geo['new_h']) * (np.float64(ph) / np.float64(geo['new_h']))).astype(np.int64), ph - 1)
        sx = np.minimum(np.floor(np.arange(geo['new_w']) * (np.float64(pw) / np.float64(geo['new_w']))).astype(np.int64), pw - 1)
        small = m[sy][:, sx] != 0
    out[geo['top']:geo['top'] + geo['new_h'], geo['left']:geo['left'] + geo['new_w']] = small
    return out


# ---------------------------------------------------------------------------------------------- the whole thing
def pixels_train_reference(frame, geo, cfg, seed, sample_id, d, defect=None):
    """patch.hip's items 2 (pixels), 3, 4 and 6 with steps b-d between the crop and the resize -> (3, H, W) float32."""
    H, W = cfg['size']
    img = np.empty((H, W, 3), np.uint8)
    img[:] = np.asarray(cfg['pad_val'], np.uint8)
    if geo['valid'] and frame is not None:
        patch = augment_reference(crop_reference(frame, geo['crop'], cfg['crop_pad_val']), seed, sample_id, d, defect)
        img[geo['top']:geo['top'] + geo['new_h'], geo['left']:geo['left'] + geo['new_w']] = \
            resize_reference(patch, geo['new_h'], geo['new_w'])
    if cfg['to_rgb']:
        img = img[..., ::-1]
    mean = np.asarray(cfg['mean'], np.float32)
    inv = (1.0 / np.asarray(cfg['std'], np.float32).astype(np.float64)).astype(np.float32)
    return np.ascontiguousarray(((img.astype(np.float32) - mean) * inv).transpose(2, 0, 1))


def patch_train_reference(frames, frame_index, K, cfg, aug, sample_ids, masks=None, meshes=None, labels=None, R=None,
                          t=None, crop_rects=None, defect=None):
    """items C and D for N objects on the poses handed in (the jittered ones).  -> dict(img, mask, crop, scale, tm, k, valid,
    draws: dict of arrays)."""
    n = len(K)
    draws = draws_reference(aug, sample_ids)
    out = dict(img=[], mask=[], crop=[], scale=[], tm=[], k=[], valid=[])
    for i in range(n):
        c = dict(cfg, size_ratio=float(draws['ratio'][i]))
        if crop_rects is not None:
            geo = geometry_reference(K[i], frames.shape[1:3], c, rect=crop_rects[i])
        else:
            verts = meshes.get(int(labels[i]), np.zeros((0, 3), np.float32))
            box, ok = box_reference(verts, R[i], t[i], K[i], cfg['vertex_stride'])
            geo = geometry_reference(K[i], frames.shape[1:3], c, box32=box.astype(np.float32), valid=ok)
        fi = int(frame_index[i])
        frame = frames[fi] if 0 <= fi < len(frames) else None
        d = {k: v[i] for k, v in draws.items()}
        out['img'].append(pixels_train_reference(frame, geo, cfg, aug['seed'], sample_ids[i], d, defect))
        if masks is not None:
            out['mask'].append(mask_reference(masks[i] if frame is not None else None, geo, cfg, aug['mask_pad_val'],
                                              bilinear=defect == 'mask_bilinear'))
        for key, val in (('crop', geo['crop']), ('scale', geo['s']), ('tm', geo['tm']), ('k', geo['k']),
                         ('valid', int(geo['valid']))):
            out[key].append(val)
    res = {k: np.stack([np.asarray(x) for x in v]) for k, v in out.items() if v}
    res['draws'] = draws
    return res


# ================================================================================== proofs of the restatement
def test_uniforms_are_exact_open_interval_and_batch_position_invariant():
    h = rng_hash(7, np.arange(1000), CROP, 0)
    u = rng_u1(h)
    assert u.min() > 0 and u.max() < 1
    assert np.array_equal(u * 2.0 ** 25, np.rint(u * 2.0 ** 25))                  # 25 significant bits: exact in fp64
    assert rng_u1(_u64([0xFFFFFF0000000000]))[0] == 1 - 2.0 ** -25 and rng_u1(_u64([0]))[0] == 2.0 ** -25
    assert abs(u.mean() - 0.5) < 5 / np.sqrt(12 * 1000)
    # the splitmix64 finaliser's published first output for state 0
    assert int(rng_mix(0)) == 0xE220A8397B1DCDAF
    # an object's draws depend on (seed, sample id) alone: alone, or at any position of any batch
    ids = np.array([5, 900, 17, 3], np.int64)
    full = draws_reference(_aug(seed=3), ids)
    for pos, sid in enumerate(ids):
        alone = draws_reference(_aug(seed=3), np.array([sid]))
        assert all(alone[k][0] == full[k][pos] for k in full)
    perm = draws_reference(_aug(seed=3), ids[::-1])
    assert all(np.array_equal(perm[k], full[k][::-1]) for k in full)
    assert not np.array_equal(draws_reference(_aug(seed=4), ids)['ratio'], full['ratio'])
    # ranges
    many = draws_reference(_aug(), np.arange(4000))
    assert 1.0 < many['ratio'].min() and many['ratio'].max() < 1.25
    assert set(np.unique(many['k'])) == {1, 3, 5}
    assert many['a'].min() > 0.8 and many['a'].max() < 1.2 and many['b'].min() > 0.5 and many['c'].max() < 1.5
    assert many['hsv_on'].all() and many['noise_on'].all()
    off = draws_reference(_aug(hsv_p=0.0, noise_p=0.0, smooth_p=0.0), np.arange(100))
    assert not off['hsv_on'].any() and not off['noise_on'].any() and (off['k'] == 1).all()


def test_normal_draws_have_unit_moments():
    z = rng_normal64(1, 2, JITTER, np.arange(200000))
    assert abs(z.mean()) < 5 / np.sqrt(z.size) and abs(z.std() - 1) < 5 / np.sqrt(2 * z.size)


def test_euler_order_is_scipys_lower_case_zyx():
    from scipy.spatial.transform import Rotation
    g = np.random.default_rng(0)
    worst, other = 0.0, 0.0
    for _ in range(50):
        a = g.normal(0, 15, 3)
        want = Rotation.from_euler('zyx', a, degrees=True).as_matrix()
        worst = max(worst, np.abs(euler_zyx(*np.deg2rad(a)) - want).max())
        other = max(other, np.abs(euler_zyx(*np.deg2rad(a), order='wrong') - want).max())
    assert worst < 1e-15 and other > 0.05, (worst, other)


def _jitter_case(n=6, seed=0):
    g = np.random.default_rng(seed)
    from scipy.spatial.transform import Rotation
    R = Rotation.random(n, random_state=seed).as_matrix().astype(np.float32)
    t = np.stack([g.uniform(-100, 100, n), g.uniform(-100, 100, n), g.uniform(400, 900, n)], 1).astype(np.float32)
    verts, _ = icosphere(2, 50.0)
    return R, t, np.zeros(n, np.int64), {0: verts.astype(np.float32)}, [100.0]


def test_jitter_reference_limits_quirk_and_failure():
    R, t, labels, meshes, diam = _jitter_case()
    ids = np.arange(100, 106)
    out = jitter_reference(R, t, labels, _aug(), ids, meshes, diam)
    assert out['ok'].all() and (out['tries'] >= 1).all()
    for n in range(len(R)):
        dR = out['rot'][n] @ R[n].astype(np.float64).T
        angle = np.rad2deg(np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1)))
        # the reference's swapped names: rot_error is the translation norm, trans_error the angle
        assert out['trans_error'][n] == pytest.approx(angle, abs=1e-9) and angle <= 45
        assert out['rot_error'][n] == pytest.approx(np.linalg.norm(out['trans'][n] - t[n]), rel=1e-12)
        assert abs(np.linalg.det(out["rot"][n]) - 1) < 1e-6                          # R_gt is an fp32 rotation
        assert 0 < out['add_error'][n] <= 1.0
    fixed = jitter_reference(R, t, labels, _aug(fix_error_swap_quirk=True), ids, meshes, diam)
    assert np.array_equal(fixed['rot_error'], out['trans_error']) and np.array_equal(fixed['trans_error'], out['rot_error'])
    assert not np.allclose(fixed['rot_error'], out['rot_error'])                 # planted defect: swap quirk off
    # wrong Euler order: another rotation
    wrong = jitter_reference(R, t, labels, _aug(), ids, meshes, diam, order='wrong')
    assert np.abs(wrong['rot'] - out['rot']).max() > 1e-3
    # a limit nothing passes: the gt pose, zero errors, ok = 0, tries = max_tries
    none = jitter_reference(R, t, labels, _aug(angle_limit=0.0, max_tries=5), ids, meshes, diam)
    assert not none['ok'].any() and (none['tries'] == 5).all() and (none['rot_error'] == 0).all()
    assert np.array_equal(none['rot'], R.astype(np.float64)) and np.array_equal(none['trans'], t.astype(np.float64))
    # tight limits reject early tries: the accepted try is not always the first
    tight = jitter_reference(R, t, labels, _aug(angle_limit=12.0, max_tries=64), np.arange(40)[:6], meshes, diam)
    assert tight['tries'].max() > 1 and tight['ok'].all()
    # label out of range, empty class under add_limit
    bad = jitter_reference(R[:2], t[:2], np.array([3, 0]), _aug(), ids[:2], {0: np.zeros((0, 3), np.float32)}, [100.0])
    assert bad['ok'].tolist() == [0, 0] and bad['tries'].tolist() == [0, 0]
    # no mesh, no add_limit: add_error is NaN
    free = jitter_reference(R, t, labels, _aug(add_limit=None), ids)
    assert np.isnan(free['add_error']).all() and free['ok'].all()
    # shipped distributions: most tries pass (97.1 % measured on 1e5 numpy draws)
    assert jitter_reference(R, t, labels, _aug(add_limit=None), np.arange(6))['tries'].max() <= 3


def test_jitter_reference_against_the_reference_class():
    """tests/golden/pose_jitter.npz: the reference's own PoseJitter.__call__ (constructor bypassed, np.random.normal
    replaying this restatement's draws; make_golden_jitter.py).  It computes the rotation in float32, so values agree to
    float32 accuracy; the decisions agree because every limit comparison is 1e-4 away from its limit."""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pose_jitter.npz'))
    aug = _aug(seed=int(z['seed']), max_tries=64, **{k[4:]: (tuple(z[k]) if z[k].ndim else float(z[k])) for k in z.files
                                                     if k.startswith('cfg_')})
    out = jitter_reference(z['R'], z['t'], z['labels'], aug, z['ids'], {0: z['verts0'], 1: z['verts1']}, list(z['diam']))
    assert out['margin'].min() > 1e-4
    assert out['tries'].tolist() == z['tries'].tolist() and out['ok'].all() and z['tries'].max() > 4
    assert np.abs(out['rot'] - z['ref_rotations']).max() < 1e-6
    assert np.allclose(out['trans'], z['ref_translations'], rtol=1e-6, atol=1e-4)
    # the swapped names: the class's init_rot_error is the translation norm, its init_trans_error the angle
    assert np.allclose(out['rot_error'], z['init_rot_error'], rtol=1e-6)
    assert np.allclose(out['trans_error'], z['init_trans_error'], rtol=1e-4, atol=1e-3)
    assert np.allclose(out['rot_error'], np.linalg.norm(z['ref_translations'] - z['t'], axis=1), rtol=1e-5)
    assert np.allclose(out['add_error'], z['init_add_error'], rtol=1e-5)
    wrong = jitter_reference(z['R'], z['t'], z['labels'], aug, z['ids'], {0: z['verts0'], 1: z['verts1']}, list(z['diam']),
                             order='wrong')
    assert np.abs(wrong['rot'] - z['ref_rotations']).max() > 1e-2                 # planted defect: the other Euler order


def test_hsv_grey_stays_grey_and_scales_by_c():
    grey = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, 1)[None]
    for c in (0.5, 0.75, 1.0, 1.25, 1.5):
        out = hsv_reference(grey, 1.1, 0.7, np.float32(c))
        want = np.minimum(np.trunc(np.arange(256, dtype=np.float32) * np.float32(c)), 255)
        assert (out[0, :, 0] == out[0, :, 1]).all() and (out[0, :, 1] == out[0, :, 2]).all()
        assert np.array_equal(out[0, :, 0], want.astype(np.uint8))


def test_hsv_hue_wraps_and_primaries():
    px = np.array([[[0, 0, 255], [0, 255, 0], [255, 0, 0], [255, 0, 255], [255, 255, 0], [0, 255, 255]]], np.uint8)   # BGR
    h, s, v = bgr_to_hsv(px)
    assert h[0].tolist() == [0, 60, 120, 150, 90, 30] and (s == 255).all() and (v == 255).all()
    # a red with a little more blue than green has a negative raw hue: it wraps to just below 180
    h, _, _ = bgr_to_hsv(np.array([[[14, 10, 200]]], np.uint8))
    assert h[0, 0] == 179
    assert np.array_equal(hsv_to_bgr(*bgr_to_hsv(px)), px)
    # a gain above 1 is clipped at 179 (no wrap to red), below 1 it is not clipped
    assert hsv_gain(np.array([170]), 1.2, 179)[0] == 179 and hsv_gain(np.array([170]), 0.5, 179)[0] == 85
    assert hsv_gain(np.array([255]), 1.0, 255)[0] == 255 and hsv_gain(np.array([255]), np.float32(0.999), 255)[0] == 254
    # planted defect: the clip applied when the gain is below 1 (and so not at >= 1) wraps in the byte
    assert hsv_gain(np.array([200]), 1.5, 255, inverted=True)[0] == 300 - 256


# Gains of exactly 1: BGR -> HSV -> BGR over the whole 8-bit cube.  The round trip is not the identity in 8 bits (H has
# 180 levels, S is quantised); the figures below are what this restatement gives, pinned so that a change of the contract
# shows.
HSV_ROUNDTRIP_MAX_DEV = 5
HSV_ROUNDTRIP_EXACT_FRACTION = (0.3095, 0.3115)      # 0.3105 found


def test_hsv_unit_gains_over_the_whole_cube():
    worst, exact = 0, 0
    g, r = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing='ij')
    for b in range(256):
        img = np.stack([np.full_like(g, b), g, r], -1)
        dev = np.abs(hsv_reference(img, 1.0, 1.0, 1.0).astype(np.int64) - img.astype(np.int64)).max(-1)
        worst = max(worst, int(dev.max()))
        exact += int((dev == 0).sum())
    frac = exact / 256 ** 3
    print(f'HSV round trip at unit gains: max deviation {worst} levels, {frac:.4f} of the cube exact')
    assert worst == HSV_ROUNDTRIP_MAX_DEV
    assert HSV_ROUNDTRIP_EXACT_FRACTION[0] < frac < HSV_ROUNDTRIP_EXACT_FRACTION[1]


def test_box_mean_against_float64_and_borders():
    g = np.random.default_rng(1)
    for (ph, pw), k in (((9, 13), 3), ((9, 13), 5), ((1, 7), 5), ((6, 1), 3), ((2, 2), 5), ((3, 4), 5)):
        patch = g.integers(0, 256, (ph, pw, 3), dtype=np.uint8)
        r = k // 2
        ys = [[reflect101(y + d, ph) for d in range(-r, r + 1)] for y in range(ph)]
        xs = [[reflect101(x + d, pw) for d in range(-r, r + 1)] for x in range(pw)]
        mean = np.array([[patch[ys[y]][:, xs[x]].astype(np.float64).mean((0, 1)) for x in range(pw)] for y in range(ph)])
        got = smooth_reference(patch, k)
        assert np.abs(got.astype(np.float64) - mean).max() <= 0.5
        assert np.array_equal(got, np.floor(mean + 0.5).astype(np.uint8))           # k^2 is odd: no ties
    assert [reflect101(i, 5) for i in (-2, -1, 0, 4, 5, 6)] == [2, 1, 0, 4, 3, 2]
    assert [reflect101(i, 2) for i in (-2, -1, 2, 3)] == [0, 1, 0, 1] and reflect101(-3, 1) == 0
    # a constant patch stays constant; planted defect: replicate instead of reflect-101 differs at the border
    assert (smooth_reference(np.full((5, 5, 3), 77, np.uint8), 5) == 77).all()
    patch = g.integers(0, 256, (12, 12, 3), dtype=np.uint8)
    a, b = smooth_reference(patch, 5), smooth_reference(patch, 5, border='replicate')
    assert np.array_equal(a[2:-2, 2:-2], b[2:-2, 2:-2]) and not np.array_equal(a, b)
    assert smooth_reference(patch, 1) is patch


def test_noise_reference_moments_and_keying():
    patch = np.full((64, 64, 3), 128, np.uint8)
    out, pre = noise_reference(patch, 0, 9, np.float32(12.75))
    n = out.size
    # trunc of 128 + 12.75 z: mean 128 - 0.5, variance 12.75^2 + 1/12 (nothing is clipped at 10 sigma)
    assert abs(out.mean() - 127.5) < 5 * np.sqrt((12.75 ** 2 + 1 / 12) / n)
    assert abs(out.std() - np.sqrt(12.75 ** 2 + 1 / 12)) < 5 * np.sqrt((12.75 ** 2 + 1 / 12) / (2 * n))
    assert np.array_equal(out, np.trunc(pre).astype(np.uint8))
    # keyed by the patch coordinate: a sub-patch of another width gets other draws, the same width the same ones
    top, _ = noise_reference(patch[:10], 0, 9, np.float32(12.75))
    assert np.array_equal(top, out[:10])
    assert not np.array_equal(noise_reference(patch[:, :32], 0, 9, np.float32(12.75))[0][1], out[1, :32])
    assert not np.array_equal(noise_reference(patch, 0, 10, np.float32(12.75))[0], out)


K0 = np.array([[600., 0, 64.5], [0, 590., 48.25], [0, 0, 1]], np.float32)


def _small_case(**aug_kw):
    g = np.random.default_rng(2)
    frames = g.integers(0, 256, (2, 96, 128, 3), dtype=np.uint8)
    rects = np.array([[10, 12, 70, 60], [-8, 30, 40, 95], [100, 5, 127, 40]], np.int32)
    masks = np.zeros((3, 96, 128), np.uint8)
    yy, xx = np.mgrid[:96, :128]
    for i, (cx, cy, rad) in enumerate(((40, 36, 20), (16, 62, 25), (114, 22, 12))):
        masks[i] = ((xx - cx) ** 2 + (yy - cy) ** 2 < rad ** 2) * 255
    cfg = _cfg(size=(32, 32), img_scale=32)
    return frames, np.array([0, 1, 0]), np.stack([K0] * 3), cfg, _aug(**aug_kw), np.array([11, 12, 13]), masks, rects


def test_planted_pixel_defects_fall_outside():
    frames, fi, K, cfg, aug, ids, masks, rects = _small_case(seed=5)
    base = patch_train_reference(frames, fi, K, cfg, aug, ids, masks=masks, crop_rects=rects)
    assert set(base['draws']['k'].tolist()) - {1} and base['valid'].all()
    again = patch_train_reference(frames, fi, K, cfg, aug, ids, masks=masks, crop_rects=rects)
    assert np.array_equal(again['img'], base['img']) and np.array_equal(again['mask'], base['mask'])
    assert (base['draws']['b'] >= 1).any() or (base['draws']['c'] >= 1).any()
    for defect in ('blur_before_noise', 'replicate', 'mask_bilinear', 'clip_inverted'):
        bad = patch_train_reference(frames, fi, K, cfg, aug, ids, masks=masks, crop_rects=rects, defect=defect)
        key = 'mask' if defect == 'mask_bilinear' else 'img'
        assert not np.array_equal(bad[key], base[key]), defect
    # masks: nearest, padded with pad_val['mask'], all-pad for an invalid object
    assert base['mask'].dtype == bool and base['mask'].any() and not base['mask'].all()
    inv = patch_train_reference(frames, fi, K, cfg, _aug(seed=5, mask_pad_val=1), ids, masks=masks,
                                crop_rects=np.array([[5, 5, 2, 9]] * 3, np.int32))
    assert not inv['valid'].any() and inv['mask'].all()


def test_all_augmentations_off_is_the_val_path():
    from test_patches_host import patch_reference
    frames, fi, K, cfg, aug, ids, masks, rects = _small_case(hsv_p=0.0, noise_p=0.0, smooth_p=0.0)
    got = patch_train_reference(frames, fi, K, cfg, aug, ids, crop_rects=rects)
    want = patch_reference(frames, fi, K, cfg, crop_rects=rects)
    assert np.array_equal(got['img'], want['img']) and np.array_equal(got['crop'], want['crop'])


# ======================================================================================================= host API
TRAIN_PIPELINE = [      # configs/refine_datasets/ycbv_real.py:27-72, copied as data
    dict(type='LoadImages', color_type='unchanged', file_client_args=dict(backend='disk')),
    dict(type='LoadMasks'),
    dict(type='PoseJitter', jitter_angle_dis=(0, 15), jitter_x_dis=(0, 15), jitter_y_dis=(0, 15), jitter_z_dis=(0, 50),
         angle_limit=45, translation_limit=200, add_limit=1., mesh_dir='data/ycbv/models_eval',
         mesh_diameter=[172.16, 269.58, 198.38, 120.66, 199.79, 90.17, 142.58, 114.39, 129.73, 198.40, 263.60, 260.76,
                        162.27, 126.86, 230.44, 237.30, 204.11, 121.46, 183.08, 231.39, 102.92],
         jitter_pose_field=['gt_rotations', 'gt_translations'], jittered_pose_field=['ref_rotations', 'ref_translations']),
    dict(type='ComputeBbox', mesh_dir='data/ycbv/models_eval', clip_border=False),
    dict(type='Crop', size_range=(1.0, 1.25), crop_bbox_field='ref_bboxes', clip_border=False, pad_val=128),
    dict(type='RandomHSV', h_ratio=0.2, s_ratio=0.5, v_ratio=0.5),
    dict(type='RandomNoise', noise_ratio=0.1),
    dict(type='RandomSmooth', max_kernel_size=5.),
    dict(type='Resize', img_scale=256, keep_ratio=True),
    dict(type='Pad', size=(256, 256), center=True, pad_val=dict(img=(128, 128, 128), mask=0)),
    dict(type='RemapPose', keep_intrinsic=False),
    dict(type='Normalize', mean=[0., 0., 0.], std=[255., 255., 255.], to_rgb=True),
    dict(type='ToTensor', stack_keys=[]),
    dict(type='Collect',
         annot_keys=['ref_rotations', 'ref_translations', 'gt_rotations', 'gt_translations', 'gt_masks', 'init_add_error',
                     'init_rot_error', 'init_trans_error', 'k', 'labels'],
         meta_keys=('img_path', 'ori_shape', 'ori_k', 'img_shape', 'img_norm_cfg', 'scale_factor', 'transform_matrix',
                    'ori_gt_rotations', 'ori_gt_translations')),
]


def _store(n=1):
    v, f = icosphere(1, 50.0)
    return MeshStore({i: make_mesh(v, f) for i in range(n)})


def test_from_cfg_reads_the_shipped_train_pipeline():
    pipe = TrainPatchPipeline.from_cfg(TRAIN_PIPELINE, _store(21), seed=3)
    assert isinstance(pipe, scflow_amd.TrainPatchPipeline) and pipe.seed == 3
    a = pipe.aug
    assert list(a.jitter_angle) == [0, 15] and list(a.jitter_z) == [0, 50] and list(a.size_range) == [1.0, 1.25]
    assert (a.angle_limit, a.translation_limit, a.add_limit, a.max_tries) == (45, 200, 1.0, 64)
    assert list(a.hsv_ratio) == [0.2, 0.5, 0.5] and (a.hsv_p, a.noise_p, a.smooth_p) == (1, 1, 1)
    assert a.noise_ratio == 0.1 and a.max_kernel_size == 5 and a.fix_error_swap_quirk == 0 and a.mask_pad_val == 0
    p = pipe.params
    assert (p.out_h, p.out_w, p.resize, p.clip_border, p.center, p.to_rgb) == (256, 256, 256, 0, 1, 1)
    assert list(p.crop_pad_val) == [128] * 3 and list(p.pad_val) == [128] * 3
    assert pipe.diameters.shape == (21,) and float(pipe.diameters[1]) == pytest.approx(269.58)
    # a pipeline without the colour transforms switches them off; overrides win
    plain = [s for s in TRAIN_PIPELINE if not s['type'].startswith('Random')]
    q = TrainPatchPipeline.from_cfg(plain, _store(21), add_limit=None, fix_error_swap_quirk=True)
    assert (q.aug.hsv_p, q.aug.noise_p, q.aug.smooth_p) == (0, 0, 0) and q.aug.add_limit < 0 and q.aug.fix_error_swap_quirk == 1
    # reset / id_base
    assert pipe.id_base == 0 and pipe.reset(40).id_base == 40
    with pytest.raises(ValueError):
        pipe.reset(-1)
    with pytest.raises(ValueError, match='mesh_diameter holds'):
        TrainPatchPipeline(_store(3), [100.0])
    # a diameter that is missing, not finite or not positive is refused: NaN would pass every ADD comparison
    for bad in ([100.0, float('nan'), 50.0], [100.0, 0.0, 50.0], [100.0, -1.0, 50.0], {0: 100.0, 2: 50.0}):
        with pytest.raises(ValueError, match='finite and positive'):
            TrainPatchPipeline(_store(3), bad)
    sparse = MeshStore({0: _store().meshes[0], 2: _store().meshes[0]})          # class 1 has no mesh: no diameter needed
    assert TrainPatchPipeline(sparse, {0: 100.0, 2: 50.0}).diameters.tolist() == [100.0, 1.0, 50.0]
    # an even max_kernel_size also draws max_kernel_size + 1, as the reference's own list does (color_transform.py:125)
    assert set(np.unique(draws_reference(_aug(max_kernel_size=4), np.arange(500))['k'])) == {1, 3, 5}
    # the val pipeline keeps refusing what it cannot do
    with pytest.raises(NotImplementedError):
        PatchPipeline.from_cfg(TRAIN_PIPELINE, None)


def _with(kind, **changes):
    return [dict(s, **changes) if s['type'] == kind else s for s in TRAIN_PIPELINE]


def _plus(step, before='Resize'):
    i = [s['type'] for s in TRAIN_PIPELINE].index(before)
    return TRAIN_PIPELINE[:i] + [step] + TRAIN_PIPELINE[i:]


@pytest.mark.parametrize('pipeline,name', [
    (_plus(dict(type='RandomBackground', background_dir='x')), 'RandomBackground'),
    (_plus(dict(type='RandomSharpness')), 'RandomSharpness'),
    (_plus(dict(type='RandomGray')), 'RandomGray'),
    (_plus(dict(type='RandomOcclusion')), 'RandomOcclusion'),
    (_plus(dict(type='RandomOcclusionV2')), 'RandomOcclusionV2'),
    (_with('Collect', annot_keys=['ref_rotations', 'depths']), 'depth'),
    (_with('Resize', keep_ratio=False), r'Resize\(keep_ratio=False\)'),
    (_with('RemapPose', keep_intrinsic=True), 'RemapPose'),
    (_with('RemapPose', dst_k=[[1, 0, 0], [0, 1, 0], [0, 0, 1]]), 'RemapPose'),
    (_with('ComputeBbox', clip_border=True), r'ComputeBbox\(clip_border=True\)'),
    (_with('ComputeBbox', filter_invalid=True), r'ComputeBbox\(filter_invalid=True\)'),
    (_with('Crop', crop_bbox_field='gt_bboxes'), 'crop_bbox_field'),
    (_plus(dict(type='Mystery')), 'Mystery'),
    ([s for s in TRAIN_PIPELINE if s['type'] != 'PoseJitter'], 'without PoseJitter'),
    (_plus(dict(type='RandomHSV', h_ratio=0.1, s_ratio=0.1, v_ratio=0.1), before='Crop')[:6]
     + [s for s in TRAIN_PIPELINE[5:] if s['type'] != 'RandomHSV'], 'order'),
])
def test_from_cfg_refuses_by_name(pipeline, name):
    with pytest.raises(NotImplementedError, match=name):
        TrainPatchPipeline.from_cfg(pipeline, _store(21))


def test_aug_params_are_validated_by_name():
    for kw, word in ((dict(seed=-1), 'seed'), (dict(jitter_angle_dis=(0, -1)), 'jitter_angle_dis'),
                     (dict(angle_limit=-3), 'angle_limit'), (dict(add_limit=float('nan')), 'add_limit'),
                     (dict(size_range=(1.2, 1.0)), 'size_range'), (dict(h_ratio=1.0), 'h_ratio'),
                     (dict(s_ratio=-0.1), 's_ratio'), (dict(hsv_p=1.5), 'hsv_p'), (dict(noise_ratio=-1), 'noise_ratio'),
                     (dict(max_tries=0), 'max_tries'), (dict(max_kernel_size=17), 'max_kernel_size')):
        with pytest.raises(_lib.ScflowHipError, match=word):
            ops.patch_aug_params(**kw)
    a = ops.patch_aug_params(angle_limit=None, max_kernel_size=5.)
    assert a.angle_limit < 0 and a.max_kernel_size == 5


def test_c_entries_check_their_arguments_and_the_struct_layout():
    lib = _lib.load()
    assert lib.scf_patch_train_workspace_bytes(0) < 0
    assert lib.scf_patch_train_workspace_bytes(5) == 5 * 128 == lib.scf_patch_workspace_bytes(5) * 2
    p, a = ops.patch_params(), ops.patch_aug_params()
    assert lib.scf_pose_jitter(None, None, None, None, None, 1, 1, C.byref(a), 0, None, *[None] * 7, None) < 0
    assert lib.scf_patch_boxes_train(None, None, None, None, None, None, 0, 480, 640, C.byref(p), C.byref(a), 0, None,
                                     *[None] * 8, None) < 0
    assert lib.scf_patch_extract_train(None, 1, 480, 640, None, None, 1, None, C.byref(p), C.byref(a), None, None, None) < 0
    bad = ops.patch_aug_params()
    bad.max_kernel_size = 16
    assert lib.scf_patch_extract_train(1, 1, 480, 640, 1, None, 1, 1, C.byref(p), C.byref(bad), 1, None, None) < 0
    assert lib.scf_patch_extract_train(1, 1, 480, 640, 1, 1, 1, 1, C.byref(p), C.byref(a), 1, None, None) < 0   # masks without mask_out
    # the ctypes mirror has the C struct's size
    import os, subprocess, tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = '#include "scflow_hip.h"\n#include <stdio.h>\nint main(){printf("%zu\\n", sizeof(scf_patch_aug_params));return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, 't.c'), 'w').write(src)
        subprocess.run(['gcc', '-I', os.path.join(root, 'include'), os.path.join(d, 't.c'), '-o', os.path.join(d, 't')], check=True)
        size = int(subprocess.run([os.path.join(d, 't')], capture_output=True, text=True, check=True).stdout)
    assert size == C.sizeof(_lib.PatchAugParams)


def test_route_model():
    """scf_patch_train_route: the footprint bound of patch_train.hip against the 50 KiB of LDS a block has."""
    def need(ph, pw, nh, nw, k):
        cap = lambda src, dst, tile: min(src, (tile - 1) * src // dst + 4)
        fh, fw, r = cap(ph, nh, 16), cap(pw, nw, 64), k // 2
        return 4 * (fh + 2 * r) * (fw + 2 * r) + (6 * (fh + 2 * r) * fw + 8 if r else 0)
    for shape in ((100, 100, 256, 256), (61, 49, 32, 26), (512, 512, 256, 256), (400, 400, 16, 16), (700, 700, 256, 256),
                  (1, 30, 1, 32), (2000, 2000, 256, 256), (3, 3, 17, 17)):
        for k in (1, 3, 5):
            want = 'lds' if need(*shape, k) <= 51200 else 'direct'
            assert ops.patch_train_route(*shape, k) == want, (shape, k)
    assert ops.patch_train_route(100, 100, 256, 256, 5) == 'lds' and ops.patch_train_route(400, 400, 16, 16, 1) == 'direct'
    assert ops.patch_train_route(2 ** 21, 10, 256, 1, 1) == 'direct'
    for bad in ((0, 1, 1, 1, 1), (1, 1, 1, 1, 2), (1, 1, 1, 1, 17), (1, 1, 0, 1, 1)):
        with pytest.raises(_lib.ScflowHipError):
            ops.patch_train_route(*bad)


def test_train_ops_reject_cpu_tensors():
    a, p = ops.patch_aug_params(add_limit=None), ops.patch_params()
    R, t, K = torch.eye(3)[None], torch.zeros(1, 3), torch.eye(3)[None]
    with pytest.raises(_lib.ScflowHipError):
        ops.pose_jitter(None, None, None, R, t, a)
    with pytest.raises(_lib.ScflowHipError):
        ops.patch_boxes_train(None, None, None, None, K, (480, 640), p, a, crop_rects=torch.zeros(1, 4, dtype=torch.int32))
    with pytest.raises(_lib.ScflowHipError):
        ops.extract_patches_train(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), torch.zeros(1, dtype=torch.int32),
                                  torch.zeros(128, dtype=torch.uint8), p, a)
    with pytest.raises(_lib.ScflowHipError, match='add_limit'):
        ops.pose_jitter(None, None, None, R, t, ops.patch_aug_params())
