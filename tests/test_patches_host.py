"""CPU: the patch pipeline's host side -- PatchPipeline.from_cfg, its option checks, the C entry points' argument
checks -- and ``patch_reference``, a numpy restatement of the semantics patch.hip states (integer arithmetic for the
pixels, float64 for the geometry), proven here on closed forms and used by test_gpu_patches.py as the yardstick."""
import ctypes as C
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import scflow_amd
from scflow_amd import _lib, ops
from scflow_amd.mesh import MeshStore, icosphere, make_mesh
from scflow_amd.patches import PatchPipeline, TrainPatchPipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')

# the shipped val_pipeline's settings
SHIPPED = dict(size=(256, 256), img_scale=256, size_ratio=1.1, aspect_ratio=1.0, keep_ratio=False, min_expand=0.0,
               clip_border=False, fix_clip_border_quirk=False, center=True, crop_pad_val=(128, 128, 128),
               pad_val=(128, 128, 128), mean=(0., 0., 0.), std=(255., 255., 255.), to_rgb=True, vertex_stride=1)
EDGE_LIMIT = 2.0 ** 29


def _cfg(**kw):
    cfg = dict(SHIPPED)
    cfg.update(kw)
    for key in ('crop_pad_val', 'pad_val'):
        if np.isscalar(cfg[key]):
            cfg[key] = (cfg[key],) * 3
    return cfg


# ------------------------------------------------------------------------------------------- restatement
def box_reference(verts, R, t, K, stride=1):
    """item 1 in float64 from the fp32 inputs -> (box float64 (4,), valid)."""
    X = np.asarray(verts, np.float32)[::stride].astype(np.float64)
    if len(X) == 0:
        return np.zeros(4), False
    R, t, K = (np.asarray(a, np.float32).astype(np.float64) for a in (R, t, K))
    p = (X @ R.reshape(3, 3).T + t.reshape(3)) @ K.reshape(3, 3).T
    if not (p[:, 2] > 0).all():
        return np.zeros(4), False
    u, v = p[:, 0] / (p[:, 2] + 1e-8), p[:, 1] / (p[:, 2] + 1e-8)
    box = np.array([u.min(), v.min(), u.max(), v.max()])
    return box, bool(np.isfinite(box).all())


def crop_edges(box32, frame_hw, cfg, clip=True):
    """item 2 up to the truncation: the four float64 edges (x1, y1, x2, y2) from the float32 box (``clip=False``: as
    they are before clip_border clips them)."""
    x1, y1, x2, y2 = (np.float32(b) for b in box32)
    xc, yc = np.float64((x1 + x2) / np.float32(2)), np.float64((y1 + y2) / np.float32(2))
    bw, bh = np.float64(x2 - x1), np.float64(y2 - y1)
    if not cfg['keep_ratio']:
        bw = max(bw, bh * cfg['aspect_ratio'])
        bh = max(bw / cfg['aspect_ratio'], bh)
    sw, sh = bw * cfg['size_ratio'], bh * cfg['size_ratio']
    if cfg['min_expand'] > 0:
        bw, bh = max(bw + 2 * cfg['min_expand'], sw), max(bh + 2 * cfg['min_expand'], sh)
    else:
        bw, bh = sw, sh
    e = [xc - bw / 2, yc - bh / 2, xc + bw / 2, yc + bh / 2]
    if cfg['clip_border']:
        if not cfg['fix_clip_border_quirk']:
            e[3] = np.float64(y2) + bh / 2
        h, w = frame_hw
        if not clip:
            return np.array(e, np.float64)
        e = [np.clip(e[0], 0, w), np.clip(e[1], 0, h), np.clip(e[2], 0, w), np.clip(e[3], 0, h)]
    return np.array(e, np.float64)


def geometry_reference(K, frame_hw, cfg, box32=None, rect=None, valid=True):
    """items 2, 3 (sizes) and 5 for one object -> dict(valid, crop, s, new_w, new_h, left, top, tm, k, edges); tm and
    k are float64 (round once to float32 to compare)."""
    K = np.asarray(K, np.float32).astype(np.float64).reshape(3, 3)
    edges = np.zeros(4)
    ok = bool(valid)
    x1 = y1 = x2 = y2 = 0
    if ok and rect is None:
        edges = crop_edges(box32, frame_hw, cfg)
        ok = bool((np.abs(edges) < EDGE_LIMIT).all())
        if ok:
            x1, y1, x2, y2 = (int(np.trunc(e)) for e in edges)
    elif ok:
        x1, y1, x2, y2 = (int(r) for r in rect)
        ok = x1 > -EDGE_LIMIT and y1 > -EDGE_LIMIT and x2 < EDGE_LIMIT and y2 < EDGE_LIMIT
    ok = ok and x2 >= x1 and y2 >= y1
    H, W = cfg['size']
    s, new_w, new_h, left, top = 1.0, 0, 0, 0, 0
    if ok:
        pw, ph = x2 - x1 + 1, y2 - y1 + 1
        s = float(cfg['img_scale']) / float(max(ph, pw))
        new_w, new_h = int(pw * s + 0.5), int(ph * s + 0.5)
        ok = 1 <= new_w <= W and 1 <= new_h <= H
        if ok and cfg['center']:
            top, left = int(H / 2 - new_h / 2), int(W / 2 - new_w / 2)
    if not ok:
        x1 = y1 = x2 = y2 = new_w = new_h = left = top = 0
        s = 1.0
    tx = s * float(-x1) + float(left) if ok else 0.0
    ty = s * float(-y1) + float(top) if ok else 0.0
    tm = np.array([[s, 0, tx], [0, s, ty], [0, 0, 1]], np.float64)
    k = np.stack([s * K[0] + tx * K[2], s * K[1] + ty * K[2], K[2]])
    return dict(valid=ok, crop=(x1, y1, x2, y2), s=s, new_w=new_w, new_h=new_h, left=left, top=top, tm=tm, k=k, edges=edges)


def axis_coef(src, dst):
    """item 3, one axis: source index, fixed-point coefficients and the float32 fraction for every destination index."""
    d = np.arange(dst, dtype=np.float64)
    f = ((d + 0.5) * (np.float64(src) / np.float64(dst)) - 0.5).astype(np.float32)
    fl = np.floor(f)
    i = fl.astype(np.int64)
    f = (f - fl).astype(np.float32)
    lo = i < 0
    i[lo], f[lo] = 0, 0
    hi = i >= src - 1
    i[hi], f[hi] = src - 1, 0
    a0 = np.rint((np.float32(1) - f) * np.float32(2048)).astype(np.int64)
    a1 = np.rint(f * np.float32(2048)).astype(np.int64)
    return i, a0, a1, f


def crop_reference(frame, rect, fill):
    """the (ph, pw, 3) uint8 patch of ``rect`` (ends inclusive), ``fill`` outside the frame."""
    x1, y1, x2, y2 = rect
    Hf, Wf = frame.shape[:2]
    patch = np.empty((y2 - y1 + 1, x2 - x1 + 1, 3), np.uint8)
    patch[:] = np.asarray(fill, np.uint8)
    ya, yb, xa, xb = max(y1, 0), min(y2, Hf - 1), max(x1, 0), min(x2, Wf - 1)
    if ya <= yb and xa <= xb:
        patch[ya - y1:yb - y1 + 1, xa - x1:xb - x1 + 1] = frame[ya:yb + 1, xa:xb + 1]
    return patch


def resize_reference(patch, new_h, new_w):
    """OpenCV's generic 8-bit INTER_LINEAR as patch.hip states it, integer arithmetic -> (new_h, new_w, 3) uint8."""
    ph, pw = patch.shape[:2]
    iy, b0, b1, _ = axis_coef(ph, new_h)
    ix, a0, a1, _ = axis_coef(pw, new_w)
    iy1, ix1 = np.minimum(iy + 1, ph - 1), np.minimum(ix + 1, pw - 1)
    P = patch.astype(np.int64)
    a0, a1 = a0[None, :, None], a1[None, :, None]
    S0 = P[iy][:, ix] * a0 + P[iy][:, ix1] * a1
    S1 = P[iy1][:, ix] * a0 + P[iy1][:, ix1] * a1
    b0, b1 = b0[:, None, None], b1[:, None, None]
    val = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2
    return np.minimum(val, 255).astype(np.uint8)


def resize_float64(patch, new_h, new_w):
    """float64 bilinear with the same coordinates (no fixed point)."""
    ph, pw = patch.shape[:2]
    iy, _, _, fy = axis_coef(ph, new_h)
    ix, _, _, fx = axis_coef(pw, new_w)
    iy1, ix1 = np.minimum(iy + 1, ph - 1), np.minimum(ix + 1, pw - 1)
    P = patch.astype(np.float64)
    fx, fy = fx.astype(np.float64)[None, :, None], fy.astype(np.float64)[:, None, None]
    top = P[iy][:, ix] * (1 - fx) + P[iy][:, ix1] * fx
    bot = P[iy1][:, ix] * (1 - fx) + P[iy1][:, ix1] * fx
    return top * (1 - fy) + bot * fy


def pixels_reference(frame, geo, cfg):
    """items 2 (pixels), 3, 4 and 6 for one object -> (3, H, W) float32."""
    H, W = cfg['size']
    img = np.empty((H, W, 3), np.uint8)
    img[:] = np.asarray(cfg['pad_val'], np.uint8)
    if geo['valid'] and frame is not None:
        small = resize_reference(crop_reference(frame, geo['crop'], cfg['crop_pad_val']), geo['new_h'], geo['new_w'])
        img[geo['top']:geo['top'] + geo['new_h'], geo['left']:geo['left'] + geo['new_w']] = small
    if cfg['to_rgb']:
        img = img[..., ::-1]
    mean = np.asarray(cfg['mean'], np.float32)
    inv = (1.0 / np.asarray(cfg['std'], np.float32).astype(np.float64)).astype(np.float32)
    return np.ascontiguousarray(((img.astype(np.float32) - mean) * inv).transpose(2, 0, 1))


def patch_reference(frames, frame_index, K, cfg, meshes=None, labels=None, R=None, t=None, crop_rects=None):
    """the whole pipeline for N objects.  ``meshes``: {label: verts (V,3) float32}.  -> dict(img (N,3,H,W) float32,
    crop (N,4), scale (N) float64, tm / k (N,3,3) float64, valid (N), edges (N,4) float64 crop edges before the
    truncation, box (N,4) float64 box corners)."""
    n = len(K)
    out = dict(img=[], crop=[], scale=[], tm=[], k=[], valid=[], edges=[], box=[])
    for i in range(n):
        if crop_rects is not None:
            box = np.zeros(4)
            geo = geometry_reference(K[i], frames.shape[1:3], cfg, rect=crop_rects[i])
        else:
            verts = meshes.get(int(labels[i]), np.zeros((0, 3), np.float32))
            box, ok = box_reference(verts, R[i], t[i], K[i], cfg['vertex_stride'])
            geo = geometry_reference(K[i], frames.shape[1:3], cfg, box32=box.astype(np.float32), valid=ok)
        fi = int(frame_index[i])
        frame = frames[fi] if 0 <= fi < len(frames) else None
        out['img'].append(pixels_reference(frame, geo, cfg))
        out['crop'].append(geo['crop'])
        out['scale'].append(geo['s'])
        out['tm'].append(geo['tm'])
        out['k'].append(geo['k'])
        out['valid'].append(int(geo['valid']))
        out['edges'].append(geo['edges'])
        out['box'].append(box)
    return {k: np.stack([np.asarray(x) for x in v]) for k, v in out.items()}


# ------------------------------------------------------------------------------- the restatement itself
K0 = np.array([[600., 0, 320.5], [0, 590., 240.25], [0, 0, 1]], np.float32)


def _frame(h=480, w=640, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (1, h, w, 3), dtype=np.uint8)


def _one(frames, rect, **kw):
    return patch_reference(frames, [0], K0[None], _cfg(**kw), crop_rects=[rect])


def test_reference_crop_rule_by_hand():
    # box (100.5, 50.25, 200.5, 120.25): xc = 150.5, yc = 85.25, bw = 100, bh = 70 -> square 100 -> x 1.1 (binary: just
    # above 110) -> edges 95.49999..., 30.25, 205.50000..., 140.25 -> truncated
    e = crop_edges((100.5, 50.25, 200.5, 120.25), (480, 640), _cfg())
    assert e == pytest.approx([95.5, 30.25, 205.5, 140.25], abs=1e-9)
    g = geometry_reference(K0, (480, 640), _cfg(), box32=np.array([100.5, 50.25, 200.5, 120.25], np.float32))
    assert g['crop'] == (95, 30, 205, 140) and g['valid']
    assert g['s'] == 256 / 111 and (g['new_w'], g['new_h'], g['left'], g['top']) == (256, 256, 0, 0)
    # keep_ratio: the box's own aspect; min_expand wins over a small ratio
    e = crop_edges((100, 50, 200, 120), (480, 640), _cfg(keep_ratio=True, size_ratio=1.0))
    assert list(e) == [100, 50, 200, 120]
    e = crop_edges((100, 50, 200, 120), (480, 640), _cfg(keep_ratio=True, size_ratio=1.0, min_expand=8))
    assert list(e) == [92, 42, 208, 128]
    # truncation is toward zero: -0.5 -> 0, not -1
    g = geometry_reference(K0, (480, 640), _cfg(size_ratio=1.0), box32=np.array([-10.5, -10.5, 9.5, 9.5], np.float32))
    assert g['crop'] == (-10, -10, 9, 9)
    # clip_border: clipped to [0, w] / [0, h]; the lower edge is the BOX's y2 + bh/2 unless the quirk is fixed
    box = (600, 400, 700, 460)
    e = crop_edges(box, (480, 640), _cfg(clip_border=True, size_ratio=1.0))
    assert list(e) == [600, 380, 640, 480]                    # y2 + bh/2 = 460 + 50 = 510 -> 480
    box = (100, 100, 200, 160)
    assert crop_edges(box, (480, 640), _cfg(clip_border=True, size_ratio=1.0))[3] == 160 + 50
    assert crop_edges(box, (480, 640), _cfg(clip_border=True, size_ratio=1.0, fix_clip_border_quirk=True))[3] == 130 + 50


def test_reference_identity_rectangle_reproduces_the_frame():
    frames = _frame()
    x1, y1 = 123, 77
    out = _one(frames, (x1, y1, x1 + 255, y1 + 255))
    want = frames[0, y1:y1 + 256, x1:x1 + 256, ::-1].astype(np.float32) * np.float32(1 / 255.)
    assert np.array_equal(out['img'][0], want.transpose(2, 0, 1))
    assert out['scale'][0] == 1.0 and out['valid'][0] == 1
    k = K0.astype(np.float64).copy()
    k[0, 2] -= x1
    k[1, 2] -= y1
    assert np.array_equal(out['k'][0], k)
    assert np.array_equal(out['tm'][0], [[1, 0, -x1], [0, 1, -y1], [0, 0, 1]])
    # BGR kept, a mean and a std
    out = _one(frames, (x1, y1, x1 + 255, y1 + 255), to_rgb=False, mean=(1., 2., 3.), std=(2., 4., 8.))
    want = (frames[0, y1:y1 + 256, x1:x1 + 256].astype(np.float32) - np.float32([1, 2, 3])) * np.float32([.5, .25, .125])
    assert np.array_equal(out['img'][0], want.transpose(2, 0, 1))


def test_reference_exact_halving_is_the_rounded_mean():
    frames = _frame(600, 700, seed=1)
    x1, y1 = 40, 30
    out = _one(frames, (x1, y1, x1 + 511, y1 + 511))
    src = frames[0, y1:y1 + 512, x1:x1 + 512].astype(np.int64)
    want = (src[0::2, 0::2] + src[0::2, 1::2] + src[1::2, 0::2] + src[1::2, 1::2] + 2) >> 2
    got = np.rint(out['img'][0] * 255).astype(np.int64)[::-1].transpose(1, 2, 0)       # back to BGR HWC grey levels
    assert np.array_equal(got, want)
    assert out['scale'][0] == 0.5 and np.array_equal(out['k'][0][0], [300., 0, 0.5 * 320.5 - 20])


@pytest.mark.parametrize('rect,inside', [
    ((-100, 50, 155, 305), (slice(None), slice(100, 256))),              # over the left border
    ((500, 50, 755, 305), (slice(None), slice(0, 140))),                 # right
    ((100, -56, 355, 199), (slice(56, 256), slice(None))),               # top
    ((100, 300, 355, 555), (slice(0, 180), slice(None))),                # bottom
    ((-40, -30, 215, 225), (slice(30, 256), slice(40, 256))),            # top-left corner
    ((450, 290, 705, 545), (slice(0, 190), slice(0, 190))),              # bottom-right corner
])
def test_reference_fills_outside_the_frame_with_128(rect, inside):
    frames = np.random.default_rng(2).integers(0, 100, (1, 480, 640, 3), dtype=np.uint8)    # no 128 in the frame
    out = _one(frames, rect)
    grey = np.rint(out['img'][0] * 255).astype(np.int64)
    mask = np.zeros((256, 256), bool)
    mask[inside] = True
    assert (grey[:, ~mask] == 128).all() and (grey[:, mask] < 100).all()
    x1, y1 = rect[:2]
    ys, xs = np.nonzero(mask)
    assert np.array_equal(grey[:, ys, xs], frames[0, ys + y1, xs + x1, ::-1].T)


def test_reference_rectangle_wholly_outside_and_invalid_objects():
    frames = np.random.default_rng(2).integers(0, 100, (1, 480, 640, 3), dtype=np.uint8)
    out = _one(frames, (700, 100, 955, 355))
    assert out['valid'][0] == 1 and (np.rint(out['img'][0] * 255) == 128).all()
    out = _one(frames, (10, 10, 5, 20), pad_val=(1, 2, 3))                   # x2 < x1
    assert out['valid'][0] == 0 and out['crop'][0].tolist() == [0, 0, 0, 0] and out['scale'][0] == 1.0
    assert np.array_equal(np.rint(out['img'][0] * 255)[:, 0, 0], [3, 2, 1])  # pad_val is BGR, the output RGB
    assert np.array_equal(out['k'][0], K0.astype(np.float64)) and np.array_equal(out['tm'][0], np.eye(3))
    out = _one(frames, (0, 0, 0, 999))                                       # new_w = int(0.256 + 0.5) = 0
    assert out['valid'][0] == 0
    # behind the camera, an empty class, a frame index out of range
    verts = icosphere(1, 50.0)[0]
    R, t = np.eye(3, dtype=np.float32), np.array([0, 0, 40.], np.float32)     # some vertices at z <= 0
    out = patch_reference(frames, [0, 0, 5], np.stack([K0] * 3), _cfg(), meshes={0: verts}, labels=[0, 3, 0],
                          R=np.stack([R] * 3), t=np.stack([t, t + [0, 0, 500], t + [0, 0, 500]]))
    assert out['valid'].tolist() == [0, 0, 1]
    assert (np.rint(out['img'][2] * 255) == 128).all()


def test_reference_one_pixel_of_padding():
    frames = _frame(seed=3)
    out = _one(frames, (100, 100, 355, 354))                    # 256 wide, 255 high: s = 1, top = int(128 - 127.5) = 0
    grey = np.rint(out['img'][0] * 255).astype(np.int64)
    assert np.array_equal(grey[:, :255], frames[0, 100:355, 100:356, ::-1].transpose(2, 0, 1)) and (grey[:, 255] == 128).all()
    out = _one(frames, (100, 100, 354, 355))                    # 255 wide: the last column pads
    grey = np.rint(out['img'][0] * 255).astype(np.int64)
    assert np.array_equal(grey[:, :, :255], frames[0, 100:356, 100:355, ::-1].transpose(2, 0, 1)) and (grey[:, :, 255] == 128).all()
    g = geometry_reference(K0, (480, 640), _cfg(), rect=(10, 10, 209, 208))       # 200 x 199: s = 1.28, new_h = 255
    assert (g['new_w'], g['new_h'], g['left'], g['top']) == (256, 255, 0, 0)
    g = geometry_reference(K0, (480, 640), _cfg(), rect=(10, 10, 109, 208))       # 100 x 199: new_w = int(128.64...) = 129
    assert (g['new_w'], g['new_h'], g['left'], g['top']) == (129, 256, 63, 0)     # left = int(128 - 64.5)
    assert g['tm'][0, 2] == 63 - g['s'] * 10
    g = geometry_reference(K0, (480, 640), _cfg(center=False), rect=(10, 10, 109, 208))
    assert (g['left'], g['top']) == (0, 0)


def test_reference_fixed_point_stays_within_one_grey_level_of_float64():
    g = np.random.default_rng(4)
    worst = 0.0
    for src in (57, 100, 173, 255, 300, 437, 611):
        patch = g.integers(0, 256, (src, src - 3, 3), dtype=np.uint8)
        new_w = int((src - 3) * (256 / src) + 0.5)
        got = resize_reference(patch, 256, new_w).astype(np.float64)
        worst = max(worst, float(np.abs(got - resize_float64(patch, 256, new_w)).max()))
    print(f'fixed point against float64 bilinear: worst {worst:.3f} grey levels')
    assert worst < 1.0


# ---------------------------------------------------------------------------------------- PatchPipeline
def _val_pipeline():
    return json.load(open(os.path.join(GOLDEN, 'val_pipeline.json')))


def _store():
    return MeshStore({0: make_mesh(*icosphere(1, 50.0))})


def test_from_cfg_reads_the_shipped_pipeline():
    pipe = PatchPipeline.from_cfg(_val_pipeline(), _store())
    p = pipe.params
    assert (p.out_h, p.out_w, p.resize) == (256, 256, 256)
    assert (p.size_ratio, p.aspect_ratio, p.min_expand) == (1.1, 1.0, 0.0)
    assert (p.keep_ratio, p.clip_border, p.fix_clip_border_quirk, p.center, p.to_rgb, p.vertex_stride) == (0, 0, 0, 1, 1, 1)
    assert list(p.crop_pad_val) == [128] * 3 and list(p.pad_val) == [128] * 3
    assert list(p.mean) == [0.] * 3 and list(p.std) == [255.] * 3
    assert pipe.img_norm_cfg == dict(mean=[0., 0., 0.], std=[255., 255., 255.], to_rgb=True)
    assert scflow_amd.PatchPipeline is PatchPipeline
    same = PatchPipeline(_store())                             # the keyword defaults are the shipped settings
    assert bytes(same.params) == bytes(p)
    pipe = PatchPipeline.from_cfg(_val_pipeline(), _store(), vertex_stride=4, fix_clip_border_quirk=True)
    assert pipe.params.vertex_stride == 4 and pipe.params.fix_clip_border_quirk == 1


def _edit(kind, **kw):
    steps = [dict(s) for s in _val_pipeline()]
    for s in steps:
        if s['type'] == kind:
            s.update(kw)
    return steps


@pytest.mark.parametrize('steps,word', [
    (_edit('Crop', size_range=(1.0, 1.25)), 'size_range'),
    (_edit('Resize', keep_ratio=False), 'keep_ratio=False'),
    (_edit('Resize', img_scale=(256, 320)), 'img_scale'),
    (_edit('RemapPose', keep_intrinsic=True), 'keep_intrinsic'),
    (_edit('RemapPose', dst_k=[1, 0, 0, 0, 1, 0, 0, 0, 1]), 'target_intrinsic'),
    (_val_pipeline() + [dict(type='RandomHSV', h_ratio=0.2)], 'RandomHSV'),
    (_edit('Collect', annot_keys=['k', 'labels', 'gt_masks']), 'gt_masks'),
    (_edit('Collect', annot_keys=['k', 'labels', 'depths']), 'depths'),
    (_edit('ComputeBbox', clip_border=True), 'ComputeBbox'),
    (_edit('ComputeBbox', filter_invalid=True), 'filter_invalid'),
    (_edit('Crop', crop_bbox_field='det_bboxes'), 'crop_bbox_field'),
    ([s for s in _val_pipeline() if s['type'] != 'RemapPose'], 'RemapPose'),
])
def test_from_cfg_refuses_what_it_cannot_do(steps, word):
    with pytest.raises(NotImplementedError, match=word):
        PatchPipeline.from_cfg(steps, _store())


@pytest.mark.parametrize('case', ['keep_ratio', 'img_scale', 'keep_intrinsic', 'dst_k', 'unknown', 'no_normalize'])
@pytest.mark.parametrize('name', ['PatchPipeline', 'TrainPatchPipeline'])
def test_shared_refusals_carry_the_asked_class_name(name, case):
    """the two classes refuse these through one base class: the message starts with the class that was asked."""
    if name == 'PatchPipeline':
        cls, steps = PatchPipeline, _val_pipeline()
    else:
        from test_patches_train_host import TRAIN_PIPELINE              # that module imports this one
        cls, steps = TrainPatchPipeline, [dict(s) for s in TRAIN_PIPELINE]

    def edit(kind, **kw):
        return [dict(s, **kw) if s['type'] == kind else s for s in steps]
    steps = dict(keep_ratio=edit('Resize', keep_ratio=False), img_scale=edit('Resize', img_scale=(256, 320)),
                 keep_intrinsic=edit('RemapPose', keep_intrinsic=True),
                 dst_k=edit('RemapPose', dst_k=[1, 0, 0, 0, 1, 0, 0, 0, 1]), unknown=steps + [dict(type='Mystery')],
                 no_normalize=[s for s in steps if s['type'] != 'Normalize'])[case]
    with pytest.raises(NotImplementedError) as err:
        cls.from_cfg(steps, _store())
    assert str(err.value).startswith(name + ': ')


def test_patch_params_are_checked_by_name():
    for kw, word in ((dict(resize=300), 'resize'), (dict(out_size=(0, 256)), 'out_size'), (dict(vertex_stride=0), 'vertex_stride'),
                     (dict(size_ratio=0.), 'size_ratio'), (dict(min_expand=-1.), 'min_expand'), (dict(pad_val=300), 'pad_val'),
                     (dict(crop_pad_val=(1, 2)), 'crop_pad_val'), (dict(std=(255., 0., 255.)), 'std')):
        with pytest.raises(_lib.ScflowHipError, match=word):
            ops.patch_params(**kw)
    with pytest.raises(TypeError):
        PatchPipeline('meshes/')


def test_ops_reject_cpu_tensors():
    p = ops.patch_params()
    with pytest.raises(_lib.ScflowHipError):
        ops.patch_boxes(None, None, None, None, torch.zeros(2, 3, 3), (480, 640), p, crop_rects=torch.zeros(2, 4, dtype=torch.int32))
    with pytest.raises(_lib.ScflowHipError):
        ops.extract_patches(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), torch.zeros(1, dtype=torch.int32),
                            torch.zeros(64, dtype=torch.uint8), p)


# ---------------------------------------------------------------------------------------------- C entries
def test_c_entries_check_their_arguments():
    lib = _lib.load()
    assert lib.scf_patch_workspace_bytes(1) == 64 and lib.scf_patch_workspace_bytes(32) == 32 * 64
    assert lib.scf_patch_workspace_bytes(0) == -1 and lib.scf_patch_workspace_bytes(-5) == -1
    p = ops.patch_params()
    fake = 16     # never dereferenced: every check fails first
    m = _lib.MeshStore(fake, fake, fake, fake, fake, fake, 1, 1)

    def boxes(mesh=m, labels=fake, R=fake, t=fake, K=fake, crop_in=None, n=1, hf=480, wf=640, params=p, box=None, crop=fake,
              scale=fake, tm=fake, k=fake, valid=fake, ws=fake):
        return lib.scf_patch_boxes(None if mesh is None else C.byref(mesh), labels, R, t, K, crop_in, n, hf, wf,
                                   None if params is None else C.byref(params), box, crop, scale, tm, k, valid, ws, None)

    for bad in (dict(mesh=None), dict(labels=None), dict(R=None), dict(t=None), dict(K=None), dict(n=0), dict(hf=0),
                dict(wf=20000), dict(params=None), dict(crop=None), dict(scale=None), dict(tm=None), dict(k=None),
                dict(valid=None), dict(ws=None), dict(mesh=_lib.MeshStore(fake, fake, fake, fake, fake, fake, 0, 1)),
                dict(mesh=_lib.MeshStore(None, fake, fake, fake, fake, fake, 1, 1)), dict(crop_in=fake, K=None)):
        assert boxes(**bad) == -1, bad

    def extract(frames=fake, f=1, hf=480, wf=640, index=fake, n=1, ws=fake, params=p, out=fake):
        return lib.scf_patch_extract(frames, f, hf, wf, index, n, ws, None if params is None else C.byref(params), out, None)

    for bad in (dict(frames=None), dict(f=0), dict(hf=-1), dict(wf=0), dict(index=None), dict(n=0), dict(n=70000),
                dict(ws=None), dict(params=None), dict(out=None)):
        assert extract(**bad) == -1, bad
    for field, value in (('out_h', 0), ('out_w', 9000), ('resize', 0), ('resize', 257), ('vertex_stride', 0),
                         ('size_ratio', 0.0), ('size_ratio', float('nan')), ('aspect_ratio', -1.0), ('min_expand', -1.0)):
        q = ops.patch_params()
        setattr(q, field, value)
        assert boxes(params=q) == -1 and extract(params=q) == -1, field
    for field, idx, value in (('pad_val', 1, 256), ('crop_pad_val', 0, -1), ('std', 2, 0.0), ('mean', 0, float('inf'))):
        q = ops.patch_params()
        getattr(q, field)[idx] = value
        assert boxes(params=q) == -1 and extract(params=q) == -1, field


def test_patch_struct_layout_matches_c():
    src = ('#include "scflow_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %zu %zu\\n", '
           'sizeof(scf_patch_params), offsetof(scf_patch_params, out_h), offsetof(scf_patch_params, crop_pad_val), '
           'offsetof(scf_patch_params, std));return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, 't.c')
        open(c, 'w').write(src)
        exe = os.path.join(d, 't')
        subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), c, '-o', exe], check=True)
        got = list(map(int, subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()))
    P = _lib.PatchParams
    assert got == [C.sizeof(P), P.out_h.offset, P.crop_pad_val.offset, P.std.offset]
