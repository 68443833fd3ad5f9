"""GPU: the patch pipeline (scflow_amd/csrc/patch.hip) against ``patch_reference`` of test_patches_host.py -- patches
bit for bit, crop rectangles exactly, box corners and intrinsics against float64 -- its hipGraph capture, and the
whole front end: frame + perturbed pose -> PatchPipeline -> format_data_test -> SCFlowRefiner.forward."""
import json
import os

import numpy as np
import pytest
import torch

import scflow_amd
from scflow_amd import ops
from scflow_amd.graph import GraphedPatches
from scflow_amd.mesh import MeshRenderer, MeshStore
from scflow_amd.patches import PatchPipeline

from test_patches_host import _cfg, box_reference, crop_edges, patch_reference
from test_render_host import SHIPPED as RENDER_SHIPPED, colored_icosphere, cube, look_at_pose

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# Worst |GPU fp32 box corner - float64 box corner| over the cases below, measured on the MI355X (patch
# pipeline): the test asserts three times that figure, capped at the 1e-2 px margin the crop-rectangle cases keep
# from the integers.
BOX_ERR_MEASURED = 1.93e-4
EDGE_MARGIN = 1e-2

MESHES = {0: colored_icosphere(3, 60.0), 2: colored_icosphere(2, 30.0), 3: cube(90.0)}      # class 1 is empty


def _k(f, hf, wf):
    return np.array([[f, 0, wf / 2 + 0.37], [0, f * 0.98, hf / 2 - 0.21], [0, 0, 1]], np.float32)


# (name, label, z, x offset and y offset in frame-width / frame-height units from the centre, expected valid)
CASES = [('up8', 2, 1240.0, 0.1, -0.1, 1), ('down3', 0, 115.0, 0.0, 0.0, 1), ('cube', 3, 420.0, -0.2, 0.15, 1),
         ('left', 0, 500.0, -0.5, 0.0, 1), ('right', 0, 500.0, 0.5, 0.1, 1), ('top', 3, 450.0, 0.1, -0.5, 1),
         ('bottom', 2, 300.0, -0.1, 0.5, 1), ('corner', 0, 400.0, 0.5, 0.5, 1), ('outside', 0, 500.0, 1.4, 0.2, 1),
         ('far_outside', 2, 500.0, -3.0, -2.5, 1), ('behind', 0, -500.0, 0.0, 0.0, 0), ('straddling', 0, 40.0, 0.0, 0.0, 0),
         ('empty_class', 1, 500.0, 0.0, 0.0, 0), ('label_out_of_range', 9, 500.0, 0.0, 0.0, 0)]


def _draw_objects(hf, wf, cfg, seed):
    """poses for CASES in a (hf, wf) frame; every case is re-drawn (jittered) until each float64 crop edge lies at
    least EDGE_MARGIN from an integer, so that the fp32 box cannot move a truncation.  No case is dropped."""
    g = np.random.default_rng(seed)
    K = _k(600.0, hf, wf)
    verts = {l: m.verts for l, m in MESHES.items()}
    Rs, ts, labels = [], [], []
    for name, label, z, ox, oy, want_valid in CASES:
        for attempt in range(1000):
            R, _ = look_at_pose(*g.uniform(-0.6, 0.6, 3), 1.0)
            zz = z * g.uniform(0.97, 1.03)
            t = np.array([(ox * wf + g.uniform(-8, 8)) * zz / 600.0, (oy * hf + g.uniform(-8, 8)) * zz / 588.0, zz], np.float32)
            box, ok = box_reference(verts.get(label, np.zeros((0, 3), np.float32)), R, t, K, cfg['vertex_stride'])
            assert ok == bool(want_valid), name
            if not ok:
                break
            e = crop_edges(box.astype(np.float32), (hf, wf), cfg, clip=False)      # a clipped edge is an integer itself
            if (np.abs(e - np.rint(e)) >= EDGE_MARGIN).all():
                break
        else:
            raise AssertionError(f'{name}: no draw kept its crop edges {EDGE_MARGIN} px from the integers')
        Rs.append(R)
        ts.append(t)
        labels.append(label)
    n = len(CASES)
    return np.stack(Rs), np.stack(ts), np.stack([K] * n), np.array(labels)


def _run(frames, frame_index, R, t, K, labels, cfg, store, crop_rects=None):
    kw = {k: v for k, v in cfg.items() if k not in ('size', 'img_scale')}
    params = ops.patch_params(cfg['size'], cfg['img_scale'], **kw)
    dev = lambda a, dt=None: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(DEV)
    if crop_rects is None:
        box = ops.patch_boxes(store.on(DEV), dev(labels), dev(R), dev(t), dev(K), frames.shape[1:3], params)
    else:
        box = ops.patch_boxes(None, None, None, None, dev(K), frames.shape[1:3], params, crop_rects=dev(crop_rects))
    img = ops.extract_patches(dev(frames), dev(frame_index, torch.int32), box['records'], params)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in dict(box, img=img).items() if k != 'records'}


def _ulp_close(got32, want64):
    want32 = want64.astype(np.float32)
    return np.abs(got32.astype(np.float64) - want32.astype(np.float64)) <= np.spacing(np.abs(want32)).astype(np.float64)


@pytest.mark.parametrize('hf,wf,cfg', [
    (480, 640, _cfg()),
    (600, 1000, _cfg()),
    (480, 640, _cfg(vertex_stride=3, size_ratio=1.25, crop_pad_val=(10, 20, 30), pad_val=(200, 100, 50), to_rgb=False,
                    mean=(123.675, 116.28, 103.53), std=(58.395, 57.12, 57.375), center=False)),
    (480, 640, _cfg(clip_border=True, keep_ratio=True, min_expand=6.0, size=(192, 320), img_scale=192)),
    (480, 640, _cfg(clip_border=True, fix_clip_border_quirk=True, aspect_ratio=1.5, size=(250, 250), img_scale=249)),
])
def test_patches_rectangles_boxes_and_intrinsics_vs_reference(hf, wf, cfg):
    store = MeshStore(MESHES)
    R, t, K, labels = _draw_objects(hf, wf, cfg, seed=hf + wf)
    g = np.random.default_rng(5)
    frames = g.integers(0, 256, (3, hf, wf, 3), dtype=np.uint8)
    n = len(labels)
    frame_index = g.permutation(np.arange(n) % 3)
    want = patch_reference(frames, frame_index, K, cfg, meshes={l: m.verts for l, m in MESHES.items()}, labels=labels,
                           R=R, t=t)
    got = _run(frames, frame_index, R, t, K, labels, cfg, store)
    names = [c[0] for c in CASES]
    assert want['valid'].tolist() == [c[5] for c in CASES]
    assert got['valid'].tolist() == want['valid'].tolist()
    # box corners: the kernel's fp32 projection against float64 from the same fp32 inputs
    ok = want['valid'] == 1
    err = np.abs(got['box'][ok].astype(np.float64) - want['box'][ok])
    worst = float(err.max())
    print(f'box corners {hf}x{wf}: worst |fp32 - fp64| = {worst:.3e} px '
          f'({float((err / np.spacing(np.abs(want["box"][ok]).astype(np.float32))).max()):.2f} fp32 ulp of the coordinate)')
    bound = min(3 * BOX_ERR_MEASURED, EDGE_MARGIN)
    assert worst <= bound
    assert (got['box'][~ok] == 0).all()
    # crop rectangles: exact
    for i in range(n):
        assert got['crop'][i].tolist() == list(want['crop'][i]), names[i]
    # scale, transform_matrix, k: within 1 fp32 ulp of float64 rounded once
    assert _ulp_close(got['scale'], want['scale']).all()
    assert _ulp_close(got['transform_matrix'], want['tm']).all()
    assert _ulp_close(got['k'], want['k']).all()
    # patches: bit for bit
    for i in range(n):
        same = got['img'][i] == want['img'][i]
        assert same.all(), f'{names[i]}: {int((~same).sum())} of {same.size} values differ'
    # the cases are what they claim to be
    if cfg == _cfg():
        s = dict(zip(names, want['scale']))
        assert 6.0 < s['up8'] < 10.0 and 1 / 4.0 < s['down3'] < 1 / 2.5, s
    pad = (np.asarray(cfg['pad_val'][::-1] if cfg['to_rgb'] else cfg['pad_val'], np.float32) - np.asarray(cfg['mean'], np.float32)) \
        * (1.0 / np.asarray(cfg['std'], np.float32).astype(np.float64)).astype(np.float32)
    for name in ('behind', 'straddling', 'empty_class', 'label_out_of_range'):
        assert (got['img'][names.index(name)] == pad[:, None, None]).all(), name


def test_caller_supplied_rectangles():
    """crop_rects in place of the box launch: no mesh, labels or poses."""
    g = np.random.default_rng(6)
    frames = g.integers(0, 256, (2, 480, 640, 3), dtype=np.uint8)
    rects = np.array([[123, 77, 378, 332], [40, 30, 551, 541 - 100], [-100, 50, 155, 305], [500, 290, 755, 545],
                      [700, 100, 955, 355], [10, 10, 5, 20], [0, 0, 0, 999], [300, 200, 331, 236], [5, 7, 617, 470]], np.int32)
    n = len(rects)
    K = np.stack([_k(600.0, 480, 640)] * n)
    frame_index = np.arange(n) % 2
    cfg = _cfg()
    want = patch_reference(frames, frame_index, K, cfg, crop_rects=rects)
    got = _run(frames, frame_index, None, None, K, None, cfg, None, crop_rects=rects)
    assert got['valid'].tolist() == want['valid'].tolist() == [1, 1, 1, 1, 1, 0, 0, 1, 1]
    assert np.array_equal(got['crop'], want['crop'])
    assert _ulp_close(got['k'], want['k']).all() and _ulp_close(got['transform_matrix'], want['tm']).all()
    assert np.array_equal(got['img'], want['img'])
    # the identity rectangle is the frame region itself
    x1, y1 = rects[0, :2]
    assert np.array_equal(got['img'][0], (frames[0, y1:y1 + 256, x1:x1 + 256, ::-1].astype(np.float32)
                                          * np.float32(1 / 255.)).transpose(2, 0, 1))


def test_odd_output_width_takes_the_scalar_stores():
    g = np.random.default_rng(7)
    frames = g.integers(0, 256, (1, 300, 410, 3), dtype=np.uint8)
    rects = np.array([[20, 30, 250, 199], [-30, 100, 120, 320]], np.int32)
    K = np.stack([_k(500.0, 300, 410)] * 2)
    cfg = _cfg(size=(131, 157), img_scale=131)
    want = patch_reference(frames, [0, 0], K, cfg, crop_rects=rects)
    got = _run(frames, [0, 0], None, None, K, None, cfg, None, crop_rects=rects)
    assert got['img'].shape == (2, 3, 131, 157) and np.array_equal(got['img'], want['img'])


def _pipeline_inputs(seed, hf=480, wf=640):
    cfg = _cfg()
    R, t, K, labels = _draw_objects(hf, wf, cfg, seed)
    keep = [i for i, c in enumerate(CASES) if c[0] in ('up8', 'cube', 'left', 'bottom', 'corner', 'behind')]
    return R[keep], t[keep], K[keep], labels[keep]


def test_pipeline_data_batch_and_hipgraph_replay():
    """PatchPipeline's data_batch layout, and the whole call captured into a hipGraph (one stream, a straight chain):
    replaying on new frame contents gives the new patches."""
    store = MeshStore(MESHES)
    pipe = PatchPipeline.from_cfg(json.load(open(os.path.join(os.path.dirname(__file__), 'golden', 'val_pipeline.json'))), store)
    R, t, K, labels = _pipeline_inputs(11)
    counts = [2, 0, 4]
    g = np.random.default_rng(8)
    frames = [g.integers(0, 256, (3, 480, 640, 3), dtype=np.uint8) for _ in range(2)]
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(DEV)
    args = dict(frames=dev(frames[0]), ref_rotations=dev(R), ref_translations=dev(t), k=dev(K), labels=dev(labels))
    batch = pipe(args['frames'], counts, args['ref_rotations'], args['ref_translations'], args['k'], args['labels'],
                 gt_rotations=args['ref_rotations'], gt_translations=args['ref_translations'])
    index = [0, 0, 2, 2, 2, 2]
    verts = {l: m.verts for l, m in MESHES.items()}
    want = [patch_reference(f, index, K, _cfg(), meshes=verts, labels=labels, R=R, t=t) for f in frames]
    assert [tuple(x.shape) for x in batch['img']] == [(2, 3, 256, 256), (0, 3, 256, 256), (4, 3, 256, 256)]
    assert np.array_equal(torch.cat(batch['img']).cpu().numpy(), want[0]['img'])
    assert batch['valid'].tolist() == want[0]['valid'].tolist() == [1, 1, 1, 1, 1, 0]
    ann = batch['annots']
    assert set(ann) == {'ref_rotations', 'ref_translations', 'labels', 'k', 'ori_k', 'transform_matrix', 'gt_rotations',
                        'gt_translations'}
    assert [len(x) for x in ann['k']] == counts and [len(x) for x in ann['labels']] == counts
    assert torch.equal(torch.cat(ann['k']), batch['flat']['k']) and torch.equal(ann['ori_k'][2], args['k'][2])
    meta = batch['img_metas'][2]
    assert meta['geometry_transform_mode'] == 'adapt_intrinsic' and meta['img_shape'] == [(256, 256, 3)] * 4
    assert meta['img_norm_cfg'] == dict(mean=[0., 0., 0.], std=[255., 255., 255.], to_rgb=True)
    assert torch.equal(meta['scale_factor'], batch['flat']['scale'][2:, None].expand(4, 4))
    # hipGraph: capture on the first frames, replay on the second
    graphed = GraphedPatches(pipe, args, counts)
    out = graphed()
    assert np.array_equal(out['flat']['img'].cpu().numpy(), want[0]['img'])
    out = graphed(dict(frames=dev(frames[1])))
    torch.cuda.synchronize()
    assert np.array_equal(out['flat']['img'].cpu().numpy(), want[1]['img'])
    assert not np.array_equal(want[0]['img'], want[1]['img'])
    graphed.static_in['frames'].copy_(dev(frames[0]))                 # written in place, called without arguments
    assert np.array_equal(graphed()['flat']['img'].cpu().numpy(), want[0]['img'])
    assert np.array_equal(out['flat']['crop'].cpu().numpy(), want[0]['crop'])


# ------------------------------------------------------------------------------------------ end to end
def _golden_shapes():
    here = os.path.dirname(os.path.abspath(__file__))
    return json.load(open(os.path.join(here, 'golden', 'state_dict_keys.json')))['shapes']


@pytest.mark.parametrize('cycles', [1, 2])
def test_frame_to_refined_pose_on_the_device(cycles):
    """render an icosphere into a 480 x 640 frame, quantise it to uint8 BGR, perturb the pose, and run
    PatchPipeline -> format_data_test -> SCFlowRefiner.forward.  The object rendered with the patch's k sits in the
    patch's centre (W/2, H/2 -- the point Pad centres on) within 1.5 px: half a pixel of truncation in each of the
    crop origin, the resized size and the padding."""
    hf, wf = 480, 640
    store = MeshStore({0: colored_icosphere(3, 60.0)})
    K = torch.tensor(_k(600.0, hf, wf), device=DEV)[None]
    R0, t0 = look_at_pose(0.3, -0.2, 0.1, 520.0, 35.0, -20.0)
    labels = torch.zeros(1, dtype=torch.int64, device=DEV)
    full = MeshRenderer(store, (hf, wf), **RENDER_SHIPPED)
    rgba = full(torch.tensor(R0, device=DEV)[None], torch.tensor(t0, device=DEV)[None], K, labels)['images']
    frame = (rgba[..., :3].clamp(0, 1) * 255).round().to(torch.uint8).flip(-1).contiguous()       # (1, Hf, Wf, 3) BGR
    assert int((frame[0].float().std(dim=(0, 1)) > 1).sum()) == 3                                  # the object is in it
    R1, t1 = look_at_pose(0.33, -0.17, 0.12, 530.0, 38.0, -17.0)                                   # the perturbed pose
    rot, trans = torch.tensor(R1, device=DEV)[None], torch.tensor(t1, device=DEV)[None]
    pipe = PatchPipeline(store)
    batch = pipe(frame, [1], rot, trans, K, labels)
    assert batch['valid'].tolist() == [1]
    small = MeshRenderer(store, (256, 256), **RENDER_SHIPPED)
    cfg = scflow_amd.scflow_model_cfg()
    cfg['test_cfg'] = dict(iters=2, cycles=cycles)
    model = scflow_amd.build_refiner(cfg)
    model.load_state_dict(scflow_amd.fill_state_dict(_golden_shapes(), seed=0), strict=True)
    model = model.to(DEV).attach_renderer(small)
    data = model.format_data_test(batch)
    assert data['real_images'].shape == (1, 3, 256, 256) and data['internel_k'].shape == (1, 3, 3)
    assert data['per_img_patch_num'] == [1] and torch.equal(data['ori_k'], K)
    assert torch.equal(data['transform_matrix'], batch['flat']['transform_matrix'])
    assert float(data['real_images'].min()) >= 0 and float(data['real_images'].max()) <= 1
    # the object, rendered at the reference pose with the patch's intrinsics, is centred in the patch
    mask = data['rendered_masks'][0] > 0
    ys, xs = torch.nonzero(mask, as_tuple=True)
    assert len(ys) > 20000
    u = [ops.render_pixel_coord(int(c), 256, 256) for c in (xs.min(), xs.max(), ys.min(), ys.max())]
    cx, cy = (u[0] + u[1]) / 2, (u[2] + u[3]) / 2
    print(f'mask centre ({cx:.2f}, {cy:.2f}) in a 256 x 256 patch')
    assert abs(cx - 128) <= 1.5 and abs(cy - 128) <= 1.5
    # and the frame's own object fills the same place in the real patch (it was rendered near that pose)
    real = data['real_images'][0]
    obj = ((real - 0.5).abs().amax(0) > 0.02)
    assert float((obj & mask).sum()) / float(mask.sum()) > 0.7
    out = model.forward(data)
    assert [tuple(r.shape) for r in out['rotations']] == [(1, 3, 3)] and [tuple(r.shape) for r in out['translations']] == [(1, 3)]
    assert all(bool(torch.isfinite(r).all()) for r in out['rotations'] + out['translations'])
