"""Generate ``losses.npz`` and ``refiner_loss.npz``: the reference's own loss classes (models/loss/sequence_loss.py,
point_matching_loss.py) and its own ``SCFlowRefiner.loss`` (models/refiner/scflow_refiner.py:184-258), executed unmodified
from the reference checkout on CPU through the import shim of ``make_golden.py``.

    python tests/golden/make_golden_loss.py

What is NOT the reference's:
* ``pytorch3d.ops.knn_points`` is a stand-in (below: float64 ``cdist``, ``topk``), installed into the stubbed module before
  the loss classes are imported;
* ``trimesh`` is a stub, so the point-matching losses are built on an empty directory and given their ``.meshes``
  after construction (the reference's ``trimesh.load`` may merge duplicate vertices: not exercised, unverified);
* for ``refiner_loss.npz`` the refiner's ``format_data_train_sup`` (pytorch3d renderer) and ``add_vis_images`` are replaced
  by functions of this file: the formatted data is the seeded ``refiner_loss_case`` of tests/test_loss_host.py.

``losses.npz`` records the inputs (``fixture_inputs`` of tests/test_loss_host.py: T=3, N=3, 24x40, classes of 65 and 300
vertices, class 1 symmetric) and, for every entry of ``PIXEL_OPTIONS`` / ``PM_OPTIONS`` there, the total and the list a
``SequenceLoss`` over the class returns.  ``refiner_loss.npz`` records seeds, the ground-truth poses and mask used, and
the scalars of ``log_vars`` in their order.  Both hold recorded results only.
"""
import json
import os
import runpy
import sys
import tempfile
import types

os.environ.setdefault('MKL_CBWR', 'COMPATIBLE')

import numpy as np  # noqa: E402
import torch  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import _refshim  # noqa: E402

_refshim.install()


def knn_points(p1, p2, K=1):
    """stand-in for pytorch3d.ops.knn_points: squared distances in float64, the K smallest per query point."""
    d = torch.cdist(p1.double(), p2.double()) ** 2
    dists, idx = torch.topk(d, K, dim=-1, largest=False)
    return types.SimpleNamespace(dists=dists, idx=idx, knn=None)


sys.modules['pytorch3d.ops'].knn_points = knn_points

import test_loss_host as H  # noqa: E402

from models.loss.builder import build_loss  # noqa: E402
from models.loss import point_matching_loss as _pm  # noqa: F401,E402
from models.loss import sequence_loss as _sl  # noqa: F401,E402
from models.refiner.builder import REFINERS  # noqa: E402
from models.refiner.scflow_refiner import SCFlowRefiner  # noqa: F401,E402
from mmcv.utils import build_from_cfg  # noqa: E402

from scflow_amd.weights import fill_state_dict  # noqa: E402

SHIM = 'reference source under mini-mmcv shim; knn_points stand-in (float64 cdist + topk)'


def seq_loss(func_cfg, gamma):
    return build_loss(dict(type='SequenceLoss', gamma=gamma, loss_func_cfg=func_cfg))


@torch.no_grad()
def losses():
    px, pm = H.fixture_inputs()
    out = dict(gt=px['gt'], valid=px['valid'], flow_a=torch.stack(px['flow_a']), flow_b=torch.stack(px['flow_b']),
               masks=torch.stack(px['masks']), verts0=pm['verts'][0], verts1=pm['verts'][1], labels=pm['labels'],
               gt_r=pm['gt_r'], gt_t=pm['gt_t'], seq_r=np.stack(pm['seq_r']), seq_t=np.stack(pm['seq_t']), scale=pm['scale'],
               diameter=np.asarray(pm['diameter'], dtype=np.float64), pm_options=json.dumps(H.PM_OPTIONS),
               pixel_options=json.dumps(H.PIXEL_OPTIONS), symmetry_types=json.dumps(H.FIX_SYMMETRY))
    gt_occ = (px['gt'][:, 0] + px['gt'][:, 1] < 400.).float()             # the refiner's target: channel sum < max_flow
    out['gt_occ'] = gt_occ
    for i, opt in enumerate(H.PIXEL_OPTIONS):
        valid = px['valid'] if opt['valid'] else None
        if opt['cls'] == 'RAFTLoss':
            f = seq_loss(dict(type='RAFTLoss', loss_weight=opt['loss_weight'], max_flow=opt['max_flow']), opt['gamma'])
            total, lst = f(px['flow_a'], gt_flow=px['gt'], valid=valid)
        else:
            f = seq_loss(dict(type='L1Loss', loss_weight=opt['loss_weight']), opt['gamma'])
            total, lst = f(px['masks'], gt_mask=gt_occ, valid=valid)
        out[f'pixel_{i}_total'], out[f'pixel_{i}_list'] = total, torch.stack(lst)
    empty = tempfile.mkdtemp()                            # _load_mesh on an empty directory: no meshes, no trimesh call
    T = lambda a: torch.from_numpy(np.asarray(a))
    for i, opt in enumerate(H.PM_OPTIONS):
        cfg = {k: v for k, v in opt.items() if k != 'cls'}
        f = seq_loss(dict(type=opt['cls'], symmetry_types=H.FIX_SYMMETRY, mesh_diameter=pm['diameter'], mesh_path=empty,
                          **cfg), 0.8)
        f.loss_func.meshes = [T(v) for v in pm['verts']]
        seq_r, seq_t = [T(r) for r in pm['seq_r']], [T(t) for t in pm['seq_t']]
        if opt['cls'] == 'RotPointMatchingLoss':
            total, lst = f(seq_r, gt_r=T(pm['gt_r']), labels=T(pm['labels']))
        else:
            total, lst = f(seq_r, seq_t, gt_r=T(pm['gt_r']), gt_t=T(pm['gt_t']), labels=T(pm['labels']),
                           scale_factors=T(pm['scale']))
        out[f'pm_{i}_total'], out[f'pm_{i}_list'] = total, torch.stack(lst)
    save('losses.npz', out)


@torch.no_grad()
def refiner_loss(input_seed=7, case_seed=5, weight_seed=0):
    case = H.refiner_loss_case(input_seed, case_seed)
    cfg = dict(runpy.run_path(_refshim.REFERENCE_ROOT + '/configs/refine_models/scflow.py')['model'])
    cfg['renderer'] = None
    cfg['pose_loss_cfg'] = dict(cfg['pose_loss_cfg'])
    cfg['pose_loss_cfg']['loss_func_cfg'] = dict(cfg['pose_loss_cfg']['loss_func_cfg'], mesh_path=tempfile.mkdtemp(),
                                                 symmetry_types=case['symmetry_types'], mesh_diameter=case['diameter'])
    model = build_from_cfg(cfg, REFINERS).eval()
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(fill_state_dict(shapes, seed=weight_seed), strict=True)
    model.decoder.iters = H.REFINER_ITERS
    model.pose_loss_func.loss_func.meshes = [torch.from_numpy(v) for v in case['verts']]
    data = H.refiner_data(case)
    model.format_data_train_sup = lambda data_batch: data
    model.add_vis_images = lambda **kw: None
    # scflow_refiner.py:213-216 reads one scale factor per sample from the image metas
    data_batch = dict(img_metas=[dict(scale_factor=np.repeat(case['scale'][:, None], 4, axis=1))])
    _, _, log_vars, _, _ = model.loss(data_batch)
    save('refiner_loss.npz', dict(input_seed=input_seed, case_seed=case_seed, weight_seed=weight_seed, iters=H.REFINER_ITERS,
                                  gt_r=case['gt_r'], gt_t=case['gt_t'],
                                  gt_masks_bits=np.packbits(case['gt_masks'].numpy().reshape(-1)),
                                  keys=np.asarray(list(log_vars.keys())),
                                  values=np.asarray(list(log_vars.values()), dtype=np.float64)))


def save(name, arrays):
    out = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in arrays.items()}
    out['pinned_under'] = np.asarray(SHIM)
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **out)
    print(f'{name}: {os.path.getsize(path) / 1024:.1f} KiB')


if __name__ == '__main__':
    torch.manual_seed(0)
    torch.set_num_threads(8)
    losses()
    refiner_loss()
