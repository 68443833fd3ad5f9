"""Generate ``tail_grads.npz``: the gradients torch autograd gives through the reference's OWN tail of an SCFlow iteration
-- ``get_pose_from_delta_pose``, ``cal_3d_2d_corr``, ``get_flow_from_delta_pose_and_points`` (models/utils/pose.py) and
``F.interpolate`` in the order of scflow_decoder.py:183-250 -- executed from the reference checkout in fp32 on the CPU under
the import shim of ``make_golden.py``.

    python tests/golden/make_golden_tail_grad.py

The head outputs, constants and cotangents are ``tail_case()`` of tests/test_tail_grad_host.py (N = 3, 16 x 24, h x w =
2 x 3, T = 3).  Recorded for the shipped flags (detach_flow, detach_pose set) and for all flags off, under both depth
transforms: the poses of the forward (the values the gradients were taken at) and the gradient of
sum <output, cotangent> with respect to every head output.  The file holds inputs and recorded results only.
"""
import os
import sys

os.environ.setdefault('MKL_CBWR', 'COMPATIBLE')

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import _refshim  # noqa: E402

_refshim.install()

from models.utils.pose import (cal_3d_2d_corr, get_flow_from_delta_pose_and_points,  # noqa: E402
                               get_pose_from_delta_pose)

import test_tail_grad_host as HT  # noqa: E402

SHIM = 'reference source under mini-mmcv shim; fp32, CPU'
CONFIGS = (('shipped', (True, True, False)), ('free', (False, False, False)))


def reference_tail(heads, consts, flags, depth_transform, scale=8):
    """scflow_decoder.py:183-250 without the network: the head outputs are the leaves."""
    detach_flow, detach_pose, detach_depth = flags
    ref_rot, ref_trans, depth, k, init_flow, invalid = consts
    n, H, W = depth.shape
    pts2d, pts3d = [], []
    for i in range(n):
        p2, p3 = cal_3d_2d_corr(depth[i], k[i], ref_rot[i], ref_trans[i])
        pts2d.append(p2)
        pts3d.append(p3)
    rot, trans, flow = ref_rot, ref_trans, init_flow
    out = {key: [] for key in HT.COT_KEYS}
    for i in range(len(heads['masks'])):
        if detach_flow:
            flow = flow.detach()
        flow = 1 / scale * F.interpolate(flow, scale_factor=(1 / scale, 1 / scale), mode='bilinear', align_corners=True)
        flow_pred = scale * F.interpolate(flow + heads['delta_flow_preds'][i], scale_factor=(scale, scale), mode='bilinear',
                                          align_corners=True)
        up_mask = F.interpolate(heads['masks'][i], scale_factor=(scale, scale), mode='bilinear', align_corners=True)
        rot, trans = get_pose_from_delta_pose(
            heads['delta_rotation_preds'][i], heads['delta_translation_preds'][i], rot.detach() if detach_pose else rot,
            trans.detach() if detach_pose else trans, depth_transform=depth_transform, detach_depth_for_xy=detach_depth)
        flow = get_flow_from_delta_pose_and_points(rot, trans, k, pts2d, pts3d, H, W, invalid_num=invalid)
        for key, val in zip(HT.COT_KEYS, (flow, flow_pred, rot, trans, up_mask)):
            out[key].append(val)
    return out


def tail_grads():
    heads, consts, cots, _ = HT.tail_case()
    rec = {key: np.stack([t.numpy() for t in heads[key]]) for key in HT.HEAD_KEYS}
    rec.update(ref_rot=consts[0], ref_trans=consts[1], depth=consts[2], k=consts[3], init_flow=consts[4])
    rec.update({'cot_' + key: np.stack([t.numpy() for t in cots[key]]) for key in HT.COT_KEYS})
    for tag, flags in CONFIGS:
        for depth_transform in ('exp', 'linear'):
            leaves = {key: [t.clone().requires_grad_() for t in heads[key]] for key in HT.HEAD_KEYS}
            out = reference_tail(leaves, consts, flags, depth_transform)
            total = sum((o * c).sum() for key in HT.COT_KEYS for o, c in zip(out[key], cots[key]))
            total.backward()
            pre = f'{tag}_{depth_transform}_'
            rec[pre + 'rot'] = np.stack([r.detach().numpy() for r in out['rotation_preds']])
            rec[pre + 'trans'] = np.stack([t.detach().numpy() for t in out['translation_preds']])
            for key in HT.HEAD_KEYS:
                rec[pre + key] = np.stack([(torch.zeros_like(t) if t.grad is None else t.grad).numpy() for t in leaves[key]])
    out = {k_: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k_, v in rec.items()}
    out['pinned_under'] = np.asarray(SHIM)
    path = os.path.join(HERE, 'tail_grads.npz')
    np.savez_compressed(path, **out)
    print(f'tail_grads.npz: {os.path.getsize(path) / 1024:.1f} KiB')


if __name__ == '__main__':
    torch.manual_seed(0)
    torch.set_num_threads(8)
    tail_grads()
