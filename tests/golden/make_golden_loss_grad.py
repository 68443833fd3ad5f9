"""Generate ``loss_grads.npz``: the GRADIENTS torch autograd gives the reference's own loss classes
(models/loss/sequence_loss.py, point_matching_loss.py), executed unmodified from the reference checkout on CPU under the
import shim and the ``knn_points`` stand-in of ``make_golden_loss.py`` (see there for what is not the reference's).

    python tests/golden/make_golden_loss_grad.py

Every entry of ``PIXEL_OPTIONS`` / ``PM_OPTIONS`` of tests/test_loss_host.py is built as a ``SequenceLoss`` over the class,
called on ``grad_fixture_inputs()`` of tests/test_loss_grad_host.py with predictions that require a gradient, and
``.backward()`` is called on the total.  The inputs are ``fixture_inputs()`` plus what only a gradient sees: pixels and mask
cells whose prediction equals the target, and a fourth iteration whose predicted pose equals the ground truth for two
samples (autograd's gradient at |d| = 0, under both norms).  The file holds recorded results only: the gradients, the
totals, the neighbour indices the ``knn_points`` stand-in returned (``pm_<i>_nn`` (T,N,V), -1 where a sample's class is
not symmetric: the neighbour is a constant of the differentiation, and a near tie may be decided otherwise elsewhere),
and the sequences that were changed (so that a test can tell a regenerated input from the recorded one).
"""
import json
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden_loss as G  # noqa: E402  (installs the shim and the knn_points stand-in)

import test_loss_grad_host as HG  # noqa: E402

H = G.H
_calls = []


def _recording_knn(p1, p2, K=1):
    out = G.knn_points(p1, p2, K)
    _calls.append(out.idx[0, :, 0].numpy().copy())
    return out


G._pm.knn_points = _recording_knn


def loss_grads():
    px, pm = HG.grad_fixture_inputs()
    out = dict(flow_a=torch.stack(px['flow_a']), masks=torch.stack(px['masks']), seq_r=np.stack(pm['seq_r']),
               seq_t=np.stack(pm['seq_t']), pm_options=json.dumps(H.PM_OPTIONS), pixel_options=json.dumps(H.PIXEL_OPTIONS))
    gt_occ = (px['gt'][:, 0] + px['gt'][:, 1] < 400.).float()
    lead = lambda seq: [torch.as_tensor(np.asarray(t)).clone().requires_grad_() for t in seq]
    for i, opt in enumerate(H.PIXEL_OPTIONS):
        valid = px['valid'] if opt['valid'] else None
        if opt['cls'] == 'RAFTLoss':
            f = G.seq_loss(dict(type='RAFTLoss', loss_weight=opt['loss_weight'], max_flow=opt['max_flow']), opt['gamma'])
            preds = lead(px['flow_a'])
            total, _ = f(preds, gt_flow=px['gt'], valid=valid)
        else:
            f = G.seq_loss(dict(type='L1Loss', loss_weight=opt['loss_weight']), opt['gamma'])
            preds = lead(px['masks'])
            total, _ = f(preds, gt_mask=gt_occ, valid=valid)
        total.backward()
        out[f'pixel_{i}_total'], out[f'pixel_{i}_grad'] = total.detach(), torch.stack([p.grad for p in preds])
    empty = tempfile.mkdtemp()
    T = lambda a: torch.from_numpy(np.asarray(a))
    for i, opt in enumerate(H.PM_OPTIONS):
        cfg = {k: v for k, v in opt.items() if k != 'cls'}
        f = G.seq_loss(dict(type=opt['cls'], symmetry_types=H.FIX_SYMMETRY, mesh_diameter=pm['diameter'], mesh_path=empty,
                            **cfg), 0.8)
        f.loss_func.meshes = [T(v) for v in pm['verts']]
        seq_r, seq_t = lead(pm['seq_r']), lead(pm['seq_t'])
        if opt['cls'] == 'RotPointMatchingLoss':
            total, _ = f(seq_r, gt_r=T(pm['gt_r']), labels=T(pm['labels']))
        else:
            total, _ = f(seq_r, seq_t, gt_r=T(pm['gt_r']), gt_t=T(pm['gt_t']), labels=T(pm['labels']),
                         scale_factors=T(pm['scale']))
        total.backward()
        nn = np.full((len(seq_r), len(pm['labels']), max(len(v) for v in pm['verts'])), -1, dtype=np.int32)
        calls = iter(_calls)
        for t in range(len(seq_r)):
            for n, c in enumerate(pm['labels']):
                if f'cls_{int(c) + 1}' in H.FIX_SYMMETRY:
                    idx = next(calls)
                    nn[t, n, :len(idx)] = idx
        assert next(calls, None) is None
        _calls.clear()
        out[f'pm_{i}_nn'] = nn
        out[f'pm_{i}_total'], out[f'pm_{i}_grad_r'] = total.detach(), torch.stack([r.grad for r in seq_r])
        if opt['cls'] != 'RotPointMatchingLoss':
            out[f'pm_{i}_grad_t'] = torch.stack([t.grad for t in seq_t])
    G.save('loss_grads.npz', out)


if __name__ == '__main__':
    torch.manual_seed(0)
    torch.set_num_threads(8)
    loss_grads()
