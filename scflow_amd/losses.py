"""Values and gradients of the supervised losses (reference models/loss/): the ``LOSSES`` registry, ``build_loss`` and
``RAFTLoss``, ``L1Loss``, ``SequenceLoss``, ``PointMatchingLoss``, ``DisentanglePointMatchingLoss``,
``RotPointMatchingLoss`` with the reference's constructor keys and call signatures, on the HIP kernels of loss.hip.

**Values and gradients.**  Called on predictions that do not require a gradient, every class returns the VALUE the
reference trains against and logs -- a 0-dim GPU tensor without a graph behind it, from the forward-only launches.
The derivative of the gamma-weighted total with respect to every prediction comes from the ``*_grad`` entries of loss.hip
(``seq_pixel_loss_grad``, ``point_matching_loss_grad``), which return the same values bit for bit and the gradients from
the same pass, in two ways:

* ``SequenceLoss.value_and_grad(*preds, **kwargs)`` -> ``(total, [loss_i], grads)``, ``grads`` a tuple of lists that
  mirrors ``preds``; no autograd involved;
* autograd: when grad mode is on and a prediction requires a gradient, the returned total carries a graph (one
  ``torch.autograd.Function``; the gradients are computed with the values and scaled by ``grad_output`` in
  ``backward``), so ``total.backward()`` leaves the same gradients in ``.grad``.  DEVIATION from the reference: the
  per-iteration list ``[loss_i]`` stays detached -- only the total can be back-propagated.

No gradient goes to ground truths, meshes or scale factors, and the network behind the predictions has no backward:
``forward(return_loss=True)`` of the refiners keeps raising (see ``loss_and_grads``).
CPU tensors are refused (``ScflowHipError``), like everywhere else in this package.

``SequenceLoss`` over one of the classes above evaluates ALL iterations in one launch (``scf_seq_pixel_loss`` /
``scf_point_matching_loss``); over anything else registered in ``LOSSES`` it runs the reference's per-iteration loop.

Restated as they are in the reference:

* ``L1Loss`` ignores ``valid`` (sequence_loss.py:35-37);
* a class is symmetric when the KEY ``'cls_<label+1>'`` is in ``symmetry_types`` (point_matching_loss.py:93; membership,
  not truthiness -- ``eval_pose_error`` uses truthiness);
* the neighbour of a symmetric class is the squared-L2 nearest point whatever ``loss_type`` is;
* any ``reduction`` other than ``'mean'`` sums.

Meshes: ``mesh_path`` (a directory, ``*.ply`` in sorted order like the reference's ``glob``, or one file) is read with
``read_ply`` at the first use, not in the constructor; a ``MeshStore`` or a list of (V,3) tensors / arrays may be assigned
to ``.meshes``.  Vertices are taken as read.  The reference loads with ``trimesh.load``, which may merge duplicate
vertices; trimesh was not available to compare against, so this is UNVERIFIED and not imitated.
"""
from __future__ import annotations

import ctypes as C
import os
from glob import glob
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib, ops
from .registry import Registry, build_from_cfg

__all__ = ['LOSSES', 'build_loss', 'RAFTLoss', 'L1Loss', 'SequenceLoss', 'PointMatchingLoss',
           'DisentanglePointMatchingLoss', 'RotPointMatchingLoss', 'seq_pixel_loss', 'point_matching_loss', 'seq_pixel_loss_grad',
           'point_matching_loss_grad', 'to_host']

Tensor = torch.Tensor
LOSSES = Registry('loss')
MAX_T = 256                      # LOSS_MAX_T_TOTAL of loss.hip

PM_FULL, PM_DISENTANGLE, PM_ROT = 0, 1, 2
PM_DISENTANGLE_Z, PM_SCALE_XY, PM_SCALE_DEPTH = 1, 2, 4


def build_loss(cfg):
    return build_from_cfg(cfg, LOSSES)


def to_host(vec: Tensor) -> List[float]:
    """the ONE device-to-host transfer of the loss path: a packed vector of scalars -> Python floats."""
    return vec.cpu().tolist()


def _ptr_array(tensors: Optional[Sequence[Tensor]]):
    if tensors is None:
        return None
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _seq(tensors, shape, name) -> Optional[List[Tensor]]:
    """a sequence of equal-shape GPU fp32 tensors, made contiguous; (N,1,H,W) masks are taken as (N,H,W)."""
    if tensors is None:
        return None
    out = []
    for i, t in enumerate(tensors):
        ops._dev(t, f'{name}[{i}]')
        if t.dim() == len(shape) + 1 and t.shape[1] == 1:
            t = t.squeeze(1)
        if tuple(t.shape) != tuple(shape):
            raise _lib.ScflowHipError(f'{name}[{i}] has shape {tuple(t.shape)}, expected {tuple(shape)}')
        out.append(t.contiguous())
    return out


def _upstream(upstream, count, device):
    """a device pointer to ``count`` fp32 scalars (or None = 1) and the tensor that keeps it alive."""
    if upstream is None:
        return None, None
    if not isinstance(upstream, torch.Tensor) or not upstream.is_cuda:
        raise _lib.ScflowHipError('upstream: expected a tensor on the GPU (it is read by the kernel, never by the host)')
    up = upstream.detach().to(torch.float32).reshape(-1).contiguous()
    if up.numel() != count:
        raise _lib.ScflowHipError(f'upstream: expected {count} scalar(s), got {up.numel()}')
    return up.data_ptr(), up


def _grad_planes(out, like, want, name):
    """the gradient tensors of one sequence: ``out`` (caller's, dense fp32 GPU tensors with the elements of the
    predictions) or one fresh allocation; None when the sequence is absent or not wanted."""
    if like is None or not want:
        return None
    if out is None:
        return list(torch.empty((len(like),) + tuple(like[0].shape), dtype=torch.float32, device=like[0].device).unbind(0))
    if len(out) != len(like):
        raise ValueError(f'{name}: {len(out)} gradient tensors for {len(like)} predictions')
    for i, g in enumerate(out):
        ops._dev(g, f'{name}[{i}]')
        if g.numel() != like[i].numel() or not g.is_contiguous():
            raise _lib.ScflowHipError(f'{name}[{i}]: expected a contiguous tensor of {like[i].numel()} elements')
    return list(out)


def _seq_pixel(gt_flow, valid, flow_a, flow_b, masks, mask_gt, max_flow, loss_weight, eps, gamma, grad=False,
               upstream=None, want=(True, True, True), grad_out=(None, None, None)):
    seqs = [s for s in (flow_a, flow_b, masks) if s is not None]
    if not seqs:
        raise ValueError('seq_pixel_loss: no sequence given')
    T = len(seqs[0])
    if T == 0 or any(len(s) != T for s in seqs):
        raise ValueError('seq_pixel_loss: the sequences must have one common, non-zero length')
    if T > MAX_T:
        raise _lib.ScflowHipError(f'seq_pixel_loss: at most {MAX_T} iterations, got {T}')
    first = seqs[0][0]
    ops._dev(first, 'prediction')
    if gt_flow is not None:
        ops._dev(gt_flow, 'gt_flow')
        if gt_flow.dim() != 4 or gt_flow.shape[1] != 2:
            raise _lib.ScflowHipError(f'gt_flow: expected (N,2,H,W), got {tuple(gt_flow.shape)}')
        n, _, h, w = gt_flow.shape
        gt_flow = gt_flow.contiguous()
    else:
        if flow_a is not None or flow_b is not None or mask_gt is None:
            raise ValueError('seq_pixel_loss: gt_flow is needed unless only masks against mask_gt are given')
        n, h, w = mask_gt.shape
    mask_shapes = None if masks is None else [tuple(m.shape) for m in masks]
    flow_a = _seq(flow_a, (n, 2, h, w), 'flow_a')
    flow_b = _seq(flow_b, (n, 2, h, w), 'flow_b')
    masks = _seq(masks, (n, h, w), 'masks')
    keep = [flow_a, flow_b, masks, gt_flow]

    def plane(t, name):
        if t is None:
            return None
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise _lib.ScflowHipError(f'{name}: expected a tensor on the GPU (HIP path only, no CPU fallback)')
        t = t.to(torch.float32).contiguous()
        if tuple(t.shape) != (n, h, w):
            raise _lib.ScflowHipError(f'{name} has shape {tuple(t.shape)}, expected {(n, h, w)}')
        keep.append(t)
        return ops._dense(t, name)
    pv, pm = plane(valid, 'valid'), plane(mask_gt, 'mask_gt')
    lib = _lib.load()
    dev = first.device
    per_iter = torch.empty((3, T), dtype=torch.float32, device=dev)
    totals = torch.empty((3,), dtype=torch.float32, device=dev)
    f3 = lambda v: (C.c_float * 3)(*[float(x) for x in v])
    head = (None if gt_flow is None else gt_flow.data_ptr(), pv, pm, _ptr_array(flow_a), _ptr_array(flow_b),
            _ptr_array(masks), T, n, h, w, float(max_flow), f3(loss_weight), f3(eps),
            (C.c_double * 3)(*[float(g) for g in gamma]))
    if not grad:
        ws = torch.empty((int(lib.scf_seq_pixel_loss_workspace_bytes(n, h, w, T)),), dtype=torch.uint8, device=dev)
        _lib.check(lib.scf_seq_pixel_loss(*head, per_iter.data_ptr(), totals.data_ptr(), ws.data_ptr(), ops._stream()),
                   'scf_seq_pixel_loss')
        return per_iter, totals
    ws = torch.empty((int(lib.scf_seq_pixel_loss_grad_workspace_bytes(n, h, w, T)),), dtype=torch.uint8, device=dev)
    up_ptr, up_keep = _upstream(upstream, 3, dev)
    grads = [_grad_planes(o, s, wnt, name) for o, s, wnt, name in
             zip(grad_out, (flow_a, flow_b, masks), want, ('grad_a', 'grad_b', 'grad_mask'))]
    _lib.check(lib.scf_seq_pixel_loss_grad(*head, up_ptr, _ptr_array(grads[0]), _ptr_array(grads[1]), _ptr_array(grads[2]),
                                           per_iter.data_ptr(), totals.data_ptr(), ws.data_ptr(), ops._stream()),
               'scf_seq_pixel_loss_grad')
    del up_keep
    if grads[2] is not None and grad_out[2] is None:
        grads[2] = [g.view(shape) for g, shape in zip(grads[2], mask_shapes)]       # (N,1,H,W) predictions get their shape
    return per_iter, totals, tuple(grads)


def seq_pixel_loss(gt_flow: Optional[Tensor], valid: Optional[Tensor] = None, flow_a=None, flow_b=None, masks=None,
                   mask_gt: Optional[Tensor] = None, max_flow: float = 400., loss_weight=(1., 1., 1.),
                   eps=(1e-10, 1e-10, 1e-10), gamma=(0.8, 0.8, 0.8)):
    """``scf_seq_pixel_loss``: SequenceLoss(RAFTLoss) of up to two flow sequences and SequenceLoss(L1Loss) of one mask
    sequence against the same ground truth, one pass -> (per_iter (3,T), totals (3)); rows flow_a, flow_b, masks, zeros
    where a sequence is absent.  Without ``mask_gt`` the mask target is ``(gt_x + gt_y < max_flow)`` -- the SUM of the two
    channels, not the magnitude, as scflow_refiner.py:230 has it."""
    return _seq_pixel(gt_flow, valid, flow_a, flow_b, masks, mask_gt, max_flow, loss_weight, eps, gamma)


def seq_pixel_loss_grad(gt_flow: Optional[Tensor], valid: Optional[Tensor] = None, flow_a=None, flow_b=None, masks=None,
                        mask_gt: Optional[Tensor] = None, max_flow: float = 400., loss_weight=(1., 1., 1.),
                        eps=(1e-10, 1e-10, 1e-10), gamma=(0.8, 0.8, 0.8), upstream: Optional[Tensor] = None,
                        want=(True, True, True), grad_out=(None, None, None)):
    """``scf_seq_pixel_loss_grad``: the values of ``seq_pixel_loss`` (the same bits) and, from the same pass, the
    derivative of ``sum_row upstream[row] * totals[row]`` -> (per_iter, totals, grads); ``grads`` = (grad_a, grad_b,
    grad_mask), each a list of T tensors shaped like the predictions, or None where the sequence is absent or its entry of
    ``want`` is false.  ``upstream``: a GPU tensor of 3 scalars (read on the device; None = 1).  ``grad_out``: tensors to
    write into instead of fresh ones."""
    return _seq_pixel(gt_flow, valid, flow_a, flow_b, masks, mask_gt, max_flow, loss_weight, eps, gamma, True, upstream,
                      want, grad_out)


class _TotalWithGrad(torch.autograd.Function):
    """the one autograd node of this module: ``run(tensors)`` -> (total, gradients aligned with ``tensors``, None where
    there is none) computes both in one launch; ``backward`` scales the kept gradients by ``grad_output`` on the device."""

    @staticmethod
    def forward(ctx, run, *tensors):
        total, grads = run(tensors)
        ctx.present = [g is not None for g in grads]
        ctx.save_for_backward(*[g for g in grads if g is not None])
        return total.clone()

    @staticmethod
    def backward(ctx, grad_output):
        kept = iter(ctx.saved_tensors)
        return (None,) + tuple(next(kept) * grad_output if p else None for p in ctx.present)


def _wants_graph(*seqs) -> bool:
    return torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad
                                           for s in seqs if s is not None for t in s)


def _through_autograd(seqs, run_grad):
    """seqs: lists of predictions (None allowed); run_grad(detached seqs, want per sequence) -> (total, extras, grads per
    sequence).  -> (total with a graph, extras)."""
    lens = [0 if s is None else len(s) for s in seqs]
    want = tuple(s is not None and any(t.requires_grad for t in s) for s in seqs)
    box = {}

    def run(flat):
        flat, det = list(flat), []
        for n, s in zip(lens, seqs):
            det.append(None if s is None else [t.detach() for t in flat[:n]])
            flat = flat[n:]
        total, box['extras'], grads = run_grad(det, want)
        out = []
        for n, g in zip(lens, grads):
            out += [None] * n if g is None else list(g)
        return total, out
    total = _TotalWithGrad.apply(run, *[t for s in seqs if s is not None for t in s])
    return total, box['extras']


@LOSSES.register_module()
class RAFTLoss:
    """sequence_loss.py:8-24: ``loss_weight * sum(valid * |pred - gt|) / (count(valid) + eps)`` with
    ``valid = (valid >= 0.5) & (|gt| < max_flow)``."""

    def __init__(self, loss_weight=1.0, max_flow=400, eps=1e-10):
        self.loss_weight, self.max_flow, self.eps = loss_weight, max_flow, eps

    def to(self, device):
        return self

    def sequence(self, preds, gt_flow, valid=None, gamma=0.8):
        if _wants_graph(preds):
            return _through_autograd([list(preds)], lambda det, want: self._with_grad(det[0], gt_flow, valid, gamma))
        per_iter, totals = seq_pixel_loss(gt_flow, valid, flow_a=preds, max_flow=self.max_flow,
                                          loss_weight=(self.loss_weight, 1., 1.), eps=(self.eps, 0., 0.),
                                          gamma=(gamma, 1., 1.))
        return totals[0], per_iter[0]

    def _with_grad(self, preds, gt_flow, valid, gamma):
        per_iter, totals, grads = seq_pixel_loss_grad(gt_flow, valid, flow_a=preds, max_flow=self.max_flow,
                                                      loss_weight=(self.loss_weight, 1., 1.), eps=(self.eps, 0., 0.),
                                                      gamma=(gamma, 1., 1.))
        return totals[0], per_iter[0], (grads[0],)

    def sequence_grad(self, preds, gt_flow, valid=None, gamma=0.8):
        """-> (total, per_iter (T), (gradients of total w.r.t. ``preds``,)); no graph."""
        return self._with_grad(preds, gt_flow, valid, gamma)

    def forward(self, pred_flow, gt_flow, valid=None):
        total, per_iter = self.sequence([pred_flow], gt_flow, valid)
        return total if total.requires_grad else per_iter[0]          # one iteration: the total IS the value (weight 1)

    __call__ = forward


@LOSSES.register_module()
class L1Loss:
    """sequence_loss.py:28-37: ``mean(|pred_mask - gt_mask|) * loss_weight``; ``valid`` and ``eps`` are accepted and
    ignored, as in the reference."""

    def __init__(self, loss_weight=1.0, eps=1e-10):
        self.loss_weight, self.eps = loss_weight, eps

    def to(self, device):
        return self

    def sequence(self, preds, gt_mask, valid=None, gamma=0.8):
        if _wants_graph(preds):
            return _through_autograd([list(preds)], lambda det, want: self._with_grad(det[0], gt_mask, gamma))
        per_iter, totals = seq_pixel_loss(None, None, masks=preds, mask_gt=gt_mask,
                                          loss_weight=(1., 1., self.loss_weight), gamma=(1., 1., gamma))
        return totals[2], per_iter[2]

    def _with_grad(self, preds, gt_mask, gamma):
        per_iter, totals, grads = seq_pixel_loss_grad(None, None, masks=preds, mask_gt=gt_mask,
                                                      loss_weight=(1., 1., self.loss_weight), gamma=(1., 1., gamma))
        return totals[2], per_iter[2], (grads[2],)

    def sequence_grad(self, preds, gt_mask, valid=None, gamma=0.8):
        """-> (total, per_iter (T), (gradients of total w.r.t. ``preds``,)); no graph."""
        return self._with_grad(preds, gt_mask, gamma)

    def forward(self, pred_mask, gt_mask, valid=None):
        total, per_iter = self.sequence([pred_mask], gt_mask, valid)
        return total if total.requires_grad else per_iter[0]

    __call__ = forward


# ------------------------------------------------------------------------------------------------- point matching
def _point_matching(verts, offsets, group, labels, symmetric, diameter, seq_r, seq_t, gt_r, gt_t, scale_factors,
                    max_points, mode, loss_type, flags, scale_depth_factor, reduction, loss_weight, gamma, return_nn,
                    grad=False, upstream=None, want=(True, True)):
    T = len(seq_r)
    if T == 0 or T > MAX_T:
        raise _lib.ScflowHipError(f'point_matching_loss: 1..{MAX_T} iterations, got {T}')
    n = int(gt_r.shape[0])
    seq_r = _seq(seq_r, (n, 3, 3), 'pred_r')
    gt_r = gt_r.contiguous()
    ops._mats(gt_r, n, (3, 3), 'gt_r')
    if mode != PM_ROT:
        if seq_t is None or len(seq_t) != T:
            raise ValueError('point_matching_loss: pred_t must have the length of pred_r')
        seq_t = _seq(seq_t, (n, 3), 'pred_t')
        gt_t = gt_t.contiguous()
        ops._mats(gt_t, n, (3,), 'gt_t')
    else:
        seq_t = gt_t = None
    if scale_factors is not None:
        if not isinstance(scale_factors, torch.Tensor) or not scale_factors.is_cuda:
            raise _lib.ScflowHipError('scale_factors: expected a tensor on the GPU')
        scale_factors = scale_factors.to(torch.float32).contiguous()
        ops._mats(scale_factors, n, (), 'scale_factors')
    for t, name, shape in ((group, 'group', (n,)), (labels, 'labels', (n,)), (offsets, 'offsets', None),
                           (symmetric, 'symmetric', None)):
        if (not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous()
                or (shape is not None and tuple(t.shape) != shape) or t.numel() == 0):
            raise _lib.ScflowHipError(f'{name}: expected a contiguous 1-D int32 GPU tensor' + (f' of shape {shape}' if shape else ''))
    if offsets.numel() < 2 or verts.dim() != 2 or verts.shape[1] != 3 or diameter.numel() != symmetric.numel():
        raise _lib.ScflowHipError('point_matching_loss: verts (total,3), offsets (groups+1), symmetric and diameter (classes)')
    lib = _lib.load()
    dev = gt_r.device
    loss_i = torch.empty((T, n), dtype=torch.float32, device=dev)
    per_iter = torch.empty((T,), dtype=torch.float32, device=dev)
    total = torch.empty((1,), dtype=torch.float32, device=dev)
    nn_idx = torch.full((T, n, max(max_points, 1)), -1, dtype=torch.int32, device=dev) if return_nn else None
    P = lambda t: None if t is None else t.data_ptr()
    head = (ops._dense(verts, 'verts'), offsets.data_ptr(), int(offsets.numel()) - 1, group.data_ptr(), labels.data_ptr(),
            int(symmetric.numel()), symmetric.data_ptr(), ops._dense(diameter, 'diameter'), _ptr_array(seq_r),
            _ptr_array(seq_t), T, gt_r.data_ptr(), P(gt_t), P(scale_factors), n, int(max_points), int(mode), int(loss_type),
            int(flags), float(scale_depth_factor), 0 if reduction == 'mean' else 1, float(loss_weight), float(gamma))
    tail = (loss_i.data_ptr(), per_iter.data_ptr(), total.data_ptr(), P(nn_idx))
    if not grad:
        ws = torch.empty((int(lib.scf_point_matching_workspace_bytes(n, T, max_points)),), dtype=torch.uint8, device=dev)
        _lib.check(lib.scf_point_matching_loss(*head, *tail, ws.data_ptr(), ops._stream()), 'scf_point_matching_loss')
        return loss_i, per_iter, total, nn_idx
    ws = torch.empty((int(lib.scf_point_matching_grad_workspace_bytes(n, T, max_points)),), dtype=torch.uint8, device=dev)
    up_ptr, up_keep = _upstream(upstream, 1, dev)
    grad_r = _grad_planes(None, seq_r, want[0], 'grad_r')
    grad_t = _grad_planes(None, seq_t, want[1], 'grad_t')
    _lib.check(lib.scf_point_matching_loss_grad(*head, up_ptr, _ptr_array(grad_r), _ptr_array(grad_t), *tail, ws.data_ptr(),
                                                ops._stream()), 'scf_point_matching_loss_grad')
    del up_keep
    return loss_i, per_iter, total, nn_idx, grad_r, grad_t


def point_matching_loss(verts: Tensor, offsets: Tensor, group: Tensor, labels: Tensor, symmetric: Tensor,
                        diameter: Tensor, seq_r, seq_t, gt_r: Tensor, gt_t: Optional[Tensor],
                        scale_factors: Optional[Tensor], max_points: int, mode: int, loss_type: int, flags: int = 0,
                        scale_depth_factor: float = 1., reduction: str = 'mean', loss_weight: float = 1.,
                        gamma: float = 0.8, return_nn: bool = False):
    """``scf_point_matching_loss`` -> (loss_i (T,N), per_iter (T), total (1), nn_idx (T,N,max_points) int32 or None;
    -1 past a sample's point count).  See include/scflow_hip.h for the arguments."""
    return _point_matching(verts, offsets, group, labels, symmetric, diameter, seq_r, seq_t, gt_r, gt_t, scale_factors,
                           max_points, mode, loss_type, flags, scale_depth_factor, reduction, loss_weight, gamma, return_nn)


def point_matching_loss_grad(verts: Tensor, offsets: Tensor, group: Tensor, labels: Tensor, symmetric: Tensor,
                             diameter: Tensor, seq_r, seq_t, gt_r: Tensor, gt_t: Optional[Tensor],
                             scale_factors: Optional[Tensor], max_points: int, mode: int, loss_type: int, flags: int = 0,
                             scale_depth_factor: float = 1., reduction: str = 'mean', loss_weight: float = 1.,
                             gamma: float = 0.8, return_nn: bool = False, upstream: Optional[Tensor] = None,
                             want=(True, True)):
    """``scf_point_matching_loss_grad``: the values of ``point_matching_loss`` (the same bits) and the derivative of
    ``upstream * total`` from the same neighbour search -> (loss_i, per_iter, total, nn_idx, grad_r, grad_t): lists of T
    (N,3,3) / (N,3) tensors; ``grad_t`` is None for ``PM_ROT``.  ``upstream``: one scalar on the GPU (None = 1)."""
    return _point_matching(verts, offsets, group, labels, symmetric, diameter, seq_r, seq_t, gt_r, gt_t, scale_factors,
                           max_points, mode, loss_type, flags, scale_depth_factor, reduction, loss_weight, gamma, return_nn,
                           True, upstream, want)


class _PointMatchingBase:
    _mode = PM_FULL

    def _init_common(self, symmetry_types, mesh_diameter, use_perspective_shape, mesh_path, loss_weight, reduction,
                     loss_type):
        if loss_type not in ('l1', 'l2'):
            raise AssertionError(f"loss_type must be 'l1' or 'l2', got {loss_type!r}")
        # the reference's attribute names (part of the interface); loss_type is kept as the order of the norm, 1 or 2
        self.__dict__.update(symmetry_types=symmetry_types, mesh_diameter=mesh_diameter, mesh_path=mesh_path,
                             use_perspective_shape=use_perspective_shape, loss_weight=loss_weight, reduction=reduction,
                             loss_type={'l1': 1, 'l2': 2}[loss_type], _meshes=None, _tables={})

    # ---- meshes: read at the first use; a MeshStore or a list of (V,3) vertex sets may be assigned
    @property
    def meshes(self):
        if self._meshes is None and not self.use_perspective_shape:
            if self.mesh_path is None:
                raise ValueError(f'{type(self).__name__}: no meshes -- give mesh_path, or assign a MeshStore or a list of '
                                 '(V,3) vertex tensors to .meshes')
            self._meshes = self._load_mesh(self.mesh_path)
        return self._meshes

    @meshes.setter
    def meshes(self, value):
        self._meshes = value
        self._tables = {}

    @staticmethod
    def _load_mesh(mesh_path, ext='.ply'):
        from .mesh import read_ply
        paths = sorted(glob(os.path.join(mesh_path, '*' + ext))) if os.path.isdir(mesh_path) else [mesh_path]
        if not paths or not all(os.path.exists(p) for p in paths):
            raise FileNotFoundError(f'no {ext} meshes at {mesh_path}')
        return [torch.from_numpy(np.asarray(read_ply(p).verts, dtype=np.float32)) for p in paths]

    def to(self, device):
        return self

    def _class_tables(self, device):
        """(verts, offsets, symmetric, diameter, max_points) of the class meshes on ``device``, built once."""
        device = torch.device(device)
        if device not in self._tables:
            from .mesh import MeshStore
            meshes = self.meshes
            if isinstance(meshes, MeshStore):
                dm = meshes.on(device)
                verts, offsets = dm.verts, dm.vert_offset
                counts = np.diff(meshes.vert_offset)
            else:
                arrs = [np.ascontiguousarray(m.detach().cpu().numpy() if isinstance(m, torch.Tensor) else m,
                                             dtype=np.float32).reshape(-1, 3) for m in meshes]
                counts = np.array([len(a) for a in arrs], dtype=np.int64)
                verts = torch.from_numpy(np.concatenate(arrs) if arrs else np.zeros((0, 3), np.float32)).to(device)
                offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)).to(device)
            if verts.numel() == 0:
                raise ValueError(f'{type(self).__name__}: the meshes hold no vertices')
            self._tables[device] = (verts, offsets, *self._class_flags(len(counts), device), int(counts.max()))
        return self._tables[device]

    def _class_flags(self, num_classes, device):
        if len(self.mesh_diameter) < num_classes:
            raise ValueError(f'mesh_diameter has {len(self.mesh_diameter)} entries for {num_classes} classes')
        # membership of the KEY, as the reference tests it
        sym = [int(f'cls_{c + 1}' in self.symmetry_types) for c in range(num_classes)]
        diam = [float(self.mesh_diameter[c]) for c in range(num_classes)]
        return (torch.tensor(sym, dtype=torch.int32, device=device),
                torch.tensor(diam, dtype=torch.float32, device=device))

    def _flags(self):
        return 0

    def sequence(self, seq_r, seq_t, gt_r, gt_t, labels, points_list=None, scale_factors=None, gamma=0.8,
                 return_nn=False):
        """all iterations in one launch -> (total (0-dim), per_iter (T), loss_i (T,N), nn_idx or None).  The total
        carries a graph when grad mode is on and a prediction requires a gradient."""
        if _wants_graph(seq_r, seq_t):
            def run_grad(det, want):
                out = self._run(det[0], det[1], gt_r, gt_t, labels, points_list, scale_factors, gamma, return_nn, True, want)
                return out[0], out[1:4], (out[4], out[5])
            total, extras = _through_autograd([list(seq_r), None if seq_t is None else list(seq_t)], run_grad)
            return (total,) + tuple(extras)
        return self._run(seq_r, seq_t, gt_r, gt_t, labels, points_list, scale_factors, gamma, return_nn)

    def sequence_grad(self, seq_r, seq_t, gt_r, gt_t, labels, points_list=None, scale_factors=None, gamma=0.8,
                      return_nn=False):
        """-> (total, per_iter, loss_i, nn_idx, grad_r, grad_t): ``sequence`` plus the gradients of the total with respect
        to every rotation and translation (``grad_t`` None for rotations only); no graph."""
        return self._run(seq_r, seq_t, gt_r, gt_t, labels, points_list, scale_factors, gamma, return_nn, True)

    def _run(self, seq_r, seq_t, gt_r, gt_t, labels, points_list, scale_factors, gamma, return_nn, grad=False,
             want=(True, True)):
        ops._dev(gt_r, 'gt_r')
        if not isinstance(labels, torch.Tensor) or not labels.is_cuda:
            raise _lib.ScflowHipError('labels: expected a tensor on the GPU (HIP path only, no CPU fallback)')
        dev = gt_r.device
        n = int(gt_r.shape[0])
        lab32 = labels.to(torch.int32).contiguous()
        flags = self._flags()
        if flags & (PM_SCALE_XY | PM_SCALE_DEPTH):
            assert scale_factors is not None
        if self.use_perspective_shape:
            assert points_list is not None
            pts = []
            for i, p in enumerate(points_list):
                ops._dev(p, f'points_list[{i}]')
                pts.append(p.reshape(-1, 3))
            if len(pts) != n:
                raise ValueError(f'points_list has {len(pts)} entries for {n} samples')
            counts = [int(p.shape[0]) for p in pts]
            verts = torch.cat(pts).contiguous()
            offsets = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32, device=dev)
            group = torch.arange(n, dtype=torch.int32, device=dev)
            sym, diam = self._class_flags(len(self.mesh_diameter), dev)
            max_points = max(counts)
        else:
            verts, offsets, sym, diam, max_points = self._class_tables(dev)
            group = lab32
        args = (verts, offsets, group, lab32, sym, diam, seq_r, seq_t, gt_r, gt_t,
                scale_factors if flags & (PM_SCALE_XY | PM_SCALE_DEPTH) else None, max_points, self._mode, self.loss_type,
                flags, getattr(self, 'scale_depth_factor', 1.), self.reduction, self.loss_weight, gamma, return_nn)
        if not grad:
            loss_i, per_iter, total, nn_idx = point_matching_loss(*args)
            return total[0], per_iter, loss_i, nn_idx
        loss_i, per_iter, total, nn_idx, grad_r, grad_t = point_matching_loss_grad(*args, want=want)
        return total[0], per_iter, loss_i, nn_idx, grad_r, grad_t


@LOSSES.register_module()
class PointMatchingLoss(_PointMatchingBase):
    """point_matching_loss.py:14-103."""
    _mode = PM_FULL

    def __init__(self, symmetry_types, mesh_diameter, scale_xy=False, scale_depth=False, scale_depth_factor=1.,
                 use_perspective_shape=False, mesh_path=None, loss_weight=1.0, reduction='mean', loss_type='l2'):
        self._init_common(symmetry_types, mesh_diameter, use_perspective_shape, mesh_path, loss_weight, reduction,
                          loss_type)
        self.scale_depth, self.scale_xy, self.scale_depth_factor = scale_depth, scale_xy, scale_depth_factor

    def _flags(self):
        return (PM_SCALE_XY if self.scale_xy else 0) | (PM_SCALE_DEPTH if self.scale_depth else 0)

    def forward(self, pred_r, pred_t, gt_r, gt_t, labels, points_list=None, scale_factors=None):
        out = self.sequence([pred_r], [pred_t], gt_r, gt_t, labels, points_list, scale_factors)
        return out[0] if out[0].requires_grad else out[1][0]           # one iteration: the total IS the value (weight 1)

    __call__ = forward


@LOSSES.register_module()
class DisentanglePointMatchingLoss(PointMatchingLoss):
    """point_matching_loss.py:106-218 (https://arxiv.org/abs/1905.12365): the rotation term uses the ground-truth
    translation on both sides; the translation term (or, with ``disentangle_z``, the depth and the xy terms) the
    ground-truth rotation."""
    _mode = PM_DISENTANGLE

    def __init__(self, symmetry_types, mesh_diameter, scale_xy=False, scale_depth=False, scale_depth_factor=1.,
                 use_perspective_shape=False, disentangle_z=False, mesh_path=None, loss_weight=1.0, reduction='mean',
                 loss_type='l2'):
        super().__init__(symmetry_types, mesh_diameter, scale_xy, scale_depth, scale_depth_factor,
                         use_perspective_shape, mesh_path, loss_weight, reduction, loss_type)
        self.disentagle_z = disentangle_z                  # the reference's spelling

    def _flags(self):
        return super()._flags() | (PM_DISENTANGLE_Z if self.disentagle_z else 0)


@LOSSES.register_module()
class RotPointMatchingLoss(_PointMatchingBase):
    """point_matching_loss.py:221-291: rotations only."""
    _mode = PM_ROT

    def __init__(self, symmetry_types, mesh_diameter, use_perspective_shape=False, mesh_path=None, loss_weight=1.0,
                 loss_type='l2', reduction='mean'):
        self._init_common(symmetry_types, mesh_diameter, use_perspective_shape, mesh_path, loss_weight, reduction,
                          loss_type)

    def forward(self, pred_r, gt_r, labels, points_list=None):
        out = self.sequence([pred_r], None, gt_r, None, labels, points_list)
        return out[0] if out[0].requires_grad else out[1][0]

    __call__ = forward


_PIXEL = (RAFTLoss, L1Loss)
_POINT = (PointMatchingLoss, DisentanglePointMatchingLoss, RotPointMatchingLoss)


@LOSSES.register_module()
class SequenceLoss:
    """sequence_loss.py:41-82: ``sum_i gamma**(T-1-i) * loss_func(preds[..][i], **kwargs)`` -> (loss, [loss_i]).
    One launch for all iterations when ``loss_func`` is one of this module's classes; the reference's loop for any other
    class registered in ``LOSSES``.  ``value_and_grad`` adds the gradients of ``loss`` with respect to every prediction
    (this module's classes only); with predictions that require a gradient, ``loss`` carries a graph and ``[loss_i]``
    stays detached."""

    def __init__(self, loss_func_cfg: dict, gamma: float = 0.8) -> None:
        self.loss_func = build_loss(loss_func_cfg)
        self.gamma = gamma

    def to(self, device):
        self.loss_func.to(device)
        return self

    def forward(self, *preds, **kwargs):
        f = self.loss_func
        n_preds = len(preds[0])
        if type(f) in _PIXEL and n_preds:
            total, per_iter = f.sequence(preds[0], *preds[1:], gamma=self.gamma, **kwargs)
            return total, list(per_iter.unbind(0))
        if type(f) in _POINT and n_preds:
            if f._mode == PM_ROT:
                total, per_iter, _, _ = f.sequence(preds[0], None, kwargs['gt_r'], None, kwargs['labels'],
                                                   kwargs.get('points_list'), gamma=self.gamma)
            else:
                total, per_iter, _, _ = f.sequence(preds[0], preds[1], gamma=self.gamma, **kwargs)
            return total, list(per_iter.unbind(0))
        # any other registered class: one call per iteration, weighted gamma^(T-1), ..., gamma^0 and added in that order
        values = [f(*(seq[step] for seq in preds), **kwargs) for step in range(n_preds)]
        total = 0.
        for step, value in enumerate(values):
            total = total + self.gamma ** (n_preds - 1 - step) * value
        return total, values

    __call__ = forward

    def value_and_grad(self, *preds, **kwargs):
        """-> (loss, [loss_i], grads): ``forward`` and d loss / d preds from the same launch; ``grads`` is a tuple of
        lists that mirrors ``preds``.  No graph is built, whatever the predictions require."""
        f = self.loss_func
        if not ((type(f) in _PIXEL or type(f) in _POINT) and len(preds[0])):
            raise NotImplementedError(f'value_and_grad: no gradient kernel for {type(f).__name__}; it exists for '
                                      + ', '.join(c.__name__ for c in _PIXEL + _POINT))
        det = [[t.detach() for t in seq] for seq in preds]
        if type(f) in _PIXEL:
            total, per_iter, grads = f.sequence_grad(det[0], *det[1:], gamma=self.gamma, **kwargs)
            return total, list(per_iter.unbind(0)), grads
        if f._mode == PM_ROT:
            out = f.sequence_grad(det[0], None, kwargs['gt_r'], None, kwargs['labels'], kwargs.get('points_list'),
                                  gamma=self.gamma)
            return out[0], list(out[1].unbind(0)), (out[4],)
        out = f.sequence_grad(det[0], det[1], gamma=self.gamma, **kwargs)
        return out[0], list(out[1].unbind(0)), (out[4], out[5])
