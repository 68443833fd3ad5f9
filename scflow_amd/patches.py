"""Object patches from full frames: ``PatchPipeline`` (the val path) and ``TrainPatchPipeline`` (the train path).

The reference builds the refiner's input object by object on the CPU with a cv2 / mmcv chain, the ``val_pipeline``
of configs/refine_datasets/ycbv_*.py: ComputeBbox, Crop, Resize, Pad, RemapPose(keep_intrinsic=False), Normalize.
``PatchPipeline`` runs that chain for a whole batch with ``scf_patch_boxes`` and ``scf_patch_extract``
(scflow_amd/csrc/patch.hip states the semantics) and returns a ``data_batch`` that ``format_data_test`` accepts as it
stands, so frame + initial poses -> refined poses stays on the device.  It implements what the shipped pipeline uses;
everything else raises ``NotImplementedError`` at construction, by name.  cv2 bit parity is not claimed (cv2 is not
a dependency); tests/test_patches_host.py holds the restatement the kernels are held to, bit for bit.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence

import torch

from . import ops
from .mesh import MeshStore

Tensor = torch.Tensor

__all__ = ['PatchPipeline', 'TrainPatchPipeline']

_IGNORED = ('LoadImages', 'ToTensor', 'Collect')
_FIELD_WORDS = ('mask', 'depth')


def _unsupported(what: str):
    raise NotImplementedError(f'PatchPipeline: {what}')


class PatchPipeline:
    """crop, resize, pad and normalise one patch per object, and adapt its intrinsics, on the GPU.

    ``vertex_stride``: the box takes every ``vertex_stride``-th vertex of the class mesh (the reference draws 1000
    random ones; see patch.hip).  ``crop_pad_val`` is Crop's fill, ``pad_val`` Pad's ``pad_val['img']``; both are in
    the frame's channel order (BGR).  ``mean`` / ``std`` are in grey levels and index the output channels."""

    def __init__(self, mesh_store: Optional[MeshStore], *, size=(256, 256), img_scale: int = 256, size_ratio: float = 1.1,
                 aspect_ratio: float = 1.0, keep_ratio: bool = False, min_expand: float = 0.0, clip_border: bool = False,
                 fix_clip_border_quirk: bool = False, center: bool = True, crop_pad_val=128, pad_val=128,
                 mean: Sequence[float] = (0., 0., 0.), std: Sequence[float] = (255., 255., 255.), to_rgb: bool = True,
                 vertex_stride: int = 1):
        if mesh_store is not None and not isinstance(mesh_store, MeshStore):
            raise TypeError('PatchPipeline: mesh_store must be a MeshStore (or None when every call brings crop_rects)')
        self.store = mesh_store
        self.size = (int(size[0]), int(size[1]))
        self.settings = dict(size_ratio=float(size_ratio), aspect_ratio=float(aspect_ratio), keep_ratio=bool(keep_ratio),
                             min_expand=float(min_expand), clip_border=bool(clip_border),
                             fix_clip_border_quirk=bool(fix_clip_border_quirk), center=bool(center),
                             crop_pad_val=crop_pad_val, pad_val=pad_val, mean=tuple(float(m) for m in mean),
                             std=tuple(float(s) for s in std), to_rgb=bool(to_rgb), vertex_stride=int(vertex_stride))
        self.img_scale = int(img_scale)
        self.params = ops.patch_params(self.size, self.img_scale, **self.settings)
        self.img_norm_cfg = dict(mean=list(self.settings['mean']), std=list(self.settings['std']), to_rgb=bool(to_rgb))
        self._frame_index: Dict = {}

    # ------------------------------------------------------------------------------------------ from_cfg
    @classmethod
    def from_cfg(cls, pipeline: Sequence[dict], mesh_store: Optional[MeshStore], **overrides) -> 'PatchPipeline':
        """from the reference's ``val_pipeline`` list, unchanged.  Reads ComputeBbox, Crop, Resize, Pad, RemapPose and
        Normalize (absent keys take the reference classes' defaults), ignores LoadImages, ToTensor and Collect."""
        kw: Dict = {}
        seen: List[str] = []
        bbox_field, crop_field = 'ref_bboxes', 'ref_bboxes'
        for step in pipeline:
            step = dict(step)
            kind = step.pop('type', None)
            seen.append(kind)
            if kind in _IGNORED:
                if kind == 'Collect':
                    keys = list(step.get('annot_keys', ())) + list(step.get('meta_keys', ()))
                    bad = [k for k in keys if any(w in k for w in _FIELD_WORDS)]
                    if bad:
                        _unsupported(f'depth or mask fields {bad} (image patches only)')
                continue
            if kind == 'ComputeBbox':
                if step.get('clip_border', True):
                    _unsupported('ComputeBbox(clip_border=True)')
                if step.get('filter_invalid', True):
                    _unsupported('ComputeBbox(filter_invalid=True) (it drops whole images on the host)')
                if list(step.get('pose_field', ['ref_rotations', 'ref_translations'])) != ['ref_rotations', 'ref_translations']:
                    _unsupported(f"ComputeBbox(pose_field={step['pose_field']!r})")
                bbox_field = step.get('bbox_field', 'ref_bboxes')
            elif kind == 'Crop':
                lo, hi = step.get('size_range', (0.8, 1.2))
                if float(lo) != float(hi):
                    _unsupported(f'Crop(size_range={(lo, hi)}) with unequal ends (a random size ratio is a training augmentation)')
                crop_field = step.get('crop_bbox_field', 'ref_bboxes')
                kw.update(size_ratio=float(lo), keep_ratio=step.get('keep_ratio', False),
                          aspect_ratio=step.get('aspect_ratio', 1.), crop_pad_val=step.get('pad_val', 128),
                          min_expand=step.get('min_expand', 0), clip_border=step.get('clip_border', True))
            elif kind == 'Resize':
                if not step.get('keep_ratio', True):
                    _unsupported('Resize(keep_ratio=False)')
                scale = step['img_scale']
                if isinstance(scale, (list, tuple)):
                    if len(set(int(s) for s in scale)) != 1:
                        _unsupported(f'Resize(img_scale={scale!r}) with unequal sides')
                    scale = scale[0]
                kw['img_scale'] = int(scale)
            elif kind == 'Pad':
                pad_val = step.get('pad_val', dict(img=0, mask=0))
                kw.update(size=tuple(step['size']), center=step.get('center', False), pad_val=pad_val.get('img', 0))
            elif kind == 'RemapPose':
                if step.get('keep_intrinsic', True):
                    _unsupported("RemapPose(keep_intrinsic=True) ('keep_intrinsic' mode re-solves the pose)")
                if step.get('dst_k') is not None:
                    _unsupported("RemapPose(dst_k=...) ('target_intrinsic' mode re-solves the pose)")
            elif kind == 'Normalize':
                kw.update(mean=step['mean'], std=step['std'], to_rgb=step.get('to_rgb', True))
            else:
                _unsupported(f'unknown transform {kind!r}')
        for need in ('ComputeBbox', 'Crop', 'Resize', 'Pad', 'RemapPose', 'Normalize'):
            if need not in seen:
                _unsupported(f'a pipeline without {need}')
        if crop_field != bbox_field:
            _unsupported(f'Crop(crop_bbox_field={crop_field!r}) is not the box ComputeBbox writes ({bbox_field!r}); '
                         'pass detector rectangles per call as crop_rects instead')
        kw.update(overrides)
        return cls(mesh_store, **kw)

    # --------------------------------------------------------------------------------------------- call
    def _index(self, per_img_patch_num: Sequence[int], device) -> Tensor:
        """frame index of every object, from the host list (uploaded once per distinct list and device)."""
        key = (tuple(int(n) for n in per_img_patch_num), str(device))
        if key not in self._frame_index:
            idx = [i for i, n in enumerate(key[0]) for _ in range(n)]
            self._frame_index[key] = torch.tensor(idx, dtype=torch.int32).to(device)
        return self._frame_index[key]

    def __call__(self, frames: Tensor, per_img_patch_num: Sequence[int], ref_rotations: Tensor, ref_translations: Tensor,
                 k: Tensor, labels: Tensor, gt_rotations: Optional[Tensor] = None,
                 gt_translations: Optional[Tensor] = None, crop_rects: Optional[Tensor] = None) -> Dict:
        """frames (F,Hf,Wf,3) uint8 BGR on the GPU, ``per_img_patch_num`` a HOST list of F object counts (sum N), the
        rest flat over the N objects in frame order: ref_rotations / k (N,3,3), ref_translations (N,3), labels (N,).
        ``crop_rects`` (N,4) int (x1, y1, x2, y2) replaces the projected box and the crop rule (a detector's box).
        -> a ``data_batch`` for ``format_data_test`` (img, annots, img_metas: per-image lists, views of the flat
        tensors) plus ``flat`` (img, box, k, transform_matrix, crop, scale, valid) and ``valid``.  No host
        synchronisation: the per-image splits come from the host list."""
        counts = [int(n) for n in per_img_patch_num]
        if frames.dim() != 4 or len(counts) != frames.shape[0] or min(counts) < 0:
            raise ValueError(f'per_img_patch_num needs one non-negative count per frame ({len(counts)} for '
                             f'{tuple(frames.shape)} frames)')
        n = sum(counts)
        if n != k.shape[0]:
            raise ValueError(f'per_img_patch_num sums to {n} but k holds {k.shape[0]} objects')
        for name, t in (('gt_rotations', gt_rotations), ('gt_translations', gt_translations),
                        ('ref_rotations', ref_rotations), ('ref_translations', ref_translations), ('labels', labels)):
            if t is not None and t.shape[0] != n:
                raise ValueError(f'{name} holds {t.shape[0]} objects, expected {n}')
        if crop_rects is None and self.store is None:
            raise ValueError('PatchPipeline was built without a MeshStore: every call needs crop_rects')
        dev = frames.device
        mesh = self.store.on(dev) if crop_rects is None else None
        k = k.contiguous()
        box = ops.patch_boxes(mesh, labels, ref_rotations.contiguous(), ref_translations.contiguous(), k,
                              (frames.shape[1], frames.shape[2]), self.params, crop_rects=crop_rects)
        img = ops.extract_patches(frames, self._index(counts, dev), box['records'], self.params)

        def split(t):
            return list(torch.split(t, counts))
        starts = [sum(counts[:i]) for i in range(len(counts))]
        annots = dict(ref_rotations=split(ref_rotations), ref_translations=split(ref_translations), labels=split(labels),
                      k=split(box['k']), transform_matrix=split(box['transform_matrix']),
                      ori_k=[k[s] if c else k.new_zeros((3, 3)) for s, c in zip(starts, counts)])
        if gt_rotations is not None:
            annots['gt_rotations'] = split(gt_rotations)
        if gt_translations is not None:
            annots['gt_translations'] = split(gt_translations)
        shape = (self.size[0], self.size[1], 3)
        scale4 = box['scale'][:, None].expand(n, 4)
        metas = [dict(img_norm_cfg=self.img_norm_cfg, geometry_transform_mode='adapt_intrinsic', img_shape=[shape] * c,
                      scale_factor=s) for c, s in zip(counts, split(scale4))]
        flat = dict(img=img, box=box['box'], k=box['k'], transform_matrix=box['transform_matrix'], crop=box['crop'], scale=box['scale'],
                    valid=box['valid'])
        return dict(img=split(img), annots=annots, img_metas=metas, flat=flat, valid=box['valid'])


# ------------------------------------------------------------------------------------------------ train
_TRAIN_IGNORED = ('LoadImages', 'LoadMasks', 'ToTensor', 'Collect')
_TRAIN_REFUSED = ('RandomBackground', 'RandomSharpness', 'RandomGray', 'RandomOcclusion', 'RandomOcclusionV2')
_TRAIN_ANNOTS = ('ref_rotations', 'ref_translations', 'gt_rotations', 'gt_translations', 'gt_masks', 'init_add_error',
                 'init_rot_error', 'init_trans_error', 'k', 'labels')


def _unsupported_train(what: str):
    raise NotImplementedError(f'TrainPatchPipeline: {what}')


class TrainPatchPipeline:
    """the reference's ``train_pipeline`` (configs/refine_datasets/ycbv_real.py:27-72) for a whole batch on the GPU:
    PoseJitter, ComputeBbox, Crop with a random size ratio, RandomHSV, RandomNoise, RandomSmooth, Resize, Pad,
    RemapPose(keep_intrinsic=False), Normalize, and the ground-truth masks through Crop, Resize and Pad.
    scflow_amd/csrc/patch_train.hip states the semantics (cv2 parity is not claimed).  It returns a ``data_batch`` that
    ``format_data_train_sup`` -- and therefore ``loss()`` -- accepts as it stands.

    ``mesh_diameter``: one diameter per class label (a sequence indexed by label, or a dict).  Every random draw is a
    function of (seed, sample id, stream, counter): an object's result does not depend on its batch.  Without
    ``sample_ids`` object n of a call gets id ``id_base + n`` and ``id_base`` advances by N per call; ``reset(step)``
    sets it back, which makes a run repeatable.  Limits of None are not applied; a ``p`` of 0 switches a transform off.
    ``fix_error_swap_quirk``: the reference stores the translation error as init_rot_error and the angle as
    init_trans_error (jitter.py:79 against :93); that is reproduced unless this is set."""

    def __init__(self, mesh_store: MeshStore, mesh_diameter, seed: int = 0, *, size=(256, 256), img_scale: int = 256,
                 size_range=(1.0, 1.25), aspect_ratio: float = 1.0, keep_ratio: bool = False, min_expand: float = 0.0,
                 clip_border: bool = False, fix_clip_border_quirk: bool = False, center: bool = True, crop_pad_val=128,
                 pad_val=128, mask_pad_val: int = 0, mean: Sequence[float] = (0., 0., 0.),
                 std: Sequence[float] = (255., 255., 255.), to_rgb: bool = True, vertex_stride: int = 1,
                 jitter_angle_dis=(0., 15.), jitter_x_dis=(0., 15.), jitter_y_dis=(0., 15.), jitter_z_dis=(0., 50.),
                 angle_limit: Optional[float] = 45., translation_limit: Optional[float] = 200.,
                 add_limit: Optional[float] = 1., max_tries: int = 64, h_ratio: float = 0.2, s_ratio: float = 0.5,
                 v_ratio: float = 0.5, hsv_p: float = 1.0, noise_ratio: float = 0.1, noise_p: float = 1.0,
                 max_kernel_size: float = 5, smooth_p: float = 1.0, fix_error_swap_quirk: bool = False):
        if not isinstance(mesh_store, MeshStore):
            raise TypeError('TrainPatchPipeline: mesh_store must be a MeshStore')
        self.store = mesh_store
        if isinstance(mesh_diameter, dict):               # a class without a mesh needs none: its objects are refused
            mesh_diameter = [mesh_diameter.get(l, None if l in mesh_store.meshes else 1.0)
                             for l in range(mesh_store.num_classes)]
        if len(mesh_diameter) < mesh_store.num_classes:
            raise ValueError(f'TrainPatchPipeline: mesh_diameter holds {len(mesh_diameter)} classes, the mesh store '
                             f'{mesh_store.num_classes}')
        bad = {l: d for l, d in enumerate(mesh_diameter[:mesh_store.num_classes])
               if d is None or not (math.isfinite(float(d)) and float(d) > 0)}
        if bad:                                           # NaN would pass every ADD comparison, 0 would fail every one
            raise ValueError(f'TrainPatchPipeline: mesh_diameter must be finite and positive for every class, got {bad}')
        diam = [float(d) for d in mesh_diameter]
        self.diameters = torch.tensor(diam[:mesh_store.num_classes], dtype=torch.float32)
        self._diam_dev: Dict = {}
        self.size = (int(size[0]), int(size[1]))
        self.img_scale = int(img_scale)
        self.vertex_stride = int(vertex_stride)
        self.settings = dict(size_ratio=float(size_range[0]), aspect_ratio=float(aspect_ratio), keep_ratio=bool(keep_ratio),
                             min_expand=float(min_expand), clip_border=bool(clip_border),
                             fix_clip_border_quirk=bool(fix_clip_border_quirk), center=bool(center),
                             crop_pad_val=crop_pad_val, pad_val=pad_val, mean=tuple(float(m) for m in mean),
                             std=tuple(float(s) for s in std), to_rgb=bool(to_rgb), vertex_stride=self.vertex_stride)
        self.params = ops.patch_params(self.size, self.img_scale, **self.settings)
        self.aug_settings = dict(jitter_angle_dis=tuple(jitter_angle_dis), jitter_x_dis=tuple(jitter_x_dis),
                                 jitter_y_dis=tuple(jitter_y_dis), jitter_z_dis=tuple(jitter_z_dis),
                                 angle_limit=angle_limit, translation_limit=translation_limit, add_limit=add_limit,
                                 max_tries=max_tries, size_range=tuple(size_range), h_ratio=h_ratio, s_ratio=s_ratio,
                                 v_ratio=v_ratio, hsv_p=hsv_p, noise_ratio=noise_ratio, noise_p=noise_p,
                                 max_kernel_size=max_kernel_size, smooth_p=smooth_p,
                                 fix_error_swap_quirk=fix_error_swap_quirk, mask_pad_val=mask_pad_val)
        self.seed = int(seed)
        self.aug = ops.patch_aug_params(seed=self.seed, **self.aug_settings)
        self.img_norm_cfg = dict(mean=list(self.settings['mean']), std=list(self.settings['std']), to_rgb=bool(to_rgb))
        self.id_base = 0
        self._frame_index: Dict = {}

    def reset(self, step: int = 0) -> 'TrainPatchPipeline':
        """the next call without ``sample_ids`` numbers its objects from ``step``."""
        if int(step) != step or step < 0:
            raise ValueError(f'TrainPatchPipeline.reset: step must be a non-negative integer, got {step!r}')
        self.id_base = int(step)
        return self

    # ------------------------------------------------------------------------------------------ from_cfg
    @classmethod
    def from_cfg(cls, pipeline: Sequence[dict], mesh_store: MeshStore, **overrides) -> 'TrainPatchPipeline':
        """from the reference's ``train_pipeline`` list, unchanged.  Reads PoseJitter (``mesh_diameter`` included),
        ComputeBbox, Crop, RandomHSV, RandomNoise, RandomSmooth, Resize, Pad, RemapPose and Normalize (absent keys take
        the reference classes' defaults; an absent colour transform is switched off), ignores LoadImages, LoadMasks,
        ToTensor and Collect.  Everything else raises ``NotImplementedError`` by name."""
        kw: Dict = dict(hsv_p=0.0, noise_p=0.0, smooth_p=0.0)
        seen: List[str] = []
        for step in pipeline:
            step = dict(step)
            kind = step.pop('type', None)
            seen.append(kind)
            if kind in _TRAIN_IGNORED:
                if kind == 'Collect':
                    keys = list(step.get('annot_keys', ())) + list(step.get('meta_keys', ()))
                    bad = [k for k in keys if 'depth' in k]
                    if bad:
                        _unsupported_train(f'depth fields {bad}')
                    more = [k for k in step.get('annot_keys', ()) if k not in _TRAIN_ANNOTS + ('ori_k', 'transform_matrix')]
                    if more:
                        _unsupported_train(f'annotation fields {more}')
                continue
            if kind in _TRAIN_REFUSED:
                _unsupported_train(f'{kind}' + (' (it reads image files)' if kind == 'RandomBackground' else ''))
            if kind == 'PoseJitter':
                if list(step.get('jitter_pose_field', ())) != ['gt_rotations', 'gt_translations'] or \
                        list(step.get('jittered_pose_field', ())) != ['ref_rotations', 'ref_translations']:
                    _unsupported_train('PoseJitter with pose fields other than gt_* -> ref_*')
                for key in ('jitter_angle_dis', 'jitter_x_dis', 'jitter_y_dis', 'jitter_z_dis'):
                    kw[key] = tuple(step[key])
                kw.update(angle_limit=step.get('angle_limit'), translation_limit=step.get('translation_limit'),
                          add_limit=step.get('add_limit'))
                if step.get('mesh_diameter') is not None:
                    kw['mesh_diameter'] = list(step['mesh_diameter'])
            elif kind == 'ComputeBbox':
                if step.get('clip_border', True):
                    _unsupported_train('ComputeBbox(clip_border=True)')
                # the shipped train_pipeline leaves filter_invalid at its default (True: an image with a box larger than
                # the frame is dropped on the host); an absent key is accepted and NO image is dropped here -- flat['box']
                # lets the caller filter -- while an explicit True is refused
                if step.get('filter_invalid', False):
                    _unsupported_train('ComputeBbox(filter_invalid=True) (it drops whole images on the host)')
                if list(step.get('pose_field', ['ref_rotations', 'ref_translations'])) != ['ref_rotations', 'ref_translations']:
                    _unsupported_train(f"ComputeBbox(pose_field={step['pose_field']!r})")
                if step.get('bbox_field', 'ref_bboxes') != 'ref_bboxes':
                    _unsupported_train(f"ComputeBbox(bbox_field={step['bbox_field']!r})")
            elif kind == 'Crop':
                if step.get('crop_bbox_field', 'ref_bboxes') != 'ref_bboxes':
                    _unsupported_train(f"Crop(crop_bbox_field={step['crop_bbox_field']!r})")
                kw.update(size_range=tuple(step.get('size_range', (0.8, 1.2))), keep_ratio=step.get('keep_ratio', False),
                          aspect_ratio=step.get('aspect_ratio', 1.), crop_pad_val=step.get('pad_val', 128),
                          min_expand=step.get('min_expand', 0), clip_border=step.get('clip_border', True))
            elif kind == 'RandomHSV':
                kw.update(h_ratio=step['h_ratio'], s_ratio=step['s_ratio'], v_ratio=step['v_ratio'], hsv_p=step.get('p', 1.0))
            elif kind == 'RandomNoise':
                kw.update(noise_ratio=step['noise_ratio'], noise_p=step.get('p', 1.0))
            elif kind == 'RandomSmooth':
                kw.update(max_kernel_size=step.get('max_kernel_size', 7), smooth_p=step.get('p', 1.0))
            elif kind == 'Resize':
                if not step.get('keep_ratio', True):
                    _unsupported_train('Resize(keep_ratio=False)')
                scale = step['img_scale']
                if isinstance(scale, (list, tuple)):
                    if len(set(int(s) for s in scale)) != 1:
                        _unsupported_train(f'Resize(img_scale={scale!r}) with unequal sides')
                    scale = scale[0]
                kw['img_scale'] = int(scale)
            elif kind == 'Pad':
                pad_val = step.get('pad_val', dict(img=0, mask=0))
                kw.update(size=tuple(step['size']), center=step.get('center', False), pad_val=pad_val.get('img', 0),
                          mask_pad_val=pad_val.get('mask', 0))
            elif kind == 'RemapPose':
                if step.get('keep_intrinsic', True):
                    _unsupported_train("RemapPose(keep_intrinsic=True) ('keep_intrinsic' mode re-solves the pose)")
                if step.get('dst_k') is not None:
                    _unsupported_train("RemapPose(dst_k=...) ('target_intrinsic' mode re-solves the pose)")
            elif kind == 'Normalize':
                kw.update(mean=step['mean'], std=step['std'], to_rgb=step.get('to_rgb', True))
            else:
                _unsupported_train(f'unknown transform {kind!r}')
        for need in ('PoseJitter', 'ComputeBbox', 'Crop', 'Resize', 'Pad', 'RemapPose', 'Normalize'):
            if need not in seen:
                _unsupported_train(f'a pipeline without {need}')
        order = [k for k in seen if k in ('Crop', 'RandomHSV', 'RandomNoise', 'RandomSmooth', 'Resize')]
        if order != [k for k in ('Crop', 'RandomHSV', 'RandomNoise', 'RandomSmooth', 'Resize') if k in order]:
            _unsupported_train(f'the order {order} (the kernels run Crop, RandomHSV, RandomNoise, RandomSmooth, Resize)')
        kw.update(overrides)
        if 'mesh_diameter' not in kw:
            _unsupported_train('a PoseJitter without mesh_diameter (pass mesh_diameter=...)')
        diam = kw.pop('mesh_diameter')
        return cls(mesh_store, diam, **kw)

    # --------------------------------------------------------------------------------------------- call
    def _index(self, counts, device) -> Tensor:
        key = (tuple(counts), str(device))
        if key not in self._frame_index:
            idx = [i for i, n in enumerate(counts) for _ in range(n)]
            self._frame_index[key] = torch.tensor(idx, dtype=torch.int32).to(device)
        return self._frame_index[key]

    def __call__(self, frames: Tensor, per_img_patch_num: Sequence[int], gt_rotations: Tensor, gt_translations: Tensor,
                 k: Tensor, labels: Tensor, masks: Tensor, sample_ids: Optional[Tensor] = None) -> Dict:
        """frames (F,Hf,Wf,3) uint8 BGR on the GPU, ``per_img_patch_num`` a HOST list of F object counts (sum N), the rest
        flat over the N objects in frame order: gt_rotations / k (N,3,3), gt_translations (N,3), labels (N,), masks
        (N,Hf,Wf) uint8 or bool, one full-frame mask per object (what LoadMasks yields), ``sample_ids`` (N,) int64 or None.
        -> a ``data_batch`` for ``format_data_train_sup`` (img, annots, img_metas: per-image lists, views of the flat
        tensors) plus ``flat`` and ``valid``.  ``flat['draws']`` holds the drawn scalars per object: ratio, a, b, c, sigma,
        k (columns 0..5).  No host synchronisation."""
        counts = [int(n) for n in per_img_patch_num]
        if frames.dim() != 4 or len(counts) != frames.shape[0] or min(counts) < 0:
            raise ValueError(f'per_img_patch_num needs one non-negative count per frame ({len(counts)} for '
                             f'{tuple(frames.shape)} frames)')
        n = sum(counts)
        if n != k.shape[0]:
            raise ValueError(f'per_img_patch_num sums to {n} but k holds {k.shape[0]} objects')
        for name, t in (('gt_rotations', gt_rotations), ('gt_translations', gt_translations), ('labels', labels),
                        ('masks', masks)):
            if t.shape[0] != n:
                raise ValueError(f'{name} holds {t.shape[0]} objects, expected {n}')
        dev = frames.device
        mesh = self.store.on(dev)
        if dev not in self._diam_dev:
            self._diam_dev[dev] = self.diameters.to(dev)
        base = self.id_base
        if sample_ids is None:
            self.id_base += n
        k = k.contiguous()
        gt_rotations, gt_translations = gt_rotations.contiguous(), gt_translations.contiguous()
        jit = ops.pose_jitter(mesh, self._diam_dev[dev], labels, gt_rotations, gt_translations, self.aug,
                              vertex_stride=self.vertex_stride, id_base=base, sample_ids=sample_ids)
        box = ops.patch_boxes_train(mesh, labels, jit['rot'], jit['trans'], k, (frames.shape[1], frames.shape[2]),
                                    self.params, self.aug, id_base=base, sample_ids=sample_ids)
        img, gt_masks = ops.extract_patches_train(frames, self._index(counts, dev), box['records'], self.params, self.aug,
                                                  masks=masks.contiguous())

        def split(t):
            return list(torch.split(t, counts))
        annots = dict(ref_rotations=split(jit['rot']), ref_translations=split(jit['trans']),
                      gt_rotations=split(gt_rotations), gt_translations=split(gt_translations), gt_masks=split(gt_masks),
                      init_add_error=split(jit['add_error']), init_rot_error=split(jit['rot_error']),
                      init_trans_error=split(jit['trans_error']), k=split(box['k']), labels=split(labels))
        starts = [sum(counts[:i]) for i in range(len(counts))]
        shape = (self.size[0], self.size[1], 3)
        scale4 = box['scale'][:, None].expand(n, 4)
        metas = [dict(img_norm_cfg=self.img_norm_cfg, geometry_transform_mode='adapt_intrinsic', img_shape=[shape] * c,
                      scale_factor=s, transform_matrix=tm, ori_k=k[st] if c else k.new_zeros((3, 3)))
                 for c, s, tm, st in zip(counts, split(scale4), split(box['transform_matrix']), starts)]
        flat = dict(img=img, gt_masks=gt_masks, box=box['box'], k=box['k'], transform_matrix=box['transform_matrix'],
                    crop=box['crop'], scale=box['scale'], valid=box['valid'], draws=box['draws'],
                    ref_rotations=jit['rot'], ref_translations=jit['trans'], init_add_error=jit['add_error'],
                    init_rot_error=jit['rot_error'], init_trans_error=jit['trans_error'], jitter_ok=jit['ok'],
                    jitter_tries=jit['tries'], records=box['records'])
        return dict(img=split(img), annots=annots, img_metas=metas, flat=flat, valid=box['valid'])
