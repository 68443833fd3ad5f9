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
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import ops
from .mesh import MeshStore

Tensor = torch.Tensor

__all__ = ['PatchPipeline', 'TrainPatchPipeline']

_FIELD_WORDS = ('mask', 'depth')
_POSE_FIELD = ['ref_rotations', 'ref_translations']


class _PatchStage:
    """what the two pipelines share: the settings behind ``scf_patch_params``, the ``from_cfg`` steps both read, and the
    host-list bookkeeping of ``__call__``."""

    _required = ('ComputeBbox', 'Crop', 'Resize', 'Pad', 'RemapPose', 'Normalize')
    _ignored = ('LoadImages', 'ToTensor', 'Collect')
    _filter_invalid_default = True

    def __init__(self, mesh_store, size, img_scale, size_ratio, aspect_ratio, keep_ratio, min_expand, clip_border,
                 fix_clip_border_quirk, center, crop_pad_val, pad_val, mean, std, to_rgb, vertex_stride):
        self.store = mesh_store
        self.size = (int(size[0]), int(size[1]))
        self.img_scale = int(img_scale)
        self.settings = dict(size_ratio=float(size_ratio), aspect_ratio=float(aspect_ratio), keep_ratio=bool(keep_ratio),
                             min_expand=float(min_expand), clip_border=bool(clip_border),
                             fix_clip_border_quirk=bool(fix_clip_border_quirk), center=bool(center),
                             crop_pad_val=crop_pad_val, pad_val=pad_val, mean=tuple(float(m) for m in mean),
                             std=tuple(float(s) for s in std), to_rgb=bool(to_rgb), vertex_stride=int(vertex_stride))
        self.params = ops.patch_params(self.size, self.img_scale, **self.settings)
        self.img_norm_cfg = dict(mean=list(self.settings['mean']), std=list(self.settings['std']), to_rgb=bool(to_rgb))
        self._frame_index: Dict = {}

    # ------------------------------------------------------------------------------------------ from_cfg
    @classmethod
    def _refuse(cls, what: str):
        raise NotImplementedError(f'{cls.__name__}: {what}')

    @classmethod
    def _own_step(cls, kind: str, step: dict, kw: Dict) -> bool:
        """what the subclass alone reads or refuses of a step, into ``kw``; called for every step.  -> whether ``kind`` is a
        step of its own (consulted only for a kind that is neither shared nor ignored: it decides "unknown transform")."""
        return False

    @classmethod
    def _read_cfg(cls, pipeline: Sequence[dict], kw: Dict) -> List[str]:
        """walk the reference's pipeline list: what both pipelines read of ComputeBbox, Crop, Resize, Pad, RemapPose and
        Normalize goes into ``kw`` here, the rest of every step to ``_own_step``.  -> the step names, in order."""
        seen: List[str] = []
        for step in pipeline:
            step = dict(step)
            kind = step.pop('type', None)
            seen.append(kind)
            shared = True
            if kind == 'ComputeBbox':
                if step.get('clip_border', True):
                    cls._refuse('ComputeBbox(clip_border=True)')
                if step.get('filter_invalid', cls._filter_invalid_default):
                    cls._refuse('ComputeBbox(filter_invalid=True) (it drops whole images on the host)')
                if list(step.get('pose_field', _POSE_FIELD)) != _POSE_FIELD:
                    cls._refuse(f"ComputeBbox(pose_field={step['pose_field']!r})")
            elif kind == 'Crop':
                kw.update(keep_ratio=step.get('keep_ratio', False), aspect_ratio=step.get('aspect_ratio', 1.),
                          crop_pad_val=step.get('pad_val', 128), min_expand=step.get('min_expand', 0),
                          clip_border=step.get('clip_border', True))
            elif kind == 'Resize':
                if not step.get('keep_ratio', True):
                    cls._refuse('Resize(keep_ratio=False)')
                scale = step['img_scale']
                if isinstance(scale, (list, tuple)):
                    if len(set(int(s) for s in scale)) != 1:
                        cls._refuse(f'Resize(img_scale={scale!r}) with unequal sides')
                    scale = scale[0]
                kw['img_scale'] = int(scale)
            elif kind == 'Pad':
                pad_val = step.get('pad_val', dict(img=0, mask=0))
                kw.update(size=tuple(step['size']), center=step.get('center', False), pad_val=pad_val.get('img', 0))
            elif kind == 'RemapPose':
                if step.get('keep_intrinsic', True):
                    cls._refuse("RemapPose(keep_intrinsic=True) ('keep_intrinsic' mode re-solves the pose)")
                if step.get('dst_k') is not None:
                    cls._refuse("RemapPose(dst_k=...) ('target_intrinsic' mode re-solves the pose)")
            elif kind == 'Normalize':
                kw.update(mean=step['mean'], std=step['std'], to_rgb=step.get('to_rgb', True))
            else:
                shared = False
            own = cls._own_step(kind, step, kw)
            if not (shared or own or kind in cls._ignored):
                cls._refuse(f'unknown transform {kind!r}')
        for need in cls._required:
            if need not in seen:
                cls._refuse(f'a pipeline without {need}')
        return seen

    # --------------------------------------------------------------------------------------------- call
    def _index(self, counts: Sequence[int], device) -> Tensor:
        """frame index of every object, from the host list (uploaded once per distinct list and device)."""
        key = (tuple(counts), str(device))
        if key not in self._frame_index:
            idx = [i for i, n in enumerate(counts) for _ in range(n)]
            self._frame_index[key] = torch.tensor(idx, dtype=torch.int32).to(device)
        return self._frame_index[key]

    @staticmethod
    def _counts(frames: Tensor, per_img_patch_num: Sequence[int], k: Tensor, flat) -> Tuple[List[int], int]:
        """the host list as ints and its sum N, checked against the frames and the length of every (name, tensor) of
        ``flat``."""
        counts = [int(n) for n in per_img_patch_num]
        if frames.dim() != 4 or len(counts) != frames.shape[0] or min(counts) < 0:
            raise ValueError(f'per_img_patch_num needs one non-negative count per frame ({len(counts)} for '
                             f'{tuple(frames.shape)} frames)')
        n = sum(counts)
        if n != k.shape[0]:
            raise ValueError(f'per_img_patch_num sums to {n} but k holds {k.shape[0]} objects')
        for name, t in flat:
            if t.shape[0] != n:
                raise ValueError(f'{name} holds {t.shape[0]} objects, expected {n}')
        return counts, n

    @staticmethod
    def _ori_k(k: Tensor, counts: Sequence[int]) -> List[Tensor]:
        """the first object's K of every image (zeros for an image without objects)."""
        out, start = [], 0
        for c in counts:
            out.append(k[start] if c else k.new_zeros((3, 3)))
            start += c
        return out

    def _metas(self, counts: Sequence[int], scale: Tensor, n: int) -> List[dict]:
        """one ``img_metas`` entry per image."""
        shape = (self.size[0], self.size[1], 3)
        return [dict(img_norm_cfg=self.img_norm_cfg, geometry_transform_mode='adapt_intrinsic', img_shape=[shape] * c,
                     scale_factor=s) for c, s in zip(counts, scale[:, None].expand(n, 4).split(counts))]


class PatchPipeline(_PatchStage):
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
        super().__init__(mesh_store, size, img_scale, size_ratio, aspect_ratio, keep_ratio, min_expand, clip_border,
                         fix_clip_border_quirk, center, crop_pad_val, pad_val, mean, std, to_rgb, vertex_stride)

    @classmethod
    def _own_step(cls, kind: str, step: dict, kw: Dict) -> bool:
        if kind == 'Collect':
            keys = list(step.get('annot_keys', ())) + list(step.get('meta_keys', ()))
            bad = [k for k in keys if any(w in k for w in _FIELD_WORDS)]
            if bad:
                cls._refuse(f'depth or mask fields {bad} (image patches only)')
        elif kind == 'Crop':
            lo, hi = step.get('size_range', (0.8, 1.2))
            if float(lo) != float(hi):
                cls._refuse(f'Crop(size_range={(lo, hi)}) with unequal ends (a random size ratio is a training augmentation)')
            kw['size_ratio'] = float(lo)
        return False

    @classmethod
    def from_cfg(cls, pipeline: Sequence[dict], mesh_store: Optional[MeshStore], **overrides) -> 'PatchPipeline':
        """from the reference's ``val_pipeline`` list, unchanged.  Reads ComputeBbox, Crop, Resize, Pad, RemapPose and
        Normalize (absent keys take the reference classes' defaults), ignores LoadImages, ToTensor and Collect."""
        kw: Dict = {}
        cls._read_cfg(pipeline, kw)
        last = {step.get('type'): step for step in pipeline}
        bbox_field = last['ComputeBbox'].get('bbox_field', 'ref_bboxes')
        crop_field = last['Crop'].get('crop_bbox_field', 'ref_bboxes')
        if crop_field != bbox_field:
            cls._refuse(f'Crop(crop_bbox_field={crop_field!r}) is not the box ComputeBbox writes ({bbox_field!r}); '
                        'pass detector rectangles per call as crop_rects instead')
        kw.update(overrides)
        return cls(mesh_store, **kw)

    def __call__(self, frames: Tensor, per_img_patch_num: Sequence[int], ref_rotations: Tensor, ref_translations: Tensor,
                 k: Tensor, labels: Tensor, gt_rotations: Optional[Tensor] = None,
                 gt_translations: Optional[Tensor] = None, crop_rects: Optional[Tensor] = None) -> Dict:
        """frames (F,Hf,Wf,3) uint8 BGR on the GPU, ``per_img_patch_num`` a HOST list of F object counts (sum N), the
        rest flat over the N objects in frame order: ref_rotations / k (N,3,3), ref_translations (N,3), labels (N,).
        ``crop_rects`` (N,4) int (x1, y1, x2, y2) replaces the projected box and the crop rule (a detector's box).
        -> a ``data_batch`` for ``format_data_test`` (img, annots, img_metas: per-image lists, views of the flat
        tensors) plus ``flat`` (img, box, k, transform_matrix, crop, scale, valid) and ``valid``.  No host
        synchronisation: the per-image splits come from the host list."""
        flat = (('gt_rotations', gt_rotations), ('gt_translations', gt_translations), ('ref_rotations', ref_rotations),
                ('ref_translations', ref_translations), ('labels', labels))
        counts, n = self._counts(frames, per_img_patch_num, k, [(name, t) for name, t in flat if t is not None])
        if crop_rects is None and self.store is None:
            raise ValueError('PatchPipeline was built without a MeshStore: every call needs crop_rects')
        dev = frames.device
        mesh = self.store.on(dev) if crop_rects is None else None
        k = k.contiguous()
        box = ops.patch_boxes(mesh, labels, ref_rotations.contiguous(), ref_translations.contiguous(), k,
                              (frames.shape[1], frames.shape[2]), self.params, crop_rects=crop_rects)
        img = ops.extract_patches(frames, self._index(counts, dev), box['records'], self.params)

        def split(t):
            return list(t.split(counts))
        annots = dict(ref_rotations=split(ref_rotations), ref_translations=split(ref_translations), labels=split(labels),
                      k=split(box['k']), transform_matrix=split(box['transform_matrix']), ori_k=self._ori_k(k, counts))
        if gt_rotations is not None:
            annots['gt_rotations'] = split(gt_rotations)
        if gt_translations is not None:
            annots['gt_translations'] = split(gt_translations)
        flat = dict(img=img, box=box['box'], k=box['k'], transform_matrix=box['transform_matrix'], crop=box['crop'], scale=box['scale'],
                    valid=box['valid'])
        return dict(img=split(img), annots=annots, img_metas=self._metas(counts, box['scale'], n), flat=flat, valid=box['valid'])


# ------------------------------------------------------------------------------------------------ train
_TRAIN_REFUSED = ('RandomBackground', 'RandomSharpness', 'RandomGray', 'RandomOcclusion', 'RandomOcclusionV2')
_TRAIN_ANNOTS = ('ref_rotations', 'ref_translations', 'gt_rotations', 'gt_translations', 'gt_masks', 'init_add_error',
                 'init_rot_error', 'init_trans_error', 'k', 'labels')
_TRAIN_ORDER = ('Crop', 'RandomHSV', 'RandomNoise', 'RandomSmooth', 'Resize')


class TrainPatchPipeline(_PatchStage):
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

    _required = ('PoseJitter',) + _PatchStage._required
    _ignored = ('LoadImages', 'LoadMasks', 'ToTensor', 'Collect')
    # the shipped train_pipeline leaves ComputeBbox's filter_invalid at its default (True: an image with a box larger than
    # the frame is dropped on the host); an absent key is accepted and NO image is dropped here -- flat['box'] lets the
    # caller filter -- while an explicit True is refused
    _filter_invalid_default = False

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
        super().__init__(mesh_store, size, img_scale, size_range[0], aspect_ratio, keep_ratio, min_expand, clip_border,
                         fix_clip_border_quirk, center, crop_pad_val, pad_val, mean, std, to_rgb, vertex_stride)
        self.vertex_stride = int(vertex_stride)
        self.aug_settings = dict(jitter_angle_dis=tuple(jitter_angle_dis), jitter_x_dis=tuple(jitter_x_dis),
                                 jitter_y_dis=tuple(jitter_y_dis), jitter_z_dis=tuple(jitter_z_dis),
                                 angle_limit=angle_limit, translation_limit=translation_limit, add_limit=add_limit,
                                 max_tries=max_tries, size_range=tuple(size_range), h_ratio=h_ratio, s_ratio=s_ratio,
                                 v_ratio=v_ratio, hsv_p=hsv_p, noise_ratio=noise_ratio, noise_p=noise_p,
                                 max_kernel_size=max_kernel_size, smooth_p=smooth_p,
                                 fix_error_swap_quirk=fix_error_swap_quirk, mask_pad_val=mask_pad_val)
        self.seed = int(seed)
        self.aug = ops.patch_aug_params(seed=self.seed, **self.aug_settings)
        self.id_base = 0

    def reset(self, step: int = 0) -> 'TrainPatchPipeline':
        """the next call without ``sample_ids`` numbers its objects from ``step``."""
        if int(step) != step or step < 0:
            raise ValueError(f'TrainPatchPipeline.reset: step must be a non-negative integer, got {step!r}')
        self.id_base = int(step)
        return self

    @classmethod
    def _own_step(cls, kind: str, step: dict, kw: Dict) -> bool:
        if kind == 'Collect':
            keys = list(step.get('annot_keys', ())) + list(step.get('meta_keys', ()))
            bad = [k for k in keys if 'depth' in k]
            if bad:
                cls._refuse(f'depth fields {bad}')
            more = [k for k in step.get('annot_keys', ()) if k not in _TRAIN_ANNOTS + ('ori_k', 'transform_matrix')]
            if more:
                cls._refuse(f'annotation fields {more}')
        elif kind in _TRAIN_REFUSED:
            cls._refuse(f'{kind}' + (' (it reads image files)' if kind == 'RandomBackground' else ''))
        elif kind == 'PoseJitter':
            if list(step.get('jitter_pose_field', ())) != ['gt_rotations', 'gt_translations'] or \
                    list(step.get('jittered_pose_field', ())) != _POSE_FIELD:
                cls._refuse('PoseJitter with pose fields other than gt_* -> ref_*')
            for key in ('jitter_angle_dis', 'jitter_x_dis', 'jitter_y_dis', 'jitter_z_dis'):
                kw[key] = tuple(step[key])
            kw.update(angle_limit=step.get('angle_limit'), translation_limit=step.get('translation_limit'),
                      add_limit=step.get('add_limit'))
            if step.get('mesh_diameter') is not None:
                kw['mesh_diameter'] = list(step['mesh_diameter'])
        elif kind == 'ComputeBbox':
            if step.get('bbox_field', 'ref_bboxes') != 'ref_bboxes':
                cls._refuse(f"ComputeBbox(bbox_field={step['bbox_field']!r})")
        elif kind == 'Crop':
            if step.get('crop_bbox_field', 'ref_bboxes') != 'ref_bboxes':
                cls._refuse(f"Crop(crop_bbox_field={step['crop_bbox_field']!r})")
            kw['size_range'] = tuple(step.get('size_range', (0.8, 1.2)))
        elif kind == 'RandomHSV':
            kw.update(h_ratio=step['h_ratio'], s_ratio=step['s_ratio'], v_ratio=step['v_ratio'], hsv_p=step.get('p', 1.0))
        elif kind == 'RandomNoise':
            kw.update(noise_ratio=step['noise_ratio'], noise_p=step.get('p', 1.0))
        elif kind == 'RandomSmooth':
            kw.update(max_kernel_size=step.get('max_kernel_size', 7), smooth_p=step.get('p', 1.0))
        elif kind == 'Pad':
            kw['mask_pad_val'] = step.get('pad_val', dict(img=0, mask=0)).get('mask', 0)
        else:
            return False
        return True

    @classmethod
    def from_cfg(cls, pipeline: Sequence[dict], mesh_store: MeshStore, **overrides) -> 'TrainPatchPipeline':
        """from the reference's ``train_pipeline`` list, unchanged.  Reads PoseJitter (``mesh_diameter`` included),
        ComputeBbox, Crop, RandomHSV, RandomNoise, RandomSmooth, Resize, Pad, RemapPose and Normalize (absent keys take
        the reference classes' defaults; an absent colour transform is switched off), ignores LoadImages, LoadMasks,
        ToTensor and Collect.  Everything else raises ``NotImplementedError`` by name."""
        kw: Dict = dict(hsv_p=0.0, noise_p=0.0, smooth_p=0.0)
        seen = cls._read_cfg(pipeline, kw)
        order = [k for k in seen if k in _TRAIN_ORDER]
        if order != [k for k in _TRAIN_ORDER if k in order]:
            cls._refuse(f'the order {order} (the kernels run Crop, RandomHSV, RandomNoise, RandomSmooth, Resize)')
        kw.update(overrides)
        if 'mesh_diameter' not in kw:
            cls._refuse('a PoseJitter without mesh_diameter (pass mesh_diameter=...)')
        diam = kw.pop('mesh_diameter')
        return cls(mesh_store, diam, **kw)

    def __call__(self, frames: Tensor, per_img_patch_num: Sequence[int], gt_rotations: Tensor, gt_translations: Tensor,
                 k: Tensor, labels: Tensor, masks: Tensor, sample_ids: Optional[Tensor] = None) -> Dict:
        """frames (F,Hf,Wf,3) uint8 BGR on the GPU, ``per_img_patch_num`` a HOST list of F object counts (sum N), the rest
        flat over the N objects in frame order: gt_rotations / k (N,3,3), gt_translations (N,3), labels (N,), masks
        (N,Hf,Wf) uint8 or bool, one full-frame mask per object (what LoadMasks yields), ``sample_ids`` (N,) int64 or None.
        -> a ``data_batch`` for ``format_data_train_sup`` (img, annots, img_metas: per-image lists, views of the flat
        tensors) plus ``flat`` and ``valid``.  ``flat['draws']`` holds the drawn scalars per object: ratio, a, b, c, sigma,
        k (columns 0..5).  No host synchronisation."""
        counts, n = self._counts(frames, per_img_patch_num, k, (('gt_rotations', gt_rotations),
                                                                ('gt_translations', gt_translations), ('labels', labels),
                                                                ('masks', masks)))
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
            return list(t.split(counts))
        annots = dict(ref_rotations=split(jit['rot']), ref_translations=split(jit['trans']),
                      gt_rotations=split(gt_rotations), gt_translations=split(gt_translations), gt_masks=split(gt_masks),
                      init_add_error=split(jit['add_error']), init_rot_error=split(jit['rot_error']),
                      init_trans_error=split(jit['trans_error']), k=split(box['k']), labels=split(labels))
        metas = self._metas(counts, box['scale'], n)
        for meta, tm, ori_k in zip(metas, box['transform_matrix'].split(counts), self._ori_k(k, counts)):
            meta['transform_matrix'], meta['ori_k'] = tm, ori_k
        flat = dict(img=img, gt_masks=gt_masks, box=box['box'], k=box['k'], transform_matrix=box['transform_matrix'],
                    crop=box['crop'], scale=box['scale'], valid=box['valid'], draws=box['draws'],
                    ref_rotations=jit['rot'], ref_translations=jit['trans'], init_add_error=jit['add_error'],
                    init_rot_error=jit['rot_error'], init_trans_error=jit['trans_error'], jitter_ok=jit['ok'],
                    jitter_tries=jit['tries'], records=box['records'])
        return dict(img=split(img), annots=annots, img_metas=metas, flat=flat, valid=box['valid'])
