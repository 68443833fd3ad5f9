"""Object patches from full frames: ``PatchPipeline``.

The reference builds the refiner's input object by object on the CPU with a cv2 / mmcv chain, the ``val_pipeline``
of configs/refine_datasets/ycbv_*.py: ComputeBbox, Crop, Resize, Pad, RemapPose(keep_intrinsic=False), Normalize.
``PatchPipeline`` runs that chain for a whole batch with ``scf_patch_boxes`` and ``scf_patch_extract``
(scflow_amd/csrc/patch.hip states the semantics) and returns a ``data_batch`` that ``format_data_test`` accepts as it
stands, so frame + initial poses -> refined poses stays on the device.  It implements what the shipped pipeline uses;
everything else raises ``NotImplementedError`` at construction, by name.  cv2 bit parity is not claimed (cv2 is not
a dependency); tests/test_patches_host.py holds the restatement the kernels are held to, bit for bit.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import torch

from . import ops
from .mesh import MeshStore

Tensor = torch.Tensor

__all__ = ['PatchPipeline']

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
