"""``SCFlowRefiner`` -- the drop-in boundary of the hot path.

Mirrors models/refiner/scflow_refiner.py:18-179 (+ base_refiner.py:17-64):
same registry name, constructor keys (``configs/refine_models/scflow.py:16-113``
applies unchanged), attribute names, ``extract_feat`` / ``get_pose`` /
``forward_single_pass`` signatures and return structure, same ``state_dict``
keys.  Losses and PnP re-mapping are outside the hot path:
their config keys are accepted and ignored, and ``forward_single_pass`` consumes an
already formatted ``data`` dict (what ``BaseRefiner.format_data_test`` produces,
base_refiner.py:79-133).  The config's ``renderer`` dict is ignored too;
``attach_renderer(MeshRenderer(...))`` enables ``format_data_test``, ``update_data``
and ``test_cfg['cycles'] > 1`` on the HIP renderer (scflow_amd/mesh.py).
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple, Union

import torch

from . import ops
from .modules import HipModule, encoder_pair_supported, raft_encoder_pair
from .ops import ACT_RELU, ACT_TANH, small_work
from .registry import REFINERS, build_decoder, build_encoder

Tensor = torch.Tensor


def _as_mask_tensor(mask, device) -> Tensor:
    """a gt mask as a bool tensor: tensors pass through, mmdet-style mask objects go through to_tensor."""
    if isinstance(mask, torch.Tensor):
        return mask.to(device=device, dtype=torch.bool)
    return mask.to_tensor(dtype=torch.bool, device=device)


class _RenderingRefiner:
    """the renderer-driven data path of BaseRefiner (base_refiner.py:79-133, 205-218) on ``MeshRenderer``:
    ``attach_renderer``, ``format_data_test`` and ``update_data``.  The constructor ignores the config's
    ``renderer`` dict (its dataset paths need not exist where the model is built)."""

    renderer = None

    def attach_renderer(self, renderer):
        """use ``renderer`` (a ``MeshRenderer``, or None to detach) for format_data_test / update_data and for
        ``test_cfg['cycles'] > 1``; returns self."""
        self.renderer = renderer
        return self

    def _need_renderer(self, what: str):
        if self.renderer is None:
            raise RuntimeError(f'{what} renders the mesh: attach a renderer first (attach_renderer(MeshRenderer(...)))')

    def format_data_test(self, data_batch: Dict) -> Dict:
        """base_refiner.py:79-133: concatenate the per-image lists, render every sample at its reference pose and
        normalise the rendered RGB with ``img_metas[0]['img_norm_cfg']`` (the kernel writes it in NCHW, already
        normalised).  ``gt_masks`` may be tensors or objects with ``to_tensor``."""
        self._need_renderer('format_data_test')
        real_images, annots, meta_infos = data_batch['img'], data_batch['annots'], data_batch['img_metas']
        per_img_patch_num = [len(images) for images in real_images]
        real_images = torch.cat(real_images)
        ref_rotations = torch.cat(annots['ref_rotations'], dim=0)
        ref_translations = torch.cat(annots['ref_translations'], dim=0)
        labels = torch.cat(annots['labels'])
        internel_k = torch.cat(annots['k'])
        output = dict(real_images=real_images, labels=labels, internel_k=internel_k,
                      ref_rotations=ref_rotations, ref_translations=ref_translations,
                      per_img_patch_num=per_img_patch_num, meta_infos=meta_infos)
        if 'transform_matrix' in annots:
            output['transform_matrix'] = torch.cat(annots['transform_matrix'])
        if 'ori_k' in annots:
            output['ori_k'] = torch.cat([k[None].expand(n, 3, 3) for k, n in zip(annots['ori_k'], per_img_patch_num)])
        norm = meta_infos[0]['img_norm_cfg']
        # the reference's torch.Tensor(mean) / 255. (fp32), handed to the kernel as its per-channel constants
        mean = (torch.tensor(norm['mean'], dtype=torch.float32) / 255.).tolist()
        std = (torch.tensor(norm['std'], dtype=torch.float32) / 255.).tolist()
        rgb, depth, mask = self.renderer.render_normalized(ref_rotations, ref_translations, internel_k, labels, mean, std)
        output.update(rendered_images=rgb, rendered_depths=depth, rendered_masks=mask)
        if 'depths' in annots:
            output['real_depths'] = torch.cat(annots['depths'], dim=0)
        if 'gt_rotations' in annots:
            output['gt_rotations'] = torch.cat(annots['gt_rotations'], dim=0)
            output['gt_translations'] = torch.cat(annots['gt_translations'], dim=0)
        if 'gt_masks' in annots:
            output['gt_masks'] = torch.cat([_as_mask_tensor(m, real_images.device) for m in annots['gt_masks']], dim=0)
        return output

    def update_data(self, update_rotations: Tensor, update_translations: Tensor, data: Dict) -> Dict:
        """base_refiner.py:205-218: re-render at the updated pose.  As in the reference, the new rendered images are
        NOT normalised with img_norm_cfg (format_data_test's are)."""
        self._need_renderer('update_data')
        data['ref_rotations'] = update_rotations
        data['ref_translations'] = update_translations
        rgb, depth, mask = self.renderer.render_normalized(update_rotations, update_translations, data['internel_k'],
                                                           data['labels'])
        data['rendered_images'] = rgb
        data['rendered_depths'] = depth
        data['rendered_masks'] = mask
        return data


@REFINERS.register_module()
class SCFlowRefiner(_RenderingRefiner, HipModule):
    def __init__(self, seperate_encoder: bool, cxt_channels: int, h_channels: int,
                 cxt_encoder: dict, encoder: dict, decoder: dict, renderer: Optional[dict] = None,
                 pose_loss_cfg: Optional[dict] = None, flow_loss_cfg: Optional[dict] = None,
                 mask_loss_cfg: Optional[dict] = None, max_flow: float = 400,
                 render_augmentations: Optional[list] = None, filter_invalid_flow: bool = True,
                 freeze_encoder: bool = False, freeze_bn: bool = False,
                 train_cfg: Optional[dict] = None, test_cfg: Optional[dict] = None,
                 init_cfg: Optional[Union[list, dict]] = None) -> None:
        super().__init__()
        self.seperate_encoder = seperate_encoder
        if seperate_encoder:
            self.render_encoder = build_encoder(encoder)
            self.real_encoder = build_encoder(encoder)
        else:                                   # base_refiner.py:36-39: one module, two names
            enc = build_encoder(encoder)
            self.render_encoder = enc
            self.real_encoder = enc
        self.decoder = build_decoder(decoder)
        self.context = build_encoder(cxt_encoder)
        # the config's renderer dict points at dataset paths: it is not built here; attach_renderer() sets one
        self.renderer = None
        self.max_flow = max_flow
        self.train_cfg = train_cfg or {}
        self.test_cfg = test_cfg or {}
        self.h_channels, self.cxt_channels = h_channels, cxt_channels
        assert self.h_channels == self.decoder.h_channels
        assert self.cxt_channels == self.decoder.cxt_channels
        assert self.h_channels + self.cxt_channels == self.context.out_channels
        self.filter_invalid_flow = filter_invalid_flow
        self.test_by_flow = self.test_cfg.get('by_flow', False)
        self.test_iter_num = self.test_cfg.get('iters', self.decoder.iters)
        self.eval()

    # -------------------------------------------------------------- features
    def extract_feat(self, render_images: Tensor, real_images: Tensor
                     ) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
        """scflow_refiner.py:88-110 -> (render_feat, real_feat, h_feat, cxt_feat).

        The shared feature encoder runs ONCE on the 2N stacked images (InstanceNorm is per
        sample, so this equals two separate passes); the context encoder's 1x1 head writes
        tanh(h) | relu(cxt) straight into the first 256 channels of the GRU input buffer."""
        n, _, H, W = render_images.shape
        dev = render_images.device
        ops._dev(render_images, 'render_images')        # GPU fp32 on the current device, or raise
        ops._dev(real_images, 'real_images')
        hc, cc = self.h_channels, self.cxt_channels
        sc = int(round(1 / self.context.scale))
        # allocated BEFORE the fork: the side branch writes it while the main stream keeps going, so
        # its memory must not be a block the allocator recycles from main-stream temporaries that
        # are enqueued after the fork (they could still be running when the side branch writes)
        hx = torch.empty((n, hc + cc + 128, H // sc, W // sc), dtype=torch.float32, device=dev)
        # ... and so is everything the side branch READS: a non-contiguous render_images is
        # materialised here, on the main stream, before the fork event (a copy enqueued after it
        # would not be ordered before the side branch's first read)
        rend = render_images.contiguous()
        ov_ctx = small_work(n, H, W, 'context')
        fork = ops.fork_point() if ov_ctx else None     # the context encoder may start from here
        if (not self.seperate_encoder and ops.branch_mode(n, H, W, 'context') == 2 and ops._CONV_EVENTS is None
                and encoder_pair_supported(self.render_encoder, self.context)):
            # r6: the context encoder's launches ride in the feature encoder's (modules.raft_encoder_pair; IN | BN encoders)
            both = torch.empty((2 * n, 3, H, W), dtype=torch.float32, device=dev)
            ops.copy_channels(rend, both[:n])
            ops.copy_channels(real_images.contiguous(), both[n:])
            feats, _ = raft_encoder_pair(self.render_encoder, both, self.context, rend, out_c=hx[:, :hc + cc],
                                         head_act=ACT_TANH, head_act2=ACT_RELU, head_split=hc)
            return feats[:n], feats[n:], hx[:, :hc], hx[:, hc:hc + cc]
        if self.seperate_encoder:
            render_feat = self.render_encoder(rend)
            real_feat = self.real_encoder(real_images.contiguous())
        else:
            both = torch.empty((2 * n, 3, H, W), dtype=torch.float32, device=dev)
            ops.copy_channels(rend, both[:n])
            ops.copy_channels(real_images.contiguous(), both[n:])
            feats = self.render_encoder(both)
            render_feat, real_feat = feats[:n], feats[n:]
        br = ops.side_stream(ov_ctx, after=fork)        # small batches: next to the feature encoder
        with br:
            self.context(rend, out=hx[:, :hc + cc], head_act=ACT_TANH,
                         head_act2=ACT_RELU, head_split=hc)
        br.join()
        return render_feat, real_feat, hx[:, :hc], hx[:, hc:hc + cc]

    # ------------------------------------------------------------------ pose
    def get_pose(self, render_images: Tensor, real_images: Tensor, ref_rotation: Tensor,
                 ref_translation: Tensor, depth: Tensor, internel_k: Tensor, label: Tensor,
                 init_flow: Optional[Tensor] = None):
        """scflow_refiner.py:112-142 -> 7-tuple of length-``iters`` lists
        (flow_from_pose, flow_from_pred, rotation_preds, translation_preds, mask_preds,
        delta_rotation_preds, delta_translation_preds)."""
        feat_render, feat_real, h_feat, cxt_feat = self.extract_feat(render_images, real_images)
        if init_flow is None:
            n, _, H, W = real_images.shape
            init_flow = ops.constant((n, 2, H, W), 0.0, feat_render.device)      # read-only, filled once
        return self.decoder(feat_render, feat_real, h_feat, cxt_feat, ref_rotation,
                            ref_translation, depth.contiguous(), internel_k.contiguous(),
                            label=label, init_flow=init_flow, invalid_flow_num=0.,
                            _consume_state=True)      # h / cxt are ours: update them in place

    def forward_single_pass(self, data: Dict, data_batch: Optional[Dict] = None,
                            return_loss: bool = False) -> Dict:
        """scflow_refiner.py:146-179 minus ``remap_pose_to_origin_resoluaion`` (identity for the
        'adapt_intrinsic' pipeline of the config; cv2 EPnP otherwise -- out of scope)."""
        labels = data['labels']
        per_img = data['per_img_patch_num']
        # the reference's index_select (pose_head.py:209) raises on an out-of-range class id;
        # the pose-update kernel cannot raise (it clamps), so the check lives at this entry
        nc = self.decoder.pose_pred.num_class
        # (one reduction, one device->host transfer; skipped while the stream is being captured
        # into a hipGraph, where a synchronising read is illegal: validate before capturing)
        if labels.numel() and not (labels.is_cuda and torch.cuda.is_current_stream_capturing()):
            lo, hi = torch.stack(torch.aminmax(labels)).tolist()
            if lo < 0 or hi >= nc:
                raise IndexError(f'label out of range [0, {nc}): min {lo}, max {hi}')
        iters = self.decoder.iters
        self.decoder.iters = self.test_iter_num
        try:
            outs = self.get_pose(data['rendered_images'], data['real_images'],
                                 data['ref_rotations'], data['ref_translations'],
                                 data['rendered_depths'], data['internel_k'], labels)
        finally:
            self.decoder.iters = iters
        rot, trans = outs[2][-1], outs[3][-1]
        return dict(rotations=torch.split(rot, per_img), translations=torch.split(trans, per_img),
                    labels=torch.split(labels, per_img),
                    scores=torch.split(torch.ones_like(labels, dtype=torch.float32), per_img))

    def forward(self, data, data_batch=None, return_loss=False):
        if return_loss:
            raise NotImplementedError('training is outside the hot path (SURVEY.md section 2)')
        if self.test_cfg.get('cycles', 1) > 1:
            # base_refiner.py:250-258: every further cycle RE-RENDERS the object at the updated pose (update_data).
            # Without an attached renderer, refuse instead of silently running one cycle.
            if self.renderer is None:
                raise NotImplementedError("test_cfg['cycles'] > 1 needs the renderer between cycles (base_refiner.py:250-258); "
                                          'attach one with attach_renderer(MeshRenderer(...)), or render outside and call '
                                          'forward_single_pass / get_pose once per cycle')
            return self.forward_multiple_pass(data, data_batch)
        return self.forward_single_pass(data, data_batch)

    def forward_multiple_pass(self, data: Dict, data_batch: Optional[Dict] = None) -> Dict:
        """base_refiner.py:249-261: ``test_cfg['cycles']`` passes, re-rendering at each refined pose in between.  The
        caller's dict is not modified (the reference updates it in place)."""
        data = dict(data)
        cycles = self.test_cfg.get('cycles', 1)
        for i in range(cycles):
            results = self.forward_single_pass(data, data_batch)
            if i == cycles - 1:
                break
            data = self.update_data(torch.cat(results['rotations']), torch.cat(results['translations']), data)
        return results


class _FlowRefinerBase(_RenderingRefiner, HipModule):
    """feature extraction, ``get_flow`` and the pose step of the pose-free RAFT refiners
    (models/refiner/raft_refiner_flow_mask.py:88-161, raft_refiner_flow.py, base_flow_refiner.py:99-154).

    The reference's pose step is cv2 RANSAC-EPnP on the CPU (models/utils/pose.py:203-249).  Here it is the batched
    HIP solver (``ops.pnp``: the same algorithm class, another sampler, no cv2 bit parity), selected explicitly with
    ``test_cfg['solve_pose_mode'] = 'hip_ransac_epnp'``; the reference's own modes ('ransacpnp', the default, and
    'progressive-x') raise ``NotImplementedError``, so the solver is never silently substituted for cv2.
    ``test_cfg['solve_pose_param']`` takes iterationscount (100), reprojectionerror (3.0) and seed (0);
    ``test_cfg['sample_points']`` (num, mode) and ``occ_thresh`` (0.5) act as in the reference."""

    def __init__(self, seperate_encoder: bool, cxt_channels: int, h_channels: int,
                 cxt_encoder: dict, encoder: dict, decoder: dict, test_cfg: Optional[dict] = None,
                 **ignored) -> None:
        super().__init__()
        self.seperate_encoder = seperate_encoder
        if seperate_encoder:
            self.render_encoder = build_encoder(encoder)
            self.real_encoder = build_encoder(encoder)
        else:
            enc = build_encoder(encoder)
            self.render_encoder = enc
            self.real_encoder = enc
        self.decoder = build_decoder(decoder)
        self.context = build_encoder(cxt_encoder)
        self.h_channels, self.cxt_channels = h_channels, cxt_channels
        self.test_cfg = test_cfg or {}
        self.test_iter_num = self.test_cfg.get('iters', self.decoder.iters)
        self.eval()

    extract_feat = SCFlowRefiner.extract_feat

    def get_flow(self, render_images: Tensor, real_images: Tensor,
                 init_flow: Optional[Tensor] = None):
        """raft_refiner_flow_mask.py:120-133: init_flow defaults to zeros at 1/8 resolution."""
        feat_render, feat_real, h_feat, cxt_feat = self.extract_feat(render_images, real_images)
        if init_flow is None:
            b, _, h, w = feat_real.shape
            init_flow = ops.constant((b, 2, h, w), 0.0, feat_real.device)
        return self.decoder(feat_render, feat_real, init_flow, h_feat, cxt_feat, _consume_state=True)

    HIP_PNP_MODE = 'hip_ransac_epnp'
    _has_occlusion = False

    def _pnp_kwargs(self) -> dict:
        mode = self.test_cfg.get('solve_pose_mode', 'ransacpnp')
        if mode == 'ransacpnp':
            raise NotImplementedError(
                "solve_pose_mode 'ransacpnp' is cv2.solvePnPRansac on the CPU (models/utils/pose.py:203-249), which "
                f"this package does not ship; set test_cfg['solve_pose_mode'] = '{self.HIP_PNP_MODE}' for the batched "
                'HIP RANSAC-EPnP solver (same algorithm class, different sampler: not bit-equal to cv2)')
        if mode != self.HIP_PNP_MODE:
            raise NotImplementedError(f'solve_pose_mode {mode!r} is not implemented; the HIP solver is '
                                      f"test_cfg['solve_pose_mode'] = '{self.HIP_PNP_MODE}'")
        prm = self.test_cfg.get('solve_pose_param', {}) or {}
        kw = dict(iterations=prm.get('iterationscount', 100), reproj_error=prm.get('reprojectionerror', 3.0),
                  seed=prm.get('seed', 0))
        sample = self.test_cfg.get('sample_points', None)
        if sample is not None:
            # base_flow_refiner.py:65-71: 'random', or top-k by confidence for any other mode
            kw.update(sample_mode='random' if sample.get('mode', 'random') == 'random' else 'topk',
                      sample_num=sample.get('num', 1000))
        ops.pnp_params(**kw)                    # reject bad parameters before any launch
        return kw

    def solve_pose(self, batch_flow: Optional[Tensor] = None, rendered_depths: Optional[Tensor] = None,
                   ref_rotations: Optional[Tensor] = None, ref_translations: Optional[Tensor] = None,
                   internel_k: Optional[Tensor] = None, labels: Optional[Tensor] = None,
                   per_img_patch_num=None, occlusion: Optional[Tensor] = None) -> Dict:
        """base_flow_refiner.py:99-154 -> dict(rotations, translations, scores, labels), each a per-image list with
        the samples whose solve failed dropped.  One launch sequence for the whole batch and ONE device-to-host
        transfer (the ok flags); no per-sample synchronisation.  Without an occlusion map, top-k sampling sees a
        confidence of 1 everywhere (the reference has no confidence there) and keeps the first points."""
        kw = self._pnp_kwargs()
        args = (batch_flow, rendered_depths, ref_rotations, ref_translations, internel_k, labels, per_img_patch_num)
        if any(a is None for a in args):
            raise TypeError('solve_pose needs batch_flow, rendered_depths, ref_rotations, ref_translations, '
                            'internel_k, labels and per_img_patch_num')
        occ = None if occlusion is None else occlusion.contiguous()
        rot, trans, ok, _ = ops.pnp(batch_flow.contiguous(), rendered_depths.contiguous(), internel_k.contiguous(),
                                    ref_rotations.contiguous(), ref_translations.contiguous(), occ,
                                    self.test_cfg.get('occ_thresh', 0.5), **kw)
        per = [int(v) for v in per_img_patch_num]
        keep = ok.cpu().bool()                  # the one device -> host transfer
        idx = torch.nonzero(keep).flatten()
        kept = [int(k.sum()) for k in torch.split(keep, per)]
        idx_dev = idx.to(rot.device, non_blocking=True)
        scores = torch.ones_like(labels, dtype=torch.float32)
        return {name: list(torch.split(t.index_select(0, idx_dev), kept))
                for name, t in (('rotations', rot), ('translations', trans), ('scores', scores), ('labels', labels))}

    @staticmethod
    def _remap_pose(rotations, translations, img_metas):
        """remap_pose_to_origin_resoluaion (models/utils/pose.py:264-310) for the 'adapt_intrinsic' pipeline: the
        identity.  The other modes re-solve with cv2 EPnP in the reference: not implemented."""
        for meta in img_metas or []:
            mode = meta.get('geometry_transform_mode') if isinstance(meta, dict) else None
            if mode != 'adapt_intrinsic':
                raise NotImplementedError(f'pose remapping for geometry_transform_mode {mode!r} is not implemented '
                                          "(only 'adapt_intrinsic', the identity)")
        return rotations, translations

    def forward_single_view(self, data: Dict, data_batch: Optional[Dict] = None, return_pose: bool = True):
        """raft_refiner_flow_mask.py:135-161 / raft_refiner_flow.py:141-172: flow at the last iteration, then the
        pose step.  return_pose=False returns (flow, occlusion, data) for the mask refiner, (flow, data) otherwise."""
        iters = self.decoder.iters
        self.decoder.iters = self.test_iter_num
        try:
            out = self.get_flow(data['rendered_images'], data['real_images'])
        finally:
            self.decoder.iters = iters
        if self._has_occlusion:
            batch_flow, batch_occ = out[0][-1], out[1][-1].squeeze(1)
        else:
            batch_flow, batch_occ = out[-1], None
        if not return_pose:
            return (batch_flow, batch_occ, data) if self._has_occlusion else (batch_flow, data)
        results = self.solve_pose(batch_flow, data['rendered_depths'], data['ref_rotations'],
                                  data['ref_translations'], data['internel_k'], data['labels'],
                                  data['per_img_patch_num'], batch_occ)
        img_metas = (data_batch or {}).get('img_metas') if isinstance(data_batch, dict) else None
        results['rotations'], results['translations'] = self._remap_pose(results['rotations'],
                                                                         results['translations'], img_metas)
        return results

    def forward(self, data, data_batch=None, return_loss=False):
        if return_loss:
            raise NotImplementedError('training is outside the hot path (SURVEY.md section 2)')
        return self.forward_single_view(data, data_batch)


@REFINERS.register_module()
class RAFTRefinerFlowMask(_FlowRefinerBase):
    """configs/refine_models/raft.py: RAFTDecoderMask -> (flows, occlusions); the pose step uses the last
    occlusion map (confidence and occ_thresh mask)."""
    _has_occlusion = True


@REFINERS.register_module()
class RAFTRefinerFlow(_FlowRefinerBase):
    """RAFTDecoder -> flows."""
