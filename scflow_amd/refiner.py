"""``SCFlowRefiner`` -- the drop-in boundary of the hot path.

Mirrors models/refiner/scflow_refiner.py:18-179 (+ base_refiner.py:17-64):
same registry name, constructor keys (``configs/refine_models/scflow.py:16-113``
applies unchanged), attribute names, ``extract_feat`` / ``get_pose`` /
``forward_single_pass`` signatures and return structure, same ``state_dict``
keys.  PnP re-mapping is outside the hot path, and
``forward_single_pass`` consumes an already formatted ``data`` dict (what
``BaseRefiner.format_data_test`` produces, base_refiner.py:79-133).  The loss
configs are kept as given and built at the first ``loss()`` call (scflow_amd/losses.py):
``loss()`` returns the forward VALUES the reference trains against, ``loss_and_grads()`` adds their gradients at
the network's outputs, the ``loss_and_*_grads()`` ladder (``_LOSS_DEPTHS``, nine depths) carries them through the decoder,
``loss_and_context_grads()`` through the context encoder, ``loss_and_network_grads()`` through the correlation build and
the feature encoders to every parameter of the network.
``train_step()`` applies those gradients with ``scflow_amd.optim.AdamW`` (the reference's ``freeze_encoder=True,
freeze_bn=True`` case, nothing else); ``train_step_network()`` takes the configuration as given, the shipped
``freeze_encoder=False, freeze_bn=False`` with BatchNorm on batch statistics (``batch_norm_training()``) included;
``forward(return_loss=True)`` keeps raising.  The config's ``renderer`` dict is ignored too;
``attach_renderer(MeshRenderer(...))`` enables ``format_data_test``, ``update_data``
and ``test_cfg['cycles'] > 1`` on the HIP renderer (scflow_amd/mesh.py).
"""
from __future__ import annotations

import contextlib
from collections import OrderedDict
from typing import Dict, Optional, Tuple, Union

import torch

from . import ops
from .modules import _GRAD_DEPTHS, _LOSS_DEPTHS, KEEP_LEVELS, HipModule, encoder_pair_supported, raft_encoder_pair  # noqa: F401
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

    # ------------------------------------------------------------------ supervised loss values and output gradients
    render_augmentations = None
    _loss_cfgs: Dict[str, Optional[dict]] = {}

    def _build_loss_funcs(self) -> None:
        """build ``<name>_loss_func`` from the stored config dicts, once, at the first ``loss()`` call -- the constructor
        accepts opaque dicts and mesh paths that do not exist where the model is built."""
        if self.__dict__.get('_loss_built'):
            return
        from .losses import build_loss
        built = {}
        for attr, (key, cfg) in self._loss_cfgs.items():
            if not isinstance(cfg, dict) or 'type' not in cfg:
                raise ValueError(f"loss(): {key} is {cfg!r}; it must be a loss config such as dict(type='SequenceLoss', "
                                 "gamma=0.8, loss_func_cfg=dict(type='RAFTLoss', ...))")
            if cfg['type'] == 'SequenceLoss' and 'loss_func_cfg' not in cfg:
                raise ValueError(f"loss(): {key} = {cfg!r} has no 'loss_func_cfg': the model was built from an opaque "
                                 'loss config (scflow_amd.config keeps them opaque); give the full dict, e.g. '
                                 'scflow_amd.config.scflow_loss_cfgs()')
            built[attr] = build_loss(cfg)
        for attr, func in built.items():
            self.__dict__[attr] = func
        self.__dict__['_loss_built'] = True

    def format_data_train_sup(self, data_batch: Dict) -> Dict:
        """base_refiner.py:136-191 on the attached ``MeshRenderer``: concatenate the per-image lists, render every sample
        at its reference pose, normalise the rendered RGB.  The ``init_*_error`` statistics (``torch.std_mean``,
        biased) are computed when the annotations carry them.  ``render_augmentations`` (kornia) are not implemented."""
        if self.render_augmentations is not None:
            raise NotImplementedError('render_augmentations (kornia augmentation of the rendered images, '
                                      'base_refiner.py:43-64, 159-160) are not implemented')
        self._need_renderer('format_data_train_sup')
        real_images, annots, meta_infos = data_batch['img'], data_batch['annots'], data_batch['img_metas']
        real_images = torch.cat(real_images)
        ref_rotations = torch.cat(annots['ref_rotations'], dim=0)
        ref_translations = torch.cat(annots['ref_translations'], dim=0)
        gt_rotations = torch.cat(annots['gt_rotations'], dim=0)
        gt_translations = torch.cat(annots['gt_translations'], dim=0)
        labels, internel_k = torch.cat(annots['labels']), torch.cat(annots['k'])
        norm = meta_infos[0]['img_norm_cfg']
        mean = (torch.tensor(norm['mean'], dtype=torch.float32) / 255.).tolist()
        std = (torch.tensor(norm['std'], dtype=torch.float32) / 255.).tolist()
        rgb, depth, mask = self.renderer.render_normalized(ref_rotations, ref_translations, internel_k, labels, mean, std)
        output = dict(ref_rotations=ref_rotations, ref_translations=ref_translations, gt_rotations=gt_rotations,
                      gt_translations=gt_translations, labels=labels, internel_k=internel_k, rendered_images=rgb,
                      real_images=real_images, rendered_masks=mask, rendered_depths=depth)
        for name in ('add', 'rot', 'trans'):
            if f'init_{name}_error' in annots:
                err = annots[f'init_{name}_error']
                err = torch.cat([e.reshape(-1) for e in err]) if isinstance(err, (list, tuple)) else err
                sd, mn = torch.std_mean(err, unbiased=False)
                output[f'init_{name}_error_mean'], output[f'init_{name}_error_std'] = mn, sd
        if 'gt_masks' in annots:
            output['gt_masks'] = torch.cat([_as_mask_tensor(m, real_images.device) for m in annots['gt_masks']], dim=0)
        return output

    @staticmethod
    def _scale_factors(data: Dict, data_batch: Optional[Dict], device) -> Optional[Tensor]:
        """scflow_refiner.py:213-216: the per-sample image scale (first column of every ``img_meta['scale_factor']``), or
        ``data['scale_factors']`` when the caller formatted the data itself."""
        if 'scale_factors' in data:
            return data['scale_factors']
        metas = (data_batch or {}).get('img_metas') if isinstance(data_batch, dict) else None
        if not metas or any('scale_factor' not in m for m in metas):
            return None
        first_column = []
        for meta in metas:                      # one row of (w, h, w, h) scales per sample of the image
            first_column += [float(row[0]) for row in torch.as_tensor(meta['scale_factor']).reshape(-1, 4)]
        return torch.tensor(first_column, dtype=torch.float32, device=device)

    def _supervision(self, data: Dict, by_mask: bool):
        """the ground-truth flow the losses are taken against: re-projection of the rendered depth from the reference to
        the ground-truth pose, ``max_flow`` where there is none, optionally filtered by the ground-truth mask."""
        from .metrics import filter_flow_by_mask, get_flow_from_delta_pose_and_depth
        gt_flow = get_flow_from_delta_pose_and_depth(data['ref_rotations'], data['ref_translations'],
                                                     data['gt_rotations'], data['gt_translations'],
                                                     data['rendered_depths'], data['internel_k'],
                                                     invalid_num=self.max_flow)
        if by_mask:
            gt_flow = filter_flow_by_mask(gt_flow, data['gt_masks'], invalid_num=self.max_flow)
        return gt_flow

    def _pixel_losses(self, gt_flow, valid, flow_funcs, flow_seqs, mask_func, mask_seq, grads=False):
        """SequenceLoss values of up to two flow sequences and the mask sequence.  One fused launch when every loss is a
        ``SequenceLoss`` over ``RAFTLoss`` / ``L1Loss`` with the refiner's ``max_flow``; else one call per loss with the
        occlusion target built as the reference builds it (the SUM of the two channels < max_flow,
        scflow_refiner.py:230 -- not the magnitude).  ``grads``: every (total, [value_i]) becomes (total, [value_i],
        [gradient_i]) -- the fused value-and-gradient launch under the same condition, ``value_and_grad`` per loss else."""
        from . import losses as L
        fusable = all(type(f) is L.SequenceLoss and type(f.loss_func) is L.RAFTLoss
                      and float(f.loss_func.max_flow) == float(self.max_flow) for f in flow_funcs)
        fusable = fusable and (mask_func is None or (type(mask_func) is L.SequenceLoss and type(mask_func.loss_func) is L.L1Loss))
        if fusable:
            fl = list(flow_funcs) + [None] * (2 - len(flow_funcs))
            sq = list(flow_seqs) + [None] * (2 - len(flow_seqs))
            get = lambda f, name, default: default if f is None else getattr(f.loss_func, name)
            kw = dict(flow_a=sq[0], flow_b=sq[1], masks=mask_seq, max_flow=self.max_flow,
                      loss_weight=(get(fl[0], 'loss_weight', 1.), get(fl[1], 'loss_weight', 1.), get(mask_func, 'loss_weight', 1.)),
                      eps=(get(fl[0], 'eps', 0.), get(fl[1], 'eps', 0.), 0.),
                      gamma=tuple(1. if f is None else f.gamma for f in (fl[0], fl[1], mask_func)))
            if grads:
                per_iter, totals, g = L.seq_pixel_loss_grad(gt_flow, valid, **kw)
            else:
                (per_iter, totals), g = L.seq_pixel_loss(gt_flow, valid, **kw), None
            row = lambda i: (totals[i], list(per_iter[i].unbind(0))) + ((g[i],) if grads else ())
            return [row(i) for i in range(len(flow_funcs))], (None if mask_func is None else row(2))
        call = (lambda f, *a, **k: f.value_and_grad(*a, **k)) if grads else (lambda f, *a, **k: f(*a, **k))
        out = [call(f, seq, gt_flow=gt_flow, valid=valid) for f, seq in zip(flow_funcs, flow_seqs)]
        mask_out = None
        if mask_func is not None:
            occluded_target = (gt_flow[:, 0] + gt_flow[:, 1] < self.max_flow).float()       # channel SUM, not magnitude
            mask_out = call(mask_func, [m[:, 0] if m.dim() == 4 else m for m in mask_seq], gt_mask=occluded_target, valid=valid)
            if grads:                           # the gradients take the shape of the predictions they belong to
                mask_out = mask_out[:2] + ([g.view(m.shape) for g, m in zip(mask_out[2][0], mask_seq)],)
        if grads:
            out = [o[:2] + (o[2][0],) for o in out]
        return out, mask_out

    @staticmethod
    def _log_vars(named) -> 'OrderedDict':
        """[(key, 0-dim GPU tensor)] -> OrderedDict of Python floats through ONE device-to-host transfer of one packed
        vector (the reference issues one ``.item()`` per entry)."""
        from .losses import to_host
        host = to_host(torch.stack([v.reshape(()).to(torch.float32) for _, v in named]))
        return OrderedDict((k, float(x)) for (k, _), x in zip(named, host))


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
        self.render_augmentations = render_augmentations
        # what train_step() may leave untouched: it trains only with BOTH set (the feature encoders and the correlation
        # build have no backward, BatchNorm runs on its running statistics); nothing else reads them
        self.freeze_encoder, self.freeze_bn = bool(freeze_encoder), bool(freeze_bn)
        # built at the first loss() call (_build_loss_funcs): attribute -> (constructor key, config as given)
        self._loss_cfgs = dict(pose_loss_func=('pose_loss_cfg', pose_loss_cfg), flow_loss_func=('flow_loss_cfg', flow_loss_cfg),
                               mask_loss_func=('mask_loss_cfg', mask_loss_cfg))
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
        # an encoder that keeps its activations for backward() / in_backward() runs its own forward, on this stream: the
        # paired walk below keeps nothing (same kernels per layer, same bits), and what it keeps is read on this stream
        # afterwards
        # afterwards; so does a context encoder on batch statistics (the paired walk assumes the folded form)
        keeping = self.context.keep or self.render_encoder.keep or self.real_encoder.keep or self.context.batch
        ov_ctx = small_work(n, H, W, 'context') and not keeping
        fork = ops.fork_point() if ov_ctx else None     # the context encoder may start from here
        if (not self.seperate_encoder and not keeping and ops.branch_mode(n, H, W, 'context') == 2
                and ops._CONV_EVENTS is None and encoder_pair_supported(self.render_encoder, self.context)):
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
        return self._pose_and_feats(render_images, real_images, ref_rotation, ref_translation, depth, internel_k, label,
                                    init_flow)[0]

    def _pose_and_feats(self, render_images: Tensor, real_images: Tensor, ref_rotation: Tensor, ref_translation: Tensor,
                        depth: Tensor, internel_k: Tensor, label: Tensor, init_flow: Optional[Tensor] = None):
        """``get_pose`` -> (its 7-tuple, (feat_render, feat_real)): the two feature maps of this forward for the
        ``'network'`` depth of ``_loss``.  The decoder only reads them (``corr_block``), so references are enough."""
        feat_render, feat_real, h_feat, cxt_feat = self.extract_feat(render_images, real_images)
        if init_flow is None:
            n, _, H, W = real_images.shape
            init_flow = ops.constant((n, 2, H, W), 0.0, feat_render.device)      # read-only, filled once
        outs = self.decoder(feat_render, feat_real, h_feat, cxt_feat, ref_rotation,
                            ref_translation, depth.contiguous(), internel_k.contiguous(),
                            label=label, init_flow=init_flow, invalid_flow_num=0.,
                            _consume_state=True)      # h / cxt are ours: update them in place
        return outs, (feat_render, feat_real)

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

    # ------------------------------------------------------------------ loss values
    def loss(self, data_batch: Optional[Dict], data: Optional[Dict] = None):
        """scflow_refiner.py:184-258 -> (loss, None, log_vars, seq_rotations, seq_translations): the forward VALUES of the
        pose, flow and mask sequence losses of ``decoder.iters`` iterations and their sum.  **No autograd**: ``loss`` is a
        0-dim GPU tensor with no graph behind it.  ``log_imgs`` is None (visualisation is out of scope).  ``log_vars``
        has the reference's keys in the reference's order (the ``init_add_*`` pair only when the data carries it) and
        reaches the host in one transfer.  ``data``: an already formatted dict (``format_data_train_sup``'s), the only
        way to call this without an attached renderer; it needs ``gt_masks`` when ``filter_invalid_flow`` is set."""
        return self._loss(data_batch, data, 'none')

    # loss_and_*_grads(): one method per rung of _LOSS_DEPTHS (modules.py, where what has no backward yet is stated once).
    # Every one returns (loss, None, log_vars, seq_rotations, seq_translations, grads); the values are the bits of loss(),
    # log_vars still costs one transfer, and from 'head' on every entry the rung before returns keeps its key and its bits.
    def loss_and_grads(self, data_batch: Optional[Dict], data: Optional[Dict] = None):
        """``loss()`` plus the training signal at the network's outputs: ``grads`` maps ``sequence_flow_from_pred``,
        ``sequence_masks`` and either ``seq_rotations`` / ``seq_translations`` or, when the pose loss is a ``RAFTLoss``,
        ``sequence_flow_from_pose`` to the list of d loss / d prediction per iteration (``loss = loss_pose + loss_flow +
        loss_mask``), from the value-and-gradient launches."""
        return self._loss(data_batch, data, 'outputs')

    def loss_and_head_grads(self, data_batch: Optional[Dict], data: Optional[Dict] = None):
        """``loss_and_grads()`` carried through the parameter-free tail of every iteration (``SCFlowDecoder.tail_backward``):
        ``grads`` maps ``delta_flow_preds``, ``masks`` (the post-sigmoid map), ``delta_rotation_preds`` and
        ``delta_translation_preds`` to the list of d loss / d head output per iteration.  These REPLACE the keys of
        ``loss_and_grads()``; every later rung adds to them."""
        return self._loss(data_batch, data, 'head')

    def loss_and_pose_tail_grads(self, data_batch: Optional[Dict], data: Optional[Dict] = None):
        """Adds the fully connected tail of the pose head (``MultiClassPoseHead.tail_backward``): ``pose_tail_inputs``, the
        list of d loss / d (raw output of the pose head's last convolution) per iteration, and ``params``, the gradients of
        that tail's parameters (``decoder.pose_pred.conv_layers.2.gn``, ``.fc_layers``, ``.rotation_pred``,
        ``.translation_pred``; keys as in ``named_parameters()``) summed over the iterations.  The top-level
        ``delta_flow_preds`` / ``masks`` are the tail's partial cotangents at every rung: the complete ones are in
        ``decoder_heads``."""
        return self._loss(data_batch, data, 'pose_tail')

    def loss_and_pose_head_grads(self, data_batch: Optional[Dict], data: Optional[Dict] = None):
        """Adds the pose head's three convolutions and GroupNorms 0 and 1 (``MultiClassPoseHead.conv_backward``):
        ``pose_head_inputs`` = (``g_hvs``, ``g_dms``), the lists of d loss / d (GRU hidden state ``hv`` (N, 128, h, w)) and
        d loss / d (delta-flow and mask features ``dm`` (N, 96, h, w)) per iteration; ``params`` now holds the gradient of
        EVERY parameter of ``decoder.pose_pred``."""
        return self._loss(data_batch, data, 'pose_head')

    def loss_and_decoder_head_grads(self, data_batch: Optional[Dict], data: Optional[Dict] = None):
        """Adds the two XHeads and the delta-flow / mask encoders (``SCFlowDecoder.heads_backward``): ``decoder_heads`` =
        ``dict(hidden_states, delta_flow_preds, mask_logits)``, a list per key over the iterations.  ``hidden_states[t]`` is
        d loss / d ``hv_t`` (N, 128, h, w) through iteration t's OWN heads, encoders and pose head: the cotangent the GRU
        backward adds the next iteration's to.  ``delta_flow_preds[t]`` is the complete d loss / d ``d_flow_t`` (the
        tail's plus the delta-flow encoder's), ``mask_logits[t]`` the complete d loss / d (pre-sigmoid mask) of iteration t,
        both up to the path into iteration t + 1 that no rung carries.  ``params`` is extended by the 16 weights and biases
        of ``decoder.flow_pred``, ``decoder.mask_pred``, ``decoder.delta_flow_encoder`` and ``decoder.mask_encoder``: every
        parameter downstream of the GRU state now has a gradient."""
        return self._loss(data_batch, data, 'decoder_heads')

    def loss_and_gru_grads(self, data_batch: Optional[Dict], data: Optional[Dict] = None):
        """Adds the GRU, a reverse scan over the iterations (``SCFlowDecoder.gru_backward``): ``gru`` =
        ``dict(initial_hidden, context, motion_features)``: d loss / d ``h0`` (N, 128, h, w), the hidden state the context
        encoder hands the decoder; d loss / d ``c`` (N, 128, h, w), its context features, summed over iterations and
        passes; and the list over the iterations of d loss / d ``x_t`` (N, 128, h, w), the motion encoder's 126 channels
        and the 2 flow channels behind them.  ``params`` is extended by the ``decoder.gru.*`` gradients (12 for
        ``'SeqConv'``, 6 for ``'Conv'``)."""
        return self._loss(data_batch, data, 'gru')

    def loss_and_motion_grads(self, data_batch: Optional[Dict], data: Optional[Dict] = None):
        """Adds the motion encoder and the correlation lookup with respect to the pyramid
        (``SCFlowDecoder.motion_backward``): ``motion`` = ``dict(correlation, flow_inputs)``: d loss / d (level 0 of the
        correlation pyramid) (N h w, h, w), summed over the iterations with the pooling adjoints of the coarser levels
        folded in, and the list over the iterations of d loss / d (the encoder's flow input) (N, 2, h, w).  ``params`` is
        extended by the ten ``decoder.encoder.*`` gradients: every parameter of the decoder now has a gradient.

        Only where nothing flows from ``x_t`` back into iteration t - 1: ``detach_flow=True``, and ``detach_mask=True``
        whenever ``mask_flow`` or ``mask_corr`` is set (the shipped configuration).  Otherwise the cotangent re-enters the
        previous iteration through ``flow_lr`` (which needs the lookup's derivative with respect to its coordinates) or
        through the mask, a reverse scan over whole iterations: NotImplementedError (``SCFlowDecoder.check_backward``)."""
        return self._loss(data_batch, data, 'motion')

    def loss_and_context_grads(self, data_batch: Optional[Dict], data: Optional[Dict] = None):
        """``loss_and_motion_grads()`` (its keys, values and bits, and its refusals) with the context encoder behind it
        (``RAFTEncoder.backward`` from ``gru['initial_hidden']`` and ``gru['context']``, complete only at that rung):
        ``params`` is extended by the 62 ``context.*`` gradients, BatchNorm with running statistics as the forward
        computes it (the reference's ``freeze_bn=True``).  Every parameter of the network except the feature encoder's
        now has a gradient: the reference's ``freeze_encoder=True`` training case.  The context encoder keeps its
        activations during this forward (``RAFTEncoder.keeping``) and drops them before returning."""
        return self._loss(data_batch, data, 'context')

    def loss_and_network_grads(self, data_batch: Optional[Dict], data: Optional[Dict] = None):
        """``loss_and_context_grads()`` (its keys, values and bits, and its refusals) with the correlation build and the
        feature encoder(s) behind it: ``SCFlowDecoder.corr_backward`` turns ``motion['correlation']`` and the two feature
        maps of this same forward into ``features`` = ``dict(render, real)``, d loss / d ``extract_feat``'s (render_feat,
        real_feat) (N, C, h, w); ``RAFTEncoder.in_backward`` carries them on.  ``params`` is extended by the 32
        ``render_encoder.*`` gradients -- with the shared encoder ONE pass over the (2N, ...) buffer the two cotangents
        are the halves of, render first, so each is the sum over both image sets -- and with ``seperate_encoder=True`` by
        32 + 32 (``render_encoder.*``, ``real_encoder.*``): ``params`` then covers all of ``named_parameters()``, and
        ``scflow_amd.optim.AdamW(list(model.named_parameters()))`` steps the whole network from it.  The encoders keep
        their activations during this forward and everything kept is dropped before returning, also on an error."""
        return self._loss(data_batch, data, 'network')

    def feature_grads(self, g_render_feat: Tensor, g_real_feat: Tensor, param_grads: Optional[dict] = None) -> dict:
        """The feature encoders' parameter gradients from the cotangents at ``extract_feat``'s (render_feat, real_feat),
        after a forward inside ``render_encoder.keeping()`` (and ``real_encoder.keeping()`` with
        ``seperate_encoder=True``): ``RAFTEncoder.in_backward``.  The shared encoder: ONE pass over the 2N stacked
        cotangents, render first as the forward stacks the images, so every gradient is the sum over both image sets;
        keys as ``named_parameters()`` has them (``render_encoder.*``, the shared module's first name).  Separate
        encoders: two passes, ``render_encoder.*`` and ``real_encoder.*``.  ``param_grads`` as in ``in_backward``.  What
        the encoders kept is dropped before returning, also on an error.

        ``loss_and_network_grads()`` is the rung that reaches this chain (it hands ``in_backward`` the correlation-build
        backward's (2N, ...) buffer directly); ``trainable_parameters()`` and ``train_step`` still stop at the
        correlation volume."""
        what = 'SCFlowRefiner.feature_grads'
        fe, re_ = self.render_encoder, self.real_encoder
        try:
            for name, g in (('g_render_feat', g_render_feat), ('g_real_feat', g_real_feat)):
                ops._dev(g, f'{what}: {name}')
            if g_render_feat.shape != g_real_feat.shape or g_render_feat.dim() != 4:
                raise ops._lib.ScflowHipError(f'{what}: the two cotangents are (N, C, h, w) tensors of one shape, got '
                                              f'{tuple(g_render_feat.shape)} and {tuple(g_real_feat.shape)}')
            return self._feature_backward(g_render_feat, g_real_feat, param_grads=param_grads)
        finally:
            fe.kept, re_.kept = {}, {}

    def _feature_backward(self, g_render: Tensor, g_real: Tensor, stacked: Optional[Tensor] = None,
                          param_grads: Optional[dict] = None) -> dict:
        """``RAFTEncoder.in_backward`` on what the feature encoder(s) kept.  Shared encoder: one pass under
        ``render_encoder.`` over ``stacked``, the (2N, ...) buffer the two cotangents are the halves of (None: a copy that
        stacks them).  Separate encoders: two passes, the second accumulating into the first's dict under ``real_encoder.``"""
        fe, re_ = self.render_encoder, self.real_encoder
        if not self.seperate_encoder:
            return fe.in_backward(fe.kept, torch.cat((g_render, g_real)) if stacked is None else stacked,
                                  param_grads=param_grads, prefix='render_encoder.')
        grads = fe.in_backward(fe.kept, g_render.contiguous(), param_grads=param_grads, prefix='render_encoder.')
        return re_.in_backward(re_.kept, g_real.contiguous(), param_grads=grads, prefix='real_encoder.')

    # ------------------------------------------------------------------ training
    def trainable_parameters(self):
        """the (name, parameter) pairs ``train_step`` updates: every parameter of ``decoder.*`` and ``context.*`` in
        ``named_parameters()`` order -- the ones ``loss_and_context_grads()`` has a gradient for.  Never the feature
        encoders (``loss_and_network_grads()`` has their gradients; ``train_step`` does not take that rung yet) and never a
        buffer (BatchNorm's running statistics stay as loaded)."""
        return [(n, p) for n, p in self.named_parameters() if n.startswith(('decoder.', 'context.'))]

    def train_step(self, data_batch: Optional[Dict], optimizer, data: Optional[Dict] = None) -> Dict:
        """base_refiner.py:325-336 -> ``dict(loss, log_vars, log_imgs=None, num_samples)``, with ONE deviation: there is no
        autograd graph behind ``loss``, so the optimizer step happens HERE (``loss_and_context_grads()``, then
        ``optimizer.step(grads['params'])``) -- a runner must not add an optimizer hook on top.  ``optimizer``: a
        ``scflow_amd.optim.AdamW`` over ``trainable_parameters()`` (``build_optimizer``).  ``log_vars`` gains ``grad_norm``
        (when the optimizer clips) and ``lr``, still through one device-to-host transfer.  After it returns the next
        forward runs on the new weights; a hipGraph captured before (``GraphedRefiner``) holds the old ones and must be
        captured again.

        ``train_cfg['cycles'] > 1`` follows ``train_multiple_iterations`` (base_refiner.py:220-247): loss, step,
        ``update_data`` at the last pose of the cycle, next cycle, on the attached renderer; ``log_vars`` is the mean over
        the cycles plus ``iter_{i}_loss`` of every cycle but the last.  The last cycle steps here too (the reference leaves
        that one to the runner's hook), and every cycle of one call uses the same learning rate.

        Trains what has a backward: NotImplementedError unless ``freeze_encoder and freeze_bn``, and everything
        ``loss_and_motion_grads()`` refuses.  ``data``: an already formatted dict (it is not modified).
        ``train_step_network()`` is this step for the other settings of the two flags, the reference's shipped
        ``freeze_encoder=False, freeze_bn=False`` among them."""
        from .optim import AdamW
        if not isinstance(optimizer, AdamW):
            raise TypeError(f'train_step needs a scflow_amd.optim.AdamW (build_optimizer), got {type(optimizer).__name__}: there '
                            'is no autograd graph behind the loss and no .grad for another optimizer to read')
        missing = []
        if not self.freeze_encoder:
            missing.append('freeze_encoder=False needs the feature-encoder and correlation-build backward')
        if not self.freeze_bn:
            missing.append('freeze_bn=False needs BatchNorm on batch statistics, forward and backward')
        if missing:
            raise NotImplementedError('train_step trains the decoder and the context encoder only (freeze_encoder=True, '
                                      'freeze_bn=True): ' + '; '.join(missing) + ', which are not implemented')
        mine = self.trainable_parameters()
        if len(mine) != len(optimizer.params) or any(a is not b for (_, a), b in zip(mine, optimizer.params)):
            raise ValueError('train_step: the optimizer was not built over this model\'s trainable_parameters()')
        return self._train_cycles(data_batch, optimizer, data, 'context', 'motion')

    @contextlib.contextmanager
    def batch_norm_training(self):
        """inside the body the context encoder runs on the statistics of the batch (``RAFTEncoder.batch_stats``): every
        ``loss*()`` rung normalises with them and moves the 15 layers' running statistics, and the rungs ``'context'`` and
        ``'network'`` take ``RAFTEncoder.bn_backward``.  The reference's ``freeze_bn=False``; off by default."""
        with self.context.batch_stats():
            yield self

    def network_parameters(self):
        """the (name, parameter) pairs of the reference's training recipe, which ``train_step_network`` updates: all of
        ``named_parameters()``, less the feature encoder(s) when ``freeze_encoder``"""
        frozen = ('render_encoder.', 'real_encoder.') if self.freeze_encoder else ()
        return [(n, p) for n, p in self.named_parameters() if not n.startswith(frozen)]

    def train_step_network(self, data_batch: Optional[Dict], optimizer, data: Optional[Dict] = None) -> Dict:
        """``train_step``'s contract (return value, ``cycles``, one device-to-host transfer, the packs invalidated after
        every step) for the model's configuration as given: the rung ``loss_and_network_grads()``, or
        ``loss_and_context_grads()`` when ``freeze_encoder``, taken inside ``batch_norm_training()`` unless ``freeze_bn``.
        With ``freeze_encoder=False, freeze_bn=False``, what the reference ships, every parameter and all BatchNorm
        running statistics move.  ``optimizer``: ``build_optimizer(..., network=True)``, an ``AdamW`` over
        ``network_parameters()``.  Refuses what ``SCFlowDecoder.check_backward('network')`` refuses, nothing else."""
        from .optim import AdamW
        if not isinstance(optimizer, AdamW):
            raise TypeError(f'train_step_network needs a scflow_amd.optim.AdamW (build_optimizer), got '
                            f'{type(optimizer).__name__}: there is no autograd graph behind the loss and no .grad for another '
                            'optimizer to read')
        mine = self.network_parameters()
        if len(mine) != len(optimizer.params) or any(a is not b for (_, a), b in zip(mine, optimizer.params)):
            raise ValueError('train_step_network: the optimizer was not built over this model\'s network_parameters() '
                             '(build_optimizer(..., network=True))')
        with contextlib.nullcontext() if self.freeze_bn else self.batch_norm_training():
            return self._train_cycles(data_batch, optimizer, data, 'context' if self.freeze_encoder else 'network',
                                      'network')

    def _train_cycles(self, data_batch, optimizer, data, depth: str, refuse: str) -> Dict:
        """the cycles of one training iteration behind ``train_step`` and ``train_step_network``: loss and gradients at
        the rung ``depth``, step, ``update_data``; ``refuse``: the depth whose refusals come before anything is rendered"""
        cycles = int(self.train_cfg.get('cycles', 1))
        if cycles > 1:
            self._need_renderer("train_cfg['cycles'] > 1")
        self.decoder.check_backward(refuse)             # refuse before anything is rendered or stepped
        if data is None:
            data = self.format_data_train_sup(data_batch)
        data = dict(data)
        num_samples = len(data_batch['img_metas']) if isinstance(data_batch, dict) and 'img_metas' in data_batch \
            else len(data['real_images'])
        named = []
        for i in range(cycles):
            loss, _, log, seq_r, seq_t, grads = self._loss(data_batch, data, depth, host_log=False)
            norm = optimizer.step(grads['params'], end_of_iteration=i == cycles - 1)
            if optimizer.model is not self:
                self.invalidate_packed()
            if norm is not None:
                log = log + [('grad_norm', norm)]
            named.append(log)
            if i < cycles - 1:
                data = self.update_data(seq_r[-1], seq_t[-1], data)
        keys = [k for k, _ in named[0]]
        flat = self._log_vars([(f'{i}.{k}', v) for i, log in enumerate(named) for k, v in log])
        log_vars = OrderedDict((k, sum(flat[f'{i}.{k}'] for i in range(cycles)) / cycles) for k in keys)
        for i in range(cycles - 1):
            log_vars[f'iter_{i}_loss'] = flat[f'{i}.loss']
        log_vars['lr'] = optimizer.lr
        return dict(loss=loss, log_vars=log_vars, log_imgs=None, num_samples=num_samples)

    def _loss(self, data_batch, data, depth, host_log=True):
        """The ladder, to the rung ``depth`` of ``_LOSS_DEPTHS``: the only place that knows its order.  ``host_log=False``
        (train_step): ``log_vars`` stays the list of (key, 0-dim GPU tensor) it is made from, so that the caller can add
        its own entries and still make ONE device-to-host transfer (``_log_vars``)."""
        from . import losses as L
        at = _LOSS_DEPTHS.index
        level = at(depth)
        with_grads = level >= at('outputs')
        dec, ctx = self.decoder, self.context
        dec_depth = _LOSS_DEPTHS[min(level, at('motion'))]           # the decoder's part of the ladder ends there
        dec.check_backward(depth)
        self._build_loss_funcs()
        if data is None:
            data = self.format_data_train_sup(data_batch)
        labels, valid = data['labels'], data['rendered_masks']
        # the encoders behind the decoder keep their activations during the forward, each under its own switch
        keepers = [ctx] if level >= at('context') else []
        if level >= at('network'):
            keepers += [self.render_encoder, self.real_encoder] if self.seperate_encoder else [self.render_encoder]
        try:
            with contextlib.ExitStack() as stack:
                for enc in keepers:
                    stack.enter_context(enc.keeping())
                stack.enter_context(dec.keeping(dec_depth if dec_depth in KEEP_LEVELS else 'none'))
                pose_args = (data['rendered_images'], data['real_images'], data['ref_rotations'], data['ref_translations'],
                             data['rendered_depths'], data['internel_k'], labels)
                if level >= at('network'):          # the correlation-build backward reads this forward's two feature maps
                    outs, (feat_render, feat_real) = self._pose_and_feats(*pose_args)
                else:
                    outs = self.get_pose(*pose_args)
            flow_from_pose, flow_from_pred, seq_rotations, seq_translations, sequence_masks = outs[:5]
            gt_flow = self._supervision(data, self.filter_invalid_flow)
            pose_is_flow = isinstance(getattr(self.pose_loss_func, 'loss_func', None), L.RAFTLoss)
            if pose_is_flow:
                (flow_out, pose_out), mask_out = self._pixel_losses(
                    gt_flow, valid, [self.flow_loss_func, self.pose_loss_func], [flow_from_pred, flow_from_pose],
                    self.mask_loss_func, sequence_masks, with_grads)
            else:
                pose_call = self.pose_loss_func.value_and_grad if with_grads else self.pose_loss_func
                pose_out = pose_call(seq_rotations, seq_translations, gt_r=data['gt_rotations'],
                                     gt_t=data['gt_translations'], labels=labels,
                                     scale_factors=self._scale_factors(data, data_batch, gt_flow.device))
                (flow_out,), mask_out = self._pixel_losses(gt_flow, valid, [self.flow_loss_func], [flow_from_pred],
                                                           self.mask_loss_func, sequence_masks, with_grads)
            (loss_pose, seq_pose), (loss_flow, seq_flow), (loss_mask, seq_mask) = pose_out[:2], flow_out[:2], mask_out[:2]
            loss = loss_pose + loss_flow + loss_mask
            named = []
            if 'init_add_error_mean' in data:
                named += [('init_add_mean', data['init_add_error_mean']), ('init_add_std', data['init_add_error_std'])]
            for i in range(len(seq_flow)):
                named += [(f'seq_{i}_pose_loss', seq_pose[i]), (f'seq_{i}_flow_loss', seq_flow[i]),
                          (f'seq_{i}_mask_loss', seq_mask[i])]
            named += [('loss_mask', loss_mask), ('loss_flow', loss_flow), ('loss_pose', loss_pose), ('loss', loss)]
            out = (loss, None, self._log_vars(named) if host_log else named, seq_rotations, seq_translations)
            if not with_grads:
                return out
            grads = dict(sequence_flow_from_pred=flow_out[2], sequence_masks=mask_out[2])
            if pose_is_flow:
                grads['sequence_flow_from_pose'] = pose_out[2]
            else:
                grads['seq_rotations'] = pose_out[2][0]
                if len(pose_out[2]) > 1 and pose_out[2][1] is not None:
                    grads['seq_translations'] = pose_out[2][1]
            if level >= at('head'):
                grads = dec.backward(dec_depth, outs, grads, labels, data['ref_rotations'], data['ref_translations'],
                                     data['rendered_depths'].contiguous(), data['internel_k'].contiguous())
            if 'params' in grads:
                grads['params'] = {'decoder.' + key: val for key, val in grads['params'].items()}
            if level >= at('context'):
                grads['params'].update((ctx.bn_backward if ctx.batch else ctx.backward)(     # batch_norm_training()
                    ctx.kept, (grads['gru']['initial_hidden'], grads['gru']['context']), head_act=ACT_TANH,
                    head_act2=ACT_RELU, head_split=self.h_channels, prefix='context.'))
            if level >= at('network'):
                n = feat_render.shape[0]
                both = torch.empty((2 * n,) + tuple(feat_render.shape[1:]), dtype=torch.float32, device=feat_render.device)
                g_render, g_real = dec.corr_backward(feat_render, feat_real, grads['motion']['correlation'],
                                                     out=(both[:n], both[n:]))
                grads['features'] = dict(render=g_render, real=g_real)
                grads['params'].update(self._feature_backward(g_render, g_real, stacked=both))
            return out + (grads,)
        finally:
            for enc in keepers:                     # what an encoder kept is dropped before returning, also on an error
                enc.kept = {}

    def forward(self, data, data_batch=None, return_loss=False):
        if return_loss:
            raise NotImplementedError('train_step and the backward of the network are not implemented; loss_and_grads() '
                                      'returns the loss values and their gradients at the network outputs, '
                                      'loss_and_head_grads() carries them to the head outputs of every iteration, '
                                      'loss_and_pose_tail_grads() through the fully connected tail of the pose head, '
                                      'loss_and_pose_head_grads() through the pose head\'s convolutions to hv and dm, '
                                      'loss_and_decoder_head_grads() through the XHeads and the delta-flow / mask encoders to hv, '
                                      'loss_and_gru_grads() through the GRU to h0, the context and the motion features, '
                                      'loss_and_motion_grads() through the motion encoder and the lookup to the correlation volume, '
                                      'loss_and_context_grads() through the context encoder to its 62 parameters')
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
                 max_flow: float = 400., render_augmentations: Optional[list] = None,
                 filter_invalid_flow_by_mask: bool = True, filter_invalid_flow_by_depth: bool = False,
                 filter_invalid_flow: Optional[bool] = None, flow_loss_cfg: Optional[dict] = None,
                 occlusion_loss_cfg: Optional[dict] = None, loss_cfg: Optional[dict] = None, **ignored) -> None:
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
        self.max_flow = max_flow
        self.render_augmentations = render_augmentations
        self.filter_invalid_flow_by_mask = filter_invalid_flow_by_mask
        self.filter_invalid_flow_by_depth = filter_invalid_flow_by_depth
        # raft_refiner_flow.py:192 reads `filter_invalid_flow`; it follows filter_invalid_flow_by_mask unless given
        self.filter_invalid_flow = filter_invalid_flow_by_mask if filter_invalid_flow is None else filter_invalid_flow
        self._loss_cfgs = self._loss_config(flow_loss_cfg, occlusion_loss_cfg, loss_cfg)
        self.eval()

    extract_feat = SCFlowRefiner.extract_feat

    def _no_depth_filter(self):
        if self.filter_invalid_flow_by_depth:
            raise NotImplementedError('filter_invalid_flow_by_depth (filter_flow_by_depth on a rendering at the '
                                      'ground-truth pose, raft_refiner_flow_mask.py:189-191) is not implemented')

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
            raise NotImplementedError('train_step and the backward of the network are not implemented; loss_and_grads() '
                                      'returns the loss values and their gradients at the network outputs')
        return self.forward_single_view(data, data_batch)


@REFINERS.register_module()
class RAFTRefinerFlowMask(_FlowRefinerBase):
    """configs/refine_models/raft.py: RAFTDecoderMask -> (flows, occlusions); the pose step uses the last
    occlusion map (confidence and occ_thresh mask)."""
    _has_occlusion = True

    @staticmethod
    def _loss_config(flow_loss_cfg, occlusion_loss_cfg, loss_cfg):
        return dict(flow_loss_func=('flow_loss_cfg', flow_loss_cfg),
                    occlusion_loss_func=('occlusion_loss_cfg', occlusion_loss_cfg))

    def loss(self, data_batch: Optional[Dict], data: Optional[Dict] = None):
        """raft_refiner_flow_mask.py:169-222 -> (loss, None, log_vars): the forward VALUES of the flow and the occlusion
        sequence losses (keys ``seq_<i>_flow_loss``, ``seq_<i>_occ_loss``, ``loss_occ``, ``loss_flow``, ``loss``).  **No
        autograd.**  ``data``: an already formatted dict, as for ``SCFlowRefiner.loss``."""
        return self._loss(data_batch, data, False)

    def loss_and_grads(self, data_batch: Optional[Dict], data: Optional[Dict] = None):
        """``loss()`` plus d loss / d prediction per iteration -> (loss, None, log_vars, grads) with the keys
        ``sequence_flow_from_pred`` and ``sequence_masks`` (the occlusion sequence)."""
        return self._loss(data_batch, data, True)

    def _loss(self, data_batch, data, with_grads):
        self._no_depth_filter()
        self._build_loss_funcs()
        if data is None:
            data = self.format_data_train_sup(data_batch)
        sequence_flow, sequence_occlusion = self.get_flow(data['rendered_images'], data['real_images'])
        gt_flow = self._supervision(data, self.filter_invalid_flow_by_mask)
        (flow_out,), occ_out = self._pixel_losses(gt_flow, data['rendered_masks'], [self.flow_loss_func], [sequence_flow],
                                                  self.occlusion_loss_func, sequence_occlusion, with_grads)
        (loss_flow, seq_flow), (loss_occ, seq_occ) = flow_out[:2], occ_out[:2]
        loss = loss_flow + loss_occ
        named = []
        for i in range(len(seq_flow)):
            named += [(f'seq_{i}_flow_loss', seq_flow[i]), (f'seq_{i}_occ_loss', seq_occ[i])]
        named += [('loss_occ', loss_occ), ('loss_flow', loss_flow), ('loss', loss)]
        out = (loss, None, self._log_vars(named))
        return out + (dict(sequence_flow_from_pred=flow_out[2], sequence_masks=occ_out[2]),) if with_grads else out


@REFINERS.register_module()
class RAFTRefinerFlow(_FlowRefinerBase):
    """RAFTDecoder -> flows."""

    @staticmethod
    def _loss_config(flow_loss_cfg, occlusion_loss_cfg, loss_cfg):
        # raft_refiner_flow.py:40 names its one loss `loss_cfg`; `flow_loss_cfg` is taken in its place
        return dict(loss_func=('loss_cfg', loss_cfg if loss_cfg is not None else flow_loss_cfg))

    def loss(self, data_batch: Optional[Dict], data: Optional[Dict] = None):
        """raft_refiner_flow.py:177-212 -> (loss, None, log_vars): the forward VALUES of the flow sequence loss (keys
        ``seq_<i>_loss``, ``loss``).  **No autograd.**  ``data``: an already formatted dict."""
        return self._loss(data_batch, data, False)

    def loss_and_grads(self, data_batch: Optional[Dict], data: Optional[Dict] = None):
        """``loss()`` plus d loss / d prediction per iteration -> (loss, None, log_vars, grads) with the key
        ``sequence_flow_from_pred``."""
        return self._loss(data_batch, data, True)

    def _loss(self, data_batch, data, with_grads):
        self._no_depth_filter()
        self._build_loss_funcs()
        if data is None:
            data = self.format_data_train_sup(data_batch)
        sequence_flow = self.get_flow(data['rendered_images'], data['real_images'])
        gt_flow = self._supervision(data, self.filter_invalid_flow)
        (flow_out,), _ = self._pixel_losses(gt_flow, data['rendered_masks'], [self.loss_func], [sequence_flow], None, None,
                                            with_grads)
        loss, seq_loss = flow_out[:2]
        named = [(f'seq_{i}_loss', v) for i, v in enumerate(seq_loss)] + [('loss', loss)]
        out = (loss, None, self._log_vars(named))
        return out + (dict(sequence_flow_from_pred=flow_out[2]),) if with_grads else out
