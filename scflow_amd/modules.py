"""Host-side mirror of the reference's encoder / decoder / head classes.

Each class keeps the reference's constructor signature, registry name and
``state_dict`` key layout (tests/golden/state_dict_keys.json),
so the reference ``model=`` config dict and reference checkpoints apply
unchanged -- but ``forward`` only sequences hand-written gfx950 kernels through
``scflow_amd.ops`` (C ABI, include/scflow_hip.h).  The ``torch.nn`` leaf
modules below are parameter containers: their own ``forward`` is never called,
and there is no CPU fallback (ops reject non-GPU tensors).

Kernel-layout copies of the parameters (``PackedConv``) are built lazily on the
parameters' device and dropped whenever the module is moved or re-loaded.
"""
from __future__ import annotations

import contextlib
from functools import partial
from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch
import torch.nn as nn

from . import ops
from .ops import (ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH, CONV_GRU_Q, CONV_GRU_ZR, PackedConv)
from .registry import DECODERS, ENCODERS, HEAD, build_head

Tensor = torch.Tensor

_ACTS = {None: ACT_NONE, 'ReLU': ACT_RELU, 'Sigmoid': ACT_SIGMOID, 'Tanh': ACT_TANH}


def _act_code(act_cfg: Optional[dict]) -> int:
    if act_cfg is None:
        return ACT_NONE
    kind = act_cfg.get('type')
    if kind not in _ACTS:
        raise NotImplementedError(f'activation {kind} has no HIP epilogue')
    return _ACTS[kind]


def _lib_error(msg):
    from ._lib import ScflowHipError
    return ScflowHipError(msg)


# what SCFlowDecoder.keep asks a forward to leave in SCFlowDecoder.kept: a level keeps what the levels before it keep
KEEP_LEVELS = ('none', 'pose_tail', 'pose_head', 'decoder_heads', 'gru', 'motion')
_KEEP = {name: i for i, name in enumerate(KEEP_LEVELS)}
# how far SCFlowRefiner._loss carries the gradient: every depth does what the ones before it do; from 'head' on the chain is
# SCFlowDecoder.backward, from 'pose_tail' on the depth is also the keep level its stage reads.  _GRAD_DEPTHS is the
# decoder's part, seven depths that end at 'motion'; _LOSS_DEPTHS is the whole ladder, nine depths: behind 'motion',
# 'context' adds the context encoder (RAFTEncoder.backward from grads['gru']['initial_hidden'] and grads['gru']['context'],
# under its own keeping() switch) and 'network' the correlation build (SCFlowDecoder.corr_backward, from
# grads['motion']['correlation']) with the feature encoders behind it (RAFTEncoder.in_backward): one walk, two norm kinds.
# No backward yet: the path from iteration t into iteration t - 1 under detach_flow=False or under mask_flow / mask_corr
# without detach_mask (SCFlowDecoder.check_backward refuses it from 'motion' on)
_GRAD_DEPTHS = ('none', 'outputs', 'head') + KEEP_LEVELS[1:]
_LOSS_DEPTHS = _GRAD_DEPTHS + ('context', 'network')


def _kept(what: str, saved, keys: Sequence[str], level: Optional[str]) -> list:
    """the entries ``keys`` of ``saved``, or the error that names the keep level whose forward leaves them in
    ``SCFlowDecoder.kept``"""
    try:
        return [saved[k] for k in keys]
    except (KeyError, TypeError):
        where = f": SCFlowDecoder.kept after a forward at keep level '{level}' or above" if level else ''
        raise _lib_error(f"{what}: saved holds {', '.join(keys)}{where}") from None


def _stacked(seq: Sequence[Tensor], m: int, c: int, h: int, w: int) -> Tensor:
    """the T per-iteration (N, c, h, w) tensors of ``seq`` as one (m = T N, c, h, w) tensor: a copy, none for T = 1"""
    return (seq[0].contiguous() if len(seq) == 1 else torch.stack(list(seq))).view(m, c, h, w)


def _layer_wgrad(grads: dict, dst: dict, acc: bool, ws: Tensor, key: str, g: Tensor, x: Tensor, conv) -> None:
    """``conv``'s weight and bias gradient from (``g``, ``x``) into ``grads`` under ``key``.weight / .bias, written to (with
    ``acc``: added to) the ``_grad_slots`` destinations ``dst``"""
    grads[f'{key}.weight'], grads[f'{key}.bias'] = ops.conv_s1_wgrad(
        g, x, tuple(conv.kernel_size), dw=dst[f'{key}.weight'], db=dst[f'{key}.bias'], accumulate=acc, workspace=ws)


class HipModule(nn.Module):
    """nn.Module with a kernel-layout copy of its parameters (``packed``).

    The copy is keyed on the identity AND version of every tensor it was built from
    (``(data_ptr, _version)`` of ``_pack_sources()``), so it follows the ways weights normally
    change: ``.to()``, ``load_state_dict`` on this module or on any wrapper / parent (mmcv's
    ``load_checkpoint`` recurses through ``_load_from_state_dict`` and never calls this
    class's ``load_state_dict``), in-place ops on the parameter under ``torch.no_grad()``
    (``weight.mul_``, ``weight.copy_``) and ``nn.init`` -- all of them bump ``_version`` or replace
    the storage.  NOT covered: edits through ``param.data`` (``param.data.copy_(...)``,
    ``param.data.mul_(...)``): ``.data`` is a detached alias with its own version counter, so the
    parameter's ``_version`` stays put.  After such an edit call ``invalidate_packed()``."""

    def invalidate_packed(self) -> None:
        """drop every kernel-layout weight copy held by this module and its children; they are
        rebuilt from the current parameters at the next forward.  Needed only after weight edits
        the version key cannot see (``param.data.copy_`` and friends)."""
        self._drop_packed()
        for m in self.modules():
            m.__dict__.pop('_ctx_cache', None)

    def _drop_folded(self) -> None:
        """drop ``packed`` of this module and its children and leave the raw packs (``_raw_packs``): for a forward that moved
        the running statistics ``packed`` folds in, and read the raw packs itself"""
        for m in self.modules():
            if isinstance(m, HipModule):
                m.__dict__['_packed'] = None

    def _drop_packed(self) -> None:
        self._drop_folded()
        for m in self.modules():
            if isinstance(m, HipModule):
                m.__dict__.pop('_pack_refs', None)
                m.__dict__.pop('_raw_packed', None)

    def _apply(self, fn, *a, **k):
        out = super()._apply(fn, *a, **k)
        self._drop_packed()
        return out

    def load_state_dict(self, *a, **k):
        out = super().load_state_dict(*a, **k)
        self._drop_packed()
        return out

    def _pack(self):
        raise NotImplementedError

    def _pack_modules(self):
        """the modules whose own parameters / buffers ``_pack`` reads (default: this module and its
        non-HipModule descendants, e.g. nn.Conv2d / norm leaves)."""
        out, stack = [], [self]
        while stack:
            m = stack.pop()
            out.append(m)
            for c in m._modules.values():
                if c is not None and not isinstance(c, HipModule):
                    stack.append(c)
        return out

    def _pack_sources(self):
        """the tensors ``_pack`` reads."""
        return [t for m in self._pack_modules() for d in (m._parameters, m._buffers)
                for t in d.values() if t is not None]

    def _pack_key(self):
        # (registry dict, name) pairs are resolved once per module (the module TREE is fixed after
        # construction); the tensors are looked up through them on every call, so a replaced
        # Parameter object (load_state_dict(assign=True), setattr) is seen like an in-place edit
        refs = self.__dict__.get('_pack_refs')
        if refs is None:
            if type(self)._pack_sources is not HipModule._pack_sources:       # composite modules name their sources
                return tuple((t.data_ptr(), t._version) for t in self._pack_sources())
            refs = self.__dict__['_pack_refs'] = [(d, n) for m in self._pack_modules()
                                                  for d in (m._parameters, m._buffers) for n in d]
        key = []
        for d, n in refs:
            t = d.get(n)
            if t is not None:
                key.append((t.data_ptr(), t._version))
        return tuple(key)

    @property
    def packed(self):
        d = self.__dict__
        key = self._pack_key()
        if d.get('_packed') is None or d.get('_packed_key') != key:
            with torch.no_grad():
                d['_packed'] = self._pack()
            d['_packed_key'] = key
        return d['_packed']


class ConvBlock(HipModule):
    """parameter layout of mmcv ``ConvModule``: ``.conv`` (+ ``.gn``); conv -> norm -> act,
    bias iff no norm."""

    def __init__(self, cin, cout, kernel_size, stride=1, padding=0, act_cfg=dict(type='ReLU'),
                 norm_cfg: Optional[dict] = None):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, kernel_size, stride=stride, padding=padding,
                              bias=norm_cfg is None)
        self.act = _act_code(act_cfg)
        self.groups = None
        if norm_cfg is not None:
            if norm_cfg.get('type') != 'GN':
                raise NotImplementedError('ConvBlock supports GN only (pose head)')
            self.groups = norm_cfg['num_groups']
            self.gn = nn.GroupNorm(self.groups, cout, eps=norm_cfg.get('eps', 1e-5))

    def _pack(self) -> PackedConv:
        c = self.conv
        return PackedConv.from_weight(c.weight, c.bias, stride=c.stride[0], padding=c.padding)

    def forward(self, x0: Tensor, x1: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
        if self.groups is None:
            return ops.conv2d(self.packed, x0, x1, out=out, act=self.act)
        if self.act != ACT_RELU:
            raise NotImplementedError('GN is fused with ReLU only')
        # small grids: K split across blocks, the normalisation adds the partial tensors (ops.conv_kslices)
        ks = ops.conv_kslices_for(self.packed, x0, x1)
        y = ops.conv2d(self.packed, x0, x1, kslices=ks)
        return ops.group_norm_relu(y, self.gn.weight, self.gn.bias, self.groups, self.gn.eps, out=out)


# =============================================================== encoder
def _raw_packs(mod: HipModule, convs: dict) -> dict:
    """the convolutions ``convs`` (key -> nn.Conv2d) of ``mod`` packed WITHOUT the norm behind them folded in: the second
    packed set, what a forward on batch statistics launches.  Cached in ``mod`` under the identity and version of the
    convolutions' own tensors (the running statistics move at every such forward and are no part of it); dropped with
    ``packed`` by ``invalidate_packed()``."""
    key = tuple((t.data_ptr(), t._version) for c in convs.values() for t in (c.weight, c.bias))
    d = mod.__dict__
    if d.get('_raw_packed') is None or d.get('_raw_packed_key') != key:
        with torch.no_grad():
            d['_raw_packed'] = {k: PackedConv.from_weight(c.weight, c.bias, c.stride[0], c.padding) for k, c in convs.items()}
        d['_raw_packed_key'] = key
    return d['_raw_packed']


def _bn_step(bn, u: Tensor, **form):
    """``ops.batch_norm_train`` of ``u`` with the parameters of the nn.BatchNorm2d ``bn``, whose running statistics and
    batch count it moves"""
    out = ops.batch_norm_train(u, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.momentum, bn.eps, **form)
    bn.num_batches_tracked += 1
    return out


def _bn_params(norm):
    """(weight, bias, running_mean, running_var) of a BatchNorm layer: what ``PackedConv.from_weight`` folds into the
    convolution in front as ``bn=`` and ``ops.batch_norm_train`` takes as ``res_bn=``; None for an InstanceNorm layer, which
    has nothing to fold"""
    return (norm.weight, norm.bias, norm.running_mean, norm.running_var) if isinstance(norm, nn.BatchNorm2d) else None


class _BasicBlock(HipModule):
    """backbone/resnet.py:14-94 parameters: conv1, {in,bn}1, conv2, {in,bn}2, downsample."""

    def __init__(self, inplanes, planes, stride, kind, downsample: bool):
        super().__init__()
        tag = 'in' if kind == 'IN' else 'bn'
        mk = (lambda c: nn.InstanceNorm2d(c)) if kind == 'IN' else (lambda c: nn.BatchNorm2d(c))
        self.kind, self.stride, self.tag = kind, stride, tag
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride=stride, padding=1, bias=True)
        setattr(self, tag + '1', mk(planes))
        self.conv2 = nn.Conv2d(planes, planes, 3, padding=1, bias=True)
        setattr(self, tag + '2', mk(planes))
        self.downsample = None
        if downsample:
            self.downsample = nn.Sequential(nn.Conv2d(inplanes, planes, 1, stride=stride, bias=True),
                                            mk(planes))

    def _convs(self) -> dict:
        """the block's convolutions under the keys of its packed sets"""
        convs = dict(c1=self.conv1, c2=self.conv2)
        if self.downsample is not None:
            convs['ds'] = self.downsample[0]
        return convs

    def _pack(self):
        n1, n2 = getattr(self, self.tag + '1'), getattr(self, self.tag + '2')
        eps = n1.eps
        p = dict(c1=PackedConv.from_weight(self.conv1.weight, self.conv1.bias, self.stride, 1,
                                           bn=_bn_params(n1), eps=eps),
                 c2=PackedConv.from_weight(self.conv2.weight, self.conv2.bias, 1, 1,
                                           bn=_bn_params(n2), eps=eps))
        if self.downsample is not None:
            ds = self.downsample[0]
            p['ds'] = PackedConv.from_weight(ds.weight, ds.bias, self.stride, 0,
                                             bn=_bn_params(self.downsample[1]), eps=eps)
        return p

    def forward(self, x: Tensor, norm, kept: Optional[dict] = None, i: int = 0) -> Tensor:
        """resnet.py:67-94, the one walk of a block: conv1 -> norm and ReLU -> conv2 -> norm, residual and ReLU.  ``norm``
        is the norm kind (``_FoldedBN``, ``_RawIN``, ``_BatchBN`` below) and supplies what differs: the packed set, what
        rides in the convolutions' epilogues, the two norm calls and whether they write in place.
        ``kept``: the encoder's dict while it keeps; block ``i`` leaves t{i} (the post-ReLU conv1 output) and y{i} (its
        output) there, the forward's own tensors, and the norm kind what its backward reads besides."""
        p = norm.packs(self)
        # a block with a shortcut convolution hands both layers that read x to ops.conv2d_pair: on full grids the blocks of a
        # 3x3 / s2 conv1 compute the 1x1 / s2 shortcut from the patch they stage anyway (conv_dma.hip, shared-input form)
        if 'ds' in p:
            u1, r = ops.conv2d_pair((p['c1'], x, norm.rides), (p['ds'], x))
        else:
            u1, r = ops.conv2d(p['c1'], x, **norm.rides), None
        t = norm.mid(self, u1, kept, f'1_{i}')
        u2 = ops.conv2d(p['c2'], t, res=(x if r is None else r) if norm.fused else None, **norm.rides)
        # (a shortcut's own normalisation rides in the block's final pass)
        out = norm.tail(self, u2, x, r, kept, i)
        if kept is not None:
            kept[f't{i}'], kept[f'y{i}'] = t, out
        return out


# The three norm kinds of an encoder, each with both directions side by side.
#
# Forward, what _BasicBlock.forward and RAFTEncoder.forward ask: packs(mod) -> the packed set the walk launches; rides: the
# conv2d keywords of every launch but the head's; fused: conv2's launch also takes the residual (the block's input, or its
# shortcut's raw output); mid(mod, u, kept, k) -> the map behind the stem (mod the encoder, k = '_stem') or behind conv1
# (mod the block, k = '1_<i>') from the raw output u; tail(block, u2, x, r, kept, i) -> block i's output from conv2's output,
# the block's input x and the shortcut's raw output r (None without one).  kept is None outside keeping(): a norm may then
# write in place; otherwise it leaves there what KEPT names: per kind the keys behind the walk's own (x, stem, t<i>, y<i>,
# out) at the stem, in every block, in a block with a shortcut convolution.  _kept_keys spells them out.  _Norm has the
# pieces of a kind that launches the folded packs bare and has no norm launch; a kind overrides what it does otherwise.
#
# Backward, what RAFTEncoder._walk_back asks: grad(...) -> six closures over one backward's state.  With a layer = (the key
# of its record, of its convolution, of its norm, the two modules): weight(*layer) -> the weight its dgrad reads (and opens
# its record); slots(ckey) -> (dw, db, accumulate) of its wgrad; put(*layer, dw, db, **launch): that wgrad's results into
# grads, the launch's operands into the record; tail(key, G, i, shortcut) -> (conv2's cotangent, the shortcut's) in block i;
# mid(nkey, g, ukey, skey) -> the cotangent at a raw convolution output (kept under ukey, its statistics under skey) from the
# one behind its norm nkey and ReLU; mask(i, x) -> the ReLU mask of x, the input of block i (the head: the block count), as
# keywords of the dgrad that produces x's cotangent.
class _Norm:
    """the forward pieces of a kind that launches ``packed`` with nothing in the epilogues and no norm behind them"""
    rides, fused = {}, False

    @staticmethod
    def packs(mod):
        return mod.packed

    @staticmethod
    def mid(mod, u, kept, k):
        return u

    @staticmethod
    def tail(blk, u2, x, r, kept, i):
        return u2


class _FoldedBN(_Norm):
    """BatchNorm on eval statistics: every layer is the folded convolution (W', b') of ``packed`` with the ReLU, and behind
    conv2 the residual, in its epilogue; no norm launch at all.  A dgrad reads ``bn_fold``'s weight, and (dW', db') are
    temporaries that ``bn_unfold`` carries to the four raw parameters"""
    KEPT = dict(stem=(), block=(), shortcut=())
    rides, fused = dict(act=ACT_RELU), True

    @staticmethod
    def grad(enc: 'RAFTEncoder', grads: dict, dst: dict, acc: bool, rec: dict, prefix: str, got: dict, eps: float):
        def weight(rkey, ckey, bkey, conv, bn):
            wf, bf = ops.bn_fold(conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)
            rec[rkey] = dict(wf=wf, bf=bf)
            return wf

        def put(rkey, ckey, bkey, conv, bn, dwf, dbf, **launch):
            ks = [f'{prefix}{ckey}.weight', f'{prefix}{ckey}.bias', f'{prefix}{bkey}.weight', f'{prefix}{bkey}.bias']
            res = ops.bn_unfold(conv.weight, conv.bias, bn.weight, bn.running_mean, bn.running_var, bn.eps, dwf, dbf,
                                out=[dst[k] for k in ks], accumulate=acc)
            grads.update(zip(ks, res))
            rec[rkey].update(dwf=dwf, dbf=dbf, **launch)

        # nothing sits between the convolution gradients: G is already the cotangent at a block's pre-ReLU sum, which conv2
        # and the shortcut both read, because every dgrad masks with its layer's input (the layer in front ends in that ReLU)
        return (weight, lambda ckey: (None, None, False), put, lambda key, G, i, shortcut: (G, G),
                lambda nkey, g, ukey, skey: g, lambda i, x: dict(a=x, act=ACT_RELU))


class _RawIN(_Norm):
    """InstanceNorm (affine=False): the convolutions of ``packed``, which fold nothing, with ``ops.instance_norm`` behind
    each, into the convolution's own output -- while keeping out of place (the same kernel on the same values, so the same
    bits), because ``in_backward`` recomputes the statistics from the raw outputs.  Backward: the raw weights, (dW, db)
    straight into their two ``_grad_slots`` destinations, and ``ops.instance_norm_grad`` between the convolution gradients"""
    KEPT = dict(stem=('u_stem',), block=('u1_', 'u2_'), shortcut=('r',))

    @staticmethod
    def mid(mod, u, kept, k):
        if kept is not None:
            kept['u' + k] = u
        return ops.instance_norm(u, relu=True, out=u if kept is None else None)

    @staticmethod
    def tail(blk, u2, x, r, kept, i):
        if kept is None:
            return ops.instance_norm(u2, res=x if r is None else r, relu=True, out=u2, res_norm=r is not None)
        kept[f'u2_{i}'] = u2
        if r is not None:
            kept[f'r{i}'] = r
        # the shortcut's raw output is normalised in a copy: the res_norm pass uses res as scratch
        return ops.instance_norm(u2, res=x if r is None else r.clone(), relu=True, res_norm=r is not None)

    @staticmethod
    def grad(enc: 'RAFTEncoder', grads: dict, dst: dict, acc: bool, rec: dict, prefix: str, got: dict, eps: float):
        def weight(rkey, ckey, bkey, conv, bn):
            rec[rkey] = {}
            return conv.weight

        def slots(ckey):
            return dst[f'{prefix}{ckey}.weight'], dst[f'{prefix}{ckey}.bias'], acc

        def put(rkey, ckey, bkey, conv, bn, dw, db, **launch):
            grads[f'{prefix}{ckey}.weight'], grads[f'{prefix}{ckey}.bias'] = dw, db
            rec[rkey].update(launch)

        def tail(key, G, i, shortcut):
            # G is the cotangent at the block's OUTPUT y: the tail form masks with y -> g' = G [y > 0], the shortcut's
            # cotangent, and du2; behind a normalised shortcut (du2, dr)
            y, u2 = got[f'y{i}'], got[f'u2_{i}']
            if not shortcut:
                g_sc, du2 = ops.instance_norm_grad(G, u2, y=y, eps=eps)
                rec[f'{key}.in2'] = dict(g=G, y=y, u=u2, gp=g_sc, du=du2)
            else:
                du2, g_sc = ops.instance_norm_grad(G, u2, y=y, r=got[f'r{i}'], eps=eps)
                rec[f'{key}.in2'] = dict(g=G, y=y, u=u2, r=got[f'r{i}'], du=du2, dr=g_sc)
            return du2, g_sc

        def mid(nkey, g, ukey, skey):
            du = ops.instance_norm_grad(g, got[ukey], eps=eps)
            rec[nkey] = dict(g=g, u=got[ukey], du=du)
            return du

        # only in front of block 0 the stem's output masks in the epilogue; elsewhere the tail form of the block in front masks
        return weight, slots, put, tail, mid, lambda i, x: dict(a=x, act=ACT_RELU) if i == 0 else {}


class _BatchBN(_Norm):
    """BatchNorm on the statistics of the batch: the raw convolutions (``_raw_packs``) with ``ops.batch_norm_train`` behind
    each, two more launches per norm than the folded form; it never writes in place (the backward reads the raw output),
    moves the layer's running statistics and batch count, and keeps each layer's (2, C) mean / rstd next to its raw output.
    Backward: ``_RawIN``'s (raw weights, unmasked joins, the stem's mask in front of block 0 only) with
    ``ops.batch_norm_train_grad`` between the convolution gradients, on the kept statistics, and its (dgamma, dbeta) into
    the slots of the norm's two parameters"""
    KEPT = dict(stem=('u_stem', 's_stem'), block=('u1_', 'u2_', 's1_', 's2_'), shortcut=('r', 'sr'))

    @staticmethod
    def packs(mod):
        return _raw_packs(mod, mod._convs())

    @staticmethod
    def mid(mod, u, kept, k):
        t, s = _bn_step(mod.bn1, u, relu=True)
        if kept is not None:
            kept['u' + k], kept['s' + k] = u, s
        return t

    @staticmethod
    def tail(blk, u2, x, r, kept, i):
        if r is None:
            out, s2 = _bn_step(blk.bn2, u2, res=x, relu=True)
        else:
            bn_r = blk.downsample[1]
            out, s2, sr = _bn_step(blk.bn2, u2, res=r, relu=True, res_bn=_bn_params(bn_r))
            bn_r.num_batches_tracked += 1
        if kept is not None:
            kept[f'u2_{i}'], kept[f's2_{i}'] = u2, s2
            if r is not None:
                kept[f'r{i}'], kept[f'sr{i}'] = r, sr
        return out

    @staticmethod
    def grad(enc: 'RAFTEncoder', grads: dict, dst: dict, acc: bool, rec: dict, prefix: str, got: dict, eps: float):
        weight, slots, put, _, _, mask = _RawIN.grad(enc, grads, dst, acc, rec, prefix, got, eps)

        def norm(bkey):
            ks = [f'{prefix}{bkey}.weight', f'{prefix}{bkey}.bias']
            return enc.get_submodule(bkey).weight, ks, [dst[k] for k in ks]

        def tail(key, G, i, shortcut):
            y, u2 = got[f'y{i}'], got[f'u2_{i}']
            gamma, ks, into = norm(f'{key}.bn2')
            if not shortcut:
                g_sc, du2, *dp = ops.batch_norm_train_grad(G, u2, got[f's2_{i}'], gamma, y=y, out=[None, None] + into,
                                                           accumulate=acc)
                rec[f'{key}.bn2'] = dict(g=G, y=y, u=u2, gp=g_sc, du=du2)
            else:
                gamma_r, ks_r, into_r = norm(f'{key}.downsample.1')
                du2, g_sc, *dp = ops.batch_norm_train_grad(G, u2, got[f's2_{i}'], gamma, y=y, r=got[f'r{i}'],
                                                           saved_r=got[f'sr{i}'], gamma_r=gamma_r,
                                                           out=[None, None] + into + into_r, accumulate=acc)
                rec[f'{key}.bn2'] = dict(g=G, y=y, u=u2, r=got[f'r{i}'], du=du2, dr=g_sc)
                ks = ks + ks_r
            grads.update(zip(ks, dp))
            return du2, g_sc

        def mid(nkey, g, ukey, skey):
            gamma, ks, into = norm(nkey)
            du, *dp = ops.batch_norm_train_grad(g, got[ukey], got[skey], gamma, out=[None] + into, accumulate=acc)
            grads.update(zip(ks, dp))
            rec[nkey] = dict(g=g, u=got[ukey], du=du)
            return du

        return weight, slots, put, tail, mid, mask


def _kept_keys(norm, blocks: Sequence['_BasicBlock'], out: bool = True) -> List[str]:
    """The keys a forward of norm kind ``norm`` under ``keeping()`` leaves in ``RAFTEncoder.kept``, which are the keys the
    kind's backward reads, for the encoder's blocks ``blocks``; ``out=False``: without the head's output, for a backward
    whose caller passes it.

    Every kind: x (the input image), stem (the stem's output), per block i t{i} (the post-ReLU conv1 output) and y{i} (the
    block's output), and out (the head's post-activation output): what ``backward()`` reads.  The forward's own tensors; out
    is a copy when the caller owns its destination.  An InstanceNorm encoder normalises out of place while keeping (same
    bits) and adds what ``in_backward()`` reads: u_stem, u1_{i}, u2_{i} (the raw outputs of the stem and of a block's two
    convolutions) and r{i} (the raw output of a shortcut convolution, i = 2, 4).  Under ``batch_stats()`` a BatchNorm
    encoder leaves the InstanceNorm set plus each layer's (2, C) batch mean / rstd: s_stem, s1_{i}, s2_{i}, sr{i} -- what
    ``bn_backward()`` reads."""
    more = norm.KEPT
    return (['x', 'stem', *more['stem']]
            + [f'{k}{i}' for i in range(len(blocks)) for k in ('t', 'y') + more['block']]
            + [f'{k}{i}' for i, blk in enumerate(blocks) if blk.downsample is not None for k in more['shortcut']]
            + (['out'] if out else []))


@ENCODERS.register_module()
class RAFTEncoder(HipModule):
    """encoder/raft_encoder.py:13-314, net_type 'Basic' (the SCFlow config):
    7x7/s2 stem, three stages of two BasicBlocks (64, 96, 128; strides 1, 2, 2), 1x1 head.
    ``norm_cfg`` IN -> feature encoder, BN -> context encoder (eval statistics)."""

    def __init__(self, in_channels: int, out_channels: int, scale: float = 1 / 8,
                 net_type: str = 'Basic', norm_cfg: dict = dict(type='BN', requires_grad=True),
                 init_cfg=None, **unsupported) -> None:
        super().__init__()
        if net_type != 'Basic':
            raise NotImplementedError("only net_type='Basic' is built (SCFlow config)")
        bad = {k: v for k, v in unsupported.items()
               if v not in (None, False, -1) and k not in ('conv_cfg',)}
        if bad:
            raise NotImplementedError(f'RAFTEncoder options not built: {sorted(bad)}')
        kind = norm_cfg['type']
        if kind not in ('IN', 'BN', 'SyncBN'):
            raise NotImplementedError(f'norm {kind}')
        kind = 'IN' if kind == 'IN' else 'BN'
        self.kind, self.tag = kind, ('in' if kind == 'IN' else 'bn')
        self.in_channels, self.out_channels, self.scale = in_channels, out_channels, scale
        mk = (lambda c: nn.InstanceNorm2d(c)) if kind == 'IN' else (lambda c: nn.BatchNorm2d(c))
        self.stem_stride = 1 if scale == 1 / 4 else 2
        self.conv1 = nn.Conv2d(in_channels, 64, 7, stride=self.stem_stride, padding=3, bias=True)
        setattr(self, self.tag + '1', mk(64))
        inplanes = 64
        self.res_layers = []
        for i, (planes, stride) in enumerate(zip((64, 96, 128), (1, 2, 2)), start=1):
            layer = nn.Sequential(
                _BasicBlock(inplanes, planes, stride, kind, stride != 1 or inplanes != planes),
                _BasicBlock(planes, planes, 1, kind, False))
            self.add_module(f'res_layer{i}', layer)
            self.res_layers.append(f'res_layer{i}')
            inplanes = planes
        self.conv2 = nn.Conv2d(128, out_channels, 1)
        # under keeping() a forward leaves in ``kept`` what the backward of its norm kind reads (_kept_keys).  Its own switch,
        # not a level of SCFlowDecoder.keep; a forward outside keeping() empties it
        self.keep = False
        self.kept = {}
        # under batch_stats() a BatchNorm encoder normalises with the statistics of the batch and moves its running
        # statistics (the reference's freeze_bn=False)
        self.batch = False

    @contextlib.contextmanager
    def batch_stats(self):
        """forwards inside the body run BatchNorm on the statistics of the batch (``ops.batch_norm_train`` behind the raw
        convolutions) and move ``running_mean``, ``running_var`` and ``num_batches_tracked`` of all 15 layers, as
        ``nn.BatchNorm2d`` does in ``train()`` mode; a setting of the caller's stays.  BatchNorm encoders only.  ``SyncBN``
        configs map to BN here as everywhere: the statistics are those of this process's own batch, nothing is exchanged
        between processes."""
        if self.kind != 'BN':
            raise NotImplementedError('RAFTEncoder.batch_stats: an InstanceNorm encoder has no batch statistics')
        prev = self.batch
        self.batch = True
        try:
            yield self
        finally:
            self.batch = prev

    @contextlib.contextmanager
    def keeping(self):
        """forwards inside the body leave their activations in ``kept`` (a setting of the caller's stays)"""
        prev = self.keep
        self.keep = True
        try:
            yield self
        finally:
            self.keep = prev

    def _convs(self) -> dict:
        """the encoder's own convolutions under the keys of its packed sets"""
        return dict(stem=self.conv1, head=self.conv2)

    def _pack(self):
        n1 = getattr(self, self.tag + '1')
        return dict(stem=PackedConv.from_weight(self.conv1.weight, self.conv1.bias, self.stem_stride, 3,
                                                bn=_bn_params(n1), eps=n1.eps),
                    head=PackedConv.from_weight(self.conv2.weight, self.conv2.bias, 1, 0))

    def _blocks(self) -> List[_BasicBlock]:
        return [blk for name in self.res_layers for blk in getattr(self, name)]

    def _norm(self):
        """the norm kind the next forward runs"""
        return _BatchBN if self.batch else (_FoldedBN if self.kind == 'BN' else _RawIN)

    def forward(self, x: Tensor, out: Optional[Tensor] = None, head_act: int = ACT_NONE,
                head_act2: int = ACT_NONE, head_split: int = 0) -> Tensor:
        """raft_encoder.py:286-314, the one walk of the encoder: stem, blocks, 1x1 head, with whatever depends on the norm
        from the norm kind (``_BasicBlock.forward``).  ``out`` / ``head_*`` let the caller have the 1x1 head write (with a
        split tanh/relu epilogue) straight into a slice of a larger buffer."""
        norm, blocks = self._norm(), self._blocks()
        p = norm.packs(self)
        kept = dict(x=x) if self.keep else None
        u = ops.conv2d(p['stem'], x, **norm.rides)
        y = norm.mid(self, u, kept, '_stem')
        if kept is not None:
            kept['stem'] = y
        for i, blk in enumerate(blocks):
            y = blk(y, norm, kept, i)
        y = ops.conv2d(p['head'], y, out=out, act=head_act, act2=head_act2, act_split=head_split)
        if self.batch:
            # the folded packs went stale as the running statistics moved: the next eval forward folds again
            self._drop_folded()
        if kept is not None:
            kept['out'] = y.clone() if out is not None else y         # with the kind's entries: _kept_keys(norm, blocks)
        self.kept = kept or {}
        return y

    def _saved_for_backward(self, what: str, saved, keys: Sequence[str], nb: int, whose: str) -> Tuple[dict, tuple]:
        """(the entries ``keys`` of ``saved``, the shape of the head's output behind the last of ``nb`` blocks), or the
        error that names ``keeping()``; first the refusal of the stem that has no wgrad"""
        if self.stem_stride != 2:
            raise NotImplementedError(f'{what}: the stride-1 stem (scale 1/4) has no weight gradient')
        try:
            got = {k: saved[k] for k in keys}
        except (KeyError, TypeError):
            raise _lib_error(f"{what}: saved holds {', '.join(keys)}: RAFTEncoder.kept after {whose} under "
                             'keeping()') from None
        y_last = got[f'y{nb - 1}']
        return got, (y_last.shape[0], self.out_channels) + tuple(y_last.shape[2:])

    def _walk_back(self, what: str, norm, got: dict, g_head: Tensor, param_grads: Optional[dict],
                   intermediates: Optional[dict], prefix: str) -> dict:
        """The one reverse walk behind ``backward``, ``bn_backward`` and ``in_backward``: the 1x1 head from ``g_head`` (the
        cotangent at its raw output), the blocks last to first (conv2, conv1, a down-sampling block's shortcut), the stem,
        on ``got`` (the kept tensors, checked by the caller).  Whatever depends on the norm kind is one of the six closures
        of ``norm.grad`` (``_FoldedBN``, ``_RawIN``, ``_BatchBN``)."""
        names = [prefix + k for k, _ in self.named_parameters()]
        grads, dst, acc = _grad_slots(f'{what}: param_grads holds some of the encoder\'s gradients', names, param_grads)
        dst = dict(zip(names, dst))
        rec = {} if intermediates is None else intermediates
        tag = self.tag
        weight, slots, put, tail, mid, mask = norm.grad(self, grads, dst, acc, rec, prefix, got, getattr(self, tag + '1').eps)
        i = len(self._blocks())
        # ---- head: 1x1, no norm
        y_last, kw, kb = got[f'y{i - 1}'], f'{prefix}conv2.weight', f'{prefix}conv2.bias'
        grads[kw], grads[kb] = ops.conv_s1_wgrad(g_head, y_last, (1, 1), dw=dst[kw], db=dst[kb], accumulate=acc)
        G = ops.conv_s1_dgrad(g_head, self.conv2.weight, **mask(i, y_last))
        rec['head'] = dict(g=g_head, x=y_last, gx=G)
        # ---- blocks, last to first
        for name in reversed(self.res_layers):
            layer = getattr(self, name)
            for j in reversed(range(len(layer))):
                i -= 1
                blk, key = layer[j], f'{name}.{j}'
                x_in, t = (got[f'y{i - 1}'] if i else got['stem']), got[f't{i}']
                g2, g_sc = tail(key, G, i, blk.downsample is not None)
                c2 = (f'{key}.conv2', f'{key}.conv2', f'{key}.{tag}2', blk.conv2, getattr(blk, tag + '2'))
                w2 = weight(*c2)
                dw, db, into = slots(c2[1])
                dw, db = ops.conv_s1_wgrad(g2, t, (3, 3), dw=dw, db=db, accumulate=into)
                g_t = ops.conv_s1_dgrad(g2, w2, a=t, act=ACT_RELU)
                put(*c2, dw, db, g=g2, x=t, gx=g_t)
                g1 = mid(f'{key}.{tag}1', g_t, f'u1_{i}', f's1_{i}')
                c1 = (f'{key}.conv1', f'{key}.conv1', f'{key}.{tag}1', blk.conv1, getattr(blk, tag + '1'))
                w1 = weight(*c1)
                dw, db, into = slots(c1[1])
                if blk.downsample is None:
                    dw, db = ops.conv_s1_wgrad(g1, x_in, (3, 3), dw=dw, db=db, accumulate=into)
                    G = ops.conv_s1_dgrad(g1, w1, add=g_sc, **mask(i, x_in))
                    put(*c1, dw, db, g=g1, x=x_in, add=g_sc, gx=G)
                else:
                    in_hw = tuple(x_in.shape[2:])
                    dw, db = ops.conv_wgrad(g1, x_in, dw=dw, accumulate=into), ops.channel_sum(g1, out=db, accumulate=into)
                    gx1 = ops.conv_dgrad(g1, w1, in_hw)
                    put(*c1, dw, db, g=g1, x=x_in, gx=gx1)
                    ds = (f'{key}.downsample', f'{key}.downsample.0', f'{key}.downsample.1', *blk.downsample)
                    wd = weight(*ds)
                    dw, db, into = slots(ds[1])
                    dw, db = ops.conv_ds_wgrad(g_sc, x_in, dw=dw, db=db, accumulate=into)
                    G = ops.conv_ds_dgrad(g_sc, wd, in_hw, add=gx1, **mask(i, x_in))
                    put(*ds, dw, db, g=g_sc, x=x_in, add=gx1, gx=G)
        # ---- stem: G carries the ReLU mask of the stem's output; the image needs no gradient
        g0 = mid(f'{tag}1', G, 'u_stem', 's_stem')
        rec['conv1'] = {}
        dw, db, into = slots('conv1')
        dw, db = ops.conv_stem_wgrad(g0, got['x'], dw=dw, db=db, accumulate=into)
        put('conv1', 'conv1', tag + '1', self.conv1, getattr(self, tag + '1'), dw, db, g=g0, x=got['x'])
        return grads

    def backward(self, saved: dict, g_out: Union[Tensor, Sequence[Tensor]], out: Optional[Tensor] = None,
                 head_act: int = ACT_NONE, head_act2: int = ACT_NONE, head_split: int = 0,
                 param_grads: Optional[dict] = None, intermediates: Optional[dict] = None, prefix: str = ''):
        """Backward of the BatchNorm (eval statistics) encoder with respect to its parameters: the reference's context
        encoder under ``freeze_bn=True``.  The input image gets no gradient.

        ``saved``: ``kept`` of a forward under ``keeping()`` (x, stem, t0 .. t5, y0 .. y5, out).  ``g_out``: the cotangent
        at the head's post-activation output (N, out_channels, h, w), or its channel slices in order (with the refiner's
        split head: d loss / d h0, d loss / d context).  ``out``: the head's post-activation output where ``saved`` does
        not hold it (``SCFlowDecoder.kept`` has h0 and c from keep level 'gru' on); ``head_*`` as the forward was called.
        -> the gradients of the parameters summed over the samples, keyed as ``named_parameters()`` behind ``prefix`` (62
        entries).  A ``param_grads`` passed in is accumulated into (entries it lacks are created; some but not all: an
        error).

        Chain: act_grad on the head's output; wgrad + dgrad (ReLU mask of y5 in the epilogue) of the 1x1 head; then per
        block in reverse, with G the cotangent at the block's pre-ReLU sum: conv2's wgrad (G, t) and dgrad with the mask
        of t -> G_t; a stride-1 conv1: wgrad (G_t, x) and ``conv_s1_dgrad(G_t, W1', add=G, a=x, act=RELU)``; a stride-2
        conv1: ``conv_wgrad`` + ``channel_sum`` (the bias), ``conv_dgrad``, the shortcut's ``conv_ds_wgrad`` (G, x) and the
        join ``conv_ds_dgrad`` that adds both input gradients under the mask of x; last the stem's ``conv_stem_wgrad``.
        Every BatchNorm layer's dgrad reads the folded weight (``bn_fold``), and its (dW', db') go through ``bn_unfold``.

        ``intermediates``: a dict that receives every launch's operands and results (None: nothing is kept)."""
        what = 'RAFTEncoder.backward'
        if self.kind != 'BN':
            raise NotImplementedError(f'{what}: this is the BatchNorm chain; the InstanceNorm feature encoder\'s is '
                                      'RAFTEncoder.in_backward, which takes a cotangent at the encoder\'s output -- the '
                                      'correlation-build backward (SCFlowDecoder.corr_backward) produces it')
        got, u = self._head_cotangent(what, _FoldedBN, saved, 'a forward', g_out, out, head_act, head_act2, head_split)
        return self._walk_back(what, _FoldedBN, got, u, param_grads, intermediates, prefix)

    def _head_cotangent(self, what: str, norm, saved, whose: str, g_out, out: Optional[Tensor], head_act: int,
                        head_act2: int, head_split: int) -> Tuple[dict, Tensor]:
        """what ``backward`` and ``bn_backward`` do in front of the walk: (the entries of ``saved`` that the norm kind
        keeps, with the head's output where the caller passes none; the cotangent at the 1x1 head's raw output from
        ``g_out`` through the head's activation(s))"""
        blocks = self._blocks()
        got, shape = self._saved_for_backward(what, saved, _kept_keys(norm, blocks, out=out is None), len(blocks), whose)
        if out is None:
            out = got['out']
        n, co = shape[:2]
        if tuple(out.shape) != shape:
            raise _lib_error(f'{what}: out must be {shape}, got {tuple(out.shape)}')
        split = int(head_split)
        if not 0 <= split < co:
            raise _lib_error(f'{what}: head_split {split} outside [0, {co})')
        parts = [(0, co, head_act)] if split == 0 else [(0, split, head_act), (split, co, head_act2)]
        gs = [g_out] if isinstance(g_out, torch.Tensor) else list(g_out)
        if len(gs) == 1:
            if tuple(gs[0].shape) != shape:
                raise _lib_error(f'{what}: g_out must be {shape}, got {tuple(gs[0].shape)}')
            gs = [gs[0][:, a:b] for a, b, _ in parts]
        elif len(gs) != len(parts) or any(tuple(g.shape) != (n, b - a) + shape[2:] for g, (a, b, _) in zip(gs, parts)):
            raise _lib_error(f'{what}: g_out is one {shape} tensor or its {len(parts)} channel slices '
                             f'{[(n, b - a) + shape[2:] for a, b, _ in parts]}, got {[tuple(g.shape) for g in gs]}')
        # ---- the head's cotangent: through its activation(s)
        u = torch.empty(shape, dtype=torch.float32, device=out.device)
        for g, (a, b, act) in zip(gs, parts):
            ops.act_grad(g, None if act == ACT_NONE else out[:, a:b], act, out=u[:, a:b])
        return got, u

    def bn_backward(self, saved: dict, g_out: Union[Tensor, Sequence[Tensor]], out: Optional[Tensor] = None,
                    head_act: int = ACT_NONE, head_act2: int = ACT_NONE, head_split: int = 0,
                    param_grads: Optional[dict] = None, intermediates: Optional[dict] = None, prefix: str = ''):
        """Backward of the BatchNorm encoder on the statistics of the batch with respect to its parameters: the reference's
        context encoder under ``freeze_bn=False``.  The input image gets no gradient, the running statistics have none.

        ``saved``: ``kept`` of a forward under ``batch_stats()`` and ``keeping()``: what ``in_backward`` reads (x, stem,
        u_stem and per block t, y, u1_, u2_, with r for the two down-sampling blocks) plus every norm's (2, C) batch mean and
        rstd (s_stem, s1_, s2_, sr).  ``g_out``, ``out``, ``head_*``, ``param_grads``, ``intermediates``, ``prefix``: as in
        ``backward``, whose head handling this is.  -> the gradients of all 62 parameters.

        Chain: ``in_backward``'s, with ``ops.batch_norm_train_grad`` where that has ``ops.instance_norm_grad``: the
        statistics couple the samples of the batch, so d loss / d u carries the two channel sums S1 and S2, which are also
        (dbeta, dgamma).  Raw weights, unmasked joins, the stem's mask in front of block 0 only.

        The bias of a convolution in front of a BatchNorm has gradient 0 in exact arithmetic (du sums to 0 over a channel);
        it is computed like any other bias gradient and comes out as rounding noise, as autograd's does.

        ``SyncBN`` configs map to BN: the statistics, and so this derivative, are those of the process's own batch."""
        what = 'RAFTEncoder.bn_backward'
        if self.kind != 'BN':
            raise NotImplementedError(f'{what}: an InstanceNorm encoder takes RAFTEncoder.in_backward')
        got, u = self._head_cotangent(what, _BatchBN, saved, 'a forward under batch_stats()', g_out, out, head_act, head_act2,
                                      head_split)
        return self._walk_back(what, _BatchBN, got, u, param_grads, intermediates, prefix)

    def in_backward(self, saved: dict, g_out: Tensor, param_grads: Optional[dict] = None,
                    intermediates: Optional[dict] = None, prefix: str = ''):
        """Backward of the InstanceNorm encoder with respect to its parameters: the reference's feature encoder
        (``norm_cfg=dict(type='IN')``, affine=False).  The input image gets no gradient.

        ``saved``: ``kept`` of a forward under ``keeping()`` (x, stem, u_stem and per block t, y, u1_, u2_, with r for the
        two down-sampling blocks).  ``g_out``: the cotangent at the 1x1 head's output (N, out_channels, h, w); that head has
        no activation.  -> the gradients of the 32 parameters summed over the samples, keyed as ``named_parameters()``
        behind ``prefix``; ``param_grads`` and ``intermediates`` as in ``backward``.

        Chain: ``backward``'s order and launches on the raw weights (nothing to fold or unfold), with the derivative of
        InstanceNorm (``ops.instance_norm_grad``) between the convolution gradients.  Head: wgrad and an unmasked dgrad ->
        G, the cotangent at the last block's output.  Per block in reverse: the tail form on (G, y, u2) -> g' = G [y > 0]
        (the shortcut's cotangent) and du2 -- a down-sampling block: (du2, dr) from (G, y, u2, r); conv2's wgrad (du2, t)
        and dgrad under the mask of t; the mid form -> du1; conv1's wgrad and a dgrad that adds g' and stays unmasked (the
        block in front masks with its own y; in front of block 0 the stem's output masks in the epilogue) -- a
        down-sampling block: ``conv_wgrad`` + ``channel_sum``, ``conv_dgrad``, the shortcut's ``conv_ds_wgrad`` (dr, x)
        and the unmasked join ``conv_ds_dgrad``.  Last the mid form at the stem and ``conv_stem_wgrad`` at Cin = 3.

        The bias of a convolution in front of an InstanceNorm has gradient 0 in exact arithmetic (du sums to 0 over a
        plane); it is computed like any other bias gradient and comes out as rounding noise, as autograd's does.

        ``SCFlowRefiner.loss_and_network_grads`` calls this with the correlation-build backward's result
        (``SCFlowDecoder.corr_backward``); ``train_step`` does not reach it yet."""
        what = 'RAFTEncoder.in_backward'
        if self.kind != 'IN':
            raise NotImplementedError(f'{what}: a BatchNorm encoder takes RAFTEncoder.backward (eval statistics, folded)')
        blocks = self._blocks()
        got, shape = self._saved_for_backward(what, saved, _kept_keys(_RawIN, blocks, out=False), len(blocks),
                                              "an InstanceNorm encoder's forward")
        if not isinstance(g_out, torch.Tensor) or tuple(g_out.shape) != shape:
            raise _lib_error(f'{what}: g_out must be a {shape} tensor, got '
                             f'{tuple(g_out.shape) if isinstance(g_out, torch.Tensor) else type(g_out).__name__}')
        return self._walk_back(what, _RawIN, got, g_out, param_grads, intermediates, prefix)   # the head has no activation


def encoder_pair_supported(fe: 'RAFTEncoder', ce: 'RAFTEncoder') -> bool:
    """``raft_encoder_pair`` walks an InstanceNorm feature encoder and a BatchNorm context encoder of the same layer geometry;
    other norm kinds run the two encoders one after the other."""
    return (fe.kind == 'IN' and ce.kind == 'BN' and fe.stem_stride == ce.stem_stride and fe.in_channels == ce.in_channels
            and fe.res_layers == ce.res_layers)


def raft_encoder_pair(fe: 'RAFTEncoder', xf: Tensor, ce: 'RAFTEncoder', xc: Tensor, out_c: Optional[Tensor] = None,
                      head_act: int = ACT_NONE, head_act2: int = ACT_NONE, head_split: int = 0) -> Tuple[Tensor, Tensor]:
    """the feature encoder (InstanceNorm) on ``xf`` and the context encoder (BatchNorm, folded) on ``xc`` -- two independent
    passes over layers of identical geometry -- walked TOGETHER, every pair of convolutions through ``ops.conv2d_pair``: at
    batch 1-4 the context encoder's launches ride in the feature encoder's wherever both grids fit the chip (r6; before: one
    after the other, or side by side on a second stream).  Same kernels per layer as the two separate passes, same bits."""
    if not encoder_pair_supported(fe, ce):
        raise ValueError('raft_encoder_pair: (InstanceNorm feature encoder, BatchNorm context encoder) of one layer geometry')
    pf, pc = fe.packed, ce.packed
    fe.kept, ce.kept = {}, {}                  # this walk keeps nothing (SCFlowRefiner.extract_feat: not taken while keeping)
    yf, yc = ops.conv2d_pair((pf['stem'], xf), (pc['stem'], xc, dict(act=ACT_RELU)))
    ops.instance_norm(yf, relu=True, out=yf)
    for name in fe.res_layers:
        for bf, bc in zip(getattr(fe, name), getattr(ce, name)):
            qf, qc = bf.packed, bc.packed
            tf_, tc_ = ops.conv2d_pair((qf['c1'], yf), (qc['c1'], yc, dict(act=ACT_RELU)))
            ops.instance_norm(tf_, relu=True, out=tf_)
            if 'ds' in qf:
                if_, ic_ = ops.conv2d_pair((qf['ds'], yf), (qc['ds'], yc))
            else:
                if_, ic_ = yf, yc
            uf_, yc = ops.conv2d_pair((qf['c2'], tf_), (qc['c2'], tc_, dict(res=ic_, act=ACT_RELU)))
            yf = ops.instance_norm(uf_, res=if_, relu=True, out=uf_, res_norm='ds' in qf)
    return ops.conv2d_pair((pf['head'], yf), (pc['head'], yc, dict(out=out_c, act=head_act, act2=head_act2,
                                                                  act_split=head_split)))


# =============================================================== decoder
class CorrelationPyramid(HipModule):
    """decoder/raft_decoder.py:19-58."""

    def __init__(self, num_levels: int = 4) -> None:
        super().__init__()
        self.num_levels = num_levels

    def forward(self, feat1: Tensor, feat2: Tensor, tiled_levels: int = 0) -> List[Tensor]:
        """``tiled_levels`` (decoder-internal, ``ops.pyramid_layout``): those levels in the lookup's
        8x4-tile layout; the default is the reference's row-major pyramid."""
        return ops.corr_build(feat1, feat2, self.num_levels, tiled_levels=tiled_levels)


class CorrLookup(HipModule):
    """utils/corr_lookup.py:71-136 (bilinear, zeros padding, align_corners=True only)."""

    def __init__(self, radius: int = 4, mode: str = 'bilinear', padding_mode: str = 'zeros',
                 align_corners: bool = True) -> None:
        super().__init__()
        if mode != 'bilinear' or padding_mode != 'zeros' or not align_corners:
            raise NotImplementedError('HIP CorrLookup: bilinear / zeros / align_corners=True')
        self.r = radius

    def forward(self, corr_pyramid: Sequence[Tensor], flow: Tensor,
                tiled_levels: int = 0) -> Tensor:
        return ops.corr_lookup(corr_pyramid, flow, self.r, tiled_levels=tiled_levels)


def _pyramid_layout(feat: Tensor, radius: int, num_levels: int, allow: bool = True) -> int:
    """the decoders keep the pyramid to themselves, so they are free to store it in the layout the
    lookup likes best (``decoder.tiled_pyramid = False`` forces the reference layout: A/B
    measurements in tools/)."""
    return ops.pyramid_layout(feat.shape[-2], feat.shape[-1], radius, num_levels) if allow else 0


class MotionEncoder(HipModule):
    """decoder/raft_decoder.py:61-166, 'Basic' channel plan."""

    def __init__(self, num_levels: int = 4, radius: int = 4, net_type: str = 'Basic',
                 conv_cfg=None, norm_cfg=None, act_cfg=dict(type='ReLU')) -> None:
        super().__init__()
        if net_type not in ('Basic', 'Large') or norm_cfg is not None:
            raise NotImplementedError('MotionEncoder: Basic, no norm')
        cin = num_levels * (2 * radius + 1) ** 2
        self.corr_net = nn.Sequential(ConvBlock(cin, 256, 1, padding=0, act_cfg=act_cfg),
                                      ConvBlock(256, 192, 3, padding=1, act_cfg=act_cfg))
        self.flow_net = nn.Sequential(ConvBlock(2, 128, 7, padding=3, act_cfg=act_cfg),
                                      ConvBlock(128, 64, 3, padding=1, act_cfg=act_cfg))
        self.out_net = nn.Sequential(ConvBlock(256, 126, 3, padding=1, act_cfg=act_cfg))
        self.out_channels = [126]

    def forward(self, corr: Tensor, flow: Tensor, out: Optional[Tensor] = None,
                overlap: bool = False, cf: Optional[Tensor] = None, fork=None) -> Tensor:
        """raft_decoder.py:152-166.  -> (N, 128, h, w) = [out_net(126) | flow(2)], optionally
        written into ``out`` (a channel slice of the GRU input buffer).  ``overlap`` (small
        batches): the flow branch runs on the side stream, from the caller's ``fork`` event
        (``ops.fork_point()``, taken once ``flow`` is enqueued); the caller then also passes ``cf``
        (N, 256, h, w), allocated BEFORE that fork point (the side branch writes it: see
        SCFlowRefiner.extract_feat for the allocator rule)."""
        n, _, h, w = flow.shape
        dev = flow.device
        if out is None:
            out = torch.empty((n, 128, h, w), dtype=torch.float32, device=dev)
        if cf is None:
            if overlap:
                raise ValueError('overlap=True needs a cf buffer allocated before the fork point')
            cf = torch.empty((n, 256, h, w), dtype=torch.float32, device=dev)
        self.branches(corr, flow, cf, overlap=overlap, fork=fork)
        self.out_net[0](cf, out=out[:, :126])
        ops.copy_channels(flow, out[:, 126:128])
        return out

    def branches(self, corr: Tensor, flow: Tensor, cf: Tensor, overlap: bool = False, fork=None,
                 c1: Optional[Tensor] = None, f1: Optional[Tensor] = None) -> Tensor:
        """the correlation and the flow branch of ``forward`` into ``cf`` (N, 256, h, w) = [corr_net (192) | flow_net (64)];
        ``c1`` (N, 256, h, w) / ``f1`` (N, 128, h, w): where the first layers' outputs go when the caller wants them (the
        backward's recomputation), else scratch"""
        if not overlap and 'flow' in ops.PAIR_BRANCHES and ops._CONV_EVENTS is None:
            # r6: the flow branch rides in the correlation branch's launches, layer by layer (ops.conv2d_pair: one launch where
            # the two grids need fewer rounds of resident blocks together, else one after the other; same bits)
            cn, fn = self.corr_net, self.flow_net
            kc, kf = dict(act=cn[0].act), dict(act=fn[0].act)
            if c1 is not None:
                kc['out'] = c1
            if f1 is not None:
                kf['out'] = f1
            c1, f1 = ops.conv2d_pair((cn[0].packed, corr, kc), (fn[0].packed, flow, kf))
            ops.conv2d_pair((cn[1].packed, c1, dict(out=cf[:, :192], act=cn[1].act)),
                            (fn[1].packed, f1, dict(out=cf[:, 192:], act=fn[1].act)))
            del c1, f1
        else:
            br = ops.side_stream(overlap, after=fork)
            with br:
                f1 = self.flow_net[0](flow, out=f1)
                self.flow_net[1](f1, out=cf[:, 192:])
                del f1
            c1 = self.corr_net[0](corr, out=c1)
            self.corr_net[1](c1, out=cf[:, :192])
            br.join()
        return cf

    # ---- backward: five stride-1 convolutions, no recurrence ----
    def param_names(self, prefix: str = '') -> Tuple[str, ...]:
        """the encoder's ten parameters as ``named_parameters()`` keys them, behind ``prefix``"""
        return tuple(f'{prefix}{m}.conv.{k}' for m in ('corr_net.0', 'corr_net.1', 'flow_net.0', 'flow_net.1', 'out_net.0')
                     for k in ('weight', 'bias'))

    def backward(self, saved: dict, g_motion_features: Sequence[Tensor], param_grads: Optional[dict] = None,
                 intermediates: Optional[dict] = None, prefix: str = ''):
        """Backward of the motion encoder (raft_decoder.py:152-166) for the T iterations of a pass at once, M = T N stacked
        samples, one launch per stage.

        ``saved``: ``corr`` (T, N, L (2r+1)^2, h, w), the looked-up (and, under ``mask_corr``, masked) correlation of every
        iteration, and ``x`` (T, N, 128, h, w), the encoder's output [out_net (126, post-activation) | flow_in (2)] that
        ``SCFlowDecoder`` keeps from ``'gru'`` on.  ``g_motion_features``: T cotangents at ``x_t`` (``ConvGRU.backward`` returns
        them).  -> (``g_corr`` (T, N, L (2r+1)^2, h, w): the cotangents at ``corr``; ``g_flow_inputs``: T cotangents at the
        encoder's flow input (N, 2, h, w), the pass-through channels included; ``param_grads``: the gradients of the ten
        parameters summed over all T N samples, keyed as in ``named_parameters()`` behind ``prefix``).  A dict passed in is
        accumulated into (entries it lacks are created; some but not all of these entries: an error).

        The hidden activations ``c1`` (256), ``f1`` (128) and ``cf`` (256) are recomputed into stacked buffers by the
        forward's OWN launches (``branches``), one iteration at a time at the forward's batch, so dispatch and bits are the
        forward's.  Chain per stacked sample: act_grad on ``g_x[:, :126]``; wgrad + dgrad of out_net (ReLU mask of ``cf``
        in the epilogue); corr_net.1 and flow_net.1 on the two column blocks of ``g_cf``; corr_net.0 (1x1) down to
        ``g_corr``; flow_net.0 (7x7) with the pass-through cotangent ``g_x[:, 126:128]`` added.

        ``intermediates``: a dict that receives every launch's operands and results (None: nothing is kept)."""
        what = 'MotionEncoder.backward'
        T = len(g_motion_features)
        if T == 0 or T > ops.TAIL_MAX_T:
            raise _lib_error(f'{what}: 1 .. {ops.TAIL_MAX_T} iterations with one cotangent at x per iteration')
        corr, x = _kept(what, saved, ('corr', 'x'), None)      # x is kept['x']; SCFlowDecoder.motion_backward recomputes corr
        cn, fn, on = self.corr_net, self.flow_net, self.out_net
        co = on[0].conv.out_channels                                  # 126
        if x.dim() != 5 or x.shape[0] != T or x.shape[2] != co + 2 or not x.is_contiguous():
            raise _lib_error(f'{what}: x must be a contiguous ({T}, N, {co + 2}, h, w) tensor, got {tuple(x.shape)}')
        n, _, h, w = x.shape[1:]
        kc = cn[0].conv.in_channels
        if tuple(corr.shape) != (T, n, kc, h, w) or not corr.is_contiguous():
            raise _lib_error(f'{what}: corr must be a contiguous {(T, n, kc, h, w)} tensor, got {tuple(corr.shape)}')
        if any(tuple(g.shape) != (n, co + 2, h, w) for g in g_motion_features):
            raise _lib_error(f'{what}: g_motion_features are {(n, co + 2, h, w)} tensors')
        act = cn[0].act
        if any(b.act != act for b in (cn[1], fn[0], fn[1], on[0])) or act not in (ACT_NONE, ACT_RELU):
            raise NotImplementedError('MotionEncoder.backward: ReLU or no activation')
        names = self.param_names(prefix)
        grads, dst, acc = _grad_slots(f'{what}: param_grads holds some of the motion encoder\'s gradients', names, param_grads)
        dst = dict(zip(names, dst))
        m = T * n
        E = lambda *shape: torch.empty(shape, dtype=torch.float32, device=x.device)       # noqa: E731
        c_c1, c_f1 = cn[0].conv.out_channels, fn[0].conv.out_channels
        c_cc, c_cf = cn[1].conv.out_channels, fn[1].conv.out_channels
        # ---- the forward's own launches, an iteration at a time: c1, f1, cf in the forward's bits
        c1, f1, cf = E(T, n, c_c1, h, w), E(T, n, c_f1, h, w), E(T, n, c_cc + c_cf, h, w)
        for t in range(T):
            self.branches(corr[t], x[t][:, co:], cf[t], c1=c1[t], f1=f1[t])
        g_x = _stacked(g_motion_features, m, co + 2, h, w)
        x_, corr_ = x.view(m, co + 2, h, w), corr.view(m, kc, h, w)
        c1_, f1_, cf_ = c1.view(m, c_c1, h, w), f1.view(m, c_f1, h, w), cf.view(m, c_cc + c_cf, h, w)
        convs = (on[0].conv, cn[1].conv, cn[0].conv, fn[1].conv, fn[0].conv)
        ws = E(max(ops.conv_s1_wgrad_workspace(m, cv.out_channels, cv.in_channels, h, w, *cv.kernel_size) for cv in convs))
        w_scratch = E(max(cv.weight.numel() for cv in convs))
        a_or_none = lambda a: a if act != ACT_NONE else None                              # noqa: E731
        wgrad = partial(_layer_wgrad, grads, dst, acc, ws)
        # 1. out_net
        u = ops.act_grad(g_x[:, :co], a_or_none(x_[:, :co]), act)
        wgrad(f'{prefix}out_net.0.conv', u, cf_, on[0].conv)
        g_cf = ops.conv_s1_dgrad(u, on[0].conv.weight, a=a_or_none(cf_), act=act, w_scratch=w_scratch)
        # 2. correlation branch
        wgrad(f'{prefix}corr_net.1.conv', g_cf[:, :c_cc], c1_, cn[1].conv)
        g_c1 = ops.conv_s1_dgrad(g_cf[:, :c_cc], cn[1].conv.weight, a=a_or_none(c1_), act=act, w_scratch=w_scratch)
        wgrad(f'{prefix}corr_net.0.conv', g_c1, corr_, cn[0].conv)
        g_corr = ops.conv_s1_dgrad(g_c1, cn[0].conv.weight, w_scratch=w_scratch)
        # 3. flow branch: the pass-through channels' cotangent joins at the flow input
        wgrad(f'{prefix}flow_net.1.conv', g_cf[:, c_cc:], f1_, fn[1].conv)
        g_f1 = ops.conv_s1_dgrad(g_cf[:, c_cc:], fn[1].conv.weight, a=a_or_none(f1_), act=act, w_scratch=w_scratch)
        wgrad(f'{prefix}flow_net.0.conv', g_f1, x_[:, co:], fn[0].conv)
        g_fl = ops.conv_s1_dgrad(g_f1, fn[0].conv.weight, add=g_x[:, co:])
        if intermediates is not None:
            intermediates.update(c1=c1, f1=f1, cf=cf, g_x=g_x, u=u, g_cf=g_cf, g_c1=g_c1, g_f1=g_f1, g_corr=g_corr, g_flow_in=g_fl)
        g_fl = g_fl.view(T, n, 2, h, w)
        return g_corr.view(T, n, kc, h, w), [g_fl[t] for t in range(T)], grads


class ConvGRU(HipModule):
    """decoder/raft_decoder.py:168-253.  z and r share their input, so their weights are
    stacked into one 256-row convolution whose epilogue emits z and r*h; the q convolution's
    epilogue applies tanh and the state update (1-z)*h + z*q in place."""
    _kernel = {'Conv': [3], 'SeqConv': [(1, 5), (5, 1)]}
    _padding = {'Conv': [1], 'SeqConv': [(0, 2), (2, 0)]}

    def __init__(self, h_channels: int, x_channels: int, net_type: str = 'SeqConv') -> None:
        super().__init__()
        self.h_channels, self.x_channels = h_channels, x_channels
        mk = lambda act: nn.ModuleList([
            ConvBlock(h_channels + x_channels, h_channels, k, padding=p, act_cfg=dict(type=act))
            for k, p in zip(self._kernel[net_type], self._padding[net_type])])
        self.conv_z, self.conv_r, self.conv_q = mk('Sigmoid'), mk('Sigmoid'), mk('Tanh')

    def _pack_sources(self):          # the packing reads the ConvBlock children's tensors
        return [t for m in (*self.conv_z, *self.conv_r, *self.conv_q) for t in (m.conv.weight, m.conv.bias)]

    def _pack(self):
        packs = []
        for z, r, q in zip(self.conv_z, self.conv_r, self.conv_q):
            w = torch.cat([z.conv.weight, r.conv.weight], 0)
            b = torch.cat([z.conv.bias, r.conv.bias], 0)
            packs.append((PackedConv.from_weight(w, b, 1, z.conv.padding),
                          PackedConv.from_weight(q.conv.weight, q.conv.bias, 1, q.conv.padding)))
        return packs

    # ---- iteration-invariant context (DESIGN.md "GRU context hoisting") ----
    # x = [c | x'] where c (the context features) is the same in every refinement iteration:
    # conv([h | c | x']) = conv([h | x']) + conv_c(c).  ``context_terms`` evaluates conv_c(c) + bias
    # for z | r | q once per pair; ``forward_inplace`` with those terms convolves [h | x'] only.
    def _ctx_packs(self, cc: int):
        """per pass: (PackedConv c -> 3 h_channels rows [z | r | q] with the biases,
        PackedConv [h | x'] -> z | r without bias, PackedConv [h | x'] -> q without bias)"""
        hc = self.h_channels
        key = ('ctx', cc, self._pack_key())
        if self.__dict__.get('_ctx_cache', (None,))[0] != key:
            packs = []
            for z, r, q in zip(self.conv_z, self.conv_r, self.conv_q):
                wz, wr, wq = z.conv.weight.detach(), r.conv.weight.detach(), q.conv.weight.detach()
                sel = lambda w: torch.cat([w[:, :hc], w[:, hc + cc:]], 1)
                w_c = torch.cat([wz[:, hc:hc + cc], wr[:, hc:hc + cc], wq[:, hc:hc + cc]], 0)
                b_c = torch.cat([z.conv.bias, r.conv.bias, q.conv.bias], 0).detach()
                packs.append((PackedConv.from_weight(w_c, b_c, 1, z.conv.padding),
                              PackedConv.from_weight(torch.cat([sel(wz), sel(wr)], 0), None, 1, z.conv.padding),
                              PackedConv.from_weight(sel(wq), None, 1, q.conv.padding)))
            self.__dict__['_ctx_cache'] = (key, packs)
        return self.__dict__['_ctx_cache'][1]

    def context_terms(self, c: Tensor) -> List[Tensor]:
        """one (N, 3 h_channels, H, W) tensor per pass: the c part of conv_z | conv_r | conv_q + bias"""
        return [ops.conv2d(pk[0], c) for pk in self._ctx_packs(c.shape[1])]

    def forward_inplace(self, hx: Tensor, ctx: Optional[Sequence[Tensor]] = None,
                        ctx_channels: int = 0, scratch: Optional[Tensor] = None) -> Tensor:
        """hx: (N, h_ch + x_ch, h, w) = [h | x]; h is updated in place.  One C-ABI call
        (``scf_sepconv_gru``: the launch sequence lives in the library).  ``ctx`` =
        ``context_terms(hx[:, h_ch:h_ch + ctx_channels])`` of this pair: those channels are then
        not convolved again (``scf_sepconv_gru_ctx``)."""
        hc = self.h_channels
        n, _, h, w = hx.shape
        if scratch is None:          # (2, N, Ch, H, W): the z and r*h buffers (a caller's loop passes its own)
            scratch = torch.empty((2, n, hc, h, w), dtype=torch.float32, device=hx.device)
        z, rh = scratch[0], scratch[1]
        if ctx is None:
            ops.sepconv_gru(self.packed, hx, hc, z, rh)
        else:
            packs = [(pk[1], pk[2]) for pk in self._ctx_packs(ctx_channels)]
            ops.sepconv_gru(packs, hx, hc, z, rh, ctx=ctx, ctx_channels=ctx_channels)
        return hx[:, :hc]

    def forward(self, h: Tensor, x: Tensor) -> Tensor:
        """raft_decoder.py:235-253 signature (copies h, x into one buffer)."""
        n, _, hh, ww = h.shape
        hx = torch.empty((n, self.h_channels + self.x_channels, hh, ww), dtype=torch.float32,
                         device=h.device)
        ops.copy_channels(h, hx[:, :self.h_channels])
        ops.copy_channels(x, hx[:, self.h_channels:])
        return self.forward_inplace(hx)

    # ---- backward: a reverse scan over the iterations, the passes of an iteration in reverse ----
    def param_names(self) -> Tuple[str, ...]:
        """the GRU's parameters as ``named_parameters()`` keys them: per pass conv_z, conv_r, conv_q, weight and bias"""
        return tuple(f'{g}.{p}.conv.{k}' for p in range(len(self.conv_z)) for g in ('conv_z', 'conv_r', 'conv_q')
                     for k in ('weight', 'bias'))

    def _saved(self, what: str, saved, T: Optional[int] = None):
        h0, c, x, hv = _kept(what, saved, ('h0', 'c', 'x', 'hv'), 'gru')
        if hv.dim() != 5 or (T is not None and hv.shape[0] != T) or hv.shape[0] == 0 or not hv.is_contiguous():
            raise _lib_error(f'{what}: hv must be a contiguous ({"T" if T is None else T}, N, C, h, w) tensor, got {tuple(hv.shape)}')
        T, n, hc, h, w = hv.shape
        if hc != self.h_channels:
            raise _lib_error(f'{what}: hv has {hc} channels, the GRU state has {self.h_channels}')
        cc = c.shape[1] if c.dim() == 4 else -1
        cx = self.x_channels - cc
        for name, t_, shape in (('h0', h0, (n, hc, h, w)), ('c', c, (n, cc, h, w)), ('x', x, (T, n, cx, h, w))):
            if tuple(t_.shape) != shape or not t_.is_contiguous() or cc < 0 or cx < 1:
                raise _lib_error(f'{what}: {name} must be a contiguous {shape} tensor, got {tuple(t_.shape)}')
        return h0, c, x, hv

    def recompute_gates(self, saved: dict) -> dict:
        """What the backward needs of the forward and the forward does not emit, from the forward's own convolution
        launches (``ops.conv2d`` on the packs of ``_pack``, sigmoid / tanh epilogue), one iteration at a time at the
        forward's batch: per pass the stacked (T, N, C, h, w) tensors ``h_in`` (the pass's input state: ``h0`` / the kept
        ``hv[t - 1]`` for the first pass, the recomputed intermediate state for the second), ``zr`` = [z | r], ``rh`` =
        r h, ``q``, and ``h_out`` (T, N, Ch, h, w), the recomputed ``hv`` (a check value: the scan reads the kept one)."""
        what = 'ConvGRU.recompute_gates'
        h0, c, x, hv = self._saved(what, saved)
        T, n, hc, h, w = hv.shape
        cc, cx = c.shape[1], x.shape[2]
        packs = self.packed
        P = len(packs)
        E = lambda *shape: torch.empty(shape, dtype=torch.float32, device=hv.device)       # noqa: E731
        hxb = E(n, hc + cc + cx, h, w)
        ops.copy_channels(c, hxb[:, hc:hc + cc])
        h_in = [E(T, n, hc, h, w) for _ in range(P)]
        h_in[0][0].copy_(h0)
        if T > 1:
            h_in[0][1:].copy_(hv[:-1])
        zr, rh, q = [E(T, n, 2 * hc, h, w) for _ in range(P)], [E(T, n, hc, h, w) for _ in range(P)], [E(T, n, hc, h, w) for _ in range(P)]
        h_out = E(T, n, hc, h, w)
        for t in range(T):
            ops.copy_channels(x[t], hxb[:, hc + cc:])
            for p, (pzr, pq) in enumerate(packs):
                ops.copy_channels(h_in[p][t], hxb[:, :hc])
                ops.conv2d(pzr, hxb, out=zr[p][t], act=ACT_SIGMOID)
                ops.gru_gate_state(h_in[p][t], zr[p][t][:, hc:], out=rh[p][t])
                ops.conv2d(pq, rh[p][t], hxb[:, hc:], out=q[p][t], act=ACT_TANH)
                ops.gru_gate_state(h_in[p][t], zr[p][t][:, :hc], q[p][t], out=h_in[p + 1][t] if p + 1 < P else h_out[t])
        return dict(h_in=h_in, zr=zr, rh=rh, q=q, h_out=h_out)

    def backward(self, saved: dict, g_hidden_states: Sequence[Tensor], param_grads: Optional[dict] = None,
                 intermediates: Optional[dict] = None):
        """Backward of the T iterations of the GRU (raft_decoder.py:235-253, both ``net_type``s): a reverse scan, t = T - 1
        ... 0, the passes of an iteration in reverse; the carried cotangent is ``g_hidden_states[t]`` plus the ``g_h`` of
        iteration t + 1.

        ``saved``: ``h0`` (N, Ch, h, w), the context ``c`` (N, Cc, h, w), the motion features ``x`` (T, N, Cx', h, w) and
        the kept states ``hv`` (T, N, Ch, h, w) -- ``SCFlowDecoder.kept`` from keep level ``'gru'`` on.
        ``g_hidden_states``: T cotangents at ``hv_t`` (``SCFlowDecoder.heads_backward`` returns them).  -> (``g_h0``: d loss
        / d ``h0``; ``g_context``: d loss / d ``c`` summed over iterations and passes; ``g_motion_features``: T cotangents
        at ``x_t`` (N, Cx', h, w), channel slices of one stacked buffer; ``param_grads``: the gradients of the GRU's
        parameters summed over all T N samples, keyed as in ``named_parameters()``).  A dict passed in is accumulated
        into (entries it lacks are created; some but not all of the GRU's entries: an error).

        Per pass (``scf_gru_gate_grad_q`` -> dgrad of conv_q -> ``scf_gru_gate_grad_r`` -> dgrad of the stacked z | r
        convolution with [g_h_direct | g_x] added) over the [h | x'] columns only; the context columns once per pass
        after the scan on the running sums of the u's (one dgrad and one wgrad at M = N each); the weight gradients
        after the scan over the M = T N stacked samples.  No atomics: every sum has one order.

        ``intermediates``: a dict that receives every launch's operands, for inspection and for the tests that check the
        scan launch by launch (None: nothing is kept or copied): per (pass, iteration) copies of the carried cotangent
        ``g``, the q dgrad's output ``g_q``, the z | r dgrad's ``add`` operand and its output ``out``; the stacked ``u_zr``,
        ``u_q``, the running sums ``s_zr``, ``s_q`` and the recomputed ``gates``."""
        what = 'ConvGRU.backward'
        T = len(g_hidden_states)
        if T == 0 or T > ops.TAIL_MAX_T:
            raise _lib_error(f'{what}: 1 .. {ops.TAIL_MAX_T} iterations with one cotangent at hv per iteration')
        h0, c, x, hv = self._saved(what, saved, T)
        n, hc, h, w = hv.shape[1:]
        cc, cx = c.shape[1], x.shape[2]
        if any(tuple(g.shape) != (n, hc, h, w) for g in g_hidden_states):
            raise _lib_error(f'{what}: g_hidden_states are {(n, hc, h, w)} tensors')
        names = self.param_names()
        grads, dst, acc = _grad_slots(f'{what}: param_grads holds some of the GRU\'s gradients', names, param_grads)
        dst = dict(zip(names, dst))
        gt = self.recompute_gates(saved)
        P = len(self.conv_z)
        E = lambda *shape: torch.empty(shape, dtype=torch.float32, device=hv.device)       # noqa: E731
        # ---- the weights by column block: [h | x'] for the scan, c for the hoisted launches
        hx_cols = lambda wt: torch.cat([wt[:, :hc], wt[:, hc + cc:]], 1).contiguous()       # noqa: E731
        c_cols = lambda wt: wt[:, hc:hc + cc].contiguous()                                 # noqa: E731
        w_zr = [torch.cat([z.conv.weight.detach(), r.conv.weight.detach()], 0) for z, r in zip(self.conv_z, self.conv_r)]
        w_q = [q.conv.weight.detach() for q in self.conv_q]
        w_zr_hx, w_q_hx, w_zr_c, w_q_c = ([f(wt) for wt in ws_] for f, ws_ in ((hx_cols, w_zr), (hx_cols, w_q),
                                                                                (c_cols, w_zr), (c_cols, w_q)))
        w_scratch = E(max(wt.numel() for wt in w_zr_hx))
        # ---- the scan
        u_zr, u_q = [E(T, n, 2 * hc, h, w) for _ in range(P)], [E(T, n, hc, h, w) for _ in range(P)]
        s_zr, s_q = [E(n, 2 * hc, h, w) for _ in range(P)], [E(n, hc, h, w) for _ in range(P)]
        out = E(T, n, hc + cx, h, w)                   # per iteration [g_h | g_x'] of its first pass: the pass's complete result
        g_q, carry = E(n, hc + cx, h, w), E(n, hc, h, w)
        rec = (lambda *a: None) if intermediates is None else (                            # noqa: E731
            lambda key, p, t, v: intermediates.setdefault(key, {}).__setitem__((p, t), v.clone()))
        for t in reversed(range(T)):
            first = t == T - 1
            g = g_hidden_states[t] if first else ops.gru_carry(out[t + 1][:, :hc], g_hidden_states[t], out=carry)
            add_x = None
            for p in reversed(range(P)):
                h_in, z, r, q = gt['h_in'][p][t], gt['zr'][p][t][:, :hc], gt['zr'][p][t][:, hc:], gt['q'][p][t]
                rec('g', p, t, g)
                ops.gru_gate_grad_q(g, h_in, z, q, u_q=u_q[p][t], u_z=u_zr[p][t][:, :hc], sum_q=s_q[p], sum_z=s_zr[p][:, :hc],
                                    first=first)
                ops.conv_s1_dgrad(u_q[p][t], w_q_hx[p], add=add_x, out=g_q, w_scratch=w_scratch)        # [g_rh | g_x']
                rec('g_q', p, t, g_q)
                ops.gru_gate_grad_r(g, z, g_q[:, :hc], h_in, r, u_r=u_zr[p][t][:, hc:], sum_r=s_zr[p][:, hc:], first=first)
                rec('add', p, t, g_q)
                ops.conv_s1_dgrad(u_zr[p][t], w_zr_hx[p], add=g_q, out=out[t], w_scratch=w_scratch)      # [g_h | g_x']
                rec('out', p, t, out[t])
                if p > 0:          # hand g_h over to the pass in front; [0 | g_x'] stays behind as its q dgrad's `add`
                    g, add_x = ops.gru_carry(out[t][:, :hc], out=carry, clear=True), out[t]
        g_h0 = ops.gru_carry(out[0][:, :hc])
        if intermediates is not None:
            intermediates.update(u_zr=u_zr, u_q=u_q, s_zr=s_zr, s_q=s_q, gates=gt)
        # ---- the context columns, once per pass on the running sums
        g_c = None
        for p in range(P):
            g_c = ops.conv_s1_dgrad(s_zr[p], w_zr_c[p], add=g_c, w_scratch=w_scratch)
            g_c = ops.conv_s1_dgrad(s_q[p], w_q_c[p], add=g_c, w_scratch=w_scratch)
        # ---- weight gradients over the M = T N stacked samples, by column block of the raw (Cout, Ch + Cc + Cx', KH, KW)
        m = T * n
        xs = x.view(m, cx, h, w)
        ks = [tuple(z.conv.kernel_size) for z in self.conv_z]
        ws = E(max(ops.conv_s1_wgrad_workspace(mm, co, ci, h, w, *k) for k in ks for co in (2 * hc, hc)
                   for mm, ci in ((m, hc), (m, cx), (n, cc))))
        for p in range(P):
            groups = ((u_zr[p].view(m, 2 * hc, h, w), s_zr[p], gt['h_in'][p].view(m, hc, h, w), (f'conv_z.{p}.conv', f'conv_r.{p}.conv')),
                      (u_q[p].view(m, hc, h, w), s_q[p], gt['rh'][p].view(m, hc, h, w), (f'conv_q.{p}.conv',)))
            for u, s_, state, mods in groups:
                prev_w = [dst[f'{k}.weight'] for k in mods] if acc else None
                old = lambda cols: torch.cat([d[:, cols] for d in prev_w], 0).contiguous() if acc else None    # noqa: E731
                db = torch.cat([dst[f'{k}.bias'] for k in mods], 0) if acc else None
                dw_h, db = ops.conv_s1_wgrad(u, state, ks[p], dw=old(slice(0, hc)), db=db, accumulate=acc, workspace=ws)
                dw_c, _ = ops.conv_s1_wgrad(s_, c, ks[p], dw=old(slice(hc, hc + cc)), bias=False, accumulate=acc, workspace=ws)
                dw_x, _ = ops.conv_s1_wgrad(u, xs, ks[p], dw=old(slice(hc + cc, None)), bias=False, accumulate=acc, workspace=ws)
                dw = torch.cat([dw_h, dw_c, dw_x], 1)
                for i, k in enumerate(mods):
                    rows = slice(i * hc, (i + 1) * hc)
                    if acc:
                        grads[f'{k}.weight'], grads[f'{k}.bias'] = dst[f'{k}.weight'].copy_(dw[rows]), dst[f'{k}.bias'].copy_(db[rows])
                    else:
                        grads[f'{k}.weight'], grads[f'{k}.bias'] = dw[rows].contiguous(), db[rows].contiguous()
        return g_h0, g_c, [out[t][:, hc:] for t in range(T)], grads


class XHead(HipModule):
    """decoder/raft_decoder.py:256-294."""

    def __init__(self, in_channels: int, feat_channels: Sequence[int], x_channels: int, x: str):
        super().__init__()
        if len(feat_channels) != 1:
            raise NotImplementedError('XHead: one hidden layer')
        self.layers = nn.Sequential(ConvBlock(in_channels, feat_channels[0], 3, padding=1))
        k = 1 if x == 'mask' else 3
        self.predict_layer = nn.Conv2d(feat_channels[0], x_channels, k, padding=k // 2)

    def _pack(self) -> PackedConv:
        c = self.predict_layer
        return PackedConv.from_weight(c.weight, c.bias, 1, c.padding)

    def predict(self, feat: Tensor, act: int = ACT_NONE) -> Tensor:
        return ops.conv2d(self.packed, feat, act=act)

    def forward(self, x: Tensor) -> Tensor:
        return self.predict(self.layers[0](x))


def _grad_slots(what: str, names: Sequence[str], param_grads: Optional[dict]) -> Tuple[dict, list, bool]:
    """(the dict a backward writes its parameter gradients to, its entries under ``names`` -- None where absent --,
    whether they are accumulated into): a ``param_grads`` that holds ``what`` must hold all of them."""
    grads = {} if param_grads is None else param_grads
    have = [k in grads for k in names]
    if any(have) and not all(have):
        raise _lib_error(what + ' but not all')
    return grads, [grads.get(k) for k in names], all(have)


@HEAD.register_module()
class MultiClassPoseHead(HipModule):
    """head/pose_head.py:110-211."""

    def __init__(self, num_class: int, in_channels: int, net_type: str, norm_cfg: dict,
                 act_cfg: dict, feat_size: Optional[tuple] = None,
                 rotation_mode: str = 'quaternion', init_cfg=None):
        super().__init__()
        if rotation_mode != 'ortho6d':
            raise NotImplementedError('quaternion branch needs kornia in the reference and is '
                                      'not used by the SCFlow config')
        feat_size = feat_size or {'Basic': (32, 32), 'Large': (64, 64)}[net_type]
        self.num_class = num_class
        self.rotation_out_channels = 6
        convs, cin, size = [], in_channels, feat_size[0] * feat_size[1]
        for _ in range(3):
            convs.append(ConvBlock(cin, 128, 3, stride=2, padding=1, act_cfg=act_cfg,
                                   norm_cfg=norm_cfg))
            cin, size = 128, int(size / 4)
        self.conv_layers = nn.Sequential(*convs)
        self.fc_layers = nn.Sequential(nn.Sequential(nn.Linear(128 * size, 1024), nn.ReLU()),
                                       nn.Sequential(nn.Linear(1024, 256), nn.ReLU()))
        self.rotation_pred = nn.Linear(256, 6 * num_class)
        self.translation_pred = nn.Linear(256, 3 * num_class)
        # reference label selection uses label[0] for the whole batch (pose_head.py:209-210,
        # SURVEY.md 8 a8); label_mode=1 selects per sample instead (what index_select was meant to do;
        # oracle.multiclass_pose_head(label_mode=1), tests/test_gpu_refiner.py::test_label_mode_per_sample).
        self.label_mode = 0
        # fc1 / fc2 / heads as split-K MFMA GEMMs with the last GroupNorm folded in (scf_fc_splitk); False = one
        # scf_linear launch per layer after a separate GroupNorm (A/B measurements, parity tests)
        self.fused_fc = True
        self.init_weights()

    def init_weights(self):
        """pose_head.py:187-198: zero heads, identity ortho6d bias."""
        nn.init.zeros_(self.translation_pred.weight)
        nn.init.zeros_(self.translation_pred.bias)
        nn.init.zeros_(self.rotation_pred.weight)
        with torch.no_grad():
            self.rotation_pred.bias.copy_(torch.tensor([1., 0., 0., 0., 1., 0.] * self.num_class))

    def fc_plan(self) -> Tuple[int, int]:
        """(K-slices of fc1, of fc2) when the fully connected tail fits ``scf_fc_splitk`` (three launches: the last
        GroupNorm + ReLU folded into fc1's load, every weight read once per batch), else (0, 0): plain
        ``scf_linear`` launches."""
        fc1, fc2, last = self.fc_layers[0][0], self.fc_layers[1][0], self.conv_layers[2]
        s1, s2 = ops.fc_slices(fc1.in_features), ops.fc_slices(fc2.in_features)
        ok = (s1 > 0 and s2 > 0 and ops.fc_slices(fc2.out_features) == 1 and last.groups is not None
              and last.act == ACT_RELU and self.fused_fc)
        if ok:      # a K-slice of fc1 must hold whole normalisation groups
            gsz = fc1.in_features // last.groups
            ok = fc1.in_features % last.groups == 0 and gsz % 2 == 0 and (fc1.in_features // s1) % gsz == 0
        return (s1, s2) if ok else (0, 0)

    def _conv_outputs(self, x0: Tensor, x1: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor]:
        """The convolution stage, the only place that sequences the three blocks: per block ``ConvBlock.forward``'s
        K-sliced convolution, GroupNorm + ReLU between blocks.  -> the raw outputs (y0, y1, y2), each (N, 128, h', w') or
        the (S, N, 128, h', w') partial tensors of a K-sliced launch."""
        ys, x = [], x0
        for i, blk in enumerate(self.conv_layers):
            if blk.groups is None or blk.act != ACT_RELU:
                raise NotImplementedError('pose head: conv + GroupNorm + ReLU blocks')
            xb = x1 if i == 0 else None
            y = ops.conv2d(blk.packed, x, xb, kslices=ops.conv_kslices_for(blk.packed, x, xb))
            ys.append(y)
            if i < 2:
                x = ops.group_norm_relu(y, blk.gn.weight, blk.gn.bias, blk.groups, blk.gn.eps)
        return tuple(ys)

    def _tail(self, y: Tensor, activations: bool = False):
        """The fully connected stage, the only place that sequences it: the last GroupNorm + ReLU, fc1, fc2 and the two
        heads on the last convolution's raw output ``y``, (M, C, h, w) or (parts, M, C, h, w) partial tensors (a stack of
        iterations included), by ``fc_plan()``'s route.  -> (rot_all, trans_all), or with ``activations`` the operands
        (x0, a1, a2) of fc1, fc2 and the heads, in the bits the route contracts, without launching the heads."""
        last, fc1, fc2 = self.conv_layers[2], self.fc_layers[0][0], self.fc_layers[1][0]
        rot, trans = self.rotation_pred, self.translation_pred
        parts = y.shape[0] if y.dim() == 5 else 1
        m, hw = y.shape[-4], y.shape[-2] * y.shape[-1]
        feat = y.shape[-3] * hw
        if feat != fc1.in_features:
            raise _lib_error(f'pose head expects {fc1.in_features} features, the maps give {feat}')
        s1, s2 = self.fc_plan()
        if s1:
            # GroupNorm + ReLU: applied by fc1's operand load, which also adds the partial tensors of a K-sliced launch
            yv, gn = y.view(parts, m, feat), (last.groups, hw, last.gn.weight, last.gn.bias, last.gn.eps)
            x0 = ops.fc_operand(yv, gn=gn) if activations else None
            p1 = ops.fc_splitk(yv, fc1.weight, gn=gn, slices=s1)
            a1 = ops.fc_operand(p1, x_bias=fc1.bias, x_relu=True) if activations else None
            p2 = ops.fc_splitk(p1, fc2.weight, x_bias=fc1.bias, x_relu=True, slices=s2)
            if activations:
                return x0, a1, ops.fc_operand(p2, x_bias=fc2.bias, x_relu=True)
            return ops.fc_splitk(p2, rot.weight, rot.bias, x_bias=fc2.bias, x_relu=True, weight2=trans.weight,
                                 bias2=trans.bias)
        x0 = ops.group_norm_relu(y[0] if y.dim() == 5 and parts == 1 else y, last.gn.weight, last.gn.bias, last.groups,
                                 last.gn.eps).view(m, feat)
        a1 = ops.linear(x0, fc1.weight, fc1.bias, ACT_RELU)
        a2 = ops.linear(a1, fc2.weight, fc2.bias, ACT_RELU)
        return (x0, a1, a2) if activations else ops.linear_pair(a2, rot.weight, rot.bias, trans.weight, trans.bias)

    def features(self, x0: Tensor, x1: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
        """(rot_all, trans_all) of the head, whose three blocks must be convolution + GroupNorm + ReLU."""
        return self._tail(self._conv_outputs(x0, x1)[2])

    def tail_input(self, x0: Tensor, x1: Optional[Tensor] = None) -> Tensor:
        """What ``features()`` computes up to and including the last convolution: its raw output ``y`` (N, 128, h', w'), or
        the (S, N, 128, h', w') partial tensors of a K-sliced launch -- the input of the fully connected tail (GroupNorm +
        ReLU, fc1, fc2, the two heads) and all ``tail_backward`` needs of an iteration."""
        return self._conv_outputs(x0, x1)[2]

    def conv_backward(self, saved: dict, g_ys: Sequence[Tensor], param_grads: Optional[dict] = None
                      ) -> Tuple[list, list, dict]:
        """Backward of the three 3x3 / stride-2 convolutions with GroupNorms 0 and 1 for the T iterations of a pass at
        once.  ``saved``: what a forward at keep level ``'pose_head'`` or above left in ``SCFlowDecoder.kept`` (``hv``
        (T, N, 128, h, w), ``dm`` (T, N, 96, h, w), the raw convolution outputs ``y0``, ``y1`` as (S, T, N, 128, h', w')
        partial tensors); ``g_ys``: what ``tail_backward`` returns.  -> (``g_x0s``, ``g_x1s``: T tensors each, the cotangents
        at ``hv`` and at ``dm``; ``param_grads``: the gradients of ``conv_layers.{0,1,2}.conv.weight`` and
        ``conv_layers.{0,1}.gn.{weight,bias}`` summed over all T N samples, keyed as in ``named_parameters()``).  A dict
        passed in is accumulated into (entries it lacks are created; some but not all of these entries: an error).

        The activations a0, a1 -- wgrad operands and, as ``a > 0``, the ReLU masks -- are recomputed from the saved raw
        outputs by the forward's own ``scf_group_norm_relu_parts`` (one block per sample and group: the forward's bits at
        any batch).  Launches: two GroupNorm forwards, then wgrad 2, dgrad 2, GroupNorm-1 grad, wgrad 1, dgrad 1,
        GroupNorm-0 grad, wgrad 0, dgrad 0 (a wgrad is two kernels, a GroupNorm grad two), after one copy that stacks
        ``g_ys`` (none for T = 1)."""
        T = len(g_ys)
        if T == 0 or T > ops.TAIL_MAX_T:
            raise _lib_error(f'conv_backward: 1 .. {ops.TAIL_MAX_T} iterations')
        L0, L1, L2 = self.conv_layers
        for blk in (L0, L1, L2):
            c = blk.conv
            if blk.groups is None or blk.act != ACT_RELU or c.bias is not None or tuple(c.kernel_size) != (3, 3) or \
                    tuple(c.stride) != (2, 2) or tuple(c.padding) != (1, 1):
                raise _lib_error('conv_backward: 3x3 / stride-2 / pad-1 convolutions without bias, GroupNorm + ReLU')
        hv, dm, y0, y1 = _kept('conv_backward', saved, ('hv', 'dm', 'y0', 'y1'), 'pose_head')
        if hv.dim() != 5 or dm.dim() != 5 or hv.shape[0] != T or dm.shape[0] != T or hv.shape[1] != dm.shape[1] or \
                hv.shape[3:] != dm.shape[3:] or hv.shape[2] + dm.shape[2] != L0.conv.in_channels or \
                not hv.is_contiguous() or not dm.is_contiguous():
            raise _lib_error(f'conv_backward: hv / dm must be contiguous ({T}, N, C, h, w) tensors of the head\'s '
                             f'{L0.conv.in_channels} input channels')
        n, c0, h, w = hv.shape[1:]
        m = T * n
        sizes = [(h, w)]
        for _ in range(3):
            sizes.append(((sizes[-1][0] - 1) // 2 + 1, (sizes[-1][1] - 1) // 2 + 1))
        for name, y, blk, hw_ in (('y0', y0, L0, sizes[1]), ('y1', y1, L1, sizes[2])):
            if y.dim() != 6 or tuple(y.shape[1:]) != (T, n, blk.conv.out_channels) + hw_ or not y.is_contiguous():
                raise _lib_error(f'conv_backward: {name} must be a contiguous (S, {T}, {n}, {blk.conv.out_channels}, '
                                 f'{hw_[0]}, {hw_[1]}) tensor, got {tuple(y.shape)}')
        c2 = L2.conv.out_channels
        if any(tuple(g.shape) != (n, c2) + sizes[3] for g in g_ys):
            raise _lib_error(f'conv_backward: g_ys are ({n}, {c2}, {sizes[3][0]}, {sizes[3][1]}) tensors')
        names = ('conv_layers.2.conv.weight', 'conv_layers.1.gn.weight', 'conv_layers.1.gn.bias',
                 'conv_layers.1.conv.weight', 'conv_layers.0.gn.weight', 'conv_layers.0.gn.bias',
                 'conv_layers.0.conv.weight')
        grads, dst, acc = _grad_slots('conv_backward: param_grads holds some of the convolutions\' gradients', names,
                                      param_grads)

        def act(y, blk, hw_):       # the forward's launch on the stacked samples
            yv = y.view(y.shape[0], m, blk.conv.out_channels, *hw_)
            return ops.group_norm_relu(yv if y.shape[0] > 1 else yv[0], blk.gn.weight, blk.gn.bias, blk.groups, blk.gn.eps)

        a0, a1 = act(y0, L0, sizes[1]), act(y1, L1, sizes[2])
        g2 = _stacked(g_ys, m, c2, *sizes[3])
        x0, x1 = hv.view(m, c0, h, w), dm.view(m, dm.shape[2], h, w)
        need = max(ops.conv_wgrad_workspace(m, blk.conv.out_channels, blk.conv.in_channels, *hw_)
                   for blk, hw_ in zip((L0, L1, L2), sizes[1:]))
        ws = torch.empty((need,), dtype=torch.float32, device=hv.device)

        def norm_grad(g_a, y, a, blk, hw_, dgam, dbet):
            k = blk.conv.out_channels * hw_[0] * hw_[1]
            g_y, dg, db = ops.group_norm_flat_grad(g_a.view(m, k), y.view(y.shape[0], m, k), a.view(m, k), blk.gn.weight,
                                                   blk.groups, hw_[0] * hw_[1], blk.gn.eps, dgam, dbet, accumulate=acc)
            return g_y.view(m, blk.conv.out_channels, *hw_), dg, db

        dw2 = ops.conv_wgrad(g2, a1, dw=dst[0], accumulate=acc, workspace=ws)
        g_a1 = ops.conv_dgrad(g2, L2.conv.weight, sizes[2])
        g_y1, dg1, db1 = norm_grad(g_a1, y1, a1, L1, sizes[2], dst[1], dst[2])
        dw1 = ops.conv_wgrad(g_y1, a0, dw=dst[3], accumulate=acc, workspace=ws)
        g_a0 = ops.conv_dgrad(g_y1, L1.conv.weight, sizes[1])
        g_y0, dg0, db0 = norm_grad(g_a0, y0, a0, L0, sizes[1], dst[4], dst[5])
        dw0 = ops.conv_wgrad(g_y0, x0, x1, dw=dst[6], accumulate=acc, workspace=ws)
        g_hv, g_dm = ops.conv_dgrad(g_y0, L0.conv.weight, (h, w), split=c0)
        grads.update(zip(names, (dw2, dg1, db1, dw1, dg0, db0, dw0)))
        g_hv, g_dm = g_hv.view(T, n, c0, h, w), g_dm.view(T, n, dm.shape[2], h, w)
        return [g_hv[t] for t in range(T)], [g_dm[t] for t in range(T)], grads

    def tail_backward(self, ys: Sequence[Tensor], label: Tensor, g_delta_rotations: Sequence[Tensor],
                      g_delta_translations: Sequence[Tensor], label_mode: Optional[int] = None,
                      param_grads: Optional[dict] = None) -> Tuple[list, dict]:
        """Backward of the fully connected tail for the T iterations of a pass at once.  ``ys``: ``tail_input()`` of every
        iteration; ``g_delta_rotations`` (N, 6) / ``g_delta_translations`` (N, 3): the cotangents of ``forward()``'s outputs
        (what ``SCFlowDecoder.tail_backward`` returns).  -> (``g_ys``: T tensors (N, 128, h', w'), the cotangent at the last
        convolution's raw output; ``param_grads``: the gradients of ``conv_layers.2.gn``, ``fc_layers``, ``rotation_pred``
        and ``translation_pred``, summed over all T N rows, keyed as in ``named_parameters()``).  A dict passed in is
        accumulated into (entries it lacks are created).

        The ReLU masks are ``a > 0`` on the activations recomputed from ``ys`` by the route ``features()`` takes (both
        ``fused_fc`` settings, any geometry), so they are the forward's.  Shipped geometry (fused route): 12 library launches
        -- ``scf_fc_operand`` x 3 and ``scf_fc_splitk`` x 2 (the activations), ``scf_pose_select_grad``, ``scf_fc_wgrad`` x 2,
        ``scf_fc_dgrad`` x 2, ``scf_group_norm_flat_grad`` (2 kernels) -- after three copies that stack the T iterations
        (none for T = 1)."""
        T = len(ys)
        if T == 0 or T > ops.TAIL_MAX_T or len(g_delta_rotations) != T or len(g_delta_translations) != T:
            raise _lib_error(f'tail_backward: 1 .. {ops.TAIL_MAX_T} iterations with one cotangent pair each')
        last, fc1, fc2 = self.conv_layers[2], self.fc_layers[0][0], self.fc_layers[1][0]
        if last.groups is None or last.act != ACT_RELU:
            raise _lib_error('tail_backward: the last convolution is followed by GroupNorm + ReLU')
        if any(y.shape != ys[0].shape or y.dim() not in (4, 5) for y in ys):
            raise _lib_error('tail_backward: ys are the (N, C, h, w) or (S, N, C, h, w) tensors of tail_input()')
        y5 = [y if y.dim() == 5 else y.unsqueeze(0) for y in ys]
        parts, n, c, h, w = y5[0].shape
        m = T * n
        y = y5[0].contiguous() if T == 1 else torch.stack(y5, 1).view(parts, m, c, h, w)
        g_rot = g_delta_rotations[0].contiguous() if T == 1 else torch.cat(list(g_delta_rotations))
        g_trans = g_delta_translations[0].contiguous() if T == 1 else torch.cat(list(g_delta_translations))
        mode = self.label_mode if label_mode is None else label_mode
        x0, a1, a2 = self._tail(y, activations=True)
        names = ('rotation_pred.weight', 'rotation_pred.bias', 'translation_pred.weight', 'translation_pred.bias',
                 'fc_layers.1.0.weight', 'fc_layers.1.0.bias', 'fc_layers.0.0.weight', 'fc_layers.0.0.bias',
                 'conv_layers.2.gn.weight', 'conv_layers.2.gn.bias')
        grads, dst, acc = _grad_slots('tail_backward: param_grads holds some of the tail\'s gradients', names, param_grads)
        g_s2, heads = ops.pose_select_grad(g_rot, g_trans, self.rotation_pred.weight, self.translation_pred.weight, a2,
                                           label, n, mode, grads=dst[0:4] if acc else None, accumulate=acc)
        dw2, db2 = ops.fc_wgrad(g_s2, a1, dst[4], dst[5], accumulate=acc)
        g_s1 = ops.fc_dgrad(g_s2, fc2.weight, a1)
        dw1, db1 = ops.fc_wgrad(g_s1, x0, dst[6], dst[7], accumulate=acc)
        g_x0 = ops.fc_dgrad(g_s1, fc1.weight)
        g_y, dgam, dbet = ops.group_norm_flat_grad(g_x0, y.view(parts, m, c * h * w), x0, last.gn.weight, last.groups, h * w,
                                                   last.gn.eps, dst[8], dst[9], accumulate=acc)
        grads.update(zip(names, (*heads, dw2, db2, dw1, db1, dgam, dbet)))
        g_y = g_y.view(T, n, c, h, w)
        return [g_y[t] for t in range(T)], grads

    def forward(self, x: Tensor, label: Tensor) -> Tuple[Tensor, Tensor]:
        """pose_head.py:201-211 -> (delta rotation (N,6), delta translation (N,3))."""
        rot_all, trans_all = self.features(x)
        n = x.shape[0]
        eye = torch.eye(3, device=x.device).repeat(n, 1, 1)
        one = torch.ones((n, 3), device=x.device)
        d_rot, d_trans, _, _ = ops.pose_update(rot_all, trans_all, label, self.num_class, eye, one,
                                               self.label_mode)
        return d_rot, d_trans


_HEAD_PARAMS = tuple(f'{m}.{p}' for m in ('flow_pred.layers.0.conv', 'flow_pred.predict_layer', 'mask_pred.layers.0.conv',
                                          'mask_pred.predict_layer', 'delta_flow_encoder.0.conv', 'delta_flow_encoder.1.conv',
                                          'mask_encoder.0.conv', 'mask_encoder.1.conv') for p in ('weight', 'bias'))


@DECODERS.register_module()
class SCFlowDecoder(HipModule):
    """decoder/scflow_decoder.py:18-251."""
    _h_channels = {'Basic': 128, 'Small': 96}
    _cxt_channels = {'Basic': 128, 'Small': 64}

    def __init__(self, net_type: str, num_levels: int, radius: int, iters: int, detach_flow: bool,
                 detach_mask: bool, detach_pose: bool, mask_flow: bool, mask_corr: bool,
                 pose_head_cfg: dict, depth_transform: str = 'exp',
                 detach_depth_for_xy: bool = False,
                 corr_lookup_cfg: dict = dict(align_corners=True), gru_type: str = 'SeqConv',
                 feat_channels: Union[int, Sequence[int]] = 256, conv_cfg=None, norm_cfg=None,
                 act_cfg=None) -> None:
        super().__init__()
        if net_type != 'Basic':
            raise NotImplementedError("SCFlowDecoder: net_type='Basic'")
        self.mask_flow, self.mask_corr = bool(mask_flow), bool(mask_corr)      # scflow_decoder.py:199-205
        # scflow_decoder.py:192-193, 232-233: autograd only -- the forward ignores them, tail_backward reads them
        self.detach_flow, self.detach_pose = bool(detach_flow), bool(detach_pose)
        self.detach_mask = bool(detach_mask)      # scflow_decoder.py:188-190: autograd only, loss_and_motion_grads reads it
        # pose.py:137-141: 'exp' -> t_z / exp(d_z); ANY other value takes the reference's else branch t_z * (d_z + 1)
        self.depth_transform = depth_transform
        self.detach_depth_for_xy = detach_depth_for_xy      # autograd only (pose.py:142-147): tail_backward reads it
        self.net_type, self.num_levels, self.radius, self.iters = net_type, num_levels, radius, iters
        self.h_channels = self._h_channels[net_type]
        self.cxt_channels = self._cxt_channels[net_type]
        self.corr_block = CorrelationPyramid(num_levels)
        cl = dict(corr_lookup_cfg)
        cl.pop('type', None)
        cl['radius'] = radius
        self.corr_lookup = CorrLookup(**cl)
        self.encoder = MotionEncoder(num_levels, radius, net_type, conv_cfg, norm_cfg, act_cfg)
        self.gru = ConvGRU(self.h_channels, 126 + 2 + self.cxt_channels, gru_type)
        self.pose_pred = build_head(pose_head_cfg)
        fc = [256]    # scflow_decoder.py:73-74: the tuple check always yields [feat_channels]
        self.flow_pred = XHead(self.h_channels, fc, 2, x='flow')
        self.mask_pred = XHead(self.h_channels, fc, 1, x='mask')
        self.delta_flow_encoder = nn.Sequential(ConvBlock(2, 128, 7, padding=3, act_cfg=act_cfg),
                                                ConvBlock(128, 64, 3, padding=1, act_cfg=act_cfg))
        self.mask_encoder = nn.Sequential(ConvBlock(1, 64, 3, padding=1, act_cfg=act_cfg),
                                          ConvBlock(64, 32, 3, padding=1, act_cfg=act_cfg))
        self.tiled_pyramid = True     # decoder-internal pyramid layout (see _pyramid_layout)
        self.hoist_context = True     # GRU: convolve the (iteration-invariant) context channels once per pair
        # the launch sequence of an iteration issued by ONE C call (scf_scflow_iteration) instead of
        # ~33 Python-sequenced ones: same kernels, same order, same bits; False = sequence from here
        self.c_iteration = True
        # what every forward leaves in ``kept`` for the backward stages, one of KEEP_LEVELS; a level adds to the one before it:
        #   'none'           nothing is kept, allocated or launched, and ``kept`` is not touched
        #   'pose_tail'      tail_inputs: per iteration the pose head's tail input (MultiClassPoseHead.tail_input), a list
        #   'pose_head'      hv, dm (T, N, C, h, w) and the raw outputs y0, y1, y2 of the head's convolutions as
        #                    (S, T, N, 128, h', w') partial tensors (S: the K-slices of the forward's launch)
        #   'decoder_heads'  the XHeads' outputs d_flow (T, N, 2, h, w) and the post-sigmoid mask (T, N, 1, h, w)
        #   'gru'            the initial state h0 (N, Ch, h, w), the context c (N, Cc, h, w), the motion encoder's output x
        #                    (T, N, 128, h, w)
        #   'motion'         flow_lr (T, N, 2, h, w) every lookup was taken at, the pyramid (the list itself: no copy, nothing
        #                    rewrites it) and its layout mask tiled
        # copies only; a forward above 'none' replaces ``kept`` with a fresh dict of exactly its level's keys
        self.keep = 'none'
        self.kept = {}

    @contextlib.contextmanager
    def keeping(self, level: str):
        """``keep`` raised to at least ``level`` for the body (a higher setting of the caller's stays) and put back after it"""
        prev = self.keep
        self.keep = max(prev, level, key=KEEP_LEVELS.index)
        try:
            yield self
        finally:
            self.keep = prev

    def pose_flags(self) -> int:
        """the ``label_mode`` bit set of ``scf_pose_update`` (scflow_hip.h: SCF_POSE_*)."""
        return (self.pose_pred.label_mode & 1) | (0 if self.depth_transform == 'exp' else 2)

    def _pack_sources(self):
        a, b = self.flow_pred.layers[0].conv, self.mask_pred.layers[0].conv
        return [a.weight, a.bias, b.weight, b.bias]

    def _pack(self):
        # the two XHead hidden layers read the same h: one 512-row convolution
        a, b = self.flow_pred.layers[0].conv, self.mask_pred.layers[0].conv
        return PackedConv.from_weight(torch.cat([a.weight, b.weight], 0),
                                      torch.cat([a.bias, b.bias], 0), 1, 1)

    def forward(self, feat_render: Tensor, feat_real: Tensor, h_feat: Tensor, cxt_feat: Tensor,
                ref_rotation: Tensor, ref_translation: Tensor, depth: Tensor, internel_k: Tensor,
                label: Tensor, init_flow: Tensor, invalid_flow_num: float,
                _consume_state: bool = False):
        """scflow_decoder.py:150-251 (inference).  Returns the reference's 7-tuple of
        per-iteration lists."""
        if self.keep not in KEEP_LEVELS:
            raise ValueError(f'SCFlowDecoder.keep is {self.keep!r}: it must be one of KEEP_LEVELS = {KEEP_LEVELS}')
        level = KEEP_LEVELS.index(self.keep)
        hc, cc = self.h_channels, self.cxt_channels
        n, H, W = depth.shape
        scale = 2 ** (self.num_levels - 1)
        h, w = H // scale, W // scale
        dev = depth.device
        f32 = dict(dtype=torch.float32, device=dev)

        if level:
            self.kept = {'tail_inputs': []}
        tiled = _pyramid_layout(feat_render, self.radius, self.num_levels, self.tiled_pyramid)
        pyramid = self.corr_block(feat_render, feat_real, tiled_levels=tiled)      # :172
        if level >= _KEEP['motion']:
            self.kept['pyramid'], self.kept['tiled'] = pyramid, tiled
        # GRU buffer [h | cxt | motion(126) | flow(2)]: the caller's own buffer only when the
        # refiner says it may be consumed (_consume_state); the public forward never mutates
        # its inputs (the reference decoder does not either)
        hx = _as_gru_buffer(h_feat, cxt_feat, hc + cc + 128, _consume_state)
        if level >= _KEEP['gru']:      # before the first iteration rewrites h in place
            for key, part in (('h0', hx[:, :hc]), ('c', hx[:, hc:hc + cc])):
                self.kept[key] = torch.empty(part.shape, **f32).copy_(part)
        rot, trans = ref_rotation.contiguous(), ref_translation.contiguous()
        rot0, trans0 = rot, trans
        flow = init_flow
        outs = ([], [], [], [], [], [], [])
        dm = torch.empty((n, 96, h, w), **f32)
        heads = torch.empty((n, 512, h, w), **f32)
        # the context channels of hx never change: their part of the GRU convolutions, once
        ctx = self.gru.context_terms(hx[:, hc:hc + cc]) if self.hoist_context else None
        # small batches: independent branches side by side
        ov_flow, ov_mask, ov_up = (ops.small_work(n, H, W, b) for b in ('flow', 'mask', 'upsample'))
        if self.c_iteration and ops._CONV_EVENTS is None:
            return self._forward_c(level, pyramid, tiled, hx, ctx, rot0, trans0, depth, internel_k, label, init_flow,
                                   invalid_flow_num, tuple(ops.branch_mode(n, H, W, b) for b in ('flow', 'mask', 'upsample')))
        # occlusion mask of the previous iteration (ones before the first: the 1/8 bilinear
        # down-sampling of a ones map, :188-190), used only with mask_flow / mask_corr
        mask = ops.constant((n, 1, h, w), 1.0, dev) if (self.mask_flow or self.mask_corr) else None
        # scratch reused by every iteration (allocated once, before any fork point: the side branches
        # write into cf; z / rh are the GRU's gate buffers)
        cf = torch.empty((n, 256, h, w), **f32)
        zbuf = torch.empty((2, n, hc, h, w), **f32)
        for _ in range(self.iters):
            flow_lr = ops.resize_bilinear(flow, (h, w), mul=1.0 / scale)           # :196-197
            flow_in = ops.mul_mask(flow_lr, mask) if self.mask_flow else flow_lr   # :203-204
            fork = ops.fork_point() if ov_flow else None    # the motion encoder's flow branch starts here
            corr = self.corr_lookup(pyramid, flow_lr, tiled_levels=tiled)          # :198
            if self.mask_corr:
                ops.mul_mask(corr, mask, out=corr)                                 # :200-201
            self.encoder(corr, flow_in, out=hx[:, hc + cc:], overlap=ov_flow, cf=cf, fork=fork)   # :206
            hv = self.gru.forward_inplace(hx, ctx, cc, scratch=zbuf)               # :207-208
            ops.conv2d(self.packed, hv, out=heads, act=ACT_RELU)
            d_flow = self.flow_pred.predict(heads[:, :256])                        # :210
            mask = self.mask_pred.predict(heads[:, 256:], act=ACT_SIGMOID)         # :212-213
            br = ops.side_stream(ov_mask)
            with br:
                m1 = self.mask_encoder[0](mask)                                    # :217
                self.mask_encoder[1](m1, out=dm[:, 64:])
                del m1
            d1 = self.delta_flow_encoder[0](d_flow)                                # :216
            self.delta_flow_encoder[1](d1, out=dm[:, :64])
            br.join()
            # the two full-resolution outputs do not feed the pose head: side branch (outputs are
            # allocated here, on the main stream, because they escape the branch)
            flow_pred = torch.empty((n, 2, H, W), **f32)
            up_mask = torch.empty((n, 1, H, W), **f32)
            br = ops.side_stream(ov_up)
            with br:
                ops.resize_bilinear(flow_lr, (H, W), mul=float(scale), b=d_flow, out=flow_pred)  # :222-224
                ops.resize_bilinear(mask, (H, W), out=up_mask)                     # :226-227
            ys = self.pose_pred._conv_outputs(hv, dm)                              # :218-219
            self._keep_iteration(level, len(outs[0]), hv, dm, ys, d_flow=d_flow, mask=mask, xm=hx[:, hc + cc:], flow_lr=flow_lr)
            rot_all, trans_all = self.pose_pred._tail(ys[2])
            d_rot, d_trans, rot, trans = ops.pose_update(                          # :230-236
                rot_all, trans_all, label, self.pose_pred.num_class, rot, trans,
                self.pose_flags())
            flow = ops.reproject_flow(depth, internel_k, rot0, trans0, rot, trans,  # :239-243
                                      invalid_flow_num)
            br.join()
            for lst, v in zip(outs, (flow, flow_pred, rot, trans, up_mask, d_rot, d_trans)):
                lst.append(v)
        return outs

    def corr_backward(self, feat_render: Tensor, feat_real: Tensor, g_vol: Tensor,
                      out: Optional[Sequence[Optional[Tensor]]] = None) -> Tuple[Tensor, Tensor]:
        """Backward of ``forward``'s ``corr_block`` call with respect to the two feature maps (``ops.corr_build_grad``):
        ``g_vol`` is d loss / d (level 0 of the pyramid) (N h w, h, w) row-major with the pools' adjoints folded in, what
        ``motion_backward`` returns as ``correlation`` -> (d loss / d ``feat_render``, d loss / d ``feat_real``).  ``forward``
        only reads the two maps (the pyramid is built from them and nothing else touches them), so the maps of that same
        forward are the operands.  ``out``: a pair of destinations, e.g. the halves of one (2N, C, h, w) buffer."""
        return ops.corr_build_grad(g_vol, feat_render, feat_real, out=out)

    def _keep_iteration(self, level: int, t: int, hv: Tensor, dm: Tensor, ys, clone: bool = False,
                        d_flow: Optional[Tensor] = None, mask: Optional[Tensor] = None, xm: Optional[Tensor] = None,
                        flow_lr: Optional[Tensor] = None) -> None:
        """What keep level ``level`` (an index into KEEP_LEVELS) asks for of iteration ``t``, copies only; 0: nothing.  One
        walk over the rows (minimum level, key, this iteration's tensor, where the iteration axis goes): the buffer for all
        iterations is allocated at the first one.  ``xm``: the motion features (the GRU buffer's last 128 channels, rewritten
        by every iteration), kept as ``x``; ``flow_lr``: in the C loop its scratch buffer of that name; the raw convolution
        outputs ``ys`` are kept as (S, T, N, C, h', w') partial tensors.  Any level: the last of ``ys`` onto ``tail_inputs``
        -- a ``clone`` where later iterations rewrite that buffer."""
        if not level:
            return
        rows = ((_KEEP['motion'], 'flow_lr', flow_lr, 0), (_KEEP['gru'], 'x', xm, 0),
                (_KEEP['decoder_heads'], 'd_flow', d_flow, 0), (_KEEP['decoder_heads'], 'mask', mask, 0),
                (_KEEP['pose_head'], 'hv', hv, 0), (_KEEP['pose_head'], 'dm', dm, 0),
                *((_KEEP['pose_head'], f'y{i}', y if y.dim() == 5 else y.unsqueeze(0), 1) for i, y in enumerate(ys)))
        for need, key, v, axis in rows:
            if level < need:
                continue
            if t == 0:
                shape = tuple(v.shape)
                self.kept[key] = torch.empty(shape[:axis] + (self.iters,) + shape[axis:], dtype=torch.float32, device=v.device)
            self.kept[key].select(axis, t).copy_(v)
        self.kept['tail_inputs'].append(ys[2].clone() if clone else ys[2])

    def check_backward(self, depth: str) -> None:
        """refuse, before any launch, what ``backward(depth, ...)`` cannot carry: at ``'motion'`` (and the two depths of
        ``_LOSS_DEPTHS`` behind it) a configuration in which something flows from ``x_t`` back into iteration t - 1; the
        depths before it refuse nothing"""
        if _LOSS_DEPTHS.index(depth) < _LOSS_DEPTHS.index('motion'):
            return
        if not self.detach_flow:
            raise NotImplementedError('loss_and_motion_grads: detach_flow=False needs the path from flow_lr of iteration t into '
                                      'iteration t - 1 (the lookup\'s derivative with respect to its coordinates and a reverse '
                                      'scan over whole iterations), which has no backward yet')
        if (self.mask_flow or self.mask_corr) and not self.detach_mask:
            raise NotImplementedError('loss_and_motion_grads: mask_flow / mask_corr without detach_mask needs the path from the '
                                      'mask of iteration t - 1 into iteration t\'s motion encoder (a reverse scan over whole '
                                      'iterations), which has no backward yet')

    def backward(self, depth: str, outs, grads: dict, label: Tensor, ref_rotation: Tensor, ref_translation: Tensor,
                 depth_map: Tensor, internel_k: Tensor) -> dict:
        """The backward stages in order, on ``self.kept`` of the forward that returned ``outs`` (run at keep level ``depth``
        or above), down to the rung ``depth`` of ``_GRAD_DEPTHS`` (``'head'`` .. ``'motion'``): ``tail_backward``,
        ``pose_pred.tail_backward``, ``pose_pred.conv_backward``, ``heads_backward``, ``gru_backward``, ``motion_backward``.
        ``grads``: the cotangents at ``outs`` under the keys of ``SCFlowRefiner.loss_and_grads()``.  -> the gradients at the
        head outputs (``tail_backward``'s dict) with, rung by rung, ``pose_tail_inputs``, ``pose_head_inputs`` = (``g_hvs``,
        ``g_dms``), ``decoder_heads`` = dict(hidden_states, delta_flow_preds, mask_logits), ``gru`` = dict(initial_hidden,
        context, motion_features), ``motion`` = dict(correlation, flow_inputs), and ``params``: every stage's parameter
        gradients summed over the iterations, keyed as in this module's ``named_parameters()``."""
        if depth not in _GRAD_DEPTHS[2:]:
            raise ValueError(f'SCFlowDecoder.backward: depth is one of {_GRAD_DEPTHS[2:]}, got {depth!r}')
        self.check_backward(depth)
        head, kept = self.pose_pred, self.kept
        grads = self.tail_backward(outs, grads, ref_rotation, ref_translation, depth_map, internel_k)
        if depth == 'head':
            return grads
        g_ys, params = head.tail_backward(_kept('backward', kept, ('tail_inputs',), 'pose_tail')[0], label,
                                          grads['delta_rotation_preds'], grads['delta_translation_preds'])
        grads['pose_tail_inputs'] = g_ys
        grads['params'] = {'pose_pred.' + key: val for key, val in params.items()}
        if depth == 'pose_tail':
            return grads
        g_hvs, g_dms, params = head.conv_backward(kept, g_ys)
        grads['pose_head_inputs'] = (g_hvs, g_dms)
        grads['params'].update(('pose_pred.' + key, val) for key, val in params.items())
        if depth == 'pose_head':
            return grads
        g_h, g_df, g_ml, params = self.heads_backward(kept, g_hvs, g_dms, grads['delta_flow_preds'], grads['masks'])
        grads['decoder_heads'] = dict(hidden_states=g_h, delta_flow_preds=g_df, mask_logits=g_ml)
        grads['params'].update(params)
        if depth == 'decoder_heads':
            return grads
        g_h0, g_c, g_x, params = self.gru_backward(kept, g_h)
        grads['gru'] = dict(initial_hidden=g_h0, context=g_c, motion_features=g_x)
        grads['params'].update(('gru.' + key, val) for key, val in params.items())
        if depth == 'gru':
            return grads
        g_vol, g_flow_inputs, params = self.motion_backward(kept, g_x)
        grads['motion'] = dict(correlation=g_vol, flow_inputs=g_flow_inputs)
        grads['params'].update(params)
        return grads

    def tail_backward(self, outs, grads, ref_rotation: Tensor, ref_translation: Tensor, depth: Tensor,
                      internel_k: Tensor, extra_flow_lr=None):
        """Vector-Jacobian product of the parameter-free tail of every iteration (scflow_decoder.py:222-249: the x8
        up-sampling of ``flow_lr + delta_flow`` and of the mask, ``get_pose_from_delta_pose``, the pose-induced flow and,
        with ``detach_flow=False``, its 1/8 down-sampling into the next iteration).

        ``outs``: the 7-tuple ``forward`` returned.  ``grads``: cotangents under the keys of ``loss_and_grads()``
        (``sequence_flow_from_pose``, ``sequence_flow_from_pred``, ``seq_rotations``, ``seq_translations``,
        ``sequence_masks``), each a list over the iterations, each optional.  ``extra_flow_lr``: optional list of cotangents
        of ``flow_lr_i`` (N,2,h,w) from a later lookup / motion-encoder backward.  Returns the gradients at the head outputs:
        ``dict(delta_flow_preds, masks, delta_rotation_preds, delta_translation_preds)``, a list per key (``masks`` at the
        post-sigmoid map; the sigmoid's derivative belongs to the head backward).  ``detach_flow`` / ``detach_pose`` /
        ``detach_depth_for_xy`` / ``depth_transform`` are the decoder's.  Launches: one for all up-sampling adjoints, one for
        the pose scan; one more when a pose-induced flow has a cotangent, one more under ``detach_flow=False``."""
        rots, transs, d_rots, d_transs = outs[2], outs[3], outs[5], outs[6]
        T = len(rots)
        n, H, W = depth.shape
        scale = 2 ** (self.num_levels - 1)
        h, w = H // scale, W // scale
        seq = lambda key: None if grads.get(key) is None else list(grads[key])       # noqa: E731
        g_fpose, g_fpred, g_mask = seq('sequence_flow_from_pose'), seq('sequence_flow_from_pred'), seq('sequence_masks')
        for name, s_ in (('sequence_flow_from_pose', g_fpose), ('sequence_flow_from_pred', g_fpred), ('sequence_masks', g_mask),
                         ('extra_flow_lr', extra_flow_lr)):
            if s_ is not None and len(s_) != T:
                raise ValueError(f'tail_backward: {name} has {len(s_)} entries for {T} iterations')
        dev = depth.device
        zeros = lambda *shape: torch.zeros((T,) + shape, dtype=torch.float32, device=dev).unbind(0)   # noqa: E731
        if g_mask is not None:
            g_mask = [m.view(n, 1, H, W) for m in g_mask]
        # ---- up-sampling adjoints: g_delta_flow_i = scale U^T g_flow_pred_i, g_mask_i = U^T g_up_mask_i, one launch
        if g_fpred is not None and g_mask is not None:
            g_dflow, g_m = ops.resize_bilinear_grad(g_fpred, (h, w), mul=float(scale), second=(g_mask, 1.0))
        elif g_fpred is not None:
            g_dflow, g_m = ops.resize_bilinear_grad(g_fpred, (h, w), mul=float(scale)), list(zeros(n, 1, h, w))
        elif g_mask is not None:
            g_dflow, g_m = list(zeros(n, 2, h, w)), ops.resize_bilinear_grad(g_mask, (h, w))
        else:
            g_dflow, g_m = list(zeros(n, 2, h, w)), list(zeros(n, 1, h, w))
        # ---- detach_flow=False: flow_lr_i = D(flow_from_pose_{i-1}) / scale, so g_flow_from_pose_{i-1} += D^T (g_flow_lr_i)
        # / scale
        if not self.detach_flow and T > 1 and (g_fpred is not None or extra_flow_lr is not None):
            src = g_dflow[1:]
            add = None if extra_flow_lr is None else list(extra_flow_lr[1:])
            if g_fpred is None:                       # only the caller's cotangents of flow_lr
                src, add = [e if e is not None else z for e, z in zip(add, g_dflow[1:])], None
            if g_fpose is None:
                g_fpose = ops.resize_bilinear_grad(src, (H, W), mul=1.0 / scale, add=add) + [None]
            else:                                     # the caller's cotangents are not written: accumulate into copies
                acc = [g.clone() for g in g_fpose[:-1]]
                ops.resize_bilinear_grad(src, (H, W), mul=1.0 / scale, add=add, out=acc, accumulate=True)
                g_fpose = acc + [g_fpose[-1]]
        # ---- re-projection sums of every iteration, one launch
        sums = None
        if g_fpose is not None:
            sums = ops.reproject_flow_grad(g_fpose, depth, internel_k, ref_rotation.contiguous(), ref_translation.contiguous(),
                                           rots, transs)
        # ---- combine + reverse scan over the pose updates, one launch
        g_drot, g_dtrans = ops.pose_update_grad(d_rots, d_transs, ref_rotation.contiguous(), ref_translation.contiguous(), rots,
                                                transs, g_rots=seq('seq_rotations'), g_transs=seq('seq_translations'),
                                                reproject_sums=sums, image_hw=(H, W), detach_pose=self.detach_pose,
                                                detach_depth_for_xy=self.detach_depth_for_xy, label_mode=self.pose_flags())
        return dict(delta_flow_preds=g_dflow, masks=g_m, delta_rotation_preds=g_drot, delta_translation_preds=g_dtrans)

    def heads_backward(self, saved: dict, g_hvs: Sequence[Tensor], g_dms: Sequence[Tensor],
                       g_delta_flows: Sequence[Tensor], g_masks: Sequence[Tensor], param_grads: Optional[dict] = None):
        """Backward of the two XHeads and the delta-flow / mask encoders (scflow_decoder.py:210-217: seven stride-1
        convolutions with bias) for the T iterations of a pass at once, M = T N stacked samples, one launch per stage.

        ``saved``: what a forward at keep level ``'decoder_heads'`` or above left in ``kept`` (``hv`` (T, N, 128, h, w), ``dm``
        (T, N, 96, h, w), ``d_flow`` (T, N, 2, h, w), the post-sigmoid ``mask`` (T, N, 1, h, w)).  ``g_hvs``, ``g_dms``: the
        cotangents at ``hv`` and ``dm`` that ``MultiClassPoseHead.conv_backward`` returns; ``g_delta_flows``, ``g_masks``: those
        at ``d_flow`` and at the post-sigmoid mask that ``tail_backward`` returns.  -> (``g_hidden_states``: the cotangents at
        ``hv`` through iteration t's own heads, encoders and pose head; ``g_delta_flow_totals``: the complete cotangents at
        ``d_flow``; ``g_mask_logits``: those at the mask head's pre-sigmoid output; T tensors each; ``param_grads``: the
        gradients of the 16 parameters summed over all T N samples, keyed as in ``named_parameters()``).  A dict passed in
        is accumulated into (entries it lacks are created; some but not all of these entries: an error).

        The hidden activations -- ``heads`` (512 channels), ``d1`` (128), ``m1`` (64): wgrad operands and activation masks --
        are recomputed into stacked buffers by the forward's OWN launches, one iteration at a time at the forward's batch,
        so dispatch and bits are the forward's.  Chain per stacked sample: act_grad on ``g_dm``; wgrad + dgrad of the
        encoders' last layers; wgrad of their first layers and dgrad with the tail's cotangents added (the mask's with the
        sigmoid factor); wgrad of the predict layers and their dgrads into the two halves of one (M, 512, h, w) tensor
        with the ReLU mask of ``heads``; wgrad and dgrad of the packed hidden layer with ``g_hv`` added."""
        what = 'heads_backward'
        T = len(g_hvs)
        if T == 0 or T > ops.TAIL_MAX_T or any(len(s_) != T for s_ in (g_dms, g_delta_flows, g_masks)):
            raise _lib_error(f'{what}: 1 .. {ops.TAIL_MAX_T} iterations with one cotangent of each kind per iteration')
        hv, dm, d_flow, mask = _kept(what, saved, ('hv', 'dm', 'd_flow', 'mask'), 'decoder_heads')
        if hv.dim() != 5 or hv.shape[0] != T or not hv.is_contiguous():
            raise _lib_error(f'{what}: hv must be a contiguous ({T}, N, C, h, w) tensor, got {tuple(hv.shape)}')
        n, hc, h, w = hv.shape[1:]
        fp, mp, de, me = self.flow_pred, self.mask_pred, self.delta_flow_encoder, self.mask_encoder
        ch = fp.layers[0].conv.out_channels                     # 256: the flow head's rows of the packed hidden layer
        c_h = ch + mp.layers[0].conv.out_channels
        c_d1, c_df, c_m1, c_mf = (b.conv.out_channels for b in (de[0], de[1], me[0], me[1]))
        for name, t_, c in (('dm', dm, c_df + c_mf), ('d_flow', d_flow, 2), ('mask', mask, 1)):
            if tuple(t_.shape) != (T, n, c, h, w) or not t_.is_contiguous():
                raise _lib_error(f'{what}: {name} must be a contiguous {(T, n, c, h, w)} tensor, got {tuple(t_.shape)}')
        for name, seq, c in (('g_hvs', g_hvs, hc), ('g_dms', g_dms, c_df + c_mf), ('g_delta_flows', g_delta_flows, 2),
                             ('g_masks', g_masks, 1)):
            if any(tuple(g.shape) != (n, c, h, w) for g in seq):
                raise _lib_error(f'{what}: {name} are {(n, c, h, w)} tensors')
        enc_act = de[0].act
        if any(b.act != enc_act for b in (de[1], me[0], me[1])) or enc_act not in (ACT_NONE, ACT_RELU):
            raise NotImplementedError('heads_backward: encoders with ReLU or no activation')
        grads, dst, acc = _grad_slots(f'{what}: param_grads holds some of the heads\' and encoders\' gradients', _HEAD_PARAMS,
                                      param_grads)
        dst = dict(zip(_HEAD_PARAMS, dst))
        m = T * n
        f32 = dict(dtype=torch.float32, device=hv.device)
        E = lambda *shape: torch.empty(shape, **f32)       # noqa: E731
        # ---- the forward's own launches, an iteration at a time: heads, d1, m1 in the forward's bits
        heads, d1, m1 = E(T, n, c_h, h, w), E(T, n, c_d1, h, w), E(T, n, c_m1, h, w)
        for t in range(T):
            ops.conv2d(self.packed, hv[t], out=heads[t], act=ACT_RELU)
            de[0](d_flow[t], out=d1[t])
            me[0](mask[t], out=m1[t])
        g_hv, g_dm, g_df, g_mk = (_stacked(seq, m, c, h, w) for seq, c in ((g_hvs, hc), (g_dms, c_df + c_mf), (g_delta_flows, 2),
                                                                          (g_masks, 1)))
        hv_, dm_, df_, mk_ = hv.view(m, hc, h, w), dm.view(m, c_df + c_mf, h, w), d_flow.view(m, 2, h, w), mask.view(m, 1, h, w)
        heads_, d1_, m1_ = heads.view(m, c_h, h, w), d1.view(m, c_d1, h, w), m1.view(m, c_m1, h, w)
        layers = ((c_df, c_d1, de[1].conv), (c_mf, c_m1, me[1].conv), (c_d1, 2, de[0].conv), (c_m1, 1, me[0].conv),
                  (2, ch, fp.predict_layer), (1, c_h - ch, mp.predict_layer), (c_h, hc, None))
        ks = lambda conv: (3, 3) if conv is None else tuple(conv.kernel_size)      # noqa: E731
        ws = E(max(ops.conv_s1_wgrad_workspace(m, co, ci, h, w, *ks(cv)) for co, ci, cv in layers))
        a_or_none = lambda a: a if enc_act != ACT_NONE else None                    # noqa: E731
        wgrad = partial(_layer_wgrad, grads, dst, acc, ws)
        # 1. encoders, last layers
        u = ops.act_grad(g_dm, a_or_none(dm_), enc_act)
        u_df, u_mf = u[:, :c_df], u[:, c_df:]
        wgrad('delta_flow_encoder.1.conv', u_df, d1_, de[1].conv)
        g_d1 = ops.conv_s1_dgrad(u_df, de[1].conv.weight, a=a_or_none(d1_), act=enc_act)
        wgrad('mask_encoder.1.conv', u_mf, m1_, me[1].conv)
        g_m1 = ops.conv_s1_dgrad(u_mf, me[1].conv.weight, a=a_or_none(m1_), act=enc_act)
        # 2. encoders, first layers: the tail's cotangents join here
        wgrad('delta_flow_encoder.0.conv', g_d1, df_, de[0].conv)
        g_df_total = ops.conv_s1_dgrad(g_d1, de[0].conv.weight, add=g_df)
        wgrad('mask_encoder.0.conv', g_m1, mk_, me[0].conv)
        g_logit = ops.conv_s1_dgrad(g_m1, me[0].conv.weight, add=g_mk, a=mk_, act=ACT_SIGMOID)
        del g_d1, g_m1, u
        # 3. predict layers: their dgrads write the two halves of one tensor, ReLU mask of heads in the epilogue
        wgrad('flow_pred.predict_layer', g_df_total, heads_[:, :ch], fp.predict_layer)
        wgrad('mask_pred.predict_layer', g_logit, heads_[:, ch:], mp.predict_layer)
        g_heads = E(m, c_h, h, w)
        ops.conv_s1_dgrad(g_df_total, fp.predict_layer.weight, a=heads_[:, :ch], act=ACT_RELU, out=g_heads[:, :ch])
        ops.conv_s1_dgrad(g_logit, mp.predict_layer.weight, a=heads_[:, ch:], act=ACT_RELU, out=g_heads[:, ch:])
        # 4. the packed hidden layer: rows :ch are the flow head's, the rest the mask head's
        a_, b_ = fp.layers[0].conv, mp.layers[0].conv
        w_hidden = torch.cat([a_.weight, b_.weight], 0)
        names_h = ('flow_pred.layers.0.conv', 'mask_pred.layers.0.conv')
        dw_h = torch.cat([dst[f'{k}.weight'] for k in names_h], 0) if acc else None      # the kernel adds the previous value LAST
        db_h = torch.cat([dst[f'{k}.bias'] for k in names_h], 0) if acc else None
        dw_h, db_h = ops.conv_s1_wgrad(g_heads, hv_, (3, 3), dw=dw_h, db=db_h, accumulate=acc, workspace=ws)
        for name, rows in zip(names_h, (slice(0, ch), slice(ch, c_h))):
            kw, kb = f'{name}.weight', f'{name}.bias'
            if acc:
                grads[kw], grads[kb] = dst[kw].copy_(dw_h[rows]), dst[kb].copy_(db_h[rows])
            else:
                grads[kw], grads[kb] = dw_h[rows].contiguous(), db_h[rows].contiguous()
        g_hidden = ops.conv_s1_dgrad(g_heads, w_hidden, add=g_hv, w_scratch=E(w_hidden.numel()))
        g_hidden, g_df_total, g_logit = g_hidden.view(T, n, hc, h, w), g_df_total.view(T, n, 2, h, w), g_logit.view(T, n, 1, h, w)
        return ([g_hidden[t] for t in range(T)], [g_df_total[t] for t in range(T)], [g_logit[t] for t in range(T)], grads)

    def gru_backward(self, saved: dict, g_hidden_states: Sequence[Tensor], param_grads: Optional[dict] = None):
        """``ConvGRU.backward`` of ``self.gru`` on what a forward at keep level ``'gru'`` or above left in ``kept``, with
        the decoder's channel split checked (``c``: ``cxt_channels``, ``x``: the motion encoder's 126 + 2) -> (``g_h0``,
        ``g_context``, ``g_motion_features``, ``param_grads``), the parameter names relative to ``self.gru``."""
        what = 'gru_backward'
        c, x = _kept(what, saved, ('c', 'x'), 'gru')
        want = (self.cxt_channels, self.gru.x_channels - self.cxt_channels)
        if c.dim() != 4 or x.dim() != 5 or (c.shape[1], x.shape[2]) != want:
            raise _lib_error(f'{what}: c and x must hold {want[0]} and {want[1]} channels, got {tuple(c.shape)} and '
                             f'{tuple(x.shape)}')
        return self.gru.backward(saved, g_hidden_states, param_grads)

    def motion_backward(self, saved: dict, g_motion_features: Sequence[Tensor], param_grads: Optional[dict] = None,
                        intermediates: Optional[dict] = None):
        """Backward of the motion encoder and of the correlation lookup with respect to the pyramid (scflow_decoder.py:196-206)
        for the T iterations of a pass at once.

        ``saved``: what a forward at keep level ``'motion'`` left in ``kept``: ``x`` (T, N, 128, h, w), ``flow_lr``
        (T, N, 2, h, w), the ``pyramid`` list with its layout mask ``tiled`` and, under ``mask_corr``, ``mask`` (T, N, 1, h, w).
        ``g_motion_features``: the T cotangents at ``x_t`` that ``gru_backward`` returns.  -> (``g_vol`` (N h w, h, w): d loss / d
        level 0 of the correlation pyramid, summed over the iterations, the pooling adjoints of the other levels folded in;
        ``g_flow_inputs``: T cotangents at the encoder's flow input (``flow_lr``, times the previous mask under ``mask_flow``) --
        where a backward through the flow recurrence (``detach_flow=False``) would start; ``param_grads``: the ten
        ``encoder.*`` gradients summed over all T N samples, keyed as in ``named_parameters()``; a dict passed in is accumulated
        into, a partial one is an error).

        ``corr_t`` is recomputed by the forward's own lookup launch on the kept pyramid (and ``mul_mask`` under ``mask_corr``),
        then ``MotionEncoder.backward``, then ``ops.corr_lookup_grad`` on the stacked ``g_corr`` (with the previous iteration's
        mask -- ones before the first -- as its per-query factor under ``mask_corr``: the product's adjoint under
        ``detach_mask``).  The lookup's derivative with respect to its coordinates is NOT taken: under ``detach_flow`` nothing
        reads it."""
        what = 'motion_backward'
        T = len(g_motion_features)
        if T == 0 or T > ops.TAIL_MAX_T:
            raise _lib_error(f'{what}: 1 .. {ops.TAIL_MAX_T} iterations with one cotangent at x per iteration')
        x, flow_lr, pyramid, tiled = _kept(what, saved, ('x', 'flow_lr', 'pyramid', 'tiled'), 'motion')
        mask = _kept(what, saved, ('mask',), 'motion')[0] if self.mask_corr else None
        if x.dim() != 5 or x.shape[0] != T or not x.is_contiguous():
            raise _lib_error(f'{what}: x must be a contiguous ({T}, N, 128, h, w) tensor, got {tuple(x.shape)}')
        n, _, h, w = x.shape[1:]
        if tuple(flow_lr.shape) != (T, n, 2, h, w) or not flow_lr.is_contiguous():
            raise _lib_error(f'{what}: flow_lr must be a contiguous {(T, n, 2, h, w)} tensor, got {tuple(flow_lr.shape)}')
        if len(pyramid) != self.num_levels:
            raise _lib_error(f'{what}: the pyramid has {len(pyramid)} levels, the decoder {self.num_levels}')
        kch = self.num_levels * (2 * self.radius + 1) ** 2
        corr = torch.empty((T, n, kch, h, w), dtype=torch.float32, device=x.device)
        mask_prev = None
        if self.mask_corr:
            if tuple(mask.shape) != (T, n, 1, h, w) or not mask.is_contiguous():
                raise _lib_error(f'{what}: mask must be a contiguous {(T, n, 1, h, w)} tensor, got {tuple(mask.shape)}')
            mask_prev = torch.cat([torch.ones_like(mask[:1]), mask[:-1]], 0)
        for t in range(T):
            ops.corr_lookup(pyramid, flow_lr[t], self.radius, out=corr[t], tiled_levels=tiled)
            if self.mask_corr:
                ops.mul_mask(corr[t], mask_prev[t], out=corr[t])
        g_corr, g_flow_inputs, grads = self.encoder.backward(dict(corr=corr, x=x), g_motion_features, param_grads, intermediates,
                                                             prefix='encoder.')
        g_vol = ops.corr_lookup_grad(g_corr, flow_lr, mask_prev, self.radius, self.num_levels)
        if intermediates is not None:
            intermediates.update(corr=corr, mask_prev=mask_prev)
        return g_vol, g_flow_inputs, grads


def _scflow_forward_c(self, level, pyramid, tiled, hx, ctx, rot0, trans0, depth, internel_k, label, init_flow,
                      invalid_flow_num, overlap):
    """the refinement loop through ``scf_scflow_iteration``: every scratch buffer and convolution
    descriptor of an iteration is set up ONCE per pass; an iteration is then a handful of pointer
    updates and one C call.  Mirrors ``SCFlowDecoder.forward``'s Python-sequenced loop launch for
    launch (``tests/test_gpu_refiner.py::test_c_iteration_is_bit_identical``)."""
    from ._lib import ScflowIter
    import ctypes as C
    hc, cc = self.h_channels, self.cxt_channels
    n, H, W = depth.shape
    scale = 2 ** (self.num_levels - 1)
    h, w = H // scale, W // scale
    f32 = dict(dtype=torch.float32, device=depth.device)
    iters = self.iters
    E = lambda *shape: torch.empty(shape, **f32)
    enc, ph = self.encoder, self.pose_pred
    kch = self.num_levels * (2 * self.radius + 1) ** 2
    # ---- scratch of one iteration (reused by all of them) ----
    flow_lr, flow_m, corr = E(n, 2, h, w), (E(n, 2, h, w) if self.mask_flow else None), E(n, kch, h, w)
    f1, c1, cf = E(n, 128, h, w), E(n, 256, h, w), E(n, 256, h, w)
    zbuf, heads, dm = E(2, n, hc, h, w), E(n, 512, h, w), E(n, 96, h, w)
    d_flow, mask, m1, d1 = E(n, 2, h, w), E(n, 1, h, w), E(n, 64, h, w), E(n, 128, h, w)
    ones = ops.constant((n, 1, h, w), 1.0, depth.device) if (self.mask_flow or self.mask_corr) else None
    hv, xm = hx[:, :hc], hx[:, hc + cc:]
    # ---- outputs of all iterations: one buffer per kind, a view per iteration ----
    flows, fpreds, masks = E(iters, n, 2, H, W), E(iters, n, 2, H, W), E(iters, n, 1, H, W)
    rots, transs, drots, dtranss = E(iters, n, 3, 3), E(iters, n, 3), E(iters, n, 6), E(iters, n, 3)
    it = ScflowIter()
    it.struct_size = C.sizeof(ScflowIter)
    it.N, it.H, it.W, it.h, it.w = n, H, W, h, w
    it.L, it.radius, it.tiled_levels, it.corr_channels = len(pyramid), self.radius, int(tiled), kch
    for l, lv in enumerate(pyramid):
        it.levels[l] = lv.data_ptr()
    it.flow_lr, it.corr = flow_lr.data_ptr(), corr.data_ptr()
    it.mask_flow, it.mask_corr = int(self.mask_flow), int(self.mask_corr)
    it.flow_masked = None if flow_m is None else flow_m.data_ptr()
    keep = [pyramid, flow_lr, flow_m, corr, f1, c1, cf, zbuf, heads, dm, d_flow, mask, m1, d1, ones, hx, ctx]
    cd = lambda blk, *a, **k: ops.conv_desc(blk.packed, *a, act=blk.act, **k)[0]
    it.flow0 = cd(enc.flow_net[0], flow_lr, out=f1)
    it.flow1 = cd(enc.flow_net[1], f1, out=cf[:, 192:])
    it.corr0 = cd(enc.corr_net[0], corr, out=c1)
    it.corr1 = cd(enc.corr_net[1], c1, out=cf[:, :192])
    it.outn = cd(enc.out_net[0], cf, out=xm[:, :126])
    it.flow_copy_dst = xm[:, 126:128].data_ptr()
    it.hx, it.hx_nstride = hx.data_ptr(), hx.stride(0)
    it.Ch, it.Cc, it.Cx = hc, cc, hx.shape[1] - hc - cc
    if ctx is not None:
        packs = [(pk[1], pk[2]) for pk in self.gru._ctx_packs(cc)]
        for i, t in enumerate(ctx):
            it.ctx[i] = t.data_ptr()
        it.ctx_nstride = ctx[0].stride(0)
    else:
        packs = self.gru.packed
    arr = ops.gru_passes(packs)
    it.npass = len(packs)
    for i in range(len(packs)):
        it.gru[i] = arr[i]
    it.z, it.rh = zbuf[0].data_ptr(), zbuf[1].data_ptr()
    it.heads = ops.conv_desc(self.packed, hv, out=heads, act=ACT_RELU)[0]
    it.fpred = ops.conv_desc(self.flow_pred.packed, heads[:, :256], out=d_flow)[0]
    it.mpred = ops.conv_desc(self.mask_pred.packed, heads[:, 256:], out=mask, act=ACT_SIGMOID)[0]
    it.menc0 = cd(self.mask_encoder[0], mask, out=m1)
    it.menc1 = cd(self.mask_encoder[1], m1, out=dm[:, 64:])
    it.denc0 = cd(self.delta_flow_encoder[0], d_flow, out=d1)
    it.denc1 = cd(self.delta_flow_encoder[1], d1, out=dm[:, :64])
    # ---- pose head ----
    x0, x1 = hv, dm
    raw_ys = []                     # the raw outputs of the head's convolutions: rewritten by every iteration
    for i, blk in enumerate(ph.conv_layers):
        if blk.groups is None or blk.act != ACT_RELU:
            raise NotImplementedError('pose head: conv + GroupNorm + ReLU blocks')
        ks = ops.conv_kslices_for(blk.packed, x0, x1)
        d_, y = ops.conv_desc(blk.packed, x0, x1, kslices=ks)       # ks > 1: (ks, N, C, h, w) partial tensors
        g = torch.empty_like(y[0] if ks > 1 else y)
        it.pose[i] = d_
        it.gn[i].gamma, it.gn[i].beta, it.gn[i].out = blk.gn.weight.data_ptr(), blk.gn.bias.data_ptr(), g.data_ptr()
        it.gn[i].C, it.gn[i].HW, it.gn[i].G, it.gn[i].eps = y.shape[-3], y.shape[-2] * y.shape[-1], blk.groups, blk.gn.eps
        keep += [y, g]
        raw_ys.append(y)
        x0, x1 = g, None
    fc1, fc2 = ph.fc_layers[0][0], ph.fc_layers[1][0]
    if fc1.in_features != x0[0].numel():
        raise _lib_error(f'pose head expects {fc1.in_features} features, the maps give {x0[0].numel()}')
    s1, s2 = ph.fc_plan()
    it.fc_fused, it.fc1_slices, it.fc2_slices = int(s1 > 0), max(s1, 1), max(s2, 1)
    y1, y2 = E(max(s1, 1), n, fc1.out_features), E(max(s2, 1), n, fc2.out_features)
    ra, ta = E(n, ph.rotation_pred.out_features), E(n, ph.translation_pred.out_features)
    keep += [y1, y2, ra, ta]
    P = lambda t: None if t is None else t.data_ptr()
    it.fc1_w, it.fc1_b, it.fc1_out, it.fc1_K, it.fc1_O = P(fc1.weight), P(fc1.bias), y1.data_ptr(), fc1.in_features, fc1.out_features
    it.fc2_w, it.fc2_b, it.fc2_out, it.fc2_O = P(fc2.weight), P(fc2.bias), y2.data_ptr(), fc2.out_features
    it.rot_w, it.rot_b, it.rot_all, it.rot_O = P(ph.rotation_pred.weight), P(ph.rotation_pred.bias), ra.data_ptr(), ra.shape[1]
    it.trans_w, it.trans_b, it.trans_all, it.trans_O = (P(ph.translation_pred.weight), P(ph.translation_pred.bias),
                                                        ta.data_ptr(), ta.shape[1])
    if not label.is_cuda or label.dtype != torch.int64 or not label.is_contiguous():
        raise _lib_error('label must be a contiguous int64 GPU tensor')
    it.label, it.num_class, it.label_mode = label.data_ptr(), ph.num_class, self.pose_flags()
    for name, t in (('depth', depth), ('internel_k', internel_k), ('ref_rotation', rot0), ('ref_translation', trans0),
                    ('init_flow', init_flow)):
        ops._dense(t, name)
    it.depth, it.K, it.R0, it.t0 = depth.data_ptr(), internel_k.data_ptr(), rot0.data_ptr(), trans0.data_ptr()
    it.invalid_flow_num = float(invalid_flow_num)
    it.overlap_flow, it.overlap_mask, it.overlap_up = (int(b) for b in overlap)      # 0 in order / 1 side stream / 2 merged launches
    it.side_stream = ops.side_stream_handle() if any(int(b) == 1 for b in overlap) else None
    outs = ([], [], [], [], [], [], [])
    flow, rot, trans = init_flow, rot0, trans0
    for i in range(iters):
        it.flow_in, it.R_in, it.t_in = flow.data_ptr(), rot.data_ptr(), trans.data_ptr()
        it.mask_prev = None if ones is None else (ones if i == 0 else mask).data_ptr()
        flow, rot, trans = flows[i], rots[i], transs[i]
        it.flow_out, it.flow_pred, it.mask_up = flow.data_ptr(), fpreds[i].data_ptr(), masks[i].data_ptr()
        it.R_out, it.t_out, it.d_rot, it.d_trans = rot.data_ptr(), trans.data_ptr(), drots[i].data_ptr(), dtranss[i].data_ptr()
        ops.scflow_iteration(it)
        self._keep_iteration(level, i, hv, dm, raw_ys, clone=True, d_flow=d_flow, mask=mask, xm=xm, flow_lr=flow_lr)
        for lst, v in zip(outs, (flow, fpreds[i], rot, trans, masks[i], drots[i], dtranss[i])):
            lst.append(v)
    if any(overlap):          # the scratch is freed on return: the side stream's last reads are joined already
        pass
    del keep
    return outs


SCFlowDecoder._forward_c = _scflow_forward_c


class _RAFTDecoderBase(HipModule):
    """shared part of RAFTDecoder / RAFTDecoderMask ('Basic'): correlation pyramid, lookup,
    motion encoder, SepConvGRU, flow head, 576-channel convex-up-sampling mask head."""
    _h_channels = {'Basic': 128, 'Small': 96}
    _cxt_channels = {'Basic': 128, 'Small': 64}

    def __init__(self, net_type: str, num_levels: int, radius: int, iters: int,
                 corr_lookup_cfg: dict = dict(type='CorrLookup', align_corners=True),
                 gru_type: str = 'SeqConv', feat_channels: Union[int, Sequence[int]] = 256,
                 mask_channels: int = 64, convex_unsample_flow: bool = True, conv_cfg=None,
                 norm_cfg=None, act_cfg=None) -> None:
        super().__init__()
        if net_type != 'Basic':
            raise NotImplementedError("RAFT decoders: net_type='Basic'")
        self.net_type, self.num_levels, self.radius, self.iters = net_type, num_levels, radius, iters
        self.h_channels = self._h_channels[net_type]
        self.cxt_channels = self._cxt_channels[net_type]
        self.mask_channels = mask_channels * (2 * radius + 1)      # raft_decoder.py:355
        self.corr_block = CorrelationPyramid(num_levels)
        cl = dict(corr_lookup_cfg)
        cl.pop('type', None)
        cl['radius'] = radius
        self.corr_lookup = CorrLookup(**cl)
        self.encoder = MotionEncoder(num_levels, radius, net_type, conv_cfg, norm_cfg, act_cfg)
        self.gru = ConvGRU(self.h_channels, 126 + 2 + self.cxt_channels, gru_type)
        self.flow_pred = XHead(self.h_channels, [256], 2, x='flow')
        self.mask_pred = XHead(self.h_channels, [256], self.mask_channels, x='mask')
        self.convex_upsample_flow = convex_unsample_flow
        self.tiled_pyramid = True     # decoder-internal pyramid layout (see _pyramid_layout)
        self.hoist_context = True     # GRU: convolve the (iteration-invariant) context channels once per pair
        if self.mask_channels != 9 * (2 ** (num_levels - 1)) ** 2:
            raise NotImplementedError('convex up-sampling kernel: 9 x 8 x 8 mask (radius 4, 4 levels)')

    def _context(self, hx):
        hc, cc = self.h_channels, self.cxt_channels
        return self.gru.context_terms(hx[:, hc:hc + cc]) if self.hoist_context else None

    def _step(self, pyramid, flow, hx, tiled=0, ctx=None):
        """one update: lookup, motion encoder, GRU (in place in hx), flow += delta."""
        hc, cc = self.h_channels, self.cxt_channels
        corr = self.corr_lookup(pyramid, flow, tiled_levels=tiled)
        self.encoder(corr, flow, out=hx[:, hc + cc:])
        hv = self.gru.forward_inplace(hx, ctx, cc)
        d_flow = self.flow_pred(hv)
        n, _, h, w = flow.shape
        return hv, ops.resize_bilinear(flow, (h, w), b=d_flow)       # flow + delta (same size)

    def _upsample(self, x: Tensor, mask: Optional[Tensor], mul: float) -> Tensor:
        scale = 2 ** (self.num_levels - 1)
        n, c, h, w = x.shape
        if mask is None:                         # raft_decoder.py:397-400
            return ops.resize_bilinear(x, (scale * h, scale * w), mul=mul)
        return ops.convex_upsample(x, mask, scale, x_mul=mul, mask_mul=0.25)


@DECODERS.register_module()
class RAFTDecoder(_RAFTDecoderBase):
    """decoder/raft_decoder.py:299-457."""

    def forward(self, feat1: Tensor, feat2: Tensor, flow: Tensor, h_feat: Tensor,
                cxt_feat: Tensor, _consume_state: bool = False) -> List[Tensor]:
        tiled = _pyramid_layout(feat1, self.radius, self.num_levels, self.tiled_pyramid)
        pyramid = self.corr_block(feat1, feat2, tiled_levels=tiled)
        hx = _as_gru_buffer(h_feat, cxt_feat, self.h_channels + self.cxt_channels + 128,
                            _consume_state)
        scale = float(2 ** (self.num_levels - 1))
        flow = flow.contiguous()
        outs = []
        ctx = self._context(hx)
        for _ in range(self.iters):
            hv, flow = self._step(pyramid, flow, hx, tiled, ctx)
            mask = self.mask_pred(hv) if self.convex_upsample_flow else None   # 0.25 folded in
            outs.append(self._upsample(flow, mask, scale))
        return outs


@DECODERS.register_module()
class RAFTDecoderMask(_RAFTDecoderBase):
    """decoder/raft_decoder_mask.py:21-208: RAFTDecoder + occlusion head."""

    def __init__(self, *args, **kwargs) -> None:
        super().__init__(*args, **kwargs)
        self.occlusion_pred = XHead(self.h_channels, [256], 1, x='mask')

    def forward(self, feat1: Tensor, feat2: Tensor, flow: Tensor, h_feat: Tensor,
                cxt_feat: Tensor, _consume_state: bool = False):
        tiled = _pyramid_layout(feat1, self.radius, self.num_levels, self.tiled_pyramid)
        pyramid = self.corr_block(feat1, feat2, tiled_levels=tiled)
        hx = _as_gru_buffer(h_feat, cxt_feat, self.h_channels + self.cxt_channels + 128,
                            _consume_state)
        scale = float(2 ** (self.num_levels - 1))
        flow = flow.contiguous()
        flows, occs = [], []
        ctx = self._context(hx)
        for _ in range(self.iters):
            hv, flow = self._step(pyramid, flow, hx, tiled, ctx)
            occ = self.occlusion_pred.predict(self.occlusion_pred.layers[0](hv), act=ACT_SIGMOID)
            mask = self.mask_pred(hv) if self.convex_upsample_flow else None
            flows.append(self._upsample(flow, mask, scale))
            occs.append(self._upsample(occ, mask, 1.0))
        return flows, occs


def _as_gru_buffer(h_feat: Tensor, cxt_feat: Tensor, total: int, consume: bool = False) -> Tensor:
    """[h | cxt | ...] buffer of ``total`` channels.  The GRU updates h in place and the motion
    features land next to cxt, so the buffer is private to one decoder run: a fresh copy of the
    inputs, unless the caller hands its own buffer over (``consume``: the refiner's get_pose /
    get_flow, whose extract_feat output is used exactly once) and h_feat / cxt_feat already are
    adjacent channel slices of such a buffer (zero-copy)."""
    n, hc, h, w = h_feat.shape
    cc = cxt_feat.shape[1]
    base = h_feat._base
    if (consume and base is not None and base is cxt_feat._base and base.dim() == 4 and base.is_contiguous()
            and tuple(base.shape) == (n, total, h, w)
            and h_feat.data_ptr() == base.data_ptr()
            and cxt_feat.data_ptr() == base.data_ptr() + hc * h * w * 4
            and h_feat.stride() == base.stride() and cxt_feat.stride() == base.stride()):
        return base
    hx = torch.empty((n, total, h, w), dtype=torch.float32, device=h_feat.device)
    ops.copy_channels(h_feat, hx[:, :hc])
    ops.copy_channels(cxt_feat, hx[:, hc:hc + cc])
    return hx
