"""Operator-level Python wrappers over the C ABI (include/scflow_hip.h).

torch is used for what it is good at here -- owning device memory and exposing
the current HIP stream; every arithmetic operation below runs in a
hand-written gfx950 kernel of libscflow_hip.so.  CPU tensors are rejected:
there is no fallback path.

Tensors may be *sample-strided* NCHW views (a channel slice of a larger
contiguous NCHW buffer): only the batch stride is free, which is how channel
concatenations are expressed without copies.
"""
from __future__ import annotations

import ctypes as C
import os
import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import (ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH, CONV_GRU_Q, CONV_GRU_ZR,
                   CONV_PLAIN, ConvDesc)

Tensor = torch.Tensor

__all__ = ['record_conv_kernels', 'PackedConv', 'conv_desc', 'gru_passes', 'scflow_iteration', 'side_stream_handle', 'pyramid_layout', 'untile_level', 'level_storage_shape', 'sepconv_gru', 'pack_conv_weight', 'pack_conv_weight_f16x3', 'f16x3_weight_excess', 'set_conv_precision', 'set_conv_winograd', 'get_conv_winograd', 'pack_conv_weight_wino', 'pack_conv_weight_wino1d', 'pack_conv_weight_wino1d4',
           'get_conv_precision', 'set_conv_kslices', 'conv_kslices', 'conv_kslices_for', 'constant', 'clear_constants', 'register_conv_workspace', 'choose_kc', 'conv2d', 'conv2d_pair', 'corr_build', 'corr_lookup',
           'instance_norm', 'group_norm_relu', 'linear', 'fc_splitk', 'fc_slices', 'pose_update', 'reproject_flow',
           'flow_corr_2d3d', 'pnp_params', 'pnp_ransac', 'pnp',
           'unproject_depth', 'linear_pair', 'resize_bilinear', 'resize_bilinear_grad', 'reproject_flow_grad', 'pose_update_grad', 'convex_upsample', 'avgpool2x2', 'copy_channels',
           'fc_operand', 'fc_dgrad', 'fc_wgrad', 'pose_select_grad', 'group_norm_flat_grad', 'batch_norm_train', 'batch_norm_train_grad',
           'ADAMW_CHUNK', 'ADAMW_NORM_THREADS', 'adamw_chunk_table', 'adamw_chunk_rows', 'AdamwChunks', 'grad_sqnorm', 'adamw_step',
           'ACT_NONE', 'ACT_RELU', 'ACT_SIGMOID', 'ACT_TANH', 'CONV_PLAIN', 'CONV_GRU_ZR',
           'CONV_GRU_Q']


# The two queries every launch makes -- current device, its current stream -- go straight to torch's C
# layer: torch.cuda.current_stream() builds a Stream object through four Python frames per call (~3 us),
# a fifth of the host cost of an eager batch-1 pass (tools/lab/host_profile.py).
_cur_dev = torch._C._cuda_getDevice
_raw_stream = torch._C._cuda_getCurrentRawStream


# ---- K-slice workspaces (scf_conv_workspace): opt-in.  With a workspace registered for a stream the library splits small-grid
#      convolutions launched on it into K slices + a combine launch.  Measured on this network (tools/lab/b1_autoslice_ab.py,
#      hipGraph replay): batch 1 3.09 vs 2.88 ms, batch 2 3.65 vs 3.42, batch 4 4.52 vs 4.47, batch 8 equal -- the combine
#      launch (~5.5 us) costs more than the shorter chains save (<= 7 us on the longest one), so nothing registers one by
#      default; ``register_conv_workspace()`` is for callers whose layers have longer chains. ----
_KWS = {}
_KWS_FLOATS = 1 << 20       # the rule slices only launches of <= 256 K-split blocks: N * Cout * Ho * Wo <= 2^18 floats, x 4 slices


def register_conv_workspace(enable: bool = True) -> None:
    """register (or clear) a 4 MB K-slice workspace for the CURRENT stream of the current device.
    The library keys its registry by the raw ``hipStream_t``: CLEAR the registration (``enable=False`` on that stream)
    before destroying a stream -- a new stream that is handed the same handle would otherwise inherit the workspace and
    could share it with another live stream."""
    dev = _cur_dev()
    handle = _raw_stream(dev)
    if enable:
        ws = torch.empty((_KWS_FLOATS,), dtype=torch.float32, device=f'cuda:{dev}')
        _lib.check(_lib.load().scf_conv_workspace(handle, ws.data_ptr(), _KWS_FLOATS), 'scf_conv_workspace')
        _KWS[(dev, handle)] = ws
    elif _KWS.pop((dev, handle), None) is not None:
        _lib.check(_lib.load().scf_conv_workspace(handle, None, 0), 'scf_conv_workspace')


def _stream() -> int:
    return _raw_stream(_cur_dev())


def _dev(t: Tensor, name: str) -> None:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.ScflowHipError(f'{name}: expected a tensor on the GPU (HIP path only, no CPU '
                                  'fallback)')
    if t.dtype != torch.float32:
        raise _lib.ScflowHipError(f'{name}: expected float32, got {t.dtype}')
    # launches go to the CURRENT device's current stream: a tensor on another GPU would be
    # touched through peer access (or fault) from the wrong device's stream
    if t.device.index != _cur_dev():
        raise _lib.ScflowHipError(
            f'{name} lives on cuda:{t.device.index} but the current device is '
            f'cuda:{_cur_dev()}: wrap the call in torch.cuda.device(tensor.device)')


def _dense(t: Tensor, name: str) -> int:
    _dev(t, name)
    if not t.is_contiguous():
        raise _lib.ScflowHipError(f'{name}: expected a contiguous tensor')
    return t.data_ptr()


def _nchw(t: Tensor, name: str) -> Tuple[int, int, int, int, int, int]:
    """(ptr, N, C, H, W, sample_stride) of a sample-strided NCHW tensor."""
    _dev(t, name)
    if t.dim() != 4:
        raise _lib.ScflowHipError(f'{name}: expected 4-D NCHW')
    n, c, h, w = t.shape
    sn, sc, sh, sw = t.stride()
    ok = (sw == 1 or w == 1) and (sh == w or h == 1) and (sc == h * w or c == 1)
    if not ok:
        raise _lib.ScflowHipError(f'{name}: not a sample-strided NCHW view (strides {t.stride()})')
    if n == 1:
        sn = c * h * w
    return t.data_ptr(), n, c, h, w, sn


def _opt(t: Optional[Tensor], name: str) -> Optional[int]:
    return None if t is None else _dense(t, name)


# ------------------------------------------------- small-batch stream overlap
# At batch 1 every kernel of the path fills a fraction of the chip (a 32x32 map is 8-32 blocks on 256
# CUs), so independent branches are put on a second HIP stream and run side by side; hipGraph
# capture records the fork / join as graph dependencies.  Large batches keep one stream.
_SIDE = {}      # (device, main stream handle) -> that stream's side stream


# r6 (tools/lab/b1_branches.py: every subset of the four branches as hipGraph replays; tools/lab/graph_fork_penalty.py; tools/lab/
# b1_pairs.py; profiles/r6_b1_branch_subsets.txt, profiles/r6_b1_pairs.txt): on this runtime a replay pays ~1.2 us per NODE as soon
# as the graph holds a real parallel branch (0.33-0.36 ms at 285 nodes, whatever the number of fork / join edges; eager two-stream
# execution pays about the same in event waits), each branch then buys 0.16-0.17 ms back ('upsample': -0.05).  Since r6 the flow and
# mask branches and the context encoder ride in the main branch's launches instead (PAIR_BRANCHES: scf_conv2d_pair, two small-grid
# layers in one launch) and NO branch uses the side stream by default: batch 1 2.71 -> 2.56 ms, batch 2 3.25 -> 3.12, batch 4
# 4.33 -> 4.24 (identical results).  The streams stay available: ops.OVERLAP_BRANCHES = {'context', 'flow', 'mask'[, 'upsample']}, ops.PAIR_BRANCHES = set().
OVERLAP_BRANCHES = set()
OVERLAP_MAX_PIXELS = {'context': 4 * 256 * 256, 'flow': 4 * 256 * 256, 'mask': 4 * 256 * 256, 'upsample': 4 * 256 * 256}


# r6: branches whose convolutions ride in the main branch's launches (scf_conv2d_pair: two small-grid layers, one launch) instead
# of running on the side stream -- the C iteration only (SCFlowDecoder.c_iteration); takes precedence over OVERLAP_BRANCHES
PAIR_BRANCHES = {'context', 'flow', 'mask'}
# ... up to this many pixels per batch (None: any size -- scf_conv2d_pair itself merges a pair only where one launch needs fewer
# rounds of resident blocks than two; the flow branch gains at EVERY batch size: at batch 32 corr_net.1 (768 blocks) and flow_net.1
# (256) are 1.5 + 0.5 rounds apart and 2 full rounds together, 14.00 -> 13.89 ms per step; batch 16: 8.40 -> 8.17).  The two encoders
# walked together lose at batch 32 (they evict each other's activations), the mask branch has no mergeable pair there.
PAIR_MAX_PIXELS = {'context': 4 * 256 * 256, 'flow': None, 'mask': None}


def branch_mode(n: int, h: int, w: int, branch: str) -> int:
    """0 = in order, 1 = side stream, 2 = merged launches, for the C iteration's ``overlap_*`` fields."""
    if branch in PAIR_BRANCHES:
        lim = PAIR_MAX_PIXELS.get(branch, 4 * 256 * 256)
        return 2 if lim is None or n * h * w <= lim else 0
    lim = OVERLAP_MAX_PIXELS.get(branch, 4 * 256 * 256)
    return 1 if n * h * w <= lim and branch in OVERLAP_BRANCHES else 0


def small_work(n: int, h: int, w: int, branch: Optional[str] = None) -> bool:
    """whether a batch of n (h, w) images is small enough for branch-level concurrency to pay
    (``branch``: and that branch is enabled)."""
    lim = OVERLAP_MAX_PIXELS.get(branch, 4 * 256 * 256)
    return n * h * w <= lim and (branch is None or branch in OVERLAP_BRANCHES)


def fork_point() -> 'torch.cuda.Event':
    """record and RETURN an event at this point of the current stream; hand it to
    ``side_stream(after=...)`` to let a side branch start from here instead of from where the
    branch is opened.  The event travels explicitly (no module-level state): an event that is never
    consumed -- an exception between the two calls, a disabled branch -- cannot leak into a later,
    unrelated branch."""
    ev = torch.cuda.Event()
    ev.record()
    return ev


class side_stream:
    """``br = side_stream(enabled, after=ev); with br: <branch>`` enqueues the block on the second
    stream that belongs to (this device, the current stream), ordered after ``ev`` (a
    ``fork_point()`` of the current stream) or, without one, after everything enqueued so far;
    ``br.join()`` -- called once the OTHER branch has been enqueued on the main stream -- makes the
    main stream wait for it.  Tensors the branch writes into are allocated before the fork point;
    tensors it allocates itself must not escape it.  ``enabled=False``: plain in-order execution.
    One side stream per main stream: a user stream and e.g. GraphedRefiner's warm-up stream never
    share one."""

    def __init__(self, enabled: bool = True, after: Optional['torch.cuda.Event'] = None) -> None:
        self.enabled, self.after, self.ctx, self.side = enabled, after, None, None

    def __enter__(self):
        if not self.enabled:
            return self
        main = torch.cuda.current_stream()
        key = (torch.cuda.current_device(), main.cuda_stream)
        self.side = _SIDE.get(key)
        if self.side is None:
            self.side = _SIDE[key] = torch.cuda.Stream(device=key[0])
        ev, self.after = self.after, None
        if ev is not None:
            self.side.wait_event(ev)
        else:
            self.side.wait_stream(main)
        self.ctx = torch.cuda.stream(self.side)
        self.ctx.__enter__()
        return self

    def __exit__(self, *exc):
        if self.enabled and self.ctx is not None:
            self.ctx.__exit__(*exc)
            self.ctx = None
        return False

    def join(self) -> None:
        if self.enabled and self.side is not None:
            torch.cuda.current_stream().wait_stream(self.side)


# ------------------------------------------------------------------ conv
def choose_kc(cin: int, kh: int, kw: int, stride: int = 1) -> int:
    """channels staged per LDS round (scf_conv2d accepts 2, 8, 32): 32 for dense 1x1
    (a chunk must carry enough MFMA work to amortise its barriers), 2 for thin inputs or
    wide kernels (LDS / prefetch-register budget), else 8."""
    if cin < 8 or kh * kw >= 25:
        return 2
    if kh * kw == 1 and stride == 1 and cin >= 32:
        return 32
    return 8


def pack_conv_weight(weight: Tensor, kc: int) -> Tuple[Tensor, int]:
    """(Cout, Cin, KH, KW) -> packed (nchunk*T*KC, Mld) with
    row = (chunk*T + tap)*KC + channel_in_chunk, col = cout; zero rows for
    padded channels; Mld = Cout rounded up to 32 (see scf_conv2d)."""
    cout, cin, kh, kw = weight.shape
    t = kh * kw
    nchunk = (cin + kc - 1) // kc
    mld = (cout + 31) // 32 * 32
    w = torch.zeros((cout, nchunk * kc, t), dtype=torch.float32, device=weight.device)
    w[:, :cin] = weight.reshape(cout, cin, t).float()
    w = w.reshape(cout, nchunk, kc, t).permute(1, 3, 2, 0).reshape(nchunk * t * kc, cout)
    out = torch.zeros((nchunk * t * kc, mld), dtype=torch.float32, device=weight.device)
    out[:, :cout] = w
    return out.contiguous(), mld


def pack_conv_weight_f16x3(weight: Tensor) -> Tensor:
    """(Cout, Cin, KH, KW) fp32 -> split-fp16 packing for conv_f16x3.hip:
    w = hi + lo' * 2**-11 with hi = fp16(w), lo' = fp16((w - hi) * 2**11); cells of 8 channels,
    shape ((chunk16*T + tap)*2 + k8, plane hi|lo, Mld, 8) float16."""
    cout, cin, kh, kw = weight.shape
    t = kh * kw
    nchunk = (cin + 31) // 32 * 2       # 16-channel chunks, padded to a multiple of 32 channels
    mld = (cout + 31) // 32 * 32
    w = torch.zeros((cout, nchunk * 16, t), dtype=torch.float32, device=weight.device)
    w[:, :cin] = weight.reshape(cout, cin, t).float()
    hi = w.half()
    lo = ((w - hi.float()) * 2048.0).half()
    out = torch.zeros((nchunk, t, 2, 2, mld, 8), dtype=torch.float16, device=weight.device)
    for plane, x in enumerate((hi, lo)):
        out[:, :, :, plane, :cout] = x.reshape(cout, nchunk, 2, 8, t).permute(1, 4, 2, 0, 3)
    return out.reshape(nchunk * t * 2, 2, mld, 8).contiguous()


F16X3_WEIGHT_EXCESS_MAX = 2.0


def f16x3_weight_excess(weight: Tensor) -> float:
    """how far a layer's weights are outside the split's domain: with w = hi + w_l + e_w (hi = fp16(w), w_l = lo' 2**-11,
    lo' = fp16((w - hi) 2**11), roundings on the host: nearest even, fp16 subnormals kept), the worst output channel's
    (sum |e_w| + 2**-11 sum |w_l|) / (2**-22 sum |w|); 0 for an all-zero channel, inf where some hi is not finite.  For
    weights in 2**-14 <= |w| < 65520 both terms are bounded by 2**-22 |w|, so the figure is at most 2
    (``F16X3_WEIGHT_EXCESS_MAX``); it grows as 2**-14 / |w| below that (843 units of 2**-24 sum|w||x| measured on weights
    of 1e-6 by the host restatement, tests/test_conv_f16x3_host.py)."""
    w = weight.detach().to('cpu', torch.float32)
    hi = w.half().float()
    lo = ((w - hi) * 2048.0).half().double()
    w, hi = w.double(), hi.double()
    e = w - hi - lo / 2048.0
    num = (e.abs() + lo.abs() / (2048.0 * 2048.0)).flatten(1).sum(1)
    den = 2.0 ** -22 * w.abs().flatten(1).sum(1)
    ratio = torch.where(num == 0, torch.zeros_like(num), num / den)
    ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float('inf')))
    return float(ratio.max())


def choose_a4_groups(cin: int, kh: int, kw: int, stride: int) -> int:
    """8G channels per staged chunk of the LDS-DMA kernel (0: layer not eligible)."""
    t = kh * kw
    if stride not in (1, 2) or cin < 8 or t >= 25:
        return 0
    if t == 1:      # dense 1x1: 32-channel chunks (stride 2 = the ResNet shortcuts: staged as a dense 1x1 over
        return 4 if cin >= 64 else 0                        # every second row / column, conv_dma.hip)
    return 2 if t <= 5 else 1


def choose_a4s_groups(cin: int, kh: int, kw: int, stride: int) -> int:
    """8G channels per staged chunk of the SMALL-GRID a4 packing (0: not eligible): at batch 1
    one block runs per CU and the per-chunk fixed cost dominates, so chunks are 2-4x bigger than on
    full grids (and dense 1x1 layers join in)."""
    t = kh * kw
    if stride not in (1, 2) or cin < 16 or t >= 25:
        return 0
    return 4 if t <= 5 else 2


def choose_a4t_groups(cin: int, kh: int, kw: int, stride: int) -> int:
    """TINY-grid a4 packing (no more K-split blocks than CUs): 32-channel chunks for the 3x3 layers,
    whose small-grid packing has 16 (0: the layer has none)."""
    t = kh * kw
    return 4 if (stride in (1, 2) and cin >= 32 and 5 < t < 25) else 0


def pack_conv_weight_a4(weight: Tensor, groups: int) -> Tuple[Tensor, int]:
    """(Cout, Cin, KH, KW) -> [chunk][tap][g][h][Mld][4] (conv_dma.hip): channel
    chunk*8G + 8g + 2s + h at float s of cell (g, h); zero-padded channels and couts."""
    cout, cin, kh, kw = weight.shape
    t, kc = kh * kw, 8 * groups
    nchunk = (cin + kc - 1) // kc
    mld = (cout + 31) // 32 * 32
    w = torch.zeros((mld, nchunk * kc, t), dtype=torch.float32, device=weight.device)
    w[:cout, :cin] = weight.reshape(cout, cin, t).float()
    # channel index -> (chunk, g, s, h)
    w = w.reshape(mld, nchunk, groups, 4, 2, t).permute(1, 5, 2, 4, 0, 3)
    return w.contiguous().reshape(-1), mld


def pack_conv_weight_thin(weight: Tensor) -> Tensor:
    """(Cout <= 4, Cin, KH, KW) -> [Cin][KH*KW][CO] (conv_thin.hip), CO = Cout rounded up to
    1 / 2 / 4, padded to a multiple of 4 floats."""
    cout, cin, kh, kw = weight.shape
    co = 1 if cout <= 1 else 2 if cout <= 2 else 4
    w = torch.zeros((cin, kh * kw, co), dtype=torch.float32, device=weight.device)
    w[:, :, :cout] = weight.reshape(cout, cin, kh * kw).permute(1, 2, 0).float()
    flat = torch.zeros(((w.numel() + 3) // 4 * 4,), dtype=torch.float32, device=weight.device)
    flat[:w.numel()] = w.reshape(-1)
    return flat


def pack_conv_weight_taps(weight: Tensor) -> Tensor:
    """(Cout, Cin <= 4, KH, KW) -> [Kp][Mld] (conv_taps.hip): row k = ci * KH*KW + t, Kp = Cin*KH*KW rounded
    up to a multiple of 8, Mld = Cout rounded up to 32; zero padded."""
    cout, cin, kh, kw = weight.shape
    t = kh * kw
    kp = (cin * t + 7) // 8 * 8
    mld = (cout + 31) // 32 * 32
    out = torch.zeros((kp, mld), dtype=torch.float32, device=weight.device)
    out[:cin * t, :cout] = weight.reshape(cout, cin * t).t().float()
    return out.contiguous()


def pack_conv_weight_wino(weight: Tensor) -> Tensor:
    """(Cout, Cin, 3, 3) -> U = G g G^T in conv_wino.hip's layout, on the weight's device: the library's
    own host packer (``scf_pack_conv_weight_wino``: computed in double, rounded once; layout in
    include/scflow_hip.h) + one copy.  No vendor BLAS on the set-up path."""
    cout, cin, kh, kw = weight.shape
    if (kh, kw) != (3, 3):
        raise ValueError('Winograd packing: 3x3 kernels')
    lib = _lib.load()
    host_w = weight.detach().to('cpu', torch.float32).contiguous()
    out = torch.empty((int(lib.scf_pack_conv_weight_wino_size(cout, cin)),), dtype=torch.float32)
    _lib.check(lib.scf_pack_conv_weight_wino(host_w.data_ptr(), cout, cin, out.data_ptr()), 'scf_pack_conv_weight_wino')
    return out.to(weight.device)


def pack_conv_weight_wino1d(weight: Tensor) -> Tensor:
    """(Cout, Cin, 1, 5) or (Cout, Cin, 5, 1) -> U = G g in conv_wino1d.hip's layout, on the weight's device
    (``scf_pack_conv_weight_wino1d``: G = the 6 x 5 matrix of the points 0, 1, -1, 2, -2, infinity; computed
    in double, rounded once)."""
    cout, cin, kh, kw = weight.shape
    if (kh, kw) not in ((1, 5), (5, 1)):
        raise ValueError('F(2, 5) packing: 1x5 / 5x1 kernels')
    lib = _lib.load()
    host_w = weight.detach().to('cpu', torch.float32).reshape(cout, cin, 5).contiguous()
    out = torch.empty((int(lib.scf_pack_conv_weight_wino1d_size(cout, cin)),), dtype=torch.float32)
    _lib.check(lib.scf_pack_conv_weight_wino1d(host_w.data_ptr(), cout, cin, out.data_ptr()), 'scf_pack_conv_weight_wino1d')
    return out.to(weight.device)


def pack_conv_weight_wino1d4(weight: Tensor) -> Tensor:
    """(Cout, Cin, 1, 5) or (Cout, Cin, 5, 1) -> U = G g in conv_wino1d4.hip's layout, on the weight's device
    (``scf_pack_conv_weight_wino1d4``: G = the 8 x 5 matrix of the points 0, 1, -1, 2, -2, 1/2, -1/2, infinity;
    computed in double, rounded once)."""
    cout, cin, kh, kw = weight.shape
    if (kh, kw) not in ((1, 5), (5, 1)):
        raise ValueError('F(4, 5) packing: 1x5 / 5x1 kernels')
    lib = _lib.load()
    host_w = weight.detach().to('cpu', torch.float32).reshape(cout, cin, 5).contiguous()
    out = torch.empty((int(lib.scf_pack_conv_weight_wino1d4_size(cout, cin)),), dtype=torch.float32)
    _lib.check(lib.scf_pack_conv_weight_wino1d4(host_w.data_ptr(), cout, cin, out.data_ptr()), 'scf_pack_conv_weight_wino1d4')
    return out.to(weight.device)


_CONV_PRECISION = 'f32'
_CONV_WINOGRAD = True


def set_conv_winograd(on: bool) -> bool:
    """3x3 / stride-1 / pad-1 layers with plain or affine epilogues through the Winograd F(2x2, 3x3)
    kernel (conv_wino.hip: fp32 throughout, 2.25x fewer matrix-core flops, sums re-associated: error vs
    fp64 1.5-1.8x the direct kernels' ~1e-6, end-to-end flow EPE unchanged at 6e-5 px) instead of the direct
    kernels, on grids of >= CUs / 2 blocks (small grids stay direct); the 1x5 / 5x1 GRU gates likewise through
    the F(2, 5) kernel (conv_wino1d.hip).  On by default.  Under conv precision 'f16x3' the layers that carry
    a split-fp16 packing take that kernel instead; layers without one (Cin < 16) still take Winograd.
    ``False`` = the direct kernels everywhere (bit-for-bit fp32 fma chains in the reference's summation
    order).  NB the kernel choice depends on the grid size (batch x map size) and the device's CU count:
    the same pair can differ by ~1e-6 between batch 1 and batch 32; ``set_conv_winograd(False)`` removes
    the largest part of that dependence (the direct kernels still pick K-split tiles on small grids).
    Returns the previous setting."""
    global _CONV_WINOGRAD
    prev, _CONV_WINOGRAD = _CONV_WINOGRAD, bool(on)
    return prev


def get_conv_winograd() -> bool:
    return _CONV_WINOGRAD


def set_conv_precision(mode: str) -> str:
    """'f32'   : v_mfma_f32_32x32x2_f32 everywhere (bit-for-bit fp32 fma chains);
    'f16x3' : spatial convolutions with >= 16 input channels run on the fp16 matrix cores as
              three MFMAs over an exact hi/lo split of both operands (fp32 accumulate, ~22
              mantissa bits; flow EPE ~1e-4 px vs fp32 on this path), everything else fp32.
    The contract of 'f16x3' (tests/test_conv_f16x3_host.py derives it, tests/test_gpu_conv_f16x3.py holds the kernel to it):
      * operands with 2**-14 <= |v| <= 65504 (or 0): |result - true| <= (3 + 2**-22) 2**-22 sum|w||x| on top of the fp32
        accumulation error (K + 1) 2**-24 sum|w||x| -- fp32 class;
      * below 2**-14 the split's error stops shrinking with the operand (<= 2**-25 per half, 2**-36 left over, absolute):
        results degrade gracefully, a layer whose operands are all near 1e-6 keeps about five bits.  WEIGHTS are checked at
        pack time (``f16x3_weight_excess``): ``PackedConv.from_weight`` gives such a layer no split packing and it runs on the
        fp32 kernels (``record_conv_kernels`` shows which); activations cannot be checked before the launch;
      * a finite activation of 65520 or more becomes an infinite high half: every output of its receptive field, in every
        output channel, is non-finite (a ReLU epilogue, compare + select, turns NaN and -inf into 0), and nothing outside the
        field changes by a bit (the fp32 routes return finite numbers).
    Returns the previous mode."""
    global _CONV_PRECISION
    if mode not in ('f32', 'f16x3'):
        raise ValueError(mode)
    prev, _CONV_PRECISION = _CONV_PRECISION, mode
    return prev


def get_conv_precision() -> str:
    return _CONV_PRECISION


@dataclass
class PackedConv:
    """a convolution's parameters in kernel layout (device resident)."""
    wp: Tensor
    bias: Optional[Tensor]
    scale: Optional[Tensor]
    shift: Optional[Tensor]
    cin: int
    cout: int
    kh: int
    kw: int
    stride: int
    pad_h: int
    pad_w: int
    kc: int
    mld: int
    wp_alt: Optional[Tensor] = None   # KC=32 packing of the same weights (short-chunk regime)
    plans: Optional[dict] = None      # (N, H, W, C0, C1) -> use the KC=32 packing?
    wp16: Optional[Tensor] = None     # split-fp16 packing (spatial kernels, Cin >= 16)
    wp4: Optional[Tensor] = None      # LDS-DMA packing (stride 1, Cin >= 8)
    g4: int = 0
    wthin: Optional[Tensor] = None    # [Cin][T][CO] packing (Cout <= 4)
    wp4s: Optional[Tensor] = None     # small-grid LDS-DMA packing (bigger chunks)
    g4s: int = 0
    wtaps: Optional[Tensor] = None    # [Cin*T][Mld] packing (Cin <= 4: contraction over taps)
    desc: Optional[ConvDesc] = None   # scf_conv_desc with this layer's own fields filled (built lazily)
    wp4t: Optional[Tensor] = None     # tiny-grid LDS-DMA packing of 3x3 layers (32-channel chunks)
    g4t: int = 0
    wwino: Optional[Tensor] = None    # G g G^T packing (3x3, stride 1, pad 1, Cin >= 8)
    wwino1d: Optional[Tensor] = None  # G g packing (1x5 / 5x1, stride 1, 'same', Cin >= 16, Cout % 64 == 0)
    wwino1d4: Optional[Tensor] = None  # the F(4, 5) packing of the same layers

    @staticmethod
    def from_weight(weight: Tensor, bias: Optional[Tensor], stride: int = 1,
                    padding=0, bn: Optional[Sequence[Tensor]] = None,
                    eps: float = 1e-5, dma_packing: bool = True) -> 'PackedConv':
        """``bn`` = (gamma, beta, running_mean, running_var): eval-mode BatchNorm
        folded into a per-channel scale/shift applied after the bias.  ``dma_packing=False``
        leaves out the LDS-DMA kernel's packing (the layer then runs on the register-staged
        kernel; used by the A/B parity tests)."""
        cout, cin, kh, kw = weight.shape
        kc = choose_kc(cin, kh, kw, stride)
        wp, mld = pack_conv_weight(weight, kc)
        wp_alt = pack_conv_weight(weight, 32)[0] if (kc == 8 and cin >= 32) else None
        # the split-fp16 route only for weights inside the split's domain (f16x3_weight_excess): a layer of tiny or
        # over-range weights keeps wp16 = None and runs on the fp32 kernels under every conv precision
        wp16 = pack_conv_weight_f16x3(weight) if (cin >= 16 and kh * kw > 1 and
                                                  f16x3_weight_excess(weight) <= F16X3_WEIGHT_EXCESS_MAX) else None
        ph, pw = (padding, padding) if isinstance(padding, int) else padding
        scale = shift = None
        if bn is not None:
            gamma, beta, mean, var = [b.float() for b in bn]
            scale = (gamma / torch.sqrt(var + eps)).contiguous()
            shift = (beta - mean * scale).contiguous()
        g4 = choose_a4_groups(cin, kh, kw, stride) if dma_packing else 0
        wp4 = pack_conv_weight_a4(weight, g4)[0] if g4 else None
        g4s = choose_a4s_groups(cin, kh, kw, stride) if dma_packing else 0
        wp4s = pack_conv_weight_a4(weight, g4s)[0] if g4s else None
        return PackedConv(wp, None if bias is None else bias.float().contiguous(), scale, shift,
                          cin, cout, kh, kw, stride, ph, pw, kc, mld, wp_alt, {}, wp16, wp4, g4,
                          pack_conv_weight_thin(weight) if (cout <= 4 and stride == 1 and cin >= 32) else None,
                          wp4s, g4s, pack_conv_weight_taps(weight) if (cin <= 4 and dma_packing) else None,
                          None, *PackedConv._tiny(weight, kh, kw, stride, dma_packing),
                          pack_conv_weight_wino(weight) if (dma_packing and (kh, kw, stride, ph, pw) == (3, 3, 1, 1, 1)
                                                            and cin >= 8) else None,
                          pack_conv_weight_wino1d(weight) if (dma_packing and stride == 1 and cin >= 16 and cout % 64 == 0
                                                              and (kh, kw, ph, pw) in ((1, 5, 0, 2), (5, 1, 2, 0))) else None,
                          pack_conv_weight_wino1d4(weight) if (dma_packing and stride == 1 and cin >= 16 and cout % 64 == 0
                                                               and (kh, kw, ph, pw) in ((1, 5, 0, 2), (5, 1, 2, 0))) else None)

    @staticmethod
    def _tiny(weight, kh, kw, stride, dma_packing):
        g = choose_a4t_groups(weight.shape[1], kh, kw, stride) if dma_packing else 0
        return (pack_conv_weight_a4(weight, g)[0] if g else None), g

    def out_hw(self, h: int, w: int) -> Tuple[int, int]:
        return ((h + 2 * self.pad_h - self.kh) // self.stride + 1,
                (w + 2 * self.pad_w - self.kw) // self.stride + 1)


def _desc_template(pc: 'PackedConv') -> ConvDesc:
    d = ConvDesc()
    d.wp, d.w_nstride, d.Mld, d.Cout = pc.wp.data_ptr(), 0, pc.mld, pc.cout
    d.KH, d.KW, d.stride, d.pad_h, d.pad_w, d.KC = pc.kh, pc.kw, pc.stride, pc.pad_h, pc.pad_w, pc.kc
    d.bias = None if pc.bias is None else pc.bias.data_ptr()
    d.scale = None if pc.scale is None else pc.scale.data_ptr()
    d.shift = None if pc.shift is None else pc.shift.data_ptr()
    d.out_div = 1.0
    if pc.wthin is not None:
        d.wp_thin = pc.wthin.data_ptr()
    if pc.wtaps is not None:
        d.wp_taps = pc.wtaps.data_ptr()
    if pc.wp4 is not None:
        d.wp_a4, d.a4_groups, d.a4_mld = pc.wp4.data_ptr(), pc.g4, pc.mld
    if pc.wp4s is not None:
        d.wp_a4s, d.a4s_groups, d.a4_mld = pc.wp4s.data_ptr(), pc.g4s, pc.mld
    if pc.wp4t is not None:
        d.wp_a4t, d.a4t_groups, d.a4_mld = pc.wp4t.data_ptr(), pc.g4t, pc.mld
    return d


def conv_desc(pc: PackedConv, x0: Tensor, x1: Optional[Tensor] = None, out: Optional[Tensor] = None,
              **kw) -> Tuple[ConvDesc, Tensor]:
    """the filled ``scf_conv_desc`` of ``conv2d(pc, x0, x1, out, **kw)`` WITHOUT launching it, and the
    output tensor: for entry points that take whole descriptors (``scf_scflow_iteration``)."""
    return conv2d(pc, x0, x1, out, _launch=False, **kw)


def conv2d(pc: PackedConv, x0: Tensor, x1: Optional[Tensor] = None, out: Optional[Tensor] = None,
           *, res: Optional[Tensor] = None, act: int = ACT_NONE, act2: int = ACT_NONE,
           act_split: int = 0, mode: int = CONV_PLAIN, gru_h: Optional[Tensor] = None,
           gru_aux: Optional[Tensor] = None, gru_z: Optional[Tensor] = None, kslices: int = 1,
           _launch: bool = True):
    """implicit-GEMM MFMA convolution with fused epilogue (scf_conv2d).
    input = channel concat of x0 and x1; ``out`` may be a channel slice.
    ``kslices`` = S > 1: the contraction over the input channels is split across S groups of blocks
    (``scf_conv_desc.k_slices``); returns the (S, N, Cout, Ho, Wo) RAW partial sums -- the consumer adds them in slice
    order (``group_norm_relu`` / ``fc_splitk`` take such a tensor).  Plain epilogue only (the layer has no bias)."""
    p0, n, c0, h, w, s0 = _nchw(x0, 'x0')
    p1, c1, s1 = None, 0, 0
    if x1 is not None:
        p1, n1, c1, h1, w1, s1 = _nchw(x1, 'x1')
        if (n1, h1, w1) != (n, h, w):
            raise _lib.ScflowHipError('x0/x1 shape mismatch')
    if c0 + c1 != pc.cin:
        raise _lib.ScflowHipError(f'conv expects {pc.cin} input channels, got {c0}+{c1}')
    ho, wo = pc.out_hw(h, w)
    sliced = None
    if kslices > 1:
        if pc.bias is not None or pc.scale is not None or res is not None or act != ACT_NONE or mode != CONV_PLAIN:
            raise _lib.ScflowHipError('conv2d(kslices > 1): partial sums take a plain epilogue (no bias / BN / res / act)')
        sliced = out if out is not None else torch.empty((kslices, n, pc.cout, ho, wo), dtype=torch.float32, device=x0.device)
        if tuple(sliced.shape) != (kslices, n, pc.cout, ho, wo) or not sliced.is_contiguous():
            raise _lib.ScflowHipError(f'conv2d(kslices={kslices}): out must be a contiguous {(kslices, n, pc.cout, ho, wo)} tensor')
        out = sliced[0]
    if out is None:
        out = torch.empty((n, pc.cout // 2 if mode == CONV_GRU_ZR else pc.cout, ho, wo),
                          dtype=torch.float32, device=x0.device)
    po, no, co, oh, ow, so = _nchw(out, 'out')
    want_c = pc.cout // 2 if mode == CONV_GRU_ZR else pc.cout   # ZR: only the z half lands in out
    if (no, co, oh, ow) != (n, want_c, ho, wo):
        raise _lib.ScflowHipError(f'out has shape {tuple(out.shape)}, expected '
                                  f'{(n, want_c, ho, wo)}')
    # the layer's own fields (weights in every packing, geometry, bias / BN) are filled once per
    # PackedConv and copied; a call sets the tensors and the epilogue
    tmpl = pc.desc
    if tmpl is None:
        tmpl = pc.desc = _desc_template(pc)
    d = ConvDesc.from_buffer_copy(tmpl)
    d.in0, d.in1, d.C0, d.C1 = p0, p1, c0, c1
    d.in0_nstride, d.in1_nstride = s0, s1
    d.N, d.H, d.W = n, h, w
    d.out, d.out_nstride = po, so
    if sliced is not None:
        d.k_slices, d.out_slice_stride = kslices, sliced.stride(0)
        out = sliced
    if res is not None:
        pr, nr, cr, hr, wr, sr = _nchw(res, 'res')
        if (nr, cr, hr, wr) != (n, pc.cout, ho, wo):
            raise _lib.ScflowHipError('res shape mismatch')
        d.res, d.res_nstride = pr, sr
    d.act, d.act2, d.act_split, d.mode = act, act2, act_split, mode
    if gru_h is not None:
        ph_, _, _, _, _, sh_ = _nchw(gru_h, 'gru_h')
        d.gru_h, d.gru_h_nstride = ph_, sh_
    if gru_aux is not None:
        pa_, _, _, _, _, sa_ = _nchw(gru_aux, 'gru_aux')
        d.gru_aux, d.gru_aux_nstride = pa_, sa_
    if gru_z is not None:
        pz_, _, _, _, _, sz_ = _nchw(gru_z, 'gru_z')
        d.gru_z, d.gru_z_nstride = pz_, sz_
    # Short-chunk regime (smallest tile, WM = WN = 1): with KC=8 the MFMA phase of a chunk
    # (T*4*WM*WN MFMAs of 64 cycles) is shorter than the L2 round trip its prefetch has to
    # hide.  Stage 32 channels per chunk instead when that packing fits (decided once per shape).
    if _CONV_PRECISION == 'f16x3' and pc.wp16 is not None:
        d.wp_f16 = pc.wp16.data_ptr()
    elif _CONV_WINOGRAD and pc.wwino is not None and mode == CONV_PLAIN:
        d.wp_wino = pc.wwino.data_ptr()
    elif _CONV_WINOGRAD and pc.wwino1d is not None:
        d.wp_wino1d = pc.wwino1d.data_ptr()
        d.wp_wino1d4 = pc.wwino1d4.data_ptr() if pc.wwino1d4 is not None else None
    if x1 is not None:
        d.wp_taps = None                # the thin-input kernel takes one input segment
    if pc.wp_alt is not None and (c1 == 0 or c0 % 32 == 0):
        key = (n, h, w, c0, c1, d.wp_f16 is not None)
        use_alt = pc.plans.get(key)
        if use_alt is None:
            lib = _lib.load()
            info = (C.c_int32 * 4)()
            use_alt = False
            # the KC decision describes the DIRECT register-staged kernel: asked with the Winograd packings
            # cleared, so that the cached plan does not depend on whether Winograd was on at the first call
            ww, ww1, ww4, d.wp_wino, d.wp_wino1d, d.wp_wino1d4 = d.wp_wino, d.wp_wino1d, d.wp_wino1d4, None, None, None
            if (lib.scf_conv2d_query(C.byref(d), info) == 0 and info[0] * info[1] == 1
                    and 0 <= info[3] * 64 < 6000):
                d.wp, d.KC = pc.wp_alt.data_ptr(), 32
                use_alt = lib.scf_conv2d_query(C.byref(d), info) == 0
                d.wp, d.KC = pc.wp.data_ptr(), pc.kc
            d.wp_wino, d.wp_wino1d, d.wp_wino1d4 = ww, ww1, ww4
            pc.plans[key] = use_alt
        if use_alt:
            d.wp, d.KC = pc.wp_alt.data_ptr(), 32
    if not _launch:
        return d, out
    if _CONV_EVENTS is not None:        # bench.py: a timer bound to this launch + algorithmic flops
        lib = _lib.load()
        tm = C.c_void_p()
        _lib.check(lib.scf_timer_create(C.byref(tm)), 'scf_timer_create')
        lib.scf_timer_arm(tm)
        try:
            _lib.check(lib.scf_conv2d(C.byref(d), _stream()), 'scf_conv2d')
        finally:
            lib.scf_timer_arm(None)
        tag = ''
        if d.wp_wino or d.wp_wino1d:    # does a Winograd kernel take this launch (grid-size policy)?
            info = (C.c_int32 * 4)()
            if lib.scf_conv2d_query(C.byref(d), info) == 0 and info[3] < 0 and info[0] in (16, 6, 8):
                tag = {16: ' [winograd]', 6: ' [winograd F(2,5)]', 8: ' [winograd F(4,5)]'}[info[0]]
        _CONV_EVENTS.append((tm, 2.0 * pc.cin * pc.kh * pc.kw * pc.cout * ho * wo * n,
                             f'{pc.cin}->{pc.cout} {pc.kh}x{pc.kw}/s{pc.stride} @{ho}x{wo} N{n}' + tag))
        return out
    rc = _lib.load().scf_conv2d(C.byref(d), _stream())
    if rc == -2 and x1 is not None and sliced is None:
        # SCF_EUNSUPPORTED with two input segments: every kernel needs the segment boundary on a channel-chunk boundary
        # (C0 % 8 / 16 / 32 == 0 by packing) -- a layer of the path never violates it, an arbitrary caller may (found by
        # tools/lab/conv_fuzz.py: 1x1 layers with C0 = 8 / 16).  Materialise the concatenation once and run the same
        # layer on one segment: still the HIP kernels, one extra copy.
        return conv2d(pc, torch.cat([x0, x1], 1), None, out, res=res, act=act, act2=act2, act_split=act_split, mode=mode,
                      gru_h=gru_h, gru_aux=gru_aux, gru_z=gru_z)
    _lib.check(rc, 'scf_conv2d')
    return out


def _pair_operand(layer):
    """(descriptor, output, joined input or None) of one layer of ``conv2d_pair``.  Two input segments whose boundary no kernel
    takes are joined first, as ``conv2d`` does on SCF_EUNSUPPORTED (the pair's fallback would otherwise refuse the layer): asked
    of the library for layers that pass an ``x1`` only -- the refiner's pairs never do.  The caller holds the joined tensor until
    the launch is enqueued: freed earlier, its memory could become the other layer's output."""
    pc, x0 = layer[0], layer[1]
    kw = dict(layer[2]) if len(layer) > 2 else {}
    d, out = conv2d(pc, x0, _launch=False, **kw)
    if kw.get('x1') is not None and kw.get('kslices', 1) <= 1:
        info = (C.c_int32 * 4)()
        if _lib.load().scf_conv2d_query(C.byref(d), info) == -2:
            x0, kw['x1'], kw['out'] = torch.cat([x0, kw['x1']], 1), None, out
            d, out = conv2d(pc, x0, _launch=False, **kw)
            return d, out, x0
    return d, out, None


def conv2d_pair(a, b):
    """two INDEPENDENT convolutions, ``a`` and ``b`` = ``(PackedConv, x0[, kwargs of conv2d])``, through ``scf_conv2d_pair``: ONE
    launch where both fall to the same small-grid kernel instantiation and fit the chip together, else one after the other.
    Returns the two outputs (bit-identical to two ``conv2d`` calls either way)."""
    da, oa, ja = _pair_operand(a)
    db, ob, jb = _pair_operand(b)
    _lib.check(_lib.load().scf_conv2d_pair(C.byref(da), C.byref(db), _stream()), 'scf_conv2d_pair')
    del ja, jb          # the joined inputs (if any) lived until the launch was enqueued on this stream
    return oa, ob


_CONV_EVENTS = None

# ---- read-only constant tensors (the all-zero initial flow, the all-ones first-iteration mask): filled ONCE per
#      (device, shape, value) and handed out again -- a steady-state step then launches no fill kernel.  Kernels only
#      READ them (init_flow feeds the first 1/8 down-sampling, the ones map the first mask multiply); callers that
#      want to write must not ask here.
#      Lifetime rules: entries are NEVER evicted -- a captured hipGraph holds only the raw pointer of the
#      tensor it read, so dropping one would hand its memory to the allocator while replays still read it
#      (``clear_constants`` is explicit and for processes that hold no graph); a constant is never CREATED while a
#      stream is capturing (its fill would be a node of that graph's private pool and eager callers would be handed an
#      unfilled tensor from the cache): create it in a warm-up pass; and the creating stream is synchronised once after
#      the fill, so a consumer on any other stream (side branches, a later capture stream) reads a finished tensor. ----
_CONSTANTS = {}


def constant(shape, value: float, device) -> Tensor:
    key = (str(torch.device(device)), tuple(int(d) for d in shape), float(value))
    t = _CONSTANTS.get(key)
    if t is None:
        if torch.cuda.is_current_stream_capturing():
            raise _lib.ScflowHipError(
                f'ops.constant{key[1]}: first use inside a stream capture -- run one eager warm-up pass of the same '
                f'shapes before capturing (scflow_amd.GraphedRefiner does, warmup >= 1)')
        t = torch.full(key[1], float(value), dtype=torch.float32, device=device)
        torch.cuda.current_stream(t.device).synchronize()
        _CONSTANTS[key] = t
    return t


def clear_constants() -> None:
    """drop the cached constant tensors.  ONLY when no captured graph that read one of them will be replayed again."""
    _CONSTANTS.clear()


# ---- K split across blocks for bias-free conv + GroupNorm blocks on small grids (the pose head's stride-2 layers) ----
_CONV_KSLICES = True


def set_conv_kslices(on: bool) -> bool:
    """False: ``conv_kslices`` answers 1 (every convolution contracts its whole K inside one block: the r4 arithmetic
    order); returns the previous setting.  Independent of the library's own automatic slicing of small grids
    (``tune('conv_autoslice', ..)``, which needs a registered workspace and is off unless a caller registers one)."""
    global _CONV_KSLICES
    prev, _CONV_KSLICES = _CONV_KSLICES, bool(on)
    return prev


def conv_kslices(pc: 'PackedConv', n: int, h: int, w: int) -> int:
    """WANTED slice count for ``conv2d(pc, x, kslices=...)`` of a bias-free layer whose consumer adds partial tensors
    (``conv_kslices_for`` = this, checked against the library for the actual tensors).
    A launch with few blocks is a serial chain of one memory round trip per staged channel chunk; S slices are S times
    the blocks and 1 / S of that chain.  Rule from ``tools/lab/kslice_sweep.py`` on the MI355X (kb = blocks of the
    32-channel x 32-pixel tile): kb < 128 -> 4 (11.8 -> 6.1 us, 18.0 -> 8.3), 128 <= kb < 512 -> 2 (4 can tip the
    launch onto the pixel-split tile: 11.9 -> 16.4 us), kb >= 512 -> 4 (64.2 -> 44.6, 31.8 -> 28.4); never more
    slices than 32-channel chunks.  NB the count depends on the batch size, so a sample's bits may differ between
    batch sizes (the partial sums re-associate); ``set_conv_kslices(False)`` is the batch-invariant setting."""
    if not _CONV_KSLICES or pc.bias is not None or pc.scale is not None or (pc.wp4 is None and pc.wp4s is None):
        return 1
    if _CONV_PRECISION == 'f16x3' and pc.wp16 is not None:
        return 1
    ho, wo = pc.out_hw(h, w)
    kb = n * ((ho * wo + 31) // 32) * ((pc.cout + 31) // 32)
    s = 2 if 128 <= kb < 512 else 4
    return max(1, min(s, pc.cin // 32))


def conv_kslices_for(pc: 'PackedConv', x0: Tensor, x1: Optional[Tensor] = None) -> int:
    """``conv_kslices`` validated by the library: an explicit ``k_slices`` launch only exists on the LDS-DMA
    dispatch, which refuses some layers outright (other strides than 1 / 2, a channel concat that splits a chunk, an
    ``S`` that leaves a slice without chunks, ...) -- the same layer unsliced would simply have run on another kernel.
    ``scf_conv2d_query`` is asked with the real descriptor, S halves until it says yes (1 = unsliced always works);
    the answer is cached per (shape, channel split, S)."""
    n, _, h, w = x0.shape
    s = conv_kslices(pc, n, h, w)
    if s <= 1:
        return 1
    c1 = 0 if x1 is None else x1.shape[1]
    key = ('ks', n, h, w, x0.shape[1], c1, s, _CONV_PRECISION, _CONV_WINOGRAD)
    if pc.plans is None:
        pc.plans = {}
    ok = pc.plans.get(key)
    if ok is None:
        lib = _lib.load()
        info = (C.c_int32 * 4)()
        ok = s
        while ok > 1:
            d, _ = conv2d(pc, x0, x1, kslices=ok, _launch=False)
            if lib.scf_conv2d_query(C.byref(d), info) == 0:
                break
            ok //= 2
        pc.plans[key] = ok = max(ok, 1)
    return ok


def _gru_passes(packs):
    arr = (_lib.GruPass * len(packs))()
    f16 = _CONV_PRECISION == 'f16x3'
    for g, (pzr, pq) in zip(arr, packs):
        g.KH, g.KW, g.pad_h, g.pad_w = pzr.kh, pzr.kw, pzr.pad_h, pzr.pad_w
        g.wp_zr, g.bias_zr = pzr.wp.data_ptr(), (None if pzr.bias is None else pzr.bias.data_ptr())
        g.wp_q, g.bias_q = pq.wp.data_ptr(), (None if pq.bias is None else pq.bias.data_ptr())
        if pzr.wp4 is not None and pq.wp4 is not None and pzr.g4 == pq.g4:
            g.wp_zr_a4, g.wp_q_a4, g.a4_groups = pzr.wp4.data_ptr(), pq.wp4.data_ptr(), pzr.g4
        if f16 and pzr.wp16 is not None and pq.wp16 is not None:
            g.wp_zr_f16, g.wp_q_f16 = pzr.wp16.data_ptr(), pq.wp16.data_ptr()
        if pzr.wp_alt is not None and pq.wp_alt is not None:
            g.wp_zr_k32, g.wp_q_k32 = pzr.wp_alt.data_ptr(), pq.wp_alt.data_ptr()
        if pzr.wp4s is not None and pq.wp4s is not None and pzr.g4s == pq.g4s:
            g.wp_zr_a4s, g.wp_q_a4s, g.a4s_groups = pzr.wp4s.data_ptr(), pq.wp4s.data_ptr(), pzr.g4s
        if pzr.wp4t is not None and pq.wp4t is not None and pzr.g4t == pq.g4t:
            g.wp_zr_a4t, g.wp_q_a4t, g.a4t_groups = pzr.wp4t.data_ptr(), pq.wp4t.data_ptr(), pzr.g4t
        if _CONV_WINOGRAD and not f16 and pzr.wwino1d is not None and pq.wwino1d is not None:
            g.wp_zr_wino1d, g.wp_q_wino1d = pzr.wwino1d.data_ptr(), pq.wwino1d.data_ptr()
            if pzr.wwino1d4 is not None and pq.wwino1d4 is not None:
                g.wp_zr_wino1d4, g.wp_q_wino1d4 = pzr.wwino1d4.data_ptr(), pq.wwino1d4.data_ptr()
    return arr


gru_passes = _gru_passes


def side_stream_handle() -> int:
    """raw handle of the side stream that belongs to (current device, current stream) -- the stream
    ``side_stream`` blocks run on; created on first use."""
    main = torch.cuda.current_stream()
    key = (torch.cuda.current_device(), main.cuda_stream)
    side = _SIDE.get(key)
    if side is None:
        side = _SIDE[key] = torch.cuda.Stream(device=key[0])
    return side.cuda_stream


def scflow_iteration(it: '_lib.ScflowIter') -> None:
    """one refinement iteration through ``scf_scflow_iteration`` (the struct is filled by
    ``SCFlowDecoder``).  With lookup timing enabled (bench.py) the lookup launch carries a timer."""
    lib = _lib.load()
    it.lookup_timer = _LOOKUP_TIMERS.take() if _LOOKUP_TIMERS is not None else None
    _lib.check(lib.scf_scflow_iteration(C.byref(it), _stream()), 'scf_scflow_iteration')


def sepconv_gru(packs, hx: Tensor, h_channels: int, z: Tensor, rh: Tensor,
                ctx: Optional[Sequence[Tensor]] = None, ctx_channels: int = 0) -> None:
    """ConvGRU.forward (raft_decoder.py:235-253) on hx = [h | x], h updated in place:
    ``scf_sepconv_gru``.  ``packs``: [(PackedConv of cat(conv_z, conv_r), PackedConv of conv_q)]
    per pass.  With ``ctx`` (one (N, 3 h_channels, H, W) tensor per pass) hx = [h | c | x'] and
    the packs cover [h | x'] only: ``scf_sepconv_gru_ctx`` (the c part of the convolutions, computed
    once per pair, enters before the gates' activations).  With convolution timers armed (bench.py)
    the same launches are issued one by one through ``conv2d`` so that each carries its own timer."""
    hc = h_channels
    if ctx is not None and (ctx_channels <= 0 or len(ctx) != len(packs)):
        raise _lib.ScflowHipError('sepconv_gru: one context term per pass, ctx_channels > 0')
    if _CONV_EVENTS is not None:
        hv, xv = hx[:, :hc], hx[:, hc + ctx_channels:]
        for i, (pzr, pq) in enumerate(packs):
            if ctx is None:
                conv2d(pzr, hx, out=z, mode=CONV_GRU_ZR, gru_h=hv, gru_aux=rh)
                conv2d(pq, rh, xv, out=hv, mode=CONV_GRU_Q, gru_h=hv, gru_z=z)
            else:
                conv2d(pzr, hv, xv, out=z, mode=CONV_GRU_ZR, gru_h=hv, gru_aux=rh, res=ctx[i][:, :2 * hc])
                conv2d(pq, rh, xv, out=hv, mode=CONV_GRU_Q, gru_h=hv, gru_z=z, res=ctx[i][:, 2 * hc:])
        return
    p, n, c, h, w, sn = _nchw(hx, 'hx')
    arr = _gru_passes(packs)
    if ctx is None:
        _lib.check(_lib.load().scf_sepconv_gru(p, sn, n, hc, c - hc, h, w, arr, len(packs),
                                               _dense(z, 'z'), _dense(rh, 'rh'), _stream()),
                   'scf_sepconv_gru')
        return
    ptrs, cs = (C.c_void_p * len(ctx))(), None
    for i, t in enumerate(ctx):
        pc_, nc, cc_, hh, ww, s_ = _nchw(t, 'ctx')
        if (nc, cc_, hh, ww) != (n, 3 * hc, h, w) or (cs is not None and s_ != cs):
            raise _lib.ScflowHipError('sepconv_gru: ctx must be (N, 3*h_channels, H, W), equal strides')
        ptrs[i], cs = pc_, s_
    _lib.check(_lib.load().scf_sepconv_gru_ctx(p, sn, n, hc, ctx_channels, c - hc - ctx_channels, h, w,
                                               arr, len(packs), ptrs, cs, _dense(z, 'z'),
                                               _dense(rh, 'rh'), _stream()),
               'scf_sepconv_gru_ctx')


def _read_timers(timers):
    lib = _lib.load()
    out = []
    for tm in timers:
        us = C.c_float()
        _lib.check(lib.scf_timer_elapsed_us(tm, C.byref(us)), 'scf_timer_elapsed_us')
        lib.scf_timer_destroy(tm)
        out.append(float(us.value))
    return out


def conv_timing(enable: bool):
    """like ``lookup_timing`` for the convolution launches: enable=False returns a list of
    (microseconds, algorithmic flops = 2*Cin*KH*KW*Cout*Ho*Wo*N, shape tag) per launch; the tag ends in
    ' [winograd]' when the F(2x2, 3x3) kernel ran the launch (it executes 1 / 2.25 of those flops), in
    ' [winograd F(2,5)]' / ' [winograd F(4,5)]' for the 1x5 / 5x1 kernels (1 / 1.667, 1 / 2.5)."""
    global _CONV_EVENTS
    if enable:
        _CONV_EVENTS = []
        return None
    evs, _CONV_EVENTS = _CONV_EVENTS or [], None
    torch.cuda.synchronize()
    return list(zip(_read_timers([e[0] for e in evs]), [e[1] for e in evs], [e[2] for e in evs]))


TUNE_KEYS = {'wino_variant': 1, 'dma_force_ksplit': 2, 'dma_ksplit_groups': 3, 'wino1d4': 4, 'lookup_pipe': 5, 'lookup_store': 6, 'conv_autoslice': 7, 'iter_merge': 8, 'wino1d4_half': 9, 'conv_pair': 10}


def tune(key: str, value: int) -> int:
    """measurement knob of the library (``scf_tune``, scflow_hip_prof.h): returns the previous value.
    ``'wino_variant'``: 0 = the dispatch's choice, 1 = pair kernel, 2 = quarter-domain kernel (3 / 4 / 5 exist in lab builds
    of the library only; the product library refuses them);
    ``'wino1d4'``: 1 = F(4, 5) where the dispatch prefers it (default), 0 = never, 2 = on every grid it supports;
    ``'lookup_pipe'``: 0 = the dispatch's choice, 1 = one group per block (r3 kernel), 2 / 3 = pipelined kernel with
    that many groups per block, 4 / 5 / 6 = two / four / three groups per block (same waves, fewer workgroups).  Unknown keys raise ``ValueError``; a value the library refuses raises
    ``RuntimeError`` (the return value is always a previous setting, never an error code)."""
    if key not in TUNE_KEYS:
        raise ValueError(f'unknown tune key {key!r}; known: {sorted(TUNE_KEYS)}')
    prev = int(_lib.load().scf_tune(TUNE_KEYS[key], int(value)))
    if prev < 0:
        _lib.check(prev, f'scf_tune({key}, {value})')
    return prev


class record_conv_kernels:
    """``with ops.record_conv_kernels() as ran: ...`` -- afterwards ``ran`` is a list of
    ``(layer tag, kernel family)`` for every convolution launch the library made inside the block, in
    launch order, INCLUDING those issued inside ``scf_sepconv_gru*`` / ``scf_scflow_iteration``
    (``scf_conv_log_*`` of scflow_hip_prof.h).  Tag = ``'<Cin>-><Cout> <KH>x<KW>/s<stride> @<Ho>x<Wo> N<N>'``
    (the tag ``conv_timing`` uses), family = one of ``_lib.KERNEL_NAMES``' values.  Parity tests assert with
    it that the kernel they name really ran (the choice depends on grid size and device).  The recorder's ``paired`` lists,
    launch by launch, how ``scf_conv2d_pair`` ran it: 0 = its own launch, 1 / 2 = first / second layer of one merged launch;
    ``variants`` the instantiation a merged launch ran each of its layers with (``scf_conv_log_entry.variant``, -1 otherwise)."""

    _active = False      # the library keeps ONE process-wide log: a nested recorder would clear the outer one's records

    def __init__(self, capacity: int = 1 << 16) -> None:
        self.capacity, self.ran, self.paired, self.variants = capacity, [], [], []

    def __enter__(self):
        if record_conv_kernels._active:
            raise RuntimeError('record_conv_kernels does not nest (one process-wide dispatch log)')
        _lib.check(_lib.load().scf_conv_log_enable(self.capacity), 'scf_conv_log_enable')
        record_conv_kernels._active = True
        return self.ran

    def __exit__(self, *exc):
        record_conv_kernels._active = False
        lib = _lib.load()
        n = lib.scf_conv_log_read(None, 0)
        buf = (_lib.ConvLogEntry * max(n, 1))()
        n = min(lib.scf_conv_log_read(buf, n), n)
        lib.scf_conv_log_enable(0)
        for e in buf[:n]:
            self.ran.append((f'{e.Cin}->{e.Cout} {e.KH}x{e.KW}/s{e.stride} @{e.Ho}x{e.Wo} N{e.N}',
                             _lib.KERNEL_NAMES.get(e.kernel, str(e.kernel))))
            self.paired.append(e.paired)
            self.variants.append(e.variant)
        return False


def time_first_kernel(fn) -> float:
    """run ``fn()`` with a launch-bound timer armed: microseconds of the FIRST kernel it launches
    through the library (e.g. the contraction of ``corr_build``, not its pooling cascade)."""
    lib = _lib.load()
    tm = C.c_void_p()
    _lib.check(lib.scf_timer_create(C.byref(tm)), 'scf_timer_create')
    lib.scf_timer_arm(tm)
    try:
        fn()
    finally:
        lib.scf_timer_arm(None)
    torch.cuda.synchronize()
    return _read_timers([tm])[0]


# ----------------------------------------------------- correlation volume
def pyramid_layout(h: int, w: int, radius: int = 4, num_levels: int = 4) -> int:
    """the pyramid layout the lookup kernel is fastest with: bit l set = level l stored in 8x4-float
    tiles of 128 B (``scf_corr_preferred_layout``: every level whose rows are >= 24 floats and that
    does not fit the lookup window whole).  0 = the reference's row-major pyramid."""
    return int(_lib.load().scf_corr_preferred_layout(h, w, radius, num_levels))


def level_storage_shape(h: int, w: int, level: int, tiled: bool) -> Tuple[int, int]:
    """(rows, cols) a query's level-``level`` map occupies: the map itself, or -- tiled -- the map
    padded to 4 rows x 8 columns."""
    lh, lw = h >> level, w >> level
    return ((lh + 3) // 4 * 4, (lw + 7) // 8 * 8) if tiled else (lh, lw)


def untile_level(level: Tensor, lh: int, lw: int) -> Tensor:
    """torch view-shuffle of a tiled pyramid level (q, 1, PH, PW) back to the reference's row-major
    (q, 1, lh, lw) (tests / debugging only; the hot path never untiles)."""
    q, _, ph, pw = level.shape
    return (level.reshape(q, ph // 4, pw // 8, 4, 8).permute(0, 1, 3, 2, 4).reshape(q, 1, ph, pw)
            [:, :, :lh, :lw].contiguous())


def untile_level0(level0: Tensor) -> Tensor:
    return untile_level(level0, level0.shape[-2], level0.shape[-1])


def _pyramid_shapes(n: int, h: int, w: int, num_levels: int, tiled_levels: int):
    return [(n * h * w, 1, *level_storage_shape(h, w, l, bool((tiled_levels >> l) & 1)))
            for l in range(num_levels)]


def corr_build(feat1: Tensor, feat2: Tensor, num_levels: int = 4,
               out: Optional[List[Tensor]] = None, tiled_levels: int = 0) -> List[Tensor]:
    """CorrelationPyramid.forward (raft_decoder.py:35-58) -> list of (N*h*w, 1, h>>l, w>>l).
    ``tiled_levels`` (bit mask, see ``pyramid_layout``): those levels are stored in 128-byte 8x4
    tiles for the lookup -- same values, permuted inside each query's map, the map padded to 4 rows x
    8 columns (``level_storage_shape``); pass the same mask to ``corr_lookup``."""
    p1 = _dense(feat1, 'feat1')
    p2 = _dense(feat2, 'feat2')
    if feat1.shape != feat2.shape or feat1.dim() != 4:
        raise _lib.ScflowHipError('feat1/feat2 must be equal-shape NCHW')
    n, c, h, w = feat1.shape
    shapes = _pyramid_shapes(n, h, w, num_levels, tiled_levels)
    if out is None:
        out = [torch.empty(sh, dtype=torch.float32, device=feat1.device) for sh in shapes]
    for l, (t, sh) in enumerate(zip(out, shapes)):
        if tuple(t.shape) != sh:
            raise _lib.ScflowHipError(f'pyramid level {l} has shape {tuple(t.shape)}, expected {sh}')
    arr = (C.c_void_p * num_levels)(*[_dense(t, 'level') for t in out])
    lib = _lib.load()
    timed = _CORR_TIMERS is not None      # bench.py: a timer bound to the FIRST launch = the contraction
    if timed:
        lib.scf_timer_arm(_CORR_TIMERS.take())
    try:
        _lib.check(lib.scf_corr_build_ex(p1, p2, arr, n, c, h, w, num_levels, int(tiled_levels),
                                         _stream()), 'scf_corr_build')
    finally:
        if timed:
            lib.scf_timer_arm(None)
    return out


def corr_lookup(pyramid: Sequence[Tensor], flow: Tensor, radius: int = 4,
                out: Optional[Tensor] = None, tiled_levels: int = 0) -> Tensor:
    """CorrLookup.forward (corr_lookup.py:102-136) -> (N, L*(2r+1)^2, h, w)."""
    pf = _dense(flow, 'flow')
    n, two, h, w = flow.shape
    if two != 2:
        raise _lib.ScflowHipError('flow must be (N,2,h,w)')
    L = len(pyramid)
    for l, (lv, sh) in enumerate(zip(pyramid, _pyramid_shapes(n, h, w, L, tiled_levels))):
        if tuple(lv.shape) != sh:
            raise _lib.ScflowHipError(f'pyramid level {l} has shape {tuple(lv.shape)}, expected {sh}')
    k = L * (2 * radius + 1) ** 2
    if out is None:
        out = torch.empty((n, k, h, w), dtype=torch.float32, device=flow.device)
    arr = (C.c_void_p * L)(*[_dense(t, 'level') for t in pyramid])
    lib = _lib.load()
    timed = _LOOKUP_TIMERS is not None      # bench.py: a HIP start/stop event pair bound to this launch
    if timed:
        lib.scf_timer_arm(_LOOKUP_TIMERS.take())
    try:
        _lib.check(lib.scf_corr_lookup_ex(arr, pf, _dense(out, 'out'), n, h, w, radius, L,
                                          int(tiled_levels), _stream()), 'scf_corr_lookup')
    finally:
        if timed:
            lib.scf_timer_arm(None)
    return out


def corr_lookup_grad(g_corr: Tensor, flow: Tensor, mask: Optional[Tensor] = None, radius: int = 4, num_levels: int = 4,
                     out: Optional[Tensor] = None, accumulate: bool = False) -> Tensor:
    """Adjoint of ``corr_lookup`` with respect to the pyramid, folded through the average pools to level 0
    (``scf_corr_lookup_grad``): ``g_corr`` (T, N, L (2r+1)^2, h, w), the cotangents of the lookup outputs of T iterations;
    ``flow`` (T, N, 2, h, w), the flow of each lookup; ``mask`` None or (T, N, 1, h, w), a per-query factor on ``g_corr``
    -> ``g_vol`` (N h w, h, w), d loss / d level 0 summed over T, every element written; ``accumulate``: added to
    ``out``.  A single iteration may be passed without the leading axis.  The order of every sum is the header's."""
    what = 'corr_lookup_grad'
    if isinstance(g_corr, torch.Tensor) and g_corr.dim() == 4:
        g_corr, flow = g_corr.unsqueeze(0), flow.unsqueeze(0) if isinstance(flow, torch.Tensor) and flow.dim() == 4 else flow
        mask = mask.unsqueeze(0) if isinstance(mask, torch.Tensor) and mask.dim() == 4 else mask
    pg = _dense(g_corr, f'{what}: g_corr')
    pf = _dense(flow, f'{what}: flow')
    if g_corr.dim() != 5 or flow.dim() != 5 or flow.shape[2] != 2:
        raise _lib.ScflowHipError(f'{what}: g_corr (T, N, K, h, w) and flow (T, N, 2, h, w), got {tuple(g_corr.shape)} and '
                                  f'{tuple(flow.shape)}')
    T, n, k, h, w = g_corr.shape
    if radius < 1 or num_levels < 1 or num_levels > _lib.MAX_LEVELS:
        raise _lib.ScflowHipError(f'{what}: radius >= 1 and 1 .. {_lib.MAX_LEVELS} levels, got {radius} and {num_levels}')
    if T == 0 or T > TAIL_MAX_T or n * h * w == 0:
        raise _lib.ScflowHipError(f'{what}: 1 .. {TAIL_MAX_T} iterations of non-empty maps, got {tuple(g_corr.shape)}')
    if k != num_levels * (2 * radius + 1) ** 2 or tuple(flow.shape) != (T, n, 2, h, w):
        raise _lib.ScflowHipError(f'{what}: g_corr must hold {num_levels * (2 * radius + 1) ** 2} channels and flow be '
                                  f'{(T, n, 2, h, w)}, got {tuple(g_corr.shape)} and {tuple(flow.shape)}')
    if (h >> (num_levels - 1)) == 0 or (w >> (num_levels - 1)) == 0:
        raise _lib.ScflowHipError(f'{what}: level {num_levels - 1} of a {h} x {w} map is empty')
    pm = None
    if mask is not None:
        pm = _dense(mask, f'{what}: mask')
        if tuple(mask.shape) != (T, n, 1, h, w):
            raise _lib.ScflowHipError(f'{what}: mask must be {(T, n, 1, h, w)}, got {tuple(mask.shape)}')
    shape = (n * h * w, h, w)
    if out is None:
        if accumulate:
            raise _lib.ScflowHipError(f'{what}: accumulate needs out')
        out = torch.empty(shape, dtype=torch.float32, device=g_corr.device)
    po = _dense(out, f'{what}: out')
    if tuple(out.shape) != shape:
        raise _lib.ScflowHipError(f'{what}: out must be {shape}, got {tuple(out.shape)}')
    _lib.check(_lib.load().scf_corr_lookup_grad(pg, pf, pm, po, int(bool(accumulate)), T, n, h, w, radius, num_levels,
                                                _stream()), 'scf_corr_lookup_grad')
    return out


def corr_lookup_grad_route(n: int, h: int, w: int, radius: int = 4, num_levels: int = 4) -> dict:
    """what ``corr_lookup_grad`` launches for these sizes (``scf_corr_lookup_grad_route``, the launcher's own decision; a
    host call) -> dict(route 'fast' | 'plain', radius: the kernel's template radius (0 on the plain route), qb_log2: log2
    of the queries per block (-1 on the plain route), ragged: the last block holds fewer queries)."""
    r = (C.c_int * 4)()
    _lib.check(_lib.load().scf_corr_lookup_grad_route(int(n), int(h), int(w), int(radius), int(num_levels), r),
               'scf_corr_lookup_grad_route')
    return dict(route=('fast', 'plain')[r[0]], radius=int(r[1]), qb_log2=int(r[2]), ragged=bool(r[3]))


def corr_build_grad(g_vol: Tensor, feat1: Tensor, feat2: Tensor, out: Optional[Sequence[Optional[Tensor]]] = None
                    ) -> Tuple[Tensor, Tensor]:
    """Adjoint of ``corr_build``'s level 0 with respect to the two feature maps (``scf_corr_build_grad``): ``g_vol``
    (N h w, h, w) or (N, h w, h w), d loss / d level 0 row-major as ``corr_lookup_grad`` writes it; ``feat1`` (the queries,
    render) and ``feat2`` (the targets, real) (N, C, h, w) -> ``(g_feat1, g_feat2)``, both (N, C, h, w).  ``out``: a pair
    of destinations (None entries are allocated) -- the two halves of one (2N, C, h, w) buffer are what the shared encoder's
    backward takes.  Every argument contiguous; the outputs alias neither each other nor an input.  The order of every
    sum is the header's."""
    what = 'corr_build_grad'
    pf1 = _dense(feat1, f'{what}: feat1')
    pf2 = _dense(feat2, f'{what}: feat2')
    pg = _dense(g_vol, f'{what}: g_vol')
    if feat1.dim() != 4 or feat1.numel() == 0:
        raise _lib.ScflowHipError(f'{what}: feat1 must be a non-empty (N, C, h, w) tensor, got {tuple(feat1.shape)}')
    shape = tuple(feat1.shape)
    n, c, h, w = shape
    if tuple(feat2.shape) != shape:
        raise _lib.ScflowHipError(f'{what}: feat2 must be {shape} like feat1, got {tuple(feat2.shape)}')
    if tuple(g_vol.shape) not in ((n * h * w, h, w), (n, h * w, h * w)):
        raise _lib.ScflowHipError(f'{what}: g_vol must be {(n * h * w, h, w)} or {(n, h * w, h * w)}, got '
                                  f'{tuple(g_vol.shape)}')
    outs = [None, None] if out is None else ([out] if isinstance(out, torch.Tensor) else list(out))
    if len(outs) != 2:
        raise _lib.ScflowHipError(f'{what}: out holds the pair (g_feat1, g_feat2), got {len(outs)} destination(s)')
    outs = [torch.empty(shape, dtype=torch.float32, device=feat1.device) if o is None else o for o in outs]
    po = []
    for i, o in enumerate(outs):
        po.append(_dense(o, f'{what}: out[{i}]'))
        if tuple(o.shape) != shape:
            raise _lib.ScflowHipError(f'{what}: out[{i}] must be {shape}, got {tuple(o.shape)}')
    spans = [(f'out[{i}]', p, feat1.numel()) for i, p in enumerate(po)]
    spans += [('feat1', pf1, feat1.numel()), ('feat2', pf2, feat2.numel()), ('g_vol', pg, g_vol.numel())]
    for i in range(2):
        for name, p, numel in spans[i + 1:]:
            if po[i] < p + 4 * numel and p < po[i] + 4 * feat1.numel():
                raise _lib.ScflowHipError(f'{what}: out[{i}] overlaps {name}')
    _lib.check(_lib.load().scf_corr_build_grad(pg, pf1, pf2, po[0], po[1], n, c, h, w, _stream()), 'scf_corr_build_grad')
    return outs[0], outs[1]


class _TimerPool:
    """launch-bound timers (scf_timer_*), created up front so that a timed loop only takes one
    from the pool; ``read()`` returns the durations of the timers used since the last reset."""

    def __init__(self, reserve: int) -> None:
        self.timers, self.used = [], 0
        self._grow(max(int(reserve), 1))

    def _grow(self, n: int) -> None:
        lib = _lib.load()
        for _ in range(n):
            tm = C.c_void_p()
            _lib.check(lib.scf_timer_create(C.byref(tm)), 'scf_timer_create')
            self.timers.append(tm)

    def take(self):
        if self.used == len(self.timers):     # pool exhausted: grow (outside the fast path by design)
            self._grow(len(self.timers))
        tm = self.timers[self.used]
        self.used += 1
        return tm

    def read(self):
        lib = _lib.load()
        out = []
        for tm in self.timers[:self.used]:
            us = C.c_float()
            _lib.check(lib.scf_timer_elapsed_us(tm, C.byref(us)), 'scf_timer_elapsed_us')
            out.append(float(us.value))
        return out

    def reset(self) -> None:
        self.used = 0

    def destroy(self) -> None:
        lib = _lib.load()
        for tm in self.timers:
            lib.scf_timer_destroy(tm)
        self.timers, self.used = [], 0


_LOOKUP_TIMERS: Optional[_TimerPool] = None
_CORR_TIMERS: Optional[_TimerPool] = None


def corr_build_timing(enable: bool, reserve: int = 16):
    """like ``lookup_timing`` for the correlation build: every ``corr_build`` call from now on carries a
    timer bound to its first kernel launch -- the contraction (with the layout the decoders use: the
    GEMM with the fused first pool, ``corr_gemm_kernel<true, true>``), not the pooling cascade behind
    it.  enable=False: stop, synchronise, return the durations in microseconds."""
    global _CORR_TIMERS
    if enable:
        if _CORR_TIMERS is not None:
            _CORR_TIMERS.destroy()
        _CORR_TIMERS = _TimerPool(reserve)
        return None
    pool, _CORR_TIMERS = _CORR_TIMERS, None
    if pool is None:
        return []
    torch.cuda.synchronize()
    out = pool.read()
    pool.destroy()
    return out


def corr_build_timing_reset() -> None:
    if _CORR_TIMERS is not None:
        torch.cuda.synchronize()
        _CORR_TIMERS.reset()


def corr_build_timing_read():
    if _CORR_TIMERS is None:
        return []
    torch.cuda.synchronize()
    return _CORR_TIMERS.read()


def lookup_timing(enable: bool, reserve: int = 64):
    """enable=True: every corr-lookup launch from now on carries a timer (HIP start / stop events
    bound to the launch on its stream: the kernel's own duration); ``reserve`` timers are created
    now, before any timed loop.  enable=False: stop, synchronise and return the per-launch
    durations in microseconds since the last ``lookup_timing_reset``."""
    global _LOOKUP_TIMERS
    if enable:
        if _LOOKUP_TIMERS is not None:
            _LOOKUP_TIMERS.destroy()
        _LOOKUP_TIMERS = _TimerPool(reserve)
        return None
    pool, _LOOKUP_TIMERS = _LOOKUP_TIMERS, None
    if pool is None:
        return []
    torch.cuda.synchronize()
    out = pool.read()
    pool.destroy()
    return out


def lookup_timing_reset() -> None:
    """forget the launches recorded so far (the timers are reused)."""
    if _LOOKUP_TIMERS is not None:
        torch.cuda.synchronize()
        _LOOKUP_TIMERS.reset()


def lookup_timing_read():
    """synchronise and return the durations (us) recorded since the last reset."""
    if _LOOKUP_TIMERS is None:
        return []
    torch.cuda.synchronize()
    return _LOOKUP_TIMERS.read()


# ------------------------------------------------------------- norms etc.
def instance_norm(x: Tensor, res: Optional[Tensor] = None, relu: bool = False,
                  out: Optional[Tensor] = None, eps: float = 1e-5, res_norm: bool = False) -> Tensor:
    """``relu?(IN(x) + res?)``.  ``res_norm``: ``res`` is normalised too, ``relu?(IN(x) + IN(res))`` -- the tail of a residual
    block with a shortcut convolution, one pass over both for planes of up to 128 x 128 (``scf_instance_norm_res_norm``); the
    bits are those of ``instance_norm(res, out=res)`` followed by ``instance_norm(x, res=res)``, and ``res`` is scratch."""
    px = _dense(x, 'x')
    n, c, h, w = x.shape
    if out is None:
        out = torch.empty_like(x)
    if res_norm:
        if res is None or res.shape != x.shape:
            raise ValueError('instance_norm(res_norm=True): res of the shape of x')
        _lib.check(_lib.load().scf_instance_norm_res_norm(px, _dense(res, 'res'), _dense(out, 'out'), n * c, h * w, eps,
                                                          int(relu), _stream()), 'scf_instance_norm_res_norm')
        return out
    _lib.check(_lib.load().scf_instance_norm(px, _opt(res, 'res'), _dense(out, 'out'), n * c,
                                             h * w, eps, int(relu), _stream()),
               'scf_instance_norm')
    return out


def group_norm_relu(x: Tensor, gamma: Tensor, beta: Tensor, groups: int, eps: float = 1e-5,
                    out: Optional[Tensor] = None) -> Tensor:
    """GroupNorm(groups, eps, affine) + ReLU of an (N, C, H, W) map, or of the (S, N, C, H, W) partial sums of
    ``conv2d(..., kslices=S)`` (added in slice order inside the kernel) -> (N, C, H, W)."""
    px = _dense(x, 'x')
    parts, pstride = 1, 0
    if x.dim() == 5:
        parts, pstride = x.shape[0], x.stride(0)
        x = x[0]
    n, c, h, w = x.shape
    if out is None:
        out = torch.empty_like(x)
    _lib.check(_lib.load().scf_group_norm_relu_parts(px, parts, pstride, _dense(gamma, 'gamma'), _dense(beta, 'beta'),
                                                     _dense(out, 'out'), n, c, h * w, groups, eps,
                                                     _stream()), 'scf_group_norm_relu')
    return out


def _fc_weight(weight: Tensor, k: int, bias: Optional[Tensor], what: str) -> int:
    """out_features of a 2-D (O, k) weight whose optional bias has O entries: the kernels index both by these sizes."""
    if weight.dim() != 2 or weight.shape[1] != k:
        raise _lib.ScflowHipError(f'{what}: weight must be 2-D (out_features, {k}), got {tuple(weight.shape)}')
    _fc_vector(bias, weight.shape[0], what, 'bias')
    return weight.shape[0]


def _fc_vector(t: Optional[Tensor], n: int, what: str, name: str, at_least: bool = False) -> None:
    if t is not None and (t.numel() < n if at_least else t.numel() != n):
        raise _lib.ScflowHipError(f'{what}: {name} has {t.numel()} entries, the kernel reads {n}')


def linear(x: Tensor, weight: Tensor, bias: Optional[Tensor], act: int = ACT_NONE,
           out: Optional[Tensor] = None) -> Tensor:
    px = _dense(x, 'x')
    if x.dim() != 2:
        raise _lib.ScflowHipError('linear: x must be (N, K)')
    n, k = x.shape
    o = _fc_weight(weight, k, bias, 'linear')
    if out is None:
        out = torch.empty((n, o), dtype=torch.float32, device=x.device)
    elif out.shape != (n, o):
        raise _lib.ScflowHipError(f'linear: out must be ({n}, {o}), got {tuple(out.shape)}')
    _lib.check(_lib.load().scf_linear(px, _dense(weight, 'weight'), _opt(bias, 'bias'),
                                      _dense(out, 'out'), n, k, o, act, _stream()), 'scf_linear')
    return out


def fc_slices(k: int) -> int:
    """K-slices ``fc_splitk`` is given for an input of ``k`` features: 256 features per slice (one block tile's
    worth of LDS) where K allows it, else 0 = the shape does not fit (callers use ``linear``)."""
    if k % 8 == 0 and k <= 256:
        return 1
    return k // 256 if k % 256 == 0 else 0


def fc_splitk(x: Tensor, weight: Tensor, bias: Optional[Tensor] = None, *, x_bias: Optional[Tensor] = None,
              x_relu: bool = False, gn=None, weight2: Optional[Tensor] = None, bias2: Optional[Tensor] = None,
              act: int = ACT_NONE, slices: int = 1):
    """nn.Linear as a split-K MFMA GEMM with fused neighbours (``scf_fc_splitk``).  ``x``: (N, K), or
    (parts, N, K) partial sums of a previous ``fc_splitk(..., slices=parts)`` whose bias / ReLU this call applies
    (``x_bias``, ``x_relu``); ``gn`` = (groups, hw, gamma, beta, eps): GroupNorm + affine + ReLU over the features
    first (the flattened (C, h, w) map of the pose head, hw = h * w).  ``slices`` > 1: returns (slices, N, O)
    partial sums (no bias / act); 1: the finished (N, O) [and (N, O2) for ``weight2``]."""
    _dev(x, 'x')
    if x.dim() == 2:
        x = x.unsqueeze(0)
    if x.dim() != 3 or not x.is_contiguous():
        raise _lib.ScflowHipError('fc_splitk: x must be a contiguous (N, K) or (parts, N, K) tensor')
    parts, n, k = x.shape
    o = _fc_weight(weight, k, bias, 'fc_splitk')
    if weight2 is not None:
        _fc_weight(weight2, k, bias2, 'fc_splitk (weight2)')
    _fc_vector(x_bias, k, 'fc_splitk', 'x_bias')
    d = _lib.FcDesc()
    d.x, d.x_parts, d.x_part_stride = x.data_ptr(), parts, n * k
    d.x_bias, d.x_relu = _opt(x_bias, 'x_bias'), int(bool(x_relu))
    if gn is not None:
        groups, hw, gamma, beta, eps = gn
        if hw <= 0:
            raise _lib.ScflowHipError('fc_splitk: gn hw must be positive')
        _fc_vector(gamma, -(-k // hw), 'fc_splitk', 'gamma', at_least=True)       # channel of feature f: f // hw
        _fc_vector(beta, -(-k // hw), 'fc_splitk', 'beta', at_least=True)
        d.gn_groups, d.gn_hw, d.gn_gamma, d.gn_beta, d.gn_eps = groups, hw, _dense(gamma, 'gamma'), _dense(beta, 'beta'), eps
    d.N, d.K = n, k
    y = torch.empty((slices, n, o) if slices > 1 else (n, o), dtype=torch.float32, device=x.device)
    d.W, d.bias, d.y, d.O = _dense(weight, 'weight'), _opt(bias, 'bias'), y.data_ptr(), o
    y2 = None
    if weight2 is not None:
        y2 = torch.empty((n, weight2.shape[0]), dtype=torch.float32, device=x.device)
        d.W2, d.bias2, d.y2, d.O2 = _dense(weight2, 'weight2'), _opt(bias2, 'bias2'), y2.data_ptr(), weight2.shape[0]
    d.act, d.slices = act, slices
    _lib.check(_lib.load().scf_fc_splitk(C.byref(d), _stream()), 'scf_fc_splitk')
    return y if y2 is None else (y, y2)


def linear_pair(x: Tensor, w1: Tensor, b1: Optional[Tensor], w2: Tensor, b2: Optional[Tensor],
                act: int = ACT_NONE) -> Tuple[Tensor, Tensor]:
    """(linear(x, w1, b1), linear(x, w2, b2)) in one launch (scf_linear_pair)."""
    px = _dense(x, 'x')
    if x.dim() != 2:
        raise _lib.ScflowHipError('linear_pair: x must be (N, K)')
    n, k = x.shape
    _fc_weight(w1, k, b1, 'linear_pair (w1)')
    _fc_weight(w2, k, b2, 'linear_pair (w2)')
    y1 = torch.empty((n, w1.shape[0]), dtype=torch.float32, device=x.device)
    y2 = torch.empty((n, w2.shape[0]), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().scf_linear_pair(px, _dense(w1, 'w1'), _opt(b1, 'b1'), y1.data_ptr(),
                                           w1.shape[0], _dense(w2, 'w2'), _opt(b2, 'b2'),
                                           y2.data_ptr(), w2.shape[0], n, k, act, _stream()),
               'scf_linear_pair')
    return y1, y2


def pose_update(rot_all: Tensor, trans_all: Tensor, label: Tensor, num_class: int,
                rot: Tensor, trans: Tensor, label_mode: int = 0):
    """-> (d_rot (N,6), d_trans (N,3), R' (N,3,3), t' (N,3))."""
    n = rot_all.shape[0]
    if not label.is_cuda or label.dtype != torch.int64 or not label.is_contiguous():
        raise _lib.ScflowHipError('label must be a contiguous int64 GPU tensor')
    dev = rot_all.device
    d_rot = torch.empty((n, 6), dtype=torch.float32, device=dev)
    d_trans = torch.empty((n, 3), dtype=torch.float32, device=dev)
    r_out = torch.empty((n, 3, 3), dtype=torch.float32, device=dev)
    t_out = torch.empty((n, 3), dtype=torch.float32, device=dev)
    _lib.check(_lib.load().scf_pose_update(
        _dense(rot_all, 'rot_all'), _dense(trans_all, 'trans_all'), label.data_ptr(), num_class,
        label_mode, _dense(rot, 'rot'), _dense(trans, 'trans'), d_rot.data_ptr(),
        d_trans.data_ptr(), r_out.data_ptr(), t_out.data_ptr(), n, _stream()), 'scf_pose_update')
    return d_rot, d_trans, r_out, t_out


def reproject_flow(depth: Tensor, k: Tensor, rot0: Tensor, trans0: Tensor, rot: Tensor,
                   trans: Tensor, invalid_num: float = 0., out: Optional[Tensor] = None) -> Tensor:
    n, h, w = depth.shape
    if out is None:
        out = torch.empty((n, 2, h, w), dtype=torch.float32, device=depth.device)
    _lib.check(_lib.load().scf_reproject_flow(
        _dense(depth, 'depth'), _dense(k, 'k'), _dense(rot0, 'rot0'), _dense(trans0, 'trans0'),
        _dense(rot, 'rot'), _dense(trans, 'trans'), _dense(out, 'out'), n, h, w,
        float(invalid_num), _stream()), 'scf_reproject_flow')
    return out


def filter_flow_by_mask_(flow: Tensor, mask: Tensor, invalid_num: float = 400.,
                         align_corners: bool = False) -> Tensor:
    """in-place ``filter_flow_by_mask`` (utils/flow.py:6-26); flow (N,2,H,W), mask (N,H,W)."""
    n, two, h, w = flow.shape
    if two != 2 or tuple(mask.shape) != (n, h, w):
        raise _lib.ScflowHipError('filter_flow_by_mask: flow (N,2,H,W), mask (N,H,W)')
    _lib.check(_lib.load().scf_filter_flow_by_mask(_dense(flow, 'flow'), _dense(mask, 'mask'), n, h, w,
                                                   float(invalid_num), int(align_corners), _stream()),
               'scf_filter_flow_by_mask')
    return flow


def _mats(t: Tensor, n: int, shape: Tuple[int, ...], name: str) -> int:
    if tuple(t.shape) != (n, *shape):
        raise _lib.ScflowHipError(f'{name}: expected shape {(n, *shape)}, got {tuple(t.shape)}')
    return _dense(t, name)


def flow_corr_2d3d(flow: Tensor, depth: Tensor, k: Tensor, rot0: Tensor, trans0: Tensor,
                   occlusion: Optional[Tensor] = None, occ_thresh: float = 0.5):
    """``get_2d_3d_corr_by_fw_flow`` (models/utils/pose.py:182-200) for the whole batch in one launch.

    flow (N,2,H,W), depth (N,H,W), k / rot0 (N,3,3), trans0 (N,3), occlusion (N,H,W) or None ->
    (pts2d (N,H*W,2), pts3d (N,H*W,3), conf (N,H*W), count (N,) int32): sample n's first count[n] rows are its
    pixels with depth > 0 (and occlusion > occ_thresh) in row-major order; pts2d is the flow's target point, pts3d
    the object-frame point, conf the occlusion value (1 without one).  Rows past count[n] are unspecified."""
    if depth.dim() != 3:
        raise _lib.ScflowHipError('flow_corr_2d3d: depth must be (N,H,W)')
    n, h, w = depth.shape
    if tuple(flow.shape) != (n, 2, h, w):
        raise _lib.ScflowHipError(f'flow_corr_2d3d: flow must be {(n, 2, h, w)}, got {tuple(flow.shape)}')
    if occlusion is not None and tuple(occlusion.shape) != (n, h, w):
        raise _lib.ScflowHipError(f'flow_corr_2d3d: occlusion must be {(n, h, w)}, got {tuple(occlusion.shape)}')
    dev = depth.device
    pts2d = torch.empty((n, h * w, 2), dtype=torch.float32, device=dev)
    pts3d = torch.empty((n, h * w, 3), dtype=torch.float32, device=dev)
    conf = torch.empty((n, h * w), dtype=torch.float32, device=dev)
    count = torch.empty((n,), dtype=torch.int32, device=dev)
    _lib.check(_lib.load().scf_flow_corr_2d3d(
        _dense(flow, 'flow'), _dense(depth, 'depth'), _opt(occlusion, 'occlusion'), float(occ_thresh),
        _mats(k, n, (3, 3), 'k'), _mats(rot0, n, (3, 3), 'rot0'), _mats(trans0, n, (3,), 'trans0'), n, h, w,
        pts2d.data_ptr(), pts3d.data_ptr(), conf.data_ptr(), count.data_ptr(), _stream()), 'scf_flow_corr_2d3d')
    return pts2d, pts3d, conf, count


_PNP_MODES = {None: _lib.PNP_SAMPLE_ALL, 'topk': _lib.PNP_SAMPLE_TOPK, 'random': _lib.PNP_SAMPLE_RANDOM}


def pnp_params(iterations: int = 100, reproj_error: float = 3.0, sample_mode: Optional[str] = None,
               sample_num: int = 1000, seed: int = 0) -> '_lib.PnpParams':
    """validated ``scf_pnp_params``: iterations > 0, a finite reproj_error >= 0 (pixels), sample_mode None / 'topk' /
    'random' with sample_num > 0, seed in [0, 2^64)."""
    if isinstance(iterations, bool) or int(iterations) != iterations or iterations <= 0:
        raise _lib.ScflowHipError(f'pnp: iterations must be a positive integer, got {iterations!r}')
    if not math.isfinite(float(reproj_error)) or float(reproj_error) < 0:
        raise _lib.ScflowHipError(f'pnp: reproj_error must be finite and >= 0, got {reproj_error!r}')
    if sample_mode not in _PNP_MODES:
        raise _lib.ScflowHipError(f"pnp: sample_mode must be None, 'topk' or 'random', got {sample_mode!r}")
    if sample_mode is not None and (int(sample_num) != sample_num or sample_num <= 0):
        raise _lib.ScflowHipError(f'pnp: sample_num must be a positive integer, got {sample_num!r}')
    if int(seed) != seed or not 0 <= seed < 2 ** 64:
        raise _lib.ScflowHipError(f'pnp: seed must be an integer in [0, 2^64), got {seed!r}')
    return _lib.PnpParams(int(iterations), float(reproj_error), _PNP_MODES[sample_mode],
                          int(sample_num) if sample_mode is not None else 0, int(seed))


def pnp_ransac(pts2d: Tensor, pts3d: Tensor, count: Tensor, k: Tensor, ref_rot: Tensor, ref_trans: Tensor,
               conf: Optional[Tensor] = None, iterations: int = 100, reproj_error: float = 3.0,
               sample_mode: Optional[str] = None, sample_num: int = 1000, seed: int = 0):
    """batched RANSAC-EPnP (``scf_pnp_ransac``; include/scflow_hip.h states the contract).

    pts2d (N,C,2), pts3d (N,C,3), conf (N,C) (read by sample_mode='topk'), count (N,) int32 -- the layout
    ``flow_corr_2d3d`` writes -- plus k, ref_rot (N,3,3), ref_trans (N,3) -> (R (N,3,3), t (N,3), ok (N,) int32,
    inliers (N,) int32).  A failed sample returns ok = 0 and the reference pose.  No host synchronisation."""
    p = pnp_params(iterations, reproj_error, sample_mode, sample_num, seed)
    if pts2d.dim() != 3 or pts2d.shape[2] != 2:
        raise _lib.ScflowHipError('pnp_ransac: pts2d must be (N,C,2)')
    n, cap = pts2d.shape[0], pts2d.shape[1]
    if tuple(pts3d.shape) != (n, cap, 3):
        raise _lib.ScflowHipError(f'pnp_ransac: pts3d must be {(n, cap, 3)}, got {tuple(pts3d.shape)}')
    if conf is not None and tuple(conf.shape) != (n, cap):
        raise _lib.ScflowHipError(f'pnp_ransac: conf must be {(n, cap)}, got {tuple(conf.shape)}')
    if sample_mode == 'topk' and conf is None:
        raise _lib.ScflowHipError("pnp_ransac: sample_mode='topk' needs conf")
    if (not isinstance(count, torch.Tensor) or not count.is_cuda or count.dtype != torch.int32
            or tuple(count.shape) != (n,) or not count.is_contiguous() or count.device != pts2d.device):
        raise _lib.ScflowHipError(f'pnp_ransac: count must be a contiguous int32 GPU tensor of shape {(n,)}')
    if n == 0 or cap == 0:
        raise _lib.ScflowHipError('pnp_ransac: empty batch')
    lib = _lib.load()
    dev = pts2d.device
    wsb = lib.scf_pnp_workspace_bytes(n, cap, C.byref(p))
    _lib.check(min(int(wsb), 0), 'scf_pnp_workspace_bytes')
    ws = torch.empty((max(int(wsb), 1),), dtype=torch.uint8, device=dev) if wsb > 0 else None
    rot = torch.empty((n, 3, 3), dtype=torch.float32, device=dev)
    trans = torch.empty((n, 3), dtype=torch.float32, device=dev)
    ok = torch.empty((n,), dtype=torch.int32, device=dev)
    inl = torch.empty((n,), dtype=torch.int32, device=dev)
    _lib.check(lib.scf_pnp_ransac(
        _dense(pts2d, 'pts2d'), _dense(pts3d, 'pts3d'), _opt(conf, 'conf'), count.data_ptr(), n, cap,
        _mats(k, n, (3, 3), 'k'), _mats(ref_rot, n, (3, 3), 'ref_rot'), _mats(ref_trans, n, (3,), 'ref_trans'),
        C.byref(p), rot.data_ptr(), trans.data_ptr(), ok.data_ptr(), inl.data_ptr(),
        None if ws is None else ws.data_ptr(), _stream()), 'scf_pnp_ransac')
    return rot, trans, ok, inl


def pnp(flow: Tensor, depth: Tensor, k: Tensor, ref_rot: Tensor, ref_trans: Tensor,
        occlusion: Optional[Tensor] = None, occ_thresh: float = 0.5, **ransac):
    """pose from flow: ``flow_corr_2d3d`` then ``pnp_ransac`` (keyword arguments of the latter pass through)
    -> (R, t, ok, inliers).  Two launches (three with sampling), no host synchronisation."""
    pts2d, pts3d, conf, count = flow_corr_2d3d(flow, depth, k, ref_rot, ref_trans, occlusion, occ_thresh)
    return pnp_ransac(pts2d, pts3d, count, k, ref_rot, ref_trans, conf=conf, **ransac)


def render_pixel_coord(index: int, size: int, other: int) -> float:
    """image-plane coordinate sampled by pixel ``index`` along an axis of ``size`` pixels when the other axis has
    ``other`` (``scf_render_pixel_coord``, the kernels' own formula; a host call)."""
    return float(_lib.load().scf_render_pixel_coord(int(index), int(size), int(other)))


def render_mesh(mesh, labels: Tensor, rot: Tensor, trans: Tensor, k: Tensor, image_size: Tuple[int, int], *,
                default_lights: bool = True, seperate_lights: bool = True,
                background: Sequence[float] = (0.5, 0.5, 0.5), images: bool = True, pix_to_face: bool = True,
                norm: Optional[Tuple[Sequence[float], Sequence[float]]] = None) -> dict:
    """hard-rasterised, Phong-shaded render of each sample's mesh (``scf_render_mesh``; render.hip states the
    semantics).  ``mesh`` is a ``mesh.DeviceMesh`` (``MeshStore.on(device)``), labels (N,) int GPU tensor selecting
    the class mesh per sample (read on the device: no host synchronisation), rot / k (N,3,3), trans (N,3).
    -> dict(zbuf (N,H,W): z or -1, pix_to_face (N,H,W) int32 or None, images (N,H,W,4) or None, rgb (N,3,H,W) =
    (rgb - mean) / std or None, present when ``norm`` = (mean, std) is given)."""
    h, w = int(image_size[0]), int(image_size[1])
    n = rot.shape[0] if rot.dim() == 3 else -1
    if n <= 0 or tuple(rot.shape) != (n, 3, 3):
        raise _lib.ScflowHipError(f'render_mesh: rot must be (N,3,3) with N > 0, got {tuple(rot.shape)}')
    if (not isinstance(labels, torch.Tensor) or not labels.is_cuda or tuple(labels.shape) != (n,)
            or labels.dtype not in (torch.int32, torch.int64) or labels.device != rot.device):
        raise _lib.ScflowHipError(f'render_mesh: labels must be an integer GPU tensor of shape {(n,)} on {rot.device}')
    if not 0 < h <= 8192 or not 0 < w <= 8192:
        raise _lib.ScflowHipError(f'render_mesh: image size {(h, w)} outside 1..8192')
    dev = rot.device
    lab = labels.to(torch.int32).contiguous()
    for t, nm in ((mesh.verts, 'verts'), (mesh.normals, 'normals'), (mesh.colors, 'colors')):
        _dense(t, nm)
    for t in (mesh.faces, mesh.vert_offset, mesh.face_offset):
        if t.device != dev or t.dtype != torch.int32 or not t.is_contiguous():
            raise _lib.ScflowHipError(f'render_mesh: the mesh store must live on {dev} (MeshStore.on(device))')
    store = _lib.MeshStore(mesh.verts.data_ptr(), mesh.normals.data_ptr(), mesh.colors.data_ptr(),
                           mesh.faces.data_ptr(), mesh.vert_offset.data_ptr(), mesh.face_offset.data_ptr(),
                           int(mesh.num_classes), int(mesh.max_faces))
    mean, std = norm if norm is not None else ((0., 0., 0.), (1., 1., 1.))
    if norm is not None and not all(math.isfinite(float(s)) and float(s) != 0 for s in std):
        raise _lib.ScflowHipError(f'render_mesh: norm std must be finite and non-zero, got {std!r}')
    f3 = C.c_float * 3
    p = _lib.RenderParams(h, w, int(bool(default_lights)), int(bool(seperate_lights)), f3(*map(float, background)),
                          f3(*map(float, mean)), f3(*map(float, std)))
    lib = _lib.load()
    wsb = int(lib.scf_render_workspace_bytes(n, int(mesh.max_faces)))
    _lib.check(min(wsb, 0), 'scf_render_workspace_bytes')
    ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
    zbuf = torch.empty((n, h, w), dtype=torch.float32, device=dev)
    p2f = torch.empty((n, h, w), dtype=torch.int32, device=dev) if pix_to_face else None
    img = torch.empty((n, h, w, 4), dtype=torch.float32, device=dev) if images else None
    rgb = torch.empty((n, 3, h, w), dtype=torch.float32, device=dev) if norm is not None else None
    _lib.check(lib.scf_render_mesh(
        C.byref(store), lab.data_ptr(), _mats(rot, n, (3, 3), 'rot'), _mats(trans, n, (3,), 'trans'),
        _mats(k, n, (3, 3), 'k'), n, C.byref(p), zbuf.data_ptr(),
        None if p2f is None else p2f.data_ptr(), None if img is None else img.data_ptr(),
        None if rgb is None else rgb.data_ptr(), ws.data_ptr(), _stream()), 'scf_render_mesh')
    return dict(zbuf=zbuf, pix_to_face=p2f, images=img, rgb=rgb)


def _triple(v, name: str) -> Tuple[float, float, float]:
    vals = tuple(float(x) for x in v) if isinstance(v, (list, tuple)) or hasattr(v, '__len__') else (float(v),) * 3
    if len(vals) != 3:
        raise _lib.ScflowHipError(f'{name}: expected a scalar or three values, got {v!r}')
    return vals


def patch_params(out_size: Tuple[int, int] = (256, 256), resize: int = 256, *, size_ratio: float = 1.1,
                 aspect_ratio: float = 1.0, keep_ratio: bool = False, min_expand: float = 0.0,
                 clip_border: bool = False, fix_clip_border_quirk: bool = False, center: bool = True,
                 crop_pad_val=128, pad_val=128, mean=(0., 0., 0.), std=(255., 255., 255.), to_rgb: bool = True,
                 vertex_stride: int = 1) -> '_lib.PatchParams':
    """``scf_patch_params`` from the pipeline's settings (the defaults are the shipped val_pipeline).  The values
    are checked here so that a bad one is named; the C entries refuse them too (``SCF_EINVAL``)."""
    oh, ow = int(out_size[0]), int(out_size[1])
    if not 0 < oh <= 8192 or not 0 < ow <= 8192:
        raise _lib.ScflowHipError(f'patch_params: out_size {(oh, ow)} outside 1..8192')
    if not 0 < int(resize) <= min(oh, ow):
        raise _lib.ScflowHipError(f'patch_params: resize={resize} must be in 1..min(out_size) = {min(oh, ow)}')
    if int(vertex_stride) < 1:
        raise _lib.ScflowHipError(f'patch_params: vertex_stride={vertex_stride} must be >= 1')
    for nm, v, ok in (('size_ratio', size_ratio, float(size_ratio) > 0), ('aspect_ratio', aspect_ratio, float(aspect_ratio) > 0),
                      ('min_expand', min_expand, float(min_expand) >= 0)):
        if not (ok and math.isfinite(float(v))):
            raise _lib.ScflowHipError(f'patch_params: {nm}={v!r} out of range')
    cp, pv, mn, sd = (_triple(crop_pad_val, 'crop_pad_val'), _triple(pad_val, 'pad_val'), _triple(mean, 'mean'),
                      _triple(std, 'std'))
    for nm, v in (('crop_pad_val', cp), ('pad_val', pv)):
        if not all(x == int(x) and 0 <= x <= 255 for x in v):
            raise _lib.ScflowHipError(f'patch_params: {nm}={v!r} must be integers in 0..255')
    if not all(math.isfinite(x) for x in mn) or not all(math.isfinite(x) and x != 0 for x in sd):
        raise _lib.ScflowHipError(f'patch_params: mean {mn!r} / std {sd!r} must be finite, std non-zero')
    i3, f3 = C.c_int32 * 3, C.c_float * 3
    return _lib.PatchParams(float(aspect_ratio), float(size_ratio), float(min_expand), oh, ow, int(resize),
                            int(vertex_stride), int(bool(keep_ratio)), int(bool(clip_border)),
                            int(bool(fix_clip_border_quirk)), int(bool(center)), int(bool(to_rgb)),
                            i3(*map(int, cp)), i3(*map(int, pv)), f3(*mn), f3(*sd))


def _int_vec(t: Tensor, shape: Tuple[int, ...], dev, name: str) -> Tensor:
    """an integer GPU tensor of ``shape`` as contiguous int32 (converted on the device: no host synchronisation)."""
    if (not isinstance(t, torch.Tensor) or not t.is_cuda or tuple(t.shape) != shape
            or t.dtype not in (torch.int32, torch.int64) or t.device != dev):
        raise _lib.ScflowHipError(f'{name} must be an int32 / int64 GPU tensor of shape {shape} on {dev}')
    return t.to(torch.int32).contiguous()


def _patch_boxes(what: str, mesh, labels, rot, trans, k, frame_size, params, crop_rects, aug=None, id_base: int = 0,
                 sample_ids: Optional[Tensor] = None) -> dict:
    """``scf_patch_boxes``, or with ``aug`` ``scf_patch_boxes_train``, for the wrapper named ``what``."""
    n = k.shape[0] if isinstance(k, torch.Tensor) and k.dim() == 3 else -1
    if n <= 0:
        raise _lib.ScflowHipError(f'{what}: k must be (N,3,3) with N > 0')
    hf, wf = int(frame_size[0]), int(frame_size[1])
    if not 0 < hf <= 16384 or not 0 < wf <= 16384:
        raise _lib.ScflowHipError(f'{what}: frame size {(hf, wf)} outside 1..16384')
    kp = _mats(k, n, (3, 3), 'k')
    dev = k.device
    store, lab, rp, tp, cin = None, None, None, None, None
    if crop_rects is not None:
        cin = _int_vec(crop_rects, (n, 4), dev, what + ': crop_rects')
    else:
        if mesh is None or labels is None or rot is None or trans is None:
            raise _lib.ScflowHipError(f'{what}: mesh, labels, rot and trans are needed without crop_rects')
        lab = _int_vec(labels, (n,), dev, what + ': labels')
        rp, tp = _mats(rot, n, (3, 3), 'rot'), _mats(trans, n, (3,), 'trans')
        store = _mesh_store(mesh, dev, what)
    sp = None if store is None else C.byref(store)
    lp = None if lab is None else lab.data_ptr()
    cp = None if cin is None else cin.data_ptr()
    lib = _lib.load()
    if aug is None:
        wsb = int(lib.scf_patch_workspace_bytes(n))
    else:
        sid = _sample_ids(sample_ids, n, dev, what)
        wsb = int(lib.scf_patch_train_workspace_bytes(n))
    _lib.check(min(wsb, 0), 'scf_patch_workspace_bytes')
    rec = torch.empty((wsb,), dtype=torch.uint8, device=dev)
    box = torch.empty((n, 4), dtype=torch.float32, device=dev)
    crop = torch.empty((n, 4), dtype=torch.int32, device=dev)
    scale = torch.empty((n,), dtype=torch.float32, device=dev)
    tm = torch.empty((n, 3, 3), dtype=torch.float32, device=dev)
    kout = torch.empty((n, 3, 3), dtype=torch.float32, device=dev)
    valid = torch.empty((n,), dtype=torch.int32, device=dev)
    out = dict(box=box, crop=crop, scale=scale, transform_matrix=tm, k=kout, valid=valid, records=rec)
    if aug is None:
        _lib.check(lib.scf_patch_boxes(
            sp, lp, rp, tp, kp, cp, n, hf, wf, C.byref(params), box.data_ptr(), crop.data_ptr(), scale.data_ptr(),
            tm.data_ptr(), kout.data_ptr(), valid.data_ptr(), rec.data_ptr(), _stream()), 'scf_patch_boxes')
    else:
        out['draws'] = draws = torch.empty((n, 8), dtype=torch.float64, device=dev)
        _lib.check(lib.scf_patch_boxes_train(
            sp, lp, rp, tp, kp, cp, n, hf, wf, C.byref(params), C.byref(aug), _id_base(id_base, what), sid,
            draws.data_ptr(), box.data_ptr(), crop.data_ptr(), scale.data_ptr(), tm.data_ptr(), kout.data_ptr(),
            valid.data_ptr(), rec.data_ptr(), _stream()), 'scf_patch_boxes_train')
    return out


def patch_boxes(mesh, labels: Optional[Tensor], rot: Optional[Tensor], trans: Optional[Tensor], k: Tensor,
                frame_size: Tuple[int, int], params: '_lib.PatchParams', crop_rects: Optional[Tensor] = None) -> dict:
    """crop rectangle, resize scale, padding and intrinsics of every object (``scf_patch_boxes``; patch.hip states
    the semantics).  ``mesh`` is a ``mesh.DeviceMesh``, labels (N,) int GPU tensor (read on the device), rot / k
    (N,3,3), trans (N,3), frame_size (Hf, Wf).  With ``crop_rects`` (N,4) int GPU tensor of (x1, y1, x2, y2) the
    caller's rectangles replace the box and the crop rule, and mesh / labels / rot / trans may be None.
    -> dict(box (N,4) the projected fp32 box, crop (N,4) int32, scale (N), transform_matrix (N,3,3), k (N,3,3), valid (N) int32, records: the
    workspace ``extract_patches`` reads).  No host synchronisation."""
    return _patch_boxes('patch_boxes', mesh, labels, rot, trans, k, frame_size, params, crop_rects)


def _patch_frames(frames: Tensor, what: str) -> tuple:
    """the frames argument of an extract wrapper, checked -> (F, Hf, Wf, device)."""
    if (not isinstance(frames, torch.Tensor) or not frames.is_cuda or frames.dtype != torch.uint8 or frames.dim() != 4
            or frames.shape[3] != 3 or frames.shape[0] < 1):
        raise _lib.ScflowHipError(f'{what}: frames must be a (F,Hf,Wf,3) uint8 tensor on the GPU '
                                  '(HIP path only, no CPU fallback)')
    if frames.device.index != _cur_dev():
        raise _lib.ScflowHipError(f'{what}: frames live on cuda:{frames.device.index} but the current device '
                                  f'is cuda:{_cur_dev()}: wrap the call in torch.cuda.device(tensor.device)')
    if not frames.is_contiguous():
        raise _lib.ScflowHipError(f'{what}: expected contiguous frames')
    f, hf, wf = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
    if not 0 < hf <= 16384 or not 0 < wf <= 16384:
        raise _lib.ScflowHipError(f'{what}: frame size {(hf, wf)} outside 1..16384')
    return f, hf, wf, frames.device


def _patch_index(frame_index: Tensor, dev, what: str) -> Tensor:
    if not isinstance(frame_index, torch.Tensor) or frame_index.dim() != 1 or frame_index.shape[0] < 1:
        raise _lib.ScflowHipError(f'{what}: frame_index must be (N,) with N > 0')
    return _int_vec(frame_index, (int(frame_index.shape[0]),), dev, what + ': frame_index')


def _patch_records(records: Tensor, nbytes: int, dev, what: str, boxes: str) -> int:
    if (not isinstance(records, torch.Tensor) or records.device != dev or records.dtype != torch.uint8
            or not records.is_contiguous() or records.numel() != nbytes):
        raise _lib.ScflowHipError(f'{what}: records must be the workspace {boxes} returned for the same N')
    return records.data_ptr()


def _patch_out(t: Optional[Tensor], shape: Tuple[int, ...], dev, what: str) -> Tensor:
    """``out`` checked against shape and device (``_dense`` does the rest at the call), or a new tensor."""
    if t is None:
        return torch.empty(shape, dtype=torch.float32, device=dev)
    if tuple(t.shape) != shape or t.device != dev:
        raise _lib.ScflowHipError(f'{what}: out must be {shape} on {dev}')
    return t


def extract_patches(frames: Tensor, frame_index: Tensor, records: Tensor, params: '_lib.PatchParams',
                    out: Optional[Tensor] = None) -> Tensor:
    """crop, resize, pad and normalise every object's patch (``scf_patch_extract``).  frames (F,Hf,Wf,3) uint8 GPU
    tensor (BGR, as cv2 loads them), frame_index (N,) int GPU tensor, ``records`` from ``patch_boxes``.
    -> (N,3,out_h,out_w) float32.  No host synchronisation."""
    f, hf, wf, dev = _patch_frames(frames, 'extract_patches')
    fidx = _patch_index(frame_index, dev, 'extract_patches')
    n = int(fidx.shape[0])
    lib = _lib.load()
    rec = _patch_records(records, int(lib.scf_patch_workspace_bytes(n)), dev, 'extract_patches', 'patch_boxes')
    out = _patch_out(out, (n, 3, int(params.out_h), int(params.out_w)), dev, 'extract_patches')
    _lib.check(lib.scf_patch_extract(frames.data_ptr(), f, hf, wf, fidx.data_ptr(), n, rec, C.byref(params), _dense(out, 'out'),
                                     _stream()), 'scf_patch_extract')
    return out


def patch_aug_params(*, seed: int = 0, jitter_angle_dis=(0., 15.), jitter_x_dis=(0., 15.), jitter_y_dis=(0., 15.),
                     jitter_z_dis=(0., 50.), angle_limit: Optional[float] = 45., translation_limit: Optional[float] = 200.,
                     add_limit: Optional[float] = 1., max_tries: int = 64, size_range=(1.0, 1.25), h_ratio: float = 0.2,
                     s_ratio: float = 0.5, v_ratio: float = 0.5, hsv_p: float = 1.0, noise_ratio: float = 0.1,
                     noise_p: float = 1.0, max_kernel_size: float = 5, smooth_p: float = 1.0,
                     fix_error_swap_quirk: bool = False, mask_pad_val: int = 0) -> '_lib.PatchAugParams':
    """``scf_patch_aug_params`` from the train pipeline's settings (the defaults are the shipped train_pipeline of
    ycbv_real.py).  A limit of None is not applied; a ``p`` of 0 switches its transform off.  The values are checked here
    so that a bad one is named; the C entries refuse them too (``SCF_EINVAL``)."""
    if int(seed) != seed or not 0 <= seed < 2 ** 64:
        raise _lib.ScflowHipError(f'patch_aug_params: seed must be an integer in [0, 2^64), got {seed!r}')
    pairs = []
    for nm, v in (('jitter_angle_dis', jitter_angle_dis), ('jitter_x_dis', jitter_x_dis), ('jitter_y_dis', jitter_y_dis),
                  ('jitter_z_dis', jitter_z_dis)):
        if not isinstance(v, (list, tuple)) or len(v) != 2 or not all(math.isfinite(float(x)) for x in v) or float(v[1]) < 0:
            raise _lib.ScflowHipError(f'patch_aug_params: {nm}={v!r} must be (mean, std >= 0)')
        pairs.append((float(v[0]), float(v[1])))
    limits = []
    for nm, v in (('angle_limit', angle_limit), ('translation_limit', translation_limit), ('add_limit', add_limit)):
        if v is not None and not (math.isfinite(float(v)) and float(v) >= 0):
            raise _lib.ScflowHipError(f'patch_aug_params: {nm}={v!r} must be None or finite and >= 0')
        limits.append(-1.0 if v is None else float(v))
    lo, hi = (float(x) for x in size_range)
    if not (0 < lo <= hi and math.isfinite(hi)):
        raise _lib.ScflowHipError(f'patch_aug_params: size_range={size_range!r} needs 0 < lo <= hi')
    for nm, v in (('h_ratio', h_ratio), ('s_ratio', s_ratio), ('v_ratio', v_ratio)):
        if not 0 <= float(v) < 1:
            raise _lib.ScflowHipError(f'patch_aug_params: {nm}={v!r} must be in [0, 1) (a gain must stay positive)')
    for nm, v in (('hsv_p', hsv_p), ('noise_p', noise_p), ('smooth_p', smooth_p)):
        if not 0 <= float(v) <= 1:
            raise _lib.ScflowHipError(f'patch_aug_params: {nm}={v!r} must be in [0, 1]')
    if not (math.isfinite(float(noise_ratio)) and float(noise_ratio) >= 0):
        raise _lib.ScflowHipError(f'patch_aug_params: noise_ratio={noise_ratio!r} must be finite and >= 0')
    if isinstance(max_tries, bool) or int(max_tries) != max_tries or not 1 <= max_tries <= 4096:
        raise _lib.ScflowHipError(f'patch_aug_params: max_tries={max_tries!r} must be an integer in 1..4096')
    # the reference truncates it (int(5.) = 5) and draws k from [2 i + 1 for i in range(max_kernel_size // 2 + 1)]: an even
    # value also draws max_kernel_size + 1
    if not 1 <= int(max_kernel_size) <= 15:
        raise _lib.ScflowHipError(f'patch_aug_params: max_kernel_size={max_kernel_size!r} must be in 1..15')
    d2, d3 = C.c_double * 2, C.c_double * 3
    return _lib.PatchAugParams(int(seed), d2(*pairs[0]), d2(*pairs[1]), d2(*pairs[2]), d2(*pairs[3]), limits[0], limits[1],
                               limits[2], d2(lo, hi), d3(float(h_ratio), float(s_ratio), float(v_ratio)), float(hsv_p),
                               float(noise_p), float(smooth_p), float(noise_ratio), int(max_tries), int(max_kernel_size),
                               int(bool(fix_error_swap_quirk)), int(bool(mask_pad_val)))


def _mesh_store(mesh, dev, what: str) -> '_lib.MeshStore':
    _dense(mesh.verts, 'verts')
    if mesh.vert_offset.device != dev or mesh.vert_offset.dtype != torch.int32 or not mesh.vert_offset.is_contiguous():
        raise _lib.ScflowHipError(f'{what}: the mesh store must live on {dev} (MeshStore.on(device))')
    return _lib.MeshStore(mesh.verts.data_ptr(), mesh.normals.data_ptr(), mesh.colors.data_ptr(), mesh.faces.data_ptr(),
                          mesh.vert_offset.data_ptr(), mesh.face_offset.data_ptr(), int(mesh.num_classes),
                          int(mesh.max_faces))


def _sample_ids(sample_ids: Optional[Tensor], n: int, dev, what: str) -> Optional[int]:
    if sample_ids is None:
        return None
    if (not isinstance(sample_ids, torch.Tensor) or not sample_ids.is_cuda or sample_ids.dtype != torch.int64
            or tuple(sample_ids.shape) != (n,) or not sample_ids.is_contiguous() or sample_ids.device != dev):
        raise _lib.ScflowHipError(f'{what}: sample_ids must be a contiguous int64 GPU tensor of shape {(n,)} on {dev}')
    return sample_ids.data_ptr()


def _id_base(id_base: int, what: str) -> int:
    if isinstance(id_base, bool) or int(id_base) != id_base or not 0 <= id_base < 2 ** 62:
        raise _lib.ScflowHipError(f'{what}: id_base must be an integer in [0, 2^62), got {id_base!r}')
    return int(id_base)


def pose_jitter(mesh, diameters: Optional[Tensor], labels: Optional[Tensor], gt_rot: Tensor, gt_trans: Tensor,
                aug: '_lib.PatchAugParams', *, vertex_stride: int = 1, id_base: int = 0,
                sample_ids: Optional[Tensor] = None) -> dict:
    """PoseJitter for a batch (``scf_pose_jitter``; patch_train.hip states the semantics).  ``mesh`` is a
    ``mesh.DeviceMesh`` with ``diameters`` (num_classes,) float32 and ``labels`` (N,) int on the GPU, or all three None
    when ``aug`` has no add_limit; gt_rot (N,3,3), gt_trans (N,3).
    -> dict(rot (N,3,3), trans (N,3), add_error, rot_error, trans_error (N) float32, ok, tries (N) int32).
    No host synchronisation."""
    n = gt_rot.shape[0] if isinstance(gt_rot, torch.Tensor) and gt_rot.dim() == 3 else -1
    if n <= 0:
        raise _lib.ScflowHipError('pose_jitter: gt_rot must be (N,3,3) with N > 0')
    if int(vertex_stride) < 1:
        raise _lib.ScflowHipError(f'pose_jitter: vertex_stride={vertex_stride} must be >= 1')
    if mesh is None and aug.add_limit >= 0:
        raise _lib.ScflowHipError('pose_jitter: add_limit needs the mesh store and the diameters')
    rp, tp = _mats(gt_rot, n, (3, 3), 'gt_rot'), _mats(gt_trans, n, (3,), 'gt_trans')
    dev = gt_rot.device
    store, lab, dp = None, None, None
    if mesh is not None:
        if diameters is None or labels is None:
            raise _lib.ScflowHipError('pose_jitter: a mesh needs diameters and labels')
        store = _mesh_store(mesh, dev, 'pose_jitter')
        if tuple(diameters.shape) != (int(mesh.num_classes),) or diameters.device != dev:
            raise _lib.ScflowHipError(f'pose_jitter: diameters must be ({int(mesh.num_classes)},) float32 on {dev}')
        dp = _dense(diameters, 'diameters')
        lab = _int_vec(labels, (n,), dev, 'pose_jitter: labels')
    sid = _sample_ids(sample_ids, n, dev, 'pose_jitter')
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    out = dict(rot=f32(n, 3, 3), trans=f32(n, 3), add_error=f32(n), rot_error=f32(n), trans_error=f32(n),
               ok=torch.empty((n,), dtype=torch.int32, device=dev), tries=torch.empty((n,), dtype=torch.int32, device=dev))
    _lib.check(_lib.load().scf_pose_jitter(
        None if store is None else C.byref(store), dp, None if lab is None else lab.data_ptr(), rp, tp, n,
        int(vertex_stride), C.byref(aug), _id_base(id_base, 'pose_jitter'), sid, out['rot'].data_ptr(),
        out['trans'].data_ptr(), out['add_error'].data_ptr(), out['rot_error'].data_ptr(), out['trans_error'].data_ptr(),
        out['ok'].data_ptr(), out['tries'].data_ptr(), _stream()), 'scf_pose_jitter')
    return out


def patch_train_route(ph: int, pw: int, new_h: int, new_w: int, k: int) -> str:
    """the route ``extract_patches_train`` takes for an object with a ``ph x pw`` crop patch resized to
    ``new_h x new_w`` under a ``k x k`` smoothing kernel: 'lds' or 'direct' (``scf_patch_train_route``, the kernel's own
    formula; a host call)."""
    r = int(_lib.load().scf_patch_train_route(int(ph), int(pw), int(new_h), int(new_w), int(k)))
    _lib.check(min(r, 0), 'scf_patch_train_route')
    return ('lds', 'direct')[r]


def patch_boxes_train(mesh, labels: Optional[Tensor], rot: Optional[Tensor], trans: Optional[Tensor], k: Tensor,
                      frame_size: Tuple[int, int], params: '_lib.PatchParams', aug: '_lib.PatchAugParams', *,
                      id_base: int = 0, sample_ids: Optional[Tensor] = None, crop_rects: Optional[Tensor] = None) -> dict:
    """``patch_boxes`` with the size ratio drawn per object from ``aug.size_range``, plus the colour draws
    (``scf_patch_boxes_train``).  -> what ``patch_boxes`` returns, with ``records`` the train workspace
    ``extract_patches_train`` reads (its head is what ``extract_patches`` reads: ``records[:64 * N]``) and ``draws``
    (N,8) float64 = (size_ratio, h gain, s gain, v gain, sigma, k, hsv on, noise on).  No host synchronisation."""
    return _patch_boxes('patch_boxes_train', mesh, labels, rot, trans, k, frame_size, params, crop_rects, aug, id_base,
                        sample_ids)


def extract_patches_train(frames: Tensor, frame_index: Tensor, records: Tensor, params: '_lib.PatchParams',
                          aug: '_lib.PatchAugParams', masks: Optional[Tensor] = None, out: Optional[Tensor] = None,
                          mask_out: Optional[Tensor] = None):
    """crop, augment (RandomHSV, RandomNoise, RandomSmooth), resize, pad and normalise every object's patch, and crop,
    resize (nearest) and pad its mask (``scf_patch_extract_train``).  frames (F,Hf,Wf,3) uint8 GPU tensor (BGR),
    frame_index (N,) int GPU tensor, ``records`` from ``patch_boxes_train``, masks (N,Hf,Wf) uint8 or bool (nonzero =
    object) or None.  -> (img (N,3,out_h,out_w) float32, mask (N,out_h,out_w) bool or None).  No host synchronisation."""
    what = 'extract_patches_train'
    f, hf, wf, dev = _patch_frames(frames, what)
    fidx = _patch_index(frame_index, dev, what)
    n = int(fidx.shape[0])
    lib = _lib.load()
    rec = _patch_records(records, int(lib.scf_patch_train_workspace_bytes(n)), dev, what, 'patch_boxes_train')
    shape = (n, 3, int(params.out_h), int(params.out_w))
    out = _patch_out(out, shape, dev, what)
    mp = None
    if masks is not None:
        if (not isinstance(masks, torch.Tensor) or masks.device != dev or masks.dtype not in (torch.uint8, torch.bool)
                or tuple(masks.shape) != (n, hf, wf) or not masks.is_contiguous()):
            raise _lib.ScflowHipError(f'{what}: masks must be a contiguous uint8 / bool tensor of shape {(n, hf, wf)} on {dev}')
        mshape = (n, shape[2], shape[3])
        if mask_out is None:
            mask_out = torch.empty(mshape, dtype=torch.bool, device=dev)
        elif (tuple(mask_out.shape) != mshape or mask_out.device != dev or mask_out.dtype != torch.bool
              or not mask_out.is_contiguous()):
            raise _lib.ScflowHipError(f'{what}: mask_out must be a contiguous bool tensor {mshape} on {dev}')
        mp = masks.data_ptr()
    elif mask_out is not None:
        raise _lib.ScflowHipError(f'{what}: mask_out without masks')
    _lib.check(lib.scf_patch_extract_train(frames.data_ptr(), f, hf, wf, fidx.data_ptr(), mp, n, rec, C.byref(params),
                                           C.byref(aug), _dense(out, 'out'), None if mask_out is None else mask_out.data_ptr(),
                                           _stream()), 'scf_patch_extract_train')
    return out, mask_out


def unproject_depth(depth: Tensor, k: Tensor, rot0: Tensor, trans0: Tensor) -> Tensor:
    n, h, w = depth.shape
    out = torch.empty((n, 3, h, w), dtype=torch.float32, device=depth.device)
    _lib.check(_lib.load().scf_unproject_depth(
        _dense(depth, 'depth'), _dense(k, 'k'), _dense(rot0, 'rot0'), _dense(trans0, 'trans0'),
        out.data_ptr(), n, h, w, _stream()), 'scf_unproject_depth')
    return out


def resize_bilinear(a: Tensor, out_hw: Tuple[int, int], mul: float = 1.0,
                    b: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """mul * F.interpolate(a + b, size=out_hw, mode='bilinear', align_corners=True)."""
    pa = _dense(a, 'a')
    n, c, h, w = a.shape
    ho, wo = out_hw
    if out is None:
        out = torch.empty((n, c, ho, wo), dtype=torch.float32, device=a.device)
    _lib.check(_lib.load().scf_resize_bilinear(pa, _opt(b, 'b'), _dense(out, 'out'), n * c, h, w,
                                               ho, wo, float(mul), _stream()),
               'scf_resize_bilinear')
    return out


TAIL_MAX_T = 32                                  # SCF_TAIL_MAX_T
TAIL_DETACH_POSE, TAIL_DETACH_DEPTH_FOR_XY = 1, 2


def _ptrs(tensors, name: str, n_expected: Optional[int] = None, shape=None, optional: bool = False):
    """HOST array of the device pointers of a list of dense fp32 GPU tensors (None entries -> NULL when ``optional``)."""
    if tensors is None:
        return None
    if n_expected is not None and len(tensors) != n_expected:
        raise ValueError(f'{name}: {len(tensors)} entries for {n_expected} iterations')
    ptrs = []
    for i, t in enumerate(tensors):
        if t is None:
            if not optional:
                raise ValueError(f'{name}[{i}] is None')
            ptrs.append(None)
            continue
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise _lib.ScflowHipError(f'{name}[{i}] has shape {tuple(t.shape)}, expected {tuple(shape)}')
        ptrs.append(_dense(t, f'{name}[{i}]'))
    return (C.c_void_p * len(ptrs))(*ptrs)


def _seq_like(seq, shape):
    """T fresh tensors of ``shape`` for the T entries of ``seq``: one allocation, a view per iteration."""
    return list(torch.empty((len(seq),) + tuple(shape), dtype=torch.float32, device=seq[0].device).unbind(0))


def resize_bilinear_grad(g, in_hw: Tuple[int, int], mul: float = 1.0, add=None, out=None, accumulate: bool = False,
                         second=None):
    """``scf_resize_bilinear_grad``: the adjoint of ``resize_bilinear(a, out_hw, mul)`` for ``a`` of size ``in_hw``.
    ``g``: one (N,C,Hout,Wout) tensor or a list of T of them (one launch for all) -> mul * U^T (g + add), (N,C,*in_hw),
    in the same structure.  ``out``: destination(s) to write, or with ``accumulate`` to add to.  ``second=(g2, mul2[, out2[,
    accumulate2]])``: a second job of the same geometry in the same launch; the result is then a pair."""
    single = isinstance(g, torch.Tensor)
    gs = [g] if single else list(g)
    T = len(gs)
    if T == 0 or T > TAIL_MAX_T:
        raise _lib.ScflowHipError(f'resize_bilinear_grad: 1 .. {TAIL_MAX_T} iterations, got {T}')
    hin, win = in_hw
    if gs[0].dim() != 4:
        raise _lib.ScflowHipError('resize_bilinear_grad: expected (N,C,Hout,Wout) gradients')
    n, c, ho, wo = gs[0].shape

    def job(gl, outs, acc, name):
        n2, c2 = gl[0].shape[:2]
        pg = _ptrs(gl, name, T, (n2, c2, ho, wo))
        if outs is None:
            if acc:
                raise ValueError(f'{name}: accumulate needs a destination')
            outs = _seq_like(gl, (n2, c2, hin, win))
        else:
            outs = [outs] if isinstance(outs, torch.Tensor) else list(outs)
        return pg, _ptrs(outs, name + ' out', T, (n2, c2, hin, win)), n2 * c2, outs

    pg, po, planes, outs = job(gs, out, accumulate, 'g')
    padd = None
    if add is not None:
        adds = [add] if isinstance(add, torch.Tensor) else list(add)
        padd = _ptrs(adds, 'add', T, (n, c, ho, wo), optional=True)
    pg1 = po1 = None
    planes1, mul1, acc1, outs1 = 0, 1.0, False, None
    if second is not None:
        g2, mul1 = second[0], float(second[1])
        out2 = second[2] if len(second) > 2 else None
        acc1 = bool(second[3]) if len(second) > 3 else False
        pg1, po1, planes1, outs1 = job([g2] if isinstance(g2, torch.Tensor) else list(g2), out2, acc1, 'second')
    _lib.check(_lib.load().scf_resize_bilinear_grad(pg, padd, po, planes, float(mul), int(bool(accumulate)), pg1, po1, planes1,
                                                    mul1, int(acc1), T, hin, win, ho, wo, _stream()),
               'scf_resize_bilinear_grad')
    res = outs[0] if single else outs
    if second is None:
        return res
    return res, (outs1[0] if isinstance(second[0], torch.Tensor) else outs1)


def reproject_flow_grad(g_flows, depth: Tensor, k: Tensor, rot0: Tensor, trans0: Tensor, rots, transs) -> Tensor:
    """``scf_reproject_flow_grad``: the re-projection sums of T iterations in one launch -> (T, N, tiles, 12) float64
    per-block partial sums, to be added over ``tiles`` in ascending order (``pose_update_grad`` does): words [0, 9) =
    d / dR_i (row-major), [9, 12) = d / dt_i.  ``g_flows``: T cotangents (N,2,H,W) of ``reproject_flow``'s output; None
    entries give exact zeros."""
    T = len(g_flows)
    n, h, w = depth.shape
    if T == 0 or T > TAIL_MAX_T:
        raise _lib.ScflowHipError(f'reproject_flow_grad: 1 .. {TAIL_MAX_T} iterations, got {T}')
    lib = _lib.load()
    nbytes = int(lib.scf_tail_grad_workspace_bytes(n, h, w, T))
    _lib.check(min(nbytes, 0), 'scf_tail_grad_workspace_bytes')
    ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=depth.device)
    _lib.check(lib.scf_reproject_flow_grad(
        _dense(depth, 'depth'), _mats(k, n, (3, 3), 'k'), _mats(rot0, n, (3, 3), 'rot0'), _mats(trans0, n, (3,), 'trans0'),
        _ptrs(rots, 'rots', T, (n, 3, 3)), _ptrs(transs, 'transs', T, (n, 3)),
        _ptrs(g_flows, 'g_flows', T, (n, 2, h, w), optional=True), T, n, h, w, ws.data_ptr(), _stream()),
        'scf_reproject_flow_grad')
    return ws.view(T, n, -1, 12)


def pose_update_grad(d_rots, d_transs, rot0: Tensor, trans0: Tensor, rots, transs, g_rots=None, g_transs=None,
                     reproject_sums: Optional[Tensor] = None, image_hw: Optional[Tuple[int, int]] = None,
                     detach_pose: bool = True, detach_depth_for_xy: bool = False, label_mode: int = 0):
    """``scf_pose_tail_grad``: the reverse scan over T pose updates -> (list of d / d delta_rotation_i (N,6), list of
    d / d delta_translation_i (N,3)).  ``d_rots`` / ``d_transs``: the selected head outputs ``pose_update`` returned;
    ``rots`` / ``transs``: the poses it returned (entry i - 1 is the input of iteration i, ``rot0`` / ``trans0`` of the
    first); ``g_rots`` / ``g_transs``: cotangents of the poses (lists, None entries allowed); ``reproject_sums``: what
    ``reproject_flow_grad`` returned for images of ``image_hw``; ``label_mode``: the depth bit of ``pose_update``."""
    T = len(d_rots)
    if T == 0 or T > TAIL_MAX_T:
        raise _lib.ScflowHipError(f'pose_update_grad: 1 .. {TAIL_MAX_T} iterations, got {T}')
    n = d_rots[0].shape[0]
    h, w = image_hw if image_hw is not None else (0, 0)
    sums = None
    if reproject_sums is not None:
        lib = _lib.load()
        if image_hw is None or reproject_sums.dtype != torch.float64 or not reproject_sums.is_cuda or \
                reproject_sums.numel() * 8 != int(lib.scf_tail_grad_workspace_bytes(n, h, w, T)):
            raise _lib.ScflowHipError('reproject_sums: expected what reproject_flow_grad returned for image_hw')
        sums = reproject_sums.contiguous()
    g_dr, g_dt = _seq_like(d_rots, (n, 6)), _seq_like(d_rots, (n, 3))
    flags = (TAIL_DETACH_POSE if detach_pose else 0) | (TAIL_DETACH_DEPTH_FOR_XY if detach_depth_for_xy else 0)
    _lib.check(_lib.load().scf_pose_tail_grad(
        _ptrs(d_rots, 'd_rots', T, (n, 6)), _ptrs(d_transs, 'd_transs', T, (n, 3)), _mats(rot0, n, (3, 3), 'rot0'),
        _mats(trans0, n, (3,), 'trans0'), _ptrs(rots, 'rots', T, (n, 3, 3)), _ptrs(transs, 'transs', T, (n, 3)),
        _ptrs(g_rots, 'g_rots', T, (n, 3, 3), optional=True), _ptrs(g_transs, 'g_transs', T, (n, 3), optional=True),
        None if sums is None else sums.data_ptr(), h, w, flags, int(label_mode) & 2, _ptrs(g_dr, 'g_d_rot'),
        _ptrs(g_dt, 'g_d_trans'), T, n, _stream()), 'scf_pose_tail_grad')
    return g_dr, g_dt


def convex_upsample(x: Tensor, mask: Tensor, scale: int = 8, x_mul: float = 1.0,
                    mask_mul: float = 1.0, out: Optional[Tensor] = None) -> Tensor:
    """RAFT convex up-sampling (raft_decoder.py:381-416): x (N,C,h,w), mask (N,9*scale^2,h,w)
    -> (N,C,scale*h,scale*w)."""
    px = _dense(x, 'x')
    n, c, h, w = x.shape
    if tuple(mask.shape) != (n, 9 * scale * scale, h, w):
        raise _lib.ScflowHipError(f'mask has shape {tuple(mask.shape)}')
    if out is None:
        out = torch.empty((n, c, scale * h, scale * w), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().scf_convex_upsample(px, _dense(mask, 'mask'), _dense(out, 'out'), n, c,
                                               h, w, scale, float(x_mul), float(mask_mul),
                                               _stream()), 'scf_convex_upsample')
    return out


def avgpool2x2(x: Tensor) -> Tensor:
    px = _dense(x, 'x')
    n, c, h, w = x.shape
    out = torch.empty((n, c, h // 2, w // 2), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().scf_avgpool2x2(px, out.data_ptr(), n * c, h, w, _stream()),
               'scf_avgpool2x2')
    return out


def mul_mask(x: Tensor, mask: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """x * mask with mask (N, 1, H, W) broadcast over the channels (scflow_decoder.py:199-205)."""
    px, n, c, h, w, sx = _nchw(x, 'x')
    if tuple(mask.shape) != (n, 1, h, w):
        raise _lib.ScflowHipError(f'mask has shape {tuple(mask.shape)}, expected {(n, 1, h, w)}')
    if out is None:
        out = torch.empty((n, c, h, w), dtype=torch.float32, device=x.device)
    po, n2, c2, h2, w2, so = _nchw(out, 'out')
    if (n2, c2, h2, w2) != (n, c, h, w):
        raise _lib.ScflowHipError('mul_mask: out shape mismatch')
    _lib.check(_lib.load().scf_mul_mask(px, sx, _dense(mask, 'mask'), po, so, n, c, h * w, _stream()),
               'scf_mul_mask')
    return out


def copy_channels(src: Tensor, dst: Tensor) -> Tensor:
    """copy a sample-strided NCHW tensor into another (same N, C, H, W)."""
    ps, n, c, h, w, ss = _nchw(src, 'src')
    pd, n2, c2, h2, w2, sd = _nchw(dst, 'dst')
    if (n, c, h, w) != (n2, c2, h2, w2):
        raise _lib.ScflowHipError('copy_channels shape mismatch')
    _lib.check(_lib.load().scf_copy_strided(ps, ss, pd, sd, n, c * h * w, _stream()),
               'scf_copy_strided')
    return dst


# ------------------------------------------------- backward of the pose head's fully connected tail (fc_grad.hip)
def _fc_matrix(t: Tensor, what: str, name: str, shape=None) -> Tuple[int, int]:
    _dev(t, f'{what}: {name}')
    if t.dim() != 2 or not t.is_contiguous() or (shape is not None and tuple(t.shape) != tuple(shape)):
        want = 'a contiguous 2-D tensor' if shape is None else f'a contiguous {tuple(shape)} tensor'
        raise _lib.ScflowHipError(f'{what}: {name} must be {want}, got {tuple(t.shape)}')
    return t.shape[0], t.shape[1]


def _fc_parts(x: Tensor, what: str, name: str) -> Tuple[Tensor, int, int, int]:
    _dev(x, f'{what}: {name}')
    if x.dim() == 2:
        x = x.unsqueeze(0)
    if x.dim() != 3 or not x.is_contiguous():
        raise _lib.ScflowHipError(f'{what}: {name} must be a contiguous (M, K) or (parts, M, K) tensor')
    return (x,) + tuple(x.shape)


def _fc_grad_out(out: Optional[Tensor], shape, like: Tensor, what: str, name: str, accumulate: bool = False) -> Tensor:
    if out is None:
        if accumulate:
            raise _lib.ScflowHipError(f'{what}: accumulate needs {name}')
        return torch.empty(shape, dtype=torch.float32, device=like.device)
    _dev(out, f'{what}: {name}')
    if tuple(out.shape) != tuple(shape) or not out.is_contiguous():
        raise _lib.ScflowHipError(f'{what}: {name} must be a contiguous {tuple(shape)} tensor, got {tuple(out.shape)}')
    return out


def fc_operand(x: Tensor, x_bias: Optional[Tensor] = None, x_relu: bool = False, gn=None,
               out: Optional[Tensor] = None) -> Tensor:
    """The (M, K) operand an ``fc_splitk`` launch with the same ``x``, ``x_bias``, ``x_relu``, ``gn`` contracted, in that
    launch's bits (``scf_fc_operand``)."""
    x, parts, m, k = _fc_parts(x, 'fc_operand', 'x')
    _fc_vector(x_bias, k, 'fc_operand', 'x_bias')
    groups, hw, gamma, beta, eps = 0, 1, None, None, 0.0
    if gn is not None:
        groups, hw, gamma, beta, eps = gn
        if hw <= 0 or groups <= 0:
            raise _lib.ScflowHipError('fc_operand: gn groups and hw must be positive')
        _fc_vector(gamma, -(-k // hw), 'fc_operand', 'gamma', at_least=True)
        _fc_vector(beta, -(-k // hw), 'fc_operand', 'beta', at_least=True)
    out = _fc_grad_out(out, (m, k), x, 'fc_operand', 'out')
    _lib.check(_lib.load().scf_fc_operand(x.data_ptr(), parts, m * k, _opt(x_bias, 'x_bias'), int(bool(x_relu)), groups, hw,
                                          _opt(gamma, 'gamma'), _opt(beta, 'beta'), eps, out.data_ptr(), m, k, _stream()),
               'scf_fc_operand')
    return out


def fc_dgrad(g: Tensor, weight: Tensor, a: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """``(g (M, O) @ weight (O, K)) * [a > 0]`` -> (M, K) (``scf_fc_dgrad``; ``a`` None: no mask)."""
    m, o = _fc_matrix(g, 'fc_dgrad', 'g')
    _fc_matrix(weight, 'fc_dgrad', 'weight')
    if weight.shape[0] != o:
        raise _lib.ScflowHipError(f'fc_dgrad: weight must be ({o}, K), got {tuple(weight.shape)}')
    k = weight.shape[1]
    if a is not None:
        _fc_matrix(a, 'fc_dgrad', 'a', (m, k))
    out = _fc_grad_out(out, (m, k), g, 'fc_dgrad', 'out')
    _lib.check(_lib.load().scf_fc_dgrad(g.data_ptr(), weight.data_ptr(), _opt(a, 'a'), out.data_ptr(), m, o, k, _stream()),
               'scf_fc_dgrad')
    return out


def fc_wgrad(g: Tensor, a: Tensor, dw: Optional[Tensor] = None, db: Optional[Tensor] = None, bias: bool = True,
             accumulate: bool = False) -> Tuple[Tensor, Optional[Tensor]]:
    """``(g^T @ a (O, K), g.sum(0) (O))`` (``scf_fc_wgrad``); ``accumulate``: added to ``dw`` / ``db``.  ``bias=False``: no
    ``db``."""
    m, o = _fc_matrix(g, 'fc_wgrad', 'g')
    _fc_matrix(a, 'fc_wgrad', 'a')
    if a.shape[0] != m:
        raise _lib.ScflowHipError(f'fc_wgrad: a must be ({m}, K), got {tuple(a.shape)}')
    k = a.shape[1]
    dw = _fc_grad_out(dw, (o, k), g, 'fc_wgrad', 'dw', accumulate)
    if bias or db is not None:
        db = _fc_grad_out(db, (o,), g, 'fc_wgrad', 'db', accumulate)
    _lib.check(_lib.load().scf_fc_wgrad(g.data_ptr(), a.data_ptr(), dw.data_ptr(), _opt(db, 'db'), m, o, k,
                                        int(bool(accumulate)), _stream()), 'scf_fc_wgrad')
    return dw, db


def pose_select_grad(g_rot: Tensor, g_trans: Tensor, w_rot: Tensor, w_trans: Tensor, a: Tensor, label: Tensor,
                     samples: int, label_mode: int = 0, mask: bool = True, grads=None, accumulate: bool = False):
    """``scf_pose_select_grad``: ``g_rot`` (M, 6), ``g_trans`` (M, 3) (row m = iteration m // samples, sample m % samples),
    the heads' weights and input ``a`` (M, K) -> (g_s (M, K), (dWr, dbr, dWt, dbt)); ``grads``: the four destinations
    (required under ``accumulate``)."""
    what = 'pose_select_grad'
    m, _ = _fc_matrix(g_rot, what, 'g_rot')
    _fc_matrix(g_rot, what, 'g_rot', (m, 6))
    _fc_matrix(g_trans, what, 'g_trans', (m, 3))
    _, k = _fc_matrix(a, what, 'a')
    _fc_matrix(a, what, 'a', (m, k))
    if w_rot.dim() != 2 or w_rot.shape[0] % 6 != 0:
        raise _lib.ScflowHipError(f'{what}: w_rot must be (6 num_class, K), got {tuple(w_rot.shape)}')
    nc = w_rot.shape[0] // 6
    _fc_matrix(w_rot, what, 'w_rot', (6 * nc, k))
    _fc_matrix(w_trans, what, 'w_trans', (3 * nc, k))
    if samples <= 0 or m % samples != 0:
        raise _lib.ScflowHipError(f'{what}: {m} rows are no multiple of {samples} samples')
    if not label.is_cuda or label.dtype != torch.int64 or not label.is_contiguous() or label.numel() < (samples if label_mode & 1 else 1):
        raise _lib.ScflowHipError('label must be a contiguous int64 GPU tensor with one entry per sample')
    shapes = ((6 * nc, k), (6 * nc,), (3 * nc, k), (3 * nc,))
    grads = (None,) * 4 if grads is None else tuple(grads)
    if len(grads) != 4:
        raise _lib.ScflowHipError(f'{what}: grads = (dWr, dbr, dWt, dbt)')
    grads = tuple(_fc_grad_out(t, s, a, what, n, accumulate) for t, s, n in zip(grads, shapes, ('dWr', 'dbr', 'dWt', 'dbt')))
    g_s = torch.empty((m, k), dtype=torch.float32, device=a.device)
    lib = _lib.load()
    head = (g_rot.data_ptr(), g_trans.data_ptr(), w_rot.data_ptr(), w_trans.data_ptr())
    tail = (int(bool(accumulate)), m, k, _stream())
    sel = (label.data_ptr(), samples, nc, label_mode)
    dst = tuple(t.data_ptr() for t in grads)
    if mask:
        _lib.check(lib.scf_pose_select_grad(*head, a.data_ptr(), *sel, g_s.data_ptr(), *dst, *tail), 'scf_pose_select_grad')
    else:       # two calls: the weight gradients need ``a``, the unmasked input gradient must not see it
        _lib.check(lib.scf_pose_select_grad(*head, None, *sel, g_s.data_ptr(), None, None, None, None, *tail),
                   'scf_pose_select_grad')
        _lib.check(lib.scf_pose_select_grad(*head, a.data_ptr(), *sel, None, *dst, *tail), 'scf_pose_select_grad')
    return g_s, grads


def group_norm_flat_grad(g_x0: Tensor, y: Tensor, x0: Tensor, gamma: Tensor, groups: int, hw: int, eps: float = 1e-5,
                         dgamma: Optional[Tensor] = None, dbeta: Optional[Tensor] = None, accumulate: bool = False,
                         params: bool = True):
    """``scf_group_norm_flat_grad``: ``y`` (M, K) or (parts, M, K), the forward's output ``x0`` (M, K) and its cotangent ->
    (g_y (M, K), dgamma, dbeta) with ceil(K / hw) entries each (None with ``params=False``)."""
    what = 'group_norm_flat_grad'
    y, parts, m, k = _fc_parts(y, what, 'y')
    _fc_matrix(g_x0, what, 'g_x0', (m, k))
    _fc_matrix(x0, what, 'x0', (m, k))
    if groups <= 0 or hw <= 0 or k % groups != 0:
        raise _lib.ScflowHipError(f'{what}: {k} features do not split into {groups} groups of channels of {hw}')
    c = -(-k // hw)
    _fc_vector(gamma, c, what, 'gamma', at_least=True)
    if params or dgamma is not None or dbeta is not None:
        dgamma = _fc_grad_out(dgamma, (c,), y, what, 'dgamma', accumulate)
        dbeta = _fc_grad_out(dbeta, (c,), y, what, 'dbeta', accumulate)
    g_y = torch.empty((m, k), dtype=torch.float32, device=y.device)
    stats = torch.empty((m, groups, 2), dtype=torch.float32, device=y.device)
    _lib.check(_lib.load().scf_group_norm_flat_grad(g_x0.data_ptr(), y.data_ptr(), parts, m * k, x0.data_ptr(),
                                                    _dense(gamma, 'gamma'), groups, hw, eps, g_y.data_ptr(),
                                                    _opt(dgamma, 'dgamma'), _opt(dbeta, 'dbeta'), int(bool(accumulate)),
                                                    stats.data_ptr(), m, k, _stream()), 'scf_group_norm_flat_grad')
    return g_y, dgamma, dbeta


# ------------------------------------------------- backward of the pose head's convolutions (conv_grad.hip)
def _conv_grad_map(t: Tensor, what: str, name: str, shape=None) -> Tuple[int, int, int, int]:
    _dev(t, f'{what}: {name}')
    if t.dim() != 4 or not t.is_contiguous() or (shape is not None and tuple(t.shape) != tuple(shape)):
        want = 'a contiguous 4-D tensor' if shape is None else f'a contiguous {tuple(shape)} tensor'
        raise _lib.ScflowHipError(f'{what}: {name} must be {want}, got {tuple(t.shape)}')
    return tuple(t.shape)


def _conv_grad_geometry(what: str, g: Tensor, weight_shape, in_hw, stride: int, padding: int):
    """(M, Cout, Ho, Wo, Cin, Hin, Win) of a 3x3 / stride-2 / pad-1 layer, or an error before the library is reached."""
    m, cout, ho, wo = _conv_grad_map(g, what, 'g')
    if len(weight_shape) != 4 or weight_shape[0] != cout:
        raise _lib.ScflowHipError(f'{what}: the weight must be ({cout}, Cin, 3, 3), got {tuple(weight_shape)}')
    cin, kh, kw = weight_shape[1:]
    if (kh, kw, stride, padding) != (3, 3, 2, 1):
        raise _lib.ScflowHipError(f'{what}: 3x3 / stride 2 / padding 1 only, got {kh}x{kw} / {stride} / {padding}')
    hin, win = in_hw
    if hin < 1 or win < 1 or ho != (hin - 1) // 2 + 1 or wo != (win - 1) // 2 + 1:
        raise _lib.ScflowHipError(f'{what}: a {hin}x{win} input does not give the {ho}x{wo} map of g')
    return m, cout, ho, wo, cin, hin, win


def conv_dgrad(g: Tensor, weight: Tensor, in_hw: Tuple[int, int], split: Optional[int] = None, stride: int = 2,
               padding: int = 1, out=None):
    """Input gradient of ``F.conv2d(x, weight, stride=2, padding=1)`` (``scf_conv_dgrad``): ``g`` (M, Cout, Ho, Wo),
    ``weight`` (Cout, Cin, 3, 3) the raw parameter -> (M, Cin, Hin, Win); ``split`` = C0: the pair of dense tensors
    (M, C0, Hin, Win), (M, Cin - C0, Hin, Win) of a two-part input instead.  ``out``: the destination(s)."""
    what = 'conv_dgrad'
    _dev(weight, f'{what}: weight')
    if not weight.is_contiguous():
        raise _lib.ScflowHipError(f'{what}: weight must be contiguous')
    m, cout, ho, wo, cin, hin, win = _conv_grad_geometry(what, g, tuple(weight.shape), in_hw, stride, padding)
    c0 = cin if split is None else int(split)
    c1 = cin - c0
    if c0 < 1 or c1 < 0 or (split is not None and c1 < 1):
        raise _lib.ScflowHipError(f'{what}: split {split} leaves no channels on one side of {cin}')
    outs = (out,) if split is None else ((None, None) if out is None else tuple(out))
    if len(outs) != (1 if split is None else 2):
        raise _lib.ScflowHipError(f'{what}: out must hold one destination per input part')
    gx0 = _fc_grad_out(outs[0], (m, c0, hin, win), g, what, 'out[0]')
    gx1 = _fc_grad_out(outs[1], (m, c1, hin, win), g, what, 'out[1]') if split is not None else None
    _lib.check(_lib.load().scf_conv_dgrad(g.data_ptr(), weight.data_ptr(), gx0.data_ptr(), c0,
                                          None if gx1 is None else gx1.data_ptr(), c1, m, cout, ho, wo, hin, win, 3, 3,
                                          stride, padding, _stream()), 'scf_conv_dgrad')
    return gx0 if split is None else (gx0, gx1)


def _workspace_floats(query: str, *sizes: int) -> int:
    """what the library's ``scf_<query>`` answers for ``sizes``; a negative answer is its refusal of them"""
    n = int(getattr(_lib.load(), 'scf_' + query)(*sizes))
    if n < 0:
        raise _lib.ScflowHipError(f'{query}: invalid sizes {sizes}')
    return n


def conv_wgrad_workspace(m: int, cout: int, cin: int, ho: int, wo: int) -> int:
    """floats of workspace ``conv_wgrad`` needs (``scf_conv_wgrad_workspace``)."""
    return _workspace_floats('conv_wgrad_workspace', m, cout, cin, ho, wo)


def conv_wgrad(g: Tensor, x0: Tensor, x1: Optional[Tensor] = None, dw: Optional[Tensor] = None, accumulate: bool = False,
               workspace: Optional[Tensor] = None, stride: int = 2, padding: int = 1, kernel_size: int = 3) -> Tensor:
    """Weight gradient of ``F.conv2d(cat(x0, x1), weight, stride=2, padding=1)`` (``scf_conv_wgrad``): ``g`` (M, Cout, Ho,
    Wo), ``x0`` (M, C0, Hin, Win), ``x1`` (M, C1, Hin, Win) or None -> (Cout, C0 + C1, 3, 3); ``accumulate``: added to
    ``dw``.  ``workspace``: a float32 tensor of at least ``conv_wgrad_workspace`` elements (allocated when None)."""
    what = 'conv_wgrad'
    m, c0, hin, win = _conv_grad_map(x0, what, 'x0')
    c1 = 0
    if x1 is not None:
        c1 = _conv_grad_map(x1, what, 'x1')[1]
        _conv_grad_map(x1, what, 'x1', (m, c1, hin, win))
    cin = c0 + c1
    _conv_grad_map(g, what, 'g')
    if g.shape[0] != m:
        raise _lib.ScflowHipError(f'{what}: g holds {g.shape[0]} samples, x0 {m}')
    _, cout, ho, wo, _, _, _ = _conv_grad_geometry(what, g, (g.shape[1], cin, kernel_size, kernel_size), (hin, win), stride,
                                                   padding)
    dw = _fc_grad_out(dw, (cout, cin, 3, 3), g, what, 'dw', accumulate)
    workspace = _grad_workspace(what, workspace, conv_wgrad_workspace(m, cout, cin, ho, wo), g)
    _lib.check(_lib.load().scf_conv_wgrad(g.data_ptr(), x0.data_ptr(), c0, None if x1 is None else x1.data_ptr(), c1,
                                          dw.data_ptr(), int(bool(accumulate)), workspace.data_ptr(), workspace.numel(), m,
                                          cout, ho, wo, hin, win, 3, 3, stride, padding, _stream()), 'scf_conv_wgrad')
    return dw


# ------------------------------------------------- backward of the stride-1 convolutions with bias (conv_s1_grad.hip)
S1_KERNELS = (1, 3, 5, 7)                        # KH and KW, chosen independently; pad = (KH // 2, KW // 2)
_S1_ACTS = (ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH)


def _s1_map(t: Tensor, what: str, name: str, shape=None) -> Tuple[int, int]:
    """(pointer, sample stride) of a (M, C, H, W) float32 tensor that is contiguous up to a channel slice."""
    ptr, n, c, h, w, sn = _nchw(t, f'{what}: {name}')
    if shape is not None and (n, c, h, w) != tuple(shape):
        raise _lib.ScflowHipError(f'{what}: {name} must be {tuple(shape)}, got {(n, c, h, w)}')
    if sn < c * h * w:
        raise _lib.ScflowHipError(f'{what}: {name} has a sample stride {sn} below its {c * h * w} elements a sample')
    return ptr, sn


def _s1_weight_shape(what: str, shape) -> Tuple[int, int, int, int]:
    if len(shape) != 4:
        raise _lib.ScflowHipError(f'{what}: the weight must be (Cout, Cin, KH, KW), got {tuple(shape)}')
    cout, cin, kh, kw = (int(v) for v in shape)
    if kh not in S1_KERNELS or kw not in S1_KERNELS:
        raise _lib.ScflowHipError(f'{what}: KH and KW must each be one of {S1_KERNELS}, got {kh}x{kw}')
    if cout < 1 or cin < 1:
        raise _lib.ScflowHipError(f'{what}: the weight must hold channels, got {tuple(shape)}')
    return cout, cin, kh, kw


def _s1_act(what: str, act: int, a: Optional[Tensor]) -> None:
    if act not in _S1_ACTS:
        raise _lib.ScflowHipError(f'{what}: unknown activation code {act}')
    if (act != ACT_NONE) != (a is not None):
        raise _lib.ScflowHipError(f'{what}: a (the post-activation value) is needed exactly when act != ACT_NONE')


def act_grad(g: Tensor, a: Optional[Tensor], act: int, out: Optional[Tensor] = None) -> Tensor:
    """``g * act'(a)`` elementwise (``scf_act_grad``): ``g``, ``a``, ``out`` (M, C, H, W), each contiguous up to a channel
    slice; ``a`` the forward's post-activation value (None exactly with ``ACT_NONE``)."""
    what = 'act_grad'
    _s1_act(what, act, a)
    pg, gs = _s1_map(g, what, 'g')
    shape = tuple(g.shape)
    pa, sa = (None, 0) if a is None else _s1_map(a, what, 'a', shape)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=g.device)
    po, so = _s1_map(out, what, 'out', shape)
    m, c, h, w = shape
    if m * c * h * w == 0:
        raise _lib.ScflowHipError(f'{what}: empty tensor {shape}')
    _lib.check(_lib.load().scf_act_grad(pg, gs, pa, sa, act, po, so, m, c * h * w, _stream()), 'scf_act_grad')
    return out


def conv_s1_dgrad(g: Tensor, weight: Tensor, add: Optional[Tensor] = None, a: Optional[Tensor] = None,
                  act: int = ACT_NONE, out: Optional[Tensor] = None, w_scratch: Optional[Tensor] = None) -> Tensor:
    """Input gradient of ``F.conv2d(x, weight, padding=(KH // 2, KW // 2))`` with a second cotangent and the activation
    backward of the layer in front fused (``scf_conv_s1_dgrad``): ``act'(a) * (dgrad(g, weight) + add)``.  ``g`` (M, Cout,
    H, W); ``weight`` (Cout, Cin, KH, KW) the raw parameter; ``add``, ``a``, ``out`` (M, Cin, H, W); all maps contiguous up to
    a channel slice.  ``w_scratch``: at least ``weight.numel()`` floats for the transposed copy the MFMA route reads."""
    what = 'conv_s1_dgrad'
    _dev(weight, f'{what}: weight')
    if not weight.is_contiguous():
        raise _lib.ScflowHipError(f'{what}: weight must be contiguous')
    cout, cin, kh, kw = _s1_weight_shape(what, tuple(weight.shape))
    _s1_act(what, act, a)
    pg, gs = _s1_map(g, what, 'g')
    m, gc, h, w = g.shape
    if gc != cout or m * h * w == 0:
        raise _lib.ScflowHipError(f'{what}: g must be (M, {cout}, H, W) with M, H, W >= 1, got {tuple(g.shape)}')
    shape = (m, cin, h, w)
    padd, sadd = (None, 0) if add is None else _s1_map(add, what, 'add', shape)
    pa, sa = (None, 0) if a is None else _s1_map(a, what, 'a', shape)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=g.device)
    po, so = _s1_map(out, what, 'out', shape)
    ps = None
    if w_scratch is not None:
        ps = _dense(w_scratch, f'{what}: w_scratch')
        _fc_vector(w_scratch, weight.numel(), what, 'w_scratch', at_least=True)
    _lib.check(_lib.load().scf_conv_s1_dgrad(pg, gs, weight.data_ptr(), padd, sadd, pa, sa, act, po, so, ps, m, cout, cin,
                                             h, w, kh, kw, _stream()), 'scf_conv_s1_dgrad')
    return out


def conv_s1_wgrad_workspace(m: int, cout: int, cin: int, h: int, w: int, kh: int, kw: int) -> int:
    """floats of workspace ``conv_s1_wgrad`` needs (``scf_conv_s1_wgrad_workspace``)."""
    return _workspace_floats('conv_s1_wgrad_workspace', m, cout, cin, h, w, kh, kw)


def conv_s1_wgrad(g: Tensor, x: Tensor, kernel_size, dw: Optional[Tensor] = None, db: Optional[Tensor] = None,
                  bias: bool = True, accumulate: bool = False, workspace: Optional[Tensor] = None):
    """Weight and bias gradient of ``F.conv2d(x, weight, bias, padding=(KH // 2, KW // 2))`` (``scf_conv_s1_wgrad``): ``g``
    (M, Cout, H, W), ``x`` (M, Cin, H, W), both contiguous up to a channel slice, ``kernel_size`` (KH, KW) -> (dw (Cout, Cin,
    KH, KW), db (Cout,) or None with ``bias=False``); ``accumulate``: added to ``dw`` / ``db``.  ``workspace``: a float32
    tensor of at least ``conv_s1_wgrad_workspace`` elements (allocated when None)."""
    what = 'conv_s1_wgrad'
    pg, gs = _s1_map(g, what, 'g')
    m, cout, h, w = g.shape
    px, xs = _s1_map(x, what, 'x')
    if x.shape[0] != m or tuple(x.shape[2:]) != (h, w):
        raise _lib.ScflowHipError(f'{what}: x {tuple(x.shape)} does not match g {tuple(g.shape)}')
    cin = x.shape[1]
    kh, kw = (kernel_size, kernel_size) if isinstance(kernel_size, int) else tuple(kernel_size)
    _s1_weight_shape(what, (cout, cin, kh, kw))
    if m * h * w == 0:
        raise _lib.ScflowHipError(f'{what}: empty maps {tuple(g.shape)}')
    dw = _fc_grad_out(dw, (cout, cin, kh, kw), g, what, 'dw', accumulate)
    if bias or db is not None:
        db = _fc_grad_out(db, (cout,), g, what, 'db', accumulate)
    workspace = _grad_workspace(what, workspace, conv_s1_wgrad_workspace(m, cout, cin, h, w, kh, kw), g)
    _lib.check(_lib.load().scf_conv_s1_wgrad(pg, gs, px, xs, dw.data_ptr(), None if db is None else db.data_ptr(),
                                             int(bool(accumulate)), workspace.data_ptr(), workspace.numel(), m, cout, cin,
                                             h, w, kh, kw, _stream()), 'scf_conv_s1_wgrad')
    return dw, db


# ------------------------------------------------- backward of the context encoder's remaining layers (encoder_grad.hip)
def _half_map(what: str, g: Tensor, x_shape) -> None:
    m, _, ho, wo = g.shape
    xm, _, hin, win = x_shape
    if xm != m or m * hin * win == 0 or ho != (hin - 1) // 2 + 1 or wo != (win - 1) // 2 + 1:
        raise _lib.ScflowHipError(f'{what}: a {tuple(x_shape)} input does not give the map of g {tuple(g.shape)}')


def _grad_workspace(what: str, workspace: Optional[Tensor], need: int, like: Tensor) -> Tensor:
    if workspace is None:
        workspace = torch.empty((need,), dtype=torch.float32, device=like.device)
    _dev(workspace, f'{what}: workspace')
    if not workspace.is_contiguous() or workspace.numel() < need:
        raise _lib.ScflowHipError(f'{what}: workspace must be contiguous with at least {need} floats, got {workspace.numel()}')
    return workspace


def conv_stem_wgrad_workspace(m: int, cout: int, cin: int, ho: int, wo: int) -> int:
    """floats of workspace ``conv_stem_wgrad`` needs (``scf_conv_stem_wgrad_workspace``)."""
    return _workspace_floats('conv_stem_wgrad_workspace', m, cout, cin, ho, wo)


def conv_stem_wgrad(g: Tensor, x: Tensor, dw: Optional[Tensor] = None, db: Optional[Tensor] = None, bias: bool = True,
                    accumulate: bool = False, workspace: Optional[Tensor] = None, kernel_size: int = 7, stride: int = 2,
                    padding: int = 3):
    """Weight and bias gradient of the encoder stem ``F.conv2d(x, weight, bias, stride=2, padding=3)`` with a 7x7 kernel and
    at most 4 input channels (``scf_conv_stem_wgrad``): ``g`` (M, Cout, Ho, Wo), ``x`` (M, Cin, Hin, Win), both contiguous up
    to a channel slice -> (dw (Cout, Cin, 7, 7), db (Cout,) or None with ``bias=False``); ``accumulate``: added to them."""
    what = 'conv_stem_wgrad'
    pg, gs = _s1_map(g, what, 'g')
    px, xs = _s1_map(x, what, 'x')
    if (kernel_size, stride, padding) != (7, 2, 3):
        raise _lib.ScflowHipError(f'{what}: 7x7 / stride 2 / padding 3 only, got {kernel_size} / {stride} / {padding}')
    _half_map(what, g, tuple(x.shape))
    m, cout, ho, wo = g.shape
    cin, hin, win = x.shape[1:]
    if not 1 <= cin <= 4 or cout < 1:
        raise _lib.ScflowHipError(f'{what}: 1 .. 4 input channels, got {cin}')
    dw = _fc_grad_out(dw, (cout, cin, 7, 7), g, what, 'dw', accumulate)
    if bias or db is not None:
        db = _fc_grad_out(db, (cout,), g, what, 'db', accumulate)
    workspace = _grad_workspace(what, workspace, conv_stem_wgrad_workspace(m, cout, cin, ho, wo), g)
    _lib.check(_lib.load().scf_conv_stem_wgrad(pg, gs, px, xs, dw.data_ptr(), None if db is None else db.data_ptr(),
                                               int(bool(accumulate)), workspace.data_ptr(), workspace.numel(), m, cout, cin,
                                               ho, wo, hin, win, 7, 7, 2, 3, _stream()), 'scf_conv_stem_wgrad')
    return dw, db


def conv_ds_dgrad(g: Tensor, weight: Tensor, in_hw: Tuple[int, int], add: Optional[Tensor] = None,
                  a: Optional[Tensor] = None, act: int = ACT_NONE, out: Optional[Tensor] = None) -> Tensor:
    """The join at the input of a down-sampling block (``scf_conv_ds_dgrad``): ``act'(a) * (add + dgrad)`` with ``dgrad`` the
    input gradient of the 1x1 / stride-2 shortcut ``F.conv2d(x, weight, stride=2)``, non-zero at the even pixels only.
    ``g`` (M, Cout, Ho, Wo); ``weight`` (Cout, Cin, 1, 1) or (Cout, Cin); ``add`` (the 3x3 / stride-2 layer's input
    gradient), ``a``, ``out`` (M, Cin, Hin, Win) with (Hin, Win) = ``in_hw``; all maps contiguous up to a channel slice."""
    what = 'conv_ds_dgrad'
    _dev(weight, f'{what}: weight')
    if not weight.is_contiguous() or weight.dim() not in (2, 4) or tuple(weight.shape[2:]) not in ((), (1, 1)):
        raise _lib.ScflowHipError(f'{what}: weight must be a contiguous (Cout, Cin, 1, 1) tensor, got {tuple(weight.shape)}')
    cout, cin = weight.shape[:2]
    _s1_act(what, act, a)
    pg, gs = _s1_map(g, what, 'g')
    m, gc = g.shape[:2]
    hin, win = in_hw
    if gc != cout or cin < 1:
        raise _lib.ScflowHipError(f'{what}: g must be (M, {cout}, Ho, Wo), got {tuple(g.shape)}')
    shape = (m, cin, hin, win)
    _half_map(what, g, shape)
    padd, sadd = (None, 0) if add is None else _s1_map(add, what, 'add', shape)
    pa, sa = (None, 0) if a is None else _s1_map(a, what, 'a', shape)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=g.device)
    po, so = _s1_map(out, what, 'out', shape)
    _lib.check(_lib.load().scf_conv_ds_dgrad(pg, gs, weight.data_ptr(), padd, sadd, pa, sa, act, po, so, m, cout, cin,
                                             g.shape[2], g.shape[3], hin, win, _stream()), 'scf_conv_ds_dgrad')
    return out


def conv_ds_wgrad_workspace(m: int, cout: int, cin: int, ho: int, wo: int) -> int:
    """floats of workspace ``conv_ds_wgrad`` needs (``scf_conv_ds_wgrad_workspace``)."""
    return _workspace_floats('conv_ds_wgrad_workspace', m, cout, cin, ho, wo)


def conv_ds_wgrad(g: Tensor, x: Tensor, dw: Optional[Tensor] = None, db: Optional[Tensor] = None, bias: bool = True,
                  accumulate: bool = False, workspace: Optional[Tensor] = None):
    """Weight and bias gradient of the 1x1 / stride-2 shortcut ``F.conv2d(x, weight, bias, stride=2)``
    (``scf_conv_ds_wgrad``): ``g`` (M, Cout, Ho, Wo), ``x`` (M, Cin, Hin, Win), both contiguous up to a channel slice ->
    (dw (Cout, Cin, 1, 1), db (Cout,) or None with ``bias=False``); ``accumulate``: added to them."""
    what = 'conv_ds_wgrad'
    pg, gs = _s1_map(g, what, 'g')
    px, xs = _s1_map(x, what, 'x')
    _half_map(what, g, tuple(x.shape))
    m, cout, ho, wo = g.shape
    cin, hin, win = x.shape[1:]
    if cin < 1 or cout < 1:
        raise _lib.ScflowHipError(f'{what}: empty channels {tuple(g.shape)}, {tuple(x.shape)}')
    dw = _fc_grad_out(dw, (cout, cin, 1, 1), g, what, 'dw', accumulate)
    if bias or db is not None:
        db = _fc_grad_out(db, (cout,), g, what, 'db', accumulate)
    workspace = _grad_workspace(what, workspace, conv_ds_wgrad_workspace(m, cout, cin, ho, wo), g)
    _lib.check(_lib.load().scf_conv_ds_wgrad(pg, gs, px, xs, dw.data_ptr(), None if db is None else db.data_ptr(),
                                             int(bool(accumulate)), workspace.data_ptr(), workspace.numel(), m, cout, cin,
                                             ho, wo, hin, win, _stream()), 'scf_conv_ds_wgrad')
    return dw, db


def channel_sum_workspace(m: int, c: int, n: int) -> int:
    """floats of workspace ``channel_sum`` needs (``scf_channel_sum_workspace``)."""
    return _workspace_floats('channel_sum_workspace', m, c, n)


def channel_sum(g: Tensor, out: Optional[Tensor] = None, accumulate: bool = False,
                workspace: Optional[Tensor] = None) -> Tensor:
    """``g.sum((0, 2, 3))`` in one fixed order (``scf_channel_sum``): the bias gradient of a layer whose weight gradient has
    none.  ``g`` (M, C, H, W), contiguous up to a channel slice -> (C,); ``accumulate``: added to ``out``."""
    what = 'channel_sum'
    pg, gs = _s1_map(g, what, 'g')
    m, c, h, w = g.shape
    if m * c * h * w == 0:
        raise _lib.ScflowHipError(f'{what}: empty tensor {tuple(g.shape)}')
    out = _fc_grad_out(out, (c,), g, what, 'out', accumulate)
    workspace = _grad_workspace(what, workspace, channel_sum_workspace(m, c, h * w), g)
    _lib.check(_lib.load().scf_channel_sum(pg, gs, out.data_ptr(), int(bool(accumulate)), workspace.data_ptr(),
                                           workspace.numel(), m, c, h * w, _stream()), 'scf_channel_sum')
    return out


def _bn_vectors(what: str, cout: int, **named) -> list:
    ptrs = []
    for name, t in named.items():
        ptrs.append(_dense(t, f'{what}: {name}'))
        if tuple(t.shape) != (cout,):
            raise _lib.ScflowHipError(f'{what}: {name} must be ({cout},), got {tuple(t.shape)}')
    return ptrs


def _bn_weight(what: str, weight: Tensor, name: str = 'weight', shape=None) -> Tuple[int, int]:
    _dev(weight, f'{what}: {name}')
    if weight.dim() < 2 or not weight.is_contiguous() or weight.numel() == 0 or (
            shape is not None and tuple(weight.shape) != tuple(shape)):
        raise _lib.ScflowHipError(f'{what}: {name} must be a contiguous (Cout, ...) tensor'
                                  f'{"" if shape is None else " of shape " + str(tuple(shape))}, got {tuple(weight.shape)}')
    return weight.shape[0], weight.numel() // weight.shape[0]


def bn_fold(weight: Tensor, bias: Tensor, gamma: Tensor, beta: Tensor, mean: Tensor, var: Tensor, eps: float,
            out: Optional[Tuple[Tensor, Tensor]] = None) -> Tuple[Tensor, Tensor]:
    """Eval-mode BatchNorm folded into the convolution in front (``scf_bn_fold``): (W', b') of ``y = W' * x + b'`` with
    ``s = gamma / sqrt(var + eps)``, ``W' = s W``, ``b' = beta + s (b - mean)``, in the raw torch layout."""
    what = 'bn_fold'
    cout, k = _bn_weight(what, weight)
    ptrs = _bn_vectors(what, cout, bias=bias, gamma=gamma, beta=beta, mean=mean, var=var)
    wf, bf = (None, None) if out is None else out
    wf = _fc_grad_out(wf, tuple(weight.shape), weight, what, 'out[0]')
    bf = _fc_grad_out(bf, (cout,), weight, what, 'out[1]')
    _lib.check(_lib.load().scf_bn_fold(weight.data_ptr(), *ptrs, float(eps), wf.data_ptr(), bf.data_ptr(), cout, k,
                                       _stream()), 'scf_bn_fold')
    return wf, bf


def bn_unfold(weight: Tensor, bias: Tensor, gamma: Tensor, mean: Tensor, var: Tensor, eps: float, dwf: Tensor, dbf: Tensor,
              out: Optional[Sequence[Optional[Tensor]]] = None, accumulate: bool = False):
    """The folded layer's gradients (``dwf``, ``dbf``) carried to the raw parameters (``scf_bn_unfold``) ->
    (d conv.weight, d conv.bias, d bn.weight, d bn.bias); ``out``: the four destinations, ``accumulate``: added to them."""
    what = 'bn_unfold'
    cout, k = _bn_weight(what, weight)
    _bn_weight(what, dwf, 'dwf', tuple(weight.shape))
    pb, pg, pm, pv, pdb = _bn_vectors(what, cout, bias=bias, gamma=gamma, mean=mean, var=var, dbf=dbf)
    outs = (None,) * 4 if out is None else tuple(out)
    if len(outs) != 4:
        raise _lib.ScflowHipError(f'{what}: out holds the four destinations (dw, db, dgamma, dbeta)')
    dw = _fc_grad_out(outs[0], tuple(weight.shape), weight, what, 'out[0]', accumulate)
    vec = [_fc_grad_out(o, (cout,), weight, what, f'out[{i + 1}]', accumulate) for i, o in enumerate(outs[1:])]
    if dw.data_ptr() == dwf.data_ptr():
        raise _lib.ScflowHipError(f'{what}: out[0] must not alias dwf')
    _lib.check(_lib.load().scf_bn_unfold(weight.data_ptr(), pb, pg, pm, pv, float(eps), dwf.data_ptr(), pdb, dw.data_ptr(),
                                         *(v.data_ptr() for v in vec), int(bool(accumulate)), cout, k, _stream()),
               'scf_bn_unfold')
    return (dw, *vec)


# ------------------------------------------------- backward of InstanceNorm (instance_norm_grad.hip)
def instance_norm_grad(g: Tensor, u: Tensor, y: Optional[Tensor] = None, r: Optional[Tensor] = None, eps: float = 1e-5,
                       out: Optional[Sequence[Optional[Tensor]]] = None):
    """Backward of ``instance_norm`` with respect to its raw input(s) (``scf_instance_norm_grad``,
    ``scf_instance_norm_res_norm_grad``).  ``u``: the raw convolution output the forward normalised; the statistics are
    recomputed from it.  Every operand a contiguous (N, C, H, W) tensor of one shape.  Three forms:

    * ``y`` None (``relu(IN(u))``): ``g`` is the cotangent at ``IN(u)``, already masked by the consumer -> ``du``;
    * ``y`` given (``y = relu(IN(u) + res)``): ``g`` the cotangent at ``y`` -> ``(g', du)`` with ``g' = g [y > 0]``, which
      is also the cotangent of ``res``;
    * ``y`` and ``r`` given (``y = relu(IN(u) + IN(r))``, ``res_norm=True``): -> ``(du, dr)``.

    ``out``: the destination(s) in the order returned (None entries are allocated); ``du`` may be ``g`` itself."""
    what = 'instance_norm_grad'
    if g.dim() != 4 or g.numel() == 0:
        raise _lib.ScflowHipError(f'{what}: g must be a non-empty (N, C, H, W) tensor, got {tuple(g.shape)}')
    if r is not None and y is None:
        raise _lib.ScflowHipError(f'{what}: r (a normalised shortcut) comes with y, the block\'s output')
    shape = tuple(g.shape)
    named = dict(g=g, u=u, y=y, r=r)
    nout = 1 if y is None else 2
    outs = [None] * nout if out is None else ([out] if isinstance(out, torch.Tensor) else list(out))
    if len(outs) != nout:
        raise _lib.ScflowHipError(f'{what}: out holds {nout} destination(s) in this form, got {len(outs)}')
    outs = [torch.empty(shape, dtype=torch.float32, device=g.device) if o is None else o for o in outs]
    named.update({f'out[{i}]': o for i, o in enumerate(outs)})
    ptr = {}
    for k, t in named.items():
        if t is None:
            ptr[k] = None
            continue
        ptr[k] = _dense(t, f'{what}: {k}')
        if tuple(t.shape) != shape:
            raise _lib.ScflowHipError(f'{what}: {k} must be {shape} like g, got {tuple(t.shape)}')
    n, c, h, w = shape
    lib = _lib.load()
    if r is None:
        gp, du = (None, ptr['out[0]']) if y is None else (ptr['out[0]'], ptr['out[1]'])
        _lib.check(lib.scf_instance_norm_grad(ptr['g'], ptr['y'], ptr['u'], gp, du, n * c, h * w, float(eps), _stream()),
                   'scf_instance_norm_grad')
    else:
        _lib.check(lib.scf_instance_norm_res_norm_grad(ptr['g'], ptr['y'], ptr['u'], ptr['r'], ptr['out[0]'], ptr['out[1]'],
                                                       n * c, h * w, float(eps), _stream()), 'scf_instance_norm_res_norm_grad')
    return outs[0] if nout == 1 else tuple(outs)


# ------------------------------------------------- BatchNorm on batch statistics (batch_norm_train.hip)
def batch_norm_train_workspace(n: int, c: int, hw: int) -> int:
    """floats of workspace ``batch_norm_train`` / ``batch_norm_train_grad`` need (``scf_batch_norm_train_workspace``)."""
    return _workspace_floats('batch_norm_train_workspace', n, c, hw)


def batch_norm_train_route(n: int, c: int, hw: int, aligned: bool = True) -> dict:
    """what ``batch_norm_train`` / ``batch_norm_train_grad`` launch for (N, C, HW) maps, ``aligned``: all of them on 16-byte
    boundaries (``scf_batch_norm_train_route``, the launcher's own decision; a host call) -> dict(stats: float4 per thread
    of the statistics kernel, 1, 4 or 16, or 'loop'; vec: float4 sweeps; K: chunks per plane; bpp: apply blocks per plane;
    groups: groups of 64 partials per channel)."""
    r = (C.c_int * 5)()
    _lib.check(_lib.load().scf_batch_norm_train_route(int(n), int(c), int(hw), int(bool(aligned)), r),
               'scf_batch_norm_train_route')
    return dict(stats=int(r[0]) or 'loop', vec=bool(r[1]), K=int(r[2]), bpp=int(r[3]), groups=int(r[4]))


def _bnt_maps(what: str, shape, named: dict) -> dict:
    """the data pointers of the (N, C, H, W) operands ``named`` (None stays None), each dense and of ``shape``"""
    ptr = {}
    for k, t in named.items():
        if t is None:
            ptr[k] = None
            continue
        ptr[k] = _dense(t, f'{what}: {k}')
        if tuple(t.shape) != shape:
            raise _lib.ScflowHipError(f'{what}: {k} must be {shape} like {next(iter(named))}, got {tuple(t.shape)}')
    return ptr


def _bnt_shape(what: str, t: Tensor, name: str) -> Tuple[int, int, int, int]:
    if not isinstance(t, torch.Tensor) or t.dim() != 4 or t.numel() == 0:
        raise _lib.ScflowHipError(f'{what}: {name} must be a non-empty (N, C, H, W) tensor, got '
                                  f'{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}')
    n, c, h, w = t.shape
    if n * h * w == 1:
        raise _lib.ScflowHipError(f'{what}: one value per channel ({tuple(t.shape)}) has no batch statistics')
    return n, c, h, w


def _bnt_out(t: Optional[Tensor], shape, like: Tensor) -> Tensor:
    return torch.empty(shape, dtype=torch.float32, device=like.device) if t is None else t


def batch_norm_train(u: Tensor, gamma: Tensor, beta: Tensor, running_mean: Optional[Tensor], running_var: Optional[Tensor],
                     momentum: Optional[float] = 0.1, eps: float = 1e-5, res: Optional[Tensor] = None, relu: bool = False,
                     res_bn: Optional[Sequence[Optional[Tensor]]] = None, out: Optional[Tensor] = None,
                     workspace: Optional[Tensor] = None):
    """Training-mode ``BatchNorm2d`` of the raw convolution output ``u`` (N, C, H, W) on the statistics of the batch
    (``scf_batch_norm_train``): biased variance for normalising, ``running = (1 - momentum) running + momentum batch`` with
    the unbiased variance, updated in place (both None: none are kept).  Three forms:

    * ``res`` None: ``BN(u)``, with ``relu`` the encoder's ``relu(BN(u))`` -> ``(y, saved)``;
    * ``res`` given: ``BN(u) + res`` -> ``(y, saved)``;
    * ``res`` and ``res_bn = (gamma, beta, running_mean, running_var)`` given: ``BN(u) + BN_b(res)``, ``res`` the raw
      output of a shortcut convolution with its own parameters and statistics -> ``(y, saved, saved_r)``.

    ``saved``: (2, C), the batch mean and ``rstd = 1 / sqrt(var + eps)``, what ``batch_norm_train_grad`` reads.  ``out``:
    the destination of ``y`` (it must not alias an operand).  ``momentum=None`` (torch's cumulative average) is not built."""
    what = 'batch_norm_train'
    if momentum is None:
        raise NotImplementedError(f'{what}: momentum=None (the cumulative moving average) is not implemented')
    n, c, h, w = _bnt_shape(what, u, 'u')
    shape = (n, c, h, w)
    if res_bn is not None and res is None:
        raise _lib.ScflowHipError(f'{what}: res_bn (a normalised shortcut\'s parameters) comes with res, its raw output')
    if res_bn is not None and len(res_bn) != 4:
        raise _lib.ScflowHipError(f'{what}: res_bn holds (gamma, beta, running_mean, running_var)')
    y = _bnt_out(out, shape, u)
    ptr = _bnt_maps(what, shape, dict(u=u, res=res, out=y))
    if any(y.data_ptr() == t.data_ptr() for t in (u, res) if t is not None):
        raise _lib.ScflowHipError(f'{what}: out must not alias u or res (the backward reads the raw u)')

    def vectors(tag, g, b, rm, rv):
        if (rm is None) != (rv is None):
            raise _lib.ScflowHipError(f'{what}: running_mean{tag} and running_var{tag} come together')
        named = {f'gamma{tag}': g, f'beta{tag}': b}
        if rm is not None:
            named.update({f'running_mean{tag}': rm, f'running_var{tag}': rv})
        ptrs = _bn_vectors(what, c, **named)
        return ptrs + [None] * (4 - len(ptrs))

    pa = vectors('', gamma, beta, running_mean, running_var)
    pb = [None] * 4 if res_bn is None else vectors('_r', *res_bn)
    saved = torch.empty((2, c), dtype=torch.float32, device=u.device)
    saved_r = None if res_bn is None else torch.empty((2, c), dtype=torch.float32, device=u.device)
    workspace = _grad_workspace(what, workspace, batch_norm_train_workspace(n, c, h * w), u)
    _lib.check(_lib.load().scf_batch_norm_train(
        ptr['u'], *pa, ptr['res'], *pb, int(bool(relu)), float(momentum), float(eps), ptr['out'], saved.data_ptr(),
        None if saved_r is None else saved_r.data_ptr(), workspace.data_ptr(), workspace.numel(), n, c, h * w, _stream()),
        'scf_batch_norm_train')
    return (y, saved) if saved_r is None else (y, saved, saved_r)


def batch_norm_train_grad(g: Tensor, u: Tensor, saved: Tensor, gamma: Tensor, y: Optional[Tensor] = None,
                          r: Optional[Tensor] = None, saved_r: Optional[Tensor] = None, gamma_r: Optional[Tensor] = None,
                          out: Optional[Sequence[Optional[Tensor]]] = None, accumulate: bool = False,
                          workspace: Optional[Tensor] = None):
    """Backward of ``batch_norm_train`` with respect to its raw input(s) and its affine parameters
    (``scf_batch_norm_train_grad``).  ``u``: the raw convolution output the forward normalised, ``saved`` its (2, C)
    statistics from that forward (they are not recomputed).  Every map a contiguous (N, C, H, W) tensor of one shape.

    * ``y`` None (``relu(BN(u))``): ``g`` is the cotangent at ``BN(u)``, already masked by the consumer
      -> ``(du, dgamma, dbeta)``;
    * ``y`` given (``y = relu(BN(u) + res)``): ``g`` the cotangent at ``y`` -> ``(g', du, dgamma, dbeta)`` with
      ``g' = g [y > 0]``, which is also the cotangent of ``res``;
    * ``y``, ``r``, ``saved_r``, ``gamma_r`` given (``y = relu(BN(u) + BN_b(r))``)
      -> ``(du, dr, dgamma, dbeta, dgamma_r, dbeta_r)``.

    ``out``: the destinations in the order returned (None entries are allocated); ``accumulate``: the parameter gradients
    are added to their destinations, as ``bn_unfold`` has it.  ``du`` may be ``g`` itself in the first form."""
    what = 'batch_norm_train_grad'
    n, c, h, w = _bnt_shape(what, g, 'g')
    shape = (n, c, h, w)
    if r is not None and y is None:
        raise _lib.ScflowHipError(f'{what}: r (a normalised shortcut) comes with y, the block\'s output')
    if (r is None) != (saved_r is None) or (r is None) != (gamma_r is None):
        raise _lib.ScflowHipError(f'{what}: r, saved_r and gamma_r (a normalised shortcut) come together')
    nmap = 1 if y is None else 2
    nvec = 2 if r is None else 4
    outs = [None] * (nmap + nvec) if out is None else list(out)
    if len(outs) != nmap + nvec:
        raise _lib.ScflowHipError(f'{what}: out holds {nmap} + {nvec} destinations in this form, got {len(outs)}')
    maps = [_bnt_out(o, shape, g) for o in outs[:nmap]]
    vecs = [_fc_grad_out(o, (c,), g, what, f'out[{nmap + i}]', accumulate) for i, o in enumerate(outs[nmap:])]
    named = dict(g=g, u=u, y=y, r=r)
    named.update({f'out[{i}]': o for i, o in enumerate(maps)})
    ptr = _bnt_maps(what, shape, named)
    stats = dict(saved=saved) if r is None else dict(saved=saved, saved_r=saved_r)
    for k, t in stats.items():
        _dense(t, f'{what}: {k}')
        if tuple(t.shape) != (2, c):
            raise _lib.ScflowHipError(f'{what}: {k} must be (2, {c}), the forward\'s (mean, rstd), got {tuple(t.shape)}')
    pg = _bn_vectors(what, c, **(dict(gamma=gamma) if r is None else dict(gamma=gamma, gamma_r=gamma_r)))
    if r is None:
        gp, du, dr = (None, ptr['out[0]'], None) if y is None else (ptr['out[0]'], ptr['out[1]'], None)
    else:
        gp, du, dr = None, ptr['out[0]'], ptr['out[1]']
    pv = [v.data_ptr() for v in vecs] + [None] * (4 - nvec)
    workspace = _grad_workspace(what, workspace, batch_norm_train_workspace(n, c, h * w), g)
    _lib.check(_lib.load().scf_batch_norm_train_grad(
        ptr['g'], ptr['y'], ptr['u'], ptr['r'], saved.data_ptr(), None if r is None else saved_r.data_ptr(), pg[0],
        None if r is None else pg[1], gp, du, dr, *pv, int(bool(accumulate)), workspace.data_ptr(), workspace.numel(),
        n, c, h * w, _stream()), 'scf_batch_norm_train_grad')
    return (*maps, *vecs)


# ------------------------------------------------- gate arithmetic of the ConvGRU backward (gru_grad.hip)
def _gg_rows(what: str, shape, named) -> list:
    """(pointer, sample stride) of every (M, C, H, W) operand of a gate kernel; None stays (None, 0)."""
    out = []
    for name, t in named:
        out.extend((None, 0) if t is None else _s1_map(t, what, name, shape))
    return out


def _gg_shape(what: str, g: Tensor) -> Tuple[int, int]:
    if g.dim() != 4 or g.numel() == 0:
        raise _lib.ScflowHipError(f'{what}: g must be a non-empty (M, C, H, W) tensor, got {tuple(g.shape)}')
    return g.shape[0], g.shape[1] * g.shape[2] * g.shape[3]


def gru_gate_grad_q(g: Tensor, h: Tensor, z: Tensor, q: Tensor, u_q: Optional[Tensor] = None, u_z: Optional[Tensor] = None,
                    sum_q: Optional[Tensor] = None, sum_z: Optional[Tensor] = None, first: bool = True
                    ) -> Tuple[Tensor, Tensor]:
    """``u_q = g z (1 - q^2)``, ``u_z = g (q - h) z (1 - z)`` of one GRU pass (``scf_gru_gate_grad_q``; the order of
    operations is the header's).  Every operand (M, C, H, W), contiguous up to a channel slice.  ``sum_q`` / ``sum_z``:
    running sums, ``sum = u`` with ``first`` and ``sum + u`` otherwise."""
    what = 'gru_gate_grad_q'
    m, n = _gg_shape(what, g)
    shape = tuple(g.shape)
    if u_q is None:
        u_q = torch.empty(shape, dtype=torch.float32, device=g.device)
    if u_z is None:
        u_z = torch.empty(shape, dtype=torch.float32, device=g.device)
    args = _gg_rows(what, shape, (('g', g), ('h', h), ('z', z), ('q', q), ('u_q', u_q), ('u_z', u_z), ('sum_q', sum_q),
                                  ('sum_z', sum_z)))
    _lib.check(_lib.load().scf_gru_gate_grad_q(*args, int(bool(first)), m, n, _stream()), 'scf_gru_gate_grad_q')
    return u_q, u_z


def gru_gate_grad_r(g: Tensor, z: Tensor, g_rh: Tensor, h: Tensor, r: Tensor, u_r: Optional[Tensor] = None,
                    sum_r: Optional[Tensor] = None, first: bool = True) -> Tuple[Tensor, Tensor]:
    """``u_r = g_rh h r (1 - r)`` and ``g_h_direct = g (1 - z) + g_rh r``, the latter written IN PLACE over ``g_rh``
    (``scf_gru_gate_grad_r``) -> (u_r, g_rh).  Operands as in ``gru_gate_grad_q``."""
    what = 'gru_gate_grad_r'
    m, n = _gg_shape(what, g)
    shape = tuple(g.shape)
    if u_r is None:
        u_r = torch.empty(shape, dtype=torch.float32, device=g.device)
    args = _gg_rows(what, shape, (('g', g), ('z', z), ('g_rh', g_rh), ('h', h), ('r', r), ('u_r', u_r), ('sum_r', sum_r)))
    _lib.check(_lib.load().scf_gru_gate_grad_r(*args, int(bool(first)), m, n, _stream()), 'scf_gru_gate_grad_r')
    return u_r, g_rh


def gru_carry(src: Tensor, add: Optional[Tensor] = None, out: Optional[Tensor] = None, clear: bool = False) -> Tensor:
    """``out = src + add`` (``add`` None: a copy); ``clear``: ``src`` is then set to +0 (``scf_gru_carry``)."""
    what = 'gru_carry'
    m, n = _gg_shape(what, src)
    shape = tuple(src.shape)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=src.device)
    args = _gg_rows(what, shape, (('src', src), ('add', add), ('out', out)))
    _lib.check(_lib.load().scf_gru_carry(*args, int(bool(clear)), m, n, _stream()), 'scf_gru_carry')
    return out


def gru_gate_state(h: Tensor, gate: Tensor, q: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """``gate * h`` (``q`` None: the forward's ``r h``) or ``(1 - gate) h + gate q`` (its state update), as the backward
    recomputes them (``scf_gru_gate_state``)."""
    what = 'gru_gate_state'
    m, n = _gg_shape(what, h)
    shape = tuple(h.shape)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=h.device)
    args = _gg_rows(what, shape, (('h', h), ('gate', gate), ('q', q), ('out', out)))
    _lib.check(_lib.load().scf_gru_gate_state(*args, m, n, _stream()), 'scf_gru_gate_state')
    return out


# ----------------------------------------------------------------------------------------------------- optimizer step
ADAMW_CHUNK = 4096            # SCF_ADAMW_CHUNK of include/scflow_hip.h: elements per block of the multi-tensor kernels
ADAMW_NORM_THREADS = 256      # SCF_ADAMW_NORM_THREADS: the block size the norm's summation depth is counted from


def adamw_chunk_table(sizes: Sequence[int]) -> Tensor:
    """``scf_adamw_chunks`` (a host function): the chunk table of tensors with ``sizes`` elements as a CPU int64 tensor
    (nchunks, 2) with the bytes of ``scf_adamw_chunk``: word 0 = tensor index | length << 32, word 1 = offset
    (``adamw_chunk_rows`` decodes it).  Upload it once and hand it to ``grad_sqnorm`` / ``adamw_step``."""
    lib = _lib.load()
    sizes = [int(s) for s in sizes]
    if any(s < 0 for s in sizes):
        raise ValueError(f'adamw_chunk_table: negative size in {sizes}')
    arr = (C.c_int64 * max(len(sizes), 1))(*sizes)
    n = lib.scf_adamw_chunks(arr, len(sizes), None, 0)
    if n < 0:
        _lib.check(int(n), 'scf_adamw_chunks')
    table = torch.zeros((n, 2), dtype=torch.int64)
    if n:
        got = lib.scf_adamw_chunks(arr, len(sizes), C.cast(table.data_ptr(), C.POINTER(_lib.AdamwChunk)), n)
        if got != n:
            raise _lib.ScflowHipError(f'scf_adamw_chunks wrote {got} chunks, counted {n}')
    return table


def adamw_chunk_rows(table: Tensor) -> List[Tuple[int, int, int]]:
    """[(tensor index, offset, length)] of an ``adamw_chunk_table``."""
    return [(int(a) & 0xffffffff, int(off), int(a) >> 32) for a, off in table.cpu().tolist()]


class AdamwChunks:
    """the uploaded chunk table of a tensor list together with what the kernels cannot check on the device: how many
    tensors it indexes and how many chunks it has.  The wrappers below refuse pointer tables of another length."""

    def __init__(self, sizes: Sequence[int], device) -> None:
        self.sizes = [int(s) for s in sizes]
        host = adamw_chunk_table(self.sizes)
        self.nchunks, self.ntensors = int(host.shape[0]), len(self.sizes)
        self.table = host.to(device)


def _adamw_tables(chunks: AdamwChunks, **ptrs: Tensor) -> None:
    """the device tables of the optimizer kernels: int64, on the current device, contiguous, one pointer per tensor"""
    if not isinstance(chunks, AdamwChunks):
        raise _lib.ScflowHipError(f'chunks: expected an ops.AdamwChunks, got {type(chunks).__name__}')
    for name, t in (('chunks', chunks.table),) + tuple(ptrs.items()):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.int64 or not t.is_contiguous():
            raise _lib.ScflowHipError(f'{name}: expected a contiguous int64 tensor on the GPU')
        if t.device.index != _cur_dev():
            raise _lib.ScflowHipError(f'{name} lives on cuda:{t.device.index} but the current device is cuda:{_cur_dev()}')
    for name, t in ptrs.items():
        if t.numel() != chunks.ntensors:
            raise _lib.ScflowHipError(f'{name}: {t.numel()} pointers for {chunks.ntensors} tensors')


def grad_sqnorm(chunks: AdamwChunks, g_ptrs: Tensor, partial: Tensor, norm: Tensor) -> Tensor:
    """``scf_grad_sqnorm``: the L2 norm of the gradient list behind ``g_ptrs`` (device int64 table of device pointers, the
    tensors of ``chunks.sizes`` elements) into the 0-dim ``norm``, through ``partial`` (>= nchunks floats).  Two launches,
    no synchronisation."""
    _adamw_tables(chunks, g_ptrs=g_ptrs)
    _dev(partial, 'partial')
    _dev(norm, 'norm')
    if partial.numel() < chunks.nchunks or not partial.is_contiguous() or norm.numel() != 1:
        raise _lib.ScflowHipError(f'grad_sqnorm: partial needs {chunks.nchunks} contiguous floats, norm one')
    _lib.check(_lib.load().scf_grad_sqnorm(chunks.table.data_ptr(), chunks.nchunks, g_ptrs.data_ptr(), partial.data_ptr(),
                                           norm.data_ptr(), _stream()), 'scf_grad_sqnorm')
    return norm


def adamw_step(chunks: AdamwChunks, p_ptrs: Tensor, g_ptrs: Tensor, m_ptrs: Tensor, v_ptrs: Tensor, norm: Optional[Tensor],
               max_norm: float, lr: float, weight_decay: float, beta1: float, beta2: float, eps: float, step: int) -> None:
    """``scf_adamw_step``: clip by ``max_norm`` against the device scalar ``norm`` (None: no clipping) and apply step
    number ``step`` (1-based) of AdamW to the tensors behind the four pointer tables.  The bias corrections are computed
    here in float64.  One launch."""
    _adamw_tables(chunks, p_ptrs=p_ptrs, g_ptrs=g_ptrs, m_ptrs=m_ptrs, v_ptrs=v_ptrs)
    if norm is not None:
        _dev(norm, 'norm')
        if norm.numel() != 1:
            raise _lib.ScflowHipError('adamw_step: norm is one float')
    if step < 1:
        raise ValueError(f'adamw_step: step counts from 1, got {step}')
    bc1, bc2 = 1.0 - float(beta1) ** step, 1.0 - float(beta2) ** step
    _lib.check(_lib.load().scf_adamw_step(chunks.table.data_ptr(), chunks.nchunks, p_ptrs.data_ptr(), g_ptrs.data_ptr(),
                                          m_ptrs.data_ptr(), v_ptrs.data_ptr(), None if norm is None else norm.data_ptr(),
                                          float(max_norm) if norm is not None else 0.0, float(lr), float(weight_decay),
                                          float(beta1), float(beta2), float(eps), bc1, bc2, _stream()), 'scf_adamw_step')

