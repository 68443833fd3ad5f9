"""CPU: exact operands for the forward convolutions -- the route table of every kernel family and instantiation a single
``scf_conv2d`` launch can reach, operands from a small integer lattice on which every product and every partial sum of every
route is exactly representable in fp32, the certificate that proves it from the operands alone, the float64 reference, and
the planted defects the reference is shown to see.  tests/test_gpu_conv_exact.py feeds these operands to the HIP kernels and
asks for the BITS of the float64 result.

Why bits.  With x, w, bias, residual and the folded BatchNorm on a common dyadic grid 2**-q, a sum whose absolute terms add up
to less than 2**24 grid units has every partial sum, in every order, on that grid and below 2**24 units: an fp32 number.  No
operation rounds, so summation order, tile shape, channel chunking, K slicing and the Winograd transforms cannot change the
result, and a dropped tap, a wrong halo row, a mis-indexed chunk tail or a wrong transform coefficient is a non-zero
difference at the pixel where it happens.

Lattices (``LATTICE``): the direct families take plain integers.  The Winograd families need the transformed weights U on a
dyadic grid as well: F(2x2, 3x3) has halves on both sides of G g G^T (weights in 4 Z), F(2, 5) has the Lagrange normalisers
4, -6, -6, 24, 24 of the points 0, 1, -1, 2, -2 (weights in 24 Z), F(4, 5) the normalisers -1, -9/2, -9/2, 90, 90, 45/32, 45/32
of 0, +-1, +-2, +-1/2 (odd part 45; weights in 45 * 2 Z = 90 Z make the C packer's U integers).  The kernels' own input and
output transforms are dyadic (F(4, 5): 21/4, 17/4, 5/4, 5/2, 1/8).

The certificate (``certify``) takes no GPU result: the bound of the direct sum, sum |w||x|, and for the Winograd families
sum |A^T| (|U| . |B^T||x|) with U from the project's own C packer (checked against the exact rational G g first), the first
followed by the epilogue on absolute values, each in units of its grid, must stay below 2**24.  Transform coefficients are dyadic and every
magnitude is far below 2**53, so the float64 evaluation of these bounds is itself exact."""
import contextlib
import ctypes as C
import zlib
from collections import namedtuple
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from scflow_amd import _lib, ops
from test_winograd_pack import _unpack

NONE, RELU = ops.ACT_NONE, ops.ACT_RELU
LIMIT = float(2 ** 24)

# ---------------------------------------------------------------------------------------------------------- route table
# One row per kernel family and instantiation a single scf_conv2d launch reaches, derived from the dispatch functions
# (scf_conv_*_dispatch, conv2d_walk) at 256 CUs.  knobs: wino = ops.set_conv_winograd, f16 = conv precision 'f16x3' (lo = which
# operand carries a non-zero low half), tune = ops.tune settings, dma_packing = PackedConv.from_weight's, kslices = explicit
# K slices (raw partial sums, plain epilogue only), workspace = a registered K-slice workspace (the autoslice + kcombine
# route).  c0 = the segment boundary of the two-segment variant (0: the family takes one segment).  info = what
# scf_conv2d_query answers for the plain single-segment descriptor; inst = the template instantiation behind it.
Row = namedtuple('Row', 'id n cin cout k stride pad H W c0 knobs family info inst')
P0, P1, PH5, PV5 = (0, 0), (1, 1), (0, 2), (2, 0)
DIRECT = dict(wino=False)
REG = dict(wino=False, dma_packing=False)


def _f16(lo):
    return dict(f16=True, lo=lo)


INFO = None
F25, F45, F45H = dict(tune=dict(wino1d4=0)), dict(tune=dict(wino1d4=2)), dict(tune=dict(wino1d4=2, wino1d4_half=1))


ROUTES = [
    # ---- thin (conv_thin.hip: launch_thin<K, CO, UNROLL>; Cout <= 4, Cin >= 32, 1x1 / 3x3 'same', one segment)
    Row('thin-k1-co1', 2, 32, 1, (1, 1), 1, P0, 9, 7, 0, {}, 'thin', (0, 0, 0, -1), 'conv_thin_kernel<1, 1, 0>'),
    Row('thin-k1-co2', 1, 40, 2, (1, 1), 1, P0, 5, 11, 0, {}, 'thin', (0, 0, 0, -1), 'conv_thin_kernel<1, 2, 0>'),
    Row('thin-k1-co4', 2, 33, 3, (1, 1), 1, P0, 6, 6, 0, {}, 'thin', (0, 0, 0, -1), 'conv_thin_kernel<1, 4, 0>'),
    Row('thin-k3-co1-u0', 1, 32, 1, (3, 3), 1, P1, 5, 37, 0, {}, 'thin', (0, 0, 0, -1), 'conv_thin_kernel<3, 1, 0>'),
    Row('thin-k3-co2-u0', 1, 34, 2, (3, 3), 1, P1, 4, 33, 0, {}, 'thin', (0, 0, 0, -1), 'conv_thin_kernel<3, 2, 0>'),
    Row('thin-k3-co4-u0', 1, 36, 4, (3, 3), 1, P1, 3, 40, 0, {}, 'thin', (0, 0, 0, -1), 'conv_thin_kernel<3, 4, 0>'),
    Row('thin-k3-co1-u4', 2, 32, 1, (3, 3), 1, P1, 8, 8, 0, {}, 'thin', (0, 0, 0, -1), 'conv_thin_kernel<3, 1, 4>'),
    Row('thin-k3-co2-u4', 1, 40, 2, (3, 3), 1, P1, 7, 9, 0, {}, 'thin', (0, 0, 0, -1), 'conv_thin_kernel<3, 2, 4>'),
    Row('thin-k3-co4-u4', 3, 35, 3, (3, 3), 1, P1, 8, 8, 0, {}, 'thin', (0, 0, 0, -1), 'conv_thin_kernel<3, 4, 4>'),
    Row('thin-k3-co1-u2', 65, 32, 1, (3, 3), 1, P1, 8, 8, 0, {}, 'thin', (0, 0, 0, -1), 'conv_thin_kernel<3, 1, 2>'),
    Row('thin-k3-co2-u2', 52, 33, 2, (3, 3), 1, P1, 9, 6, 0, {}, 'thin', (0, 0, 0, -1), 'conv_thin_kernel<3, 2, 2>'),
    Row('thin-k3-co4-u2', 33, 32, 4, (3, 3), 1, P1, 16, 5, 0, {}, 'thin', (0, 0, 0, -1), 'conv_thin_kernel<3, 4, 2>'),
    # ---- taps (conv_taps.hip: Cin <= 4, contraction over taps; WM = 64 channels per block when every CU still gets two
    #      blocks; more tiles than 3 x CUs blocks: the persistent kernel walks tiles slot, slot + nslots, ..)
    Row('taps-wm1', 3, 4, 40, (3, 3), 1, P1, 12, 20, 0, {}, 'taps', (1, 1, 18, -20), 'conv_taps_kernel<1>'),
    Row('taps-wm1-5x5s2', 2, 2, 96, (5, 5), 2, (2, 2), 30, 22, 0, {}, 'taps', (1, 1, 12, -28), 'conv_taps_kernel<1>, stride 2, 3 channel blocks'),
    Row('taps-wm2', 66, 1, 64, (3, 3), 1, P1, 31, 30, 0, {}, 'taps', (2, 1, 528, -16), 'conv_taps_kernel<2>'),
    Row('taps-walk-even', 192, 1, 32, (3, 3), 1, P1, 32, 32, 0, {}, 'taps', (1, 1, 1536, -8), 'conv_taps_persist_kernel<1>: 1536 tiles on 768 slots'),
    Row('taps-walk-ragged', 125, 3, 64, (3, 3), 1, P1, 32, 32, 0, {}, 'taps', (2, 1, 1000, -32), 'conv_taps_persist_kernel<2>: 1000 tiles on 768 slots'),
    # ---- direct-dma (conv_dma.hip: conv_dma_kernel<WM, WN, 2, KSP, PX4, NG>).  Pixel-split tiles need >= 512 blocks
    Row('dma-22-x4', 128, 12, 64, (3, 3), 1, P1, 32, 32, 8, DIRECT, 'direct-dma', (2, 2, 512, -144), '<2, 2, 2, false, true, 1>'),
    Row('dma-22-dword', 128, 12, 64, (3, 3), 1, P1, 31, 30, 8, DIRECT, 'direct-dma', (2, 2, 512, -144), '<2, 2, 2, false, false, 1>'),
    Row('dma-31-x4', 128, 20, 96, (3, 3), 1, P1, 32, 16, 8, DIRECT, 'direct-dma', (3, 1, 512, -108), '<3, 1, 2, false, true, 1>, 16-column fragments'),
    Row('dma-31-dword', 128, 20, 96, (3, 3), 1, P1, 31, 15, 16, DIRECT, 'direct-dma', (3, 1, 512, -108), '<3, 1, 2, false, false, 1>'),
    Row('dma-21-x4', 64, 24, 40, (3, 3), 1, P1, 24, 40, 16, DIRECT, 'direct-dma', (2, 1, 640, -72), '<2, 1, 2, false, true, 1>, 8-column fragments'),
    Row('dma-21-dword', 64, 24, 40, (3, 3), 1, P1, 23, 38, 8, DIRECT, 'direct-dma', (2, 1, 640, -72), '<2, 1, 2, false, false, 1>, 8-column fragments'),
    Row('dma-11-x4', 128, 16, 64, (3, 3), 1, P1, 16, 16, 8, DIRECT, 'direct-dma', (1, 1, 512, -36), '<1, 1, 2, false, true, 1>'),
    Row('dma-11-dword', 128, 20, 64, (3, 3), 1, P1, 15, 15, 8, DIRECT, 'direct-dma', (1, 1, 512, -36), '<1, 1, 2, false, false, 1>'),
    Row('dma-g2-1x5', 128, 24, 64, (1, 5), 1, PH5, 16, 16, 16, DIRECT, 'direct-dma', (1, 1, 512, -40), '<1, 1, 2, false, true, 1>, G = 2 windows'),
    Row('dma-g2-5x1', 128, 24, 64, (5, 1), 1, PV5, 15, 14, 16, DIRECT, 'direct-dma', (1, 1, 512, -40), '<1, 1, 2, false, false, 1>, G = 2 windows'),
    Row('dma-s2-x4', 128, 24, 64, (3, 3), 2, P1, 32, 32, 8, DIRECT, 'direct-dma', (1, 1, 512, -36), '<1, 1, 2, false, true, 1>, stride 2: parity-split rows'),
    Row('dma-s2-dword', 128, 24, 64, (3, 3), 2, P1, 30, 22, 16, DIRECT, 'direct-dma', (1, 1, 512, -36), '<1, 1, 2, false, false, 1>, stride 2'),
    Row('dma-1x1-x4', 32, 68, 64, (1, 1), 1, P0, 32, 32, 32, DIRECT, 'direct-dma', (1, 1, 512, -16), '<1, 1, 2, false, true, 1>, dense 1x1 on a full grid'),
    Row('dma-dilated-pixel', 36, 72, 96, (1, 1), 2, P0, 33, 41, 32, DIRECT, 'direct-dma', (1, 1, 540, -16), '<1, 1, 2, false, false, 1>, 1x1 / s2 gather'),
    Row('dma-dilated-ksplit', 8, 72, 96, (1, 1), 2, P0, 33, 41, 32, DIRECT, 'direct-dma', (1, 1, 408, -4), '<1, 1, 2, true, false, 1>, 1x1 / s2 gather'),
    Row('dma-ksp-ng1-x4', 6, 44, 40, (3, 3), 1, P1, 25, 32, 16, DIRECT, 'direct-dma', (1, 1, 300, -18), '<1, 1, 2, true, true, 1>, 16-channel chunks'),
    Row('dma-ksp-ng1-dword', 12, 44, 40, (3, 3), 1, P1, 13, 30, 16, DIRECT, 'direct-dma', (1, 1, 312, -18), '<1, 1, 2, true, false, 1>, 16-channel chunks'),
    Row('dma-ksp-tiny-x4', 1, 128, 64, (3, 3), 1, P1, 8, 8, 32, DIRECT, 'direct-dma', (1, 1, 4, -36), '<1, 1, 2, true, true, 1>, 32-channel chunks (tiny grid)'),
    Row('dma-ksp-tiny-dword', 3, 40, 33, (3, 3), 1, P1, 9, 7, 32, DIRECT, 'direct-dma', (1, 1, 18, -36), '<1, 1, 2, true, false, 1>, 32-channel chunks (tiny grid)'),
    Row('dma-ksp-tiny-s2', 1, 72, 64, (3, 3), 2, P1, 15, 13, 32, DIRECT, 'direct-dma', (1, 1, 4, -36), '<1, 1, 2, true, false, 1>, stride 2'),
    Row('dma-ksp-ng2-x4', 1, 132, 64, (1, 1), 1, P0, 8, 8, 32, DIRECT, 'direct-dma', (1, 2, 4, -4), '<1, 1, 2, true, true, 2>'),
    Row('dma-ksp-ng2-dword', 1, 132, 64, (1, 1), 1, P0, 7, 9, 32, DIRECT, 'direct-dma', (1, 2, 8, -4), '<1, 1, 2, true, false, 2>'),
    Row('dma-ksp-ng2-1x5', 1, 136, 64, (1, 5), 1, PH5, 8, 8, 64, DIRECT, 'direct-dma', (1, 2, 4, -20), '<1, 1, 2, true, true, 2>'),
    Row('dma-kslices-4', 1, 128, 64, (3, 3), 2, P1, 16, 16, 32, dict(wino=False, kslices=4), 'direct-dma', (1, 1, 16, -36), 'k_slices = 4'),
    Row('dma-kslices-2', 5, 96, 64, (3, 3), 2, P1, 12, 12, 32, dict(wino=False, kslices=2), 'direct-dma', (1, 1, 40, -36), 'k_slices = 2'),
    Row('dma-kslices-2-1x1', 2, 100, 40, (1, 1), 1, P0, 9, 7, 32, dict(wino=False, kslices=2), 'direct-dma', (1, 1, 24, -4), 'k_slices = 2, dense 1x1'),
    Row('dma-autoslice', 1, 132, 64, (1, 1), 1, P0, 8, 8, 32, dict(wino=False, workspace=True), 'direct-dma', (1, 2, 4, -4), 'autoslice + kcombine'),
    # ---- direct-mfma (conv_mfma.hip, dma_packing=False: conv_mfma_kernel<WM, WN, KC>): the six SCF_CASE tiles, the three KC
    Row('mfma-11-kc8', 40, 20, 33, (3, 3), 1, P1, 15, 13, 8, REG, 'direct-mfma', (1, 1, 160, 36), '<1, 1, 8>'),
    Row('mfma-11-kc2', 40, 3, 64, (7, 7), 2, (3, 3), 32, 32, 0, REG, 'direct-mfma', (1, 1, 160, 49), '<1, 1, 2>'),
    Row('mfma-11-kc32', 64, 68, 64, (1, 1), 1, P0, 16, 16, 32, REG, 'direct-mfma', (1, 1, 256, 16), '<1, 1, 32>'),
    Row('mfma-12', 128, 9, 32, (1, 1), 1, P0, 64, 64, 0, REG, 'direct-mfma', (1, 2, 2048, 8), '<1, 2, 8>'),
    Row('mfma-21', 64, 12, 64, (3, 3), 1, P1, 32, 32, 8, REG, 'direct-mfma', (2, 1, 512, 72), '<2, 1, 8>'),
    Row('mfma-22', 128, 9, 64, (1, 1), 1, P0, 64, 64, 0, REG, 'direct-mfma', (2, 2, 2048, 16), '<2, 2, 8>'),
    Row('mfma-31', 128, 12, 96, (3, 3), 1, P1, 32, 16, 8, REG, 'direct-mfma', (3, 1, 512, 108), '<3, 1, 8>'),
    Row('mfma-41', 256, 9, 130, (1, 1), 1, P0, 8, 8, 0, REG, 'direct-mfma', (4, 1, 512, 16), '<4, 1, 8>, 5 fragments'),
    # ---- direct-mfma-ksplit (conv_mfma_ksplit_kernel<KC>: fewer than 128 blocks)
    Row('ksplit-kc32', 1, 68, 64, (1, 1), 1, P0, 8, 8, 32, REG, 'direct-mfma-ksplit', (1, 1, 4, 4), '<32>'),
    Row('ksplit-kc8', 1, 20, 40, (3, 3), 1, P1, 9, 7, 8, REG, 'direct-mfma-ksplit', (1, 1, 6, 9), '<8>'),
    Row('ksplit-kc2', 2, 2, 96, (7, 7), 1, (3, 3), 8, 8, 0, REG, 'direct-mfma-ksplit', (1, 1, 12, 12), '<2>'),
    Row('ksplit-kc2-5x5s2', 1, 6, 40, (5, 5), 2, (2, 2), 13, 11, 2, REG, 'direct-mfma-ksplit', (1, 1, 4, 6), '<2>, stride 2'),
    # ---- winograd F(2x2, 3x3) (conv_wino.hip): the pair kernel conv_wino_kernel<1, 2, PX4> (odd fragment counts, or forced)
    Row('wino-pair-dword', 128, 16, 32, (3, 3), 1, P1, 7, 10, 8, {}, 'winograd', (16, 2, 128, -49152), 'conv_wino_kernel<1, 2, false>'),
    Row('wino-pair-x4', 128, 18, 24, (3, 3), 1, P1, 9, 12, 8, {}, 'winograd', (16, 2, 128, -61440), 'conv_wino_kernel<1, 2, true>'),
    Row('wino-pair-forced', 64, 16, 64, (3, 3), 1, P1, 16, 16, 8, dict(tune=dict(wino_variant=1)), 'winograd', (16, 2, 128, -61440), 'conv_wino_kernel<1, 2, true>, two fragments'),
    # ---- winograd-q: the quarter-domain kernel conv_wino_q_kernel<1, PX4> (even fragment counts)
    Row('wino-q-x4', 64, 16, 64, (3, 3), 1, P1, 16, 16, 8, {}, 'winograd-q', (16, 2, 128, -61440), 'conv_wino_q_kernel<1, true>'),
    Row('wino-q-dword', 64, 18, 40, (3, 3), 1, P1, 15, 14, 8, {}, 'winograd-q', (16, 2, 128, -61440), 'conv_wino_q_kernel<1, false>'),
    # ---- winograd F(2, 5) (conv_wino1d.hip: conv_wino1d_kernel<VERT, PX4>), ops.tune('wino1d4', 0)
    Row('f25-h-dword', 32, 40, 64, (1, 5), 1, PH5, 20, 30, 16, F25, 'winograd F(2,5)', (6, 4, 160, -55296), 'conv_wino1d_kernel<false, false>'),
    Row('f25-h-x4', 32, 40, 64, (1, 5), 1, PH5, 19, 28, 16, F25, 'winograd F(2,5)', (6, 4, 160, -61440), 'conv_wino1d_kernel<false, true>'),
    Row('f25-v-32', 24, 48, 64, (5, 1), 1, PV5, 21, 28, 16, F25, 'winograd F(2,5)', (6, 4, 144, -73728), 'conv_wino1d_kernel<true, true>, 32 columns x 1 tile row'),
    Row('f25-v-16', 48, 20, 64, (5, 1), 1, PV5, 21, 12, 8, F25, 'winograd F(2,5)', (6, 4, 144, -73728), 'conv_wino1d_kernel<true, true>, 16 columns x 2 tile rows'),
    # ---- winograd F(4, 5) (conv_wino1d4.hip: conv_wino1d4_kernel<VERT, PX4, NPI>), ops.tune('wino1d4', 2) below its grid threshold
    Row('f45-h-dword', 32, 40, 64, (1, 5), 1, PH5, 20, 30, 16, F45, 'winograd F(4,5)', (8, 4, 96, -56320), 'conv_wino1d4_kernel<false, false, 5>'),
    Row('f45-h-x4', 32, 40, 64, (1, 5), 1, PH5, 19, 28, 16, F45, 'winograd F(4,5)', (8, 4, 96, -65536), 'conv_wino1d4_kernel<false, true, 2>'),
    Row('f45-v-npi2', 24, 44, 64, (5, 1), 1, PV5, 21, 28, 16, F45, 'winograd F(4,5)', (8, 4, 72, -65536), 'conv_wino1d4_kernel<true, true, 2>'),
    Row('f45-v-npi3', 24, 20, 64, (5, 1), 1, PV5, 21, 12, 8, F45, 'winograd F(4,5)', (8, 4, 48, -77824), 'conv_wino1d4_kernel<true, true, 3>'),
    Row('f45-default', 40, 20, 128, (1, 5), 1, PH5, 13, 20, 8, {}, 'winograd F(4,5)', (8, 4, 160, -65536), 'conv_wino1d4_kernel<false, true, 2>, the dispatch\'s own choice'),
    Row('f45-half-h-dword', 16, 40, 64, (1, 5), 1, PH5, 20, 30, 16, F45H, 'winograd F(4,5)', (8, 4, 48, -65536), 'conv_wino1d4h_kernel<false, false, 5>'),
    Row('f45-half-h-x4', 16, 36, 64, (1, 5), 1, PH5, 19, 28, 16, F45H, 'winograd F(4,5)', (8, 4, 48, -65536), 'conv_wino1d4h_kernel<false, true, 2>'),
    Row('f45-half-v-npi2', 12, 44, 64, (5, 1), 1, PV5, 21, 28, 16, F45H, 'winograd F(4,5)', (8, 4, 36, -65536), 'conv_wino1d4h_kernel<true, true, 2>'),
    Row('f45-half-v-npi3', 12, 36, 64, (5, 1), 1, PV5, 21, 12, 16, F45H, 'winograd F(4,5)', (8, 4, 24, -77824), 'conv_wino1d4h_kernel<true, true, 3>'),
    # ---- f16x3 (conv_f16x3.hip: conv_f16x3_kernel<WM, WN, NK>), conv precision 'f16x3'; lo = the operand with a low half
    Row('f16-21-nk1', 128, 16, 64, (3, 3), 1, P1, 32, 16, 0, _f16('x'), 'f16x3', (2, 1, 512, -54), '<2, 1, 1>'),
    Row('f16-21-nk2', 128, 40, 64, (1, 5), 1, PH5, 31, 14, 32, _f16('w'), 'f16x3', (2, 1, 512, -60), '<2, 1, 2>'),
    Row('f16-12', 128, 20, 30, (5, 1), 1, PV5, 63, 15, 0, _f16('x'), 'f16x3', (1, 2, 512, -30), '<1, 2, 1>'),
    Row('f16-11-nk1', 3, 20, 40, (3, 3), 1, P1, 12, 20, 0, _f16('w'), 'f16x3', (1, 1, 18, -27), '<1, 1, 1>'),
    Row('f16-11-nk2', 2, 36, 33, (3, 3), 1, P1, 13, 21, 32, _f16('x'), 'f16x3', (1, 1, 16, -54), '<1, 1, 2>'),
    Row('f16-11-nk2-wlo', 2, 36, 33, (3, 3), 1, P1, 13, 21, 32, _f16('w'), 'f16x3', (1, 1, 16, -54), '<1, 1, 2>'),
]
BY_ID = {}

# what a family's dispatch refuses (the launch then goes on down conv2d_walk to another family, which must be exact too)
REFUSES = {'thin': {'res', 'bn', 'split', 'two'}, 'taps': {'two'}, 'winograd': {'split'}, 'winograd-q': {'split'}}
# rows for which no lattice certifies: id -> reason (they get the guard-band, NaN and determinism checks only)
UNCERTIFIED = {}

LATTICE = {'winograd': 4, 'winograd-q': 4, 'winograd F(2,5)': 24, 'winograd F(4,5)': 90}
# (largest integer multiple m, density) in the order they are tried: the first rung that certifies is the row's
RUNGS = ((3, 1.0), (2, 0.6), (1, 0.5), (1, 0.3), (1, 0.15), (1, 0.08))
BN_VARS = (0.25, 1.0, 4.0, 16.0)


def out_hw(row):
    return ((row.H + 2 * row.pad[0] - row.k[0]) // row.stride + 1, (row.W + 2 * row.pad[1] - row.k[1]) // row.stride + 1)


def variants(row):
    """name -> epilogue spec of the bit-equality runs of a row (section b)."""
    plain = dict(bias=False, res=False, bn=False, act=NONE, act2=NONE, split=0, two=False)
    if row.knobs.get('kslices', 1) > 1:
        return {'plain': plain}
    v = {'plain': plain, 'bias': dict(plain, bias=True), 'bias_res_relu': dict(plain, bias=True, res=True, act=RELU),
         'bn': dict(plain, bias=True, bn=True)}
    splits = ([('on', 32)] if row.cout > 32 else []) + ([('off', min(row.cout - 1, 13))] if row.cout > 1 else [])
    for where, s in splits:
        v[f'split_{where}_relu'] = dict(plain, bias=True, act=RELU, act2=NONE, split=s)
        v[f'split_{where}_none'] = dict(plain, bias=True, act=NONE, act2=RELU, split=s)
    if row.c0:
        v['two'] = dict(plain, bias=True, two=True)
    return v


def refused(row, spec):
    """does the row's family hand this epilogue on to another one?"""
    no = REFUSES.get(row.family, set())
    return (spec['res'] and 'res' in no) or (spec['bn'] and 'bn' in no) or (spec['split'] > 0 and 'split' in no) or \
        (spec['two'] and 'two' in no)


@contextlib.contextmanager
def route_knobs(row):
    """the process-wide settings of a row, restored afterwards"""
    k = row.knobs
    prev_w = ops.set_conv_winograd(bool(k.get('wino', True)))
    prev_p = ops.set_conv_precision('f16x3' if k.get('f16') else 'f32')
    tuned = []
    try:
        for key, val in k.get('tune', {}).items():
            tuned.append((key, ops.tune(key, val)))
        yield
    finally:
        for key, prev in reversed(tuned):
            ops.tune(key, prev)
        ops.set_conv_precision(prev_p)
        ops.set_conv_winograd(prev_w)


# ------------------------------------------------------------------------------------------------------------ operands
def grid_exp(t, limit=40):
    """smallest q >= 0 with t * 2**q integral everywhere"""
    a = np.asarray(t.detach().cpu().double().numpy() if isinstance(t, torch.Tensor) else t, dtype=np.float64).ravel()
    for q in range(limit + 1):
        s = a * 2.0 ** q
        if np.all(s == np.rint(s)):
            return q
    raise AssertionError('not on a dyadic grid')


def _kept_channels(row):
    """first and last channel of every chunk of 4 (hence of 8, 16, 32), the tail chunk, both sides of the segment boundary"""
    keep = {c for c in range(row.cin) if c % 4 in (0, 3)} | set(range((row.cin - 1) // 4 * 4, row.cin))
    if row.c0:
        keep |= {row.c0 - 1, row.c0}
    return sorted(keep)


def _draw(rng, shape, m, density):
    v = rng.integers(1, m + 1, size=shape) * rng.choice([-1, 1], size=shape)
    return v * (rng.random(shape) < density)


def _fill(rng, a, m):
    """the zeros of ``a`` (a view) replaced by non-zero lattice points"""
    z = a == 0
    a[z] = (rng.integers(1, m + 1, size=a.shape) * rng.choice([-1, 1], size=a.shape))[z]


def _operands(row, seed, m, density):
    rng = np.random.default_rng(zlib.crc32(row.id.encode()) + 7919 * seed)
    n, cin, cout, (kh, kw), H, W = row.n, row.cin, row.cout, row.k, row.H, row.W
    ho, wo = out_hw(row)
    x = _draw(rng, (n, cin, H, W), m, density)
    w = _draw(rng, (cout, cin, kh, kw), m, density)
    keep = _kept_channels(row)
    ring = sorted({0, cin - 1} | ({row.c0 - 1, row.c0} if row.c0 else set()))
    for c in keep:                                        # corners; one non-zero tap per (cout, kept channel)
        for i in (0, H - 1):
            for j in (0, W - 1):
                _fill(rng, x[:, c, i, j], m)
        flat = w[:, c].reshape(cout, kh * kw)
        dead = np.flatnonzero(np.all(flat == 0, axis=1))
        taps = rng.integers(0, kh * kw, size=dead.size)
        flat[dead, taps] = rng.integers(1, m + 1, size=dead.size) * rng.choice([-1, 1], size=dead.size)
        w[:, c] = flat.reshape(cout, kh, kw)
    for c in ring:                                        # all four borders
        _fill(rng, x[:, c, 0, :], m), _fill(rng, x[:, c, H - 1, :], m), _fill(rng, x[:, c, :, 0], m), _fill(rng, x[:, c, :, W - 1], m)
    lw = LATTICE.get(row.family, 1)
    lx = 1.0 if row.family in LATTICE else 0.5            # a power of two per tensor: the direct rows carry a fraction bit
    case = dict(m=m, density=density, lw=lw, lx=lx,
                x=torch.from_numpy(x * lx).float(), w=torch.from_numpy(w * lw).float(),
                b=torch.from_numpy(rng.integers(-m, m + 1, size=(cout,))).float(),
                res=torch.from_numpy(rng.integers(-m, m + 1, size=(n, cout, ho, wo))).float(),
                bn=(torch.from_numpy(rng.integers(1, 3, size=(cout,)) * rng.choice([-1, 1], size=(cout,))).float(),      # gamma
                    torch.from_numpy(rng.integers(-m, m + 1, size=(cout,))).float(),                                    # beta
                    torch.from_numpy(rng.integers(-1, 2, size=(cout,))).float(),                                        # mean
                    torch.from_numpy(rng.choice(BN_VARS, size=(cout,))).float()))                                       # var
    lo = row.knobs.get('lo')
    if lo:          # split-fp16: a non-zero LOW half on one operand (k * 2**-13 beside a non-zero integer), none on the other
        t = case['x' if lo == 'x' else 'w']
        tail = torch.from_numpy(rng.integers(-7, 8, size=tuple(t.shape))).float() * 2.0 ** -13
        t += tail * (t != 0)
    return case


_CASES = {}


def lattice_case(row, seed=0):
    """x, w, bias, residual and BN parameters of a row on its lattice: the first rung of RUNGS that ``certify`` accepts (the
    magnitude, then the density shrinks -- never the claim).  Cached: the tests share one case per (row, seed) and leave it
    unchanged."""
    key = (row.id, seed)
    if key not in _CASES:
        case = None
        for m, density in RUNGS:
            case = _operands(row, seed, m, density)
            case['certificate'] = certify(row, case)
            if case['certificate']['ok']:
                break
        _CASES[key] = case
    return _CASES[key]


# ----------------------------------------------------------------------------------------------------------- reference
def bn_affine(case):
    gamma, beta, mean, var = (t.double() for t in case['bn'])
    scale = gamma / torch.sqrt(var)                       # eps = 0: var in {1/4, 1, 4, 16} -> gamma * {2, 1, 1/2, 1/4}, exact
    return scale, beta - mean * scale


def conv64(row, x, w, pads=None):
    """the float64 convolution of a row's geometry; pads = (left, right, top, bottom) overrides the symmetric padding"""
    ph, pw = row.pad
    l, r, t, b = pads if pads is not None else (pw, pw, ph, ph)
    return F.conv2d(F.pad(x.double(), (l, r, t, b)), w.double(), None, stride=row.stride)


def epilogue64(case, acc, spec, samples=slice(None), b=None, res=None, relu_first=False):
    v = acc
    if spec['bias']:
        v = v + (case['b'] if b is None else b).double().view(1, -1, 1, 1)
    if spec['bn']:
        scale, shift = bn_affine(case)
        v = v * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    co = torch.arange(v.shape[1])
    act = torch.full((v.shape[1],), spec['act'])
    if spec['split'] > 0:
        act = torch.where(co < spec['split'], torch.tensor(spec['act']), torch.tensor(spec['act2']))
    relu = (act == RELU).view(1, -1, 1, 1)
    if relu_first:
        v = torch.where(relu, torch.relu(v), v)
    if spec['res']:
        v = v + (case['res'] if res is None else res)[samples].double()
    if not relu_first:
        v = torch.where(relu, torch.relu(v), v)
    return v


def reference(row, case, spec):
    """float64 F.conv2d on the row's operands (exact below 2**53), then the epilogue in float64"""
    if 'conv64' not in case:
        case['conv64'] = conv64(row, case['x'], case['w'])
    return epilogue64(case, case['conv64'], spec)


def same_bits(a, b):
    """bit equality of two fp32 tensors (NaNs compare by payload; -0.0 differs from 0.0)"""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))


# --------------------------------------------------------------------------------------------------------- certificate
def _frac_matrix(rows):
    return [[Fraction(v) for v in r] for r in rows]


def _lagrange_g(points, taps, flip_first=False):
    """G of the Toom-Cook form the C packers state: row i = (1, a_i, ..) / prod_{k != i} (a_i - a_k), then the row of infinity"""
    g = []
    for i, a in enumerate(points):
        nrm = Fraction(1)
        for k, b in enumerate(points):
            if k != i:
                nrm *= a - b
        if flip_first and i == 0:
            nrm = -nrm
        g.append([a ** k / nrm for k in range(taps)])
    g.append([Fraction(int(k == taps - 1)) for k in range(taps)])
    return g


H_ = Fraction(1, 2)
WINO = {
    # transforms as tests/test_winograd_pack.py states them for the kernels; kc = channels per packed chunk
    '2d': dict(G=_frac_matrix([[1, 0, 0], [H_, H_, H_], [H_, -H_, H_], [0, 0, 1]]),
               BT=np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=np.float64),
               AT=np.array([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=np.float64), kc=4, pack=ops.pack_conv_weight_wino),
    'f25': dict(G=_lagrange_g([Fraction(p) for p in (0, 1, -1, 2, -2)], 5),
                BT=np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0],
                             [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]], dtype=np.float64),
                AT=np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 1]], dtype=np.float64), kc=8, pack=ops.pack_conv_weight_wino1d),
    'f45': dict(G=_lagrange_g([Fraction(p) for p in (0, 1, -1, 2, -2)] + [H_, -H_], 5, flip_first=True),
                BT=np.array([[1, 0, -5.25, 0, 5.25, 0, -1, 0], [0, 1, 1, -4.25, -4.25, 1, 1, 0], [0, -1, 1, 4.25, -4.25, -1, 1, 0],
                             [0, 0.5, 0.25, -2.5, -1.25, 2, 1, 0], [0, -0.5, 0.25, 2.5, -1.25, -2, 1, 0],
                             [0, 2, 4, -2.5, -5, 0.5, 1, 0], [0, -2, 4, 2.5, -5, -0.5, 1, 0], [0, -1, 0, 5.25, 0, -5.25, 0, 1]],
                            dtype=np.float64),
                AT=np.array([[1, 1, 1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0.5, -0.5, 0], [0, 1, 1, 4, 4, 0.25, 0.25, 0],
                             [0, 1, -1, 8, -8, 0.125, -0.125, 1]], dtype=np.float64), kc=4, pack=ops.pack_conv_weight_wino1d4),
}
WINO_OF = {'winograd': '2d', 'winograd-q': '2d', 'winograd F(2,5)': 'f25', 'winograd F(4,5)': 'f45'}
WINDOW = {'winograd': 4, 'winograd-q': 4, 'winograd F(2,5)': 6, 'winograd F(4,5)': 8}


def packed_u(kind, w):
    """U[pos..., cout, cin] (float64) as the project's C packer returns it for these weights, in transform order"""
    t = WINO[kind]
    cout, cin = w.shape[:2]
    npos = len(t['G']) ** (2 if kind == '2d' else 1)
    u, full = _unpack(t['pack'](w).numpy().astype(np.float64), npos, cout, cin, t['kc'])
    assert np.all(full[:, cout:, :] == 0) and np.all(full[:, :, cin:] == 0)
    if kind == '2d':                                      # storage rows of the transform domain: 0, 1, 3, 2
        out = np.zeros((4, 4, cout, cin))
        for ip, i in enumerate((0, 1, 3, 2)):
            out[i] = u[4 * ip:4 * ip + 4]
        return out
    return u


def exact_u(kind, w):
    """G g (G g G^T) in exact integer arithmetic: (D U, D) with D the common denominator of G's entries"""
    g = WINO[kind]['G']
    den = 1
    for r in g:
        for v in r:
            den = den * v.denominator // np.gcd(den, v.denominator)
    gi = np.array([[int(v * den) for v in r] for r in g], dtype=np.int64)
    wi = w.double().numpy()
    assert np.all(wi == np.rint(wi))
    wi = wi.astype(np.int64)
    if kind == '2d':
        return np.einsum('ia,ocab,jb->ijoc', gi, wi, gi), den * den
    return np.einsum('ik,ock->ioc', gi, wi.reshape(w.shape[0], w.shape[1], 5)), den


def _windows(a, axis, win, step, lead, count):
    """(.., count, win) windows of ``a`` along ``axis`` starting at -lead, zero padded"""
    size = a.shape[axis]
    total = (count - 1) * step + win
    pad = [0, 0] * a.dim()
    pad[2 * (a.dim() - 1 - axis)] = lead
    pad[2 * (a.dim() - 1 - axis) + 1] = max(0, total - lead - size)
    return F.pad(a, pad).unfold(axis, win, step).narrow(axis, 0, count)


def winograd_bound(row, case):
    """max over the outputs of sum |A^T| (|U| . |B^T||x|), its grid exponent, and whether the packed U is the exact G g"""
    kind = WINO_OF[row.family]
    t = WINO[kind]
    u = packed_u(kind, case['w'])
    du, den = exact_u(kind, case['w'])
    exact = bool(np.all(u * den == du))
    if not exact:
        return float('inf'), 0, False
    ua = torch.from_numpy(np.abs(u))
    bt, at = torch.from_numpy(np.abs(t['BT'])), torch.from_numpy(np.abs(t['AT']))
    win, step = bt.shape[0], at.shape[0]
    xa = case['x'].double().abs()
    qx, qu, qb, qa = grid_exp(case['x']), grid_exp(u), grid_exp(t['BT']), grid_exp(t['AT'])
    worst = 0.0
    if kind == '2d':
        ty, tx = (row.H + 1) // 2, (row.W + 1) // 2
        for s in range(0, row.n, 8):                      # in slabs of samples: the window tensor is 4x the input
            d = _windows(_windows(xa[s:s + 8], 2, win, step, 1, ty), 3, win, step, 1, tx)          # n c ty tx a b
            v = torch.einsum('ia,jb,ncyxab->ncyxij', bt, bt, d)
            mm = torch.einsum('ijoc,ncyxij->noyxij', ua, v)
            worst = max(worst, float(torch.einsum('ai,bj,noyxij->noyxab', at, at, mm).max()))
        return worst, qx + qu + 2 * qb + 2 * qa, exact
    vert = row.k == (5, 1)
    if vert:
        xa = xa.transpose(2, 3)
    tiles = (xa.shape[3] + step - 1) // step
    for s in range(0, row.n, 8):
        d = _windows(xa[s:s + 8], 3, win, step, 2, tiles)                                        # n c h t w
        v = torch.einsum('iw,nchtw->nchti', bt, d)
        mm = torch.einsum('ioc,nchti->nohti', ua, v)
        worst = max(worst, float(torch.einsum('ai,nohti->nohta', at, mm).max()))
    return worst, qx + qu + qb + qa, exact


def f16_split_ok(t):
    """conv_f16x3.hip: x = hi + lo' * 2**-11 with hi = fp16(x), lo' = fp16((x - hi) * 2**11), exactly, inside fp16's normal
    range (|hi| <= 65504; lo' = 0 or |lo'| >= 2**-14).  -> (the split is exact, some low half is non-zero)"""
    hi = t.half().float()
    lo = ((t - hi) * 2048.0).half().float()
    ok = bool(torch.equal(hi + lo / 2048.0, t)) and bool(torch.isfinite(hi).all()) and \
        bool(((lo == 0) | (lo.abs() >= 2.0 ** -14)).all())
    return ok, bool((lo != 0).any())


def certify(row, case):
    """the proof, from the operands alone, that every route gives the float64 result's bits; -> dict(ok, units, q, ...).
    Direct sum: every output's sum |w||x| + |b|, times the largest |BN scale| plus the largest |shift|, plus |res|, in units of
    the common grid 2**-q, is below 2**24.  A Winograd row also carries the bound of its transform-domain sum plus |b| and
    |res| (the residual counted four times: the F(4, 5) kernel seeds its accumulators with it) on the transform's own grid;
    behind the output transform stands the convolution's value and the direct bound covers the epilogue.  Its packed U must
    be the exact G g.  A split-fp16 row's operands must split exactly, with a non-zero low half on one operand only (the kernel
    drops lo * lo)."""
    scale, shift = bn_affine(case)
    q_epi = max(grid_exp(case['b']), grid_exp(case['res']), grid_exp(shift))
    s_max, sh_max = float(scale.abs().max()), float(shift.abs().max())
    b_max, r_max = float(case['b'].abs().max()), float(case['res'].abs().max())
    plain_only = row.knobs.get('kslices', 1) > 1

    direct = float(conv64(row, case['x'].abs(), case['w'].abs()).max())
    q = max(grid_exp(case['x']) + grid_exp(case['w']), q_epi) + grid_exp(scale)
    units = (direct if plain_only else (direct + b_max) * max(s_max, 1.0) + sh_max + 4.0 * r_max) * 2.0 ** q
    cert = dict(direct_units=units, q=q, ok=units < LIMIT)
    if row.family in WINO_OF:
        # the transform-domain sum with bias and residual (they may be seeded into it); what the output transform returns is
        # the convolution's own value, an fp32 number, and the affine epilogue on it is the direct bound's above
        acc, qw, exact = winograd_bound(row, case)
        qw = max(qw, grid_exp(case['b']), grid_exp(case['res']))
        wu = (acc + b_max + 4.0 * r_max) * 2.0 ** qw
        cert.update(wino_units=wu, wino_q=qw, u_exact=exact, ok=cert['ok'] and exact and wu < LIMIT)
    if row.knobs.get('f16'):
        okx, lox = f16_split_ok(case['x'])
        okw, low = f16_split_ok(case['w'])
        cert.update(split_exact=okx and okw, lo_x=lox, lo_w=low, ok=cert['ok'] and okx and okw and not (lox and low))
    cert['units'] = max(cert['direct_units'], cert.get('wino_units', 0.0))
    return cert


# ------------------------------------------------------------------------------------------------------ planted defects
def _swap_pairs(c):
    idx = torch.arange(c) ^ 1
    return torch.where(idx < c, idx, torch.arange(c))


def planted_defects(row, case, samples=slice(0, 2)):
    """name -> (defective, clean) float64 outputs on the row's operands (the first samples: the defects do not depend on the
    sample), each defect an edit of the operands or of the geometry of the reference.  Only the defects that apply to the row."""
    x, w = case['x'][samples], case['w']
    (kh, kw), (ph, pw), s, c0 = row.k, row.pad, row.stride, row.c0
    vs = variants(row)
    full = vs.get('bias_res_relu')
    clean = conv64(row, x, w)
    d = {}

    def acc(name, out):
        d[name] = (out, clean)

    if kh > 1:
        acc('kernel flipped along H', conv64(row, x, w.flip(2)))
    if kw > 1:
        acc('kernel flipped along W', conv64(row, x, w.flip(3)))
    if kh == kw and kh > 1:
        acc('kh and kw transposed', conv64(row, x, w.transpose(2, 3)))
    for name, dl, dt in (('left', 1, 0), ('right', -1, 0), ('top', 0, 1), ('bottom', 0, -1)):
        acc(f'padding shifted by one, {name}', conv64(row, x, w, (pw + dl, pw - dl, ph + dt, ph - dt)))
    if s > 1:
        acc('stride phase starting at 1', conv64(row, x, w, (pw - 1, pw + 1, ph - 1, ph + 1)))
    wz = w.clone()
    wz[:, -1] = 0
    acc('the last input channel dropped', conv64(row, x, wz))
    if c0:
        wz = w.clone()
        wz[:, c0 - 1] = 0
        acc('the last channel of the first segment dropped', conv64(row, x, wz))
        if 2 * c0 == row.cin:
            acc('the two segments swapped', conv64(row, torch.cat([x[:, c0:], x[:, :c0]], 1), w))
        else:                                             # unequal segments: the second one read where the first one is
            xs = x.clone()
            m_ = min(c0, row.cin - c0)
            xs[:, :m_], xs[:, c0:c0 + m_] = x[:, c0:c0 + m_], x[:, :m_]
            acc('the two segments swapped', conv64(row, xs, w))
    z = clean.clone()
    z[:, :, -1, :] = 0
    acc('the last output row dropped', z)
    z = clean.clone()
    z[:, :, :, -1] = 0
    acc('the last output column dropped', z)
    for name, idx in (('topmost halo row', (slice(None), slice(None), 0)), ('bottommost halo row', (slice(None), slice(None), row.H - 1)),
                      ('leftmost halo column', (slice(None), slice(None), slice(None), 0)),
                      ('rightmost halo column', (slice(None), slice(None), slice(None), row.W - 1))):
        xz = x.clone()
        xz[idx] = 0
        acc(f'the {name} zeroed', conv64(row, xz, w))
    if row.cout > 1:
        acc('output channel c written to c ^ 1', clean[:, _swap_pairs(row.cout)])
        if 'bias' in vs:
            d['bias of channel c applied to c + 1'] = (epilogue64(case, clean, vs['bias'], samples, b=case['b'].roll(1)),
                                                        epilogue64(case, clean, vs['bias'], samples))
    if full is not None:
        want = epilogue64(case, clean, full, samples)
        rz = case['res'].clone()
        rz[:, (row.cout - 1) // 32 * 32:] = 0
        d['the residual left out on the last 32-channel fragment'] = (epilogue64(case, clean, full, samples, res=rz), want)
        d['ReLU applied before the residual'] = (epilogue64(case, clean, full, samples, relu_first=True), want)
    return d


# --------------------------------------------------------------------------------------- the table against the dispatch
@contextlib.contextmanager
def _host_descriptors():
    """ops.conv2d(.., _launch=False) on host tensors: the descriptor depends on shapes, strides and pointer alignment only"""
    prev, ops._dev = ops._dev, (lambda t, name: None)
    try:
        yield
    finally:
        ops._dev = prev


def packed_conv(row, case, spec, device='cpu'):
    ks = row.knobs.get('kslices', 1) > 1
    b = case['b'].to(device) if spec['bias'] and not ks else None
    bn = [t.to(device) for t in case['bn']] if spec['bn'] else None
    return ops.PackedConv.from_weight(case['w'].to(device), b, stride=row.stride, padding=row.pad, bn=bn, eps=0.0,
                                      dma_packing=row.knobs.get('dma_packing', True))


def launch_args(row, case, spec, x, res=None):
    """(x0, x1, kwargs) of ops.conv2d for a variant; x / res already on the device of the launch"""
    x0, x1 = (x[:, :row.c0], x[:, row.c0:]) if spec['two'] else (x, None)
    kw = dict(act=spec['act'], act2=spec['act2'], act_split=spec['split'])
    if spec['res']:
        kw['res'] = res
    if row.knobs.get('kslices', 1) > 1:
        kw['kslices'] = row.knobs['kslices']
    return x0, x1, kw


def host_query(row, spec=None):
    """scf_conv2d_query for the row's descriptor, built on host tensors: (return code, info)"""
    spec = spec or variants(row)['plain']
    ho, wo = out_hw(row)
    zero = dict(w=torch.zeros((row.cout, row.cin, *row.k)), b=torch.zeros(row.cout),
                bn=[torch.ones(row.cout)] * 4)
    x, res = torch.zeros((row.n, row.cin, row.H, row.W)), torch.zeros((row.n, row.cout, ho, wo))
    with route_knobs(row), _host_descriptors():
        pc = packed_conv(row, zero, spec)
        x0, x1, kw = launch_args(row, zero, spec, x, res)
        d, _ = ops.conv2d(pc, x0, x1, _launch=False, **kw)
        info = (C.c_int32 * 4)()
        rc = _lib.load().scf_conv2d_query(C.byref(d), info)
    return rc, tuple(info)


BY_ID.update({r.id: r for r in ROUTES})
IDS = [r.id for r in ROUTES]


def test_route_table_is_well_formed():
    assert len(BY_ID) == len(ROUTES)
    assert {r.family for r in ROUTES} == set(_lib.KERNEL_NAMES.values())
    for r in ROUTES:
        ho, wo = out_hw(r)
        assert ho >= 1 and wo >= 1 and 0 <= r.c0 < r.cin
        assert set(UNCERTIFIED) <= set(BY_ID)


@pytest.mark.parametrize('rid', IDS)
def test_table_matches_the_dispatch_at_256_cus(rid):
    """without a device the library plans for 256 CUs (scf_cu_count): the dry run of the row's plain descriptor answers the
    pinned info.  With another device present the plan is that device's: the GPU test compares there."""
    if torch.cuda.is_available() and torch.cuda.get_device_properties(0).multi_processor_count != 256:
        pytest.skip('the table is pinned for 256 CUs')
    row = BY_ID[rid]
    rc, info = host_query(row)
    assert rc == 0 and info == tuple(row.info), (rid, rc, info)


@pytest.mark.parametrize('rid', IDS)
def test_every_row_certifies(rid):
    row = BY_ID[rid]
    case = lattice_case(row)
    cert = case['certificate']
    print(f"[measured] {rid}: m={case['m']} density={case['density']} units {cert['units']:.3g} of 2^24 (q={cert['q']})")
    if rid in UNCERTIFIED:
        assert not cert['ok'], f'{rid} certifies: take it off UNCERTIFIED'
        return
    assert cert['ok'], (rid, cert)
    assert cert.get('u_exact', True)
    # the sparse operands keep what the kernels' edges need: chunk ends, the tail chunk, both segments, borders and corners
    x, w = case['x'], case['w']
    for c in _kept_channels(row):
        assert bool((x[:, c, [0, 0, -1, -1], [0, -1, 0, -1]] != 0).all()) and bool((w[:, c].reshape(row.cout, -1) != 0).any(1).all())
    for c in (0, row.cin - 1):
        assert bool((x[:, c, 0] != 0).all() and (x[:, c, -1] != 0).all() and (x[:, c, :, 0] != 0).all() and (x[:, c, :, -1] != 0).all())
    # and the reference is exact: fp32 holds every element of it
    ref = reference(row, case, variants(row)['plain'])
    assert torch.equal(ref.float().double(), ref)


@pytest.mark.parametrize('rid', IDS)
def test_planted_defects_move_the_reference(rid):
    row = BY_ID[rid]
    case = lattice_case(row)
    for name, (bad, clean) in planted_defects(row, case).items():
        assert bad.shape == clean.shape and not torch.equal(bad, clean), f'{rid}: degenerate operands for "{name}"'


def test_the_certificate_refuses_what_is_not_exact():
    """operands just past the bound, weights off the Winograd lattice and two non-zero low halves are all refused"""
    row = BY_ID[IDS[0]]
    case = dict(lattice_case(row))
    assert case['certificate']['ok']
    big = dict(case, x=case['x'] * 2.0 ** 22)
    assert not certify(row, big)['ok']
    for r in ROUTES:
        if r.family == 'winograd F(2,5)':
            c = dict(lattice_case(r))
            off = dict(c, w=c['w'] + 1.0)                 # 24 Z + 1: U has thirds, the packed fp32 value is not G g
            cert = certify(r, off)
            assert not cert['ok'], (r.id, cert)
            break
    for r in ROUTES:
        if r.knobs.get('f16'):
            c = dict(lattice_case(r))
            both = dict(c, x=c['x'] + (c['x'] != 0) * 2.0 ** -13, w=c['w'] + (c['w'] != 0) * 2.0 ** -13)
            assert not certify(r, both)['ok']
            break
