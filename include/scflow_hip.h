/*
 * scflow_hip.h -- C ABI of libscflow_hip.so: hand-written gfx950 (MI355X) kernels for
 * the SCFlow recurrent flow/pose refinement hot path.
 *
 * Conventions (all entry points)
 *   - plain C, no C++/torch types; every pointer is a DEVICE pointer to fp32 data laid
 *     out exactly as the reference's contiguous NCHW torch tensors unless stated;
 *   - pointers are borrowed: nothing is allocated, freed or retained;
 *   - work is enqueued asynchronously on `stream` (a hipStream_t; NULL = default
 *     stream); the call returns after launch, it never synchronises;
 *   - return value: SCF_OK (0) or a negative SCF_E* code; scf_error_string() decodes;
 *   - thread-safety: calls are independent; concurrent calls on different streams OK.
 *
 * The reference is pure Python on torch (no FFI of its own).  Each entry point names the
 * reference operator (file:line under the reference checkout) whose arithmetic it
 * replaces; INTEGRATION.md shows the ctypes stub a reference maintainer would add.
 */
#ifndef SCFLOW_HIP_H
#define SCFLOW_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* scf_stream_t; /* bit-compatible with hipStream_t */

enum {
  SCF_OK = 0,
  SCF_EINVAL = -1,      /* bad argument (null pointer, non-positive size, ...) */
  SCF_EUNSUPPORTED = -2,/* shape/config outside what the kernels implement */
  SCF_ELAUNCH = -3,     /* HIP reported a launch error */
  SCF_ENODEVICE = -4    /* no gfx950 device visible */
};

/* Pyramid levels an entry point accepts.  Level l of an h x w map is (h >> l) x (w >> l) and the
 * volume holds (h w)^2 floats per pair, so 12 levels already means a pyramid of more than 288 GB:
 * the bound never binds on this device. */
#define SCF_MAX_LEVELS 12

/* activation codes used by scf_conv2d / scf_linear */
enum { SCF_ACT_NONE = 0, SCF_ACT_RELU = 1, SCF_ACT_SIGMOID = 2, SCF_ACT_TANH = 3 };

/* fused epilogues of scf_conv2d */
enum {
  SCF_CONV_PLAIN = 0,
  SCF_CONV_GRU_ZR = 1, /* rows [0,Cout/2): z=sigmoid -> out; rows [Cout/2,Cout): r=sigmoid, aux = r*h */
  SCF_CONV_GRU_Q = 2   /* q=tanh; out = (1-z)*h + z*q                                   */
};

/* ABI version of this header: SCF_ABI_MAJOR changes whenever a struct layout or a signature changes
 * (scf_conv_desc has grown twice), the minor part when entry points are added.  scf_version()
 * returns the number the LIBRARY was built with: a C caller compares scf_version() / 100 with
 * SCF_ABI_MAJOR before its first call; structs additionally carry no size field,
 * so a mismatch must be refused, not worked around. */
#define SCF_ABI_MAJOR 5
#define SCF_VERSION (SCF_ABI_MAJOR * 100 + 3)   /* .1: label_mode is a bit set (SCF_POSE_*); .2: scf_conv2d_pair, overlap_* = 2;
                                                  .3: scf_flow_corr_2d3d, scf_pnp_ransac, scf_pnp_workspace_bytes */
int scf_version(void);
const char* scf_error_string(int code);
/* number of HIP devices visible (>=0) or SCF_ENODEVICE */
int scf_device_count(void);

/* ---------------------------------------------------------------------------------
 * Correlation volume + pyramid.            replaces CorrelationPyramid.forward
 *                                          models/decoder/raft_decoder.py:35-58
 * level0[n, i, j] = sum_c feat1[n,c,i] * feat2[n,c,j] / sqrt(C)   (i, j in [0, h*w))
 * level(l+1) = 2x2/stride-2 average pool of level l over the target (j) dims.
 * levels[l] : (N*h*w, 1, h>>l, w>>l) contiguous, l < L (host array of device ptrs).
 * MFMA (v_mfma_f32_32x32x2_f32) contraction; exact fp32 fma chain over c.
 * --------------------------------------------------------------------------------- */
int scf_corr_build(const float* feat1, const float* feat2, float* const* levels,
                   int N, int C, int h, int w, int L, scf_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Multi-scale correlation lookup.          replaces CorrLookup.forward
 *                                          models/utils/corr_lookup.py:102-136
 * out[n, 81*l + 9*a + b, y, x] = bilinear(level l of query (n,y,x)) sampled at
 *   ((x + flow[n,0,y,x]) / 2^l + a - r, (y + flow[n,1,y,x]) / 2^l + b - r),
 * zero padding, align_corners=True semantics; out is (N, L*(2r+1)^2, h, w).
 * HBM-bound gather: 2904 B/query algorithmic traffic at r=4, L=4.
 * --------------------------------------------------------------------------------- */
int scf_corr_lookup(const float* const* levels, const float* flow, float* out,
                    int N, int h, int w, int r, int L, scf_stream_t stream);

/* The same pair with a lookup-friendly layout for the levels the caller names: bit l of
 * `tiled_levels` set = every query's level-l map is stored in 8(x) x 4(y)-float tiles of one
 * 128-byte line each -- tile-major, row-major inside a tile, the map padded to a multiple of 4 rows
 * and 8 columns (padding floats are never read and may hold anything).  A (2r+2)^2 lookup window
 * then touches ~(1 + (2r+1)/8)(1 + (2r+1)/4) = 6.9 lines at r = 4 instead of one or two lines per
 * window row of a row-major map.  Level 0 is written by the correlation GEMM whose fragments are
 * whole tiles: bit 0 needs w % 8 == 0 and h % 4 == 0 (SCF_EUNSUPPORTED otherwise).
 *   scf_corr_level_floats      floats per query of level `level` in the given layout
 *                              (levels[l] holds N*h*w maps of that many floats)
 *   scf_corr_preferred_layout  the mask the lookup kernel is fastest with (tiles for every level
 *                              whose rows are at least 24 floats long and that does not fit the
 *                              lookup window whole)
 * tiled_levels = 0 is exactly scf_corr_build / scf_corr_lookup.  Both calls of a pair must be given
 * the same mask.
 * scf_corr_lookup[_ex] accepts ANY radius >= 1, level count <= SCF_MAX_LEVELS and map size
 * (CorrLookup's constructor arguments, corr_lookup.py:91-102): r <= 4 with maps of at most 32767
 * floats run on the LDS-DMA kernel, everything else on a plain gather kernel with the same
 * arithmetic.  A query whose flow is NaN / inf yields NaN in all its taps, as torch's
 * grid_sample does on the reference's CPU path. */
int64_t scf_corr_level_floats(int h, int w, int level, int tiled);
unsigned scf_corr_preferred_layout(int h, int w, int r, int L);
int scf_corr_build_ex(const float* feat1, const float* feat2, float* const* levels, int N, int C,
                      int h, int w, int L, unsigned tiled_levels, scf_stream_t stream);
int scf_corr_lookup_ex(const float* const* levels, const float* flow, float* out, int N, int h,
                       int w, int r, int L, unsigned tiled_levels, scf_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Direct convolution as implicit GEMM on MFMA with fused epilogue.
 * replaces every torch conv2d (+bias +BN(eval) +residual +activation +GRU gating) on
 * the path: raft_encoder.py:286-314, resnet.py:67-94, raft_decoder.py:152-166,
 * :235-253, :292-294, scflow_decoder.py:216-217, pose_head.py:148-160.
 *
 * Input = channel-concatenation of up to two NCHW segments (avoids torch.cat).
 * Weights are pre-packed by scf_pack_conv_weight_size/scf_pack layout rules:
 *   wp[((chunk*T + t)*KC + cl) * Mld + co],  chunk = ci / KC, cl = ci % KC, t = ky*KW+kx,
 *   rows for ci >= Cin are zero, Mld = row stride (>= Cout, multiple of 4).
 * Epilogue order: v = acc / out_div (+bias) -> v*scale+shift -> +res -> act -> mode.
 * --------------------------------------------------------------------------------- */
typedef struct scf_conv_desc {
  const float* in0; const float* in1;   /* input segments (in1 may be NULL)            */
  int32_t C0, C1;                       /* channels of each segment                    */
  int64_t in0_nstride, in1_nstride;     /* floats between consecutive samples          */
  int32_t N, H, W;                      /* batch, input height/width                   */
  const float* wp;                      /* packed weights                              */
  int64_t w_nstride;                    /* 0 = shared weights; else per-sample stride  */
  int32_t Mld;                          /* packed row stride                           */
  int32_t Cout;
  int32_t KH, KW, stride, pad_h, pad_w;
  int32_t KC;                           /* channel chunk used at packing time (2, 8, 32) */
  float* out; int64_t out_nstride;
  const float* bias;                    /* [Cout] or NULL                              */
  const float* scale; const float* shift; /* [Cout] each or both NULL (BN eval)        */
  const float* res; int64_t res_nstride;  /* residual added before act (GRU modes: before
                                             the gate's sigmoid / tanh), or NULL       */
  float out_div;                        /* accumulator divided by this (1 = off)       */
  int32_t act, act2, act_split;         /* act for co < act_split, act2 otherwise;
                                           act_split <= 0 -> act everywhere            */
  int32_t mode;                         /* SCF_CONV_*                                  */
  const float* gru_h; int64_t gru_h_nstride; /* hidden state (ZR, Q)                   */
  float* gru_aux; int64_t gru_aux_nstride;   /* ZR: r*h destination                    */
  const float* gru_z; int64_t gru_z_nstride; /* Q: z                                   */
  const void* wp_f16;                   /* optional split-fp16 packing of the same weights:
                                           [(chunk16*T + tap)*2 + k8][plane hi|lo][Mld][8] halves;
                                           non-NULL selects the 3xMFMA fp16 kernel where the
                                           shape fits (fp32-class accuracy)   */
  const float* wp_a4;                   /* optional second packing of the same weights for the
                                           LDS-DMA kernel (stride 1): [chunk][tap][g][h][Mld_a4][4]
                                           floats, channel = chunk*8G + 8g + 2s + h at float s      */
  int32_t a4_groups;                    /* G in {1,2,4}: 8G channels per staged chunk              */
  int32_t a4_mld;                       /* Cout rounded up to 32                                    */
  const float* wp_a4s;                  /* optional: the same a4 packing with MORE channels per chunk
                                           (a4s_groups = 4 for 1x1 / 1x5 / 5x1, 2 for 3x3), used on
                                           SMALL grids (batch 1): there one block runs per CU, a chunk's
                                           fixed cost (barrier, staging issue) dominates 8-channel chunks,
                                           and LDS is free for a deep ring of bigger ones                */
  int32_t a4s_groups;
  const float* wp_thin;                 /* optional third packing for Cout <= 4 layers (vector-ALU
                                           kernel): [Cin][KH*KW][CO] floats, CO = 1, 2 or 4 (Cout
                                           rounded up), zero padded                                */
  int32_t out_tile8x4;                  /* 1: store every output plane in 8(x) x 4(y)-float tiles
                                           of 128 B (tile-major, row-major inside) instead of
                                           row-major; needs Wo % 8 == 0 and Ho % 4 == 0          */
  const float* wp_taps;                 /* optional packing for thin INPUTS (Cin <= 4: the 7x7 stems, the
                                           2 -> 128 7x7 and 1 -> 64 3x3 first layers): [Kp][Mld] floats,
                                           row k = ci * KH*KW + t, Kp = Cin*KH*KW rounded up to a multiple of
                                           8, zero padded; selects the kernel that contracts over taps x channels
                                           as one dense K dimension                                  */
  const float* wp_a4t;                  /* optional: the a4 packing with a4t_groups = 4 (32-channel chunks) for
                                           3x3 layers, used on TINY grids (no more K-split blocks than CUs:
                                           every block is alone on its CU, a launch is a chain of one memory
                                           round trip per chunk, so half as many chunks is half the chain)    */
  int32_t a4t_groups;
  const float* wp_wino1d;               /* optional: G g of a 1x5 / 5x1 stride-1 'same' layer (scf_pack_conv_weight_wino1d);
                                           selects the one-dimensional Winograd F(2, 5) fp32 kernel (every epilogue
                                           kind incl. the GRU gates) on grids of >= CUs / 2 blocks (128 on the
                                           MI355X); same contract as wp_wino */
  const float* wp_wino;                 /* optional: G g G^T of a 3x3 / stride-1 / pad-1 layer
                                           (scf_pack_conv_weight_wino); selects the Winograd F(2x2, 3x3)
                                           fp32 kernel for plain / affine epilogues (bias, BN, residual,
                                           ReLU) on grids of >= CUs / 2 blocks (smaller grids: the direct kernels).
                                           Same fp32 arithmetic, re-associated sums: results differ from the direct
                                           kernels by a few ulp of sum |w||x|.  Kernel selection therefore depends on
                                           N and on the device: leave both Winograd packings NULL for results that
                                           do not */
  const float* wp_wino1d4;              /* optional: the F(4, 5) packing of the same 1x5 / 5x1 layer (scf_pack_conv_weight_wino1d4):
                                           four outputs per 8 multiplies; taken before wp_wino1d on grids of more than CUs / 2 of its
                                           blocks (64 channels x 256 pixels); same contract as wp_wino */
  int32_t k_slices;                     /* 0 / 1: off.  S > 1 (r5): the contraction over the input channels is split across
                                           S groups of BLOCKS: slice s contracts its share of the channel chunks and stores the
                                           raw partial sums at out + s * out_slice_stride; the CONSUMER adds the S partial
                                           tensors in slice order (scf_group_norm_relu_parts, scf_fc_splitk's x_parts) -- no
                                           atomics, a fixed summation order.  Small grids only (a block there is a chain of one
                                           memory round trip per chunk: S slices = 1 / S of the chain on S times the blocks).
                                           Plain epilogue required: no bias / scale / res / act / GRU mode / out_div / tiled
                                           output; LDS-DMA kernel only (wp_a4 or wp_a4s), else SCF_EUNSUPPORTED */
  int64_t out_slice_stride;             /* floats between consecutive partial tensors (>= N * out_nstride) */
} scf_conv_desc;

int scf_conv2d(const scf_conv_desc* desc, scf_stream_t stream);

/* Optional scratch for small grids (r5): register `floats` floats of device memory for launches on `stream` (borrowed until
 * replaced or cleared with ptr = NULL, floats = 0; one workspace per stream -- concurrent streams must not share one).  A
 * convolution whose every block would be alone on its CU with a chain of >= 4 staged chunks (batch 1 ... 4: one memory
 * round trip per chunk, whatever it computes) is then split into up to 4 K slices that write partial tensors to the
 * workspace, followed by one combine launch that adds them in slice order and applies the descriptor's whole epilogue (any
 * kind, GRU gates included).  Same result as the single launch up to the re-association of the partial sums;
 * deterministic; applies to every entry point that launches convolutions on that stream (scf_sepconv_gru*,
 * scf_scflow_iteration).  Needs N * Cout * Ho * Wo * slices floats; launches that need more stay unsliced.
 * The registry is keyed by the raw stream handle: clear the entry (ptr = NULL) BEFORE destroying the stream, a later
 * stream that gets the same handle would inherit it. */
int scf_conv_workspace(scf_stream_t stream, float* ptr, int64_t floats);

/* r6: two INDEPENDENT convolutions (no data flows between them) as ONE launch where both fall to the same small-grid kernel
 * instantiation (the K-split LDS-DMA tile, the thin-input kernel): blocks [0, nA) run a, the rest b.  Sub-chip grids
 * (batch 1-4: a layer is 8-64 blocks on 256 CUs) then run side by side without a second stream -- on this runtime a hipGraph
 * replay pays ~1.2 us per node once the graph holds a parallel branch.  Any other pair: the two launches one after the
 * other.  Results are those of scf_conv2d(a) and scf_conv2d(b), bit for bit, in both cases. */
int scf_conv2d_pair(const scf_conv_desc* a, const scf_conv_desc* b, scf_stream_t stream);

/* Host-side weight packers (plain CPU loops, run once per checkpoint): w is a HOST pointer to a
 * contiguous (Cout, Cin, KH, KW) fp32 tensor -- a torch Conv2d weight as stored in the reference's
 * state_dict -- and out a HOST buffer of scf_pack_conv_weight*_size() floats; copy the result
 * to the device and pass it as scf_conv_desc.wp (+ KC, Mld = Cout rounded up to 32) or
 * scf_conv_desc.wp_a4 (+ a4_groups, a4_mld = Cout rounded up to 32).
 *   KC packing : out[((chunk*T + t)*KC + cl)*Mld + co] = w[co][chunk*KC + cl][t], zeros elsewhere
 *   a4 packing : out[((((chunk*T + t)*G + g)*2 + h)*Mld + co)*4 + s] = w[co][chunk*8G + 8g + 2s + h][t] */
int64_t scf_pack_conv_weight_size(int Cout, int Cin, int KH, int KW, int KC);
int scf_pack_conv_weight(const float* w, int Cout, int Cin, int KH, int KW, int KC, float* out);
int64_t scf_pack_conv_weight_a4_size(int Cout, int Cin, int KH, int KW, int groups);
int scf_pack_conv_weight_a4(const float* w, int Cout, int Cin, int KH, int KW, int groups, float* out);
/*   taps packing (scf_conv_desc.wp_taps, Cin <= 4): out[(ci*KH*KW + t)*Mld + co] = w[co][ci][t], Mld = Cout
 *   rounded up to 32, rows rounded up to a multiple of 8, zeros elsewhere */
int64_t scf_pack_conv_weight_taps_size(int Cout, int Cin, int KH, int KW);
int scf_pack_conv_weight_taps(const float* w, int Cout, int Cin, int KH, int KW, float* out);
/*   Winograd packing (scf_conv_desc.wp_wino, 3x3 only): U[i][j] = (G g G^T)[i][j] per (co, ci), computed
 *   in double and rounded once;  out[((chunk*F + co/32)*16 + 4*pi(i) + j)*128 + (cl & 1)*64 + (co % 32)*2 + (cl >> 1)],
 *   pi = (0, 1, 3, 2): the rows of the transform domain are stored in the order 0, 1, 3, 2,
 *   with ci = 4*chunk + cl, F = Cout rounded up to 32, / 32; zeros elsewhere */
int64_t scf_pack_conv_weight_wino1d_size(int32_t Cout, int32_t Cin);
int scf_pack_conv_weight_wino1d(const float* w, int32_t Cout, int32_t Cin, float* out);   /* w: (Cout, Cin, 5) taps;
     out[((chunk*F + co/32)*6 + i)*256 + (cl & 1)*128 + (co % 32)*4 + (cl >> 1)] = (G g)[i], ci = 8*chunk + cl,
     G = the 6 x 5 matrix of the points 0, 1, -1, 2, -2, infinity */
int64_t scf_pack_conv_weight_wino1d4_size(int32_t Cout, int32_t Cin);
int scf_pack_conv_weight_wino1d4(const float* w, int32_t Cout, int32_t Cin, float* out);  /* w: (Cout, Cin, 5) taps;
     out[((chunk*F + co/32)*8 + i)*128 + (cl & 1)*64 + (co % 32)*2 + (cl >> 1)] = (G g)[i], ci = 4*chunk + cl,
     G = the 8 x 5 matrix of the points 0, 1, -1, 2, -2, 1/2, -1/2, infinity, row 0 negated */
int64_t scf_pack_conv_weight_wino_size(int32_t Cout, int32_t Cin);
int scf_pack_conv_weight_wino(const float* w, int32_t Cout, int32_t Cin, float* out);

/* ---------------------------------------------------------------------------------
 * Convolutional GRU update, whole cell.     replaces ConvGRU.forward
 *                                           models/decoder/raft_decoder.py:235-253
 * hx = [h (Ch channels) | x (Cx channels)] of one sample-strided NCHW buffer; for every pass
 * (SeqConv: a (1,5) then a (5,1) convolution triple, :180-181; Conv: one 3x3 triple)
 *     z = sigmoid(conv_z(hx)),  r = sigmoid(conv_r(hx)),  q = tanh(conv_q([r*h | x])),
 *     h <- (1 - z)*h + z*q                                              (in place in hx)
 * as two launches: one 2*Ch-row convolution whose epilogue emits z and r*h, one Ch-row
 * convolution whose epilogue applies tanh and the state update.  z and rh are caller-provided
 * dense (N, Ch, H, W) scratch buffers.
 * Weights per pass, DEVICE pointers in the packings above:
 *   wp_zr : KC = 8 packing of the (2*Ch, Ch+Cx, KH, KW) tensor cat([conv_z.weight, conv_r.weight], 0)
 *   wp_q  : KC = 8 packing of conv_q.weight (Ch, Ch+Cx, KH, KW);  bias_zr [2*Ch], bias_q [Ch]
 *   wp_*_a4 (+ a4_groups: 2 for (1,5)/(5,1), 1 for 3x3) select the LDS-DMA kernel (optional, faster)
 *   wp_*_f16 select the split-fp16 3xMFMA kernel (optional, see scf_conv_desc.wp_f16)
 *   wp_*_a4s (+ a4s_groups) : small-grid a4 packings (see scf_conv_desc.wp_a4s), optional
 *   wp_*_k32 : KC = 32 packings of the same tensors (optional): used instead of the KC = 8 ones
 *              when the grid is so small (batch 1) that the register-staged kernel with its
 *              smallest tile runs and an 8-channel chunk is too short to hide its prefetch
 * --------------------------------------------------------------------------------- */
typedef struct scf_gru_pass {
  int32_t KH, KW, pad_h, pad_w;
  const float* wp_zr; const float* bias_zr;
  const float* wp_q; const float* bias_q;
  const float* wp_zr_a4; const float* wp_q_a4; int32_t a4_groups;
  const void* wp_zr_f16; const void* wp_q_f16;
  const float* wp_zr_k32; const float* wp_q_k32;
  const float* wp_zr_a4s; const float* wp_q_a4s; int32_t a4s_groups;
  const float* wp_zr_a4t; const float* wp_q_a4t; int32_t a4t_groups;   /* 3x3 passes: tiny-grid packings (scf_conv_desc.wp_a4t), optional */
  const float* wp_zr_wino1d; const float* wp_q_wino1d;   /* 1x5 / 5x1 passes: F(2, 5) packings (scf_conv_desc.wp_wino1d), optional */
  const float* wp_zr_wino1d4; const float* wp_q_wino1d4; /* 1x5 / 5x1 passes: F(4, 5) packings (scf_conv_desc.wp_wino1d4), optional */
} scf_gru_pass;

int scf_sepconv_gru(float* hx, int64_t hx_nstride, int N, int Ch, int Cx, int H, int W,
                    const scf_gru_pass* passes, int npass, float* z, float* rh,
                    scf_stream_t stream);

/* The same update (ConvGRU.forward, raft_decoder.py:235-253) with the iteration-invariant part
 * of x hoisted out of the refinement loop.  hx = [h (Ch) | c (Cc) | x' (Cx)], where c -- the
 * context features, scflow_decoder.py:189-190 / raft_decoder.py:430 -- is the same in every
 * iteration: conv([h | c | x']) = conv([h | x']) + conv_c(c).  The caller computes, once per
 * pair and per pass i, ctx[i] = conv_c(c) + bias as a plain scf_conv2d over c whose weight is the
 * c columns of conv_z | conv_r | conv_q stacked into 3 Ch output rows: (N, 3 Ch, H, W) with
 * sample stride ctx_nstride, channels [0, 2 Ch) for z | r and [2 Ch, 3 Ch) for q.  `passes` then
 * holds packings over the remaining Ch + Cx input channels, with bias_zr = bias_q = NULL (folded
 * into ctx).  Results equal scf_sepconv_gru's up to fp32 summation order. */
int scf_sepconv_gru_ctx(float* hx, int64_t hx_nstride, int N, int Ch, int Cc, int Cx, int H, int W,
                        const scf_gru_pass* passes, int npass, const float* const* ctx,
                        int64_t ctx_nstride, float* z, float* rh, scf_stream_t stream);

/* ---------------------------------------------------------------------------------
 * One whole refinement iteration.           replaces the loop body of SCFlowDecoder.forward
 *                                           models/decoder/scflow_decoder.py:196-243
 * The launch sequence of an iteration -- 1/8 flow, lookup, motion encoder, SepConvGRU, flow / mask
 * heads, delta-flow / mask encoders, full-resolution outputs, pose head, pose update, pose-induced
 * flow: ~33 launches -- behind ONE call, so that a caller without hipGraph capture is bound by the
 * launch API and not by its interpreter.  Nothing new is computed: every step is one of the
 * operator entry points of this header, issued in a fixed order (results are bit-identical to
 * issuing them one by one).  The caller fills the struct ONCE per decoder pass (all scratch buffers
 * and convolution descriptors, weights in the packings of scf_conv_desc) and changes only the
 * "per iteration" pointers between calls.  struct_size = sizeof(scf_scflow_iter) is checked.
 * overlap_* (small batches): that branch is issued on side_stream between event fork / join points,
 * beside the main stream's work; the call itself never synchronises (hipGraph-capturable).
 * --------------------------------------------------------------------------------- */
typedef struct scf_iter_gn {          /* GroupNorm(G, eps, affine) + ReLU after a pose-head convolution */
  const float* gamma; const float* beta; float* out;
  int32_t C, HW, G; float eps;
} scf_iter_gn;

typedef struct scf_scflow_iter {
  int32_t struct_size;
  int32_t N, H, W, h, w;                     /* batch; full-resolution and 1/8-resolution sizes        */
  /* correlation pyramid (scf_corr_build_ex) and lookup */
  int32_t L, radius; uint32_t tiled_levels; int32_t corr_channels;   /* L * (2 radius + 1)^2            */
  const float* levels[SCF_MAX_LEVELS];
  float* flow_lr;                            /* (N, 2, h, w) scratch                                    */
  float* corr;                               /* (N, corr_channels, h, w) scratch                        */
  /* decoder switches mask_flow / mask_corr (:199-205) */
  int32_t mask_flow, mask_corr;
  const float* mask_prev;                    /* (N, 1, h, w): previous iteration's mask (ones before the first) */
  float* flow_masked;                        /* (N, 2, h, w) scratch, mask_flow only                    */
  /* motion encoder (in / out pointers set; flow0.in0 is replaced by the call) */
  scf_conv_desc flow0, flow1, corr0, corr1, outn;
  float* flow_copy_dst;                      /* hx[:, Ch + Cc + 126 ...]: the 2 flow channels of x      */
  /* SepConvGRU: hx = [h (Ch) | context (Cc) | motion features (Cx)] */
  float* hx; int64_t hx_nstride; int32_t Ch, Cc, Cx, npass;
  scf_gru_pass gru[2];
  const float* ctx[2]; int64_t ctx_nstride;  /* hoisted context terms (scf_sepconv_gru_ctx) or NULLs    */
  float* z; float* rh;
  /* heads and their encoders */
  scf_conv_desc heads, fpred, mpred, menc0, menc1, denc0, denc1;
  /* pose head: 3 x (conv -> GroupNorm + ReLU), 2 FC layers, rotation / translation heads */
  scf_conv_desc pose[3];
  scf_iter_gn gn[3];
  const float* fc1_w; const float* fc1_b; float* fc1_out; int32_t fc1_K, fc1_O;
  const float* fc2_w; const float* fc2_b; float* fc2_out; int32_t fc2_O;
  /* fc_fused != 0: the tail runs as three scf_fc_splitk launches -- the third GroupNorm + ReLU is applied by
   * fc1's operand load (gn[2].out unused), fc1_out / fc2_out are (fc1_slices, N, fc1_O) / (fc2_slices, N, fc2_O)
   * partial-sum buffers whose bias + ReLU the next layer's load applies.  0: scf_linear launches as before. */
  int32_t fc_fused, fc1_slices, fc2_slices;
  const float* rot_w; const float* rot_b; float* rot_all; int32_t rot_O;
  const float* trans_w; const float* trans_b; float* trans_all; int32_t trans_O;
  const int64_t* label; int32_t num_class, label_mode;
  /* pose-induced flow */
  const float* depth; const float* K; const float* R0; const float* t0; float invalid_flow_num;
  /* ---- per iteration ---- */
  const float* flow_in;                      /* (N, 2, H, W): the previous pose-induced flow (init_flow first) */
  const float* R_in; const float* t_in;
  float* flow_out; float* flow_pred; float* mask_up;       /* (N,2,H,W), (N,2,H,W), (N,1,H,W)           */
  float* R_out; float* t_out; float* d_rot; float* d_trans;
  /* ---- two-stream overlap ---- */
  scf_stream_t side_stream; int32_t overlap_flow, overlap_mask, overlap_up;
  void* lookup_timer;                        /* optional scf_timer_t (scflow_hip_prof.h) bound to the lookup launch */
} scf_scflow_iter;

int scf_scflow_iteration(const scf_scflow_iter* iter, scf_stream_t stream);

/* ---------------------------------------------------------------------------------
 * InstanceNorm2d(eps, affine=False) [+ residual] [+ ReLU] over N*C planes of HW floats.
 * replaces F.instance_norm at resnet.py:75-86 / raft_encoder.py:300-302 (norm_cfg IN).
 * out = relu?( (x - mean) * rsqrt(var_biased + eps) + res? ).  In-place allowed.
 * --------------------------------------------------------------------------------- */
int scf_instance_norm(const float* x, const float* res, float* out, int64_t planes,
                      int HW, float eps, int relu, scf_stream_t stream);
/* The tail of a residual block whose shortcut is normalised too (resnet.py:88-94 with a downsample branch):
 * out = relu?( IN(x) + IN(r) ), bit for bit scf_instance_norm(r -> r) followed by scf_instance_norm(x, res = r -> out),
 * in ONE pass over x and r for 16-byte-aligned planes of up to 16384 floats with HW % 4 == 0.  Other planes run those two
 * launches, which normalise r in place: the contents of r after the call are unspecified.  out may alias x or r.
 * Added without a version bump (SCF_VERSION stays at .3), as the renderer's entries were: its presence marks the feature. */
int scf_instance_norm_res_norm(const float* x, float* r, float* out, int64_t planes,
                               int HW, float eps, int relu, scf_stream_t stream);

/* GroupNorm(G, eps, affine) + ReLU on (N, C, HW).     replaces pose_head.py:151-159 */
int scf_group_norm_relu(const float* x, const float* gamma, const float* beta, float* out,
                        int N, int C, int HW, int G, float eps, scf_stream_t stream);
/* the same on an input that arrives as `parts` partial tensors part_stride floats apart (a convolution launched
 * with scf_conv_desc.k_slices = parts): every element is the sum of its parts in part order */
int scf_group_norm_relu_parts(const float* x, int parts, int64_t part_stride, const float* gamma,
                              const float* beta, float* out, int N, int C, int HW, int G, float eps,
                              scf_stream_t stream);

/* y[n, o] = act(sum_k W[o,k] x[n,k] + b[o]);  W row-major (O, K). replaces nn.Linear
 * at pose_head.py:166-172, 203-206.                                                 */
int scf_linear(const float* x, const float* W, const float* b, float* y, int N, int K,
               int O, int act, scf_stream_t stream);

/* Two linear layers over the same input in one launch: y1 = act(W1 x + b1), y2 = act(W2 x + b2)
 * (rotation_pred and translation_pred, pose_head.py:203-206).  Same arithmetic as two scf_linear
 * calls.                                                                            */
int scf_linear_pair(const float* x, const float* W1, const float* b1, float* y1, int O1,
                    const float* W2, const float* b2, float* y2, int O2, int N, int K, int act,
                    scf_stream_t stream);

/* ---------------------------------------------------------------------------------
 * nn.Linear as a split-K GEMM on the matrix cores, with its element-wise neighbours folded into the operand
 * loads: the pose head's flatten -> fc1 -> ReLU -> fc2 -> ReLU -> rotation_pred | translation_pred
 * (pose_head.py:166-172, 201-211) in three launches that read every weight once per batch.
 *   input    x[n][k] = f( sum_{s < x_parts} x[s][n][k] + x_bias[k] ), f = ReLU if x_relu: the partial sums a
 *            previous scf_fc_splitk wrote (x_part_stride floats between parts; x_parts = 1, x_bias = NULL: a plain
 *            (N, K) tensor);
 *            gn_groups > 0: GroupNorm(gn_groups, gn_eps, affine) + ReLU over the K features of each sample first
 *            (group = K / gn_groups consecutive features, channel of feature k = k / gn_hw: the flattened
 *            (C, h, w) map of pose_head.py:151-159 with gn_hw = h w) -- replaces scf_group_norm_relu on that map;
 *   output   slices == 1: y[n][o] = act(sum_k W[o][k] x[n][k] + bias[o]), and the same for the optional second
 *            matrix (W2, bias2, y2, O2: rotation_pred and translation_pred read the same features);
 *            slices  > 1: y = (slices, N, O) partial sums over K / slices features each, no bias / act -- the
 *            consumer adds them in slice order (x_parts, x_bias, x_relu of the next call).
 * K % slices == 0, K / slices <= 256 and a multiple of 8 (and of the group size), 16-byte aligned rows.
 * W row-major (O, K) like nn.Linear.weight.  Sums are fp32 fma chains in a fixed order (deterministic).
 * --------------------------------------------------------------------------------- */
typedef struct scf_fc_desc {
  const float* x; int32_t x_parts; int64_t x_part_stride;
  const float* x_bias; int32_t x_relu;
  int32_t gn_groups, gn_hw; const float* gn_gamma; const float* gn_beta; float gn_eps;
  int32_t N, K;
  const float* W; const float* bias; float* y; int32_t O;
  const float* W2; const float* bias2; float* y2; int32_t O2;
  int32_t act;                          /* SCF_ACT_* of the finished outputs (slices == 1)  */
  int32_t slices;
} scf_fc_desc;
int scf_fc_splitk(const scf_fc_desc* desc, scf_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Pose head tail + pose update.  replaces pose_head.py:207-210 (class select) and
 * get_pose_from_delta_pose, models/utils/pose.py:124-149 (+ :153-169 ortho6d).
 * rot_all (N, num_class*6), trans_all (N, num_class*3) are the two linear heads' outputs.
 * label_mode is a bit set (any other bit: SCF_EINVAL):
 *   0                          the reference's inference path: every sample is decoded with class label[0]
 *                              (index_select(...)[:, 0], pose_head.py:209-210), depth_transform='exp' (pose.py:137-138)
 *   SCF_POSE_LABEL_PER_SAMPLE  sample n uses label[n]
 *   SCF_POSE_DEPTH_LINEAR      the other depth_transform branch, pose.py:139-141: t_z' = t_z * (d_z + 1)
 * Outputs: d_rot (N,6), d_trans (N,3), R_out (N,3,3), t_out (N,3).  R_out/t_out may alias R_in/t_in.
 * A label outside [0, num_class) is CLAMPED (a kernel cannot raise; the reference's index_select
 * does): validate labels on the host (SCFlowRefiner.forward_single_pass does).
 * --------------------------------------------------------------------------------- */
#define SCF_POSE_LABEL_PER_SAMPLE 1
#define SCF_POSE_DEPTH_LINEAR 2
int scf_pose_update(const float* rot_all, const float* trans_all, const int64_t* label,
                    int num_class, int label_mode, const float* R_in, const float* t_in,
                    float* d_rot, float* d_trans, float* R_out, float* t_out, int N,
                    scf_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Pose-induced flow (dense form of cal_3d_2d_corr + get_flow_from_delta_pose_and_points,
 * models/utils/pose.py:44-64, 66-88).  For every pixel with depth > 0:
 *   P = R0^-1 (K^-1 [x y 1]^T d - t0);  p = K (R P + t);  flow = (p_x/p_z - x, p_y/p_z - y)
 * else flow = invalid_num.  depth (N,H,W); K,R0,R (N,3,3); t0,t (N,3); flow (N,2,H,W).
 * --------------------------------------------------------------------------------- */
int scf_reproject_flow(const float* depth, const float* K, const float* R0, const float* t0,
                       const float* R, const float* t, float* flow, int N, int H, int W,
                       float invalid_num, scf_stream_t stream);

/* BaseDataset.eval_pose_error (datasets/base_dataset.py:378-424; project_3d_point,
 * datasets/pose.py:18-78) for the samples sample_idx[0..nsel) that share one vertex set
 * verts (nv,3): err3d[s] = ADD (symmetric = 0) or ADD-S (closest predicted point, symmetric
 * != 0), err2d[s] = mean reprojection distance with x / (z + 1e-8).  float64 throughout, like
 * the reference's numpy arrays; gt_r/pred_r/K (N,3,3), gt_t/pred_t (N,3), outputs (N). */
int scf_pose_error(const double* verts, int nv, const double* gt_r, const double* gt_t,
                   const double* pred_r, const double* pred_t, const double* K,
                   const int* sample_idx, int nsel, int symmetric, double* err3d, double* err2d,
                   scf_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Flow -> 2-D/3-D correspondences.   replaces get_2d_3d_corr_by_fw_flow + cal_3d_2d_corr,
 *                                    models/utils/pose.py:44-64, 182-200
 * Per sample n, every pixel (x, y) with depth > 0 (and, when occ is not NULL, occ > occ_thresh;
 * a NaN occlusion is not kept) is written out compacted in row-major order (torch.nonzero's order):
 *   pts2d[n, i] = (x + flow[n,0,y,x], y + flow[n,1,y,x])              (the target-image point)
 *   pts3d[n, i] = R0^-1 (K^-1 [x y 1]^T d - t0)                         (lift_2d_to_3d, as scf_reproject_flow)
 *   conf[n, i]  = occ[n,y,x] (1 without occ);  count[n] = number of kept pixels.
 * flow (N,2,H,W); depth, occ (N,H,W); K, R0 (N,3,3); t0 (N,3); outputs have capacity H*W per sample:
 * pts2d (N,H*W,2), pts3d (N,H*W,3), conf (N,H*W), count (N) int32.  Entries >= count[n] are left untouched.
 * --------------------------------------------------------------------------------- */
int scf_flow_corr_2d3d(const float* flow, const float* depth, const float* occ, float occ_thresh,
                       const float* K, const float* R0, const float* t0, int N, int H, int W,
                       float* pts2d, float* pts3d, float* conf, int32_t* count, scf_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Batched RANSAC-EPnP.               replaces sample_points + solve_pose_by_pnp (cv2.solvePnPRansac with
 *                                    SOLVEPNP_EPNP), base_flow_refiner.py:49-71, pose.py:203-249
 * Inputs: the outputs of scf_flow_corr_2d3d (capacity = points per sample; conf only read by TOPK), K (N,3,3),
 * the reference pose R_ref (N,3,3), t_ref (N,3).  Per sample:
 *   sampling   ALL: every point.  TOPK: the sample_num points of highest conf, ties to the lower index (-0.0 ties
 *              with +0.0; NaN ranks above +inf); the kept indices are ascending.
 *              RANDOM: sample_num distinct indices of [0, count-1) chosen by a counter-based hash of
 *              (seed, index) -- the reference's randperm(count - 1) quirk kept, its generator not reproduced.
 *              Both keep every point when sample_num > count.
 *   hypotheses `iterations` of them; hypothesis h takes 5 distinct points of the m kept ones: draws a = 1..64
 *              give index hash(seed, h, a) % m, a repeat is skipped, and a hypothesis with fewer than 5 distinct
 *              points after 64 draws is invalid (hash: pnp_hash in pnp.hip, the splitmix64 finaliser) -- the
 *              sample's position in the batch does not enter, so a sample gives the same bits alone or batched --
 *              and solves EPnP on them (Lepetit et al.: control points at the centroid and at centroid +
 *              sqrt(variance) along each principal axis, each axis oriented so that its largest-magnitude component
 *              is positive; M over normalised camera coordinates K^-1 [u v 1]; 12x12 M^T M, the beta cases
 *              N = 1..3 each refined by 5 Gauss-Newton steps, lowest summed reprojection distance kept; fp64).
 *   scoring    inlier: projected depth > 0 and reprojection error < reproj_error pixels (NaN: outlier); the
 *              hypothesis with the most inliers wins, ties to the lowest h; all hypotheses run (no early stop).
 *   final      EPnP over every inlier of the winner, re-scored: inliers[n] = its inlier count.
 *   failure    ok[n] = 0, R/t = the reference pose, inliers[n] = 0 when count < 4, fewer than 5 points remain,
 *              the winner has fewer than 5 inliers, the inlier set is collinear or planar (smallest principal
 *              variance <= 1e-8 of the largest), or anything is non-finite.  Otherwise ok[n] = 1.
 * Outputs R (N,3,3), t (N,3) fp32; ok, inliers (N) int32.  workspace: scf_pnp_workspace_bytes(N, capacity, params)
 * bytes of device memory (0 for ALL: workspace may be NULL).  One workgroup per sample (see pnp.hip for the layout).
 * --------------------------------------------------------------------------------- */
enum { SCF_PNP_SAMPLE_ALL = 0, SCF_PNP_SAMPLE_TOPK = 1, SCF_PNP_SAMPLE_RANDOM = 2 };
typedef struct scf_pnp_params {
  int32_t iterations;     /* hypotheses (iterationscount), > 0                      */
  float reproj_error;     /* inlier threshold in pixels (reprojectionerror), >= 0   */
  int32_t sample_mode;    /* SCF_PNP_SAMPLE_*                                        */
  int32_t sample_num;     /* points kept by TOPK / RANDOM, > 0                       */
  uint64_t seed;          /* hypothesis and RANDOM draws                             */
} scf_pnp_params;
/* bytes of workspace scf_pnp_ransac needs, or SCF_EINVAL for bad arguments */
int64_t scf_pnp_workspace_bytes(int N, int capacity, const scf_pnp_params* params);
int scf_pnp_ransac(const float* pts2d, const float* pts3d, const float* conf, const int32_t* count, int N,
                   int capacity, const float* K, const float* R_ref, const float* t_ref,
                   const scf_pnp_params* params, float* R, float* t, int32_t* ok, int32_t* inliers,
                   void* workspace, scf_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Mesh renderer.                     replaces Renderer.forward (models/utils/rendering.py, pytorch3d
 *                                    MeshRasterizer + HardPhongShader) under the shipped configuration:
 *                                    faces_per_pixel=1, blur_radius=0, hard blending, Phong, no mask pass.
 * Added without a version bump (SCF_VERSION stays at .3): the presence of scf_render_mesh,
 * scf_render_workspace_bytes and scf_render_pixel_coord marks the feature.  render.hip states the semantics
 * in full; in short, per sample n with mesh m = labels[n]:
 *   camera     OpenCV R (N,3,3), t (N,3), K (N,3,3): X_c = R X + t, u = fx X_c.x / X_c.z + cx (v likewise).
 *   sampling   output column c samples u(c) = (W-1)/2 - (S-1)(W-2c-1)/(2S), S = min(H,W); rows likewise with H
 *              (pytorch3d's flipped non-square NDC grid under cameras_from_opencv_projection); see
 *              scf_render_pixel_coord.
 *   coverage   all three screen barycentrics >= 0; faces of zero screen area or with every vertex at z <= 0 are
 *              skipped, hits whose perspective-correct z <= 0 are discarded; no back-face culling.
 *   depth      the hit is the lexicographic minimum of (z, face index); 1/z is linear in screen space.
 *   outputs    zbuf (N,H,W) = z or -1; pix_to_face (N,H,W) int32 = face index within mesh m, or -1;
 *              rgba (N,H,W,4) and / or rgb_nchw (N,3,H,W) = (rgb - norm_mean[c]) / norm_std[c]; either may be NULL.
 *   shading    pytorch3d phong_shading + hard_rgb_blend in the object frame, perspective-correct barycentrics,
 *              material colours 1, shininess 64; lights per default_lights / seperate_lights (render.hip).
 * A label outside [0, num_classes) renders background (the kernels cannot raise; validate labels beforehand).
 * The mesh store holds every class mesh concatenated: class k owns vertices [vert_offset[k], vert_offset[k+1])
 * and faces [face_offset[k], face_offset[k+1]); face indices are local to the class.  max_faces >= the largest
 * class's face count.  workspace: scf_render_workspace_bytes(N, max_faces) bytes of device memory.
 * --------------------------------------------------------------------------------- */
typedef struct scf_mesh_store {
  const float* verts;          /* (V,3) object-frame positions                         */
  const float* normals;        /* (V,3) vertex normals (need not be unit length)       */
  const float* colors;         /* (V,3) vertex colours in [0,1]                         */
  const int32_t* faces;        /* (F,3) vertex indices, local to the face's class       */
  const int32_t* vert_offset;  /* (num_classes+1)                                       */
  const int32_t* face_offset;  /* (num_classes+1)                                       */
  int32_t num_classes;
  int32_t max_faces;
} scf_mesh_store;
typedef struct scf_render_params {
  int32_t H, W;                /* image size, 1..8192 each                             */
  int32_t default_lights;      /* 1: pytorch3d PointLights colours; 0: ambient .8, diffuse .5, specular 1 */
  int32_t seperate_lights;     /* 1: light at R (0, 0, max(zmin_n - 400, 0)) per sample */
  float background[3];         /* RGB of uncovered pixels                              */
  float norm_mean[3];          /* rgb_nchw = (rgb - norm_mean) / norm_std per channel  */
  float norm_std[3];
} scf_render_params;
/* image-plane coordinate sampled by pixel `index` along an axis of `size` pixels when the other axis has `other`
 * pixels (host function, no device involved) */
double scf_render_pixel_coord(int index, int size, int other);
/* bytes of workspace scf_render_mesh needs, or SCF_EINVAL for bad arguments */
int64_t scf_render_workspace_bytes(int N, int max_faces);
int scf_render_mesh(const scf_mesh_store* mesh, const int32_t* labels, const float* R, const float* t,
                    const float* K, int N, const scf_render_params* params, float* zbuf, int32_t* pix_to_face,
                    float* rgba, float* rgb_nchw, void* workspace, scf_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Object patches from full frames.   replaces the val_pipeline of configs/refine_datasets/ycbv_*.py (ComputeBbox,
 *                                    Crop, Resize(keep_ratio=True), Pad, RemapPose(keep_intrinsic=False), Normalize),
 *                                    which the reference runs on the CPU through cv2 / mmcv.
 * Added without a version bump (SCF_VERSION stays at .3), as the renderer's entries were: the presence of
 * scf_patch_workspace_bytes, scf_patch_boxes and scf_patch_extract marks the feature.  patch.hip states the
 * semantics in full; in short, per object n:
 *   box        min / max of u = p.x / (p.z + 1e-8), v likewise, p = K (R X + t), over every vertex_stride-th vertex
 *              of class labels[n] (fp32).  Invalid: label outside [0, num_classes), empty class, any p.z <= 0.
 *   crop       Crop's rectangle from the box (aspect_ratio / keep_ratio, size_ratio, min_expand, clip_border) in fp64,
 *              truncated toward zero, ends inclusive; pixels outside the frame are crop_pad_val.  With crop_in
 *              (N,4) int32 the caller's rectangles (x1, y1, x2, y2) are used instead and mesh, labels, R, t may be
 *              NULL (the reference's crop_bbox_field when a detector box is at hand).
 *   resize     s = resize / max(ph, pw); OpenCV's generic 8-bit INTER_LINEAR (11-bit fixed-point coefficients).
 *   pad        to (out_h, out_w) with pad_val, centred when center != 0.
 *   intrinsics transform_matrix = P S C, k = transform_matrix K, fp64 rounded once; poses pass through.
 *   normalize  out (N,3,out_h,out_w) = (float(v) - mean[c]) * float(1.0 / std[c]), c the output channel; the frame is
 *              read as BGR and to_rgb swaps channels 0 and 2.  crop_pad_val / pad_val are in the frame's channel order.
 * An invalid object gets an all-pad_val patch, valid = 0, a zero rectangle, scale 1, an identity transform_matrix and
 * k = K (the kernels cannot raise).  scf_patch_boxes writes box (N,4) fp32 (the projected box
 * (x1, y1, x2, y2); may be NULL; zeros for an invalid object or with crop_in), crop (N,4) int32, scale (N), transform_matrix (N,3,3),
 * k (N,3,3), valid (N) int32 and one record per object into workspace (scf_patch_workspace_bytes(N) bytes of device
 * memory); scf_patch_extract reads those records on the device, so nothing passes through the host.  frames is
 * (F,frame_h,frame_w,3) uint8, frame_index (N) int32 selects each object's frame (outside [0, F): all-pad_val patch).
 * --------------------------------------------------------------------------------- */
typedef struct scf_patch_params {
  double aspect_ratio;           /* Crop aspect_ratio (> 0), read when keep_ratio == 0                */
  double size_ratio;             /* Crop size_range, both ends (> 0)                                  */
  double min_expand;             /* Crop min_expand (>= 0)                                            */
  int32_t out_h, out_w;          /* Pad size, 1..8192 each                                            */
  int32_t resize;                /* Resize img_scale: longer side of the resized patch, 1..min(out_h, out_w) */
  int32_t vertex_stride;         /* the box takes every vertex_stride-th vertex (>= 1)                */
  int32_t keep_ratio;            /* Crop keep_ratio                                                   */
  int32_t clip_border;           /* Crop clip_border                                                  */
  int32_t fix_clip_border_quirk; /* 0: lower edge y2 + bh/2 under clip_border, as the reference; 1: yc + bh/2 */
  int32_t center;                /* Pad center                                                        */
  int32_t to_rgb;                /* Normalize to_rgb                                                  */
  int32_t crop_pad_val[3];       /* Crop pad_val, 0..255, frame channel order                         */
  int32_t pad_val[3];            /* Pad pad_val['img'], 0..255, frame channel order                   */
  float mean[3];                 /* Normalize mean / std in grey levels, output channel order; std != 0 */
  float std[3];
} scf_patch_params;
/* bytes of workspace (the per-object records) scf_patch_boxes writes and scf_patch_extract reads, or SCF_EINVAL */
int64_t scf_patch_workspace_bytes(int N);
int scf_patch_boxes(const scf_mesh_store* mesh, const int32_t* labels, const float* R, const float* t,
                    const float* K, const int32_t* crop_in, int N, int frame_h, int frame_w,
                    const scf_patch_params* params, float* box, int32_t* crop, float* scale, float* transform_matrix,
                    float* k, int32_t* valid, void* workspace, scf_stream_t stream);
int scf_patch_extract(const uint8_t* frames, int F, int frame_h, int frame_w, const int32_t* frame_index, int N,
                      const void* workspace, const scf_patch_params* params, float* out, scf_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Train patches.                     replaces the train_pipeline of configs/refine_datasets/ycbv_real.py (LoadMasks,
 *                                    PoseJitter, ComputeBbox, Crop(size_range=(lo, hi)), RandomHSV, RandomNoise,
 *                                    RandomSmooth, Resize, Pad, RemapPose(keep_intrinsic=False), Normalize).
 * Added without a version bump (SCF_VERSION stays at .3): the presence of scf_pose_jitter, scf_patch_boxes_train,
 * scf_patch_extract_train, scf_patch_train_workspace_bytes and scf_patch_train_route marks the feature.
 * patch_train.hip states the semantics in full (cv2 parity is not claimed); in short:
 *   random     counter-based: every draw is hash(seed, sample_id, stream, counter) (splitmix64 finaliser), sample_id =
 *              id_base + n or sample_ids[n] (int64, device; may be NULL): an object's draws do not depend on its batch.
 *   jitter     up to max_tries tries of dR = Rx(a2) Ry(a1) Rz(a0) (degrees, N(jitter_angle)), noise N(jitter_x/y/z), in
 *              fp64; R_ref = dR R_gt, t_ref = t_gt + noise; a try is rejected when its rotation error (degrees),
 *              |noise| or ADD / diameter exceeds its limit (a negative limit = none).  No accepted try, a label outside
 *              the mesh store, or an empty class under add_limit: the gt pose, errors 0, ok = 0.  mesh may be NULL
 *              without add_limit (add_error is then NaN); diameters is (num_classes) fp32 on the device.
 *              rot_error holds |noise| and trans_error the angle, as the reference's init_rot_error /
 *              init_trans_error do, unless fix_error_swap_quirk is set.
 *   boxes      scf_patch_boxes with size_ratio drawn per object from size_range; also draws the colour augmentation
 *              and writes draws (N,8) fp64 = (size_ratio, h gain, s gain, v gain, sigma, k, hsv on, noise on).
 *              workspace: scf_patch_train_workspace_bytes(N) bytes; its first scf_patch_workspace_bytes(N) bytes are
 *              the records scf_patch_extract reads.
 *   extract    scf_patch_extract with RandomHSV, RandomNoise and RandomSmooth applied to the crop patch before the
 *              resize, and the object's mask: masks (N,frame_h,frame_w) uint8, nonzero = object, cropped with fill 0,
 *              resized to nearest, padded with mask_pad_val -> mask_out (N,out_h,out_w) bytes 0 / 1.  masks and
 *              mask_out are both NULL or both given.
 *   route      scf_patch_train_route(ph, pw, new_h, new_w, k) = 0 when an object of that crop size, resized size and
 *              smoothing kernel runs from LDS, 1 when its threads read the frame directly (same bits), SCF_EINVAL
 *              for bad arguments.  A host function: the kernel's own formula.
 * --------------------------------------------------------------------------------- */
typedef struct scf_patch_aug_params {
  uint64_t seed;
  double jitter_angle[2];        /* PoseJitter jitter_angle_dis: mean, std in degrees (std >= 0)       */
  double jitter_x[2], jitter_y[2], jitter_z[2];
  double angle_limit;            /* degrees; negative: none                                            */
  double translation_limit;      /* negative: none                                                     */
  double add_limit;              /* in diameters; negative: none                                       */
  double size_range[2];          /* Crop size_range, 0 < lo <= hi                                      */
  double hsv_ratio[3];           /* RandomHSV h_ratio, s_ratio, v_ratio, each in [0, 1)                */
  double hsv_p, noise_p, smooth_p; /* the transforms' p in [0, 1]; 0 switches one off                  */
  double noise_ratio;            /* RandomNoise noise_ratio (>= 0)                                     */
  int32_t max_tries;             /* 1..4096                                                            */
  int32_t max_kernel_size;       /* RandomSmooth max_kernel_size, 1..15: k is drawn from the reference's list
                                    {1, 3, .., 2 (max_kernel_size / 2) + 1}, so an even value also draws
                                    max_kernel_size + 1 (4 gives {1, 3, 5}; color_transform.py:125)     */
  int32_t fix_error_swap_quirk;  /* 0: rot_error / trans_error swapped, as the reference; 1: as named  */
  int32_t mask_pad_val;          /* Pad pad_val['mask']: 0 or not                                      */
} scf_patch_aug_params;
int scf_pose_jitter(const scf_mesh_store* mesh, const float* diameters, const int32_t* labels, const float* R_gt,
                    const float* t_gt, int N, int vertex_stride, const scf_patch_aug_params* aug, int64_t id_base,
                    const int64_t* sample_ids, float* R_ref, float* t_ref, float* add_error, float* rot_error,
                    float* trans_error, int32_t* ok, int32_t* tries, scf_stream_t stream);
int64_t scf_patch_train_workspace_bytes(int N);
int scf_patch_train_route(int ph, int pw, int new_h, int new_w, int k);
int scf_patch_boxes_train(const scf_mesh_store* mesh, const int32_t* labels, const float* R, const float* t,
                          const float* K, const int32_t* crop_in, int N, int frame_h, int frame_w,
                          const scf_patch_params* params, const scf_patch_aug_params* aug, int64_t id_base,
                          const int64_t* sample_ids, double* draws, float* box, int32_t* crop, float* scale,
                          float* transform_matrix, float* k, int32_t* valid, void* workspace, scf_stream_t stream);
int scf_patch_extract_train(const uint8_t* frames, int F, int frame_h, int frame_w, const int32_t* frame_index,
                            const uint8_t* masks, int N, const void* workspace, const scf_patch_params* params,
                            const scf_patch_aug_params* aug, float* out, uint8_t* mask_out, scf_stream_t stream);

/* filter_flow_by_mask (models/utils/flow.py:6-26), in place on flow (N,2,H,W): a vector is set
 * to invalid_num when both components are >= invalid_num or when mask (N,H,W), sampled
 * bilinearly (zeros padding) at the vector's end point, is < 0.9.  The end point is normalised
 * with (size-1) (coords_grid, warp.py:9-29) and de-normalised per align_corners, as the
 * reference does (its default align_corners=0 therefore samples at (x+fx)*W/(W-1) - 0.5). */
int scf_filter_flow_by_mask(float* flow, const float* mask, int N, int H, int W,
                            float invalid_num, int align_corners, scf_stream_t stream);

/* cal_epe (models/utils/flow.py:64-88), all three reductions from one pass over flow_tgt / flow_pred
 * (N,2,H,W) and the optional mask (N,H,W; NULL = none):
 *   valid = sqrt(tgt_x^2 + tgt_y^2) < max_flow [&& mask >= 0.5],  err = |flow_tgt - flow_pred|_2
 *   err_map      (N,H,W) or NULL      reduction='none':  err * valid
 *   mean, ratios (N), (nthr,N) / NULL reduction='mean':  sum(err * valid) / (count(valid) + 1e-10) per sample;
 *                                     ratios[t][n] = count(err < threshs[t] among the INVALID pixels) / that
 *                                     total -- the reference overwrites the valid pixels with 1e8 before the
 *                                     comparison (flow.py:79), reproduced as-is; fix_threshold_quirk != 0
 *                                     counts the valid pixels instead
 *   total_mean, total_ratios (1), (nthr) / NULL   reduction='total_mean': the same over the whole batch,
 *                                     ratios over the valid pixels (flow.py:84-87)
 * threshs is a HOST array of nthr <= 8 thresholds.  Squares, adds and square roots are separately rounded
 * fp32 operations as in torch; error sums are accumulated in fp64 in a fixed order and rounded once.
 * workspace: scf_cal_epe_workspace_bytes(N, H, W) bytes of device memory (block partials). */
int64_t scf_cal_epe_workspace_bytes(int N, int H, int W);
int scf_cal_epe(const float* flow_tgt, const float* flow_pred, const float* mask, int N, int H, int W,
                float max_flow, const float* threshs, int nthr, int fix_threshold_quirk, float* err_map,
                float* mean, float* ratios, float* total_mean, float* total_ratios, void* workspace,
                scf_stream_t stream);

/* Forward values of the supervised losses (models/loss/sequence_loss.py, point_matching_loss.py) for all T iterations
 * of a prediction sequence; the *_grad entries further down add the gradients.  Every sequence is a HOST array of T device pointers, T <= 256 (32 travel
 * per launch; longer sequences take several launches inside the call).  Sums are accumulated in fp64 in a fixed
 * order and rounded to fp32 once; there are no atomics, so results are bitwise reproducible.
 *
 * scf_seq_pixel_loss: SequenceLoss over RAFTLoss for up to two flow sequences (flow_a, flow_b: (N,2,H,W) each, NULL =
 * none) and over L1Loss for one mask sequence (mask_seq: (N,H,W) each, NULL = none) against gt_flow (N,2,H,W) and the
 * optional valid (N,H,W), which are read once per pixel:
 *   mag = sqrt(gx*gx + gy*gy) (three fp32 roundings),  v = (valid >= 0.5) && (mag < max_flow)   [mag < max_flow alone]
 *   flow value_i = loss_weight * (float)sum(v*|px-gx| + v*|py-gy|) / ((float)count(v) + eps)    (NaN * 0 stays NaN)
 *   mask value_i = ((float)sum|m - occ| / (float)(N*H*W)) * loss_weight,   occ = mask_gt (N,H,W), or, when mask_gt is
 *                  NULL, (gx + gy < max_flow).  gt_flow may be NULL when only a mask sequence against mask_gt is given.
 * The derived occ compares the SUM of the two channels, not the magnitude, and the mask loss ignores valid: both are the
 * reference's (scflow_refiner.py:230, sequence_loss.py:35-37), restated as they are.
 * loss_weight, eps, gamma: HOST arrays of 3 (rows flow_a, flow_b, mask_seq; eps[2] is unused).
 * per_iter (3,T): the values above, 0 in the rows of absent sequences; totals (3): sum_i (float)(gamma^(T-1-i)) *
 * value_i, added in fp32 in ascending i from 0.
 * workspace: scf_seq_pixel_loss_workspace_bytes(N, H, W, T) bytes of device memory. */
int64_t scf_seq_pixel_loss_workspace_bytes(int N, int H, int W, int T);
int scf_seq_pixel_loss(const float* gt_flow, const float* valid, const float* mask_gt, const float* const* flow_a,
                       const float* const* flow_b, const float* const* mask_seq, int T, int N, int H, int W,
                       float max_flow, const float* loss_weight, const float* eps, const double* gamma,
                       float* per_iter, float* totals, void* workspace, scf_stream_t stream);

/* scf_point_matching_loss: PointMatchingLoss (SCF_PM_FULL), DisentanglePointMatchingLoss (SCF_PM_DISENTANGLE) and
 * RotPointMatchingLoss (SCF_PM_ROT; pred_t, gt_t, scale_factors unused).
 * Points: verts (total,3) holds num_groups point sets, set g = rows [offsets[g], offsets[g+1]); sample n uses set
 * group[n] (its class for class meshes -- the layout of scf_mesh_store -- or n for per-sample point lists).
 * labels (N) index symmetric (num_classes; != 0: each ground-truth-posed point is compared with its squared-L2 NEAREST
 * predicted-posed point, lowest index on exact ties, whatever loss_type is) and diameter (num_classes).
 * A group or label outside its table makes that sample's value NaN and reads nothing.
 *   t' = (t.xy * s if SCF_PM_SCALE_XY,  t.z * s * scale_depth_factor if SCF_PM_SCALE_DEPTH else t.z * scale_depth_factor)
 *   FULL         mean_p |(R_pred p + t_pred') - (R_gt p + t_gt')|
 *   DISENTANGLE  mean_p |(R_pred p + t_gt') - (R_gt p + t_gt')| + the translation term mean_p |(R_gt p + t_pred') -
 *                (R_gt p + t_gt')|, or with SCF_PM_DISENTANGLE_Z the depth term (t_gt'.xy, t_pred'.z) plus the xy term
 *                (t_pred'.xy, t_gt'.z), each built per point as written
 *   ROT          mean_p |R_pred p - R_gt p|
 * | | is the L1 (loss_type 1) or L2 (2) norm.  loss_i (T,N) = that / diameter[label]; per_iter (T) = loss_weight *
 * (sum_n loss_i in sample order [/ N for SCF_PM_REDUCE_MEAN]); total (1) = sum_i (float)(gamma^(T-1-i)) * per_iter_i.
 * nn_idx (T,N,max_points) int32 or NULL: the index compared with each point (its own for non-symmetric classes);
 * entries past a sample's point count are left untouched.  max_points >= the largest point set in use.
 * workspace: scf_point_matching_workspace_bytes(N, T, max_points) bytes of device memory. */
#define SCF_PM_FULL 0
#define SCF_PM_DISENTANGLE 1
#define SCF_PM_ROT 2
#define SCF_PM_DISENTANGLE_Z 1
#define SCF_PM_SCALE_XY 2
#define SCF_PM_SCALE_DEPTH 4
#define SCF_PM_REDUCE_MEAN 0
#define SCF_PM_REDUCE_SUM 1
int64_t scf_point_matching_workspace_bytes(int N, int T, int max_points);
int scf_point_matching_loss(const float* verts, const int32_t* offsets, int num_groups, const int32_t* group,
                            const int32_t* labels, int num_classes, const int32_t* symmetric, const float* diameter,
                            const float* const* pred_r, const float* const* pred_t, int T, const float* gt_r,
                            const float* gt_t, const float* scale_factors, int N, int max_points, int mode,
                            int loss_type, int flags, float scale_depth_factor, int reduction, float loss_weight,
                            double gamma, float* loss_i, float* per_iter, float* total, int32_t* nn_idx,
                            void* workspace, scf_stream_t stream);

/* Value AND gradient of the supervised losses: each entry takes the arguments of the forward entry above it is named
 * after and returns the same values bit for bit (same pixel-to-thread mapping, same reduction tree), plus the derivative
 * of  sum_row upstream[row] * total[row]  with respect to every prediction, from the same pass over the predictions and
 * the same neighbour search.  The gamma weight w_i = (float)(gamma^(T-1-i)) of iteration i is therefore included.
 * upstream: DEVICE pointer to fp32 scalars (3 for the pixel entry, one per row; 1 for point matching), NULL = 1, so
 * that a 0-dim grad_output is passed on without a host sync.  No gradient goes to ground truths, meshes or scales.
 *
 * scf_seq_pixel_loss_grad: grad_a, grad_b (N,2,H,W each) and grad_mask (N,H,W each) are HOST arrays of T device
 * pointers; any of them may be NULL (that sequence gets no gradient).
 *   flow  g = c_i * v * sgn(p - q),  c_i = ((upstream * w_i) * loss_weight) / ((float)count(v) + eps) in fp32, v the
 *         forward's own decision;  mask  g = ((upstream * w_i) * loss_weight) / (float)(N*H*W) * sgn(m - occ); valid is
 *         ignored by the mask gradient as by its value.
 *   sgn compares its two operands: 0 when equal, +-1 for +-inf, NaN when either is NaN -- also where v = 0 (0 * NaN).
 *   count(v) = 0: every flow gradient is 0 for eps > 0 and NaN (0 * inf) for eps = 0.
 * count(v) comes from a pre-pass over gt_flow / valid; the predictions are read once and the gradients written once.
 * Loads take the quad route by the alignment rule of the forward entry; the stores take it when, in addition, every
 * gradient plane is 16-byte aligned.  Either way the bits are the same.
 * workspace: scf_seq_pixel_loss_grad_workspace_bytes(N, H, W, T) bytes of device memory. */
int64_t scf_seq_pixel_loss_grad_workspace_bytes(int N, int H, int W, int T);
int scf_seq_pixel_loss_grad(const float* gt_flow, const float* valid, const float* mask_gt, const float* const* flow_a,
                            const float* const* flow_b, const float* const* mask_seq, int T, int N, int H, int W,
                            float max_flow, const float* loss_weight, const float* eps, const double* gamma,
                            const float* upstream, float* const* grad_a, float* const* grad_b, float* const* grad_mask,
                            float* per_iter, float* totals, void* workspace, scf_stream_t stream);

/* scf_point_matching_loss_grad: grad_r (T pointers to (N,3,3)) and grad_t (T pointers to (N,3); NULL for SCF_PM_ROT)
 * are HOST arrays of device pointers; either may be NULL.  With d_p = pred_point[idx_p] - target_p in the bits the
 * forward normed, u_p = d_p / |d_p| (0 where |d_p| = 0) for L2 and sgn(d_p) per component for L1, the neighbour index a
 * constant, and k = upstream * w_i * loss_weight / (V * diameter[label]) [/ N for SCF_PM_REDUCE_MEAN]:
 *   FULL         grad_R = k sum_p u_p (x) verts[idx_p]  (the model point of the NEIGHBOUR),  grad_t' = k sum_p u_p
 *   DISENTANGLE  grad_R from the rotation term; grad_t' from the translation term, or with SCF_PM_DISENTANGLE_Z its z
 *                from the depth term and its xy from the xy term (structurally zero components are exact zeros)
 *   ROT          grad_R only
 *   grad_t.xy = s * grad_t'.xy under SCF_PM_SCALE_XY;  grad_t.z = s * factor * grad_t'.z under SCF_PM_SCALE_DEPTH, else
 *   factor * grad_t'.z.
 * u and its product with the coordinate are fp32; the 9 + 3 sums go through the fixed-order fp64 reduction of the
 * values and are scaled by k in fp64 and rounded once.  A group or label out of range gives NaN gradients for that
 * sample and reads nothing; an empty point set gives NaN as it does for the value.
 * workspace: scf_point_matching_grad_workspace_bytes(N, T, max_points) bytes of device memory. */
int64_t scf_point_matching_grad_workspace_bytes(int N, int T, int max_points);
int scf_point_matching_loss_grad(const float* verts, const int32_t* offsets, int num_groups, const int32_t* group,
                                 const int32_t* labels, int num_classes, const int32_t* symmetric, const float* diameter,
                                 const float* const* pred_r, const float* const* pred_t, int T, const float* gt_r,
                                 const float* gt_t, const float* scale_factors, int N, int max_points, int mode,
                                 int loss_type, int flags, float scale_depth_factor, int reduction, float loss_weight,
                                 double gamma, const float* upstream, float* const* grad_r, float* const* grad_t,
                                 float* loss_i, float* per_iter, float* total, int32_t* nn_idx, void* workspace,
                                 scf_stream_t stream);

/* object-frame points of every pixel (dense cal_3d_2d_corr): pts (N,3,H,W), 0 where
 * depth <= 0.  Test/diagnostic entry; scf_reproject_flow recomputes them on the fly. */
int scf_unproject_depth(const float* depth, const float* K, const float* R0, const float* t0,
                        float* pts, int N, int H, int W, scf_stream_t stream);

/* out = mul * bilinear_resize(a + b?) with align_corners=True (F.interpolate semantics,
 * scflow_decoder.py:188-197, 222-227).  a, b: (planes, Hin, Win); out (planes, Hout, Wout) */
int scf_resize_bilinear(const float* a, const float* b, float* out, int64_t planes, int Hin,
                        int Win, int Hout, int Wout, float mul, scf_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Backward of the parameter-free tail of an SCFlow iteration (scflow_decoder.py:222-249): the vector-Jacobian product
 * that takes d loss / d (flow_from_pose, flow_from_pred, rotation, translation, up-sampled mask) of every iteration to
 * d loss / d (delta_flow, mask, delta_rotation, delta_translation).  Every entry takes the T <= SCF_TAIL_MAX_T
 * iterations as HOST arrays of device pointers and is one launch; none allocates, synchronises or reads back; no
 * entry uses atomics, and every sum has one order fixed by the geometry, so results are bit-identical from run to run
 * and do not depend on how many iterations share a call.
 * Added without a version bump (SCF_VERSION stays at .3), as the renderer's and the losses' entries were: the presence of
 * scf_pose_tail_grad marks the feature.
 * --------------------------------------------------------------------------------- */
#define SCF_TAIL_MAX_T 32
#define SCF_TAIL_DETACH_POSE 1            /* detach_pose: no gradient from iteration i into the pose of iteration i - 1 */
#define SCF_TAIL_DETACH_DEPTH_FOR_XY 2    /* detach_depth_for_xy (pose.py:142-147): v_z is a constant in v_x, v_y */

/* Adjoint of scf_resize_bilinear for the same (Hin, Win, Hout, Wout):  out[t] (planes, Hin, Win) = mul * U^T (g[t] +
 * g_add[t]?) with g[t] (planes, Hout, Wout) and U the forward's interpolation matrix, its coordinate fl(fl(scale) *
 * index) and its weights l = f - i0, 1 - l included; the clamped +1 tap at the last row / column puts both weights
 * on the same node.  accumulate != 0: out[t] += instead of =.  g_add may be NULL, and so may any of its entries.
 * A second job of the same geometry (g1, out1, planes1, mul1, accumulate1; planes1 = 0: none) rides in the launch:
 * the flow planes and the mask planes of a pass.
 * Order of the sums (fp32, no contraction): per input node, rows ascending of  wy * (quads of four output columns
 * ascending of (columns ascending of wx * g)); see tail_grad.hip.  Two kernels produce these bits: a workgroup-per-plane
 * walk with 16-byte loads when Wout % 4 == 0, every g[t] / g1[t] is 16-byte aligned, there is no g_add and the x scale
 * is <= 1/4 (the x8 up-sampling of the decoder), and a thread-per-node gather otherwise. */
int scf_resize_bilinear_grad(const float* const* g, const float* const* g_add, float* const* out, int64_t planes, float mul,
                             int accumulate, const float* const* g1, float* const* out1, int64_t planes1, float mul1,
                             int accumulate1, int T, int Hin, int Win, int Hout, int Wout, scf_stream_t stream);

/* Re-projection sums of scf_reproject_flow's backward: for iteration i and sample n, over the pixels the forward
 * treats as foreground (depth > 0; NaN is background), with P and q = K (R_i P + t_i) recomputed as the forward does,
 *   g_q = (gu / qz, gv / qz, -(gu qx + gv qy) / qz^2),  g_p = K^T g_q   (fp32),
 *   words [0, 9) = sum g_p (x) P  (row-major: d / dR_i),  words [9, 12) = sum g_p  (d / dt_i)   (fp64, fixed order).
 * g_flow[i] (N,2,H,W) may be NULL: exact zeros, as for a sample without foreground.  The workspace receives
 * (T, N, tiles, 12) doubles, tiles = workspace_bytes / (T * N * 96): per-block partial sums that scf_pose_tail_grad
 * (or the caller) adds in ascending tile order.  scf_tail_grad_workspace_bytes(N, H, W, T) bytes of device memory. */
int64_t scf_tail_grad_workspace_bytes(int N, int H, int W, int T);
int scf_reproject_flow_grad(const float* depth, const float* K, const float* R0, const float* t0, const float* const* R,
                            const float* const* t, const float* const* g_flow, int T, int N, int H, int W, void* workspace,
                            scf_stream_t stream);

/* Reverse scan over the pose updates  R_i = Rd(d_rot_i) R_{i-1},  t_i = compose(d_trans_i, t_{i-1})  (scf_pose_update
 * on the selected rows; R_{-1} = R0, t_{-1} = t0 get no gradient), one thread per sample, i = T-1 .. 0:
 *   G = g_R[i] | g_t[i]  +  the re-projection sums of iteration i  +  carry
 *   g_d_rot[i]   = ortho6d backward of  G_R R_{i-1}^T  (F.normalize's backward: through the norm only where it is
 *                  not clamped at 1e-12)
 *   g_d_trans[i] = backward of the compose, for both depth transforms (label_mode & SCF_POSE_DEPTH_LINEAR)
 *   carry        = (Rd^T G_R, (d t_i / d t_{i-1})^T G_t), or 0 under SCF_TAIL_DETACH_POSE.
 * Evaluated in fp64 from the fp32 values the forward stored (d_rot[i] (N,6), d_trans[i] (N,3), R[i] (N,3,3), t[i] (N,3):
 * entry i - 1 is the input of iteration i; entry T - 1 is not read); each output is rounded to fp32 once.
 * g_R, g_t: NULL, or arrays whose entries may be NULL.  reproject_sums: NULL, or the workspace scf_reproject_flow_grad
 * wrote for the same (T, N, H, W). */
int scf_pose_tail_grad(const float* const* d_rot, const float* const* d_trans, const float* R0, const float* t0,
                       const float* const* R, const float* const* t, const float* const* g_R, const float* const* g_t,
                       const void* reproject_sums, int H, int W, int flags, int label_mode, float* const* g_d_rot,
                       float* const* g_d_trans, int T, int N, scf_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Backward of the pose head's fully connected tail (pose_head.py:151-172, 201-211): from d loss / d (delta_rotation,
 * delta_translation) to d loss / d (raw output of the last convolution) and to the gradients of fc1, fc2, the two heads
 * and the last GroupNorm's affine.  The weights are shared by the T iterations of a pass: the caller stacks the
 * iterations, M = T N rows (row m = iteration m / N, sample m % N), and every entry is one launch over all of them
 * (scf_group_norm_flat_grad: two).  None allocates, synchronises or reads back; none uses atomics; every sum has one
 * order fixed by the shapes (fc_grad.hip), so results are bit-identical from run to run.  ReLU masks are `a > 0` on the
 * activations the forward computed: a NaN activation is 0 (the forward's fmaxf / v > 0 ? v : 0) and passes no gradient.
 * Added without a version bump; the presence of scf_fc_dgrad marks the feature.
 * --------------------------------------------------------------------------------- */

/* The operand an scf_fc_splitk launch contracted, as a finished (M, K) matrix in the launch's own bits: the in-order
 * sum of `parts` tensors part_stride floats apart, + x_bias (may be NULL), ReLU if x_relu; gn_groups > 0: then
 * GroupNorm(gn_groups, gn_eps, affine) + ReLU over groups of K / gn_groups (even) consecutive features, channel of
 * feature k = k / gn_hw, in the arithmetic and operation order of the forward's fold. */
int scf_fc_operand(const float* x, int parts, int64_t part_stride, const float* x_bias, int x_relu, int gn_groups,
                   int gn_hw, const float* gn_gamma, const float* gn_beta, float gn_eps, float* out, int M, int K,
                   scf_stream_t stream);

/* rotation_pred | translation_pred and the class selection, backward.  Class of row m: label[0], or label[m % N] under
 * SCF_POSE_LABEL_PER_SAMPLE, clamped as scf_pose_update clamps it.  g_rot (M, 6), g_trans (M, 3), Wr (6 num_class, K),
 * Wt (3 num_class, K), a (M, K): the heads' input (fc2's activation).
 *   g_s (M, K) = (g_rot . Wr[6c : 6c + 6] + g_trans . Wt[3c : 3c + 3]) * [a > 0]   (a NULL: no mask; g_s NULL: skipped)
 *   dWr[6c + r] = sum over the rows of class c, ascending, of g_rot[m][r] a[m],  dbr[6c + r] = sum g_rot[m][r], and the
 *   same for dWt / dbt (all four or none).  Rows of classes no row selected: exact zeros, or untouched under accumulate.
 * Plain fp32, no contraction: nine products added in the order r = 0..5 (rotation), 0..2 (translation). */
int scf_pose_select_grad(const float* g_rot, const float* g_trans, const float* Wr, const float* Wt, const float* a,
                         const int64_t* label, int N, int num_class, int label_mode, float* g_s, float* dWr,
                         float* dbr, float* dWt, float* dbt, int accumulate, int M, int K, scf_stream_t stream);

/* g_s (M, K) = (g (M, O) . W (O, K)) * [a > 0]  (a (M, K), NULL: no mask): nn.Linear's input gradient, W row-major
 * (O, K) like nn.Linear.weight, contracted over O on the matrix cores in one fma chain per output, o ascending.  A
 * row of g_s depends on that row of g (and of a) alone, whatever M is. */
int scf_fc_dgrad(const float* g, const float* W, const float* a, float* g_s, int M, int O, int K, scf_stream_t stream);

/* dW (O, K) = sum_m g[m][o] a[m][k],  db (O) = sum_m g[m][o] (db may be NULL): nn.Linear's parameter gradients,
 * contracted over the M rows on the matrix cores.  Rows go in ascending chunks of 32: a chunk's chain starts at +0, the
 * chunk partials are added in ascending order.  accumulate != 0: the sum is added to what dW / db hold. */
int scf_fc_wgrad(const float* g, const float* a, float* dW, float* db, int M, int O, int K, int accumulate,
                 scf_stream_t stream);

/* GroupNorm(groups, eps, affine) + ReLU on the flattened (C, hw) map, backward.  y: the raw input in parts form (as
 * scf_fc_operand's x), x0 (M, K): the forward's output (the mask is x0 > 0), g_x0 (M, K).  With mean, rstd recomputed
 * from y in fp32 (two passes), xh = (y - mean) rstd, g_u = g_x0 [x0 > 0], t = gamma[k / hw] g_u:
 *   g_y = rstd (t - mean_g(t) - xh mean_g(t xh)),   dbeta[c] = sum g_u,   dgamma[c] = sum g_u xh   over rows and hw
 * (dgamma / dbeta: both or neither; accumulate as above).  K % groups == 0, K / groups even, any hw.
 * stats: 2 M groups floats of device memory (mean, rstd per row and group; written, then read by the parameter pass). */
int scf_group_norm_flat_grad(const float* g_x0, const float* y, int y_parts, int64_t y_part_stride, const float* x0,
                             const float* gamma, int groups, int hw, float eps, float* g_y, float* dgamma,
                             float* dbeta, int accumulate, float* stats, int M, int K, scf_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Backward of the pose head's convolutions (pose_head.py:131-149: three 3x3 / stride-2 / pad-1 ConvModules without bias):
 * the input gradient and the weight gradient of one layer, fp32 on v_mfma_f32_32x32x2_f32.  The weights are shared by the
 * T iterations of a pass: the caller stacks them, M = T N samples, and dgrad is one launch over all of them, wgrad two
 * (the second combines the partial sums).  Neither allocates, synchronises or reads back; neither uses atomics; every sum
 * has one order fixed by the shapes (conv_grad.hip), so results are bit-identical from run to run.
 * Geometry: KH = KW = 3, stride 2, pad 1, any Hin, Win >= 1 with Ho = (Hin - 1) / 2 + 1, Wo = (Win - 1) / 2 + 1; another
 * kernel, stride or padding: SCF_EUNSUPPORTED; sizes that do not belong together, a missing pointer: SCF_EINVAL; both with
 * nothing launched.  w and dW are the raw (Cout, C0 + C1, 3, 3) parameter in the torch layout, not a packed weight.
 * Added without a version bump; the presence of scf_conv_dgrad marks the feature.
 * --------------------------------------------------------------------------------- */

/* g (M, Cout, Ho, Wo) -> the input gradient, written whole as two dense tensors gx0 (M, C0, Hin, Win) and gx1 (M, C1,
 * Hin, Win), the two parts the forward read (gx1 NULL <=> C1 = 0).  Only the taps that meet an output pixel are
 * computed (1, 2, 2 or 4 of the 9, by the parity of (iy, ix)): 9 Cout Cin multiply-adds per 2 x 2 input pixels.  Per
 * element ONE fma chain from +0: the contributing taps in ascending (ky, kx), inside a tap co ascending (padded with
 * zeros to a multiple of 32; a tap that leaves the output map at the far border of an even-sized input contributes
 * zeros).  A sample's result depends on that sample alone, whatever M is. */
int scf_conv_dgrad(const float* g, const float* w, float* gx0, int C0, float* gx1, int C1, int M, int Cout, int Ho,
                   int Wo, int Hin, int Win, int KH, int KW, int stride, int pad, scf_stream_t stream);

/* dW[co][ci][ky][kx] = sum_{m, oy, ox} g[m, co, oy, ox] x[m, ci, 2 oy - 1 + ky, 2 ox - 1 + kx]  (zero outside the map), x
 * in two parts x0 (M, C0, Hin, Win), x1 (M, C1, Hin, Win) (x1 NULL <=> C1 = 0).  The contraction over the M Ho Wo output
 * pixels, (m, oy, ox) row-major, is cut into S splits of consecutive pixels (conv_grad.hip: cg_wgrad_plan); a split is
 * ONE fma chain from +0 per element, pixels ascending, written to workspace[s][tap][co][ci]; the second launch takes
 * partial 0, adds partials 1 .. S - 1 in ascending order and, with accumulate != 0, the previous value of dW last.
 * workspace: scf_conv_wgrad_workspace(M, Cout, C0 + C1, Ho, Wo) floats of device memory (-1: invalid sizes); fewer:
 * SCF_EINVAL.  The pose head's convolutions have no bias, so there is no bias gradient. */
int64_t scf_conv_wgrad_workspace(int M, int Cout, int Cin, int Ho, int Wo);
int scf_conv_wgrad(const float* g, const float* x0, int C0, const float* x1, int C1, float* dW, int accumulate,
                   float* workspace, int64_t workspace_floats, int M, int Cout, int Ho, int Wo, int Hin, int Win, int KH,
                   int KW, int stride, int pad, scf_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Backward of a stride-1, same-padding convolution with bias (scflow_decoder.py:210-217: the XHeads and the delta-flow /
 * mask encoders; the family also covers the GRU's 1x5 / 5x1 gates and the motion encoder's layers): input gradient with
 * a fused second cotangent and activation backward, weight + bias gradient, and the elementwise activation backward.
 * fp32; no atomics, allocation, synchronisation or read-back; every sum has one order fixed by the shapes
 * (conv_s1_grad.hip), so results are bit-identical from run to run.
 * Geometry: stride 1, pad = (KH / 2, KW / 2), KH and KW each in {1, 3, 5, 7}, any H, W >= 1; an even or larger kernel:
 * SCF_EUNSUPPORTED; a null required pointer, a non-positive size, an unknown act, act != NONE without a, a sample stride
 * smaller than C H W: SCF_EINVAL; all with nothing launched or written.  Sample strides are in elements, so a channel
 * slice of a wider tensor is an operand.  w / dW are the raw (Cout, Cin, KH, KW) parameter in the torch layout.
 * Route: min(Cout, Cin) >= 32 runs on v_mfma_f32_32x32x2_f32, everything else on the vector ALU; a function of
 * (Cout, Cin) only.  Added without a version bump; the presence of scf_conv_s1_dgrad marks the feature.
 * --------------------------------------------------------------------------------- */

/* out[m, i] = g[m, i] act'(a[m, i]), i < n: RELU a > 0 ? g : +0, SIGMOID g (a (1 - a)), TANH g fma(-a, a, 1), NONE g;
 * a: the forward's post-activation value (required exactly when act != SCF_ACT_NONE). */
int scf_act_grad(const float* g, int64_t g_stride, const float* a, int64_t a_stride, int act, float* out,
                 int64_t out_stride, int M, int64_t n, scf_stream_t stream);

/* gx[m, ci, iy, ix] = act'(a) (sum_{ky, kx, co} g[m, co, iy + KH / 2 - ky, ix + KW / 2 - kx] w[co, ci, ky, kx] + add)
 * g (M, Cout, H, W), add / a / gx (M, Cin, H, W), each with its sample stride; add NULL: none.  Per element ONE fma chain
 * from +0, taps in ascending (ky, kx), inside a tap co ascending (MFMA route: padded with zeros to a multiple of 32, taps
 * outside the map contribute zeros; vector route: such taps are skipped); then + add, then the factor as scf_act_grad.
 * w_scratch: NULL, or KH KW Cout Cin floats of device memory: the MFMA route then reads w through a [tap][co][ci] copy
 * that a launch in front writes (same bits, coalesced loads); unused on the vector route.  A sample's result depends
 * on that sample alone, whatever M is. */
int scf_conv_s1_dgrad(const float* g, int64_t g_stride, const float* w, const float* add, int64_t add_stride,
                      const float* a, int64_t a_stride, int act, float* gx, int64_t gx_stride, float* w_scratch, int M,
                      int Cout, int Cin, int H, int W, int KH, int KW, scf_stream_t stream);

/* dW[co][ci][ky][kx] = sum_{m, y, x} g[m, co, y, x] x[m, ci, y - KH / 2 + ky, x - KW / 2 + kx]  (zero outside the map),
 * db[co] = sum_{m, y, x} g[m, co, y, x] from the same pass (db NULL: none).  The contraction is cut into S splits
 * (conv_s1_grad.hip: s1_wgrad_plan), a partial each in the workspace; the second launch takes partial 0, adds partials
 * 1 .. S - 1 in ascending order and, with accumulate != 0, the previous value of dW / db last.
 * workspace: scf_conv_s1_wgrad_workspace(...) floats of device memory (-1: invalid sizes or kernel); fewer: SCF_EINVAL. */
int64_t scf_conv_s1_wgrad_workspace(int M, int Cout, int Cin, int H, int W, int KH, int KW);
int scf_conv_s1_wgrad(const float* g, int64_t g_stride, const float* x, int64_t x_stride, float* dW, float* db,
                      int accumulate, float* workspace, int64_t workspace_floats, int M, int Cout, int Cin, int H, int W,
                      int KH, int KW, scf_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Backward of the context encoder's remaining layers (raft_encoder.py:286-314, resnet.py:14-94 with eval-mode BatchNorm;
 * encoder_grad.hip): the weight gradient of the thin-input 7x7 / stride-2 stem, the input and weight gradient of a
 * down-sampling block's 1x1 / stride-2 shortcut, a per-channel sum (the bias gradient scf_conv_wgrad lacks), and the
 * BatchNorm fold with its gradient.  fp32; no atomics, allocation, synchronisation or read-back; every sum has one order
 * fixed by the shapes (encoder_grad.hip), so results are bit-identical from run to run.  Half-size maps: Ho = (Hin - 1) / 2
 * + 1, Wo = (Win - 1) / 2 + 1, any Hin, Win >= 1.  A null required pointer, a non-positive size, maps that do not belong
 * together, an unknown act, act != NONE without a, a sample stride below C H W, a workspace that is too small: SCF_EINVAL;
 * a geometry that is not built: SCF_EUNSUPPORTED; both with nothing launched or written.  Sample strides are in elements.
 * w / dW are raw parameters in the torch layout.  Added without a version bump; the presence of scf_conv_stem_wgrad marks
 * the feature.
 * --------------------------------------------------------------------------------- */

/* dW[co][ci][ky][kx] = sum_{m, oy, ox} g[m, co, oy, ox] x[m, ci, 2 oy - 3 + ky, 2 ox - 3 + kx]  (zero outside the map),
 * db[co] = sum g (db NULL: none), of F.conv2d(x, w, b, stride=2, padding=3) with a 7x7 kernel and Cin <= 4 (another
 * kernel, stride or padding, the encoder's stride-1 stem of scale 1/4 included, or a wider input: SCF_EUNSUPPORTED).
 * g (M, Cout, Ho, Wo), x (M, Cin, Hin, Win).  A GEMM of Cout x 49 Cin on v_mfma_f32_32x32x2_f32 whose patch operand is
 * built from input rows staged in LDS.  Chunks (m, oy, segment of 16 output pixels) row-major are cut into S splits of
 * consecutive chunks; a split is ONE fma chain from +0 per element, chunks then pixels ascending (zeros in the padding
 * and past Wo), db one chain of plain adds in the same order; the second launch takes partial 0, adds partials 1 .. S - 1
 * in ascending order and, with accumulate != 0, the previous value of dW / db last.
 * workspace: scf_conv_stem_wgrad_workspace(...) floats of device memory (-1: invalid sizes). */
int64_t scf_conv_stem_wgrad_workspace(int M, int Cout, int Cin, int Ho, int Wo);
int scf_conv_stem_wgrad(const float* g, int64_t g_stride, const float* x, int64_t x_stride, float* dW, float* db,
                        int accumulate, float* workspace, int64_t workspace_floats, int M, int Cout, int Cin, int Ho,
                        int Wo, int Hin, int Win, int KH, int KW, int stride, int pad, scf_stream_t stream);

/* The join at the input of a down-sampling block, whose 1x1 / stride-2 shortcut F.conv2d(x, w, stride=2) reads the even
 * pixels:  gx[m, ci, iy, ix] = act'(a) (add + [iy and ix even] sum_co g[m, co, iy / 2, ix / 2] w[co, ci])
 * g (M, Cout, Ho, Wo); w (Cout, Cin); add (the 3x3 / stride-2 layer's input gradient; NULL: none), a, gx (M, Cin, Hin,
 * Win).  Per even pixel ONE fma chain from +0 over co ascending (padded with zeros to a multiple of 32), then + add, then
 * the factor as scf_act_grad; every other pixel gets act'(a) add.  A sample's result depends on that sample alone. */
int scf_conv_ds_dgrad(const float* g, int64_t g_stride, const float* w, const float* add, int64_t add_stride,
                      const float* a, int64_t a_stride, int act, float* gx, int64_t gx_stride, int M, int Cout, int Cin,
                      int Ho, int Wo, int Hin, int Win, scf_stream_t stream);

/* dW[co][ci] = sum_{m, oy, ox} g[m, co, oy, ox] x[m, ci, 2 oy, 2 ox], db[co] = sum g (db NULL: none).  Splits of
 * consecutive chunks (m, oy, segment of 16 output pixels), ONE fma chain from +0 per element inside a split, and the
 * combine launch, all as scf_conv_stem_wgrad.  workspace: scf_conv_ds_wgrad_workspace(...) floats. */
int64_t scf_conv_ds_wgrad_workspace(int M, int Cout, int Cin, int Ho, int Wo);
int scf_conv_ds_wgrad(const float* g, int64_t g_stride, const float* x, int64_t x_stride, float* dW, float* db,
                      int accumulate, float* workspace, int64_t workspace_floats, int M, int Cout, int Cin, int Ho, int Wo,
                      int Hin, int Win, scf_stream_t stream);

/* out[c] = sum_{m, i} g[m, c, i], g (M, C, n) with a sample stride: the bias gradient of a layer whose weight gradient
 * has none.  q = (m, i) row-major is cut into S splits of `per` elements (a multiple of 256); in a split thread t adds
 * q0 + t, q0 + t + 256, ... in one chain from +0, then the 256 values pairwise, v[t] += v[t + k] for k = 128, ..., 1;
 * the second launch adds the splits in ascending order, then with accumulate != 0 the previous value of out last.
 * workspace: scf_channel_sum_workspace(M, C, n) floats. */
int64_t scf_channel_sum_workspace(int M, int C, int64_t n);
int scf_channel_sum(const float* g, int64_t g_stride, float* out, int accumulate, float* workspace,
                    int64_t workspace_floats, int M, int C, int64_t n, scf_stream_t stream);

/* Eval-mode BatchNorm folded into the convolution in front: y = W' * x + b' with sd = sqrt(var + eps), s = gamma / sd
 * (one rounding each), W'[c] = s[c] W[c], b' = fma(s, b - mean, beta).  W, Wf (Cout, K) rows of K = Cin KH KW floats. */
int scf_bn_fold(const float* W, const float* b, const float* gamma, const float* beta, const float* mean, const float* var,
                float eps, float* Wf, float* bf, int Cout, int64_t K, scf_stream_t stream);

/* From the folded layer's gradients (dWf, dbf): dW = s dWf, db = s dbf, dbeta = dbf,
 * dgamma[c] = fma(b - mean, dbf, <W_c, dWf_c>) / sd.  <W_c, dWf_c> (= sum g (W * x)): lane l of the channel's wave runs one
 * fma chain from +0 over k = l, l + 64, ... (k the torch order of a row), then v[l] += v[l + j] for j = 32, 16, ..., 1.
 * accumulate != 0: the previous value of each of the four is added last.  The running statistics get no gradient.
 * A channel reads and writes its own rows only.  dW must not alias dWf. */
int scf_bn_unfold(const float* W, const float* b, const float* gamma, const float* mean, const float* var, float eps,
                  const float* dWf, const float* dbf, float* dW, float* db, float* dgamma, float* dbeta, int accumulate,
                  int Cout, int64_t K, scf_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Backward of scf_instance_norm / scf_instance_norm_res_norm (instance_norm_grad.hip): InstanceNorm2d(eps, affine =
 * False, biased variance, eps inside the root) as the feature encoder applies it.  Every operand is (planes, HW) dense.
 * Per plane, with u the raw convolution output, mean / rstd recomputed from u with the forward's partial sums in the
 * forward's order, xhat = (u - mean) rstd (one rounding each) and g' the cotangent at IN(u):
 *   S1 = sum g', S2 = sum g' xhat, m1 = S1 / HW, m2 = S2 / HW, du = ((g' - m1) - xhat m2) rstd    (one rounding each)
 * scf_instance_norm_grad, y == NULL and gp == NULL ("mid", relu(IN(u))): g' = g, which the consumer's dgrad epilogue has
 *   already masked.  y != NULL and gp != NULL ("tail", y = relu(IN(u) + r)): g' = y > 0 ? g : +0, written to gp (the
 *   shortcut's cotangent) as well.  Exactly one of y / gp NULL: SCF_EINVAL.
 * scf_instance_norm_res_norm_grad (y = relu(IN(u) + IN(r)), the down-sampling blocks): g' as in the tail form; du from
 *   u's statistics and S2, dr from r's own statistics and its own S2r = sum g' rhat; one g' and S1 for both.
 * The mask is always read from y, the forward's own bits (a NaN in y masks), never from a recomputed xhat.
 * Order: HW % 4 == 0, every pointer 16-byte aligned and HW <= 16384: the plane stays in registers, thread t of 256
 * owns the float4 t, t + 256, ...; a thread adds its float4 as (a + b) + (c + d) to one chain from +0, then the
 * workgroup's tree of the forward.  Other planes: four sweeps, HW % 4 == 0 aligned up to 81920 with 1024 threads
 * in the same float4 pattern, else thread t of 256 adds elements t, t + 256, ... in one chain.  No atomics, allocation
 * or synchronisation; bit-identical from run to run; a plane's result depends on that plane alone.  HW == 1 gives zeros.
 * Outputs may alias g element for element (du over g) and nothing else.
 * A null required pointer, planes <= 0 or HW <= 0: SCF_EINVAL; planes >= 2^31: SCF_EUNSUPPORTED; nothing launched or
 * written.  Added without a version bump; the presence of scf_instance_norm_grad marks the feature.
 * --------------------------------------------------------------------------------- */
int scf_instance_norm_grad(const float* g, const float* y, const float* u, float* gp, float* du, int64_t planes, int HW,
                           float eps, scf_stream_t stream);
int scf_instance_norm_res_norm_grad(const float* g, const float* y, const float* u, const float* r, float* du, float* dr,
                                    int64_t planes, int HW, float eps, scf_stream_t stream);

/* ---------------------------------------------------------------------------------
 * BatchNorm2d on the statistics of the batch, forward and backward (batch_norm_train.hip): affine, eps inside the root,
 * biased variance for normalising, unbiased (x M / (M - 1)) for the running estimate, M = N HW values per channel -- the
 * context encoder under freeze_bn=False.  u, res / r, y, g, gp, du, dr are (N, C, HW) dense; gamma, beta, the running
 * statistics and dgamma, dbeta are (C,); saved is (2, C): mean, then rstd = 1 / sqrt(var + eps).
 * scf_batch_norm_train, with xhat = (u - mean) rstd (one rounding each) and v = xhat gamma + beta:
 *   res == NULL: y = v ("mid" with relu != 0); res != NULL, gamma_r == NULL ("tail"): y = v + res; gamma_r != NULL
 *   ("tail + shortcut"): res is the raw shortcut output r, y = v + (rhat gamma_r + beta_r) with r's own statistics, kept in
 *   saved_r; beta_r, saved_r required, every *_r NULL in the other forms.  relu != 0: y = y > 0 ? y : 0.
 *   running = (1 - momentum) running + momentum batch; both running pointers of an operand NULL: none are kept.
 * Two launches.  (1) a workgroup per plane, or per 16384-element chunk of a larger plane (K chunks): count, mean = sum /
 *   count, then the sum of (x - mean)^2 -- never a raw sum of x^2 -- to workspace[3 ((n C + c) K + k)], r's behind u's.
 *   HW % 4 == 0 and u, res, y 16-byte aligned: the chunk stays in registers, thread t of 256 owns the float4 t, t + 256, ...
 *   and adds each as (a + b) + (c + d) to one chain from +0; otherwise thread t adds elements t, t + 256, ... in two sweeps;
 *   then the workgroup's tree.  (2) every wave combines its channel's N K triples, p = n K + k, with Chan's formula
 *   (n = na + nb, d = mean_b - mean_a, f = nb / n, mean = mean_a + d f, m2 = (m2_a + m2_b) + (d d) (na f)): groups of 64
 *   consecutive p in a butterfly over lane distance 1, 2, ..., 32 with the lower lane as a, the groups folded in ascending
 *   order; var = m2 / M.  The block of sample 0 that holds a plane's first element writes saved and the running statistics.
 * scf_batch_norm_train_grad, with g' the cotangent at BN(u), S1 = sum g', S2 = sum g' xhat over the channel:
 *   du = ((g' - S1 / M) - xhat (S2 / M)) (gamma rstd)   (one rounding each),   dbeta = S1, dgamma = S2.
 *   y == NULL, gp == NULL, r == NULL ("mid"): g' = g, which the consumer's dgrad epilogue has already masked.
 *   y, gp != NULL, r == NULL ("tail"): g' = y > 0 ? g : +0, written to gp (the cotangent of res) as well.
 *   y, r != NULL, gp == NULL ("tail + shortcut"): g' as in the tail form; du from saved / gamma / S2, dr from saved_r /
 *   gamma_r / S2r = sum g' rhat; dbeta_r = S1; saved_r, gamma_r, dr, dgamma_r, dbeta_r required, NULL in the other forms.
 *   mean and rstd are read from saved, never recomputed; the mask is read from y, the forward's own bits.
 *   Two launches.  (1) per plane or chunk (S1, S2, S2r), a thread's elements in one chain from +0 (float4: (a + b) +
 *   (c + d)), the workgroup's tree, to workspace[3 ((n C + c) K + k)].  (2) lane l of a wave adds the triples p = l, l + 64,
 *   ... in one chain from +0, then v[l] += v[l ^ j] for j = 32, ..., 1; accumulate != 0: the previous value of dgamma /
 *   dbeta is added last.  du may alias g element for element in the mid form; nothing else may alias.
 * workspace: scf_batch_norm_train_workspace(N, C, HW) floats for either call (or its error code).
 * No atomics, allocation or synchronisation; bit-identical from run to run, the order fixed by (N, HW) and the alignment.
 * A null required pointer, a pointer that is not 4-byte aligned, a form's NULL rule broken, a size <= 0, a workspace too
 * small, or M == 1 (no unbiased variance; torch raises there too): SCF_EINVAL.  M > 2^24 (the counts travel as floats) or
 * more than 2^31 - 1 blocks: SCF_EUNSUPPORTED.  Nothing is launched or written then.
 * Added without a version bump; the presence of scf_batch_norm_train marks the feature.
 * scf_batch_norm_train_route (a host call, the launcher's own decision): what both entries launch for (N, C, HW) with
 *   aligned != 0: every (N, C, HW) operand on a 16-byte boundary -> route[0] the statistics kernel (1, 4 or 16 float4 per
 *   thread in registers; 0: the looped kernel), route[1] 1: float4 sweeps in every pass, 0: scalar, route[2] K chunks per
 *   plane, route[3] apply blocks per plane (4096 elements each), route[4] groups of 64 partials per channel
 *   (ceil(N K / 64)).  Returns SCF_OK, or the size's error code as above (route NULL: SCF_EINVAL) with route unwritten.
 * --------------------------------------------------------------------------------- */
int64_t scf_batch_norm_train_workspace(int N, int C, int HW);
int scf_batch_norm_train_route(int N, int C, int HW, int aligned, int* route);
int scf_batch_norm_train(const float* u, const float* gamma, const float* beta, float* running_mean, float* running_var,
                         const float* res, const float* gamma_r, const float* beta_r, float* running_mean_r,
                         float* running_var_r, int relu, float momentum, float eps, float* y, float* saved, float* saved_r,
                         float* workspace, int64_t workspace_floats, int N, int C, int HW, scf_stream_t stream);
int scf_batch_norm_train_grad(const float* g, const float* y, const float* u, const float* r, const float* saved,
                              const float* saved_r, const float* gamma, const float* gamma_r, float* gp, float* du, float* dr,
                              float* dgamma, float* dbeta, float* dgamma_r, float* dbeta_r, int accumulate, float* workspace,
                              int64_t workspace_floats, int N, int C, int HW, scf_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Gate arithmetic of the ConvGRU backward (raft_decoder.py:168-253; gru_grad.hip), between the convolution gradients
 * above.  One pass of the forward: z = sigmoid(conv_z([h|x])), r = sigmoid(conv_r([h|x])), q = tanh(conv_q([r h|x])),
 * h' = (1 - z) h + z q.  With g = d loss / d h':  u_q = g z (1 - q^2), u_z = g (q - h) z (1 - z), [g_rh | g_x] =
 * dgrad_q(u_q), u_r = g_rh h r (1 - r), g_h = g (1 - z) + g_rh r + the h columns of dgrad_zr([u_z | u_r]).
 * Every operand is (M, n): rows of n floats with a row stride in elements (a channel slice of a wider NCHW tensor is
 * an operand).  Elementwise, fp32, no atomics / allocation / synchronisation; each line below is ONE rounding:
 *   grad_q: t1 = g z, dq = fma(-q, q, 1), u_q = t1 dq;  d = q - h, t2 = g d, dz = z (1 - z), u_z = t2 dz + 0
 *   grad_r: t3 = g_rh h, dr = r (1 - r), u_r = t3 dr + 0;  a = 1 - z, b = g a, g_h_direct = fma(g_rh, r, b)
 * dq / dz / dr are scf_act_grad's factors applied the same way: u_q == scf_act_grad(g z, q, TANH) bit for bit, and so
 * on.  "+ 0" turns a -0 product into +0: a zero cotangent gives +0 everywhere.
 * sum_* (optional, NULL: none): running sums over the calls of a scan, sum = first ? u : sum + u.
 * A null required pointer, M <= 0, n <= 0 or a stride below n: SCF_EINVAL with nothing launched or written.
 * Added without a version bump; the presence of scf_gru_gate_grad_q marks the feature.
 * --------------------------------------------------------------------------------- */

/* (g, h, z, q) -> u_q, u_z (u_z usually rows [0, Ch) of the (M, 2 Ch, H, W) tensor [u_z | u_r]). */
int scf_gru_gate_grad_q(const float* g, int64_t g_stride, const float* h, int64_t h_stride, const float* z,
                        int64_t z_stride, const float* q, int64_t q_stride, float* u_q, int64_t u_q_stride, float* u_z,
                        int64_t u_z_stride, float* sum_q, int64_t sum_q_stride, float* sum_z, int64_t sum_z_stride,
                        int first, int M, int64_t n, scf_stream_t stream);

/* (g, z, g_rh, h, r) -> u_r, and g_h_direct = g (1 - z) + g_rh r written IN PLACE over g_rh (the first Ch channels
 * of the q convolution's input gradient: that buffer is then the `add` operand of the z|r convolution's dgrad). */
int scf_gru_gate_grad_r(const float* g, int64_t g_stride, const float* z, int64_t z_stride, float* g_rh,
                        int64_t g_rh_stride, const float* h, int64_t h_stride, const float* r, int64_t r_stride,
                        float* u_r, int64_t u_r_stride, float* sum_r, int64_t sum_r_stride, int first, int M, int64_t n,
                        scf_stream_t stream);

/* The carried cotangent of the reverse scan: out = src + add (add NULL: out = src), one rounding; clear != 0: src is
 * then set to +0 (a pass hands its g_h over and leaves [0 | g_x] behind as the next dgrad's `add` operand). */
int scf_gru_carry(float* src, int64_t src_stride, const float* add, int64_t add_stride, float* out, int64_t out_stride,
                  int clear, int M, int64_t n, scf_stream_t stream);

/* What the backward recomputes of the forward's gate epilogues next to the convolutions: q NULL: out = gate h (the
 * q convolution's input r h); else a = 1 - gate, b = a h, out = fma(gate, q, b) (the state update (1 - z) h + z q). */
int scf_gru_gate_state(const float* h, int64_t h_stride, const float* gate, int64_t gate_stride, const float* q,
                       int64_t q_stride, float* out, int64_t out_stride, int M, int64_t n, scf_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Adjoint of scf_corr_lookup with respect to the pyramid, carried back to level 0 through the 2x2 / stride-2 average
 * pools of scf_corr_build (corr_lookup_grad.hip).  g_corr (T, N, L (2r+1)^2, h, w): the cotangents of the lookup outputs
 * of T iterations in the forward's channel order (channel (2r+1)^2 l + (2r+1) a + b: x-offset a - r, y-offset b - r);
 * flow (T, N, 2, h, w): the flow each lookup was taken at; mask: NULL or (T, N, 1, h, w), a per-query factor on g_corr
 * (one rounding); g_vol (N h w, h, w) row-major: d loss / d level 0, summed over T -- every element is written (no
 * pre-zeroing), with accumulate != 0 the previous value is added last.  The pyramid is not read.
 * With x0, y0, nw, ne, sw, se of the forward's window centre of (query, level, iteration), i = jx - x0, k = jy - y0 and
 * G[a, b] = mask g_corr of tap (a, b), +0 outside [0, 2r]^2:
 *   S_l[jy, jx] = sum_t  nw G[i, k] + ne G[i - 1, k] + sw G[i, k - 1] + se G[i - 1, k - 1]
 *   g_vol[q, jy, jx] = sum_l 4^-l S_l[jy >> l, jx >> l]   over the l with (jy >> l) < (h >> l) and (jx >> l) < (w >> l)
 * A size-1 axis: cell 0 takes every offset of that axis.  A query with a NaN / inf flow at iteration t contributes zero
 * at t (its window is all padding).  Order: S_l from +0, t ascending, offsets of a size-1 x axis then of a size-1 y
 * axis ascending, the four terms as one fma chain in nw, ne, sw, se order; levels ascending, v = fma(4^-l, S_l, v)
 * from v = S_0.  No atomics, allocation or synchronisation; bit-identical from run to run; a sample's result does not
 * depend on N.  r <= 4 with a query's accumulators inside 64 KB of LDS: staged through LDS; else one thread per element.
 * A null g_corr / flow / g_vol, a non-positive size, r < 1, an empty level: SCF_EINVAL; L > SCF_MAX_LEVELS or
 * T > SCF_TAIL_MAX_T: SCF_EUNSUPPORTED; nothing launched or written.  Added without a version bump; the presence of
 * the symbol marks the feature.
 * scf_corr_lookup_grad_route (a host call, the launcher's own decision): what a call with these sizes launches ->
 *   route[0] 0: staged through LDS, 1: one thread per element; on the staged route route[1] the radius the kernel is
 *   instantiated for (1 .. 4), route[2] log2 of the queries per block (0 .. 4: the largest whose staging, centres and
 *   accumulators fit in 64 KB with at most 24 cotangents per thread), route[3] 1 when the last block holds fewer queries
 *   than that (N h w is no multiple); on the other route 0, -1, 0.  Returns SCF_OK, or the sizes' error code as above
 *   (route NULL: SCF_EINVAL) with route unwritten.
 * --------------------------------------------------------------------------------- */
int scf_corr_lookup_grad(const float* g_corr, const float* flow, const float* mask, float* g_vol, int accumulate, int T,
                         int N, int h, int w, int r, int L, scf_stream_t stream);
int scf_corr_lookup_grad_route(int N, int h, int w, int r, int L, int* route);

/* ---------------------------------------------------------------------------------
 * Adjoint of scf_corr_build's level 0 with respect to the two feature maps (corr_build_grad.hip).  g_vol (N, hw, hw)
 * row-major: d loss / d level 0, exactly what scf_corr_lookup_grad writes (the tiled pyramid layout never reaches this
 * stage); feat1 (queries i) / feat2 (targets j) and both outputs (N, C, h, w) dense.  With s = 1/sqrt(C):
 *   g_feat1[n][c][i] = s sum_j g_vol[n][i][j] feat2[n][c][j]
 *   g_feat2[n][c][j] = s sum_i g_vol[n][i][j] feat1[n][c][i]
 * Two fp32 matrix-instruction GEMMs, one launch each; a block owns 128 channels x 128 positions of one sample and walks
 * the whole contraction.  Order: per output ONE fma chain from +0 over the contraction index ascending (j resp. i), then
 * the scale once -- multiplied by s when sqrt(C) is a power of two (exact), otherwise a correctly rounded division by
 * sqrtf(C): scf_corr_build's rule.  One route: every N, C, h, w >= 1 and any 4-byte aligned pointers, every load and
 * store under an explicit bound.  No atomics, allocation or synchronisation; bit-identical from run to run; a sample's
 * result does not depend on N.  A NaN at g_vol[n][i][j] reaches g_feat1[n][:, i] and g_feat2[n][:, j] only.
 * A null pointer, a non-positive size, or an output that overlaps the other output or an input: SCF_EINVAL; h w or C
 * within 128 of 2^31, an operand of 2^61 floats and more, or 2^31 tiles and more: SCF_EUNSUPPORTED; nothing launched or
 * written.  Added without a version bump; the presence of the symbol marks the feature.
 * --------------------------------------------------------------------------------- */
int scf_corr_build_grad(const float* g_vol, const float* feat1, const float* feat2, float* g_feat1, float* g_feat2, int N,
                        int C, int h, int w, scf_stream_t stream);

/* RAFT convex up-sampling (x8, 3x3 neighbourhood).  replaces RAFTDecoder._upsample
 * models/decoder/raft_decoder.py:381-416 and RAFTDecoderMask.upsample_flow/upsample_mask
 * raft_decoder_mask.py:104-160:  out[n,c,8y+sy,8x+sx] = sum_k softmax_k(mask_mul *
 * mask[n, k*64+sy*8+sx, y, x]) * x_mul * x[n, c, y+k/3-1, x+k%3-1] (zero padded).
 * x (N,C,h,w); mask (N,9*64,h,w); out (N,C,8h,8w).                                     */
int scf_convex_upsample(const float* x, const float* mask, float* out, int N, int C, int h,
                        int w, int scale, float x_mul, float mask_mul, scf_stream_t stream);

/* 2x2 stride-2 average pool over (planes, Hin, Win) -> (planes, Hin/2, Win/2)          */
int scf_avgpool2x2(const float* x, float* out, int64_t planes, int Hin, int Win,
                   scf_stream_t stream);

/* out[n, c, :] = x[n, c, :] * mask[n, 0, :]  (mask (N, 1, HW) dense; x / out sample-strided): the
 * occlusion masking of the looked-up correlation / of the flow, scflow_decoder.py:199-205
 * (constructor switches mask_corr / mask_flow; both False in configs/refine_models/scflow.py). */
int scf_mul_mask(const float* x, int64_t x_nstride, const float* mask, float* out,
                 int64_t out_nstride, int N, int C, int HW, scf_stream_t stream);

/* elementwise helpers used for glue (split tanh/relu of the context features etc.)   */
int scf_copy_strided(const float* src, int64_t src_nstride, float* dst, int64_t dst_nstride,
                     int N, int64_t count, scf_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Optimizer step (optim.hip): gradient-norm clipping and AdamW over a LIST of tensors in at most three launches.
 * replaces torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW(amsgrad=False) as the reference's runner applies them
 * (configs/refine_models/scflow.py: optimizer, optimizer_config.grad_clip).
 * Added without a version bump (SCF_VERSION stays at .3): the presence of scf_adamw_step marks the feature.
 *
 * The tensors are cut into chunks of SCF_ADAMW_CHUNK elements, a tensor's last chunk ragged; one block of
 * SCF_ADAMW_NORM_THREADS threads owns one chunk.  scf_adamw_chunks is a HOST function: it writes the table for tensors of
 * sizes[0..ntensors) elements to out[0..capacity) (host memory) and returns the number of chunks; out = NULL only
 * counts.  Empty tensors get no chunk.  The caller uploads the table once.
 *
 * p, g, m, v are DEVICE arrays of ntensors device pointers (parameter, gradient, first and second moment; fp32, each
 * tensor contiguous, any 4-byte alignment).  The chunk table is trusted: it must come from scf_adamw_chunks over the
 * sizes of exactly these tensors.
 *
 * scf_grad_sqnorm: partial[b] = sum of g^2 over chunk b, then *norm = sqrt(sum_b partial[b]); both sums in a fixed
 * order without atomics (bitwise reproducible for the same pointers; the order depends on the chunking and on each
 * gradient's address modulo 16).  fp32 accumulation.  partial: nchunks floats of scratch.  Two launches.
 *
 * scf_adamw_step: with c = min(max_norm / (*norm + 1e-6), 1) (c = 1 when norm is NULL; a NaN norm gives c = NaN), per
 * element, in fp32 and in torch's operation order:
 *   g' = c g;  p *= 1 - lr wd;  m += (g' - m)(1 - beta1);  v = beta2 v + (1 - beta2) g'^2;
 *   p -= (lr / bias_correction1) * (m / (sqrt(v) / sqrt(bias_correction2) + eps))
 * g is not modified.  lr, the step count and both bias corrections (1 - beta^t) are the caller's, in double; the
 * entry rounds the derived factors to fp32 once.  One launch.  Nothing here synchronises: norm is read on the device. */
#define SCF_ADAMW_CHUNK 4096
#define SCF_ADAMW_NORM_THREADS 256
typedef struct scf_adamw_chunk {
  int32_t tensor;   /* index into p / g / m / v */
  int32_t length;   /* 1 .. SCF_ADAMW_CHUNK elements */
  int64_t offset;   /* first element, a multiple of SCF_ADAMW_CHUNK */
} scf_adamw_chunk;
int64_t scf_adamw_chunks(const int64_t* sizes, int ntensors, scf_adamw_chunk* out, int64_t capacity);
int scf_grad_sqnorm(const scf_adamw_chunk* chunks, int64_t nchunks, const float* const* g, float* partial,
                    float* norm, scf_stream_t stream);
int scf_adamw_step(const scf_adamw_chunk* chunks, int64_t nchunks, float* const* p, const float* const* g,
                   float* const* m, float* const* v, const float* norm, double max_norm, double lr,
                   double weight_decay, double beta1, double beta2, double eps, double bias_correction1,
                   double bias_correction2, scf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SCFLOW_HIP_H */
