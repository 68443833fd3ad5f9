// Backward of a stride-1, same-padding convolution with bias (the decoder's XHeads and delta-flow / mask encoders,
// scflow_decoder.py:210-217; the family also covers the GRU's 1x5 / 5x1 gates and the motion encoder's 1x1 / 3x3 / 7x7
// layers), for gfx950, fp32 throughout.  KH and KW each in {1, 3, 5, 7}, pad = (KH / 2, KW / 2), any H, W >= 1.
//
//   scf_conv_s1_dgrad            gx[m, ci, iy, ix] = act'(a) (sum_{ky, kx, co} g[m, co, iy + py - ky, ix + px - kx] w[co, ci, ky, kx] + add)
//   scf_conv_s1_wgrad            dW[co, ci, ky, kx] = sum_{m, y, x} g[m, co, y, x] x[m, ci, y - py + ky, x - px + kx],  db[co] = sum g
//   scf_conv_s1_wgrad_workspace  the floats of device memory the second needs
//   scf_act_grad                 out = g act'(a), elementwise
//
// No atomics, no allocation, no synchronisation: every sum has ONE order, fixed by the shapes alone.  g, add, a, gx, x
// take a sample stride in elements (channel slices of wider tensors are operands); w / dW are the raw torch layout.
//
// Routes, a function of (Cout, Cin) only, never of M or the map:
//   wide   min(Cout, Cin) >= S1_MFMA_MIN_C = 32: v_mfma_f32_32x32x2_f32 (the XHeads' packed hidden layer 128 -> 512,
//          delta_flow_encoder[1] 128 -> 64, mask_encoder[1] 64 -> 32)
//   thin   everything else: vector ALU (the predict layers 256 -> 2 and 256 -> 1, delta_flow_encoder[0] 2 -> 128,
//          mask_encoder[0] 1 -> 64); an MFMA tile would be at least half zeros there and the layers are bound by HBM
//
//   dgrad  Per output ONE fma chain that starts at +0: taps in ascending (ky, kx), inside a tap co ascending.
//          wide: a block owns SD_PIX = 64 pixels (numbered (m, iy, ix) row-major) x SD_CI = 128 input channels (wave v:
//          channels [32 v, 32 v + 32), two 32 x 32 accumulators); co goes in chunks of SD_CHUNK = 32 (zero columns past
//          Cout), a tap that leaves the map contributes zeros (g is read as +0 there): length KH KW 32 ceil(Cout / 32).
//          w is read at the strides the host passes: the torch layout, or (w_scratch given) a [tap][co][ci] copy that a
//          launch in front writes, so that the lanes of a load are 4 bytes apart, not 4 KH KW.
//          thin: a thread owns one pixel of SDV_CI = 2 input channels (one g load for both; the pair is the block's, so
//          w comes through scalar loads); taps outside the map are skipped: length <= KH KW Cout.
//          Then in both: + add (one rounding), times the factor: RELU a > 0 ? v : +0; SIGMOID v * (a * (1 - a)), TANH
//          v * fma(-a, a, 1).  A pixel's chain reads its own sample only: the result does not depend on M.
//   wgrad  The contraction over the pixels is cut into S splits with a partial each in workspace[s][tap][co][ci] (then
//          S Cout floats of db partials [s][co]); the combine launch takes partial 0, adds partials 1 .. S - 1 in
//          ascending order, adds the destination's previous value LAST under `accumulate`, writes the torch layout.
//          wide: the map's rows are cut into segments of SW_PIX = 16 pixels; chunk c = (m, y, segment) row-major.  A block
//          owns SW_TILE = 64 output x 64 input channels (2 x 2 waves), ONE kernel row ky with its KW taps (KW
//          accumulators per wave) and one split: cps = max(SW_MIN_CHUNKS, ceil(chunks / max(1, SW_BLOCKS / tiles)))
//          consecutive chunks, tiles = co tiles x ci tiles x KH, S = ceil(chunks / cps).  A chunk stages the g segment
//          and the halo row of x (16 + KW - 1 values per channel, each ONCE for the KW taps).  Inside a split ONE fma
//          chain per (tap, co, ci) from +0, chunks ascending, pixels ascending (zeros in the padding and past W): 16 cps
//          steps.  db: the blocks of (ky = 0, ci tile 0) add the staged g values, one chain of plain adds from +0 in
//          the same order.
//          thin: a block owns one (co, ci), all taps, and one split of per = max(VW_MIN_PIX, ceil(Q / max(1, VW_BLOCKS /
//          (Cout Cin)))) rounded up to a multiple of VW_THREADS = 256 pixels q = (m, y, x) row-major, S = ceil(Q / per).
//          Per tap, thread t: one fma chain from +0 over q = q0 + t, q0 + t + 256, ... (taps outside the map skipped; a
//          kernel row's KW taps share the g load); then the 256 values are added pairwise in LDS, v[t] += v[t + k] for
//          k = 128, 64, ..., 1.  db: the blocks of ci = 0 sum g the same way.
#include "scf_common.h"

typedef float s1_f32x16 __attribute__((ext_vector_type(16)));

#define S1_THREADS 256
#define S1_MFMA_MIN_C 32              // min(Cout, Cin) >= this: the MFMA route
#define S1_MAX_K 7
#define SD_PIX 64                     // pixels per block: two MFMA column tiles
#define SD_CI 128                     // input channels per block: 4 waves x 32
#define SD_CHUNK 32                   // output channels staged at a time
#define SD_WPITCH (SD_CI + 32)
#define SD_GPITCH (SD_PIX + 32)
#define SDV_CI 2                      // input channels a thread of the vector dgrad owns
#define SW_TILE 64                    // output channels x input channels of a block: 2 x 2 waves
#define SW_PIX 16                     // pixels of a row segment staged at a time
#define SW_PITCH 65
#define SW_MIN_CHUNKS 16              // a split holds at least this many chunks (when there are as many)
#define SW_BLOCKS 1024                // the splits aim at this many blocks
#define VW_THREADS 256
#define VW_MIN_PIX 1024               // a thin split holds at least this many pixels (when there are as many)
#define VW_BLOCKS 2048

static inline bool s1_kernel_ok(int K) { return K == 1 || K == 3 || K == 5 || K == 7; }
static inline bool s1_wide(int Cout, int Cin) { return (Cout < Cin ? Cout : Cin) >= S1_MFMA_MIN_C; }

__device__ __forceinline__ float s1_act_factor(float v, float a, int act) {
  if (act == SCF_ACT_RELU) return a > 0.f ? v : 0.f;
  if (act == SCF_ACT_SIGMOID) return v * (a * (1.f - a));
  if (act == SCF_ACT_TANH) return v * __fmaf_rn(-a, a, 1.f);
  return v;
}

// ========================================================================================================= act_grad
__global__ __launch_bounds__(S1_THREADS) void s1_act_grad_kernel(const float* g, long long gs, const float* a, long long as,
                                                                 int act, float* out, long long os, long long n,
                                                                 long long total) {
  const long long e = (long long)blockIdx.x * S1_THREADS + threadIdx.x;
  if (e >= total) return;
  const long long m = e / n, r = e - m * n;
  const float v = g[m * gs + r];
  out[m * os + r] = act == SCF_ACT_NONE ? v : s1_act_factor(v, a[m * as + r], act);
}

extern "C" int scf_act_grad(const float* g, int64_t g_stride, const float* a, int64_t a_stride, int act, float* out,
                            int64_t out_stride, int M, int64_t n, scf_stream_t stream) {
  if (!g || !out || M <= 0 || n <= 0 || g_stride < n || out_stride < n) return SCF_EINVAL;
  if (act != SCF_ACT_NONE && act != SCF_ACT_RELU && act != SCF_ACT_SIGMOID && act != SCF_ACT_TANH) return SCF_EINVAL;
  if (act != SCF_ACT_NONE && (!a || a_stride < n)) return SCF_EINVAL;
  const long long total = (long long)M * n, blocks = scf_cdiv(total, S1_THREADS);
  if (blocks > 0x7fffffffll) return SCF_EUNSUPPORTED;
  scf_launch(s1_act_grad_kernel, dim3((unsigned)blocks), dim3(S1_THREADS), 0, scf_stream(stream), g, (long long)g_stride,
             a, (long long)a_stride, act, out, (long long)out_stride, (long long)n, total);
  return scf_launch_status();
}

// ============================================================================================================ dgrad
struct S1Dgrad {
  const float* g; const float* w; const float* add; const float* a; float* gx;
  long long gs, adds, as, gxs, wco, wci, wtap;
  int M, Cout, Cin, H, W, KH, KW, act;
};

// w (Cout, Cin, KH KW) -> scratch [tap][co][ci]
__global__ __launch_bounds__(S1_THREADS) void s1_transpose_w_kernel(const float* w, float* wt, int Cout, int Cin, int KK) {
  const long long n = (long long)KK * Cout * Cin;
  const long long e = (long long)blockIdx.x * S1_THREADS + threadIdx.x;
  if (e >= n) return;
  const int ci = (int)(e % Cin);
  const long long r = e / Cin;
  const int co = (int)(r % Cout), tap = (int)(r / Cout);
  wt[e] = w[((long long)co * Cin + ci) * KK + tap];
}

__global__ __launch_bounds__(S1_THREADS) void s1_dgrad_mfma_kernel(S1Dgrad p) {
  __shared__ float Wt[SD_CHUNK * SD_WPITCH];      // [co][ci]
  __shared__ float Gt[SD_CHUNK * SD_GPITCH];      // [co][pixel]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l32 = lane & 31;
  const long long plane = (long long)p.H * p.W;
  const long long P = (long long)p.M * plane;
  const long long p0 = (long long)blockIdx.x * SD_PIX;
  const int ci0 = (int)blockIdx.y * SD_CI;
  const int pad_y = p.KH >> 1, pad_x = p.KW >> 1;
  const int ncc = (p.Cout + SD_CHUNK - 1) / SD_CHUNK, steps = p.KH * p.KW * ncc;
  // loader coordinates: g tile 32 x 64 (8 per thread), w tile 32 x 128 (16 per thread)
  const int gp = tid & 63, go = tid >> 6;          // + 4 i
  const int wk = tid & 127, wo = tid >> 7;         // + 2 i
  const long long gq = p0 + gp;
  const bool gvalid = gq < P;
  int gm = 0, giy = 0, gix = 0;
  if (gvalid) { gix = (int)(gq % p.W); const long long r = gq / p.W; giy = (int)(r % p.H); gm = (int)(r / p.H); }
  float gv[8], wv[16];
  auto fetch = [&](int s) {
    const int t = s / ncc, oc = (s - t * ncc) * SD_CHUNK;
    const int ky = t / p.KW, kx = t - ky * p.KW;
    const int oy = giy + pad_y - ky, ox = gix + pad_x - kx;
    const bool ok = gvalid && oy >= 0 && oy < p.H && ox >= 0 && ox < p.W;
    const float* gb = p.g + (long long)gm * p.gs + (long long)oy * p.W + ox;      // read only under ok
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int co = oc + go + 4 * i;
      gv[i] = (ok && co < p.Cout) ? gb[(long long)co * plane] : 0.f;
    }
    const int ci = ci0 + wk;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int co = oc + wo + 2 * i;
      wv[i] = (co < p.Cout && ci < p.Cin) ? p.w[co * p.wco + ci * p.wci + t * p.wtap] : 0.f;
    }
  };
  s1_f32x16 acc0, acc1;
#pragma unroll
  for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
  fetch(0);
  for (int s = 0; s < steps; ++s) {
    __syncthreads();                                 // the previous chunk's operands are read
#pragma unroll
    for (int i = 0; i < 8; ++i) Gt[(go + 4 * i) * SD_GPITCH + gp] = gv[i];
#pragma unroll
    for (int i = 0; i < 16; ++i) Wt[(wo + 2 * i) * SD_WPITCH + wk] = wv[i];
    __syncthreads();
    if (s + 1 < steps) fetch(s + 1);                 // in flight while this chunk is contracted
    const float* ap = Wt + half * SD_WPITCH + wave * 32 + l32;
    const float* bp = Gt + half * SD_GPITCH + l32;
#pragma unroll
    for (int o = 0; o < SD_CHUNK; o += 2) {
      const float a = ap[o * SD_WPITCH];
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bp[o * SD_GPITCH], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bp[o * SD_GPITCH + 32], acc1, 0, 0, 0);
    }
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const long long q = p0 + 32 * j + l32;
    if (q >= P) continue;
    const long long m = q / plane, pix = q - m * plane;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ci = ci0 + wave * 32 + 8 * (r >> 2) + 4 * half + (r & 3);
      if (ci >= p.Cin) continue;
      const long long off = (long long)ci * plane + pix;
      float v = j ? acc1[r] : acc0[r];
      if (p.add) v = v + p.add[m * p.adds + off];
      if (p.act != SCF_ACT_NONE) v = s1_act_factor(v, p.a[m * p.as + off], p.act);
      p.gx[m * p.gxs + off] = v;
    }
  }
}

__global__ __launch_bounds__(S1_THREADS) void s1_dgrad_valu_kernel(S1Dgrad p, long long total) {
  const long long e = (long long)blockIdx.x * S1_THREADS + threadIdx.x;
  if (e >= total) return;
  const long long plane = (long long)p.H * p.W;
  const int ix = (int)(e % p.W);
  const long long r = e / p.W;
  const int iy = (int)(r % p.H);
  const long long m = r / p.H;
  const int ci = (int)blockIdx.y * SDV_CI;               // channels ci, ci + 1 (one g load for both): the same for the whole
                                                         // block, so the loads of w are scalar loads
  const bool two = ci + 1 < p.Cin;
  const int pad_y = p.KH >> 1, pad_x = p.KW >> 1, KK = p.KH * p.KW;
  const float* gm = p.g + m * p.gs;
  const float* wc = p.w + (long long)ci * KK;
  const long long wstep = (long long)p.Cin * KK;
  float acc0 = 0.f, acc1 = 0.f;
  for (int ky = 0; ky < p.KH; ++ky) {
    const int oy = iy + pad_y - ky;
    if (oy < 0 || oy >= p.H) continue;
    for (int kx = 0; kx < p.KW; ++kx) {
      const int ox = ix + pad_x - kx;
      if (ox < 0 || ox >= p.W) continue;
      const float* gp = gm + (long long)oy * p.W + ox;
      const float* wp = wc + ky * p.KW + kx;
      if (two) {
        for (int co = 0; co < p.Cout; ++co) {
          const float gval = gp[co * plane];
          acc0 = __fmaf_rn(gval, wp[co * wstep], acc0);
          acc1 = __fmaf_rn(gval, wp[co * wstep + KK], acc1);
        }
      } else {
        for (int co = 0; co < p.Cout; ++co) acc0 = __fmaf_rn(gp[co * plane], wp[co * wstep], acc0);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < SDV_CI; ++j) {
    if (j == 1 && !two) break;
    const long long off = (long long)(ci + j) * plane + (long long)iy * p.W + ix;
    float v = j ? acc1 : acc0;
    if (p.add) v = v + p.add[m * p.adds + off];
    if (p.act != SCF_ACT_NONE) v = s1_act_factor(v, p.a[m * p.as + off], p.act);
    p.gx[m * p.gxs + off] = v;
  }
}

extern "C" int scf_conv_s1_dgrad(const float* g, int64_t g_stride, const float* w, const float* add, int64_t add_stride,
                                 const float* a, int64_t a_stride, int act, float* gx, int64_t gx_stride, float* w_scratch,
                                 int M, int Cout, int Cin, int H, int W, int KH, int KW, scf_stream_t stream) {
  if (!g || !w || !gx || M <= 0 || Cout <= 0 || Cin <= 0 || H <= 0 || W <= 0 || KH <= 0 || KW <= 0) return SCF_EINVAL;
  if (act != SCF_ACT_NONE && act != SCF_ACT_RELU && act != SCF_ACT_SIGMOID && act != SCF_ACT_TANH) return SCF_EINVAL;
  if (act != SCF_ACT_NONE && !a) return SCF_EINVAL;
  const long long plane = (long long)H * W;
  if (g_stride < Cout * plane || gx_stride < Cin * plane || (add && add_stride < Cin * plane) ||
      (act != SCF_ACT_NONE && a_stride < Cin * plane))
    return SCF_EINVAL;
  if (!s1_kernel_ok(KH) || !s1_kernel_ok(KW)) return SCF_EUNSUPPORTED;
  const int KK = KH * KW;
  S1Dgrad p;
  p.g = g; p.w = w; p.add = add; p.a = act != SCF_ACT_NONE ? a : nullptr; p.gx = gx;
  p.gs = g_stride; p.adds = add_stride; p.as = a_stride; p.gxs = gx_stride;
  p.wco = (long long)Cin * KK; p.wci = KK; p.wtap = 1;
  p.M = M; p.Cout = Cout; p.Cin = Cin; p.H = H; p.W = W; p.KH = KH; p.KW = KW; p.act = act;
  if (!s1_wide(Cout, Cin)) {
    const long long total = (long long)M * plane, blocks = scf_cdiv(total, S1_THREADS), cg = scf_cdiv(Cin, SDV_CI);
    if (blocks > 0x7fffffffll || cg > 65535) return SCF_EUNSUPPORTED;
    scf_launch(s1_dgrad_valu_kernel, dim3((unsigned)blocks, (unsigned)cg), dim3(S1_THREADS), 0, scf_stream(stream), p, total);
    return scf_launch_status();
  }
  const long long pt = scf_cdiv((long long)M * plane, SD_PIX), ct = scf_cdiv(Cin, SD_CI);
  if (pt > 0x7fffffffll || ct > 65535) return SCF_EUNSUPPORTED;
  if (w_scratch) {
    const long long n = (long long)KK * Cout * Cin, blocks = scf_cdiv(n, S1_THREADS);
    if (blocks > 0x7fffffffll) return SCF_EUNSUPPORTED;
    scf_launch(s1_transpose_w_kernel, dim3((unsigned)blocks), dim3(S1_THREADS), 0, scf_stream(stream), w, w_scratch, Cout,
               Cin, KK);
    const int rc = scf_launch_status();
    if (rc != SCF_OK) return rc;
    p.w = w_scratch; p.wtap = (long long)Cout * Cin; p.wco = Cin; p.wci = 1;
  }
  scf_launch(s1_dgrad_mfma_kernel, dim3((unsigned)pt, (unsigned)ct), dim3(S1_THREADS), 0, scf_stream(stream), p);
  return scf_launch_status();
}

// ============================================================================================================ wgrad
struct S1Wgrad {
  const float* g; const float* x; float* ws; float* wsdb;      // wsdb NULL: no bias gradient
  long long gs, xs, Q, per;                                     // thin: Q pixels, per pixels a split
  long long chunks;                                             // wide: M H segs
  int M, Cout, Cin, H, W, KH, KW, cps, segs, cit;
};

struct S1Plan { long long splits, per_or_cps; };

static inline S1Plan s1_wgrad_plan(int M, int Cout, int Cin, int H, int W, int KH) {
  S1Plan pl;
  if (s1_wide(Cout, Cin)) {
    const long long chunks = (long long)M * H * scf_cdiv(W, SW_PIX);
    const long long tiles = scf_cdiv(Cout, SW_TILE) * scf_cdiv(Cin, SW_TILE) * KH;
    long long want = SW_BLOCKS / tiles;
    if (want < 1) want = 1;
    long long c = scf_cdiv(chunks, want);
    if (c < SW_MIN_CHUNKS) c = SW_MIN_CHUNKS;
    pl.per_or_cps = c;
    pl.splits = scf_cdiv(chunks, c);
  } else {
    const long long Q = (long long)M * H * W;
    long long want = VW_BLOCKS / ((long long)Cout * Cin);
    if (want < 1) want = 1;
    long long per = scf_cdiv(Q, want);
    if (per < VW_MIN_PIX) per = VW_MIN_PIX;
    per = scf_cdiv(per, VW_THREADS) * VW_THREADS;
    pl.per_or_cps = per;
    pl.splits = scf_cdiv(Q, per);
  }
  return pl;
}

template <int KW>
__global__ __launch_bounds__(S1_THREADS) void s1_wgrad_mfma_kernel(S1Wgrad p) {
  constexpr int XW = SW_PIX + KW - 1;                 // the halo row: each x value staged once for the KW taps
  constexpr int NX = (XW * SW_TILE + S1_THREADS - 1) / S1_THREADS;
  __shared__ float Gt[SW_PIX * SW_PITCH];             // [pixel][co]
  __shared__ float Xt[XW * SW_PITCH];                 // [halo pixel][ci]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l32 = lane & 31;
  const int wr = wave >> 1, wc = wave & 1;
  const int ci0 = (int)blockIdx.y * SW_TILE;
  const int ky = (int)blockIdx.z % p.KH, co0 = ((int)blockIdx.z / p.KH) * SW_TILE;
  const int pad_y = p.KH >> 1, pad_x = KW >> 1;
  const long long chunk0 = (long long)blockIdx.x * p.cps;
  const long long chunk1 = chunk0 + p.cps < p.chunks ? chunk0 + p.cps : p.chunks;
  const long long plane = (long long)p.H * p.W;
  const int lp = tid & 15, lc = tid >> 4;             // g: pixel lp, co lc + 16 i
  const bool do_db = p.wsdb && ky == 0 && blockIdx.y == 0;
  float gv[4], xv[NX];
  auto fetch = [&](long long c) {
    const int seg = (int)(c % p.segs);
    const long long rr = c / p.segs;
    const int y = (int)(rr % p.H);
    const long long m = rr / p.H;
    const int x0 = seg * SW_PIX;
    const float* gb = p.g + m * p.gs + (long long)y * p.W + x0 + lp;
    const bool gok = x0 + lp < p.W;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int co = co0 + lc + 16 * i;
      gv[i] = (gok && co < p.Cout) ? gb[(long long)co * plane] : 0.f;
    }
    const int iy = y - pad_y + ky;
    const bool yok = iy >= 0 && iy < p.H;
    const float* xb = p.x + m * p.xs + (long long)iy * p.W;      // read only under yok
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      const int e = tid + S1_THREADS * i;
      const int cl = e / XW, j = e - cl * XW;
      const int ci = ci0 + cl, ix = x0 - pad_x + j;
      xv[i] = (yok && cl < SW_TILE && ci < p.Cin && ix >= 0 && ix < p.W) ? xb[(long long)ci * plane + ix] : 0.f;
    }
  };
  s1_f32x16 acc[KW];
#pragma unroll
  for (int t = 0; t < KW; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  float dbacc = 0.f;
  fetch(chunk0);
  for (long long c = chunk0; c < chunk1; ++c) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) Gt[lp * SW_PITCH + lc + 16 * i] = gv[i];
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      const int e = tid + S1_THREADS * i;
      const int cl = e / XW, j = e - cl * XW;
      if (cl < SW_TILE) Xt[j * SW_PITCH + cl] = xv[i];
    }
    __syncthreads();
    if (c + 1 < chunk1) fetch(c + 1);
    if (do_db && tid < SW_TILE) {
#pragma unroll
      for (int k = 0; k < SW_PIX; ++k) dbacc = dbacc + Gt[k * SW_PITCH + tid];
    }
    const float* ap = Gt + half * SW_PITCH + wr * 32 + l32;
    const float* bp = Xt + half * SW_PITCH + wc * 32 + l32;
#pragma unroll
    for (int k = 0; k < SW_PIX; k += 2) {
      const float a = ap[k * SW_PITCH];
#pragma unroll
      for (int t = 0; t < KW; ++t)
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bp[(k + t) * SW_PITCH], acc[t], 0, 0, 0);
    }
  }
  if (do_db && tid < SW_TILE && co0 + tid < p.Cout) p.wsdb[(long long)blockIdx.x * p.Cout + co0 + tid] = dbacc;
  const int ci = ci0 + wc * 32 + l32;
  if (ci >= p.Cin) return;
  float* dst = p.ws + (long long)blockIdx.x * p.KH * KW * p.Cout * p.Cin;
#pragma unroll
  for (int t = 0; t < KW; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = co0 + wr * 32 + 8 * (r >> 2) + 4 * half + (r & 3);
      if (co < p.Cout) dst[((long long)(ky * KW + t) * p.Cout + co) * p.Cin + ci] = acc[t][r];
    }
}

// thin route: block (split, ci, co), one kernel row ky at a time with KW accumulators a thread (one g load for the KW taps);
// blocks of ci = 0 also sum g for db (with ky = 0).  A thread's pixels q0 + t + 256 k are walked by coordinates, no division.
template <int KW>
__global__ __launch_bounds__(VW_THREADS) void s1_wgrad_valu_kernel(S1Wgrad p) {
  __shared__ float red[(KW + 1) * VW_THREADS];
  const int tid = threadIdx.x, ci = (int)blockIdx.y, co = (int)blockIdx.z;
  const long long s = blockIdx.x;
  const long long q0 = s * p.per, q1 = q0 + p.per < p.Q ? q0 + p.per : p.Q;
  const long long plane = (long long)p.H * p.W;
  const int pad_y = p.KH >> 1, pad_x = KW >> 1, KK = p.KH * KW;
  const bool do_db = p.wsdb && ci == 0;
  const long long qt = q0 + tid;
  const long long m0 = qt / plane;
  const int pix0 = (int)(qt - m0 * plane), y0 = pix0 / p.W, x0 = pix0 - y0 * p.W;
  const int sm = (int)(VW_THREADS / plane), sr = (int)(VW_THREADS - sm * plane), sy = sr / p.W, sx = sr - sy * p.W;
  for (int ky = 0; ky < p.KH; ++ky) {
    float acc[KW], accb = 0.f;
#pragma unroll
    for (int kx = 0; kx < KW; ++kx) acc[kx] = 0.f;
    long long m = m0;
    int y = y0, x = x0;
    for (long long q = qt; q < q1; q += VW_THREADS) {
      const float gval = p.g[m * p.gs + (long long)co * plane + (long long)y * p.W + x];
      if (do_db && ky == 0) accb = accb + gval;
      const int iy = y - pad_y + ky;
      if (iy >= 0 && iy < p.H) {
        const float* xr = p.x + m * p.xs + (long long)ci * plane + (long long)iy * p.W;
#pragma unroll
        for (int kx = 0; kx < KW; ++kx) {
          const int ix = x - pad_x + kx;
          if (ix >= 0 && ix < p.W) acc[kx] = __fmaf_rn(gval, xr[ix], acc[kx]);
        }
      }
      x += sx;                                         // the pixel VW_THREADS further: sx < W, sy < H
      if (x >= p.W) { x -= p.W; ++y; }
      y += sy;
      if (y >= p.H) { y -= p.H; ++m; }
      m += sm;
    }
    __syncthreads();                                   // the previous row's sums are read
#pragma unroll
    for (int kx = 0; kx < KW; ++kx) red[kx * VW_THREADS + tid] = acc[kx];
    red[KW * VW_THREADS + tid] = accb;
    __syncthreads();
    for (int k = VW_THREADS / 2; k >= 1; k >>= 1) {
      if (tid < k) {
#pragma unroll
        for (int kx = 0; kx <= KW; ++kx) red[kx * VW_THREADS + tid] = red[kx * VW_THREADS + tid] + red[kx * VW_THREADS + tid + k];
      }
      __syncthreads();
    }
    if (tid < KW) p.ws[((s * KK + ky * KW + tid) * p.Cout + co) * p.Cin + ci] = red[tid * VW_THREADS];
    if (tid == KW && do_db && ky == 0) p.wsdb[s * p.Cout + co] = red[KW * VW_THREADS];
  }
}

// partials [s][tap][co][ci] -> dW [co][ci][tap], db partials [s][co] -> db: partial 0, + partial 1, ... + partial S - 1,
// + the old value
__global__ __launch_bounds__(S1_THREADS) void s1_wgrad_combine_kernel(const float* ws, const float* wsdb, float* dW,
                                                                      float* db, int splits, int Cout, int Cin, int KK,
                                                                      int accumulate) {
  const long long n = (long long)KK * Cout * Cin;
  const long long e = (long long)blockIdx.x * S1_THREADS + threadIdx.x;
  if (e < n) {
    float tot = ws[e];
    for (int s = 1; s < splits; ++s) tot = tot + ws[(long long)s * n + e];
    const int ci = (int)(e % Cin);
    const long long r = e / Cin;
    const int co = (int)(r % Cout), tap = (int)(r / Cout);
    float* d = dW + ((long long)co * Cin + ci) * KK + tap;
    *d = accumulate ? tot + *d : tot;
  } else if (db && e < n + Cout) {
    const int co = (int)(e - n);
    float tot = wsdb[co];
    for (int s = 1; s < splits; ++s) tot = tot + wsdb[(long long)s * Cout + co];
    db[co] = accumulate ? tot + db[co] : tot;
  }
}

extern "C" int64_t scf_conv_s1_wgrad_workspace(int M, int Cout, int Cin, int H, int W, int KH, int KW) {
  if (M <= 0 || Cout <= 0 || Cin <= 0 || H <= 0 || W <= 0 || !s1_kernel_ok(KH) || !s1_kernel_ok(KW)) return -1;
  const S1Plan pl = s1_wgrad_plan(M, Cout, Cin, H, W, KH);
  return pl.splits * ((long long)KH * KW * Cout * Cin + Cout);
}

extern "C" int scf_conv_s1_wgrad(const float* g, int64_t g_stride, const float* x, int64_t x_stride, float* dW, float* db,
                                 int accumulate, float* workspace, int64_t workspace_floats, int M, int Cout, int Cin, int H,
                                 int W, int KH, int KW, scf_stream_t stream) {
  if (!g || !x || !dW || !workspace || M <= 0 || Cout <= 0 || Cin <= 0 || H <= 0 || W <= 0 || KH <= 0 || KW <= 0)
    return SCF_EINVAL;
  const long long plane = (long long)H * W;
  if (g_stride < Cout * plane || x_stride < Cin * plane) return SCF_EINVAL;
  if (!s1_kernel_ok(KH) || !s1_kernel_ok(KW)) return SCF_EUNSUPPORTED;
  const S1Plan pl = s1_wgrad_plan(M, Cout, Cin, H, W, KH);
  const int KK = KH * KW;
  const long long n = (long long)KK * Cout * Cin;
  if (workspace_floats < pl.splits * (n + Cout)) return SCF_EINVAL;
  if (pl.splits > 0x7fffffffll || pl.per_or_cps > 0x7fffffffll) return SCF_EUNSUPPORTED;
  const long long blocks = scf_cdiv(n + Cout, S1_THREADS);
  if (blocks > 0x7fffffffll) return SCF_EUNSUPPORTED;
  S1Wgrad p;
  p.g = g; p.x = x; p.ws = workspace; p.wsdb = db ? workspace + pl.splits * n : nullptr;
  p.gs = g_stride; p.xs = x_stride; p.Q = (long long)M * plane; p.per = pl.per_or_cps;
  p.M = M; p.Cout = Cout; p.Cin = Cin; p.H = H; p.W = W; p.KH = KH; p.KW = KW;
  p.segs = (int)scf_cdiv(W, SW_PIX); p.chunks = (long long)M * H * p.segs; p.cps = (int)pl.per_or_cps;
  p.cit = (int)scf_cdiv(Cin, SW_TILE);
  if (s1_wide(Cout, Cin)) {
    const long long cot = scf_cdiv(Cout, SW_TILE);
    if (p.cit > 65535 || cot * KH > 65535) return SCF_EUNSUPPORTED;
    const dim3 grid((unsigned)pl.splits, (unsigned)p.cit, (unsigned)(cot * KH));
    if (KW == 1) scf_launch(s1_wgrad_mfma_kernel<1>, grid, dim3(S1_THREADS), 0, scf_stream(stream), p);
    else if (KW == 3) scf_launch(s1_wgrad_mfma_kernel<3>, grid, dim3(S1_THREADS), 0, scf_stream(stream), p);
    else if (KW == 5) scf_launch(s1_wgrad_mfma_kernel<5>, grid, dim3(S1_THREADS), 0, scf_stream(stream), p);
    else scf_launch(s1_wgrad_mfma_kernel<7>, grid, dim3(S1_THREADS), 0, scf_stream(stream), p);
  } else {
    if (Cin > 65535 || Cout > 65535 || plane > 0x3fffffffll) return SCF_EUNSUPPORTED;
    const dim3 grid((unsigned)pl.splits, (unsigned)Cin, (unsigned)Cout);
    if (KW == 1) scf_launch(s1_wgrad_valu_kernel<1>, grid, dim3(VW_THREADS), 0, scf_stream(stream), p);
    else if (KW == 3) scf_launch(s1_wgrad_valu_kernel<3>, grid, dim3(VW_THREADS), 0, scf_stream(stream), p);
    else if (KW == 5) scf_launch(s1_wgrad_valu_kernel<5>, grid, dim3(VW_THREADS), 0, scf_stream(stream), p);
    else scf_launch(s1_wgrad_valu_kernel<7>, grid, dim3(VW_THREADS), 0, scf_stream(stream), p);
  }
  const int rc = scf_launch_status();
  if (rc != SCF_OK) return rc;
  scf_launch(s1_wgrad_combine_kernel, dim3((unsigned)blocks), dim3(S1_THREADS), 0, scf_stream(stream),
             (const float*)workspace, (const float*)(workspace + pl.splits * n), dW, db, (int)pl.splits, Cout, Cin, KK,
             accumulate);
  return scf_launch_status();
}
