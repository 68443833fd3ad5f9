// Backward of a 3x3 / stride-2 / pad-1 convolution (the pose head's three ConvModules, pose_head.py:131-149), for gfx950:
// the input gradient and the weight gradient, fp32 throughout on v_mfma_f32_32x32x2_f32.  The weights are shared by the
// T iterations of a refinement pass, so all M = T N stacked samples go through ONE launch (wgrad: one more that combines).
//
//   scf_conv_dgrad            gx[m, ci, iy, ix] = sum_{ky, kx, co} g[m, co, (iy + 1 - ky) / 2, (ix + 1 - kx) / 2] w[co, ci, ky, kx]
//                             over the taps whose (iy + 1 - ky, ix + 1 - kx) are even and inside the output map
//   scf_conv_wgrad            dW[co, ci, ky, kx] = sum_{m, oy, ox} g[m, co, oy, ox] x[m, ci, 2 oy - 1 + ky, 2 ox - 1 + kx]
//   scf_conv_wgrad_workspace  the floats of device memory the second needs
//
// No atomics, no allocation, no synchronisation: every sum has ONE order, fixed by the shapes alone.
//   dgrad   The input pixels fall into four parity classes (iy & 1, ix & 1) with 1, 2, 2 and 4 contributing taps: a
//           block owns DG_PIX = 64 pixels of ONE class (pixels numbered (m, iy >> 1, ix >> 1) row-major inside the class)
//           x DG_CI = 128 input channels (wave w: channels [32 w, 32 w + 32), two 32 x 32 accumulators: pixels [0, 32) and
//           [32, 64)), so no product with a zero of the dilated gradient is computed.  Per output ONE fma chain that starts
//           at +0: the class' taps in ascending (ky, kx), inside a tap co ascending in chunks of DG_CHUNK = 32 (zero columns
//           past Cout; a tap that leaves the output map at the last row / column of an even-sized input contributes
//           zeros: g is read as +0 there).  Length: taps x 32 ceil(Cout / 32).  A pixel's chain reads that pixel's sample
//           alone: the result does not depend on M.  w is read in the torch layout (Cout, Cin, 3, 3), no copy of it is made.
//           MFMA operands: A = w tile [co][ci] (rows ci), B = g tile [co][pixel] (columns pixel), both staged in LDS with
//           lanes along the tile's rows, the next chunk's global loads in flight while this one is contracted; a lane of
//           the result holds 16 channels of one pixel, so the stores of a wave walk the map's rows.
//   wgrad   One GEMM per tap, contracted over the Q = M Ho Wo output pixels q = (m, oy, ox) row-major.  A block owns
//           WG_TILE = 64 output x 64 input channels (2 x 2 waves of 32 x 32) and ALL nine taps (nine accumulators per
//           wave: the g tile is staged once for the nine), and one SPLIT of the contraction: chunks of WG_PIX = 16 pixels,
//           cps = max(WG_MIN_CHUNKS, ceil(chunks / max(1, WG_BLOCKS / tiles))) consecutive chunks per split, S = ceil(chunks /
//           cps) splits.  Inside a split ONE fma chain per (tap, co, ci) that starts at +0, q ascending (zeros where the tap
//           reads the padding and past Q): 16 cps steps.  The partial goes to workspace[s][tap][co][ci]; the combine launch
//           takes partial 0, adds partials 1 .. S - 1 in ascending order, adds the destination's previous value LAST
//           under `accumulate`, and writes the torch layout.
#include "scf_common.h"

typedef float cg_f32x16 __attribute__((ext_vector_type(16)));

#define CG_THREADS 256
#define DG_PIX 64                     // pixels of one parity class per block: two MFMA column tiles
#define DG_CI 128                     // input channels per block: 4 waves x 32
#define DG_CHUNK 32                   // output channels staged at a time
#define DG_WPITCH (DG_CI + 32)        // pitches in fc_grad.hip's manner: rows k and k + 1 of an operand 32 words further
#define DG_GPITCH (DG_PIX + 32)
#define WG_TILE 64                    // output channels x input channels of a block: 2 x 2 waves
#define WG_PIX 16                     // output pixels staged at a time
#define WG_PITCH 65                   // odd: the loaders write with lanes along the pixels
#define WG_MIN_CHUNKS 16              // a split holds at least this many chunks (when there are as many)
#define WG_BLOCKS 512                 // the splits aim at this many blocks

static inline bool cg_geometry_ok(int Ho, int Wo, int Hin, int Win) {
  return Hin >= 1 && Win >= 1 && Ho == (Hin - 1) / 2 + 1 && Wo == (Win - 1) / 2 + 1;
}

// ============================================================================================================ dgrad
struct CgDgrad {
  const float* g; const float* w; float* gx0; float* gx1;
  int C0, C1, M, Cout, Ho, Wo, Hin, Win;
};

__global__ __launch_bounds__(CG_THREADS) void cg_dgrad_kernel(CgDgrad p) {
  __shared__ float Wt[DG_CHUNK * DG_WPITCH];      // [co][ci]
  __shared__ float Gt[DG_CHUNK * DG_GPITCH];      // [co][pixel]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l32 = lane & 31;
  const int py = (int)blockIdx.z >> 1, px = (int)blockIdx.z & 1;
  const int Hc = (p.Hin + 1 - py) >> 1, Wc = (p.Win + 1 - px) >> 1;       // rows / columns of this parity
  const long long P = (long long)p.M * Hc * Wc;
  const long long p0 = (long long)blockIdx.x * DG_PIX;
  if (p0 >= P) return;                             // the whole block: the odd classes are the smaller ones
  const int Cin = p.C0 + p.C1, ci0 = (int)blockIdx.y * DG_CI;
  const int nky = py ? 2 : 1, nkx = px ? 2 : 1;
  const int ncc = (p.Cout + DG_CHUNK - 1) / DG_CHUNK, steps = nky * nkx * ncc;
  // loader coordinates: g tile 32 x 64 (8 per thread), w tile 32 x 128 (16 per thread)
  const int gp = tid & 63, go = tid >> 6;          // + 4 i
  const int wk = tid & 127, wo = tid >> 7;         // + 2 i
  const long long gq = p0 + gp;
  const bool gvalid = gq < P;
  int gm = 0, giy = 0, gix = 0;
  if (gvalid) { gix = (int)(gq % Wc); const long long r = gq / Wc; giy = (int)(r % Hc); gm = (int)(r / Hc); }
  float gv[8], wv[16];
  auto fetch = [&](int s) {
    const int t = s / ncc, oc = (s - t * ncc) * DG_CHUNK;
    const int ty = t / nkx, tx = t - ty * nkx;
    const int ky = py ? 2 * ty : 1, kx = px ? 2 * tx : 1;
    const int oy = giy + (ky == 0 ? 1 : 0), ox = gix + (kx == 0 ? 1 : 0);      // (iy + 1 - ky) / 2
    const bool ok = gvalid && oy < p.Ho && ox < p.Wo;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int co = oc + go + 4 * i;
      gv[i] = (ok && co < p.Cout) ? p.g[(((long long)gm * p.Cout + co) * p.Ho + oy) * p.Wo + ox] : 0.f;
    }
    const int ci = ci0 + wk, tap = ky * 3 + kx;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int co = oc + wo + 2 * i;
      wv[i] = (co < p.Cout && ci < Cin) ? p.w[((long long)co * Cin + ci) * 9 + tap] : 0.f;
    }
  };
  cg_f32x16 acc0, acc1;
#pragma unroll
  for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
  fetch(0);
  for (int s = 0; s < steps; ++s) {
    __syncthreads();                                 // the previous chunk's operands are read
#pragma unroll
    for (int i = 0; i < 8; ++i) Gt[(go + 4 * i) * DG_GPITCH + gp] = gv[i];
#pragma unroll
    for (int i = 0; i < 16; ++i) Wt[(wo + 2 * i) * DG_WPITCH + wk] = wv[i];
    __syncthreads();
    if (s + 1 < steps) fetch(s + 1);                 // in flight while this chunk is contracted
    const float* ap = Wt + half * DG_WPITCH + wave * 32 + l32;
    const float* bp = Gt + half * DG_GPITCH + l32;
#pragma unroll
    for (int o = 0; o < DG_CHUNK; o += 2) {
      const float a = ap[o * DG_WPITCH];
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bp[o * DG_GPITCH], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bp[o * DG_GPITCH + 32], acc1, 0, 0, 0);
    }
  }
  const long long plane = (long long)p.Hin * p.Win;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const long long q = p0 + 32 * j + l32;
    if (q >= P) continue;
    const int ix = 2 * (int)(q % Wc) + px;
    const long long rr = q / Wc;
    const int iy = 2 * (int)(rr % Hc) + py, m = (int)(rr / Hc);
    const long long pix = (long long)iy * p.Win + ix;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ci = ci0 + wave * 32 + 8 * (r >> 2) + 4 * half + (r & 3);
      if (ci >= Cin) continue;
      const float v = j ? acc1[r] : acc0[r];
      if (ci < p.C0) p.gx0[((long long)m * p.C0 + ci) * plane + pix] = v;
      else p.gx1[((long long)m * p.C1 + (ci - p.C0)) * plane + pix] = v;
    }
  }
}

extern "C" int scf_conv_dgrad(const float* g, const float* w, float* gx0, int C0, float* gx1, int C1, int M, int Cout,
                              int Ho, int Wo, int Hin, int Win, int KH, int KW, int stride, int pad,
                              scf_stream_t stream) {
  if (!g || !w || !gx0 || C0 <= 0 || C1 < 0 || (C1 > 0) != (gx1 != nullptr) || M <= 0 || Cout <= 0 || Ho <= 0 || Wo <= 0 ||
      Hin <= 0 || Win <= 0)
    return SCF_EINVAL;
  if (KH != 3 || KW != 3 || stride != 2 || pad != 1) return SCF_EUNSUPPORTED;
  if (!cg_geometry_ok(Ho, Wo, Hin, Win)) return SCF_EINVAL;
  const long long pt = scf_cdiv((long long)M * ((Hin + 1) / 2) * ((Win + 1) / 2), DG_PIX);
  const long long ct = scf_cdiv((long long)C0 + C1, DG_CI);
  if (pt > 0x7fffffffll || ct > 65535) return SCF_EUNSUPPORTED;
  CgDgrad p;
  p.g = g; p.w = w; p.gx0 = gx0; p.gx1 = gx1; p.C0 = C0; p.C1 = C1; p.M = M; p.Cout = Cout;
  p.Ho = Ho; p.Wo = Wo; p.Hin = Hin; p.Win = Win;
  scf_launch(cg_dgrad_kernel, dim3((unsigned)pt, (unsigned)ct, 4), dim3(CG_THREADS), 0, scf_stream(stream), p);
  return scf_launch_status();
}

// ============================================================================================================ wgrad
struct CgWgrad {
  const float* g; const float* x0; const float* x1; float* ws;
  int C0, C1, M, Cout, Ho, Wo, Hin, Win, cps;
  long long Q;
};

// (chunks per split, splits) of a contraction over Q output pixels for `tiles` output tiles
static inline void cg_wgrad_plan(long long Q, long long tiles, long long* cps, long long* splits) {
  const long long chunks = scf_cdiv(Q, WG_PIX);
  long long want = WG_BLOCKS / tiles;
  if (want < 1) want = 1;
  long long c = scf_cdiv(chunks, want);
  if (c < WG_MIN_CHUNKS) c = WG_MIN_CHUNKS;
  *cps = c;
  *splits = scf_cdiv(chunks, c);
}

__global__ __launch_bounds__(CG_THREADS) void cg_wgrad_kernel(CgWgrad p) {
  __shared__ float Gt[WG_PIX * WG_PITCH];          // [pixel][co]
  __shared__ float Xt[9 * WG_PIX * WG_PITCH];      // [tap][pixel][ci]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l32 = lane & 31;
  const int wr = wave >> 1, wc = wave & 1;
  const int Cin = p.C0 + p.C1, ci0 = (int)blockIdx.y * WG_TILE, co0 = (int)blockIdx.z * WG_TILE;
  const long long chunk0 = (long long)blockIdx.x * p.cps;
  const long long nchunks = (p.Q + WG_PIX - 1) / WG_PIX;
  const long long chunk1 = chunk0 + p.cps < nchunks ? chunk0 + p.cps : nchunks;
  // loader coordinates: lanes along the pixels, 16 channels apart per step
  const int lp = tid & 15, lc = tid >> 4;          // g: co lc + 16 i (i < 4); x: ci lc + 16 (i & 3), tap i >> 2 (i < 36)
  const long long plane = (long long)p.Hin * p.Win;
  float gv[4], xv[36];
  auto fetch = [&](long long c) {
    const long long q = c * WG_PIX + lp;
    const bool ok = q < p.Q;
    int ox = 0, oy = 0, m = 0;
    if (ok) { ox = (int)(q % p.Wo); const long long r = q / p.Wo; oy = (int)(r % p.Ho); m = (int)(r / p.Ho); }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int co = co0 + lc + 16 * i;
      gv[i] = (ok && co < p.Cout) ? p.g[(((long long)m * p.Cout + co) * p.Ho + oy) * p.Wo + ox] : 0.f;
    }
    const float* xb[4];
    bool cok[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int ci = ci0 + lc + 16 * j;
      cok[j] = ok && ci < Cin;
      xb[j] = ci < p.C0 ? p.x0 + ((long long)m * p.C0 + ci) * plane
                        : p.x1 + ((long long)m * p.C1 + (ci - p.C0)) * plane;      // read only under cok
    }
#pragma unroll
    for (int i = 0; i < 36; ++i) {
      const int tap = i >> 2, ky = tap / 3, kx = tap - 3 * ky;
      const int iy = 2 * oy - 1 + ky, ix = 2 * ox - 1 + kx;
      const bool in = iy >= 0 && iy < p.Hin && ix >= 0 && ix < p.Win;
      xv[i] = (cok[i & 3] && in) ? xb[i & 3][(long long)iy * p.Win + ix] : 0.f;
    }
  };
  cg_f32x16 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  fetch(chunk0);
  for (long long c = chunk0; c < chunk1; ++c) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) Gt[lp * WG_PITCH + lc + 16 * i] = gv[i];
#pragma unroll
    for (int i = 0; i < 36; ++i) Xt[((i >> 2) * WG_PIX + lp) * WG_PITCH + lc + 16 * (i & 3)] = xv[i];
    __syncthreads();
    if (c + 1 < chunk1) fetch(c + 1);
    const float* ap = Gt + half * WG_PITCH + wr * 32 + l32;
    const float* bp = Xt + half * WG_PITCH + wc * 32 + l32;
#pragma unroll
    for (int k = 0; k < WG_PIX; k += 2) {
      const float a = ap[k * WG_PITCH];
#pragma unroll
      for (int t = 0; t < 9; ++t)
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bp[(t * WG_PIX + k) * WG_PITCH], acc[t], 0, 0, 0);
    }
  }
  const int ci = ci0 + wc * 32 + l32;
  if (ci >= Cin) return;
  float* dst = p.ws + (long long)blockIdx.x * 9 * p.Cout * Cin;
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = co0 + wr * 32 + 8 * (r >> 2) + 4 * half + (r & 3);
      if (co < p.Cout) dst[((long long)t * p.Cout + co) * Cin + ci] = acc[t][r];
    }
}

// partials [s][tap][co][ci] -> dW [co][ci][tap]: partial 0, + partial 1, ... + partial S - 1, + the old value
__global__ __launch_bounds__(CG_THREADS) void cg_wgrad_combine_kernel(const float* ws, float* dW, int splits, int Cout,
                                                                      int Cin, int accumulate) {
  const long long n = 9ll * Cout * Cin;
  const long long e = (long long)blockIdx.x * CG_THREADS + threadIdx.x;
  if (e >= n) return;
  float tot = ws[e];
  for (int s = 1; s < splits; ++s) tot = tot + ws[(long long)s * n + e];
  const int ci = (int)(e % Cin);
  const long long r = e / Cin;
  const int co = (int)(r % Cout), tap = (int)(r / Cout);
  float* d = dW + ((long long)co * Cin + ci) * 9 + tap;
  *d = accumulate ? tot + *d : tot;
}

extern "C" int64_t scf_conv_wgrad_workspace(int M, int Cout, int Cin, int Ho, int Wo) {
  if (M <= 0 || Cout <= 0 || Cin <= 0 || Ho <= 0 || Wo <= 0) return -1;
  long long cps, splits;
  cg_wgrad_plan((long long)M * Ho * Wo, scf_cdiv(Cout, WG_TILE) * scf_cdiv(Cin, WG_TILE), &cps, &splits);
  return splits * 9 * Cout * Cin;
}

extern "C" int scf_conv_wgrad(const float* g, const float* x0, int C0, const float* x1, int C1, float* dW, int accumulate,
                              float* workspace, int64_t workspace_floats, int M, int Cout, int Ho, int Wo, int Hin,
                              int Win, int KH, int KW, int stride, int pad, scf_stream_t stream) {
  if (!g || !x0 || !dW || !workspace || C0 <= 0 || C1 < 0 || (C1 > 0) != (x1 != nullptr) || M <= 0 || Cout <= 0 ||
      Ho <= 0 || Wo <= 0 || Hin <= 0 || Win <= 0)
    return SCF_EINVAL;
  if (KH != 3 || KW != 3 || stride != 2 || pad != 1) return SCF_EUNSUPPORTED;
  if (!cg_geometry_ok(Ho, Wo, Hin, Win)) return SCF_EINVAL;
  const long long Cin = (long long)C0 + C1;
  const long long cot = scf_cdiv(Cout, WG_TILE), cit = scf_cdiv(Cin, WG_TILE);
  if (cot > 65535 || cit > 65535) return SCF_EUNSUPPORTED;
  long long cps, splits;
  cg_wgrad_plan((long long)M * Ho * Wo, cot * cit, &cps, &splits);
  if (splits > 0x7fffffffll || cps > 0x7fffffffll) return SCF_EUNSUPPORTED;
  const long long n = 9ll * Cout * Cin;
  if (workspace_floats < splits * n) return SCF_EINVAL;
  const long long blocks = scf_cdiv(n, CG_THREADS);
  if (blocks > 0x7fffffffll) return SCF_EUNSUPPORTED;
  CgWgrad p;
  p.g = g; p.x0 = x0; p.x1 = x1; p.ws = workspace; p.C0 = C0; p.C1 = C1; p.M = M; p.Cout = Cout;
  p.Ho = Ho; p.Wo = Wo; p.Hin = Hin; p.Win = Win; p.cps = (int)cps; p.Q = (long long)M * Ho * Wo;
  scf_launch(cg_wgrad_kernel, dim3((unsigned)splits, (unsigned)cit, (unsigned)cot), dim3(CG_THREADS), 0,
             scf_stream(stream), p);
  int rc = scf_launch_status();
  if (rc != SCF_OK) return rc;
  scf_launch(cg_wgrad_combine_kernel, dim3((unsigned)blocks), dim3(CG_THREADS), 0, scf_stream(stream),
             (const float*)workspace, dW, (int)splits, Cout, (int)Cin, accumulate);
  return scf_launch_status();
}
