// Backward of the context encoder's layers that the stride-1 family (conv_s1_grad.hip) and the pose head's 3x3 / stride-2
// family (conv_grad.hip) do not cover (raft_encoder.py:286-314, resnet.py:14-94 with eval-mode BatchNorm), for gfx950, fp32.
//
//   scf_conv_stem_wgrad   dW, db of the thin-input 7x7 / stride-2 / pad-3 stem (Cin <= 4)
//   scf_conv_ds_dgrad     the join at a stride-2 block's input: act'(a) (add + the 1x1 / stride-2 shortcut's input gradient)
//   scf_conv_ds_wgrad     dW, db of the 1x1 / stride-2 shortcut
//   scf_channel_sum       out[c] = sum_{m, i} g[m, c, i]: the bias gradient of the 3x3 / stride-2 layers
//   scf_bn_fold           (W, b, gamma, beta, mean, var) -> (W', b') of y = W' * x + b'
//   scf_bn_unfold         (dW', db') -> dW, db, dgamma, dbeta
//
// No atomics, no allocation, no synchronisation: every sum has ONE order, fixed by the shapes alone.
//
//   stem wgrad  A GEMM of Cout x K, K = Cin 49 columns k = (ci, ky, kx) row-major (the torch layout of a row of dW), the
//          contraction over the M Ho Wo output pixels on v_mfma_f32_32x32x2_f32.  An output row is cut into segments of
//          EW_PIX = 16 pixels; chunk c = (m, oy, segment) row-major.  The contraction is cut into S splits of
//          cps = max(ST_MIN_CHUNKS, ceil(chunks / ST_SPLITS)) consecutive chunks, S = ceil(chunks / cps); ONE WAVE owns a
//          split (a block: 4 splits x one tile of 64 output channels) and all the split's accumulators: 2 row tiles x
//          ceil(K / 32) column tiles.  A chunk stages, once, the g segment [pixel][co] and the 7 Cin input rows that the
//          output row reads, 2 * 16 + 5 values each (zeros outside the map and past Wo) at a pitch of 39 floats: column k
//          of pixel p is then at 39 (k / 7) + k % 7 + 2 p, i.e. the 32 lanes of an MFMA operand load read 32 different
//          banks (39 = 7 mod 32), and every input value is read from global memory once per chunk, not once per tap.
//          Inside a split ONE fma chain per (co, k) from +0, chunks ascending, pixels ascending: 16 cps steps.
//          db: lane co of the wave adds the staged g values, one chain of plain adds from +0 in the same order.
//          Partials: workspace[s][co][k], then S Cout floats [s][co] of db.
//   ds dgrad  A block owns ED_PIX = 64 OUTPUT pixels (numbered (m, oy, ox) row-major) x ED_CI = 128 input channels; co goes
//          in chunks of 32 (zero columns past Cout): per even input pixel ONE fma chain from +0 over co ascending, length
//          32 ceil(Cout / 32); then + add (one rounding), then the factor of scf_act_grad.  The block also writes the up
//          to three other input pixels of each 2 x 2 quad: act'(a) add (add NULL: act'(a) (+0)).  A sample's result does
//          not depend on M.
//   ds wgrad  As the wide route of scf_conv_s1_wgrad with one tap: chunk c = (m, oy, segment of 16 output pixels), a block
//          owns 64 x 64 channels and one split of cps = max(EW_MIN_CHUNKS, ceil(chunks / max(1, EW_BLOCKS / tiles)))
//          chunks; x is read at (2 oy, 2 ox).  ONE fma chain per (co, ci) from +0, chunks then pixels ascending (zeros
//          past Wo): 16 cps steps.  db: the blocks of ci tile 0, plain adds in the same order.  Partials [s][co][ci].
//   channel sum  q = (m, i) row-major over Q = M n; a block owns one channel and one split of per = max(CS_MIN, ceil(Q /
//          max(1, CS_BLOCKS / C))) rounded up to a multiple of 256.  Thread t: one chain of plain adds from +0 over
//          q = q0 + t, q0 + t + 256, ...; then the 256 values are added pairwise in LDS, v[t] += v[t + k], k = 128 .. 1.
//   combine (all three): partial 0, + partial 1, ... + partial S - 1, then + the destination's previous value LAST
//          under `accumulate`.
//   fold   sd = sqrt(var + eps), s = gamma / sd (one rounding each); W' = s W; b' = fma(s, b - mean, beta).
//   unfold dW = s dW', db = s db', dbeta = db', dgamma = fma(b - mean, db', <W_c, dW'_c>) / sd.  <W_c, dW'_c>: one wave a
//          channel, lane l one fma chain from +0 over k = l, l + 64, ... (k the torch order (ci, ky, kx) of a row), then
//          v[l] += v[l + j] for j = 32, 16, ..., 1.  With `accumulate` the previous value is added last.  A channel reads
//          and writes its own row only: a non-finite value stays in its channel.
#include "scf_common.h"

typedef float eg_f32x16 __attribute__((ext_vector_type(16)));

#define EG_THREADS 256
#define EW_PIX 16                     // output pixels of a row segment staged at a time
#define EW_PITCH 65
#define ST_K 7                        // the stem's kernel
#define ST_XW (2 * EW_PIX + ST_K - 2) // 37 input values of a row a segment reads
#define ST_XPITCH 39                  // = 7 mod 32: column k at 39 (k / 7) + k % 7 is bank k mod 32
#define ST_MAX_CIN 4
#define ST_MIN_CHUNKS 4               // a split holds at least this many chunks (when there are as many)
#define ST_SPLITS 1024                // the splits aim at this many waves
#define ED_PIX 64
#define ED_CI 128
#define ED_CHUNK 32
#define ED_WPITCH (ED_CI + 32)
#define ED_GPITCH (ED_PIX + 32)
#define EW_TILE 64
#define EW_MIN_CHUNKS 16
#define EW_BLOCKS 1024
#define CS_MIN 4096
#define CS_BLOCKS 2048

__device__ __forceinline__ float eg_act_factor(float v, float a, int act) {
  if (act == SCF_ACT_RELU) return a > 0.f ? v : 0.f;
  if (act == SCF_ACT_SIGMOID) return v * (a * (1.f - a));
  if (act == SCF_ACT_TANH) return v * __fmaf_rn(-a, a, 1.f);
  return v;
}

static inline bool eg_act_ok(int act) {
  return act == SCF_ACT_NONE || act == SCF_ACT_RELU || act == SCF_ACT_SIGMOID || act == SCF_ACT_TANH;
}

// partials [s][n] -> dst (n floats), db partials [s][C] -> db: partial 0, + partial 1, ..., + the old value
__global__ __launch_bounds__(EG_THREADS) void eg_combine_kernel(const float* ws, const float* wsdb, float* dst, float* db,
                                                                int splits, long long n, int C, int accumulate) {
  const long long e = (long long)blockIdx.x * EG_THREADS + threadIdx.x;
  const float* src;
  float* d;
  long long step;
  if (e < n) { src = ws + e; d = dst + e; step = n; }
  else if (db && e < n + C) { src = wsdb + (e - n); d = db + (e - n); step = C; }
  else return;
  float tot = src[0];
#pragma unroll 8
  for (int s = 1; s < splits; ++s) tot = tot + src[(long long)s * step];
  *d = accumulate ? tot + *d : tot;
}

static inline int eg_combine(const float* ws, const float* wsdb, float* dst, float* db, long long splits, long long n, int C,
                             int accumulate, scf_stream_t stream) {
  const long long blocks = scf_cdiv(n + C, EG_THREADS);
  scf_launch(eg_combine_kernel, dim3((unsigned)blocks), dim3(EG_THREADS), 0, scf_stream(stream), ws, wsdb, dst, db,
             (int)splits, n, C, accumulate);
  return scf_launch_status();
}

// ======================================================================================================= stem wgrad
struct EgStem {
  const float* g; const float* x; float* ws; float* wsdb;
  long long gs, xs, chunks, splits;
  int Cout, H, W, Ho, Wo, cps, segs;
};

static inline long long eg_stem_cps(long long chunks) {
  long long c = scf_cdiv(chunks, ST_SPLITS);
  return c < ST_MIN_CHUNKS ? ST_MIN_CHUNKS : c;
}

template <int CIN>
__global__ __launch_bounds__(EG_THREADS) void eg_stem_wgrad_kernel(EgStem p) {
  constexpr int K = CIN * ST_K * ST_K, NKT = (K + 31) / 32, ROWS = CIN * ST_K;
  constexpr int NXE = ROWS * ST_XW, NX = (NXE + 63) / 64;
  __shared__ float Gs[4][EW_PIX * EW_PITCH];          // per wave [pixel][co]
  __shared__ float Xs[4][ROWS * ST_XPITCH];           // per wave [(ci, ky)][input column]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l32 = lane & 31;
  const int co0 = (int)blockIdx.y * EW_TILE;
  const long long s = (long long)blockIdx.x * 4 + wave;
  const bool live = s < p.splits;
  const long long chunk0 = s * p.cps;
  long long chunk1 = chunk0 + p.cps < p.chunks ? chunk0 + p.cps : p.chunks;
  if (!live) chunk1 = chunk0;
  const long long gplane = (long long)p.Ho * p.Wo, xplane = (long long)p.H * p.W;
  const int lp = lane & 15, lc = lane >> 4;            // g: pixel lp, co lc + 4 i
  float* G = Gs[wave];
  float* X = Xs[wave];
  float gv[16], xv[NX];
  auto fetch = [&](long long c) {
    const int seg = (int)(c % p.segs);
    const long long rr = c / p.segs;
    const int oy = (int)(rr % p.Ho);
    const long long m = rr / p.Ho;
    const int ox0 = seg * EW_PIX;
    const bool gok = ox0 + lp < p.Wo;
    const float* gb = p.g + m * p.gs + (long long)oy * p.Wo + ox0 + lp;      // read only under gok
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int co = co0 + lc + 4 * i;
      gv[i] = (gok && co < p.Cout) ? gb[(long long)co * gplane] : 0.f;
    }
    const float* xb = p.x + m * p.xs;
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      const int e = lane + 64 * i;
      const int r = e / ST_XW, j = e - r * ST_XW;
      const int ci = r / ST_K, ky = r - ci * ST_K;
      const int iy = 2 * oy - 3 + ky, ix = 2 * ox0 - 3 + j;
      xv[i] = (e < NXE && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W) ? xb[(long long)ci * xplane + (long long)iy * p.W + ix]
                                                                     : 0.f;
    }
  };
  eg_f32x16 acc[2][NKT];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int t = 0; t < NKT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][t][r] = 0.f;
  float dbacc = 0.f;
  // the patch column of this lane in every column tile (columns past K read column K - 1: never stored)
  int boff[NKT];
#pragma unroll
  for (int t = 0; t < NKT; ++t) {
    int k = t * 32 + l32;
    if (k > K - 1) k = K - 1;
    boff[t] = ST_XPITCH * (k / ST_K) + k % ST_K + 2 * half;
  }
  if (chunk0 < chunk1) fetch(chunk0);
  for (int it = 0; it < p.cps; ++it) {                 // the same trip count in every wave: the barriers are the block's
    const long long c = chunk0 + it;
    const bool on = c < chunk1;
    __syncthreads();                                   // the previous chunk's operands are read
    if (on) {
#pragma unroll
      for (int i = 0; i < 16; ++i) G[lp * EW_PITCH + lc + 4 * i] = gv[i];
#pragma unroll
      for (int i = 0; i < NX; ++i) {
        const int e = lane + 64 * i;
        const int r = e / ST_XW, j = e - r * ST_XW;
        if (e < NXE) X[r * ST_XPITCH + j] = xv[i];
      }
    }
    __syncthreads();
    if (!on) continue;
    if (c + 1 < chunk1) fetch(c + 1);
    if (p.wsdb) {
#pragma unroll
      for (int k = 0; k < EW_PIX; ++k) dbacc = dbacc + G[k * EW_PITCH + lane];
    }
    const float* ap = G + half * EW_PITCH + l32;
#pragma unroll
    for (int k = 0; k < EW_PIX; k += 2) {
      const float a0 = ap[k * EW_PITCH], a1 = ap[k * EW_PITCH + 32];
#pragma unroll
      for (int t = 0; t < NKT; ++t) {
        const float b = X[boff[t] + 2 * k];
        acc[0][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b, acc[0][t], 0, 0, 0);
        acc[1][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b, acc[1][t], 0, 0, 0);
      }
    }
  }
  if (!live) return;
  if (p.wsdb && co0 + lane < p.Cout) p.wsdb[s * p.Cout + co0 + lane] = dbacc;
  float* dst = p.ws + s * (long long)p.Cout * K;
#pragma unroll
  for (int t = 0; t < NKT; ++t) {
    const int k = t * 32 + l32;
    if (k >= K) continue;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = co0 + a * 32 + 8 * (r >> 2) + 4 * half + (r & 3);
        if (co < p.Cout) dst[(long long)co * K + k] = acc[a][t][r];
      }
  }
}

static inline bool eg_half_map(int Hin, int Win, int Ho, int Wo) {
  return Hin >= 1 && Win >= 1 && Ho == (Hin - 1) / 2 + 1 && Wo == (Win - 1) / 2 + 1;
}

extern "C" int64_t scf_conv_stem_wgrad_workspace(int M, int Cout, int Cin, int Ho, int Wo) {
  if (M <= 0 || Cout <= 0 || Cin <= 0 || Cin > ST_MAX_CIN || Ho <= 0 || Wo <= 0) return -1;
  const long long chunks = (long long)M * Ho * scf_cdiv(Wo, EW_PIX);
  const long long cps = eg_stem_cps(chunks);
  return scf_cdiv(chunks, cps) * ((long long)Cout * Cin * ST_K * ST_K + Cout);
}

extern "C" int scf_conv_stem_wgrad(const float* g, int64_t g_stride, const float* x, int64_t x_stride, float* dW, float* db,
                                   int accumulate, float* workspace, int64_t workspace_floats, int M, int Cout, int Cin,
                                   int Ho, int Wo, int Hin, int Win, int KH, int KW, int stride, int pad,
                                   scf_stream_t stream) {
  if (!g || !x || !dW || !workspace || M <= 0 || Cout <= 0 || Cin <= 0 || Ho <= 0 || Wo <= 0 || Hin <= 0 || Win <= 0 ||
      KH <= 0 || KW <= 0 || stride <= 0 || pad < 0)
    return SCF_EINVAL;
  if (g_stride < (long long)Cout * Ho * Wo || x_stride < (long long)Cin * Hin * Win) return SCF_EINVAL;
  if (KH != ST_K || KW != ST_K || stride != 2 || pad != 3 || Cin > ST_MAX_CIN) return SCF_EUNSUPPORTED;
  if (!eg_half_map(Hin, Win, Ho, Wo)) return SCF_EINVAL;
  const int K = Cin * ST_K * ST_K;
  const long long n = (long long)Cout * K;
  EgStem p;
  p.segs = (int)scf_cdiv(Wo, EW_PIX);
  p.chunks = (long long)M * Ho * p.segs;
  const long long cps = eg_stem_cps(p.chunks);
  p.splits = scf_cdiv(p.chunks, cps);
  if (workspace_floats < p.splits * (n + Cout)) return SCF_EINVAL;
  const long long cot = scf_cdiv(Cout, EW_TILE);
  if (cps > 0x7fffffffll || cot > 65535) return SCF_EUNSUPPORTED;
  p.g = g; p.x = x; p.ws = workspace; p.wsdb = db ? workspace + p.splits * n : nullptr;
  p.gs = g_stride; p.xs = x_stride; p.Cout = Cout; p.H = Hin; p.W = Win; p.Ho = Ho; p.Wo = Wo; p.cps = (int)cps;
  const dim3 grid((unsigned)scf_cdiv(p.splits, 4), (unsigned)cot);
  if (Cin == 1) scf_launch(eg_stem_wgrad_kernel<1>, grid, dim3(EG_THREADS), 0, scf_stream(stream), p);
  else if (Cin == 2) scf_launch(eg_stem_wgrad_kernel<2>, grid, dim3(EG_THREADS), 0, scf_stream(stream), p);
  else if (Cin == 3) scf_launch(eg_stem_wgrad_kernel<3>, grid, dim3(EG_THREADS), 0, scf_stream(stream), p);
  else scf_launch(eg_stem_wgrad_kernel<4>, grid, dim3(EG_THREADS), 0, scf_stream(stream), p);
  const int rc = scf_launch_status();
  if (rc != SCF_OK) return rc;
  return eg_combine(workspace, workspace + p.splits * n, dW, db, p.splits, n, Cout, accumulate, stream);
}

// ========================================================================================================= ds dgrad
struct EgDsDgrad {
  const float* g; const float* w; const float* add; const float* a; float* gx;
  long long gs, adds, as, gxs;
  int M, Cout, Cin, Ho, Wo, H, W, act;
};

__global__ __launch_bounds__(EG_THREADS) void eg_ds_dgrad_kernel(EgDsDgrad p) {
  __shared__ float Wt[ED_CHUNK * ED_WPITCH];      // [co][ci]
  __shared__ float Gt[ED_CHUNK * ED_GPITCH];      // [co][pixel]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l32 = lane & 31;
  const long long oplane = (long long)p.Ho * p.Wo, plane = (long long)p.H * p.W;
  const long long P = (long long)p.M * oplane;
  const long long p0 = (long long)blockIdx.x * ED_PIX;
  const int ci0 = (int)blockIdx.y * ED_CI;
  const int steps = (p.Cout + ED_CHUNK - 1) / ED_CHUNK;
  const int gp = tid & 63, go = tid >> 6;          // g tile 32 x 64: co go + 4 i
  const int wk = tid & 127, wo = tid >> 7;         // w tile 32 x 128: co wo + 2 i
  const long long gq = p0 + gp;
  const bool gvalid = gq < P;
  const long long gm = gvalid ? gq / oplane : 0;
  const float* gb = p.g + gm * p.gs + (gvalid ? gq - gm * oplane : 0);
  float gv[8], wv[16];
  auto fetch = [&](int s) {
    const int oc = s * ED_CHUNK;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int co = oc + go + 4 * i;
      gv[i] = (gvalid && co < p.Cout) ? gb[(long long)co * oplane] : 0.f;
    }
    const int ci = ci0 + wk;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int co = oc + wo + 2 * i;
      wv[i] = (co < p.Cout && ci < p.Cin) ? p.w[(long long)co * p.Cin + ci] : 0.f;
    }
  };
  eg_f32x16 acc0, acc1;
#pragma unroll
  for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
  fetch(0);
  for (int s = 0; s < steps; ++s) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 8; ++i) Gt[(go + 4 * i) * ED_GPITCH + gp] = gv[i];
#pragma unroll
    for (int i = 0; i < 16; ++i) Wt[(wo + 2 * i) * ED_WPITCH + wk] = wv[i];
    __syncthreads();
    if (s + 1 < steps) fetch(s + 1);
    const float* ap = Wt + half * ED_WPITCH + wave * 32 + l32;
    const float* bp = Gt + half * ED_GPITCH + l32;
#pragma unroll
    for (int o = 0; o < ED_CHUNK; o += 2) {
      const float a = ap[o * ED_WPITCH];
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bp[o * ED_GPITCH], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bp[o * ED_GPITCH + 32], acc1, 0, 0, 0);
    }
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const long long q = p0 + 32 * j + l32;
    if (q >= P) continue;
    const long long m = q / oplane, pix = q - m * oplane;
    const int oy = (int)(pix / p.Wo), ox = (int)(pix - (long long)oy * p.Wo);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ci = ci0 + wave * 32 + 8 * (r >> 2) + 4 * half + (r & 3);
      if (ci >= p.Cin) continue;
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const int iy = 2 * oy + (d >> 1), ix = 2 * ox + (d & 1);
        if (iy >= p.H || ix >= p.W) continue;
        const long long off = (long long)ci * plane + (long long)iy * p.W + ix;
        float v;
        if (d == 0) {
          v = j ? acc1[r] : acc0[r];
          if (p.add) v = v + p.add[m * p.adds + off];
        } else {
          v = p.add ? p.add[m * p.adds + off] : 0.f;
        }
        if (p.act != SCF_ACT_NONE) v = eg_act_factor(v, p.a[m * p.as + off], p.act);
        p.gx[m * p.gxs + off] = v;
      }
    }
  }
}

extern "C" int scf_conv_ds_dgrad(const float* g, int64_t g_stride, const float* w, const float* add, int64_t add_stride,
                                 const float* a, int64_t a_stride, int act, float* gx, int64_t gx_stride, int M, int Cout,
                                 int Cin, int Ho, int Wo, int Hin, int Win, scf_stream_t stream) {
  if (!g || !w || !gx || M <= 0 || Cout <= 0 || Cin <= 0 || Ho <= 0 || Wo <= 0 || !eg_half_map(Hin, Win, Ho, Wo))
    return SCF_EINVAL;
  if (!eg_act_ok(act) || (act != SCF_ACT_NONE && !a)) return SCF_EINVAL;
  const long long plane = (long long)Hin * Win;
  if (g_stride < (long long)Cout * Ho * Wo || gx_stride < Cin * plane || (add && add_stride < Cin * plane) ||
      (act != SCF_ACT_NONE && a_stride < Cin * plane))
    return SCF_EINVAL;
  const long long pt = scf_cdiv((long long)M * Ho * Wo, ED_PIX), ct = scf_cdiv(Cin, ED_CI);
  if (pt > 0x7fffffffll || ct > 65535) return SCF_EUNSUPPORTED;
  EgDsDgrad p;
  p.g = g; p.w = w; p.add = add; p.a = act != SCF_ACT_NONE ? a : nullptr; p.gx = gx;
  p.gs = g_stride; p.adds = add_stride; p.as = a_stride; p.gxs = gx_stride;
  p.M = M; p.Cout = Cout; p.Cin = Cin; p.Ho = Ho; p.Wo = Wo; p.H = Hin; p.W = Win; p.act = act;
  scf_launch(eg_ds_dgrad_kernel, dim3((unsigned)pt, (unsigned)ct), dim3(EG_THREADS), 0, scf_stream(stream), p);
  return scf_launch_status();
}

// ========================================================================================================= ds wgrad
struct EgDsWgrad {
  const float* g; const float* x; float* ws; float* wsdb;
  long long gs, xs, chunks;
  int Cout, Cin, Ho, Wo, H, W, cps, segs;
};

static inline long long eg_ds_cps(long long chunks, int Cout, int Cin) {
  const long long tiles = scf_cdiv(Cout, EW_TILE) * scf_cdiv(Cin, EW_TILE);
  long long want = EW_BLOCKS / tiles;
  if (want < 1) want = 1;
  long long c = scf_cdiv(chunks, want);
  return c < EW_MIN_CHUNKS ? EW_MIN_CHUNKS : c;
}

__global__ __launch_bounds__(EG_THREADS) void eg_ds_wgrad_kernel(EgDsWgrad p) {
  __shared__ float Gt[EW_PIX * EW_PITCH];             // [pixel][co]
  __shared__ float Xt[EW_PIX * EW_PITCH];             // [pixel][ci]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l32 = lane & 31;
  const int wr = wave >> 1, wc = wave & 1;
  const int ci0 = (int)blockIdx.y * EW_TILE, co0 = (int)blockIdx.z * EW_TILE;
  const long long chunk0 = (long long)blockIdx.x * p.cps;
  const long long chunk1 = chunk0 + p.cps < p.chunks ? chunk0 + p.cps : p.chunks;
  const long long oplane = (long long)p.Ho * p.Wo, plane = (long long)p.H * p.W;
  const int lp = tid & 15, lc = tid >> 4;             // pixel lp, channel lc + 16 i
  const bool do_db = p.wsdb && blockIdx.y == 0;
  float gv[4], xv[4];
  auto fetch = [&](long long c) {
    const int seg = (int)(c % p.segs);
    const long long rr = c / p.segs;
    const int oy = (int)(rr % p.Ho);
    const long long m = rr / p.Ho;
    const int ox = seg * EW_PIX + lp;
    const bool ok = ox < p.Wo;
    const float* gb = p.g + m * p.gs + (long long)oy * p.Wo + ox;                   // read only under ok
    const float* xb = p.x + m * p.xs + (long long)(2 * oy) * p.W + 2 * ox;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int co = co0 + lc + 16 * i, ci = ci0 + lc + 16 * i;
      gv[i] = (ok && co < p.Cout) ? gb[(long long)co * oplane] : 0.f;
      xv[i] = (ok && ci < p.Cin) ? xb[(long long)ci * plane] : 0.f;
    }
  };
  eg_f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  float dbacc = 0.f;
  fetch(chunk0);
  for (long long c = chunk0; c < chunk1; ++c) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      Gt[lp * EW_PITCH + lc + 16 * i] = gv[i];
      Xt[lp * EW_PITCH + lc + 16 * i] = xv[i];
    }
    __syncthreads();
    if (c + 1 < chunk1) fetch(c + 1);
    if (do_db && tid < EW_TILE) {
#pragma unroll
      for (int k = 0; k < EW_PIX; ++k) dbacc = dbacc + Gt[k * EW_PITCH + tid];
    }
    const float* ap = Gt + half * EW_PITCH + wr * 32 + l32;
    const float* bp = Xt + half * EW_PITCH + wc * 32 + l32;
#pragma unroll
    for (int k = 0; k < EW_PIX; k += 2)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[k * EW_PITCH], bp[k * EW_PITCH], acc, 0, 0, 0);
  }
  if (do_db && tid < EW_TILE && co0 + tid < p.Cout) p.wsdb[(long long)blockIdx.x * p.Cout + co0 + tid] = dbacc;
  const int ci = ci0 + wc * 32 + l32;
  if (ci >= p.Cin) return;
  float* dst = p.ws + (long long)blockIdx.x * p.Cout * p.Cin;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int co = co0 + wr * 32 + 8 * (r >> 2) + 4 * half + (r & 3);
    if (co < p.Cout) dst[(long long)co * p.Cin + ci] = acc[r];
  }
}

extern "C" int64_t scf_conv_ds_wgrad_workspace(int M, int Cout, int Cin, int Ho, int Wo) {
  if (M <= 0 || Cout <= 0 || Cin <= 0 || Ho <= 0 || Wo <= 0) return -1;
  const long long chunks = (long long)M * Ho * scf_cdiv(Wo, EW_PIX);
  return scf_cdiv(chunks, eg_ds_cps(chunks, Cout, Cin)) * ((long long)Cout * Cin + Cout);
}

extern "C" int scf_conv_ds_wgrad(const float* g, int64_t g_stride, const float* x, int64_t x_stride, float* dW, float* db,
                                 int accumulate, float* workspace, int64_t workspace_floats, int M, int Cout, int Cin,
                                 int Ho, int Wo, int Hin, int Win, scf_stream_t stream) {
  if (!g || !x || !dW || !workspace || M <= 0 || Cout <= 0 || Cin <= 0 || Ho <= 0 || Wo <= 0 ||
      !eg_half_map(Hin, Win, Ho, Wo))
    return SCF_EINVAL;
  if (g_stride < (long long)Cout * Ho * Wo || x_stride < (long long)Cin * Hin * Win) return SCF_EINVAL;
  EgDsWgrad p;
  p.segs = (int)scf_cdiv(Wo, EW_PIX);
  p.chunks = (long long)M * Ho * p.segs;
  const long long cps = eg_ds_cps(p.chunks, Cout, Cin), splits = scf_cdiv(p.chunks, cps);
  const long long n = (long long)Cout * Cin;
  if (workspace_floats < splits * (n + Cout)) return SCF_EINVAL;
  const long long cot = scf_cdiv(Cout, EW_TILE), cit = scf_cdiv(Cin, EW_TILE);
  if (splits > 0x7fffffffll || cps > 0x7fffffffll || cot > 65535 || cit > 65535) return SCF_EUNSUPPORTED;
  p.g = g; p.x = x; p.ws = workspace; p.wsdb = db ? workspace + splits * n : nullptr;
  p.gs = g_stride; p.xs = x_stride; p.Cout = Cout; p.Cin = Cin; p.Ho = Ho; p.Wo = Wo; p.H = Hin; p.W = Win;
  p.cps = (int)cps;
  scf_launch(eg_ds_wgrad_kernel, dim3((unsigned)splits, (unsigned)cit, (unsigned)cot), dim3(EG_THREADS), 0,
             scf_stream(stream), p);
  const int rc = scf_launch_status();
  if (rc != SCF_OK) return rc;
  return eg_combine(workspace, workspace + splits * n, dW, db, splits, n, Cout, accumulate, stream);
}

// ====================================================================================================== channel sum
static inline long long eg_cs_per(long long Q, int C) {
  long long want = CS_BLOCKS / C;
  if (want < 1) want = 1;
  long long per = scf_cdiv(Q, want);
  if (per < CS_MIN) per = CS_MIN;
  return scf_cdiv(per, EG_THREADS) * EG_THREADS;
}

__global__ __launch_bounds__(EG_THREADS) void eg_channel_sum_kernel(const float* g, long long gs, float* ws, long long n,
                                                                    long long Q, long long per, int C) {
  __shared__ float red[EG_THREADS];
  const int tid = threadIdx.x, c = (int)blockIdx.y;
  const long long q0 = (long long)blockIdx.x * per, q1 = q0 + per < Q ? q0 + per : Q;
  float acc = 0.f;
  for (long long q = q0 + tid; q < q1; q += EG_THREADS) {
    const long long m = q / n, i = q - m * n;
    acc = acc + g[m * gs + (long long)c * n + i];
  }
  red[tid] = acc;
  __syncthreads();
  for (int k = EG_THREADS / 2; k >= 1; k >>= 1) {
    if (tid < k) red[tid] = red[tid] + red[tid + k];
    __syncthreads();
  }
  if (tid == 0) ws[(long long)blockIdx.x * C + c] = red[0];
}

extern "C" int64_t scf_channel_sum_workspace(int M, int C, int64_t n) {
  if (M <= 0 || C <= 0 || n <= 0) return -1;
  const long long Q = (long long)M * n;
  return scf_cdiv(Q, eg_cs_per(Q, C)) * C;
}

extern "C" int scf_channel_sum(const float* g, int64_t g_stride, float* out, int accumulate, float* workspace,
                               int64_t workspace_floats, int M, int C, int64_t n, scf_stream_t stream) {
  if (!g || !out || !workspace || M <= 0 || C <= 0 || n <= 0 || g_stride < C * n) return SCF_EINVAL;
  const long long Q = (long long)M * n, per = eg_cs_per(Q, C), splits = scf_cdiv(Q, per);
  if (workspace_floats < splits * C) return SCF_EINVAL;
  if (splits > 0x7fffffffll || C > 65535) return SCF_EUNSUPPORTED;
  scf_launch(eg_channel_sum_kernel, dim3((unsigned)splits, (unsigned)C), dim3(EG_THREADS), 0, scf_stream(stream), g,
             (long long)g_stride, workspace, (long long)n, Q, per, C);
  const int rc = scf_launch_status();
  if (rc != SCF_OK) return rc;
  return eg_combine(workspace, workspace, nullptr, out, splits, 0, C, accumulate, stream);
}

// ================================================================================================== fold and unfold
__global__ __launch_bounds__(EG_THREADS) void eg_bn_fold_kernel(const float* W, const float* b, const float* gamma,
                                                                const float* beta, const float* mean, const float* var,
                                                                float eps, float* Wf, float* bf, long long K,
                                                                long long total) {
  const long long e = (long long)blockIdx.x * EG_THREADS + threadIdx.x;
  if (e >= total) return;
  const long long c = e / K;
  const float s = gamma[c] / sqrtf(var[c] + eps);
  Wf[e] = s * W[e];
  if (e == c * K) bf[c] = __fmaf_rn(s, b[c] - mean[c], beta[c]);
}

extern "C" int scf_bn_fold(const float* W, const float* b, const float* gamma, const float* beta, const float* mean,
                           const float* var, float eps, float* Wf, float* bf, int Cout, int64_t K, scf_stream_t stream) {
  if (!W || !b || !gamma || !beta || !mean || !var || !Wf || !bf || Cout <= 0 || K <= 0 || !(eps >= 0.f)) return SCF_EINVAL;
  const long long total = (long long)Cout * K, blocks = scf_cdiv(total, EG_THREADS);
  if (blocks > 0x7fffffffll) return SCF_EUNSUPPORTED;
  scf_launch(eg_bn_fold_kernel, dim3((unsigned)blocks), dim3(EG_THREADS), 0, scf_stream(stream), W, b, gamma, beta, mean,
             var, eps, Wf, bf, (long long)K, total);
  return scf_launch_status();
}

__global__ __launch_bounds__(64) void eg_bn_unfold_kernel(const float* W, const float* b, const float* gamma,
                                                          const float* mean, const float* var, float eps, const float* dWf,
                                                          const float* dbf, float* dW, float* db, float* dgamma,
                                                          float* dbeta, int accumulate, long long K) {
  __shared__ float red[64];
  const int lane = threadIdx.x;
  const long long c = blockIdx.x;
  const float sd = sqrtf(var[c] + eps), s = gamma[c] / sd;
  const float* w = W + c * K;
  const float* dwf = dWf + c * K;
  float* dw = dW + c * K;
  float dot = 0.f;
  for (long long k = lane; k < K; k += 64) {
    const float d = dwf[k];
    dot = __fmaf_rn(w[k], d, dot);
    const float v = s * d;
    dw[k] = accumulate ? v + dw[k] : v;
  }
  red[lane] = dot;
  __syncthreads();
  for (int j = 32; j >= 1; j >>= 1) {
    if (lane < j) red[lane] = red[lane] + red[lane + j];
    __syncthreads();
  }
  if (lane == 0) {
    const float d = dbf[c];
    const float vb = s * d, vg = __fmaf_rn(b[c] - mean[c], d, red[0]) / sd;
    db[c] = accumulate ? vb + db[c] : vb;
    dbeta[c] = accumulate ? d + dbeta[c] : d;
    dgamma[c] = accumulate ? vg + dgamma[c] : vg;
  }
}

extern "C" int scf_bn_unfold(const float* W, const float* b, const float* gamma, const float* mean, const float* var,
                             float eps, const float* dWf, const float* dbf, float* dW, float* db, float* dgamma,
                             float* dbeta, int accumulate, int Cout, int64_t K, scf_stream_t stream) {
  if (!W || !b || !gamma || !mean || !var || !dWf || !dbf || !dW || !db || !dgamma || !dbeta || Cout <= 0 || K <= 0 ||
      !(eps >= 0.f))
    return SCF_EINVAL;
  scf_launch(eg_bn_unfold_kernel, dim3((unsigned)Cout), dim3(64), 0, scf_stream(stream), W, b, gamma, mean, var, eps, dWf,
             dbf, dW, db, dgamma, dbeta, accumulate, (long long)K);
  return scf_launch_status();
}
