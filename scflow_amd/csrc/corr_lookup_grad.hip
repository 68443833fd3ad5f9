// Adjoint of the multi-scale correlation lookup (corr_lookup.hip; corr_lookup.py:102-136) with respect to the pyramid,
// carried back to level 0 through the 2x2 / stride-2 average pools (raft_decoder.py:35-58), for gfx950, fp32.
//
//   g_corr (T, N, L (2r+1)^2, h, w)   cotangents of the lookup outputs of T iterations, the forward's channel order:
//                                     channel (2r+1)^2 l + (2r+1) a + b = the tap at x-offset a - r, y-offset b - r
//   flow   (T, N, 2, h, w)            the flow each lookup was taken at
//   mask   NULL | (T, N, 1, h, w)     a per-query factor on g_corr:  G = mask * g_corr, one rounding
//   g_vol  (N h w, h, w)              d loss / d level 0 of the pyramid, summed over T; every element is written
//
// The forward's tap (a, b) of one (query, level) blends the four map cells (y0 + b [+ 1], x0 + a [+ 1]) with the weights
// nw, ne, sw, se of lk_centre (lk_centre.h), which all taps of that (query, level) share.  So a level-l cell (jy, jx) of
// the query's own map receives, per iteration, with i = jx - x0, k = jy - y0 and G[a, b] = 0 outside [0, 2r]^2,
//     S_l[jy, jx] += nw G[i, k] + ne G[i - 1, k] + sw G[i, k - 1] + se G[i - 1, k - 1]
// a GATHER of at most four cotangents: no cell is written by two threads, nothing is atomic.  Along a size-1 axis the
// forward puts every tap on index 0 (both the "near" and the "far" cell), so cell 0 takes all 2r + 1 offsets of that
// axis, near and far entries being the same G.  A query whose flow is NaN / inf at iteration t ("bad": lk_centre gives
// NaN weights on an all-padding window) contributes ZERO at t: the volume never influenced that output.  A centre
// clamped to +-30000 contributes zero by itself (no cell of the map is inside its window).
//
// ONE summation order, the same in both kernels below:
//   S_l[cell]  from +0; iterations t ascending; inside an iteration the offsets of a size-1 x axis ascending, inside
//              them those of a size-1 y axis ascending (one pass each otherwise); inside a pass ONE fma chain
//              S = fma(nw, G[i, k], S); S = fma(ne, G[i - 1, k], S); S = fma(sw, G[i, k - 1], S); S = fma(se, G[i - 1, k - 1], S)
//              (an entry outside [0, 2r]^2 enters as +0: the step then leaves S as it is);
//   g_vol[q, jy, jx] = S_0[jy, jx], then for l = 1 .. L - 1 ascending, where (jy >> l) < (h >> l) and (jx >> l) < (w >> l)
//              (the floor pooling drops the last row / column of an odd map):  v = fma(4^-l, S_l[jy >> l, jx >> l], v)
//              -- the factor is a power of two, so this is one rounding of v + 4^-l S_l;
//   accumulate != 0: the previous value of g_vol is added last.
// No atomics, no allocation, no synchronisation with the host; a query's row depends on that query alone, so the
// result of a sample does not depend on N, and two runs give the same bits.  The pyramid itself is never read.
//
// Fast route (r <= 4 and the accumulators of at least one query fit in 64 KB of LDS): a block owns QB <= 16 consecutive
// queries (consecutive in the (n, y, x) order = consecutive floats of every g_corr channel and one contiguous piece of
// g_vol).  Per iteration it stages the QB x L (2r+1)^2 cotangents channel-major through LDS (coalesced runs of QB
// floats; loaded into registers an iteration ahead), the centres of its QB x L (query, level) pairs, and then updates ONLY the (2r+2)^2 cells of each window --
// the other cells of S_l would add zeros.  S_l lives in LDS for all T iterations; the fold writes g_vol once, coalesced.
// Traffic: g_corr read once, g_vol written once (+ read once with accumulate).
// Plain route (any radius / map size): one thread per element of g_vol, the same arithmetic straight from global memory.
#include "lk_centre.h"

#define LG_THREADS 256
#define LG_MAXV 24                // cotangents of one iteration a thread holds in registers: L (2r+1)^2 QB / 256 at most
#define LG_LDS_BYTES (64 * 1024)

struct LgParams {
  const float* g;
  const float* flow;
  const float* mask;
  float* out;
  int accumulate, T, N, h, w, r, L;
  int qb_log2;                    // fast route: log2 of the queries per block
  int sstride;                    // fast route: floats per query accumulator (all levels; odd)
  int lh[SCF_MAX_LEVELS], lw[SCF_MAX_LEVELS];
  int soff[SCF_MAX_LEVELS];       // offset (floats) of S_l inside a query's accumulator
  long long total_q;              // N h w
};

struct LgCentre {                 // what the window pass needs of LkCentre; bad: the query contributes nothing
  int x0, y0;
  float nw, ne, sw, se;
  int bad, pad_;
};

// one iteration's contribution to one cell, in the stated order.  G(a, b): the (masked) cotangent of tap (a, b), +0
// outside [0, 2r]^2.
template <class GF>
__device__ __forceinline__ float lg_cell(float acc, const LgCentre& c, int jx, int jy, bool flat_x, bool flat_y, int D, GF G) {
  const int i = jx - c.x0, k = jy - c.y0;
  const int na = flat_x ? D : 1, nb = flat_y ? D : 1;
  for (int a_ = 0; a_ < na; ++a_) {
    const int ia = flat_x ? a_ : i, ia1 = flat_x ? a_ : i - 1;
    for (int b_ = 0; b_ < nb; ++b_) {
      const int kb = flat_y ? b_ : k, kb1 = flat_y ? b_ : k - 1;
      acc = __builtin_fmaf(c.nw, G(ia, kb), acc);
      acc = __builtin_fmaf(c.ne, G(ia1, kb), acc);
      acc = __builtin_fmaf(c.sw, G(ia, kb1), acc);
      acc = __builtin_fmaf(c.se, G(ia1, kb1), acc);
    }
  }
  return acc;
}

__device__ __forceinline__ LgCentre lg_centre_at(const LgParams& p, int pix, float fx, float fy, int lvl) {
  const int y = pix / p.w, x = pix - y * p.w;
  const LkCentre c = lk_centre<0>((float)x + fx, (float)y + fy, 1.0f / (float)(1 << lvl), p.lw[lvl] == 1, p.lh[lvl] == 1, p.r);
  LgCentre o;
  o.x0 = c.x0; o.y0 = c.y0;
  o.bad = c.nw != c.nw;           // NaN weights <=> lk_centre's bad case
  o.nw = o.bad ? 0.f : c.nw; o.ne = o.bad ? 0.f : c.ne; o.sw = o.bad ? 0.f : c.sw; o.se = o.bad ? 0.f : c.se;
  o.pad_ = 0;
  return o;
}

__device__ __forceinline__ LgCentre lg_centre(const LgParams& p, int t, long long n, int pix, int lvl) {
  const int hw = p.h * p.w;
  const float* f = p.flow + (((long long)t * p.N + n) * 2) * hw + pix;
  return lg_centre_at(p, pix, f[0], f[hw], lvl);
}

template <int R>
__global__ __launch_bounds__(LG_THREADS) void corr_lookup_grad_kernel(LgParams p) {
  extern __shared__ float lg_lds[];
  constexpr int D = 2 * R + 1, DD = D * D, W1 = D + 1, WC = W1 * W1;
  const int L = p.L, K = L * DD, hw = p.h * p.w;
  const int QB = 1 << p.qb_log2, tid = threadIdx.x;
  float* Gs = lg_lds;                                           // [K][QB]
  LgCentre* Cs = reinterpret_cast<LgCentre*>(Gs + K * QB);      // [L][QB]
  float* S = reinterpret_cast<float*>(Cs + L * QB);             // [QB][sstride]
  // Blocks are dealt to the 8 XCDs round-robin; the blocks that share the 128-byte lines of g_corr (a line holds 32
  // queries of one channel, a block reads QB of them) are given to ONE XCD, next to each other in its dispatch order,
  // so that the line comes from HBM once and from that XCD's L2 afterwards.  Speed only: any placement is correct.
  const unsigned nblk = gridDim.x, xcd = blockIdx.x & 7u, per = nblk >> 3, rem = nblk & 7u;
  const unsigned group = (xcd < rem ? xcd * (per + 1) : rem * (per + 1) + (xcd - rem) * per) + (blockIdx.x >> 3);
  const long long q0 = (long long)group * QB;
  // QB divides the block size: a thread serves ONE query in the staging and in the window pass
  const int qi = tid & (QB - 1), k0 = tid >> p.qb_log2, kstep = LG_THREADS >> p.qb_log2;
  const long long q = q0 + qi;
  const bool qok = q < p.total_q;
  const long long n = qok ? q / hw : 0;
  const int pix = qok ? (int)(q - n * hw) : 0;
  const bool centre_thread = tid < L * QB;
  // a thread's share of one iteration's cotangents (at most LG_MAXV: the dispatch sees to it), its mask factor and, for
  // the centre threads, its flow: loaded an iteration ahead, so that the loads are in flight during the window pass
  float v[LG_MAXV], m = 1.f, fx = 0.f, fy = 0.f;
  auto prefetch = [&](int t) {
    const long long tn = (long long)t * p.N + n;
    const float* g = p.g + tn * K * hw + pix;
#pragma unroll
    for (int u = 0; u < LG_MAXV; ++u) {
      // unconditional loads from clamped, always valid addresses (a query past the end reads query 0 of sample 0): a
      // load under a per-element condition would be branched around and waited for one by one
      const int k = k0 + u * kstep;
      v[u] = g[(long long)(k < K ? k : K - 1) * hw];
    }
    if (p.mask) m = p.mask[tn * hw + pix];
    const float* f = p.flow + (tn * 2) * hw + pix;
    fx = f[0]; fy = f[hw];
  };
  prefetch(0);
  for (int i = tid; i < QB * p.sstride; i += LG_THREADS) S[i] = 0.f;
  for (int t = 0; t < p.T; ++t) {
    __syncthreads();                                            // the previous window pass has read Gs / Cs
#pragma unroll
    for (int u = 0; u < LG_MAXV; ++u) {
      const int k = k0 + u * kstep;
      if (k < K) Gs[k * QB + qi] = !qok ? 0.f : p.mask ? m * v[u] : v[u];
    }
    if (centre_thread) {
      // the level is kept wave-uniform (a loop with one live pass per thread): a per-lane index into the kernel
      // arguments would be a vector load from memory
      for (int lvl = 0; lvl < L; ++lvl) {
        if ((tid >> p.qb_log2) != lvl) continue;
        LgCentre c;
        if (qok) c = lg_centre_at(p, pix, fx, fy, lvl);
        else { c.x0 = c.y0 = 0; c.nw = c.ne = c.sw = c.se = 0.f; c.bad = 1; c.pad_ = 0; }
        Cs[lvl * QB + qi] = c;
      }
    }
    __syncthreads();
    if (t + 1 < p.T) prefetch(t + 1);
    // window pass: item = (level, window cell, query); a cell of S_l belongs to one item of this pass.  The level loop
    // is outside, so that everything that depends on the level alone is scalar.
    for (int lvl = 0; lvl < L; ++lvl) {
      const LgCentre c = Cs[lvl * QB + qi];
      if (c.bad) continue;
      const int lw = p.lw[lvl], lh = p.lh[lvl];
      const bool flat_x = lw == 1, flat_y = lh == 1;
      const float* gl = Gs + (lvl * DD) * QB + qi;
      float* sl = S + qi * p.sstride + p.soff[lvl];
      for (int wc = k0; wc < WC; wc += kstep) {
        const int wk = wc / W1, wi = wc - wk * W1;               // neighbouring lanes: neighbouring cells of a map row
        if ((flat_x && wi > 0) || (flat_y && wk > 0)) continue;  // a size-1 axis: the one cell takes every offset
        const int jx = flat_x ? 0 : c.x0 + wi, jy = flat_y ? 0 : c.y0 + wk;
        if ((unsigned)jx >= (unsigned)lw || (unsigned)jy >= (unsigned)lh) continue;
        float* s = sl + jy * lw + jx;
        *s = lg_cell(*s, c, jx, jy, flat_x, flat_y, D, [&](int a, int b) -> float {
          return ((unsigned)a < (unsigned)D && (unsigned)b < (unsigned)D) ? gl[(a * D + b) * QB] : 0.f;
        });
      }
    }
  }
  __syncthreads();
  // fold to level 0 and write this block's contiguous piece of g_vol
  long long left = p.total_q - q0;
  const int nq = left < QB ? (int)left : QB;
  for (int i = tid; i < nq * hw; i += LG_THREADS) {
    const int qq = i / hw, cell = i - qq * hw;
    const int jy = cell / p.w, jx = cell - jy * p.w;
    const float* s = S + qq * p.sstride;
    float v = s[cell];
    float scale = 0.25f;
    for (int l = 1; l < L; ++l) {
      const int yy = jy >> l, xx = jx >> l;
      if (yy < p.lh[l] && xx < p.lw[l]) v = __builtin_fmaf(scale, s[p.soff[l] + yy * p.lw[l] + xx], v);
      scale *= 0.25f;
    }
    float* o = p.out + q0 * hw + i;
    if (p.accumulate) v = v + *o;
    *o = v;
  }
}

__global__ __launch_bounds__(LG_THREADS) void corr_lookup_grad_plain_kernel(LgParams p) {
  const int D = 2 * p.r + 1, L = p.L, hw = p.h * p.w;
  const long long DD = (long long)D * D, K = L * DD;
  const long long total = p.total_q * hw;
  for (long long idx = (long long)blockIdx.x * LG_THREADS + threadIdx.x; idx < total; idx += (long long)gridDim.x * LG_THREADS) {
    const long long q = idx / hw;
    const int cell = (int)(idx - q * hw);
    const long long n = q / hw;
    const int pix = (int)(q - n * hw);
    const int jy0 = cell / p.w, jx0 = cell - jy0 * p.w;
    float v = 0.f, scale = 1.f;
    for (int l = 0; l < L; ++l, scale *= 0.25f) {
      const int jy = jy0 >> l, jx = jx0 >> l;
      const int lw = p.lw[l], lh = p.lh[l];
      if (jy >= lh || jx >= lw) continue;
      const bool flat_x = lw == 1, flat_y = lh == 1;
      float s = 0.f;
      for (int t = 0; t < p.T; ++t) {
        const LgCentre c = lg_centre(p, t, n, pix, l);
        if (c.bad) continue;
        const long long tn = (long long)t * p.N + n;
        const float* g = p.g + (tn * K + l * DD) * hw + pix;
        const bool masked = p.mask != nullptr;
        const float m = masked ? p.mask[tn * hw + pix] : 1.f;
        s = lg_cell(s, c, jx, jy, flat_x, flat_y, D, [&](int a, int b) -> float {
          if ((unsigned)a >= (unsigned)D || (unsigned)b >= (unsigned)D) return 0.f;
          const float gv = g[(long long)(a * D + b) * hw];
          return masked ? m * gv : gv;
        });
      }
      v = l == 0 ? s : __builtin_fmaf(scale, s, v);
    }
    if (p.accumulate) v = v + p.out[idx];
    p.out[idx] = v;
  }
}

// The launch plan, a function of the sizes alone: the size checks, the level geometry and the route.  scf_corr_lookup_grad
// launches what it says and scf_corr_lookup_grad_route reports it.  -> 1: the fast route (p.qb_log2, p.sstride set), 0: the
// plain route, < 0: the error code of sizes the kernels do not take.  Fills N, h, w, r, L, total_q, lh, lw, soff of p.
static int lg_plan(int T, int N, int h, int w, int r, int L, LgParams& p) {
  if (T <= 0 || N <= 0 || h <= 0 || w <= 0 || L <= 0 || r < 1) return SCF_EINVAL;
  if (L > SCF_MAX_LEVELS || T > SCF_TAIL_MAX_T) return SCF_EUNSUPPORTED;
  if ((long long)h * w > 0x7fffffffLL || r > 16383) return SCF_EUNSUPPORTED;
  p.T = T; p.N = N; p.h = h; p.w = w; p.r = r; p.L = L;
  p.total_q = (long long)N * h * w;
  if ((long long)h * w > 0x7fffffffffffLL / p.total_q) return SCF_EUNSUPPORTED;         // 64-bit element offsets of g_vol
  long long cells = 0;
  for (int l = 0; l < SCF_MAX_LEVELS; ++l) {
    p.lh[l] = p.lw[l] = p.soff[l] = 0;
    if (l >= L) continue;
    const int lh = h >> l, lw = w >> l;
    if (lh <= 0 || lw <= 0) return SCF_EINVAL;
    p.lh[l] = lh; p.lw[l] = lw;
    p.soff[l] = (int)(cells > 0x7fffffffLL ? 0 : cells);
    cells += (long long)lh * lw;
  }
  const long long D = 2LL * r + 1, K = L * D * D;
  if (K * h * w > 0x7fffffffffffLL / ((long long)T * N)) return SCF_EUNSUPPORTED;      // 64-bit element offsets
  // fast route: the largest QB <= 16 whose staging + centres + accumulators fit
  int qb_log2 = -1;
  const long long sstride = cells | 1;
  if (r <= 4)
    for (int e = 4; e >= 0; --e) {
      const long long qb = 1LL << e;
      const long long bytes = (K * qb + sstride * qb) * (long long)sizeof(float) + (long long)L * qb * (long long)sizeof(LgCentre);
      if (bytes <= LG_LDS_BYTES && scf_cdiv(K * qb, LG_THREADS) <= LG_MAXV) { qb_log2 = e; break; }
    }
  if (qb_log2 >= 0 && scf_cdiv(p.total_q, 1LL << qb_log2) <= 0x7fffffffLL) {
    p.qb_log2 = qb_log2;
    p.sstride = (int)sstride;
    return 1;
  }
  p.qb_log2 = 0; p.sstride = 0;
  return 0;
}

extern "C" int scf_corr_lookup_grad_route(int N, int h, int w, int r, int L, int* route) {
  if (!route) return SCF_EINVAL;
  LgParams p;
  const int fast = lg_plan(1, N, h, w, r, L, p);
  if (fast < 0) return fast;
  route[0] = fast ? 0 : 1;
  route[1] = fast ? (r < 4 ? r : 4) : 0;
  route[2] = fast ? p.qb_log2 : -1;
  route[3] = fast && (p.total_q & ((1LL << p.qb_log2) - 1)) != 0;
  return SCF_OK;
}

extern "C" int scf_corr_lookup_grad(const float* g_corr, const float* flow, const float* mask, float* g_vol,
                                    int accumulate, int T, int N, int h, int w, int r, int L, scf_stream_t stream) {
  if (!g_corr || !flow || !g_vol) return SCF_EINVAL;
  LgParams p;
  const int fast = lg_plan(T, N, h, w, r, L, p);
  if (fast < 0) return fast;
  p.g = g_corr; p.flow = flow; p.mask = mask; p.out = g_vol;
  p.accumulate = accumulate != 0;
  if (fast) {
    const long long D = 2LL * r + 1, K = L * D * D;
    const int qb = 1 << p.qb_log2;
    const size_t lds = ((size_t)K * qb + (size_t)p.sstride * qb) * sizeof(float) + (size_t)L * qb * sizeof(LgCentre);
    const dim3 grid((unsigned)scf_cdiv(p.total_q, qb));
    switch (r) {
      case 1: scf_launch(corr_lookup_grad_kernel<1>, grid, dim3(LG_THREADS), lds, scf_stream(stream), p); break;
      case 2: scf_launch(corr_lookup_grad_kernel<2>, grid, dim3(LG_THREADS), lds, scf_stream(stream), p); break;
      case 3: scf_launch(corr_lookup_grad_kernel<3>, grid, dim3(LG_THREADS), lds, scf_stream(stream), p); break;
      default: scf_launch(corr_lookup_grad_kernel<4>, grid, dim3(LG_THREADS), lds, scf_stream(stream), p); break;
    }
    return scf_launch_status();
  }
  long long nb = scf_cdiv(p.total_q * h * w, LG_THREADS);
  if (nb > 262144) nb = 262144;
  scf_launch(corr_lookup_grad_plain_kernel, dim3((unsigned)nb), dim3(LG_THREADS), 0, scf_stream(stream), p);
  return scf_launch_status();
}
