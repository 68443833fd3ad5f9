// BatchNorm2d(eps, momentum, affine) on the statistics of the batch, forward and backward, as the context encoder applies
// it while it trains (norm_cfg BN, freeze_bn=False), for gfx950.  Memory-bound: vector ALU and vector stores only.
//
// u is the raw convolution output (N, C, HW); per channel M = N HW values.  Three forms, the ones instance_norm_grad.hip has:
//   mid       relu(BN(u))                                                                   backward -> du
//   tail      y = relu(BN(u) + res)              g' = g [y > 0], also the cotangent of res  backward -> g', du
//   tail + ds y = relu(BN_a(u) + BN_b(r))        two parameter sets, two statistics         backward -> du, dr
// and (dgamma, dbeta) = (S2, S1) per normalised operand, with
//   xhat = (u - mean) rstd,   S1 = sum g',   S2 = sum g' xhat,   du = ((g' - S1 / M) - xhat S2 / M) (gamma rstd).
//
// Forward, two launches.  Statistics: one workgroup per (n, c) plane, or per chunk of BNT_CHUNK elements of a larger plane,
// writes (count, mean, centred sum of squares) of its elements to the workspace -- the mean first, then the squares of the
// differences from it, so an input with a large offset loses nothing (a raw sum of x^2 would cancel in E[x^2] - mean^2).
// Apply: every wave combines its channel's N K triples with Chan's formula in one fixed tree (bnt_channel_moments), then
// the elementwise part; the first block of a channel also writes (mean, rstd) to `saved` and moves the running statistics.
// Backward, two launches.  Reduce: per plane or chunk (S1, S2[, S2r]) to the workspace, mean / rstd from `saved`, the mask
// from the kept y; the tail form writes g'.  Apply: the partials summed across N in one fixed order, du (dr), and from the
// first block of a channel dgamma / dbeta.
// No atomics, allocation or synchronisation; the order of every sum is fixed by (N, HW) and the alignment class alone.
//
// Contraction is off in this file so that the float64 restatement's error model (tests/test_bn_train_host.py) counts the
// operations that are written here, one rounding each.
#include "scf_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int BNT_NT = 256;
constexpr int BNT_CHUNK = 16384;  // elements one workgroup of a statistics / reduce pass takes: 16 float4 per thread
constexpr int BNT_BLOCK = 4096;   // elements one workgroup of an apply pass takes: 4 float4 per thread

__device__ __forceinline__ float bnt_wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// K sums over the 256-thread workgroup at once (norm.hip's block_sum order), results broadcast to every thread
template <int K>
__device__ __forceinline__ void bnt_block_sum(float (&v)[K], float* red) {
  constexpr int NW = BNT_NT / 64;
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = bnt_wave_sum(v[k]);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) red[k * NW + wave] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = (red[k * NW] + red[k * NW + 1]) + (red[k * NW + 2] + red[k * NW + 3]);
}

__device__ __forceinline__ float4 bnt_zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

__device__ __forceinline__ float bnt_mask(float g, float y) { return y > 0.f ? g : 0.f; }

struct BntMoments {
  float n, mean, m2;  // count, mean, sum of squared differences from the mean
};

// Chan's combination of two sets; a is the set with the lower partial indices.  An empty set is the identity.
__device__ __forceinline__ BntMoments bnt_chan(const BntMoments a, const BntMoments b) {
  if (b.n == 0.f) return a;
  if (a.n == 0.f) return b;
  const float n = a.n + b.n, d = b.mean - a.mean, f = b.n / n;
  BntMoments r;
  r.n = n;
  r.mean = a.mean + d * f;
  r.m2 = (a.m2 + b.m2) + (d * d) * (a.n * f);
  return r;
}

// The moments of channel c over its P = N K partials (index p = n K + k, ws entry ((n C + c) K + k)), the same bits in
// every lane of every wave: groups of 64 partials in a butterfly whose lower lane is the left operand at every level, the
// groups folded in ascending order.
__device__ __forceinline__ BntMoments bnt_channel_moments(const float* ws, int c, int C, int N, int K) {
  const int lane = threadIdx.x & 63, P = N * K;
  BntMoments acc = {0.f, 0.f, 0.f};
  for (int p0 = 0; p0 < P; p0 += 64) {
    const int p = p0 + lane;
    BntMoments m = {0.f, 0.f, 0.f};
    if (p < P) {
      const int n = p / K, k = p - n * K;
      const float* t = ws + 3 * (((long long)n * C + c) * K + k);
      m.n = t[0]; m.mean = t[1]; m.m2 = t[2];
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      BntMoments o;
      o.n = __shfl_xor(m.n, off); o.mean = __shfl_xor(m.mean, off); o.m2 = __shfl_xor(m.m2, off);
      m = (lane & off) ? bnt_chan(o, m) : bnt_chan(m, o);
    }
    acc = bnt_chan(acc, m);
  }
  return acc;
}

// ---------------------------------------------------------------------------------
// Forward, statistics.  Block pc = plane K + chunk.  Register form: the chunk stays in VEC4 float4 per thread between the
// two sums, one read.  Looped form (any HW, any alignment): two sweeps, the second out of L2.
// ---------------------------------------------------------------------------------
template <int VEC4>
__global__ __launch_bounds__(BNT_NT) void bnt_stats_kernel(const float* u, float* ws, int HW, int K) {
  __shared__ float red[BNT_NT / 64];
  const long long pc = blockIdx.x, pl = pc / K;
  const int e0 = (int)(pc - pl * K) * BNT_CHUNK;
  const int cnt = min(HW - e0, BNT_CHUNK), n4 = cnt >> 2;
  const float4* up = reinterpret_cast<const float4*>(u + pl * HW + e0);
  float4 v[VEC4];
  float s[1] = {0.f};
#pragma unroll
  for (int i = 0; i < VEC4; ++i) {
    const int idx = i * BNT_NT + threadIdx.x;
    v[i] = idx < n4 ? up[idx] : bnt_zero4();
    s[0] += (v[i].x + v[i].y) + (v[i].z + v[i].w);
  }
  bnt_block_sum<1>(s, red);
  const float mean = s[0] / (float)cnt;
  float q[1] = {0.f};
#pragma unroll
  for (int i = 0; i < VEC4; ++i) {
    const int idx = i * BNT_NT + threadIdx.x;
    if (idx < n4) {
      const float a = v[i].x - mean, b = v[i].y - mean, c = v[i].z - mean, d = v[i].w - mean;
      q[0] += (a * a + b * b) + (c * c + d * d);
    }
  }
  bnt_block_sum<1>(q, red);
  if (threadIdx.x == 0) {
    float* t = ws + 3 * pc;
    t[0] = (float)cnt; t[1] = mean; t[2] = q[0];
  }
}

__global__ __launch_bounds__(BNT_NT) void bnt_stats_loop_kernel(const float* u, float* ws, int HW, int K) {
  __shared__ float red[BNT_NT / 64];
  const long long pc = blockIdx.x, pl = pc / K;
  const int e0 = (int)(pc - pl * K) * BNT_CHUNK;
  const int cnt = min(HW - e0, BNT_CHUNK);
  const float* up = u + pl * HW + e0;
  float s[1] = {0.f};
  for (int i = threadIdx.x; i < cnt; i += BNT_NT) s[0] += up[i];
  bnt_block_sum<1>(s, red);
  const float mean = s[0] / (float)cnt;
  float q[1] = {0.f};
  for (int i = threadIdx.x; i < cnt; i += BNT_NT) {
    const float a = up[i] - mean;
    q[0] += a * a;
  }
  bnt_block_sum<1>(q, red);
  if (threadIdx.x == 0) {
    float* t = ws + 3 * pc;
    t[0] = (float)cnt; t[1] = mean; t[2] = q[0];
  }
}

// ---------------------------------------------------------------------------------
// Forward, apply.  Block b = plane bpp + j takes elements [j BNT_BLOCK, (j + 1) BNT_BLOCK) of its plane.
// FORM 0: BN(u); 1: BN(u) + res; 2: BN_a(u) + BN_b(res), the second operand's partials behind the first's.
// ---------------------------------------------------------------------------------
struct BntSet {          // one normalised operand's parameters
  const float* gamma;
  const float* beta;
  float* run_mean;       // NULL: no running statistics are kept
  float* run_var;
  float* saved;          // (2, C): mean, rstd
};

__device__ __forceinline__ void bnt_finalise(const BntMoments m, const BntSet p, int c, int C, float momentum, float eps,
                                             bool first, float& mean, float& rstd) {
  mean = m.mean;
  rstd = 1.0f / sqrtf(m.m2 / m.n + eps);
  if (first) {
    p.saved[c] = mean;
    p.saved[C + c] = rstd;
    if (p.run_mean) {
      const float keep = 1.0f - momentum, unbiased = m.m2 / (m.n - 1.0f);
      p.run_mean[c] = keep * p.run_mean[c] + momentum * mean;
      p.run_var[c] = keep * p.run_var[c] + momentum * unbiased;
    }
  }
}

template <bool VEC, int FORM>
__global__ __launch_bounds__(BNT_NT) void bnt_apply_kernel(const float* u, const float* res, BntSet pa, BntSet pb,
                                                           const float* ws, float* y, int N, int C, int HW, int K, int bpp,
                                                           int relu, float momentum, float eps) {
  const long long b = blockIdx.x, pl = b / bpp;
  const int j = (int)(b - pl * bpp), c = (int)(pl % C);
  const bool first = pl < C && j == 0 && threadIdx.x == 0;       // sample 0, block 0 of the channel
  float mean, rstd, mean_r = 0.f, rstd_r = 0.f, ga_r = 0.f, be_r = 0.f;
  bnt_finalise(bnt_channel_moments(ws, c, C, N, K), pa, c, C, momentum, eps, first, mean, rstd);
  const float ga = pa.gamma[c], be = pa.beta[c];
  if constexpr (FORM == 2) {
    bnt_finalise(bnt_channel_moments(ws + 3ll * N * C * K, c, C, N, K), pb, c, C, momentum, eps, first, mean_r, rstd_r);
    ga_r = pb.gamma[c];
    be_r = pb.beta[c];
  }
  auto one = [&](float x, float r) {
    float v = ((x - mean) * rstd) * ga + be;
    if constexpr (FORM == 1) v = v + r;
    if constexpr (FORM == 2) v = v + (((r - mean_r) * rstd_r) * ga_r + be_r);
    return relu ? (v > 0.f ? v : 0.f) : v;
  };
  const long long base = pl * HW;
  const int e0 = j * BNT_BLOCK;
  if constexpr (VEC) {
#pragma unroll
    for (int i = 0; i < BNT_BLOCK / (4 * BNT_NT); ++i) {
      const int e = e0 + 4 * (i * BNT_NT + threadIdx.x);
      if (e < HW) {
        const float4 x = *reinterpret_cast<const float4*>(u + base + e);
        const float4 r = FORM ? *reinterpret_cast<const float4*>(res + base + e) : bnt_zero4();
        scf_store4<false>(y + base + e, one(x.x, r.x), one(x.y, r.y), one(x.z, r.z), one(x.w, r.w));
      }
    }
  } else {
    const int e1 = min(HW, e0 + BNT_BLOCK);
    for (int e = e0 + threadIdx.x; e < e1; e += BNT_NT) y[base + e] = one(u[base + e], FORM ? res[base + e] : 0.f);
  }
}

// ---------------------------------------------------------------------------------
// Backward, reduce.  Block pc = plane K + chunk -> ws[3 pc ..] = (S1, S2, S2r) of its elements: a thread adds its
// elements (float4: (a + b) + (c + d)) to one chain from +0, then the workgroup's tree.  TAIL: g is the cotangent at y
// and is masked here; the form without a normalised shortcut writes the masked g' to gp.
// ---------------------------------------------------------------------------------
template <bool VEC, bool TAIL, bool DS>
__global__ __launch_bounds__(BNT_NT) void bnt_grad_reduce_kernel(const float* g, const float* y, const float* u,
                                                                 const float* r, const float* saved, const float* saved_r,
                                                                 float* gp, float* ws, int C, int HW, int K) {
  __shared__ float red[3 * BNT_NT / 64];
  const long long pc = blockIdx.x, pl = pc / K;
  const int e0 = (int)(pc - pl * K) * BNT_CHUNK, c = (int)(pl % C);
  const int cnt = min(HW - e0, BNT_CHUNK);
  const long long base = pl * HW + e0;
  const float mean = saved[c], rstd = saved[C + c];
  const float mean_r = DS ? saved_r[c] : 0.f, rstd_r = DS ? saved_r[C + c] : 0.f;
  float t[3] = {0.f, 0.f, 0.f};
  if constexpr (VEC) {
    for (int idx = threadIdx.x; idx < (cnt >> 2); idx += BNT_NT) {
      const long long at = base + 4ll * idx;
      float4 gv = *reinterpret_cast<const float4*>(g + at);
      const float4 uv = *reinterpret_cast<const float4*>(u + at);
      if constexpr (TAIL) {
        const float4 yv = *reinterpret_cast<const float4*>(y + at);
        gv.x = bnt_mask(gv.x, yv.x); gv.y = bnt_mask(gv.y, yv.y); gv.z = bnt_mask(gv.z, yv.z); gv.w = bnt_mask(gv.w, yv.w);
        if constexpr (!DS) scf_store4<false>(gp + at, gv.x, gv.y, gv.z, gv.w);
      }
      t[0] += (gv.x + gv.y) + (gv.z + gv.w);
      t[1] += (gv.x * ((uv.x - mean) * rstd) + gv.y * ((uv.y - mean) * rstd)) +
              (gv.z * ((uv.z - mean) * rstd) + gv.w * ((uv.w - mean) * rstd));
      if constexpr (DS) {
        const float4 rv = *reinterpret_cast<const float4*>(r + at);
        t[2] += (gv.x * ((rv.x - mean_r) * rstd_r) + gv.y * ((rv.y - mean_r) * rstd_r)) +
                (gv.z * ((rv.z - mean_r) * rstd_r) + gv.w * ((rv.w - mean_r) * rstd_r));
      }
    }
  } else {
    for (int i = threadIdx.x; i < cnt; i += BNT_NT) {
      float gm = g[base + i];
      if constexpr (TAIL) {
        gm = bnt_mask(gm, y[base + i]);
        if constexpr (!DS) gp[base + i] = gm;
      }
      t[0] += gm;
      t[1] += gm * ((u[base + i] - mean) * rstd);
      if constexpr (DS) t[2] += gm * ((r[base + i] - mean_r) * rstd_r);
    }
  }
  bnt_block_sum<3>(t, red);
  if (threadIdx.x == 0) {
    float* w = ws + 3 * pc;
    w[0] = t[0]; w[1] = t[1]; w[2] = t[2];
  }
}

// ---------------------------------------------------------------------------------
// Backward, apply.  Every wave sums its channel's P = N K partial triples: lane l adds p = l, l + 64, ... to one chain
// from +0, then v[l] += v[l ^ off] for off = 32, ..., 1.  gq is the cotangent at BN(u): the mid form's g or the tail form's
// g' of the reduce pass; DS masks g with y again (that form keeps no g').
// ---------------------------------------------------------------------------------
template <bool VEC, bool DS>
__global__ __launch_bounds__(BNT_NT) void bnt_grad_apply_kernel(const float* gq, const float* y, const float* u, const float* r,
                                                                const float* saved, const float* saved_r, const float* gamma,
                                                                const float* gamma_r, const float* ws, float* du, float* dr,
                                                                float* dgamma, float* dbeta, float* dgamma_r, float* dbeta_r,
                                                                int accumulate, int N, int C, int HW, int K, int bpp) {
  const long long b = blockIdx.x, pl = b / bpp;
  const int j = (int)(b - pl * bpp), c = (int)(pl % C), lane = threadIdx.x & 63, P = N * K;
  float s[3] = {0.f, 0.f, 0.f};
  for (int p = lane; p < P; p += 64) {
    const int n = p / K, k = p - n * K;
    const float* t = ws + 3 * (((long long)n * C + c) * K + k);
    s[0] += t[0]; s[1] += t[1]; s[2] += t[2];
  }
#pragma unroll
  for (int q = 0; q < 3; ++q) s[q] = bnt_wave_sum(s[q]);
  const float M = (float)((long long)N * HW);
  const float mean = saved[c], rstd = saved[C + c], kf = gamma[c] * rstd;
  const float m1 = s[0] / M, m2 = s[1] / M;
  float mean_r = 0.f, rstd_r = 0.f, kf_r = 0.f, m3 = 0.f;
  if constexpr (DS) {
    mean_r = saved_r[c]; rstd_r = saved_r[C + c]; kf_r = gamma_r[c] * rstd_r; m3 = s[2] / M;
  }
  if (pl < C && j == 0 && threadIdx.x == 0) {
    dbeta[c] = accumulate ? s[0] + dbeta[c] : s[0];
    dgamma[c] = accumulate ? s[1] + dgamma[c] : s[1];
    if constexpr (DS) {
      dbeta_r[c] = accumulate ? s[0] + dbeta_r[c] : s[0];
      dgamma_r[c] = accumulate ? s[2] + dgamma_r[c] : s[2];
    }
  }
  auto grad = [](float gm, float x, float mu, float rs, float a1, float a2, float k) {
    return ((gm - a1) - ((x - mu) * rs) * a2) * k;
  };
  const long long base = pl * HW;
  const int e0 = j * BNT_BLOCK;
  if constexpr (VEC) {
#pragma unroll
    for (int i = 0; i < BNT_BLOCK / (4 * BNT_NT); ++i) {
      const int e = e0 + 4 * (i * BNT_NT + threadIdx.x);
      if (e < HW) {
        float4 gv = *reinterpret_cast<const float4*>(gq + base + e);
        const float4 uv = *reinterpret_cast<const float4*>(u + base + e);
        if constexpr (DS) {
          const float4 yv = *reinterpret_cast<const float4*>(y + base + e);
          const float4 rv = *reinterpret_cast<const float4*>(r + base + e);
          gv.x = bnt_mask(gv.x, yv.x); gv.y = bnt_mask(gv.y, yv.y); gv.z = bnt_mask(gv.z, yv.z); gv.w = bnt_mask(gv.w, yv.w);
          scf_store4<false>(dr + base + e, grad(gv.x, rv.x, mean_r, rstd_r, m1, m3, kf_r), grad(gv.y, rv.y, mean_r, rstd_r, m1, m3, kf_r),
                            grad(gv.z, rv.z, mean_r, rstd_r, m1, m3, kf_r), grad(gv.w, rv.w, mean_r, rstd_r, m1, m3, kf_r));
        }
        scf_store4<false>(du + base + e, grad(gv.x, uv.x, mean, rstd, m1, m2, kf), grad(gv.y, uv.y, mean, rstd, m1, m2, kf),
                          grad(gv.z, uv.z, mean, rstd, m1, m2, kf), grad(gv.w, uv.w, mean, rstd, m1, m2, kf));
      }
    }
  } else {
    const int e1 = min(HW, e0 + BNT_BLOCK);
    for (int e = e0 + threadIdx.x; e < e1; e += BNT_NT) {
      float gm = gq[base + e];
      if constexpr (DS) {
        gm = bnt_mask(gm, y[base + e]);
        dr[base + e] = grad(gm, r[base + e], mean_r, rstd_r, m1, m3, kf_r);
      }
      du[base + e] = grad(gm, u[base + e], mean, rstd, m1, m2, kf);
    }
  }
}

// ---------------------------------------------------------------------------------
// Host side.
// ---------------------------------------------------------------------------------
struct BntGeom {
  int64_t planes, chunks, blocks;  // N C; planes K; planes bpp
  int K, bpp;
};

// SCF_OK and the launch geometry, or the error code of a size the kernels do not take
int bnt_geometry(int N, int C, int HW, BntGeom& geo) {
  if (N <= 0 || C <= 0 || HW <= 0) return SCF_EINVAL;
  const int64_t M = (int64_t)N * HW;
  if (M == 1) return SCF_EINVAL;                  // the unbiased variance divides by M - 1
  if (M > (1ll << 24)) return SCF_EUNSUPPORTED;   // the counts travel as floats
  geo.K = (int)scf_cdiv(HW, BNT_CHUNK);
  geo.bpp = (int)scf_cdiv(HW, BNT_BLOCK);
  geo.planes = (int64_t)N * C;
  geo.chunks = geo.planes * geo.K;
  geo.blocks = geo.planes * geo.bpp;
  if (geo.blocks > 0x7fffffffLL || (int64_t)N * geo.K > 0x7fffffffLL) return SCF_EUNSUPPORTED;
  return SCF_OK;
}

inline uintptr_t bnt_bits(const void* p) { return (uintptr_t)p; }

// What the two entries launch, a function of (N, C, HW) and of the alignment class of the maps alone (aligned: every
// (N, C, HW) operand on a 16-byte boundary).  The entries launch what it says and scf_batch_norm_train_route reports it.
struct BntRoute {
  BntGeom geo;
  bool vec;    // the float4 sweeps of every pass
  int stats;   // VEC4 of bnt_stats_kernel: 1, 4 or 16; 0: bnt_stats_loop_kernel
};

int bnt_route(int N, int C, int HW, bool aligned, BntRoute& rt) {
  const int rc = bnt_geometry(N, C, HW, rt.geo);
  if (rc != SCF_OK) return rc;
  rt.vec = (HW % 4 == 0) && aligned;
  const int n4 = (HW < BNT_CHUNK ? HW : BNT_CHUNK) / 4;
  rt.stats = !rt.vec ? 0 : n4 <= 256 ? 1 : n4 <= 1024 ? 4 : 16;
  return SCF_OK;
}

}  // namespace

extern "C" int64_t scf_batch_norm_train_workspace(int N, int C, int HW) {
  BntGeom geo;
  const int rc = bnt_geometry(N, C, HW, geo);
  return rc != SCF_OK ? rc : 6 * geo.chunks;
}

extern "C" int scf_batch_norm_train_route(int N, int C, int HW, int aligned, int* route) {
  if (!route) return SCF_EINVAL;
  BntRoute rt;
  const int rc = bnt_route(N, C, HW, aligned != 0, rt);
  if (rc != SCF_OK) return rc;
  route[0] = rt.stats;
  route[1] = rt.vec;
  route[2] = rt.geo.K;
  route[3] = rt.geo.bpp;
  route[4] = (int)scf_cdiv((int64_t)N * rt.geo.K, 64);   // groups of 64 partials a channel's N K partials fold in
  return SCF_OK;
}

extern "C" int scf_batch_norm_train(const float* u, const float* gamma, const float* beta, float* running_mean,
                                    float* running_var, const float* res, const float* gamma_r, const float* beta_r,
                                    float* running_mean_r, float* running_var_r, int relu, float momentum, float eps, float* y,
                                    float* saved, float* saved_r, float* workspace, int64_t workspace_floats, int N, int C,
                                    int HW, scf_stream_t stream) {
  if (!u || !gamma || !beta || !y || !saved || !workspace) return SCF_EINVAL;
  if ((running_mean == nullptr) != (running_var == nullptr)) return SCF_EINVAL;
  const bool ds = gamma_r != nullptr;
  if (ds && (!res || !beta_r || !saved_r || (running_mean_r == nullptr) != (running_var_r == nullptr))) return SCF_EINVAL;
  if (!ds && (beta_r || saved_r || running_mean_r || running_var_r)) return SCF_EINVAL;
  const uintptr_t big = bnt_bits(u) | bnt_bits(res) | bnt_bits(y);
  const uintptr_t all = big | bnt_bits(gamma) | bnt_bits(beta) | bnt_bits(running_mean) | bnt_bits(running_var) |
                        bnt_bits(gamma_r) | bnt_bits(beta_r) | bnt_bits(running_mean_r) | bnt_bits(running_var_r) |
                        bnt_bits(saved) | bnt_bits(saved_r) | bnt_bits(workspace);
  if (all & 3) return SCF_EINVAL;
  BntRoute rt;
  const int rc = bnt_route(N, C, HW, (big & 15) == 0, rt);
  if (rc != SCF_OK) return rc;
  const BntGeom& geo = rt.geo;
  if (workspace_floats < 6 * geo.chunks) return SCF_EINVAL;
  hipStream_t st = scf_stream(stream);
  const dim3 blk(BNT_NT), sgrid((unsigned)geo.chunks), agrid((unsigned)geo.blocks);
  const bool vec = rt.vec;
  float* ws_r = workspace + 3 * geo.chunks;
  auto stats = [&](const float* x, float* ws) {
    if (rt.stats == 1) scf_launch((bnt_stats_kernel<1>), sgrid, blk, 0, st, x, ws, HW, geo.K);
    else if (rt.stats == 4) scf_launch((bnt_stats_kernel<4>), sgrid, blk, 0, st, x, ws, HW, geo.K);
    else if (rt.stats == 16) scf_launch((bnt_stats_kernel<16>), sgrid, blk, 0, st, x, ws, HW, geo.K);
    else scf_launch(bnt_stats_loop_kernel, sgrid, blk, 0, st, x, ws, HW, geo.K);
  };
  stats(u, workspace);
  if (ds) stats(res, ws_r);
  const BntSet pa = {gamma, beta, running_mean, running_var, saved};
  const BntSet pb = {gamma_r, beta_r, running_mean_r, running_var_r, saved_r};
#define BNT_APPLY(V, F)                                                                                             \
  scf_launch((bnt_apply_kernel<V, F>), agrid, blk, 0, st, u, res, pa, pb, (const float*)workspace, y, N, C, HW, geo.K, \
             geo.bpp, relu, momentum, eps)
  const int form = ds ? 2 : (res ? 1 : 0);
  if (vec) {
    if (form == 0) BNT_APPLY(true, 0); else if (form == 1) BNT_APPLY(true, 1); else BNT_APPLY(true, 2);
  } else {
    if (form == 0) BNT_APPLY(false, 0); else if (form == 1) BNT_APPLY(false, 1); else BNT_APPLY(false, 2);
  }
#undef BNT_APPLY
  return scf_launch_status();
}

extern "C" int scf_batch_norm_train_grad(const float* g, const float* y, const float* u, const float* r, const float* saved,
                                         const float* saved_r, const float* gamma, const float* gamma_r, float* gp, float* du,
                                         float* dr, float* dgamma, float* dbeta, float* dgamma_r, float* dbeta_r,
                                         int accumulate, float* workspace, int64_t workspace_floats, int N, int C, int HW,
                                         scf_stream_t stream) {
  if (!g || !u || !saved || !gamma || !du || !dgamma || !dbeta || !workspace) return SCF_EINVAL;
  const bool ds = r != nullptr;
  if (ds && (!y || gp || !saved_r || !gamma_r || !dr || !dgamma_r || !dbeta_r)) return SCF_EINVAL;
  if (!ds && ((y == nullptr) != (gp == nullptr) || saved_r || gamma_r || dr || dgamma_r || dbeta_r)) return SCF_EINVAL;
  const bool tail = y != nullptr;
  const uintptr_t big = bnt_bits(g) | bnt_bits(y) | bnt_bits(u) | bnt_bits(r) | bnt_bits(gp) | bnt_bits(du) | bnt_bits(dr);
  const uintptr_t all = big | bnt_bits(saved) | bnt_bits(saved_r) | bnt_bits(gamma) | bnt_bits(gamma_r) | bnt_bits(dgamma) |
                        bnt_bits(dbeta) | bnt_bits(dgamma_r) | bnt_bits(dbeta_r) | bnt_bits(workspace);
  if (all & 3) return SCF_EINVAL;
  BntRoute rt;
  const int rc = bnt_route(N, C, HW, (big & 15) == 0, rt);
  if (rc != SCF_OK) return rc;
  const BntGeom& geo = rt.geo;
  if (workspace_floats < 6 * geo.chunks) return SCF_EINVAL;
  hipStream_t st = scf_stream(stream);
  const dim3 blk(BNT_NT), rgrid((unsigned)geo.chunks), agrid((unsigned)geo.blocks);
  const bool vec = rt.vec;
#define BNT_REDUCE(V, T, D) \
  scf_launch((bnt_grad_reduce_kernel<V, T, D>), rgrid, blk, 0, st, g, y, u, r, saved, saved_r, gp, workspace, C, HW, geo.K)
  if (vec) {
    if (ds) BNT_REDUCE(true, true, true); else if (tail) BNT_REDUCE(true, true, false); else BNT_REDUCE(true, false, false);
  } else {
    if (ds) BNT_REDUCE(false, true, true); else if (tail) BNT_REDUCE(false, true, false); else BNT_REDUCE(false, false, false);
  }
#undef BNT_REDUCE
  const float* gq = (tail && !ds) ? gp : g;   // the tail form's apply pass reads the masked g' of the reduce pass
#define BNT_GAPPLY(V, D)                                                                                                  \
  scf_launch((bnt_grad_apply_kernel<V, D>), agrid, blk, 0, st, gq, y, u, r, saved, saved_r, gamma, gamma_r,                \
             (const float*)workspace, du, dr, dgamma, dbeta, dgamma_r, dbeta_r, accumulate, N, C, HW, geo.K, geo.bpp)
  if (vec) {
    if (ds) BNT_GAPPLY(true, true); else BNT_GAPPLY(true, false);
  } else {
    if (ds) BNT_GAPPLY(false, true); else BNT_GAPPLY(false, false);
  }
#undef BNT_GAPPLY
  return scf_launch_status();
}
