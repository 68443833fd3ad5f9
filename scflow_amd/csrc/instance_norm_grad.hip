// Backward of InstanceNorm2d(eps, affine=False, biased variance) as the feature encoder uses it (norm.hip:
// scf_instance_norm, scf_instance_norm_res_norm), for gfx950.  Memory-bound like the forward: one workgroup per (n, c)
// plane; planes of up to 128 x 128 stay in registers, so each operand is read once and each result written once.
//
// With u the raw convolution output of a plane of HW elements, mean / rstd what the forward computes from it and
// xhat = (u - mean) rstd, the cotangent g' at IN(u) gives
//     du = rstd (g' - S1 / HW - xhat S2 / HW),    S1 = sum g',  S2 = sum g' xhat.
// Three forms:
//   mid       relu(IN(u)):               g' arrives masked (the consumer's dgrad epilogue)        -> du
//   tail      y = relu(IN(u) + r):       g' = G [y > 0], also the shortcut's cotangent            -> g', du
//   tail + ds y = relu(IN(u) + IN(r)):   one g' and S1, one S2 per operand                        -> du, dr
// mean and rstd are recomputed from u with the forward's partial sums in the forward's order (the same thread owns the
// same elements, the same wave / block tree, the same fused multiply-add in the sum of squares); the ReLU mask is read
// from the kept y -- the forward's own bits -- and never from a recomputed xhat.  No atomics; the summation order is
// fixed by HW alone; a plane's result depends on that plane alone.
//
// Contraction is off in this file so that the statistics keep the forward's bits (norm.hip: instance_norm_res_norm_kernel
// has the argument) and so that the float64 restatement's error model (tests/test_feature_grad_host.py) counts the
// operations that are written here, one rounding each.
#include "scf_common.h"

#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ float ing_wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// K sums over an NT-thread workgroup at once, each in norm.hip's block_sum order, results broadcast to every thread
template <int NT, int K>
__device__ __forceinline__ void ing_block_sum(float (&v)[K], float* red) {
  constexpr int NW = NT / 64;
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = ing_wave_sum(v[k]);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) red[k * NW + wave] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < NW; w += 4) s += (red[k * NW + w] + red[k * NW + w + 1]) + (red[k * NW + w + 2] + red[k * NW + w + 3]);
    v[k] = s;
  }
}

// the forward's sum of four squares: plain in its one-vector form, fma(a, a, b b) + fma(c, c, d d) in the others
template <bool FMA>
__device__ __forceinline__ float ing_sum_sq4(float a, float b, float c, float d) {
  if constexpr (!FMA) return (a * a + b * b) + (c * c + d * d);
  else return __builtin_fmaf(a, a, b * b) + __builtin_fmaf(c, c, d * d);
}

__device__ __forceinline__ float4 ing_zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

__device__ __forceinline__ float ing_mask(float g, float y) { return y > 0.f ? g : 0.f; }

// rstd (g - m1 - xhat m2): the final expression, one rounding per operation
__device__ __forceinline__ float ing_du(float g, float xhat, float m1, float m2, float rstd) {
  return ((g - m1) - xhat * m2) * rstd;
}

// ---------------------------------------------------------------------------------
// Register form: VEC4 float4 per thread and operand, 256 threads -- the forward's instance_norm_kernel<VEC4> /
// instance_norm_res_norm_kernel<VEC4> layout, so the statistics have its partial sums.
// TAIL: g is the cotangent at y and is masked here (and written to gp); DS: r is a second normalised operand.
// ---------------------------------------------------------------------------------
template <int VEC4, bool TAIL, bool DS>
__global__ __launch_bounds__(256) void instance_norm_grad_kernel(const float* g, const float* y, const float* u, const float* r,
                                                                 float* gp, float* du, float* dr, int HW, float eps) {
  constexpr int NT = 256, NS = DS ? 2 : 1;
  __shared__ float red[3 * NT / 64];
  const long long pl = blockIdx.x;
  const long long base = pl * HW;
  const int n4 = HW >> 2;
  const float4* up = reinterpret_cast<const float4*>(u + base);
  const float4* gq = reinterpret_cast<const float4*>(g + base);
  float4 uv[VEC4], gv[VEC4], rv[DS ? VEC4 : 1];
#pragma unroll
  for (int i = 0; i < VEC4; ++i) {
    const int idx = i * NT + threadIdx.x;
    const bool in = idx < n4;
    uv[i] = in ? up[idx] : ing_zero4();
    gv[i] = in ? gq[idx] : ing_zero4();
    if constexpr (DS) rv[i] = in ? reinterpret_cast<const float4*>(r + base)[idx] : ing_zero4();
    if constexpr (TAIL) {
      const float4 yv = in ? reinterpret_cast<const float4*>(y + base)[idx] : ing_zero4();
      gv[i].x = ing_mask(gv[i].x, yv.x);
      gv[i].y = ing_mask(gv[i].y, yv.y);
      gv[i].z = ing_mask(gv[i].z, yv.z);
      gv[i].w = ing_mask(gv[i].w, yv.w);
      if (!DS && in) *reinterpret_cast<float4*>(gp + base + 4ll * idx) = gv[i];
    }
  }
  // ---- the forward's statistics
  float s[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) s[k] = 0.f;
#pragma unroll
  for (int i = 0; i < VEC4; ++i) {
    s[0] += (uv[i].x + uv[i].y) + (uv[i].z + uv[i].w);
    if constexpr (DS) s[1] += (rv[i].x + rv[i].y) + (rv[i].z + rv[i].w);
  }
  ing_block_sum<NT, NS>(s, red);
  const float mu = s[0] / (float)HW;
  const float mr = DS ? s[NS - 1] / (float)HW : 0.f;
  float q[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) q[k] = 0.f;
#pragma unroll
  for (int i = 0; i < VEC4; ++i) {
    const int idx = i * NT + threadIdx.x;
    if (idx < n4) {
      q[0] += ing_sum_sq4<(VEC4 > 1)>(uv[i].x - mu, uv[i].y - mu, uv[i].z - mu, uv[i].w - mu);
      if constexpr (DS) q[1] += ing_sum_sq4<(VEC4 > 1)>(rv[i].x - mr, rv[i].y - mr, rv[i].z - mr, rv[i].w - mr);
    }
  }
  ing_block_sum<NT, NS>(q, red);
  const float rsu = 1.0f / sqrtf(q[0] / (float)HW + eps);
  const float rsr = DS ? 1.0f / sqrtf(q[NS - 1] / (float)HW + eps) : 0.f;
  // ---- xhat in place of the operands, the two (three) sums of the backward
  float t[1 + NS];
#pragma unroll
  for (int k = 0; k < 1 + NS; ++k) t[k] = 0.f;
#pragma unroll
  for (int i = 0; i < VEC4; ++i) {
    const int idx = i * NT + threadIdx.x;
    if (idx < n4) {
      uv[i].x = (uv[i].x - mu) * rsu; uv[i].y = (uv[i].y - mu) * rsu;
      uv[i].z = (uv[i].z - mu) * rsu; uv[i].w = (uv[i].w - mu) * rsu;
      t[0] += (gv[i].x + gv[i].y) + (gv[i].z + gv[i].w);
      t[1] += (gv[i].x * uv[i].x + gv[i].y * uv[i].y) + (gv[i].z * uv[i].z + gv[i].w * uv[i].w);
      if constexpr (DS) {
        rv[i].x = (rv[i].x - mr) * rsr; rv[i].y = (rv[i].y - mr) * rsr;
        rv[i].z = (rv[i].z - mr) * rsr; rv[i].w = (rv[i].w - mr) * rsr;
        t[NS] += (gv[i].x * rv[i].x + gv[i].y * rv[i].y) + (gv[i].z * rv[i].z + gv[i].w * rv[i].w);
      }
    }
  }
  ing_block_sum<NT, 1 + NS>(t, red);
  const float m1 = t[0] / (float)HW, m2 = t[1] / (float)HW;
  const float m3 = DS ? t[NS] / (float)HW : 0.f;
#pragma unroll
  for (int i = 0; i < VEC4; ++i) {
    const int idx = i * NT + threadIdx.x;
    if (idx < n4) {
      scf_store4<false>(du + base + 4ll * idx, ing_du(gv[i].x, uv[i].x, m1, m2, rsu), ing_du(gv[i].y, uv[i].y, m1, m2, rsu),
                        ing_du(gv[i].z, uv[i].z, m1, m2, rsu), ing_du(gv[i].w, uv[i].w, m1, m2, rsu));
      if constexpr (DS)
        scf_store4<false>(dr + base + 4ll * idx, ing_du(gv[i].x, rv[i].x, m1, m3, rsr), ing_du(gv[i].y, rv[i].y, m1, m3, rsr),
                          ing_du(gv[i].z, rv[i].z, m1, m3, rsr), ing_du(gv[i].w, rv[i].w, m1, m3, rsr));
    }
  }
}

// ---------------------------------------------------------------------------------
// Multi-sweep fallback: any HW, any alignment; four sweeps over the plane, the later ones out of L2.
// VEC: the forward's 1024-thread float4 layout (its planes of 16 K to 80 K elements); otherwise its generic kernel's
// 256-thread strided scalar sums.
// ---------------------------------------------------------------------------------
template <int NT, bool VEC>
struct IngSweep {
  // sum over the plane of f(element index), in the forward's per-thread order
  template <typename F4, typename F1>
  static __device__ __forceinline__ float run(int HW, F4 quad, F1 one) {
    float s = 0.f;
    if constexpr (VEC) {
      const int n4 = HW >> 2;
      for (int idx = threadIdx.x; idx < n4; idx += NT) s += quad(idx);
    } else {
      for (int i = threadIdx.x; i < HW; i += NT) s = one(i, s);
    }
    return s;
  }
};

template <int NT, bool VEC, bool TAIL, bool DS>
__global__ __launch_bounds__(NT) void instance_norm_grad_sweep_kernel(const float* g, const float* y, const float* u,
                                                                      const float* r, float* gp, float* du, float* dr, int HW,
                                                                      float eps) {
  constexpr int NS = DS ? 2 : 1;
  __shared__ float red[3 * NT / 64];
  const long long base = (long long)blockIdx.x * HW;
  const float* up = u + base;
  const float* rp = DS ? r + base : nullptr;
  const float* gq = g + base;
  const float* yp = TAIL ? y + base : nullptr;
  auto ld4 = [](const float* p, int idx) { return reinterpret_cast<const float4*>(p)[idx]; };
  auto gmask = [&](int i) { return TAIL ? ing_mask(gq[i], yp[i]) : gq[i]; };
  using S = IngSweep<NT, VEC>;
  // ---- the forward's statistics of one operand
  auto stats = [&](const float* p, float& mean, float& rstd) {
    float s[1] = {S::run(HW, [&](int idx) { const float4 v = ld4(p, idx); return (v.x + v.y) + (v.z + v.w); },
                         [&](int i, float acc) { return acc + p[i]; })};
    ing_block_sum<NT, 1>(s, red);
    mean = s[0] / (float)HW;
    const float m = mean;
    float q[1] = {S::run(HW, [&](int idx) { const float4 v = ld4(p, idx);
                                            return ing_sum_sq4<true>(v.x - m, v.y - m, v.z - m, v.w - m); },
                         [&](int i, float acc) { const float a = p[i] - m; return __builtin_fmaf(a, a, acc); })};
    ing_block_sum<NT, 1>(q, red);
    rstd = 1.0f / sqrtf(q[0] / (float)HW + eps);
  };
  float mu, rsu, mr = 0.f, rsr = 0.f;
  stats(up, mu, rsu);
  if constexpr (DS) stats(rp, mr, rsr);
  // ---- the sums of the backward
  float t[1 + NS];
  t[0] = S::run(HW, [&](int idx) { const int i = 4 * idx; return (gmask(i) + gmask(i + 1)) + (gmask(i + 2) + gmask(i + 3)); },
                [&](int i, float acc) { return acc + gmask(i); });
  auto dot = [&](const float* p, float m, float rs) {
    auto term = [&](int i) { return gmask(i) * ((p[i] - m) * rs); };
    return S::run(HW, [&](int idx) { const int i = 4 * idx; return (term(i) + term(i + 1)) + (term(i + 2) + term(i + 3)); },
                  [&](int i, float acc) { return acc + term(i); });
  };
  t[1] = dot(up, mu, rsu);
  if constexpr (DS) t[NS] = dot(rp, mr, rsr);
  ing_block_sum<NT, 1 + NS>(t, red);
  const float m1 = t[0] / (float)HW, m2 = t[1] / (float)HW;
  const float m3 = DS ? t[NS] / (float)HW : 0.f;
  for (int i = threadIdx.x; i < HW; i += NT) {
    const float gm = gmask(i);
    const float a = ing_du(gm, (up[i] - mu) * rsu, m1, m2, rsu);
    if constexpr (DS) dr[base + i] = ing_du(gm, (rp[i] - mr) * rsr, m1, m3, rsr);
    if constexpr (TAIL && !DS) gp[base + i] = gm;
    du[base + i] = a;
  }
}

template <bool TAIL, bool DS>
int ing_launch(const float* g, const float* y, const float* u, const float* r, float* gp, float* du, float* dr, int64_t planes,
               int HW, float eps, scf_stream_t stream) {
  if (planes > 0x7fffffffLL) return SCF_EUNSUPPORTED;
  hipStream_t st = scf_stream(stream);
  const dim3 grid((unsigned)planes), blk(256);
  const uintptr_t bits = (uintptr_t)g | (uintptr_t)y | (uintptr_t)u | (uintptr_t)r | (uintptr_t)gp | (uintptr_t)du | (uintptr_t)dr;
  const bool vec = (HW % 4 == 0) && ((bits & 15) == 0);
  const int n4 = HW / 4;
  // the forward's own thresholds: its statistics are summed in a layout that HW and the alignment select
  if (vec && n4 <= 256) scf_launch((instance_norm_grad_kernel<1, TAIL, DS>), grid, blk, 0, st, g, y, u, r, gp, du, dr, HW, eps);
  else if (vec && n4 <= 1024) scf_launch((instance_norm_grad_kernel<4, TAIL, DS>), grid, blk, 0, st, g, y, u, r, gp, du, dr, HW, eps);
  else if (vec && n4 <= 4096) scf_launch((instance_norm_grad_kernel<16, TAIL, DS>), grid, blk, 0, st, g, y, u, r, gp, du, dr, HW, eps);
  else if (vec && n4 <= 20480)
    scf_launch((instance_norm_grad_sweep_kernel<1024, true, TAIL, DS>), grid, dim3(1024), 0, st, g, y, u, r, gp, du, dr, HW, eps);
  else scf_launch((instance_norm_grad_sweep_kernel<256, false, TAIL, DS>), grid, blk, 0, st, g, y, u, r, gp, du, dr, HW, eps);
  return scf_launch_status();
}

}  // namespace

extern "C" int scf_instance_norm_grad(const float* g, const float* y, const float* u, float* gp, float* du, int64_t planes,
                                      int HW, float eps, scf_stream_t stream) {
  if (!g || !u || !du || planes <= 0 || HW <= 0) return SCF_EINVAL;
  if ((y == nullptr) != (gp == nullptr)) return SCF_EINVAL;
  if (y) return ing_launch<true, false>(g, y, u, nullptr, gp, du, nullptr, planes, HW, eps, stream);
  return ing_launch<false, false>(g, nullptr, u, nullptr, nullptr, du, nullptr, planes, HW, eps, stream);
}

extern "C" int scf_instance_norm_res_norm_grad(const float* g, const float* y, const float* u, const float* r, float* du,
                                               float* dr, int64_t planes, int HW, float eps, scf_stream_t stream) {
  if (!g || !y || !u || !r || !du || !dr || planes <= 0 || HW <= 0) return SCF_EINVAL;
  return ing_launch<true, true>(g, y, u, r, nullptr, du, dr, planes, HW, eps, stream);
}
