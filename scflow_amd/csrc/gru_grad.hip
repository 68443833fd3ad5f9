// Gate arithmetic of the ConvGRU backward (raft_decoder.py:168-253) between the convolution gradients of
// conv_s1_grad.hip, for gfx950, fp32 throughout.  One GRU pass of the forward is
//   z = sigmoid(conv_z([h | x])), r = sigmoid(conv_r([h | x])), q = tanh(conv_q([r h | x])), h' = (1 - z) h + z q
// and, with g = d loss / d h', its backward
//   u_q = g z (1 - q^2), u_z = g (q - h) z (1 - z), [g_rh | g_x] = dgrad_q(u_q), u_r = g_rh h r (1 - r),
//   g_h = g (1 - z) + g_rh r + (the h columns of dgrad_zr([u_z | u_r])).
//
//   scf_gru_gate_grad_q   (g, h, z, q) -> u_q, u_z                        [+ running sums of both]
//   scf_gru_gate_grad_r   (g, z, g_rh, h, r) -> u_r, g_rh := g (1 - z) + g_rh r   [+ running sum of u_r]
//   scf_gru_carry         out = src (+ add); src := +0 on request (the hand-over of a pass's g_h to the next pass)
//   scf_gru_gate_state    out = gate h  (q NULL: the forward's r h)  or  (1 - gate) h + gate q  (the forward's h')
//
// Every operand is a (M, n) matrix of rows n floats long with its own row stride in elements (n = C H W of a channel
// slice of a wider NCHW tensor).  Elementwise: element (m, i) of every output depends on element (m, i) of the
// inputs alone; no atomics, no allocation, no synchronisation, one order of operations (each line ONE rounding):
//
//   grad_q   t1 = g * z            dq = fma(-q, q, 1)       u_q = t1 * dq
//            d  = q - h            t2 = g * d               dz  = z * (1 - z)       u_z = t2 * dz + 0
//   grad_r   t3 = g_rh * h         dr = r * (1 - r)         u_r = t3 * dr + 0
//            a  = 1 - z            b  = g * a               g_h_direct = fma(g_rh, r, b)
//   sums     sum = first ? u : sum + u
//   carry    out = add ? src + add : src
//   state    q NULL: out = gate * h;  else  a = 1 - gate, b = a * h, out = fma(gate, q, b)
//
// dq, dz, dr are the factors of scf_act_grad (TANH: fma(-a, a, 1); SIGMOID: a * (1 - a)) applied the same way
// (cotangent times factor), so u_q == scf_act_grad(g * z, q, TANH) and u_z == scf_act_grad(g * (q - h), z, SIGMOID)
// bit for bit.  The "+ 0" (exact for every value but -0) makes a zero cotangent give +0 whatever the sign of q - h or h.
//
// HBM-bound (grad_q: 4 reads + 2 writes, + 2 reads + 2 writes with sums): a thread owns 4 consecutive floats of a row
// and moves them as one 16-byte access when every pointer is 16-byte aligned and every stride a multiple of 4 (the last
// quad of a row whose length is no multiple of 4 goes float by float); otherwise the scalar instantiation runs.  The
// grid is capped at GG_MAX_BLOCKS and strides over the rest.
#include "scf_common.h"

#define GG_THREADS 256
#define GG_MAX_BLOCKS 2048

struct GGOp { float* p; long long s; };      // base pointer (NULL: absent) and row stride

template <int V>
struct GGVal { float v[V]; };

template <int V>
__device__ __forceinline__ GGVal<V> gg_load(const GGOp& o, long long m, long long i, int cnt) {
  GGVal<V> r;
  const float* p = o.p + m * o.s + i;
  if (V == 4 && cnt == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    r.v[0] = t.x; r.v[1] = t.y; r.v[2] = t.z; r.v[3] = t.w;
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j) r.v[j] = j < cnt ? p[j] : 0.f;
  }
  return r;
}

template <int V>
__device__ __forceinline__ void gg_store(const GGOp& o, long long m, long long i, int cnt, const GGVal<V>& r) {
  float* p = o.p + m * o.s + i;
  if (V == 4 && cnt == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j)
      if (j < cnt) p[j] = r.v[j];
  }
}

template <int V>
__device__ __forceinline__ void gg_sum(const GGOp& o, long long m, long long i, int cnt, const GGVal<V>& u, int first) {
  if (!o.p) return;
  GGVal<V> s = u;
  if (!first) {
    const GGVal<V> old = gg_load<V>(o, m, i, cnt);
#pragma unroll
    for (int j = 0; j < V; ++j) s.v[j] = old.v[j] + u.v[j];
  }
  gg_store<V>(o, m, i, cnt, s);
}

struct GGQ { GGOp g, h, z, q, uq, uz, sq, sz; long long n, per, total; int first; };
struct GGR { GGOp g, z, grh, h, r, ur, sr; long long n, per, total; int first; };
struct GGC { GGOp src, add, out; long long n, per, total; int clear; };
struct GGS { GGOp h, gate, q, out; long long n, per, total; };

#pragma clang fp contract(off)

template <int V>
__global__ __launch_bounds__(GG_THREADS) void gg_grad_q_kernel(GGQ p) {
  for (long long e = (long long)blockIdx.x * GG_THREADS + threadIdx.x; e < p.total; e += (long long)gridDim.x * GG_THREADS) {
    const long long m = e / p.per, i = (e - m * p.per) * V;
    const int cnt = p.n - i < V ? (int)(p.n - i) : V;
    const GGVal<V> g = gg_load<V>(p.g, m, i, cnt), h = gg_load<V>(p.h, m, i, cnt), z = gg_load<V>(p.z, m, i, cnt),
                   q = gg_load<V>(p.q, m, i, cnt);
    GGVal<V> uq, uz;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const float t1 = g.v[j] * z.v[j];
      const float dq = __fmaf_rn(-q.v[j], q.v[j], 1.f);
      uq.v[j] = t1 * dq;
      const float d = q.v[j] - h.v[j];
      const float t2 = g.v[j] * d;
      const float dz = z.v[j] * (1.f - z.v[j]);
      uz.v[j] = t2 * dz + 0.f;
    }
    gg_store<V>(p.uq, m, i, cnt, uq);
    gg_store<V>(p.uz, m, i, cnt, uz);
    gg_sum<V>(p.sq, m, i, cnt, uq, p.first);
    gg_sum<V>(p.sz, m, i, cnt, uz, p.first);
  }
}

template <int V>
__global__ __launch_bounds__(GG_THREADS) void gg_grad_r_kernel(GGR p) {
  for (long long e = (long long)blockIdx.x * GG_THREADS + threadIdx.x; e < p.total; e += (long long)gridDim.x * GG_THREADS) {
    const long long m = e / p.per, i = (e - m * p.per) * V;
    const int cnt = p.n - i < V ? (int)(p.n - i) : V;
    const GGVal<V> g = gg_load<V>(p.g, m, i, cnt), z = gg_load<V>(p.z, m, i, cnt), grh = gg_load<V>(p.grh, m, i, cnt),
                   h = gg_load<V>(p.h, m, i, cnt), r = gg_load<V>(p.r, m, i, cnt);
    GGVal<V> ur, gh;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const float t3 = grh.v[j] * h.v[j];
      const float dr = r.v[j] * (1.f - r.v[j]);
      ur.v[j] = t3 * dr + 0.f;
      const float a = 1.f - z.v[j];
      const float b = g.v[j] * a;
      gh.v[j] = __fmaf_rn(grh.v[j], r.v[j], b);
    }
    gg_store<V>(p.ur, m, i, cnt, ur);
    gg_store<V>(p.grh, m, i, cnt, gh);           // in place: this thread's own elements, read above
    gg_sum<V>(p.sr, m, i, cnt, ur, p.first);
  }
}

template <int V>
__global__ __launch_bounds__(GG_THREADS) void gg_carry_kernel(GGC p) {
  for (long long e = (long long)blockIdx.x * GG_THREADS + threadIdx.x; e < p.total; e += (long long)gridDim.x * GG_THREADS) {
    const long long m = e / p.per, i = (e - m * p.per) * V;
    const int cnt = p.n - i < V ? (int)(p.n - i) : V;
    GGVal<V> s = gg_load<V>(p.src, m, i, cnt);
    if (p.add.p) {
      const GGVal<V> a = gg_load<V>(p.add, m, i, cnt);
#pragma unroll
      for (int j = 0; j < V; ++j) s.v[j] = s.v[j] + a.v[j];
    }
    gg_store<V>(p.out, m, i, cnt, s);
    if (p.clear) {
      GGVal<V> zero;
#pragma unroll
      for (int j = 0; j < V; ++j) zero.v[j] = 0.f;
      gg_store<V>(p.src, m, i, cnt, zero);
    }
  }
}

template <int V>
__global__ __launch_bounds__(GG_THREADS) void gg_state_kernel(GGS p) {
  for (long long e = (long long)blockIdx.x * GG_THREADS + threadIdx.x; e < p.total; e += (long long)gridDim.x * GG_THREADS) {
    const long long m = e / p.per, i = (e - m * p.per) * V;
    const int cnt = p.n - i < V ? (int)(p.n - i) : V;
    const GGVal<V> h = gg_load<V>(p.h, m, i, cnt), gate = gg_load<V>(p.gate, m, i, cnt);
    GGVal<V> o;
    if (p.q.p) {
      const GGVal<V> q = gg_load<V>(p.q, m, i, cnt);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float a = 1.f - gate.v[j];
        const float b = a * h.v[j];
        o.v[j] = __fmaf_rn(gate.v[j], q.v[j], b);
      }
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j) o.v[j] = gate.v[j] * h.v[j];
    }
    gg_store<V>(p.out, m, i, cnt, o);
  }
}

// ------------------------------------------------------------------------------------------------------------ host
static inline GGOp gg_op(const float* p, int64_t s) { GGOp o; o.p = const_cast<float*>(p); o.s = (long long)s; return o; }
static inline bool gg_bad(const float* p, int64_t s, int64_t n, bool required) {
  return p ? s < n : required;                   // a present operand needs a row stride of at least the row length
}
static inline bool gg_vec_ok(const GGOp& o) { return !o.p || ((((uintptr_t)o.p) & 15) == 0 && (o.s & 3) == 0); }

// quads (or floats) a row, the work items in all, the grid: SCF_EUNSUPPORTED past 2^62 items
static inline int gg_plan(bool vec, int M, int64_t n, long long* per, long long* total, unsigned* blocks) {
  *per = vec ? scf_cdiv(n, 4) : (long long)n;
  if (*per > (1ll << 62) / M) return SCF_EUNSUPPORTED;
  *total = *per * M;
  const long long b = scf_cdiv(*total, GG_THREADS);
  *blocks = (unsigned)(b < GG_MAX_BLOCKS ? b : GG_MAX_BLOCKS);
  return SCF_OK;
}

extern "C" int scf_gru_gate_grad_q(const float* g, int64_t g_stride, const float* h, int64_t h_stride, const float* z,
                                   int64_t z_stride, const float* q, int64_t q_stride, float* u_q, int64_t u_q_stride,
                                   float* u_z, int64_t u_z_stride, float* sum_q, int64_t sum_q_stride, float* sum_z,
                                   int64_t sum_z_stride, int first, int M, int64_t n, scf_stream_t stream) {
  if (M <= 0 || n <= 0) return SCF_EINVAL;
  if (gg_bad(g, g_stride, n, true) || gg_bad(h, h_stride, n, true) || gg_bad(z, z_stride, n, true) ||
      gg_bad(q, q_stride, n, true) || gg_bad(u_q, u_q_stride, n, true) || gg_bad(u_z, u_z_stride, n, true) ||
      gg_bad(sum_q, sum_q_stride, n, false) || gg_bad(sum_z, sum_z_stride, n, false))
    return SCF_EINVAL;
  GGQ p;
  p.g = gg_op(g, g_stride); p.h = gg_op(h, h_stride); p.z = gg_op(z, z_stride); p.q = gg_op(q, q_stride);
  p.uq = gg_op(u_q, u_q_stride); p.uz = gg_op(u_z, u_z_stride); p.sq = gg_op(sum_q, sum_q_stride);
  p.sz = gg_op(sum_z, sum_z_stride);
  p.n = n; p.first = first != 0;
  const bool vec = gg_vec_ok(p.g) && gg_vec_ok(p.h) && gg_vec_ok(p.z) && gg_vec_ok(p.q) && gg_vec_ok(p.uq) &&
                   gg_vec_ok(p.uz) && gg_vec_ok(p.sq) && gg_vec_ok(p.sz);
  unsigned blocks;
  const int rc = gg_plan(vec, M, n, &p.per, &p.total, &blocks);
  if (rc != SCF_OK) return rc;
  if (vec) scf_launch(gg_grad_q_kernel<4>, dim3(blocks), dim3(GG_THREADS), 0, scf_stream(stream), p);
  else scf_launch(gg_grad_q_kernel<1>, dim3(blocks), dim3(GG_THREADS), 0, scf_stream(stream), p);
  return scf_launch_status();
}

extern "C" int scf_gru_gate_grad_r(const float* g, int64_t g_stride, const float* z, int64_t z_stride, float* g_rh,
                                   int64_t g_rh_stride, const float* h, int64_t h_stride, const float* r, int64_t r_stride,
                                   float* u_r, int64_t u_r_stride, float* sum_r, int64_t sum_r_stride, int first, int M,
                                   int64_t n, scf_stream_t stream) {
  if (M <= 0 || n <= 0) return SCF_EINVAL;
  if (gg_bad(g, g_stride, n, true) || gg_bad(z, z_stride, n, true) || gg_bad(g_rh, g_rh_stride, n, true) ||
      gg_bad(h, h_stride, n, true) || gg_bad(r, r_stride, n, true) || gg_bad(u_r, u_r_stride, n, true) ||
      gg_bad(sum_r, sum_r_stride, n, false))
    return SCF_EINVAL;
  GGR p;
  p.g = gg_op(g, g_stride); p.z = gg_op(z, z_stride); p.grh = gg_op(g_rh, g_rh_stride); p.h = gg_op(h, h_stride);
  p.r = gg_op(r, r_stride); p.ur = gg_op(u_r, u_r_stride); p.sr = gg_op(sum_r, sum_r_stride);
  p.n = n; p.first = first != 0;
  const bool vec = gg_vec_ok(p.g) && gg_vec_ok(p.z) && gg_vec_ok(p.grh) && gg_vec_ok(p.h) && gg_vec_ok(p.r) &&
                   gg_vec_ok(p.ur) && gg_vec_ok(p.sr);
  unsigned blocks;
  const int rc = gg_plan(vec, M, n, &p.per, &p.total, &blocks);
  if (rc != SCF_OK) return rc;
  if (vec) scf_launch(gg_grad_r_kernel<4>, dim3(blocks), dim3(GG_THREADS), 0, scf_stream(stream), p);
  else scf_launch(gg_grad_r_kernel<1>, dim3(blocks), dim3(GG_THREADS), 0, scf_stream(stream), p);
  return scf_launch_status();
}

extern "C" int scf_gru_carry(float* src, int64_t src_stride, const float* add, int64_t add_stride, float* out,
                             int64_t out_stride, int clear, int M, int64_t n, scf_stream_t stream) {
  if (M <= 0 || n <= 0) return SCF_EINVAL;
  if (gg_bad(src, src_stride, n, true) || gg_bad(add, add_stride, n, false) || gg_bad(out, out_stride, n, true))
    return SCF_EINVAL;
  GGC p;
  p.src = gg_op(src, src_stride); p.add = gg_op(add, add_stride); p.out = gg_op(out, out_stride);
  p.n = n; p.clear = clear != 0;
  const bool vec = gg_vec_ok(p.src) && gg_vec_ok(p.add) && gg_vec_ok(p.out);
  unsigned blocks;
  const int rc = gg_plan(vec, M, n, &p.per, &p.total, &blocks);
  if (rc != SCF_OK) return rc;
  if (vec) scf_launch(gg_carry_kernel<4>, dim3(blocks), dim3(GG_THREADS), 0, scf_stream(stream), p);
  else scf_launch(gg_carry_kernel<1>, dim3(blocks), dim3(GG_THREADS), 0, scf_stream(stream), p);
  return scf_launch_status();
}

extern "C" int scf_gru_gate_state(const float* h, int64_t h_stride, const float* gate, int64_t gate_stride, const float* q,
                                  int64_t q_stride, float* out, int64_t out_stride, int M, int64_t n,
                                  scf_stream_t stream) {
  if (M <= 0 || n <= 0) return SCF_EINVAL;
  if (gg_bad(h, h_stride, n, true) || gg_bad(gate, gate_stride, n, true) || gg_bad(q, q_stride, n, false) ||
      gg_bad(out, out_stride, n, true))
    return SCF_EINVAL;
  GGS p;
  p.h = gg_op(h, h_stride); p.gate = gg_op(gate, gate_stride); p.q = gg_op(q, q_stride); p.out = gg_op(out, out_stride);
  p.n = n;
  const bool vec = gg_vec_ok(p.h) && gg_vec_ok(p.gate) && gg_vec_ok(p.q) && gg_vec_ok(p.out);
  unsigned blocks;
  const int rc = gg_plan(vec, M, n, &p.per, &p.total, &blocks);
  if (rc != SCF_OK) return rc;
  if (vec) scf_launch(gg_state_kernel<4>, dim3(blocks), dim3(GG_THREADS), 0, scf_stream(stream), p);
  else scf_launch(gg_state_kernel<1>, dim3(blocks), dim3(GG_THREADS), 0, scf_stream(stream), p);
  return scf_launch_status();
}
