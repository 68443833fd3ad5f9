// Multi-tensor optimizer step for gfx950: the L2 norm of a list of gradient tensors and clip + AdamW over the same list,
// three launches whatever the number of tensors.
//
// The tensors are cut into chunks of SCF_ADAMW_CHUNK elements (the last chunk of a tensor is ragged); block b owns chunk b
// of a device table of (tensor, length, offset) and finds the tensor's base in per-role device tables of pointers.
//
//   adamw_sqnorm_kernel   partial[b] = sum of g^2 over chunk b, in a FIXED order: every lane adds its own elements in
//                         address order (scalar head, 16-byte vectors at stride 256, scalar tail), the 64 lanes of a wave
//                         fold by halves (xor 32, 16, ..., 1), the 4 waves add through LDS in wave order.  No atomics.
//   adamw_norm_finish     one block: the same fixed-order sum over partial[], then sqrt -> *norm.
//   adamw_update_kernel   c = min(max_norm / (norm + 1e-6), 1) (NaN propagates, as torch.clamp), then per element
//                           g' = c g;  p = p (1 - lr wd);  m = m + (g' - m)(1 - beta1);  v = beta2 v + (1 - beta2) g'^2;
//                           p = p - (lr / bc1) (m / (sqrt(v) / sqrt(bc2) + eps))
//                         -- torch.optim.AdamW after clip_grad_norm_, in torch's operation order.  The clipped gradient is
//                         NOT written back (the reference clips .grad in place; nothing reads it afterwards).
//
// The order of the norm's additions depends on the chunking AND on the 16-byte phase of each gradient's base (the head is
// (16 - base % 16) / 4 elements): the same values at another alignment or in another arrangement may differ in the last bits;
// the same pointers give the same bits on every run.
//
// Alignment is not assumed: a chunk takes 16-byte accesses from the first element at which the parameter's address is a
// multiple of 16, provided the other three roles are 16-byte aligned at that element too; otherwise the whole chunk is
// scalar.  Chunk offsets are multiples of SCF_ADAMW_CHUNK, so a chunk's phase is its tensor's.
#include "scf_common.h"

#define ADAMW_THREADS 256
#define ADAMW_WAVES (ADAMW_THREADS / SCF_WAVE)

static_assert((SCF_ADAMW_CHUNK & (SCF_ADAMW_CHUNK - 1)) == 0, "SCF_ADAMW_CHUNK must be a power of two");
static_assert(SCF_ADAMW_CHUNK % (4 * ADAMW_THREADS) == 0, "a full chunk is a whole number of 16-byte rounds of the block");
static_assert(SCF_ADAMW_NORM_THREADS == ADAMW_THREADS, "the header states the block size the norm's depth is counted from");

// elements in front of the first 16-byte boundary of `p` (0..3), at most `len`
__device__ __forceinline__ int adamw_head(const void* p, int len) {
  const int h = (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) >> 2);
  return h < len ? h : len;
}

// fixed-order sum over the block: lanes by halves, then the waves in order; every thread returns the total
__device__ __forceinline__ float adamw_block_sum(float acc, float* lds) {
#pragma unroll
  for (int off = SCF_WAVE / 2; off > 0; off >>= 1) acc += __shfl_xor(acc, off, SCF_WAVE);
  const int wave = threadIdx.x / SCF_WAVE;
  if ((threadIdx.x & (SCF_WAVE - 1)) == 0) lds[wave] = acc;
  __syncthreads();
  float total = lds[0];
#pragma unroll
  for (int w = 1; w < ADAMW_WAVES; ++w) total += lds[w];
  return total;
}

__global__ __launch_bounds__(ADAMW_THREADS) void adamw_sqnorm_kernel(const scf_adamw_chunk* __restrict__ chunks,
                                                                     const float* const* __restrict__ gptr,
                                                                     float* __restrict__ partial) {
  __shared__ float lds[ADAMW_WAVES];
  const scf_adamw_chunk c = chunks[blockIdx.x];
  const float* g = gptr[c.tensor] + c.offset;
  const int len = c.length, t = threadIdx.x;
  const int head = adamw_head(g, len);
  const int nvec = (len - head) >> 2;
  const int tail0 = head + 4 * nvec;
  float acc = 0.f;
  if (t < head) acc = g[t] * g[t];
  const float4* g4 = reinterpret_cast<const float4*>(g + head);
  for (int i = t; i < nvec; i += ADAMW_THREADS) {
    const float4 x = g4[i];
    acc = fmaf(x.x, x.x, acc);
    acc = fmaf(x.y, x.y, acc);
    acc = fmaf(x.z, x.z, acc);
    acc = fmaf(x.w, x.w, acc);
  }
  if (tail0 + t < len) acc = fmaf(g[tail0 + t], g[tail0 + t], acc);
  const float total = adamw_block_sum(acc, lds);
  if (t == 0) partial[blockIdx.x] = total;
}

__global__ __launch_bounds__(ADAMW_THREADS) void adamw_norm_finish(const float* __restrict__ partial, int64_t n,
                                                                   float* __restrict__ norm) {
  __shared__ float lds[ADAMW_WAVES];
  float acc = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += ADAMW_THREADS) acc += partial[i];
  const float total = adamw_block_sum(acc, lds);
  if (threadIdx.x == 0) *norm = sqrtf(total);
}

struct AdamwScalars {
  float max_norm, decay, one_minus_beta1, beta2, one_minus_beta2, step_size, bc2_sqrt, eps;
};

__device__ __forceinline__ void adamw_element(float& p, float g, float& m, float& v, float c, const AdamwScalars& s) {
  g *= c;
  p *= s.decay;
  m += (g - m) * s.one_minus_beta1;
  v = v * s.beta2 + s.one_minus_beta2 * (g * g);
  const float denom = sqrtf(v) / s.bc2_sqrt + s.eps;
  p -= s.step_size * (m / denom);
}

__global__ __launch_bounds__(ADAMW_THREADS) void adamw_update_kernel(const scf_adamw_chunk* __restrict__ chunks,
                                                                     float* const* __restrict__ pptr,
                                                                     const float* const* __restrict__ gptr,
                                                                     float* const* __restrict__ mptr,
                                                                     float* const* __restrict__ vptr,
                                                                     const float* __restrict__ norm, AdamwScalars s) {
  const scf_adamw_chunk ch = chunks[blockIdx.x];
  float* p = pptr[ch.tensor] + ch.offset;
  const float* g = gptr[ch.tensor] + ch.offset;
  float* m = mptr[ch.tensor] + ch.offset;
  float* v = vptr[ch.tensor] + ch.offset;
  const int len = ch.length, t = threadIdx.x;
  float c = 1.f;
  if (norm != nullptr) {
    const float x = s.max_norm / (*norm + 1e-6f);
    c = x > 1.f ? 1.f : x;                    // NaN > 1 is false: NaN stays, as in torch.clamp(max=1)
  }
  int head = adamw_head(p, len);
  const uintptr_t others = reinterpret_cast<uintptr_t>(g + head) | reinterpret_cast<uintptr_t>(m + head) |
                           reinterpret_cast<uintptr_t>(v + head);
  if (others & 15u) head = len;               // the roles disagree on the phase: this chunk is scalar throughout
  const int nvec = (len - head) >> 2;
  const int tail0 = head + 4 * nvec;
  for (int i = t; i < head; i += ADAMW_THREADS) adamw_element(p[i], g[i], m[i], v[i], c, s);
  float4* p4 = reinterpret_cast<float4*>(p + head);
  const float4* g4 = reinterpret_cast<const float4*>(g + head);
  float4* m4 = reinterpret_cast<float4*>(m + head);
  float4* v4 = reinterpret_cast<float4*>(v + head);
  for (int i = t; i < nvec; i += ADAMW_THREADS) {
    float4 pp = p4[i], mm = m4[i], vv = v4[i];
    const float4 gg = g4[i];
    adamw_element(pp.x, gg.x, mm.x, vv.x, c, s);
    adamw_element(pp.y, gg.y, mm.y, vv.y, c, s);
    adamw_element(pp.z, gg.z, mm.z, vv.z, c, s);
    adamw_element(pp.w, gg.w, mm.w, vv.w, c, s);
    p4[i] = pp;
    m4[i] = mm;
    v4[i] = vv;
  }
  if (tail0 + t < len) adamw_element(p[tail0 + t], g[tail0 + t], m[tail0 + t], v[tail0 + t], c, s);
}

extern "C" int64_t scf_adamw_chunks(const int64_t* sizes, int ntensors, scf_adamw_chunk* out, int64_t capacity) {
  if (ntensors < 0 || (ntensors > 0 && !sizes)) return SCF_EINVAL;
  int64_t n = 0;
  for (int i = 0; i < ntensors; ++i) {
    if (sizes[i] < 0) return SCF_EINVAL;
    for (int64_t off = 0; off < sizes[i]; off += SCF_ADAMW_CHUNK, ++n) {
      if (!out) continue;
      if (n >= capacity) return SCF_EINVAL;
      const int64_t left = sizes[i] - off;
      out[n].tensor = i;
      out[n].length = (int32_t)(left < SCF_ADAMW_CHUNK ? left : SCF_ADAMW_CHUNK);
      out[n].offset = off;
    }
  }
  return n;
}

extern "C" int scf_grad_sqnorm(const scf_adamw_chunk* chunks, int64_t nchunks, const float* const* g, float* partial,
                               float* norm, scf_stream_t stream) {
  if (nchunks < 0 || nchunks > INT32_MAX || !norm || (nchunks > 0 && (!chunks || !g || !partial))) return SCF_EINVAL;
  hipStream_t st = scf_stream(stream);
  if (nchunks > 0) scf_launch(adamw_sqnorm_kernel, dim3((unsigned)nchunks), dim3(ADAMW_THREADS), 0, st, chunks, g, partial);
  scf_launch(adamw_norm_finish, dim3(1), dim3(ADAMW_THREADS), 0, st, (const float*)partial, nchunks, norm);
  return scf_launch_status();
}

extern "C" int scf_adamw_step(const scf_adamw_chunk* chunks, int64_t nchunks, float* const* p, const float* const* g,
                              float* const* m, float* const* v, const float* norm, double max_norm, double lr,
                              double weight_decay, double beta1, double beta2, double eps, double bias_correction1,
                              double bias_correction2, scf_stream_t stream) {
  if (nchunks < 0 || nchunks > INT32_MAX) return SCF_EINVAL;
  if (nchunks == 0) return SCF_OK;
  if (!chunks || !p || !g || !m || !v) return SCF_EINVAL;
  if (!(bias_correction1 > 0.) || !(bias_correction2 > 0.)) return SCF_EINVAL;
  AdamwScalars s;
  s.max_norm = (float)max_norm;
  s.decay = (float)(1. - lr * weight_decay);
  s.one_minus_beta1 = (float)(1. - beta1);
  s.beta2 = (float)beta2;
  s.one_minus_beta2 = (float)(1. - beta2);
  s.step_size = (float)(lr / bias_correction1);
  s.bc2_sqrt = (float)sqrt(bias_correction2);
  s.eps = (float)eps;
  scf_launch(adamw_update_kernel, dim3((unsigned)nchunks), dim3(ADAMW_THREADS), 0, scf_stream(stream), chunks, p, g, m, v,
             norm, s);
  return scf_launch_status();
}
