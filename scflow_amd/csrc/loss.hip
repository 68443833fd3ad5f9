// Forward values of the supervised losses (reference models/loss/sequence_loss.py, point_matching_loss.py), for ALL
// iterations of a prediction sequence at once: the numbers the reference trains against and logs, and (the *_grad
// entries, WITH_GRAD instantiations of the same kernels) the derivative of the gamma-weighted total with respect to
// every prediction, from the same pass.
//
// (a) scf_seq_pixel_loss -- SequenceLoss over RAFTLoss (up to two flow sequences) and over L1Loss on the occlusion mask
//     (one mask sequence), one pass: the ground-truth flow and `valid` are read ONCE per pixel and kept in registers while
//     the T predictions stream by.
//         mag = sqrt(gx*gx + gy*gy)                  three separately rounded fp32 operations (torch: **2, sum, sqrt)
//         v   = (valid >= 0.5) & (mag < max_flow)    or mag < max_flow alone without `valid`
//         flow_i = w * (float)sum(v*|px-gx| + v*|py-gy|) / ((float)count(v) + eps)       valid[:, None] * loss: NaN * 0 = NaN
//         mask_i = w * ((float)sum|m - occ| / (float)(N*H*W)),  occ = mask_gt, or (gx + gy < max_flow) without one
//     occ compares the SUM OF THE TWO CHANNELS with max_flow, not the magnitude (scflow_refiner.py:230), and L1Loss ignores
//     `valid`: both restated as they are.
// (b) scf_point_matching_loss -- PointMatchingLoss / DisentanglePointMatchingLoss / RotPointMatchingLoss; for a symmetric
//     class every ground-truth-posed vertex takes its squared-L2 nearest predicted-posed vertex (brute force, difference
//     form, lowest index on exact ties), whatever the norm of the loss is.
//
// Sums: per-thread partials in a fixed order -> wave shuffle tree -> the block's waves in order through LDS -> workspace ->
// a one-block combine in block order; all in fp64, rounded to fp32 once.  No atomics: results are bitwise reproducible.
#include <math.h>

#include "scf_common.h"

#define LOSS_MAX_T 32            // device pointers per sequence carried by one launch
#define LOSS_MAX_T_TOTAL 256     // longer sequences are refused
#define LOSS_THREADS 256
#define LOSS_WAVES (LOSS_THREADS / 64)

__device__ __forceinline__ double loss_wave_sum(double s) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
  return s;
}

// ================================================================================================ (a) pixel losses
#define PIX_PER_THREAD 16
#define PIX_PER_BLOCK (LOSS_THREADS * PIX_PER_THREAD)

struct SeqPixK {
  const float* gt; const float* valid; const float* mask_gt;
  const float* seq[3][LOSS_MAX_T];      // [0] flow sequence a, [1] flow sequence b, [2] mask sequence; NULL rows are skipped
  int active[3];
  int T;                                // iterations of THIS launch (<= LOSS_MAX_T), written at t0 .. t0 + T - 1
  int t0, Tall;
  int HW, blocks_per_sample;
  float max_flow;
};

// workspace per block: [count(v)] [3][Tall] fp64 sums, all as 64-bit words
__device__ __host__ __forceinline__ int pix_ws_words(int Tall) { return 1 + 3 * Tall; }

// pixel i of a thread: VEC reads quads (HW % 4 == 0 and 16-byte aligned planes, decided by the host), else dwords
template <bool VEC>
__device__ __forceinline__ int pix_index(int p0, int tid, int i) {
  return VEC ? p0 + 4 * (tid + LOSS_THREADS * (i >> 2)) + (i & 3) : p0 + tid + LOSS_THREADS * i;
}

template <bool VEC>
__device__ __forceinline__ void pix_load(const float* plane, int p0, int tid, int HW, float (&out)[PIX_PER_THREAD]) {
  if constexpr (VEC) {
#pragma unroll
    for (int j = 0; j < PIX_PER_THREAD / 4; ++j) {
      const int p = p0 + 4 * (tid + LOSS_THREADS * j);
      float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
      if (p < HW) q = *reinterpret_cast<const float4*>(plane + p);          // HW % 4 == 0: p + 3 < HW
      out[4 * j] = q.x; out[4 * j + 1] = q.y; out[4 * j + 2] = q.z; out[4 * j + 3] = q.w;
    }
  } else {
#pragma unroll
    for (int i = 0; i < PIX_PER_THREAD; ++i) {
      const int p = p0 + tid + LOSS_THREADS * i;
      out[i] = p < HW ? plane[p] : 0.f;
    }
  }
}

// the mirror of pix_load for a gradient plane; QUAD only on the quad mapping and 16-byte aligned gradient planes
template <bool VEC, bool QUAD>
__device__ __forceinline__ void pix_store(float* plane, int p0, int tid, int HW, const float (&v)[PIX_PER_THREAD]) {
  if constexpr (VEC && QUAD) {
#pragma unroll
    for (int j = 0; j < PIX_PER_THREAD / 4; ++j) {
      const int p = p0 + 4 * (tid + LOSS_THREADS * j);
      if (p < HW) *reinterpret_cast<float4*>(plane + p) = make_float4(v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]);
    }
  } else {
#pragma unroll
    for (int i = 0; i < PIX_PER_THREAD; ++i) {
      const int p = pix_index<VEC>(p0, tid, i);
      if (p < HW) plane[p] = v[i];
    }
  }
}

// sgn(p - q) decided on the operands: 0 when equal, NaN when either is NaN, +-1 for +-inf
__device__ __forceinline__ float pix_sgn(float p, float q) { return p > q ? 1.f : (p < q ? -1.f : (p == q ? 0.f : NAN)); }

// the gradient side of one launch: coef (3, Tall) as written by seq_pixel_coef_kernel, NULL planes are not written
struct SeqPixGradK {
  float* grad[3][LOSS_MAX_T];
  const float* coef;
};

struct SeqPixNoGrad {};

// G = SeqPixNoGrad: the forward entry; G = SeqPixGradK: the same pass also writes the gradients
template <bool VEC, bool QUAD, class G>
__global__ __launch_bounds__(LOSS_THREADS)
void seq_pixel_partial_kernel(SeqPixK k, unsigned long long* ws, G gk) {
  // the validity decision and every |p - g| are the separately rounded fp32 operations of torch: no fma contraction
#pragma clang fp contract(off)
  constexpr bool WITH_GRAD = !__is_same(G, SeqPixNoGrad);
  const int n = (int)(blockIdx.x / (unsigned)k.blocks_per_sample), b = (int)(blockIdx.x - (unsigned)n * (unsigned)k.blocks_per_sample);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int p0 = b * PIX_PER_BLOCK;
  const long long base1 = (long long)n * k.HW, base2 = 2 * base1;
  float gx[PIX_PER_THREAD], gy[PIX_PER_THREAD], vf[PIX_PER_THREAD], occ[PIX_PER_THREAD];
  if (k.gt) {
    pix_load<VEC>(k.gt + base2, p0, tid, k.HW, gx);
    pix_load<VEC>(k.gt + base2 + k.HW, p0, tid, k.HW, gy);
  } else {                                               // a mask sequence against mask_gt alone
#pragma unroll
    for (int i = 0; i < PIX_PER_THREAD; ++i) gx[i] = gy[i] = 0.f;
  }
  if (k.valid) pix_load<VEC>(k.valid + base1, p0, tid, k.HW, vf);
  if (k.mask_gt) pix_load<VEC>(k.mask_gt + base1, p0, tid, k.HW, occ);
  unsigned inb = 0, cnt = 0;
#pragma unroll
  for (int i = 0; i < PIX_PER_THREAD; ++i) {
    const bool in = pix_index<VEC>(p0, tid, i) < k.HW;
    const float mag = sqrtf(gx[i] * gx[i] + gy[i] * gy[i]);
    bool v = mag < k.max_flow;
    if (k.valid) v = v && (vf[i] >= 0.5f);
    v = v && in;
    inb |= in ? (1u << i) : 0u;
    vf[i] = v ? 1.f : 0.f;
    if (!k.mask_gt) occ[i] = (gx[i] + gy[i] < k.max_flow) ? 1.f : 0.f;
    cnt += v ? 1u : 0u;
  }
  __shared__ double s_sum[LOSS_WAVES][3 * LOSS_MAX_T];
  __shared__ unsigned s_cnt[LOSS_WAVES];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o, 64);
  if (lane == 0) s_cnt[wave] = cnt;

  float a[PIX_PER_THREAD], c[PIX_PER_THREAD];
  for (int t = 0; t < k.T; ++t) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      if (!k.active[s]) continue;
      const float* px = k.seq[s][t] + base2;
      pix_load<VEC>(px, p0, tid, k.HW, a);
      pix_load<VEC>(px + k.HW, p0, tid, k.HW, c);
      double sum = 0.0;
#pragma unroll
      for (int i = 0; i < PIX_PER_THREAD; ++i) {
        if (inb & (1u << i)) {
          sum += (double)(vf[i] * fabsf(a[i] - gx[i]));        // NaN * 0 stays NaN, as valid[:, None] * loss does
          sum += (double)(vf[i] * fabsf(c[i] - gy[i]));
        }
      }
      sum = loss_wave_sum(sum);
      if (lane == 0) s_sum[wave][s * LOSS_MAX_T + t] = sum;
      if constexpr (WITH_GRAD) {
        float* gp = gk.grad[s][t];
        if (gp) {
          const float cf = gk.coef[s * k.Tall + k.t0 + t];
#pragma unroll
          for (int i = 0; i < PIX_PER_THREAD; ++i) {
            const float cv = cf * vf[i];                           // inf * 0 = NaN, as autograd's valid * (1 / 0) is
            a[i] = cv * pix_sgn(a[i], gx[i]);
            c[i] = cv * pix_sgn(c[i], gy[i]);
          }
          pix_store<VEC, QUAD>(gp + base2, p0, tid, k.HW, a);
          pix_store<VEC, QUAD>(gp + base2 + k.HW, p0, tid, k.HW, c);
        }
      }
    }
    if (k.active[2]) {
      pix_load<VEC>(k.seq[2][t] + base1, p0, tid, k.HW, a);
      double sum = 0.0;
#pragma unroll
      for (int i = 0; i < PIX_PER_THREAD; ++i)
        if (inb & (1u << i)) sum += (double)fabsf(a[i] - occ[i]);
      sum = loss_wave_sum(sum);
      if (lane == 0) s_sum[wave][2 * LOSS_MAX_T + t] = sum;
      if constexpr (WITH_GRAD) {
        float* gp = gk.grad[2][t];
        if (gp) {
          const float cf = gk.coef[2 * k.Tall + k.t0 + t];
#pragma unroll
          for (int i = 0; i < PIX_PER_THREAD; ++i) a[i] = cf * pix_sgn(a[i], occ[i]);
          pix_store<VEC, QUAD>(gp + base1, p0, tid, k.HW, a);
        }
      }
    }
  }
  __syncthreads();
  unsigned long long* o = ws + (long long)blockIdx.x * pix_ws_words(k.Tall);
  if (tid == 0) {
    unsigned long long cv = 0;
    for (int w = 0; w < LOSS_WAVES; ++w) cv += s_cnt[w];
    o[0] = cv;
  }
  for (int j = tid; j < 3 * k.T; j += LOSS_THREADS) {
    const int s = j / k.T, t = j - s * k.T;
    double v = 0.0;
    if (k.active[s]) {
      v = s_sum[0][s * LOSS_MAX_T + t];
      for (int w = 1; w < LOSS_WAVES; ++w) v += s_sum[w][s * LOSS_MAX_T + t];
    }
    o[1 + s * k.Tall + k.t0 + t] = (unsigned long long)__double_as_longlong(v);
  }
}

// the pre-pass of the gradient entry: count(v) of a block from the ground truth alone, into the word the main pass
// writes again -- the same loads and the same decision
template <bool VEC>
__global__ __launch_bounds__(LOSS_THREADS)
void seq_pixel_count_kernel(SeqPixK k, unsigned long long* ws) {
#pragma clang fp contract(off)
  const int n = (int)(blockIdx.x / (unsigned)k.blocks_per_sample), b = (int)(blockIdx.x - (unsigned)n * (unsigned)k.blocks_per_sample);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int p0 = b * PIX_PER_BLOCK;
  const long long base1 = (long long)n * k.HW, base2 = 2 * base1;
  float gx[PIX_PER_THREAD], gy[PIX_PER_THREAD], vf[PIX_PER_THREAD];
  pix_load<VEC>(k.gt + base2, p0, tid, k.HW, gx);
  pix_load<VEC>(k.gt + base2 + k.HW, p0, tid, k.HW, gy);
  if (k.valid) pix_load<VEC>(k.valid + base1, p0, tid, k.HW, vf);
  unsigned cnt = 0;
#pragma unroll
  for (int i = 0; i < PIX_PER_THREAD; ++i) {
    const float mag = sqrtf(gx[i] * gx[i] + gy[i] * gy[i]);
    bool v = mag < k.max_flow;
    if (k.valid) v = v && (vf[i] >= 0.5f);
    v = v && pix_index<VEC>(p0, tid, i) < k.HW;
    cnt += v ? 1u : 0u;
  }
  __shared__ unsigned s_cnt[LOSS_WAVES];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o, 64);
  if (lane == 0) s_cnt[wave] = cnt;
  __syncthreads();
  if (tid == 0) {
    unsigned long long cv = 0;
    for (int w = 0; w < LOSS_WAVES; ++w) cv += s_cnt[w];
    ws[(long long)blockIdx.x * pix_ws_words(k.Tall)] = cv;
  }
}

struct SeqPixFinalK {
  int active[3];
  int Tall;
  long long nblocks;
  float numel;                 // (float)(N*H*W)
  float w[3], eps[3];
  float gw[3][LOSS_MAX_T_TOTAL];        // (float)(gamma ** (T - 1 - i)), the weight torch multiplies the fp32 loss with
};

// thread j combines (sequence, iteration) j over the blocks in block order; thread s < 3 then folds the T values of sequence s
__global__ __launch_bounds__(LOSS_THREADS)
void seq_pixel_final_kernel(SeqPixFinalK k, const unsigned long long* ws, float* per_iter, float* totals) {
#pragma clang fp contract(off)
  const int words = pix_ws_words(k.Tall);
  for (int j = (int)threadIdx.x; j < 3 * k.Tall; j += LOSS_THREADS) {
    const int s = j / k.Tall;
    float val = 0.f;
    if (k.active[s]) {
      double sum = 0.0;
      unsigned long long cnt = 0;
      for (long long b = 0; b < k.nblocks; ++b) {
        sum += __longlong_as_double((long long)ws[b * words + 1 + j]);
        cnt += ws[b * words];
      }
      if (s < 2) val = k.w[s] * ((float)sum / ((float)(long long)cnt + k.eps[s]));
      else val = ((float)sum / k.numel) * k.w[s];
    }
    per_iter[j] = val;
  }
  __syncthreads();                      // per_iter was written by this block: visible after the barrier
  if (threadIdx.x < 3) {
    const int s = (int)threadIdx.x;
    float total = 0.f;
    if (k.active[s])
      for (int i = 0; i < k.Tall; ++i) total = total + k.gw[s][i] * per_iter[s * k.Tall + i];
    totals[s] = total;
  }
}

// coef[s][i] = ((upstream[s] * w_i) * loss_weight[s]) / ((float)count(v) + eps[s])   for the flow rows,
//              ((upstream[2] * w_i) * loss_weight[2]) / (float)(N*H*W)                 for the mask row: fp32, in that order
__global__ __launch_bounds__(LOSS_THREADS)
void seq_pixel_coef_kernel(SeqPixFinalK k, const unsigned long long* ws, const float* upstream, int have_count, float* coef) {
#pragma clang fp contract(off)
  const int words = pix_ws_words(k.Tall);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  __shared__ unsigned long long s_cnt[LOSS_WAVES];
  unsigned long long cnt = 0;
  if (have_count)
    for (long long b = tid; b < k.nblocks; b += LOSS_THREADS) cnt += ws[b * words];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o, 64);
  if (lane == 0) s_cnt[wave] = cnt;
  __syncthreads();
  cnt = 0;
  for (int w = 0; w < LOSS_WAVES; ++w) cnt += s_cnt[w];
  for (int j = tid; j < 3 * k.Tall; j += LOSS_THREADS) {
    const int s = j / k.Tall, i = j - s * k.Tall;
    const float up = upstream ? upstream[s] : 1.f;
    const float num = (up * k.gw[s][i]) * k.w[s];
    coef[j] = s < 2 ? num / ((float)(long long)cnt + k.eps[s]) : num / k.numel;
  }
}

static int pix_blocks(int HW) { return (HW + PIX_PER_BLOCK - 1) / PIX_PER_BLOCK; }

extern "C" int64_t scf_seq_pixel_loss_workspace_bytes(int N, int H, int W, int T) {
  if (N <= 0 || H <= 0 || W <= 0 || T <= 0 || T > LOSS_MAX_T_TOTAL || (int64_t)H * W > 0x7fffffffLL) return SCF_EINVAL;
  return (int64_t)N * pix_blocks(H * W) * pix_ws_words(T) * 8;
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

static int seq_pixel_impl(const float* gt_flow, const float* valid, const float* mask_gt, const float* const* flow_a,
                         const float* const* flow_b, const float* const* mask_seq, int T, int N, int H, int W,
                         float max_flow, const float* loss_weight, const float* eps, const double* gamma,
                         bool with_grad, const float* upstream, float* const* const* grads, float* per_iter,
                         float* totals, void* workspace, scf_stream_t stream) {
  if ((!gt_flow && (flow_a || flow_b || !mask_gt)) || !workspace || !per_iter || !totals || !loss_weight || !eps || !gamma || N <= 0 || H <= 0 || W <= 0 ||
      T <= 0 || (!flow_a && !flow_b && !mask_seq))
    return SCF_EINVAL;
  if (T > LOSS_MAX_T_TOTAL || (int64_t)H * W > 0x7fffffffLL || (int64_t)N * pix_blocks(H * W) > 0x7fffffffLL ||
      (int64_t)N * 2 * H * W > 0x7fffffffffffLL)
    return SCF_EUNSUPPORTED;
  const float* const* seqs[3] = {flow_a, flow_b, mask_seq};
  const int HW = H * W;
  bool vec = HW % 4 == 0 && aligned16(gt_flow) && aligned16(valid) && aligned16(mask_gt);      // NULL counts as aligned
  bool quad = true;                     // the gradient planes join the test: quad stores only when they all pass it too
  for (int s = 0; s < 3; ++s)
    if (seqs[s])
      for (int t = 0; t < T; ++t) {
        if (!seqs[s][t]) return SCF_EINVAL;
        vec = vec && aligned16(seqs[s][t]);
        if (with_grad && grads[s]) {
          if (!grads[s][t]) return SCF_EINVAL;
          quad = quad && aligned16(grads[s][t]);
        }
      }
  hipStream_t st = scf_stream(stream);
  unsigned long long* ws = static_cast<unsigned long long*>(workspace);
  SeqPixK k;
  k.gt = gt_flow; k.valid = valid; k.mask_gt = mask_gt; k.HW = HW; k.blocks_per_sample = pix_blocks(HW); k.max_flow = max_flow; k.Tall = T;
  for (int s = 0; s < 3; ++s) k.active[s] = seqs[s] ? 1 : 0;
  const unsigned grid = (unsigned)((int64_t)k.blocks_per_sample * N);
  SeqPixFinalK f;
  f.Tall = T; f.nblocks = grid; f.numel = (float)((int64_t)N * H * W);
  for (int s = 0; s < 3; ++s) {
    f.active[s] = k.active[s]; f.w[s] = loss_weight[s]; f.eps[s] = eps[s];
    for (int i = 0; i < LOSS_MAX_T_TOTAL; ++i) f.gw[s][i] = i < T ? (float)pow(gamma[s], (double)(T - 1 - i)) : 0.f;
  }
  SeqPixGradK gk;
  if (with_grad) {
    // count(v) depends on the ground truth alone: a pre-pass at 1/T of the traffic, then the coefficients of every
    // (row, iteration) once, so that the main pass only multiplies
    float* coef = reinterpret_cast<float*>(ws + (int64_t)grid * pix_ws_words(T));
    const int have_count = (k.active[0] || k.active[1]) ? 1 : 0;
    k.t0 = 0; k.T = 0;
    for (int s = 0; s < 3; ++s)
      for (int t = 0; t < LOSS_MAX_T; ++t) k.seq[s][t] = nullptr;
    if (have_count) {
      if (vec) scf_launch(seq_pixel_count_kernel<true>, dim3(grid), dim3(LOSS_THREADS), 0, st, k, ws);
      else scf_launch(seq_pixel_count_kernel<false>, dim3(grid), dim3(LOSS_THREADS), 0, st, k, ws);
      if (scf_launch_status() != SCF_OK) return SCF_ELAUNCH;
    }
    scf_launch(seq_pixel_coef_kernel, dim3(1), dim3(LOSS_THREADS), 0, st, f, (const unsigned long long*)ws, upstream, have_count, coef);
    if (scf_launch_status() != SCF_OK) return SCF_ELAUNCH;
    gk.coef = coef;
  }
  for (int t0 = 0; t0 < T; t0 += LOSS_MAX_T) {
    k.t0 = t0; k.T = T - t0 < LOSS_MAX_T ? T - t0 : LOSS_MAX_T;
    for (int s = 0; s < 3; ++s)
      for (int t = 0; t < LOSS_MAX_T; ++t) k.seq[s][t] = (seqs[s] && t < k.T) ? seqs[s][t0 + t] : nullptr;
    if (with_grad) {
      for (int s = 0; s < 3; ++s)
        for (int t = 0; t < LOSS_MAX_T; ++t) gk.grad[s][t] = (seqs[s] && grads[s] && t < k.T) ? grads[s][t0 + t] : nullptr;
      if (vec && quad) scf_launch(seq_pixel_partial_kernel<true, true, SeqPixGradK>, dim3(grid), dim3(LOSS_THREADS), 0, st, k, ws, gk);
      else if (vec) scf_launch(seq_pixel_partial_kernel<true, false, SeqPixGradK>, dim3(grid), dim3(LOSS_THREADS), 0, st, k, ws, gk);
      else scf_launch(seq_pixel_partial_kernel<false, false, SeqPixGradK>, dim3(grid), dim3(LOSS_THREADS), 0, st, k, ws, gk);
    } else if (vec) scf_launch(seq_pixel_partial_kernel<true, false, SeqPixNoGrad>, dim3(grid), dim3(LOSS_THREADS), 0, st, k, ws, SeqPixNoGrad());
    else scf_launch(seq_pixel_partial_kernel<false, false, SeqPixNoGrad>, dim3(grid), dim3(LOSS_THREADS), 0, st, k, ws, SeqPixNoGrad());
    if (scf_launch_status() != SCF_OK) return SCF_ELAUNCH;
  }
  scf_launch(seq_pixel_final_kernel, dim3(1), dim3(LOSS_THREADS), 0, st, f, (const unsigned long long*)ws, per_iter, totals);
  return scf_launch_status();
}

extern "C" int scf_seq_pixel_loss(const float* gt_flow, const float* valid, const float* mask_gt, const float* const* flow_a,
                                  const float* const* flow_b, const float* const* mask_seq, int T, int N, int H, int W,
                                  float max_flow, const float* loss_weight, const float* eps, const double* gamma,
                                  float* per_iter, float* totals, void* workspace, scf_stream_t stream) {
  return seq_pixel_impl(gt_flow, valid, mask_gt, flow_a, flow_b, mask_seq, T, N, H, W, max_flow, loss_weight, eps, gamma,
                        false, nullptr, nullptr, per_iter, totals, workspace, stream);
}

extern "C" int64_t scf_seq_pixel_loss_grad_workspace_bytes(int N, int H, int W, int T) {
  const int64_t fwd = scf_seq_pixel_loss_workspace_bytes(N, H, W, T);
  return fwd < 0 ? fwd : fwd + (int64_t)3 * T * 8;            // + the coefficient table
}

extern "C" int scf_seq_pixel_loss_grad(const float* gt_flow, const float* valid, const float* mask_gt,
                                       const float* const* flow_a, const float* const* flow_b,
                                       const float* const* mask_seq, int T, int N, int H, int W, float max_flow,
                                       const float* loss_weight, const float* eps, const double* gamma,
                                       const float* upstream, float* const* grad_a, float* const* grad_b,
                                       float* const* grad_mask, float* per_iter, float* totals, void* workspace,
                                       scf_stream_t stream) {
  float* const* grads[3] = {grad_a, grad_b, grad_mask};
  return seq_pixel_impl(gt_flow, valid, mask_gt, flow_a, flow_b, mask_seq, T, N, H, W, max_flow, loss_weight, eps, gamma,
                        true, upstream, grads, per_iter, totals, workspace, stream);
}

// ================================================================================================ (b) point matching
#define PM_PT 4                              // target points a thread keeps in registers
#define PM_TILE (LOSS_THREADS * PM_PT)       // targets per block = predicted points per LDS chunk
#define PM_WS_WORDS 3                        // per block: [main / rotation term] [translation or depth term] [xy term]
#define PM_GRAD_WORDS 12                     // per block of the gradient entry: sum u (x) x (9, row-major), sum u (3)

struct PmK {
  const float* verts; const int* offsets; const int* group; const int* labels; const int* symmetric;
  const float* pred_r[LOSS_MAX_T]; const float* pred_t[LOSS_MAX_T];
  const float* gt_r; const float* gt_t; const float* scale;
  int num_groups, num_classes, N, tiles, t0, Tall, max_points;
  int mode, loss_type, flags;
  float sdf;
  int* nn_idx;
};

// R p + t in the order r0 p0 + r1 p1 + r2 p2 (+ t): separately rounded, so that a point recomputed for the norm has the
// bits it had when it was compared
__device__ __forceinline__ void pm_rot(const float (&r)[9], float x, float y, float z, float (&o)[3]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < 3; ++i) o[i] = r[3 * i] * x + r[3 * i + 1] * y + r[3 * i + 2] * z;
}

__device__ __forceinline__ float pm_norm(float dx, float dy, float dz, int loss_type) {
#pragma clang fp contract(off)
  return loss_type == 1 ? fabsf(dx) + fabsf(dy) + fabsf(dz) : sqrtf(dx * dx + dy * dy + dz * dz);
}

// the reference's scaled translation: xy * s when scale_xy; z * s * factor when scale_depth, else z * factor
__device__ __forceinline__ void pm_scaled_t(const float* t, float s, int flags, float sdf, float (&o)[3]) {
#pragma clang fp contract(off)
  o[0] = (flags & SCF_PM_SCALE_XY) ? t[0] * s : t[0];
  o[1] = (flags & SCF_PM_SCALE_XY) ? t[1] * s : t[1];
  o[2] = (flags & SCF_PM_SCALE_DEPTH) ? t[2] * s * sdf : t[2] * sdf;
}

// d |d| / d d for the bits the forward normed: d / |d| (0 where |d| = 0, as autograd's norm backward) or sgn(d)
__device__ __forceinline__ void pm_unit(float dx, float dy, float dz, float nm, int loss_type, float (&u)[3]) {
#pragma clang fp contract(off)
  if (loss_type == 1) {
    u[0] = pix_sgn(dx, 0.f); u[1] = pix_sgn(dy, 0.f); u[2] = pix_sgn(dz, 0.f);
  } else if (nm == 0.f) {
    u[0] = u[1] = u[2] = 0.f;
  } else {
    u[0] = dx / nm; u[1] = dy / nm; u[2] = dz / nm;
  }
}

// gws (WITH_GRAD): PM_GRAD_WORDS sums per block, laid out like ws
template <bool WITH_GRAD>
__global__ __launch_bounds__(LOSS_THREADS)
void point_matching_partial_kernel(PmK k, double* ws, double* gws) {
  const int tile = blockIdx.x, n = blockIdx.y, tl = blockIdx.z, tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  double* out = ws + (((long long)(k.t0 + tl) * k.N + n) * k.tiles + tile) * PM_WS_WORDS;
  const int g = k.group[n], lab = k.labels[n];
  // a label or a group outside its table reads nothing; the combine kernel turns the sample into NaN
  const bool ok = g >= 0 && g < k.num_groups && lab >= 0 && lab < k.num_classes;
  const int v0 = ok ? k.offsets[g] : 0;
  int V = ok ? k.offsets[g + 1] - v0 : 0;
  if (V > k.max_points) V = k.max_points;                  // nn_idx rows and the tile count were sized by max_points
  double* gout = nullptr;
  if constexpr (WITH_GRAD) gout = gws + (((long long)(k.t0 + tl) * k.N + n) * k.tiles + tile) * PM_GRAD_WORDS;
  if (tile * PM_TILE >= V) {
    if (tid < PM_WS_WORDS) out[tid] = 0.0;
    if constexpr (WITH_GRAD)
      if (tid < PM_GRAD_WORDS) gout[tid] = 0.0;
    return;
  }
  const bool sym = k.symmetric[lab] != 0;
  float rp[9], rg[9], tp[3] = {0.f, 0.f, 0.f}, tg[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 9; ++i) { rp[i] = k.pred_r[tl][(long long)n * 9 + i]; rg[i] = k.gt_r[(long long)n * 9 + i]; }
  if (k.mode != SCF_PM_ROT) {
    const float s = k.scale ? k.scale[n] : 1.f;
    pm_scaled_t(k.pred_t[tl] + (long long)n * 3, s, k.flags, k.sdf, tp);
    pm_scaled_t(k.gt_t + (long long)n * 3, s, k.flags, k.sdf, tg);
  }
  // the translation added to the predicted-rotation points: the prediction's own (PointMatchingLoss), the ground
  // truth's (disentangled rotation term), none (RotPointMatchingLoss: both are 0)
  float tpr[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) tpr[c] = k.mode == SCF_PM_DISENTANGLE ? tg[c] : tp[c];
  const float* vb = k.verts + (long long)v0 * 3;

  float gr[PM_PT][3], tgt[PM_PT][3];                       // R_gt p, and R_gt p + t_gt
  int jv[PM_PT];
#pragma unroll
  for (int q = 0; q < PM_PT; ++q) {
#pragma clang fp contract(off)
    const int j = tile * PM_TILE + q * LOSS_THREADS + tid;
    jv[q] = j;
    const int jj = j < V ? j : V - 1;                      // an idle slot follows the last point and is never summed
    pm_rot(rg, vb[3 * (long long)jj], vb[3 * (long long)jj + 1], vb[3 * (long long)jj + 2], gr[q]);
#pragma unroll
    for (int c = 0; c < 3; ++c) tgt[q][c] = gr[q][c] + tg[c];
  }

  int best_i[PM_PT];
#pragma unroll
  for (int q = 0; q < PM_PT; ++q) best_i[q] = jv[q] < V ? jv[q] : V - 1;
  if (sym) {
    __shared__ float4 s_pts[PM_TILE];
    float best_d[PM_PT];
#pragma unroll
    for (int q = 0; q < PM_PT; ++q) { best_d[q] = INFINITY; best_i[q] = 0; }
    for (int c0 = 0; c0 < V; c0 += PM_TILE) {
      const int cnt = V - c0 < PM_TILE ? V - c0 : PM_TILE;
      __syncthreads();                                     // the previous chunk has been read by every thread
      for (int i = tid; i < cnt; i += LOSS_THREADS) {
#pragma clang fp contract(off)
        float o[3];
        const long long j = c0 + i;
        pm_rot(rp, vb[3 * j], vb[3 * j + 1], vb[3 * j + 2], o);
        s_pts[i] = make_float4(o[0] + tpr[0], o[1] + tpr[1], o[2] + tpr[2], 0.f);
      }
      __syncthreads();
      for (int i = 0; i < cnt; ++i) {
        const float4 p = s_pts[i];                         // every lane reads the same address: one broadcast
#pragma unroll
        for (int q = 0; q < PM_PT; ++q) {
          const float dx = p.x - tgt[q][0], dy = p.y - tgt[q][1], dz = p.z - tgt[q][2];
          const float d = dx * dx + dy * dy + dz * dz;     // difference form; a fused evaluation only rounds less
          if (d < best_d[q]) { best_d[q] = d; best_i[q] = c0 + i; }       // ascending index, strict <: lowest index on ties
        }
      }
    }
  }

  double s_main = 0.0, s_b = 0.0, s_c = 0.0;
  double gacc[WITH_GRAD ? PM_GRAD_WORDS : 1];
#pragma unroll
  for (int i = 0; i < (WITH_GRAD ? PM_GRAD_WORDS : 1); ++i) gacc[i] = 0.0;
#pragma unroll
  for (int q = 0; q < PM_PT; ++q) {
#pragma clang fp contract(off)
    if (jv[q] >= V) continue;
    if (k.nn_idx) k.nn_idx[((long long)(k.t0 + tl) * k.N + n) * k.max_points + jv[q]] = best_i[q];
    float o[3];
    const long long bi = best_i[q];
    if constexpr (!WITH_GRAD) {
      pm_rot(rp, vb[3 * bi], vb[3 * bi + 1], vb[3 * bi + 2], o);
      s_main += (double)pm_norm((o[0] + tpr[0]) - tgt[q][0], (o[1] + tpr[1]) - tgt[q][1], (o[2] + tpr[2]) - tgt[q][2], k.loss_type);
    } else {
      const float vx = vb[3 * bi], vy = vb[3 * bi + 1], vz = vb[3 * bi + 2];
      pm_rot(rp, vx, vy, vz, o);
      const float dx = (o[0] + tpr[0]) - tgt[q][0], dy = (o[1] + tpr[1]) - tgt[q][1], dz = (o[2] + tpr[2]) - tgt[q][2];
      const float nm = pm_norm(dx, dy, dz, k.loss_type);
      s_main += (double)nm;
      // the neighbour is a constant: d/dR of R x_idx + t is u (x) x_idx with the model-space point of the NEIGHBOUR
      float u[3];
      pm_unit(dx, dy, dz, nm, k.loss_type, u);
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        gacc[3 * i] += (double)(u[i] * vx); gacc[3 * i + 1] += (double)(u[i] * vy); gacc[3 * i + 2] += (double)(u[i] * vz);
        if (k.mode == SCF_PM_FULL) gacc[9 + i] += (double)u[i];
      }
    }
    if constexpr (!WITH_GRAD) {
      if (k.mode == SCF_PM_DISENTANGLE) {
        // per point (R_gt p + t') - (R_gt p + t_gt), as the reference builds it
        if (k.flags & SCF_PM_DISENTANGLE_Z) {
          s_b += (double)pm_norm((gr[q][0] + tg[0]) - tgt[q][0], (gr[q][1] + tg[1]) - tgt[q][1], (gr[q][2] + tp[2]) - tgt[q][2], k.loss_type);
          s_c += (double)pm_norm((gr[q][0] + tp[0]) - tgt[q][0], (gr[q][1] + tp[1]) - tgt[q][1], (gr[q][2] + tg[2]) - tgt[q][2], k.loss_type);
        } else {
          s_b += (double)pm_norm((gr[q][0] + tp[0]) - tgt[q][0], (gr[q][1] + tp[1]) - tgt[q][1], (gr[q][2] + tp[2]) - tgt[q][2], k.loss_type);
        }
      }
    } else if (k.mode == SCF_PM_DISENTANGLE) {
      // the same terms, kept apart for their derivatives
      if (k.flags & SCF_PM_DISENTANGLE_Z) {
        const float bx = (gr[q][0] + tg[0]) - tgt[q][0], by = (gr[q][1] + tg[1]) - tgt[q][1], bz = (gr[q][2] + tp[2]) - tgt[q][2];
        const float cx = (gr[q][0] + tp[0]) - tgt[q][0], cy = (gr[q][1] + tp[1]) - tgt[q][1], cz = (gr[q][2] + tg[2]) - tgt[q][2];
        const float nb = pm_norm(bx, by, bz, k.loss_type), nc = pm_norm(cx, cy, cz, k.loss_type);
        s_b += (double)nb;
        s_c += (double)nc;
        if constexpr (WITH_GRAD) {
          // the depth term's xy and the xy term's z are exact zeros, so one accumulator per component serves both
          float ub[3], uc[3];
          pm_unit(bx, by, bz, nb, k.loss_type, ub);
          pm_unit(cx, cy, cz, nc, k.loss_type, uc);
#pragma unroll
          for (int i = 0; i < 3; ++i) { gacc[9 + i] += (double)ub[i]; gacc[9 + i] += (double)uc[i]; }
        }
      } else {
        const float bx = (gr[q][0] + tp[0]) - tgt[q][0], by = (gr[q][1] + tp[1]) - tgt[q][1], bz = (gr[q][2] + tp[2]) - tgt[q][2];
        const float nb = pm_norm(bx, by, bz, k.loss_type);
        s_b += (double)nb;
        if constexpr (WITH_GRAD) {
          float ub[3];
          pm_unit(bx, by, bz, nb, k.loss_type, ub);
#pragma unroll
          for (int i = 0; i < 3; ++i) gacc[9 + i] += (double)ub[i];
        }
      }
    }
  }
  __shared__ double s_red[LOSS_WAVES][PM_WS_WORDS + (WITH_GRAD ? PM_GRAD_WORDS : 0)];
  s_main = loss_wave_sum(s_main); s_b = loss_wave_sum(s_b); s_c = loss_wave_sum(s_c);
  if (lane == 0) { s_red[wave][0] = s_main; s_red[wave][1] = s_b; s_red[wave][2] = s_c; }
  if constexpr (WITH_GRAD) {
#pragma unroll
    for (int i = 0; i < PM_GRAD_WORDS; ++i) {
      const double g = loss_wave_sum(gacc[i]);
      if (lane == 0) s_red[wave][PM_WS_WORDS + i] = g;
    }
  }
  __syncthreads();
  if (tid < PM_WS_WORDS) {
    double s = s_red[0][tid];
    for (int w = 1; w < LOSS_WAVES; ++w) s += s_red[w][tid];
    out[tid] = s;
  }
  if constexpr (WITH_GRAD) {
    if (tid >= 64 && tid < 64 + PM_GRAD_WORDS) {            // another wave than the one that folds the values
      const int i = tid - 64;
      double s = s_red[0][PM_WS_WORDS + i];
      for (int w = 1; w < LOSS_WAVES; ++w) s += s_red[w][PM_WS_WORDS + i];
      gout[i] = s;
    }
  }
}

struct PmFinalK {
  const int* offsets; const int* group; const int* labels; const float* diameter;
  int num_groups, num_classes, N, tiles, Tall, max_points, mode, flags, reduction;
  float loss_weight;
  float gw[LOSS_MAX_T_TOTAL];
};

__global__ __launch_bounds__(LOSS_THREADS)
void point_matching_final_kernel(PmFinalK k, const double* ws, float* loss_i, float* per_iter, float* total) {
#pragma clang fp contract(off)
  for (int j = (int)threadIdx.x; j < k.Tall * k.N; j += LOSS_THREADS) {
    const int n = j % k.N;
    const int g = k.group[n], lab = k.labels[n];
    float val = NAN;
    if (g >= 0 && g < k.num_groups && lab >= 0 && lab < k.num_classes) {
      int V = k.offsets[g + 1] - k.offsets[g];
      if (V > k.max_points) V = k.max_points;
      double s[PM_WS_WORDS] = {0.0, 0.0, 0.0};
      for (int tile = 0; tile < k.tiles; ++tile)
        for (int c = 0; c < PM_WS_WORDS; ++c) s[c] += ws[((long long)j * k.tiles + tile) * PM_WS_WORDS + c];
      const float fv = (float)V;
      val = (float)s[0] / fv;                                          // torch.mean of the norms (0 / 0 = NaN when empty)
      if (k.mode == SCF_PM_DISENTANGLE) {
        float tr = (float)s[1] / fv;
        if (k.flags & SCF_PM_DISENTANGLE_Z) tr = tr + (float)s[2] / fv;  // loss_depth_i + loss_xy_i
        val = tr + val;                                                // loss_trans_i + loss_rotation_i
      }
      val = val / k.diameter[lab];
    }
    loss_i[j] = val;
  }
  __syncthreads();
  for (int t = (int)threadIdx.x; t < k.Tall; t += LOSS_THREADS) {
    float s = 0.f;
    for (int n = 0; n < k.N; ++n) s = s + loss_i[(long long)t * k.N + n];          // loss = loss + loss_i, in sample order
    if (k.reduction == SCF_PM_REDUCE_MEAN) s = s / (float)k.N;
    per_iter[t] = k.loss_weight * s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float tot = 0.f;
    for (int i = 0; i < k.Tall; ++i) tot = tot + k.gw[i] * per_iter[i];
    total[0] = tot;
  }
}

// gradients of one chunk of iterations: thread j = (iteration of the chunk, sample) folds the tiles in tile order and
// scales once, in fp64, by k = upstream w_i loss_weight / (V diameter [N]); rounded to fp32 once
struct PmGradFinalK {
  float* grad_r[LOSS_MAX_T]; float* grad_t[LOSS_MAX_T];
  const float* scale; const float* upstream;
  int t0, T;
  float sdf;
};

__global__ __launch_bounds__(LOSS_THREADS)
void point_matching_grad_final_kernel(PmFinalK k, PmGradFinalK g, const double* gws) {
  for (int j = (int)threadIdx.x + (int)blockIdx.x * LOSS_THREADS; j < g.T * k.N; j += LOSS_THREADS * (int)gridDim.x) {
    const int tl = j / k.N, n = j - tl * k.N, t = g.t0 + tl;
    const int grp = k.group[n], lab = k.labels[n];
    double r[PM_GRAD_WORDS];
    const bool ok = grp >= 0 && grp < k.num_groups && lab >= 0 && lab < k.num_classes;
    if (ok) {
      int V = k.offsets[grp + 1] - k.offsets[grp];
      if (V > k.max_points) V = k.max_points;
#pragma unroll
      for (int c = 0; c < PM_GRAD_WORDS; ++c) r[c] = 0.0;
      for (int tile = 0; tile < k.tiles; ++tile)
#pragma unroll
        for (int c = 0; c < PM_GRAD_WORDS; ++c) r[c] += gws[(((long long)t * k.N + n) * k.tiles + tile) * PM_GRAD_WORDS + c];
      const double up = g.upstream ? (double)g.upstream[0] : 1.0;
      double kk = up * (double)k.gw[t] * (double)k.loss_weight / ((double)V * (double)k.diameter[lab]);   // V = 0: 0 * inf = NaN
      if (k.reduction == SCF_PM_REDUCE_MEAN) kk = kk / (double)k.N;
#pragma unroll
      for (int c = 0; c < PM_GRAD_WORDS; ++c) r[c] = kk * r[c];
      // back through t' = (t.xy * s, t.z * s * factor | t.z * factor)
      const double s = g.scale ? (double)g.scale[n] : 1.0;
      if (k.flags & SCF_PM_SCALE_XY) { r[9] = s * r[9]; r[10] = s * r[10]; }
      r[11] = (k.flags & SCF_PM_SCALE_DEPTH) ? s * (double)g.sdf * r[11] : (double)g.sdf * r[11];
    } else {
#pragma unroll
      for (int c = 0; c < PM_GRAD_WORDS; ++c) r[c] = (double)NAN;
    }
    if (g.grad_r[tl])
#pragma unroll
      for (int c = 0; c < 9; ++c) g.grad_r[tl][(long long)n * 9 + c] = (float)r[c];
    if (g.grad_t[tl])
#pragma unroll
      for (int c = 0; c < 3; ++c) g.grad_t[tl][(long long)n * 3 + c] = (float)r[9 + c];
  }
}

static int pm_tiles(int max_points) { return max_points > 0 ? (max_points + PM_TILE - 1) / PM_TILE : 1; }

extern "C" int64_t scf_point_matching_workspace_bytes(int N, int T, int max_points) {
  if (N <= 0 || T <= 0 || T > LOSS_MAX_T_TOTAL || max_points < 0) return SCF_EINVAL;
  return (int64_t)N * T * pm_tiles(max_points) * PM_WS_WORDS * 8;
}

static int point_matching_impl(const float* verts, const int32_t* offsets, int num_groups, const int32_t* group,
                               const int32_t* labels, int num_classes, const int32_t* symmetric,
                               const float* diameter, const float* const* pred_r, const float* const* pred_t,
                               int T, const float* gt_r, const float* gt_t, const float* scale_factors, int N,
                               int max_points, int mode, int loss_type, int flags, float scale_depth_factor,
                               int reduction, float loss_weight, double gamma, bool with_grad, const float* upstream,
                               float* const* grad_r, float* const* grad_t, float* loss_i, float* per_iter,
                               float* total, int32_t* nn_idx, void* workspace, scf_stream_t stream) {
  if (!verts || !offsets || !group || !labels || !symmetric || !diameter || !pred_r || !gt_r || !loss_i || !per_iter ||
      !total || !workspace || N <= 0 || T <= 0 || num_groups <= 0 || num_classes <= 0 || max_points < 0)
    return SCF_EINVAL;
  if (mode != SCF_PM_FULL && mode != SCF_PM_DISENTANGLE && mode != SCF_PM_ROT) return SCF_EINVAL;
  if (loss_type != 1 && loss_type != 2) return SCF_EINVAL;
  if (reduction != SCF_PM_REDUCE_MEAN && reduction != SCF_PM_REDUCE_SUM) return SCF_EINVAL;
  if (flags & ~(SCF_PM_DISENTANGLE_Z | SCF_PM_SCALE_XY | SCF_PM_SCALE_DEPTH)) return SCF_EINVAL;
  if (mode != SCF_PM_ROT && (!pred_t || !gt_t)) return SCF_EINVAL;
  if (mode == SCF_PM_ROT) flags = 0;
  if ((flags & (SCF_PM_SCALE_XY | SCF_PM_SCALE_DEPTH)) && !scale_factors) return SCF_EINVAL;
  if (T > LOSS_MAX_T_TOTAL || N > 65535) return SCF_EUNSUPPORTED;
  for (int t = 0; t < T; ++t)
    if (!pred_r[t] || (mode != SCF_PM_ROT && !pred_t[t]) || (with_grad && ((grad_r && !grad_r[t]) || (grad_t && !grad_t[t]))))
      return SCF_EINVAL;
  hipStream_t st = scf_stream(stream);
  PmK k;
  k.verts = verts; k.offsets = offsets; k.group = group; k.labels = labels; k.symmetric = symmetric;
  k.gt_r = gt_r; k.gt_t = gt_t; k.scale = scale_factors;
  k.num_groups = num_groups; k.num_classes = num_classes; k.N = N; k.tiles = pm_tiles(max_points); k.Tall = T;
  k.max_points = max_points; k.mode = mode; k.loss_type = loss_type; k.flags = flags; k.sdf = scale_depth_factor;
  k.nn_idx = nn_idx;
  double* ws = static_cast<double*>(workspace);
  double* gws = ws + (int64_t)N * T * k.tiles * PM_WS_WORDS;
  for (int t0 = 0; t0 < T; t0 += LOSS_MAX_T) {
    const int tc = T - t0 < LOSS_MAX_T ? T - t0 : LOSS_MAX_T;
    k.t0 = t0;
    for (int t = 0; t < LOSS_MAX_T; ++t) {
      k.pred_r[t] = t < tc ? pred_r[t0 + t] : nullptr;
      k.pred_t[t] = (t < tc && mode != SCF_PM_ROT) ? pred_t[t0 + t] : nullptr;
    }
    if (with_grad) scf_launch(point_matching_partial_kernel<true>, dim3((unsigned)k.tiles, (unsigned)N, (unsigned)tc), dim3(LOSS_THREADS), 0, st, k, ws, gws);
    else scf_launch(point_matching_partial_kernel<false>, dim3((unsigned)k.tiles, (unsigned)N, (unsigned)tc), dim3(LOSS_THREADS), 0, st, k, ws, (double*)nullptr);
    if (scf_launch_status() != SCF_OK) return SCF_ELAUNCH;
  }
  PmFinalK f;
  f.offsets = offsets; f.group = group; f.labels = labels; f.diameter = diameter;
  f.num_groups = num_groups; f.num_classes = num_classes; f.N = N; f.tiles = k.tiles; f.Tall = T; f.max_points = max_points;
  f.mode = mode; f.flags = flags; f.reduction = reduction; f.loss_weight = loss_weight;
  for (int i = 0; i < LOSS_MAX_T_TOTAL; ++i) f.gw[i] = i < T ? (float)pow(gamma, (double)(T - 1 - i)) : 0.f;
  scf_launch(point_matching_final_kernel, dim3(1), dim3(LOSS_THREADS), 0, st, f, (const double*)ws, loss_i, per_iter, total);
  if (!with_grad || scf_launch_status() != SCF_OK) return scf_launch_status();
  PmGradFinalK g;
  g.scale = scale_factors; g.upstream = upstream; g.sdf = scale_depth_factor;
  for (int t0 = 0; t0 < T; t0 += LOSS_MAX_T) {
    g.t0 = t0; g.T = T - t0 < LOSS_MAX_T ? T - t0 : LOSS_MAX_T;
    for (int t = 0; t < LOSS_MAX_T; ++t) {
      g.grad_r[t] = (grad_r && t < g.T) ? grad_r[t0 + t] : nullptr;
      g.grad_t[t] = (grad_t && mode != SCF_PM_ROT && t < g.T) ? grad_t[t0 + t] : nullptr;
    }
    const int blocks = (g.T * N + LOSS_THREADS - 1) / LOSS_THREADS;
    scf_launch(point_matching_grad_final_kernel, dim3((unsigned)blocks), dim3(LOSS_THREADS), 0, st, f, g, (const double*)gws);
    if (scf_launch_status() != SCF_OK) return SCF_ELAUNCH;
  }
  return scf_launch_status();
}

extern "C" int scf_point_matching_loss(const float* verts, const int32_t* offsets, int num_groups, const int32_t* group,
                                       const int32_t* labels, int num_classes, const int32_t* symmetric,
                                       const float* diameter, const float* const* pred_r, const float* const* pred_t,
                                       int T, const float* gt_r, const float* gt_t, const float* scale_factors, int N,
                                       int max_points, int mode, int loss_type, int flags, float scale_depth_factor,
                                       int reduction, float loss_weight, double gamma, float* loss_i, float* per_iter,
                                       float* total, int32_t* nn_idx, void* workspace, scf_stream_t stream) {
  return point_matching_impl(verts, offsets, num_groups, group, labels, num_classes, symmetric, diameter, pred_r, pred_t, T,
                             gt_r, gt_t, scale_factors, N, max_points, mode, loss_type, flags, scale_depth_factor, reduction,
                             loss_weight, gamma, false, nullptr, nullptr, nullptr, loss_i, per_iter, total, nn_idx,
                             workspace, stream);
}

extern "C" int64_t scf_point_matching_grad_workspace_bytes(int N, int T, int max_points) {
  if (N <= 0 || T <= 0 || T > LOSS_MAX_T_TOTAL || max_points < 0) return SCF_EINVAL;
  return (int64_t)N * T * pm_tiles(max_points) * (PM_WS_WORDS + PM_GRAD_WORDS) * 8;
}

extern "C" int scf_point_matching_loss_grad(const float* verts, const int32_t* offsets, int num_groups,
                                            const int32_t* group, const int32_t* labels, int num_classes,
                                            const int32_t* symmetric, const float* diameter, const float* const* pred_r,
                                            const float* const* pred_t, int T, const float* gt_r, const float* gt_t,
                                            const float* scale_factors, int N, int max_points, int mode, int loss_type,
                                            int flags, float scale_depth_factor, int reduction, float loss_weight,
                                            double gamma, const float* upstream, float* const* grad_r,
                                            float* const* grad_t, float* loss_i, float* per_iter, float* total,
                                            int32_t* nn_idx, void* workspace, scf_stream_t stream) {
  return point_matching_impl(verts, offsets, num_groups, group, labels, num_classes, symmetric, diameter, pred_r, pred_t, T,
                             gt_r, gt_t, scale_factors, N, max_points, mode, loss_type, flags, scale_depth_factor, reduction,
                             loss_weight, gamma, true, upstream, grad_r, grad_t, loss_i, per_iter, total, nn_idx,
                             workspace, stream);
}
