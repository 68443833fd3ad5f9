// Backward of the pose head's fully connected tail (pose_head.py:151-172, 201-211: GroupNorm + ReLU -> fc1 + ReLU -> fc2 +
// ReLU -> rotation_pred | translation_pred -> class selection), for gfx950: the vector-Jacobian product to the raw output
// of the last convolution and the gradients of every parameter on the way.  The weights are shared by the T iterations
// of a refinement pass, so all M = T N rows go through ONE launch per stage.
//
//   scf_fc_operand            the operand a forward launch (fc.hip) staged, as a finished (M, K) matrix: same bits
//   scf_pose_select_grad      the two heads and the class selection: a 9-wide contraction in plain fp32
//   scf_fc_dgrad              g_s (M, K) = (g (M, O) . W (O, K)) * [a > 0]     v_mfma_f32_32x32x2_f32, contraction over O
//   scf_fc_wgrad              dW (O, K) = sum_m g[m, o] a[m, k], db = sum_m g    v_mfma_f32_32x32x2_f32, contraction over M
//   scf_group_norm_flat_grad  GroupNorm + affine + ReLU backward on the flattened map, dgamma, dbeta
//
// No atomics, no allocation, no synchronisation: every sum has ONE order, fixed by the shapes alone.
//   dgrad   a block owns 32 rows x 128 columns (wave w: columns [32 w, 32 w + 32)); O is walked in ascending chunks of 32,
//           both operand tiles staged in LDS (g [32][33], W [32][160]: pitches in fc.hip's manner; bank conflicts not measured),
//           the next chunk's global loads in flight while this one is contracted.  Per output: ONE fma chain over o
//           ascending (zero columns past O), then the mask.  A row's result depends on that row of g alone.
//   wgrad   a block owns 32 features x 128 columns; the M rows are walked in ascending chunks of 32: a chunk is contracted
//           by a chain that starts at +0, the chunk partials are added in ascending order to a total that starts at +0,
//           `accumulate` adds the destination's previous value last.  db[o]: the same chunks, rows ascending inside.
//   no fp contraction in the plain fp32 kernels (select, GroupNorm backward): every product and sum is rounded once,
//   tests/test_fc_grad_host.py replays them.
#include "scf_common.h"

typedef float fg_f32x16 __attribute__((ext_vector_type(16)));

#define FG_THREADS 256
#define FG_CHUNK 32                   // contraction steps staged at a time (dgrad: features o, wgrad: rows m)
#define FG_COLS 128                   // output columns of a block: 4 waves x 32
#define FG_WPITCH (FG_COLS + 32)      // pitch of the [32][128] tile: rows k and k + 1 of an MFMA operand 32 words further
#define FG_GPITCH 33
#define FG_SELECT_TABLE 1024          // per-sample classes of a launch kept in LDS (more samples: looked up per row)

// ====================================================================================================== the operand
struct FgOperand {
  const float* x; int parts; long long part_stride; const float* x_bias; int x_relu;
  int gn_size, gn_hw; const float* gamma; const float* beta; float eps;
  float* out; int M, K;
};

// what fc_splitk_kernel stages before its GroupNorm: parts added in part order, + x_bias, ReLU (fmaxf: NaN -> 0)
__device__ __forceinline__ float fg_staged(const FgOperand& p, long long e, int k) {
  float v = p.x[e];
  for (int s = 1; s < p.parts; ++s) v += p.x[e + (long long)s * p.part_stride];
  if (p.x_bias) v += p.x_bias[k];
  if (p.x_relu) v = fmaxf(v, 0.f);
  return v;
}

__global__ __launch_bounds__(FG_THREADS) void fg_operand_kernel(FgOperand p) {
  const long long e = (long long)blockIdx.x * FG_THREADS + threadIdx.x;
  if (e >= (long long)p.M * p.K) return;
  p.out[e] = fg_staged(p, e, (int)(e % p.K));
}

// fc_group_norm_half's arithmetic and order (fc.hip), restated: a (row, group) pair goes to a PAIR of threads, each sums
// its half of the group serially, the halves meet in one shuffle; two-pass statistics.  Every fused multiply-add the
// forward executes is spelled out here, so that the bits do not hang on what the compiler contracts: the squares
// accumulate as q = fma(a, a, q), the result is fma(((v - mean) * rstd), gamma, beta).  One order is the compiled
// forward's and not the source's: in the unrolled half group of 32 (fc_group_norm_half<32>, groups of 64) the first two
// squares meet as fma(a0, a0, fl(a1 a1)) -- contraction may fuse either product of a0 a0 + a1 a1, and there it fused the
// first; the generic loop starts from q = 0.  tests/test_gpu_fc_grad.py holds both to the forward's staged operand.
__global__ __launch_bounds__(FG_THREADS) void fg_operand_gn_kernel(FgOperand p) {
  const long long t = (long long)blockIdx.x * FG_THREADS + threadIdx.x;
  const int gpr = p.K / p.gn_size, hsz = p.gn_size >> 1, gn_size = p.gn_size;
  const long long ngroups = (long long)p.M * gpr;
  long long gi = t >> 1;
  const bool live = gi < ngroups;
  if (!live) gi = ngroups - 1;                    // the pair of a dead slot is dead too; keep the shuffle convergent
  const int m = (int)(gi / gpr), g = (int)(gi - (long long)m * gpr);
  const int f0 = g * gn_size + (int)(t & 1) * hsz;
  const long long e0 = (long long)m * p.K + f0;
  float s = 0.f;
  for (int i = 0; i < hsz; ++i) s += fg_staged(p, e0 + i, f0 + i);
  s += __shfl_xor(s, 1);
  const float mean = s / (float)gn_size;
  float q = 0.f;
  int i0 = 0;
  if (hsz == 32) {
    const float a0 = fg_staged(p, e0, f0) - mean, a1 = fg_staged(p, e0 + 1, f0 + 1) - mean;
    q = fmaf(a0, a0, __fmul_rn(a1, a1));
    i0 = 2;
  }
  for (int i = i0; i < hsz; ++i) { const float a = fg_staged(p, e0 + i, f0 + i) - mean; q = fmaf(a, a, q); }
  q += __shfl_xor(q, 1);
  const float rstd = 1.0f / sqrtf(q / (float)gn_size + p.eps);
  if (!live) return;
  for (int i = 0; i < hsz; ++i) {
    const int c = (f0 + i) / p.gn_hw;
    const float v = fg_staged(p, e0 + i, f0 + i);
    p.out[e0 + i] = fmaxf(fmaf(__fmul_rn(v - mean, rstd), p.gamma[c], p.beta[c]), 0.f);
  }
}

extern "C" int scf_fc_operand(const float* x, int parts, int64_t part_stride, const float* x_bias, int x_relu,
                              int gn_groups, int gn_hw, const float* gn_gamma, const float* gn_beta, float gn_eps,
                              float* out, int M, int K, scf_stream_t stream) {
  if (!x || !out || M <= 0 || K <= 0 || parts < 1 || gn_groups < 0 || (parts > 1 && part_stride < (int64_t)M * K))
    return SCF_EINVAL;
  FgOperand p;
  p.x = x; p.parts = parts; p.part_stride = part_stride; p.x_bias = x_bias; p.x_relu = x_relu;
  p.gn_size = 0; p.gn_hw = 1; p.gamma = gn_gamma; p.beta = gn_beta; p.eps = gn_eps;
  p.out = out; p.M = M; p.K = K;
  const long long total = (long long)M * K;
  if (gn_groups > 0) {
    if (!gn_gamma || !gn_beta || gn_hw <= 0 || K % gn_groups != 0) return SCF_EINVAL;
    p.gn_size = K / gn_groups; p.gn_hw = gn_hw;
    if ((p.gn_size & 1) != 0) return SCF_EUNSUPPORTED;
    const long long blocks = scf_cdiv(2ll * M * gn_groups, FG_THREADS);
    if (blocks > 0x7fffffffll) return SCF_EUNSUPPORTED;
    scf_launch(fg_operand_gn_kernel, dim3((unsigned)blocks), dim3(FG_THREADS), 0, scf_stream(stream), p);
    return scf_launch_status();
  }
  const long long blocks = scf_cdiv(total, FG_THREADS);
  if (blocks > 0x7fffffffll) return SCF_EUNSUPPORTED;
  scf_launch(fg_operand_kernel, dim3((unsigned)blocks), dim3(FG_THREADS), 0, scf_stream(stream), p);
  return scf_launch_status();
}

// ================================================================================== the heads and the class selection
struct FgSelect {
  const float* g_rot; const float* g_trans; const float* Wr; const float* Wt; const float* a;
  const long long* label; int N, num_class, label_mode;
  float* g_s; float* dWr; float* dbr; float* dWt; float* dbt; int accumulate, M, K, blocks_a;
};

// pose_update_one's class of a row (pose.hip): row m of the stacked iterations is sample m % N
__device__ __forceinline__ int fg_class(const FgSelect& p, int m) {
  long long cls = (p.label_mode & SCF_POSE_LABEL_PER_SAMPLE) ? p.label[m % p.N] : p.label[0];
  if (cls < 0) cls += p.num_class;
  if (cls < 0) cls = 0;
  if (cls >= p.num_class) cls = p.num_class - 1;
  return (int)cls;
}

__global__ __launch_bounds__(FG_THREADS) void fg_select_kernel(FgSelect p) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x;
  if ((int)blockIdx.x < p.blocks_a) {
    // g_s[m][j] = (sum_r g_rot[m][r] Wr[6 c + r][j], r ascending, then sum_r g_trans[m][r] Wt[3 c + r][j]) * [a > 0]
    if (!p.g_s) return;
    const long long e = (long long)blockIdx.x * FG_THREADS + tid;
    if (e >= (long long)p.M * p.K) return;
    const int m = (int)(e / p.K), j = (int)(e - (long long)m * p.K);
    const int c = fg_class(p, m);
    float acc = 0.f;
    for (int r = 0; r < 6; ++r) acc = acc + p.g_rot[(long long)m * 6 + r] * p.Wr[(long long)(6 * c + r) * p.K + j];
    for (int r = 0; r < 3; ++r) acc = acc + p.g_trans[(long long)m * 3 + r] * p.Wt[(long long)(3 * c + r) * p.K + j];
    if (p.a) acc = p.a[e] > 0.f ? acc : 0.f;
    p.g_s[e] = acc;
    return;
  }
  // one block per row of [dWr ; dWt]: the rows m whose class selected it, ascending.  The class of a row is looked up once
  // per block (label[0]: one class for all rows -- every other block writes its zeros and leaves; per sample: a table of
  // the N classes in LDS); the bias gradient is column K of the same walk, with 1 for the activation (g * 1 is exact).
  __shared__ int s_cls[FG_SELECT_TABLE];
  int rr = (int)blockIdx.x - p.blocks_a;
  const float* g; float* dW; float* db; int wd;
  if (rr < 6 * p.num_class) { g = p.g_rot; wd = 6; dW = p.dWr; db = p.dbr; }
  else { rr -= 6 * p.num_class; g = p.g_trans; wd = 3; dW = p.dWt; db = p.dbt; }
  const int cls = rr / wd, r = rr - cls * wd;
  const bool per_sample = (p.label_mode & SCF_POSE_LABEL_PER_SAMPLE) != 0;
  const bool table = per_sample && p.N <= FG_SELECT_TABLE;
  if (table) {
    for (int n = tid; n < p.N; n += FG_THREADS) s_cls[n] = fg_class(p, n);
    __syncthreads();
  }
  const bool all = !per_sample && fg_class(p, 0) == cls, none = !per_sample && !all;
  const int T = p.M / p.N;
  for (int j = tid; j <= p.K; j += FG_THREADS) {      // j == K: the bias gradient
    float acc = 0.f;
    bool any = false;
    if (!none) {
      for (int t = 0; t < T; ++t) {
        for (int n = 0; n < p.N; ++n) {
          if (!all && (table ? s_cls[n] : fg_class(p, n)) != cls) continue;
          const int m = t * p.N + n;
          any = true;
          acc = acc + g[(long long)m * wd + r] * (j < p.K ? p.a[(long long)m * p.K + j] : 1.f);
        }
      }
    }
    float* dst = j < p.K ? dW + (long long)rr * p.K + j : db + rr;
    if (!p.accumulate) *dst = acc;
    else if (any) *dst = *dst + acc;
  }
}

extern "C" int scf_pose_select_grad(const float* g_rot, const float* g_trans, const float* Wr, const float* Wt,
                                    const float* a, const int64_t* label, int N, int num_class, int label_mode,
                                    float* g_s, float* dWr, float* dbr, float* dWt, float* dbt, int accumulate, int M,
                                    int K, scf_stream_t stream) {
  if (!g_rot || !g_trans || !label || M <= 0 || K <= 0 || N <= 0 || num_class <= 0 || M % N != 0 ||
      (label_mode & ~(SCF_POSE_LABEL_PER_SAMPLE | SCF_POSE_DEPTH_LINEAR)))
    return SCF_EINVAL;
  const bool wants_w = dWr || dbr || dWt || dbt;
  if (wants_w && (!dWr || !dbr || !dWt || !dbt || !a)) return SCF_EINVAL;       // the four come together, and need a
  if (g_s && (!Wr || !Wt)) return SCF_EINVAL;
  if (!g_s && !wants_w) return SCF_EINVAL;
  FgSelect p;
  p.g_rot = g_rot; p.g_trans = g_trans; p.Wr = Wr; p.Wt = Wt; p.a = a; p.label = (const long long*)label;
  p.N = N; p.num_class = num_class; p.label_mode = label_mode;
  p.g_s = g_s; p.dWr = dWr; p.dbr = dbr; p.dWt = dWt; p.dbt = dbt; p.accumulate = accumulate; p.M = M; p.K = K;
  const long long ba = g_s ? scf_cdiv((long long)M * K, FG_THREADS) : 0;
  const long long blocks = ba + (wants_w ? 9ll * num_class : 0);
  if (blocks > 0x7fffffffll) return SCF_EUNSUPPORTED;
  p.blocks_a = (int)ba;
  scf_launch(fg_select_kernel, dim3((unsigned)blocks), dim3(FG_THREADS), 0, scf_stream(stream), p);
  return scf_launch_status();
}

// ============================================================================================================ dgrad
struct FgGemm { const float* g; const float* W; const float* a; float* out; float* db; int M, O, K, accumulate; };

__global__ __launch_bounds__(FG_THREADS) void fg_dgrad_kernel(FgGemm p) {
  __shared__ float Gt[32 * FG_GPITCH];       // [m][o]
  __shared__ float Wt[32 * FG_WPITCH];       // [o][k]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l32 = lane & 31;
  const int k0 = blockIdx.x * FG_COLS, m0 = blockIdx.y * 32;
  // loader coordinates: g tile 32 x 32 (4 per thread), W tile 32 x 128 (16 per thread), lanes along the rows' memory
  const int go = tid & 31, gm = tid >> 5;             // + 8 i
  const int wk = tid & 127, wo = tid >> 7;            // + 2 i
  float gv[4], wv[16];
  auto fetch = [&](int oc) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = m0 + gm + 8 * i, o = oc + go;
      gv[i] = (m < p.M && o < p.O) ? p.g[(long long)m * p.O + o] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int o = oc + wo + 2 * i, k = k0 + wk;
      wv[i] = (o < p.O && k < p.K) ? p.W[(long long)o * p.K + k] : 0.f;
    }
  };
  fg_f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  fetch(0);
  for (int oc = 0; oc < p.O; oc += FG_CHUNK) {
    __syncthreads();                                   // the previous chunk's operands are read
#pragma unroll
    for (int i = 0; i < 4; ++i) Gt[(gm + 8 * i) * FG_GPITCH + go] = gv[i];
#pragma unroll
    for (int i = 0; i < 16; ++i) Wt[(wo + 2 * i) * FG_WPITCH + wk] = wv[i];
    __syncthreads();
    if (oc + FG_CHUNK < p.O) fetch(oc + FG_CHUNK);     // in flight while this chunk is contracted
    const float* ap = Gt + l32 * FG_GPITCH + half;
    const float* bp = Wt + half * FG_WPITCH + wave * 32 + l32;
#pragma unroll
    for (int o = 0; o < FG_CHUNK; o += 2)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[o], bp[o * FG_WPITCH], acc, 0, 0, 0);
  }
  const int k = k0 + wave * 32 + l32;
  if (k >= p.K) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = m0 + 8 * (r >> 2) + 4 * half + (r & 3);
    if (m < p.M) {
      const long long e = (long long)m * p.K + k;
      float v = acc[r];
      if (p.a) v = p.a[e] > 0.f ? v : 0.f;
      p.out[e] = v;
    }
  }
}

extern "C" int scf_fc_dgrad(const float* g, const float* W, const float* a, float* g_s, int M, int O, int K,
                            scf_stream_t stream) {
  if (!g || !W || !g_s || M <= 0 || O <= 0 || K <= 0) return SCF_EINVAL;
  const long long mt = scf_cdiv(M, 32), kt = scf_cdiv(K, FG_COLS);
  if (mt > 65535 || kt > 0x7fffffffll) return SCF_EUNSUPPORTED;
  FgGemm p;
  p.g = g; p.W = W; p.a = a; p.out = g_s; p.db = nullptr; p.M = M; p.O = O; p.K = K; p.accumulate = 0;
  scf_launch(fg_dgrad_kernel, dim3((unsigned)kt, (unsigned)mt), dim3(FG_THREADS), 0, scf_stream(stream), p);
  return scf_launch_status();
}

// ============================================================================================================ wgrad
__global__ __launch_bounds__(FG_THREADS) void fg_wgrad_kernel(FgGemm p) {
#pragma clang fp contract(off)
  __shared__ float Gt[32 * 32];              // [m][o]
  __shared__ float At[32 * FG_WPITCH];       // [m][k]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l32 = lane & 31;
  const int k0 = blockIdx.x * FG_COLS, o0 = blockIdx.y * 32;
  const int go = tid & 31, gm = tid >> 5;             // + 8 i
  const int ak = tid & 127, am = tid >> 7;            // + 2 i
  float gv[4], av[16];
  auto fetch = [&](int mc) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = mc + gm + 8 * i, o = o0 + go;
      gv[i] = (m < p.M && o < p.O) ? p.g[(long long)m * p.O + o] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int m = mc + am + 2 * i, k = k0 + ak;
      av[i] = (m < p.M && k < p.K) ? p.a[(long long)m * p.K + k] : 0.f;
    }
  };
  fg_f32x16 tot;
#pragma unroll
  for (int r = 0; r < 16; ++r) tot[r] = 0.f;
  float dbt = 0.f;
  const bool bias_lane = p.db && blockIdx.x == 0 && tid < 32;
  fetch(0);
  for (int mc = 0; mc < p.M; mc += FG_CHUNK) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) Gt[(gm + 8 * i) * 32 + go] = gv[i];
#pragma unroll
    for (int i = 0; i < 16; ++i) At[(am + 2 * i) * FG_WPITCH + ak] = av[i];
    __syncthreads();
    if (mc + FG_CHUNK < p.M) fetch(mc + FG_CHUNK);
    fg_f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const float* ap = Gt + half * 32 + l32;
    const float* bp = At + half * FG_WPITCH + wave * 32 + l32;
#pragma unroll
    for (int m = 0; m < FG_CHUNK; m += 2)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[m * 32], bp[m * FG_WPITCH], acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) tot[r] = tot[r] + acc[r];
    if (bias_lane) {
      float part = 0.f;
      for (int m = 0; m < FG_CHUNK; ++m) part = part + Gt[m * 32 + tid];
      dbt = dbt + part;
    }
  }
  if (bias_lane && o0 + tid < p.O) p.db[o0 + tid] = p.accumulate ? p.db[o0 + tid] + dbt : dbt;
  const int k = k0 + wave * 32 + l32;
  if (k >= p.K) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int o = o0 + 8 * (r >> 2) + 4 * half + (r & 3);
    if (o < p.O) {
      float* d = p.out + (long long)o * p.K + k;
      *d = p.accumulate ? *d + tot[r] : tot[r];
    }
  }
}

extern "C" int scf_fc_wgrad(const float* g, const float* a, float* dW, float* db, int M, int O, int K, int accumulate,
                            scf_stream_t stream) {
  if (!g || !a || !dW || M <= 0 || O <= 0 || K <= 0) return SCF_EINVAL;
  const long long ot = scf_cdiv(O, 32), kt = scf_cdiv(K, FG_COLS);
  if (ot > 65535 || kt > 0x7fffffffll) return SCF_EUNSUPPORTED;
  FgGemm p;
  p.g = g; p.W = nullptr; p.a = a; p.out = dW; p.db = db; p.M = M; p.O = O; p.K = K; p.accumulate = accumulate;
  scf_launch(fg_wgrad_kernel, dim3((unsigned)kt, (unsigned)ot), dim3(FG_THREADS), 0, scf_stream(stream), p);
  return scf_launch_status();
}

// =============================================================================================== GroupNorm backward
struct FgNorm {
  const float* g_x0; const float* y; int parts; long long part_stride; const float* x0; const float* gamma;
  int groups, gn_size, hw; float eps; float* g_y; float* dgamma; float* dbeta; int accumulate; float* stats; int M, K;
};

__device__ __forceinline__ float fg_wave_sum(float v) {      // xor butterfly: every lane ends with the same bits
#pragma clang fp contract(off)
  for (int s = 32; s >= 1; s >>= 1) v = v + __shfl_xor(v, s);
  return v;
}

__device__ __forceinline__ float fg_y(const FgNorm& p, long long e) {
  float v = p.y[e];
  for (int s = 1; s < p.parts; ++s) v += p.y[e + (long long)s * p.part_stride];
  return v;
}

// one wave per (row, group): lane l owns the elements l, l + 64, ... of the group (serial, ascending), the lanes meet
// in the butterfly.  mean and rstd are two-pass fp32 statistics like the forward's, but summed in THIS order: not the
// forward's bits (its fold adds two serial halves); the difference is inside the bound.  Kept in `stats` for the parameter pass.
__global__ __launch_bounds__(FG_THREADS) void fg_norm_grad_kernel(FgNorm p) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const long long gi = (long long)blockIdx.x * (FG_THREADS / 64) + (threadIdx.x >> 6);
  if (gi >= (long long)p.M * p.groups) return;           // whole waves leave
  const int m = (int)(gi / p.groups), g = (int)(gi - (long long)m * p.groups);
  const int f0 = g * p.gn_size;
  const long long e0 = (long long)m * p.K + f0;
  const float n = (float)p.gn_size;
  float s = 0.f;
  for (int i = lane; i < p.gn_size; i += 64) s = s + fg_y(p, e0 + i);
  const float mean = fg_wave_sum(s) / n;
  float q = 0.f;
  for (int i = lane; i < p.gn_size; i += 64) { const float a = fg_y(p, e0 + i) - mean; q = q + a * a; }
  const float rstd = 1.0f / sqrtf(fg_wave_sum(q) / n + p.eps);
  if (lane == 0) { p.stats[2 * gi] = mean; p.stats[2 * gi + 1] = rstd; }
  float sa = 0.f, sb = 0.f;
  for (int i = lane; i < p.gn_size; i += 64) {
    const float xh = (fg_y(p, e0 + i) - mean) * rstd;
    const float gu = p.x0[e0 + i] > 0.f ? p.g_x0[e0 + i] : 0.f;
    const float t = p.gamma[(f0 + i) / p.hw] * gu;
    sa = sa + t;
    sb = sb + t * xh;
  }
  const float ma = fg_wave_sum(sa) / n, mb = fg_wave_sum(sb) / n;
  for (int i = lane; i < p.gn_size; i += 64) {
    const float xh = (fg_y(p, e0 + i) - mean) * rstd;
    const float gu = p.x0[e0 + i] > 0.f ? p.g_x0[e0 + i] : 0.f;
    const float t = p.gamma[(f0 + i) / p.hw] * gu;
    p.g_y[e0 + i] = rstd * ((t - ma) - xh * mb);
  }
}

// one block per channel: thread j walks the rows j, j + 256, ... (ascending; the channel's features ascending inside a
// row), then the 256 partials fold in a fixed tree (stride 128, 64, ... 1)
__global__ __launch_bounds__(FG_THREADS) void fg_norm_param_kernel(FgNorm p) {
#pragma clang fp contract(off)
  __shared__ float sg[FG_THREADS], sb[FG_THREADS];
  const int c = blockIdx.x, tid = threadIdx.x;
  const int ks = c * p.hw, ke = min(ks + p.hw, p.K);
  float dg = 0.f, db = 0.f;
  for (int m = tid; m < p.M; m += FG_THREADS) {
    for (int k = ks; k < ke; ++k) {
      const long long e = (long long)m * p.K + k;
      const long long gi = (long long)m * p.groups + k / p.gn_size;
      const float xh = (fg_y(p, e) - p.stats[2 * gi]) * p.stats[2 * gi + 1];
      const float gu = p.x0[e] > 0.f ? p.g_x0[e] : 0.f;
      db = db + gu;
      dg = dg + gu * xh;
    }
  }
  sg[tid] = dg; sb[tid] = db;
  __syncthreads();
  for (int s = FG_THREADS / 2; s >= 1; s >>= 1) {
    if (tid < s) { sg[tid] = sg[tid] + sg[tid + s]; sb[tid] = sb[tid] + sb[tid + s]; }
    __syncthreads();
  }
  if (tid == 0) {
    p.dgamma[c] = p.accumulate ? p.dgamma[c] + sg[0] : sg[0];
    p.dbeta[c] = p.accumulate ? p.dbeta[c] + sb[0] : sb[0];
  }
}

extern "C" int scf_group_norm_flat_grad(const float* g_x0, const float* y, int y_parts, int64_t y_part_stride,
                                        const float* x0, const float* gamma, int groups, int hw, float eps, float* g_y,
                                        float* dgamma, float* dbeta, int accumulate, float* stats, int M, int K,
                                        scf_stream_t stream) {
  if (!g_x0 || !y || !x0 || !gamma || !g_y || !stats || M <= 0 || K <= 0 || groups <= 0 || hw <= 0 || y_parts < 1 ||
      (y_parts > 1 && y_part_stride < (int64_t)M * K) || (dgamma == nullptr) != (dbeta == nullptr))
    return SCF_EINVAL;
  if (K % groups != 0) return SCF_EINVAL;
  if (((K / groups) & 1) != 0) return SCF_EUNSUPPORTED;        // the forward's geometries: an even group size
  FgNorm p;
  p.g_x0 = g_x0; p.y = y; p.parts = y_parts; p.part_stride = y_part_stride; p.x0 = x0; p.gamma = gamma;
  p.groups = groups; p.gn_size = K / groups; p.hw = hw; p.eps = eps; p.g_y = g_y; p.dgamma = dgamma; p.dbeta = dbeta;
  p.accumulate = accumulate; p.stats = stats; p.M = M; p.K = K;
  const long long blocks = scf_cdiv((long long)M * groups, FG_THREADS / 64);
  if (blocks > 0x7fffffffll) return SCF_EUNSUPPORTED;
  scf_launch(fg_norm_grad_kernel, dim3((unsigned)blocks), dim3(FG_THREADS), 0, scf_stream(stream), p);
  int rc = scf_launch_status();
  if (rc != SCF_OK || !dgamma) return rc;
  scf_launch(fg_norm_param_kernel, dim3((unsigned)scf_cdiv(K, hw)), dim3(FG_THREADS), 0, scf_stream(stream), p);
  return scf_launch_status();
}
