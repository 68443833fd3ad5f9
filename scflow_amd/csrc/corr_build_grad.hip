// Adjoint of the correlation build (corr_gemm.hip; CorrelationPyramid.forward, raft_decoder.py:35-58) with respect to its
// two feature maps, for gfx950.  With G = d loss / d level 0, (N, hw, hw) row-major as scf_corr_lookup_grad writes it, and
// level0[n][i][j] = s sum_c f1[n][c][i] f2[n][c][j], s = 1/sqrt(C):
//     g_f1[n][c][i] = s sum_j G[n][i][j] f2[n][c][j]        contraction over the targets j
//     g_f2[n][c][j] = s sum_i G[n][i][j] f1[n][c][i]        contraction over the queries i
// Two batched fp32 GEMMs on v_mfma_f32_32x32x2_f32, one launch each.
//
//   block tile  : 128 channels x 128 positions of ONE sample; 4 waves as 2 x 2, each 64 x 64 = 2 x 2 accumulator
//                 fragments.  The block walks the WHOLE contraction in ascending chunks of 32; the contraction is never
//                 split across blocks.
//   operands    : g_f1  A = f2 [M = c][K = j], B = G [N = i][K = j]: both rows contiguous along the contraction;
//                 g_f2  A = f1 [M = c][K = i], B = G [K = i][N = j]: the forward's own K-major form.
//                 An operand whose memory runs along the contraction sits in LDS as [row][33]; a K-major one as [k][128].
//                 ds_read_b32 / ds_write_b32 bank a 32-lane half over 32 banks and the halves never meet: with the odd
//                 pitch 33 the 32 rows of a fragment read 32 banks, the 32 steps of a row write 32 banks, and the K-major
//                 rows are consecutive words both ways.  By that rule no access conflicts; bank conflicts were NOT measured.
//   staging     : plain global loads -> registers -> LDS, the next chunk's loads in flight while this one is contracted.
//                 Every load is a scalar 4-byte load under an explicit predicate (row < rows and step < contraction) with a
//                 +0 fill, every store is under (channel < C and position < hw): ONE route takes every N, C, h, w >= 1 and
//                 any 4-byte aligned pointers; there is no second kernel.
//   order       : per output ONE fma chain from +0 over the contraction ascending (the matrix instruction chains its two
//                 steps in order; the zero steps past the end add +0 products), then the scale ONCE: multiplied by s when
//                 sqrt(C) is a power of two (exact), else a correctly rounded division by sqrtf(C): the forward's rule.
//                 c0 of the error bound (K + c0) U s sum |G| |f| is therefore 0 resp. 2 (sqrtf's rounding and the
//                 division's), on every shape; there are no chunk combines, the accumulator runs through the chunks.
// No atomics, no allocation, no synchronisation: the bits are the same from run to run, and a sample's bits do not depend
// on the batch it travels in (a block reads and writes one sample).  A NaN at G[n][i][j] reaches g_f1[n][:, i] and
// g_f2[n][:, j] only: an output column is contracted from its own column of the B operand.
#include "scf_common.h"

typedef float cbg_f32x16 __attribute__((ext_vector_type(16)));

#define CBG_THREADS 256
#define CBG_TILE 128                  // channels / positions of a block
#define CBG_KC 32                     // contraction steps staged at a time
#define CBG_RPITCH (CBG_KC + 1)       // [row][k] operands
#define CBG_OP_FLOATS (CBG_TILE * CBG_RPITCH)      // 4224 >= 32 * 128, the K-major form

struct CbgParams {
  const float* a;        // features (N, C, hw): rows c, contraction along the row
  const float* g;        // G (N, hw, hw)
  float* out;            // (N, C, hw)
  int C, hw, ctiles, ptiles;
  float scale, divisor; int exact_scale;
};

// BK = false: out[c][i] = sum_j a[c][j] G[i][j];  BK = true: out[c][j] = sum_i a[c][i] G[i][j]
template <bool BK>
__global__ __launch_bounds__(CBG_THREADS) void cbg_kernel(CbgParams p) {
  __shared__ float As[CBG_OP_FLOATS];
  __shared__ float Bs[CBG_OP_FLOATS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l32 = lane & 31;
  const int wm = wave >> 1, wn = wave & 1;
  const int hw = p.hw, C = p.C;
  const int pt = blockIdx.x % p.ptiles;
  const int t2 = blockIdx.x / p.ptiles;
  const int ct = t2 % p.ctiles;
  const int n = t2 / p.ctiles;
  const int c0 = ct * CBG_TILE, p0 = pt * CBG_TILE;
  const float* a_n = p.a + (long long)n * C * hw;
  const float* g_n = p.g + (long long)n * hw * hw;
  // loader coordinates.  [row][k] operands: k = tid & 31, rows tid >> 5 + 8 i; K-major: column tid & 127, k = tid >> 7 + 2 i
  const int rk = tid & 31, rr = tid >> 5;
  const int kn = tid & 127, kk = tid >> 7;
  float av[16], bv[16];
  auto fetch = [&](int kc) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int c = c0 + rr + 8 * i, k = kc + rk;
      av[i] = (c < C && k < hw) ? a_n[(long long)c * hw + k] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      if (BK) {
        const int k = kc + kk + 2 * i, j = p0 + kn;
        bv[i] = (k < hw && j < hw) ? g_n[(long long)k * hw + j] : 0.f;
      } else {
        const int q = p0 + rr + 8 * i, k = kc + rk;
        bv[i] = (q < hw && k < hw) ? g_n[(long long)q * hw + k] : 0.f;
      }
    }
  };
  cbg_f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  fetch(0);
  for (int kc = 0; kc < hw; kc += CBG_KC) {
    __syncthreads();                                   // the previous chunk's operands are read
#pragma unroll
    for (int i = 0; i < 16; ++i) As[(rr + 8 * i) * CBG_RPITCH + rk] = av[i];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      if (BK) Bs[(kk + 2 * i) * CBG_TILE + kn] = bv[i];
      else Bs[(rr + 8 * i) * CBG_RPITCH + rk] = bv[i];
    }
    __syncthreads();
    if (kc + CBG_KC < hw) fetch(kc + CBG_KC);          // in flight while this chunk is contracted
    const float* ap = As + (wm * 64 + l32) * CBG_RPITCH + half;
    const float* bp = BK ? Bs + half * CBG_TILE + wn * 64 + l32 : Bs + (wn * 64 + l32) * CBG_RPITCH + half;
#pragma unroll
    for (int k = 0; k < CBG_KC; k += 2) {
      const float a0 = ap[k], a1 = ap[32 * CBG_RPITCH + k];
      const float b0 = BK ? bp[k * CBG_TILE] : bp[k];
      const float b1 = BK ? bp[k * CBG_TILE + 32] : bp[32 * CBG_RPITCH + k];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    }
  }
  // D fragment: column = lane & 31 (position), row = 8 (r >> 2) + 4 half + (r & 3) (channel)
  float* o_n = p.out + (long long)n * C * hw;
#pragma unroll
  for (int fj = 0; fj < 2; ++fj) {
    const int pos = p0 + wn * 64 + fj * 32 + l32;
    if (pos >= hw) continue;
#pragma unroll
    for (int fi = 0; fi < 2; ++fi) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int c = c0 + wm * 64 + fi * 32 + 8 * (r >> 2) + 4 * half + (r & 3);
        if (c < C) {
          const float v = acc[fi][fj][r];
          o_n[(long long)c * hw + pos] = p.exact_scale ? v * p.scale : v / p.divisor;
        }
      }
    }
  }
}

static bool cbg_overlap(const void* a, long long na, const void* b, long long nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + (uintptr_t)nb * 4u && b0 < a0 + (uintptr_t)na * 4u;
}

extern "C" int scf_corr_build_grad(const float* g_vol, const float* feat1, const float* feat2, float* g_feat1,
                                   float* g_feat2, int N, int C, int h, int w, scf_stream_t stream) {
  // everything is validated BEFORE the first launch
  if (!g_vol || !feat1 || !feat2 || !g_feat1 || !g_feat2 || N <= 0 || C <= 0 || h <= 0 || w <= 0) return SCF_EINVAL;
  const long long hw = (long long)h * w;
  if (hw > 0x7fffffffLL - CBG_TILE || (long long)C > 0x7fffffffLL - CBG_TILE) return SCF_EUNSUPPORTED;
  // N C hw and N hw hw floats, as bytes, stay inside 63 bits: bounded before they are multiplied out
  const long long cap = 0x7fffffffffffffffLL / 4;
  if ((long long)C * hw > cap / N || hw * hw > cap / N) return SCF_EUNSUPPORTED;
  const long long nf = (long long)N * C * hw, ng = (long long)N * hw * hw;
  if (cbg_overlap(g_feat1, nf, g_feat2, nf) || cbg_overlap(g_feat1, nf, g_vol, ng) || cbg_overlap(g_feat2, nf, g_vol, ng) ||
      cbg_overlap(g_feat1, nf, feat1, nf) || cbg_overlap(g_feat1, nf, feat2, nf) || cbg_overlap(g_feat2, nf, feat1, nf) ||
      cbg_overlap(g_feat2, nf, feat2, nf))
    return SCF_EINVAL;
  CbgParams p;
  p.C = C; p.hw = (int)hw;
  p.ctiles = (int)scf_cdiv(C, CBG_TILE); p.ptiles = (int)scf_cdiv(hw, CBG_TILE);
  const long long nblk = (long long)N * p.ctiles * p.ptiles;
  if (nblk > 0x7fffffffLL) return SCF_EUNSUPPORTED;
  const float sq = sqrtf((float)C);
  int ex = 0;
  p.exact_scale = (frexpf(sq, &ex) == 0.5f) ? 1 : 0;       // sqrt(C) is a power of two: the forward's rule
  p.scale = 1.0f / sq;
  p.divisor = sq;
  hipStream_t st = scf_stream(stream);
  p.a = feat2; p.g = g_vol; p.out = g_feat1;
  scf_launch(cbg_kernel<false>, dim3((unsigned)nblk), dim3(CBG_THREADS), 0, st, p);
  int rc = scf_launch_status();
  if (rc != SCF_OK) return rc;
  p.a = feat1; p.out = g_feat2;
  scf_launch(cbg_kernel<true>, dim3((unsigned)nblk), dim3(CBG_THREADS), 0, st, p);
  return scf_launch_status();
}
