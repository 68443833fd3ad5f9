// Flow -> 2-D/3-D correspondences, point sampling and batched RANSAC-EPnP for the pose step of the pose-free RAFT
// refiners (BaseFlowRefiner.solve_pose, models/refiner/base_flow_refiner.py:99-154), for gfx950.
//
// The reference builds the correspondences per sample with torch.nonzero (get_2d_3d_corr_by_fw_flow,
// models/utils/pose.py:182-200), optionally keeps a subset (sample_points, base_flow_refiner.py:49-71) and calls
// cv2.solvePnPRansac(SOLVEPNP_EPNP) once per sample on the CPU (pose.py:203-249).  Here the three steps are three
// launches over the whole batch, with no host synchronisation in between.
//
// Layout (one workgroup of 256 threads = 4 waves per sample in every kernel):
//   corr_2d3d_kernel   block-wide compaction in row-major order: each thread tests 16 consecutive pixels of a
//                      4096-pixel chunk, a block scan of the per-thread counts gives every kept pixel its slot.
//   pnp_select_kernel  top-`num` keys (confidence bits, or a counter-based hash for 'random') by a 4-pass
//                      8-bit radix select with an LDS histogram, then the same ordered compaction: ties go to the
//                      lower index, the selected indices stay in ascending order.
//   pnp_ransac_kernel  hypotheses are solved in rounds of 256, one minimal 5-point EPnP per thread (fp64, in
//                      registers and scratch); their 3x4 projection matrices K [R | t] are staged in LDS as fp32.
//                      Scoring walks the points in block-wide strides (one point per thread) against every
//                      hypothesis of the round; each wave counts its inliers with a ballot and adds the popcount
//                      to the hypothesis' LDS counter (integer adds: the count is order-independent).  The final
//                      EPnP over the best hypothesis' inliers accumulates its moments (PCA, 12x12 M^T M, the
//                      barycentric moments) per thread in fp64 and sums them with a fixed shuffle tree per wave and
//                      a fixed-order sum over the waves, so every result is bit-reproducible and independent of
//                      the other samples of the batch.
#include "scf_common.h"
#include "scf_pose.h"

#define PNP_THREADS 256
#define PNP_WAVES (PNP_THREADS / SCF_WAVE)
#define CORR_ITEMS 16

// ---------------------------------------------------------------------------------------------- block helpers
// exclusive prefix of `c` over the block (thread order) and the block total; every thread must call it
__device__ __forceinline__ int block_scan(int c, int* lds_w, int& total) {
  const int lane = threadIdx.x & (SCF_WAVE - 1), wid = threadIdx.x / SCF_WAVE;
  int inc = c;
  for (int o = 1; o < SCF_WAVE; o <<= 1) {
    const int v = __shfl_up(inc, o);
    if (lane >= o) inc += v;
  }
  if (lane == SCF_WAVE - 1) lds_w[wid] = inc;
  __syncthreads();
  int off = 0, tot = 0;
  for (int w = 0; w < PNP_WAVES; ++w) {
    const int v = lds_w[w];
    off += w < wid ? v : 0;
    tot += v;
  }
  __syncthreads();
  total = tot;
  return off + inc - c;
}

// out[k] = sum over the block of v[k], k < NV; a fixed reduction order (xor tree per wave, waves in order).
// Every thread must call it; the result is in `out` (LDS) after the call.
template <int NV>
__device__ __forceinline__ void block_sum(const double* v, double* lds_part, double* out) {
  const int lane = threadIdx.x & (SCF_WAVE - 1), wid = threadIdx.x / SCF_WAVE;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    double x = v[k];
    for (int o = SCF_WAVE / 2; o > 0; o >>= 1) x += __shfl_xor(x, o);
    if (lane == 0) lds_part[wid * NV + k] = x;
  }
  __syncthreads();
  for (int k = threadIdx.x; k < NV; k += blockDim.x) {
    double s = 0.0;
    for (int w = 0; w < PNP_WAVES; ++w) s += lds_part[w * NV + k];
    out[k] = s;
  }
  __syncthreads();
}

// counter-based hash (splitmix64 finaliser over a combined key)
__device__ __forceinline__ uint64_t pnp_mix(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ uint64_t pnp_hash(uint64_t seed, uint64_t a, uint64_t b) {
  return pnp_mix(pnp_mix(pnp_mix(seed) ^ a) ^ b);
}

// ---------------------------------------------------------------------------------------------- correspondences
__global__ __launch_bounds__(PNP_THREADS) void corr_2d3d_kernel(
    const float* __restrict__ flow, const float* __restrict__ depth, const float* __restrict__ occ, float occ_thresh,
    const float* __restrict__ K, const float* __restrict__ R0, const float* __restrict__ t0, int H, int W,
    float* __restrict__ pts2d, float* __restrict__ pts3d, float* __restrict__ conf, int* __restrict__ count) {
  __shared__ PoseMats s;
  __shared__ int wsum[PNP_WAVES];
  const int n = blockIdx.x;
  load_mats(&s, K, R0, t0, nullptr, nullptr, n);
  const int hw = H * W;
  const float* dp = depth + (long long)n * hw;
  const float* op = occ ? occ + (long long)n * hw : nullptr;
  const float* fx = flow + (long long)n * 2 * hw;
  const float* fy = fx + hw;
  float* o2 = pts2d + (long long)n * hw * 2;
  float* o3 = pts3d + (long long)n * hw * 3;
  float* oc = conf + (long long)n * hw;
  int run = 0;
  for (int base = 0; base < hw; base += PNP_THREADS * CORR_ITEMS) {
    const int p0 = base + threadIdx.x * CORR_ITEMS;
    unsigned keep = 0;
    int c = 0;
#pragma unroll
    for (int k = 0; k < CORR_ITEMS; ++k) {
      const int p = p0 + k;
      bool kp = false;
      if (p < hw) {
        kp = dp[p] > 0.f;
        if (op) kp = kp && op[p] > occ_thresh;     // NaN occlusion: not kept
      }
      keep |= (unsigned)kp << k;
      c += kp;
    }
    int total;
    int slot = run + block_scan(c, wsum, total);
    for (int k = 0; k < CORR_ITEMS; ++k) {
      if (!((keep >> k) & 1u)) continue;
      const int p = p0 + k;
      const int yi = p / W, xi = p - yi * W;
      const float x = (float)xi, y = (float)yi;
      float X, Y, Z;
      unproject(s, x, y, dp[p], X, Y, Z);
      o2[2 * slot] = x + fx[p];
      o2[2 * slot + 1] = y + fy[p];
      o3[3 * slot] = X;
      o3[3 * slot + 1] = Y;
      o3[3 * slot + 2] = Z;
      oc[slot] = op ? op[p] : 1.f;
      ++slot;
    }
    run += total;
  }
  if (threadIdx.x == 0) count[n] = run;
}

extern "C" int scf_flow_corr_2d3d(const float* flow, const float* depth, const float* occ, float occ_thresh,
                                  const float* K, const float* R0, const float* t0, int N, int H, int W,
                                  float* pts2d, float* pts3d, float* conf, int32_t* count, scf_stream_t stream) {
  if (!flow || !depth || !K || !R0 || !t0 || !pts2d || !pts3d || !conf || !count || N <= 0 || H <= 0 || W <= 0)
    return SCF_EINVAL;
  if ((int64_t)H * W > (1 << 30)) return SCF_EUNSUPPORTED;
  scf_launch(corr_2d3d_kernel, dim3(N), dim3(PNP_THREADS), 0, scf_stream(stream), flow, depth, occ, occ_thresh, K, R0,
             t0, H, W, pts2d, pts3d, conf, (int*)count);
  return scf_launch_status();
}

// ---------------------------------------------------------------------------------------------- sampling
// order-preserving map of a float to uint32 (larger float -> larger key; NaN above +inf, as torch.topk ranks it).
// -0.0 == +0.0 as floats, so both take +0.0's key: a tie between them goes to the lower index like any other.
__device__ __forceinline__ uint32_t pnp_fkey(float f) {
  const uint32_t u = __float_as_uint(f);
  if (f != f) return 0xFFFFFFFFu;
  if (f == 0.f) return 0x80000000u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ uint32_t pnp_key(int mode, const float* cf, uint64_t seed, int i) {
  return mode == SCF_PNP_SAMPLE_TOPK ? pnp_fkey(cf[i]) : (uint32_t)(pnp_hash(seed, 0x5e1ec7ull, (uint64_t)i) >> 32);
}

// per sample: sel[n, 0..m) = the kept point indices (ascending), m -> msel[n]
__global__ __launch_bounds__(PNP_THREADS) void pnp_select_kernel(const float* __restrict__ conf,
                                                                 const int* __restrict__ count, int cap, int mode,
                                                                 int num, uint64_t seed, int* __restrict__ sel,
                                                                 int* __restrict__ msel) {
  __shared__ int hist[256];
  __shared__ int wsum[PNP_WAVES];
  __shared__ uint32_t s_prefix;
  __shared__ int s_need;
  const int n = blockIdx.x;
  int cnt = count[n];
  cnt = cnt < 0 ? 0 : (cnt > cap ? cap : cnt);
  const float* cf = conf + (long long)n * cap;
  int* out = sel + (long long)n * cap;
  // the reference keeps every point when num > count; 'random' draws from randperm(count - 1): the last point never
  int elig = cnt, want = num;
  if (num > cnt) want = cnt;
  else if (mode == SCF_PNP_SAMPLE_RANDOM) { elig = cnt > 0 ? cnt - 1 : 0; want = num < elig ? num : elig; }
  if (want >= elig) {                           // everything eligible is kept: identity
    for (int i = threadIdx.x; i < elig; i += blockDim.x) out[i] = i;
    if (threadIdx.x == 0) msel[n] = elig;
    return;
  }
  // radix select of the want-th largest key, MSB first
  uint32_t prefix = 0, pmask = 0;
  int need = want;
  for (int shift = 24; shift >= 0; shift -= 8) {
    for (int b = threadIdx.x; b < 256; b += blockDim.x) hist[b] = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < elig; i += blockDim.x) {
      const uint32_t k = pnp_key(mode, cf, seed, i);
      if ((k & pmask) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int acc = 0, b = 255;
      for (; b > 0; --b) {
        if (acc + hist[b] >= need) break;
        acc += hist[b];
      }
      s_prefix = prefix | ((uint32_t)b << shift);
      s_need = need - acc;
    }
    __syncthreads();
    prefix = s_prefix;
    need = s_need;
    pmask |= 255u << shift;
    __syncthreads();
  }
  // keys > T all kept; the first `need` keys == T (ascending index) kept
  const uint32_t T = prefix;
  int run = 0, run_eq = 0;
  for (int base = 0; base < elig; base += PNP_THREADS * CORR_ITEMS) {
    const int i0 = base + threadIdx.x * CORR_ITEMS;
    unsigned gt = 0, eq = 0;
    int ceq = 0;
    for (int k = 0; k < CORR_ITEMS; ++k) {
      const int i = i0 + k;
      if (i >= elig) break;
      const uint32_t key = pnp_key(mode, cf, seed, i);
      gt |= (unsigned)(key > T) << k;
      eq |= (unsigned)(key == T) << k;
      ceq += key == T;
    }
    int tot_eq;
    int r_eq = run_eq + block_scan(ceq, wsum, tot_eq);
    unsigned take = gt;
    for (int k = 0; k < CORR_ITEMS; ++k)
      if ((eq >> k) & 1u) { take |= (unsigned)(r_eq < need) << k; ++r_eq; }
    int tot;
    int slot = run + block_scan(__popc(take), wsum, tot);
    for (int k = 0; k < CORR_ITEMS; ++k)
      if ((take >> k) & 1u) out[slot++] = i0 + k;
    run += tot;
    run_eq += tot_eq;
  }
  if (threadIdx.x == 0) msel[n] = run;
}

// ---------------------------------------------------------------------------------------------- EPnP (fp64)
// cyclic Jacobi eigen-decomposition of a symmetric n x n matrix A (row-major, overwritten: its diagonal ends up
// holding the eigenvalues); V receives the eigenvectors as columns
template <int n>
__device__ void jacobi_eig(double* A, double* V) {
  for (int i = 0; i < n * n; ++i) V[i] = (i / n == i % n) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 40; ++sweep) {
    double off = 0.0, dia = 0.0;
    for (int p = 0; p < n; ++p) {
      dia += A[p * n + p] * A[p * n + p];
      for (int q = p + 1; q < n; ++q) off += A[p * n + q] * A[p * n + q];
    }
    if (!(off > 1e-30 * dia)) break;          // also ends on NaN
    for (int p = 0; p < n - 1; ++p)
      for (int q = p + 1; q < n; ++q) {
        const double apq = A[p * n + q];
        if (apq == 0.0) continue;
        const double th = (A[q * n + q] - A[p * n + p]) / (2.0 * apq);
        const double t = (th >= 0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < n; ++k) {
          const double akp = A[k * n + p], akq = A[k * n + q];
          A[k * n + p] = c * akp - s * akq;
          A[k * n + q] = s * akp + c * akq;
        }
        for (int k = 0; k < n; ++k) {
          const double apk = A[p * n + k], aqk = A[q * n + k];
          A[p * n + k] = c * apk - s * aqk;
          A[q * n + k] = s * apk + c * aqk;
        }
        for (int k = 0; k < n; ++k) {
          const double vkp = V[k * n + p], vkq = V[k * n + q];
          V[k * n + p] = c * vkp - s * vkq;
          V[k * n + q] = s * vkp + c * vkq;
        }
      }
  }
}

// least squares A x = b (A rows x cols, row-major) by the normal equations and Gaussian elimination with
// partial pivoting; false when singular
template <int rows, int cols>
__device__ bool lsq(const double* A, const double* b, double* x) {
  double M[cols][cols + 1];
  for (int i = 0; i < cols; ++i) {
    for (int j = 0; j < cols; ++j) {
      double s = 0.0;
      for (int r = 0; r < rows; ++r) s += A[r * cols + i] * A[r * cols + j];
      M[i][j] = s;
    }
    double s = 0.0;
    for (int r = 0; r < rows; ++r) s += A[r * cols + i] * b[r];
    M[i][cols] = s;
  }
  double scale = 0.0;
  for (int i = 0; i < cols; ++i) scale = fmax(scale, fabs(M[i][i]));
  for (int c = 0; c < cols; ++c) {
    int piv = c;
    for (int r = c + 1; r < cols; ++r)
      if (fabs(M[r][c]) > fabs(M[piv][c])) piv = r;
    if (!(fabs(M[piv][c]) > 1e-300 + 1e-14 * scale)) return false;
    if (piv != c)
      for (int j = 0; j <= cols; ++j) { const double tmp = M[c][j]; M[c][j] = M[piv][j]; M[piv][j] = tmp; }
    for (int r = c + 1; r < cols; ++r) {
      const double f = M[r][c] / M[c][c];
      for (int j = c; j <= cols; ++j) M[r][j] -= f * M[c][j];
    }
  }
  for (int c = cols - 1; c >= 0; --c) {
    double s = M[c][cols];
    for (int j = c + 1; j < cols; ++j) s -= M[c][j] * x[j];
    x[c] = s / M[c][c];
  }
  return true;
}

// control points of EPnP (Lepetit et al.): the centroid and the centroid + sqrt(eigenvalue) * axis for the three
// principal axes of the points.  alpha'_k(p) = axis_k . (p - c0) / sqrt(eigenvalue_k), alpha_0 = 1 - sum alpha'.
// Each axis is oriented so that its largest-magnitude component (the first of equal ones) is positive: the
// least-squares null space over noisy points depends on that sign, and Jacobi's own sign is an accident of its
// rotation order.
struct EpnpCtl {
  double c0[3], ax[3][3], inv_s[3], cw[4][3];
};

// moments: m[0..3) = sum p, m[3..9) = sum p p^T (xx xy xz yy yz zz), m[9] = point count.  False when the points are
// (numerically) collinear or planar: the smallest principal spread must exceed 1e-8 of the largest (variances).
__device__ bool epnp_control(const double* m, EpnpCtl& c) {
  const double n = m[9];
  if (!(n >= 4.0)) return false;
  for (int i = 0; i < 3; ++i) c.c0[i] = m[i] / n;
  double C[9], V[9];
  C[0] = m[3] / n - c.c0[0] * c.c0[0];
  C[1] = C[3] = m[4] / n - c.c0[0] * c.c0[1];
  C[2] = C[6] = m[5] / n - c.c0[0] * c.c0[2];
  C[4] = m[6] / n - c.c0[1] * c.c0[1];
  C[5] = C[7] = m[7] / n - c.c0[1] * c.c0[2];
  C[8] = m[8] / n - c.c0[2] * c.c0[2];
  jacobi_eig<3>(C, V);
  const double w0 = C[0], w1 = C[4], w2 = C[8];
  const double wmax = fmax(w0, fmax(w1, w2)), wmin = fmin(w0, fmin(w1, w2));
  if (!(wmax > 0.0) || !(wmin > 1e-8 * wmax)) return false;
  const double w[3] = {w0, w1, w2};
  for (int k = 0; k < 3; ++k) {
    const double sq = sqrt(w[k]);
    int big = 0;
    for (int i = 1; i < 3; ++i)
      if (fabs(V[i * 3 + k]) > fabs(V[big * 3 + k])) big = i;
    const double sgn = V[big * 3 + k] < 0 ? -1.0 : 1.0;
    c.inv_s[k] = 1.0 / sq;
    for (int i = 0; i < 3; ++i) {
      c.ax[k][i] = sgn * V[i * 3 + k];
      c.cw[k + 1][i] = c.c0[i] + sq * c.ax[k][i];
    }
  }
  for (int i = 0; i < 3; ++i) c.cw[0][i] = c.c0[i];
  return true;
}

__device__ __forceinline__ void epnp_alpha(const EpnpCtl& c, double X, double Y, double Z, double* a) {
  const double dx = X - c.c0[0], dy = Y - c.c0[1], dz = Z - c.c0[2];
  double s = 0.0;
  for (int k = 0; k < 3; ++k) {
    a[k + 1] = (c.ax[k][0] * dx + c.ax[k][1] * dy + c.ax[k][2] * dz) * c.inv_s[k];
    s += a[k + 1];
  }
  a[0] = 1.0 - s;
}

#define EPNP_NACC (78 + 14)      // upper triangle of M^T M (12 x 12), sum alpha (4), sum alpha alpha^T (10)

// adds one correspondence: pixel (u, v) -> normalised camera coordinates through Kinv, object point (X, Y, Z)
__device__ __forceinline__ void epnp_accum(const EpnpCtl& c, const double* Kinv, double u, double v, double X,
                                           double Y, double Z, double* acc) {
  const double hx = Kinv[0] * u + Kinv[1] * v + Kinv[2];
  const double hy = Kinv[3] * u + Kinv[4] * v + Kinv[5];
  const double hz = Kinv[6] * u + Kinv[7] * v + Kinv[8];
  const double xn = hx / hz, yn = hy / hz;
  double a[4];
  epnp_alpha(c, X, Y, Z, a);
  double r1[12], r2[12];
  for (int j = 0; j < 4; ++j) {
    r1[3 * j] = a[j]; r1[3 * j + 1] = 0.0; r1[3 * j + 2] = -a[j] * xn;
    r2[3 * j] = 0.0; r2[3 * j + 1] = a[j]; r2[3 * j + 2] = -a[j] * yn;
  }
  int e = 0;
  for (int i = 0; i < 12; ++i)
    for (int j = i; j < 12; ++j) acc[e++] += r1[i] * r1[j] + r2[i] * r2[j];
  for (int j = 0; j < 4; ++j) acc[78 + j] += a[j];
  e = 82;
  for (int i = 0; i < 4; ++i)
    for (int j = i; j < 4; ++j) acc[e++] += a[i] * a[j];
}

// rotation mapping the object-frame control points onto the camera-frame ones (Horn's quaternion method on the
// alpha moments: both point sets are linear in alpha), t = centroid difference
__device__ bool epnp_pose(const EpnpCtl& c, const double (*ccs)[3], const double* acc, double n, double* R,
                          double* t) {
  double am[4], S[16];
  for (int j = 0; j < 4; ++j) am[j] = acc[78 + j] / n;
  int e = 82;
  for (int i = 0; i < 4; ++i)
    for (int j = i; j < 4; ++j) {
      S[i * 4 + j] = S[j * 4 + i] = acc[e++] / n - am[i] * am[j];
    }
  double pc0[3], pw0[3];
  for (int d = 0; d < 3; ++d) {
    pc0[d] = pw0[d] = 0.0;
    for (int j = 0; j < 4; ++j) { pc0[d] += ccs[j][d] * am[j]; pw0[d] += c.cw[j][d] * am[j]; }
  }
  // H[a][b] = sum (pw - pw0)_a (pc - pc0)_b / n = Cw S Ccs^T
  double Hm[9];
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      double s = 0.0;
      for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) s += c.cw[i][a] * S[i * 4 + j] * ccs[j][b];
      Hm[a * 3 + b] = s;
    }
  const double Sxx = Hm[0], Sxy = Hm[1], Sxz = Hm[2], Syx = Hm[3], Syy = Hm[4], Syz = Hm[5], Szx = Hm[6],
               Szy = Hm[7], Szz = Hm[8];
  double Nm[16] = {Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx,
                   Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz,
                   Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy,
                   Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz};
  double V[16];
  jacobi_eig<4>(Nm, V);
  int best = 0;
  for (int k = 1; k < 4; ++k)
    if (Nm[k * 5] > Nm[best * 5]) best = k;
  double w = V[0 * 4 + best], x = V[1 * 4 + best], y = V[2 * 4 + best], z = V[3 * 4 + best];
  const double qn = sqrt(w * w + x * x + y * y + z * z);
  if (!(qn > 0.0)) return false;
  w /= qn; x /= qn; y /= qn; z /= qn;
  R[0] = w * w + x * x - y * y - z * z; R[1] = 2 * (x * y - w * z); R[2] = 2 * (x * z + w * y);
  R[3] = 2 * (x * y + w * z); R[4] = w * w - x * x + y * y - z * z; R[5] = 2 * (y * z - w * x);
  R[6] = 2 * (x * z - w * y); R[7] = 2 * (y * z + w * x); R[8] = w * w - x * x - y * y + z * z;
  for (int d = 0; d < 3; ++d) t[d] = pc0[d] - (R[d * 3] * pw0[0] + R[d * 3 + 1] * pw0[1] + R[d * 3 + 2] * pw0[2]);
  for (int i = 0; i < 9; ++i) if (!isfinite(R[i])) return false;
  for (int i = 0; i < 3; ++i) if (!isfinite(t[i])) return false;
  return true;
}

// the three beta cases of EPnP (approximations over 4, 2 and 3 null vectors, each refined by 5 Gauss-Newton steps
// on all six control-point distances) -> up to three candidate poses; valid[k] tells which were found
__device__ __noinline__ void epnp_solve(const double* acc, double n, const EpnpCtl& c, double (*Rc)[9],
                                        double (*tc)[3], bool* valid) {
  double A[144], V[144];
  int e = 0;
  for (int i = 0; i < 12; ++i)
    for (int j = i; j < 12; ++j) { A[i * 12 + j] = A[j * 12 + i] = acc[e++]; }
  jacobi_eig<12>(A, V);
  // indices of the 4 smallest eigenvalues, ascending (ties: lower index)
  int ord[4];
  bool used[12] = {};
  for (int k = 0; k < 4; ++k) {
    int b = -1;
    for (int i = 0; i < 12; ++i)
      if (!used[i] && (b < 0 || A[i * 13] < A[b * 13])) b = i;
    used[b] = true;
    ord[k] = b;
  }
  double v[4][12];
  for (int k = 0; k < 4; ++k)
    for (int i = 0; i < 12; ++i) v[k][i] = V[i * 12 + ord[k]];
  // L (6 x 10) and rho (6): squared control-point distances
  const int pa[6] = {0, 0, 0, 1, 1, 2}, pb[6] = {1, 2, 3, 2, 3, 3};
  double L[60], rho[6];
  for (int r = 0; r < 6; ++r) {
    double dv[4][3];
    for (int k = 0; k < 4; ++k)
      for (int d = 0; d < 3; ++d) dv[k][d] = v[k][3 * pa[r] + d] - v[k][3 * pb[r] + d];
    auto dot = [&](int a, int b) { return dv[a][0] * dv[b][0] + dv[a][1] * dv[b][1] + dv[a][2] * dv[b][2]; };
    double* l = L + 10 * r;
    l[0] = dot(0, 0); l[1] = 2 * dot(0, 1); l[2] = dot(1, 1); l[3] = 2 * dot(0, 2); l[4] = 2 * dot(1, 2);
    l[5] = dot(2, 2); l[6] = 2 * dot(0, 3); l[7] = 2 * dot(1, 3); l[8] = 2 * dot(2, 3); l[9] = dot(3, 3);
    double s = 0.0;
    for (int d = 0; d < 3; ++d) { const double q = c.cw[pa[r]][d] - c.cw[pb[r]][d]; s += q * q; }
    rho[r] = s;
  }
  for (int cs = 0; cs < 3; ++cs) {
    valid[cs] = false;
    double beta[4] = {0, 0, 0, 0};
    if (cs == 0) {                    // B11 B12 B13 B14
      const int col[4] = {0, 1, 3, 6};
      double Ls[24], B[4];
      for (int r = 0; r < 6; ++r) for (int j = 0; j < 4; ++j) Ls[r * 4 + j] = L[r * 10 + col[j]];
      if (!lsq<6, 4>(Ls, rho, B)) continue;
      if (B[0] < 0) { beta[0] = sqrt(-B[0]); for (int j = 1; j < 4; ++j) beta[j] = -B[j] / beta[0]; }
      else { beta[0] = sqrt(B[0]); for (int j = 1; j < 4; ++j) beta[j] = beta[0] > 0 ? B[j] / beta[0] : 0.0; }
    } else {                          // cs 1: B11 B12 B22; cs 2: B11 B12 B22 B13 B23
      double Ls[30], B[5];
      const int nc = cs == 1 ? 3 : 5;
      for (int r = 0; r < 6; ++r) for (int j = 0; j < nc; ++j) Ls[r * nc + j] = L[r * 10 + j];
      if (cs == 1 ? !lsq<6, 3>(Ls, rho, B) : !lsq<6, 5>(Ls, rho, B)) continue;
      if (B[0] < 0) { beta[0] = sqrt(-B[0]); beta[1] = B[2] < 0 ? sqrt(-B[2]) : 0.0; }
      else { beta[0] = sqrt(B[0]); beta[1] = B[2] > 0 ? sqrt(B[2]) : 0.0; }
      if (B[1] < 0) beta[0] = -beta[0];
      if (cs == 2) beta[2] = beta[0] != 0.0 ? B[3] / beta[0] : 0.0;
    }
    for (int it = 0; it < 5; ++it) {  // Gauss-Newton on the 6 distance constraints
      double J[24], res[6], dx[4];
      const double b0 = beta[0], b1 = beta[1], b2 = beta[2], b3 = beta[3];
      const double bb[10] = {b0 * b0, b0 * b1, b1 * b1, b0 * b2, b1 * b2, b2 * b2, b0 * b3, b1 * b3, b2 * b3, b3 * b3};
      for (int r = 0; r < 6; ++r) {
        const double* l = L + 10 * r;
        J[r * 4 + 0] = 2 * l[0] * b0 + l[1] * b1 + l[3] * b2 + l[6] * b3;
        J[r * 4 + 1] = l[1] * b0 + 2 * l[2] * b1 + l[4] * b2 + l[7] * b3;
        J[r * 4 + 2] = l[3] * b0 + l[4] * b1 + 2 * l[5] * b2 + l[8] * b3;
        J[r * 4 + 3] = l[6] * b0 + l[7] * b1 + l[8] * b2 + 2 * l[9] * b3;
        double s = 0.0;
        for (int j = 0; j < 10; ++j) s += l[j] * bb[j];
        res[r] = rho[r] - s;
      }
      if (!lsq<6, 4>(J, res, dx)) break;
      for (int j = 0; j < 4; ++j) beta[j] += dx[j];
    }
    double ccs[4][3];
    for (int j = 0; j < 4; ++j)
      for (int d = 0; d < 3; ++d) {
        double s = 0.0;
        for (int k = 0; k < 4; ++k) s += beta[k] * v[k][3 * j + d];
        ccs[j][d] = s;
      }
    // the object lies in front of the camera: the depth of the points' centroid decides the sign
    double zc = 0.0;
    for (int j = 0; j < 4; ++j) zc += ccs[j][2] * acc[78 + j];
    if (zc < 0)
      for (int j = 0; j < 4; ++j) for (int d = 0; d < 3; ++d) ccs[j][d] = -ccs[j][d];
    valid[cs] = epnp_pose(c, ccs, acc, n, Rc[cs], tc[cs]);
  }
}

// pixel reprojection distance of one point under (R, t), fp64 (case selection)
__device__ __forceinline__ double reproj_d(const double* K, const double* R, const double* t, double u, double v,
                                           double X, double Y, double Z) {
  const double px = R[0] * X + R[1] * Y + R[2] * Z + t[0];
  const double py = R[3] * X + R[4] * Y + R[5] * Z + t[1];
  const double pz = R[6] * X + R[7] * Y + R[8] * Z + t[2];
  const double qx = K[0] * px + K[1] * py + K[2] * pz, qy = K[3] * px + K[4] * py + K[5] * pz,
               qz = K[6] * px + K[7] * py + K[8] * pz;
  const double du = qx / qz - u, dv = qy / qz - v;
  return sqrt(du * du + dv * dv);
}

// P = K [R | t] in fp32 (row-major 3 x 4) for scoring
__device__ __forceinline__ void proj_matrix(const double* K, const double* R, const double* t, float* P) {
  for (int r = 0; r < 3; ++r) {
    for (int cc = 0; cc < 3; ++cc)
      P[r * 4 + cc] = (float)(K[r * 3] * R[cc] + K[r * 3 + 1] * R[3 + cc] + K[r * 3 + 2] * R[6 + cc]);
    P[r * 4 + 3] = (float)(K[r * 3] * t[0] + K[r * 3 + 1] * t[1] + K[r * 3 + 2] * t[2]);
  }
}

// a point is an inlier when it projects in front of the camera within `thr` pixels; NaN anywhere: an outlier
__device__ __forceinline__ bool pnp_inlier(const float* P, float u, float v, float X, float Y, float Z, float thr2) {
  const float qx = P[0] * X + P[1] * Y + P[2] * Z + P[3];
  const float qy = P[4] * X + P[5] * Y + P[6] * Z + P[7];
  const float qz = P[8] * X + P[9] * Y + P[10] * Z + P[11];
  if (!(qz > 0.f)) return false;
  const float du = qx / qz - u, dv = qy / qz - v;
  return du * du + dv * dv < thr2;
}

// ---------------------------------------------------------------------------------------------- RANSAC
struct PnpBlock {
  float hP[PNP_THREADS][12];
  int hcnt[PNP_THREADS];
  int hval[PNP_THREADS];
  float bestP[12];
  int best_cnt;
  int flag;
  EpnpCtl ctl;
  double part[PNP_WAVES * EPNP_NACC];
  double sum[EPNP_NACC];
  double Rc[3][9], tc[3][3];
  bool cval[3];
  double R[9], t[3];
};

__global__ __launch_bounds__(PNP_THREADS) void pnp_ransac_kernel(
    const float* __restrict__ pts2d, const float* __restrict__ pts3d, const int* __restrict__ count,
    const int* __restrict__ sel, const int* __restrict__ msel, int cap, const float* __restrict__ Kmat,
    const float* __restrict__ R_ref, const float* __restrict__ t_ref, int iters, float thr, uint64_t seed,
    float* __restrict__ R_out, float* __restrict__ t_out, int* __restrict__ ok_out, int* __restrict__ inl_out) {
  __shared__ PnpBlock sb;
  const int n = blockIdx.x, tid = threadIdx.x;
  const float thr2 = thr * thr;
  int cnt = count[n];
  cnt = cnt < 0 ? 0 : (cnt > cap ? cap : cnt);
  int m = sel ? msel[n] : cnt;
  m = m < 0 ? 0 : (m > cnt ? cnt : m);
  const float* p2 = pts2d + (long long)n * cap * 2;
  const float* p3 = pts3d + (long long)n * cap * 3;
  const int* sl = sel ? sel + (long long)n * cap : nullptr;
  auto load = [&](int i, float& u, float& v, float& X, float& Y, float& Z) {
    int j = sl ? sl[i] : i;
    j = j < 0 ? 0 : (j >= cnt ? cnt - 1 : j);
    u = p2[2 * j]; v = p2[2 * j + 1];
    X = p3[3 * j]; Y = p3[3 * j + 1]; Z = p3[3 * j + 2];
  };
  double K[9], Kinv[9];
  {
    for (int i = 0; i < 9; ++i) K[i] = Kmat[9 * n + i];
    const double a = K[0], b = K[1], c = K[2], d = K[3], e = K[4], f = K[5], g = K[6], h = K[7], i = K[8];
    const double A = e * i - f * h, B = -(d * i - f * g), C = d * h - e * g;
    const double id = 1.0 / (a * A + b * B + c * C);
    Kinv[0] = A * id; Kinv[1] = -(b * i - c * h) * id; Kinv[2] = (b * f - c * e) * id;
    Kinv[3] = B * id; Kinv[4] = (a * i - c * g) * id; Kinv[5] = -(a * f - c * d) * id;
    Kinv[6] = C * id; Kinv[7] = -(a * h - b * g) * id; Kinv[8] = (a * e - b * d) * id;
  }
  auto fail = [&]() {
    if (tid < 9) R_out[9 * n + tid] = R_ref[9 * n + tid];
    if (tid < 3) t_out[3 * n + tid] = t_ref[3 * n + tid];
    if (tid == 0) { ok_out[n] = 0; inl_out[n] = 0; }
  };
  if (cnt < 4 || m < 5) { fail(); return; }

  if (tid == 0) sb.best_cnt = -1;
  for (int h0 = 0; h0 < iters; h0 += PNP_THREADS) {
    // ---- one minimal solve per thread
    const int h = h0 + tid;
    bool valid = false;
    float P[12];
    if (h < iters) {
      int idx[5];
      int got = 0;
      for (int a = 0; a < 64 && got < 5; ++a) {
        const int j = (int)(pnp_hash(seed, (uint64_t)h, (uint64_t)(a + 1)) % (uint64_t)m);
        bool dup = false;
        for (int q = 0; q < got; ++q) dup |= idx[q] == j;
        if (!dup) idx[got++] = j;
      }
      if (got == 5) {
        float pu[5], pv[5], pX[5], pY[5], pZ[5];
        double mom[10] = {};
        bool fin = true;
        for (int q = 0; q < 5; ++q) {
          load(idx[q], pu[q], pv[q], pX[q], pY[q], pZ[q]);
          fin &= isfinite(pu[q]) && isfinite(pv[q]) && isfinite(pX[q]) && isfinite(pY[q]) && isfinite(pZ[q]);
          const double X = pX[q], Y = pY[q], Z = pZ[q];
          mom[0] += X; mom[1] += Y; mom[2] += Z;
          mom[3] += X * X; mom[4] += X * Y; mom[5] += X * Z; mom[6] += Y * Y; mom[7] += Y * Z; mom[8] += Z * Z;
        }
        mom[9] = 5.0;
        EpnpCtl c;
        if (fin && epnp_control(mom, c)) {
          double acc[EPNP_NACC] = {};
          for (int q = 0; q < 5; ++q) epnp_accum(c, Kinv, pu[q], pv[q], pX[q], pY[q], pZ[q], acc);
          double Rc[3][9], tc[3][3];
          bool cv[3];
          epnp_solve(acc, 5.0, c, Rc, tc, cv);
          double best_e = 0.0;
          int bc = -1;
          for (int k = 0; k < 3; ++k) {
            if (!cv[k]) continue;
            double e = 0.0;
            for (int q = 0; q < 5; ++q) e += reproj_d(K, Rc[k], tc[k], pu[q], pv[q], pX[q], pY[q], pZ[q]);
            if (isfinite(e) && (bc < 0 || e < best_e)) { bc = k; best_e = e; }
          }
          if (bc >= 0) {
            proj_matrix(K, Rc[bc], tc[bc], P);
            valid = true;
            for (int i = 0; i < 12; ++i) valid &= isfinite(P[i]);
          }
        }
      }
    }
    for (int i = 0; i < 12; ++i) sb.hP[tid][i] = valid ? P[i] : 0.f;
    sb.hval[tid] = valid;
    sb.hcnt[tid] = 0;
    __syncthreads();
    // ---- scoring: a point per thread against every hypothesis of the round
    const int nh = iters - h0 < PNP_THREADS ? iters - h0 : PNP_THREADS;
    for (int i0 = 0; i0 < m; i0 += PNP_THREADS) {
      const int i = i0 + tid;
      float u = 0.f, v = 0.f, X = 0.f, Y = 0.f, Z = 0.f;
      const bool live = i < m;
      if (live) load(i, u, v, X, Y, Z);
      for (int hh = 0; hh < nh; ++hh) {
        if (!sb.hval[hh]) continue;                  // uniform across the block
        const bool in = live && pnp_inlier(sb.hP[hh], u, v, X, Y, Z, thr2);
        const unsigned long long b = __ballot(in);
        if ((tid & (SCF_WAVE - 1)) == 0 && b) atomicAdd(&sb.hcnt[hh], (int)__popcll(b));
      }
    }
    __syncthreads();
    if (tid == 0)
      for (int hh = 0; hh < nh; ++hh)
        if (sb.hval[hh] && sb.hcnt[hh] > sb.best_cnt) {
          sb.best_cnt = sb.hcnt[hh];
          for (int k = 0; k < 12; ++k) sb.bestP[k] = sb.hP[hh][k];
        }
    __syncthreads();
  }
  if (sb.best_cnt < 5) { fail(); return; }

  // ---- final EPnP over every inlier of the best hypothesis
  float bP[12];
  for (int k = 0; k < 12; ++k) bP[k] = sb.bestP[k];
  {
    double mom[10] = {};
    for (int i = tid; i < m; i += PNP_THREADS) {
      float u, v, X, Y, Z;
      load(i, u, v, X, Y, Z);
      if (!pnp_inlier(bP, u, v, X, Y, Z, thr2)) continue;
      const double x = X, y = Y, z = Z;
      mom[0] += x; mom[1] += y; mom[2] += z;
      mom[3] += x * x; mom[4] += x * y; mom[5] += x * z; mom[6] += y * y; mom[7] += y * z; mom[8] += z * z;
      mom[9] += 1.0;
    }
    block_sum<10>(mom, sb.part, sb.sum);
    if (tid == 0) sb.flag = epnp_control(sb.sum, sb.ctl);
    __syncthreads();
  }
  if (!sb.flag) { fail(); return; }
  const double ninl = sb.sum[9];
  {
    double acc[EPNP_NACC] = {};
    for (int i = tid; i < m; i += PNP_THREADS) {
      float u, v, X, Y, Z;
      load(i, u, v, X, Y, Z);
      if (pnp_inlier(bP, u, v, X, Y, Z, thr2)) epnp_accum(sb.ctl, Kinv, u, v, X, Y, Z, acc);
    }
    block_sum<EPNP_NACC>(acc, sb.part, sb.sum);
    if (tid == 0) epnp_solve(sb.sum, ninl, sb.ctl, sb.Rc, sb.tc, sb.cval);
    __syncthreads();
  }
  {
    double err[3] = {0.0, 0.0, 0.0};
    bool cv[3] = {sb.cval[0], sb.cval[1], sb.cval[2]};
    for (int i = tid; i < m; i += PNP_THREADS) {
      float u, v, X, Y, Z;
      load(i, u, v, X, Y, Z);
      if (!pnp_inlier(bP, u, v, X, Y, Z, thr2)) continue;
      for (int k = 0; k < 3; ++k)
        if (cv[k]) err[k] += reproj_d(K, sb.Rc[k], sb.tc[k], u, v, X, Y, Z);
    }
    block_sum<3>(err, sb.part, sb.sum);
    if (tid == 0) {
      int bc = -1;
      for (int k = 0; k < 3; ++k)
        if (cv[k] && isfinite(sb.sum[k]) && (bc < 0 || sb.sum[k] < sb.sum[bc])) bc = k;
      sb.flag = bc >= 0;
      if (bc >= 0) {
        for (int i = 0; i < 9; ++i) sb.R[i] = sb.Rc[bc][i];
        for (int i = 0; i < 3; ++i) sb.t[i] = sb.tc[bc][i];
        proj_matrix(K, sb.R, sb.t, sb.bestP);
        for (int i = 0; i < 9; ++i) sb.flag &= isfinite((float)sb.R[i]);
        for (int i = 0; i < 3; ++i) sb.flag &= isfinite((float)sb.t[i]);
        for (int i = 0; i < 12; ++i) sb.flag &= isfinite(sb.bestP[i]);
      }
      sb.hcnt[0] = 0;
    }
    __syncthreads();
  }
  if (!sb.flag) { fail(); return; }
  // ---- re-score the final pose over all points
  for (int k = 0; k < 12; ++k) bP[k] = sb.bestP[k];
  for (int i0 = 0; i0 < m; i0 += PNP_THREADS) {
    const int i = i0 + tid;
    float u = 0.f, v = 0.f, X = 0.f, Y = 0.f, Z = 0.f;
    const bool live = i < m;
    if (live) load(i, u, v, X, Y, Z);
    const bool in = live && pnp_inlier(bP, u, v, X, Y, Z, thr2);
    const unsigned long long b = __ballot(in);
    if ((tid & (SCF_WAVE - 1)) == 0 && b) atomicAdd(&sb.hcnt[0], (int)__popcll(b));
  }
  __syncthreads();
  if (tid < 9) R_out[9 * n + tid] = (float)sb.R[tid];
  if (tid < 3) t_out[3 * n + tid] = (float)sb.t[tid];
  if (tid == 0) { ok_out[n] = 1; inl_out[n] = sb.hcnt[0]; }
}

static int pnp_check(const scf_pnp_params* p) {
  if (!p || p->iterations <= 0 || !(p->reproj_error >= 0.f) || !(p->reproj_error <= 3.0e38f)) return SCF_EINVAL;
  if (p->sample_mode != SCF_PNP_SAMPLE_ALL && p->sample_mode != SCF_PNP_SAMPLE_TOPK &&
      p->sample_mode != SCF_PNP_SAMPLE_RANDOM)
    return SCF_EINVAL;
  if (p->sample_mode != SCF_PNP_SAMPLE_ALL && p->sample_num <= 0) return SCF_EINVAL;
  return SCF_OK;
}

extern "C" int64_t scf_pnp_workspace_bytes(int N, int capacity, const scf_pnp_params* p) {
  if (N <= 0 || capacity <= 0 || pnp_check(p) != SCF_OK) return SCF_EINVAL;
  if (p->sample_mode == SCF_PNP_SAMPLE_ALL) return 0;
  const int64_t b = ((int64_t)N * capacity + N) * (int64_t)sizeof(int32_t);
  return (b + 255) / 256 * 256;
}

extern "C" int scf_pnp_ransac(const float* pts2d, const float* pts3d, const float* conf, const int32_t* count, int N,
                              int capacity, const float* K, const float* R_ref, const float* t_ref,
                              const scf_pnp_params* p, float* R, float* t, int32_t* ok, int32_t* inliers,
                              void* workspace, scf_stream_t stream) {
  if (!pts2d || !pts3d || !count || !K || !R_ref || !t_ref || !R || !t || !ok || !inliers || N <= 0 || capacity <= 0)
    return SCF_EINVAL;
  const int e = pnp_check(p);
  if (e != SCF_OK) return e;
  int* sel = nullptr;
  int* msel = nullptr;
  if (p->sample_mode != SCF_PNP_SAMPLE_ALL) {
    if (!workspace || (p->sample_mode == SCF_PNP_SAMPLE_TOPK && !conf)) return SCF_EINVAL;
    sel = (int*)workspace;
    msel = sel + (int64_t)N * capacity;
    scf_launch(pnp_select_kernel, dim3(N), dim3(PNP_THREADS), 0, scf_stream(stream), conf, (const int*)count,
               capacity, (int)p->sample_mode, (int)p->sample_num, (uint64_t)p->seed, sel, msel);
    const int st = scf_launch_status();
    if (st != SCF_OK) return st;
  }
  scf_launch(pnp_ransac_kernel, dim3(N), dim3(PNP_THREADS), 0, scf_stream(stream), pts2d, pts3d, (const int*)count,
             (const int*)sel, (const int*)msel, capacity, K, R_ref, t_ref, (int)p->iterations, p->reproj_error,
             (uint64_t)p->seed, R, t, (int*)ok, (int*)inliers);
  return scf_launch_status();
}
