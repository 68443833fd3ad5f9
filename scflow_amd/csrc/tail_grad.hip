// Backward of the parameter-free tail of an SCFlow iteration (scflow_decoder.py:222-249), for gfx950: the adjoint of
// the align_corners bilinear resize, the re-projection sums and the reverse scan over the pose updates.  All three take
// the T iterations of a refinement pass as arrays of device pointers and are launched once per pass, not per iteration.
// No atomics anywhere: every sum has one order, fixed by the geometry alone, so the bits do not depend on the grid, on
// the number of iterations that share a launch, or on the run.
#include "scf_common.h"
#include "scf_pose.h"

#define TG_MAX_T SCF_TAIL_MAX_T
#define TG_THREADS 256
#define TG_WAVES (TG_THREADS / 64)

// ================================================================================================ resize adjoint
// Forward (resample.hip): out[oy, ox] = mul * (hy * (hx * v[y0, x0] + lx * v[y0, x1]) + ly * (hx * v[y1, x0] + lx * v[y1, x1]))
// with f = fl(fl(scale) * index), i0 = (int)f, l = f - i0, h = 1 - l, i1 = i0 + 1 clamped to the last node.
// Adjoint, per input node (iy, ix), in THIS order (both kernels below, and tests/test_tail_grad_host.py's replay):
//   part(oy, q) = sum over the columns ox of quad q = ox / 4, ascending, of  [x0 == ix] hx g  then  [x1 == ix] lx g
//   r(oy)       = sum over the quads that hold a column with x0 in {ix - 1, ix}, ascending, of part(oy, q)
//   acc         = sum over the rows with y0 in {iy - 1, iy}, ascending, of  [y0 == iy] hy r(oy)  then  [y1 == iy] ly r(oy)
//   out         = mul * acc  (+ the destination's previous value when accumulating)
// every accumulator starts at +0 and every product and sum is rounded to fp32 (no contraction).  A clamped +1 tap
// (x1 == x0 at the last column, y1 == y0 at the last row) puts both of its weights on that node, hx g first.  An
// accumulator that starts at +0 is never -0, so adding further +0 terms (quad slots no column wrote) changes no bit:
// the two kernels may differ in which empty slots they add, not in anything else.
struct ResizeGradJobs {             // job 0 and the optional job 1 (planes[1] = 0: none) of one geometry
  const float* src[2][TG_MAX_T];   // per iteration: (planes, Hout, Wout) gradient at the resize's OUTPUT
  const float* srcb[TG_MAX_T];     // job 0 only: optional second addend of the same shape (NULL entries: none)
  float* dst[2][TG_MAX_T];         // per iteration: (planes, Hin, Win) gradient at the resize's INPUT
  int planes[2];
  float mul[2];
  int accumulate[2];
};

__device__ __forceinline__ void tg_coord(float s, int o, int nin, int& i0, int& i1, float& l) {
#pragma clang fp contract(off)
  const float f = s * (float)o;
  i0 = (int)f;
  if (i0 > nin - 1) i0 = nin - 1;
  i1 = i0 + (i0 < nin - 1 ? 1 : 0);
  l = f - (float)i0;
}

// first output index in [0, nout] whose i0 is >= key (i0 is monotone in the index: fl(s * o) is)
__device__ __forceinline__ int tg_lower(float s, int nin, int nout, int key) {
  int lo = 0, hi = nout;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    int i0, i1;
    float l;
    tg_coord(s, mid, nin, i0, i1, l);
    if (i0 >= key) hi = mid; else lo = mid + 1;
  }
  return lo;
}

struct TgPlane { const float* src; const float* srcb; float* dst; float mul; int accumulate; };
__device__ __forceinline__ TgPlane tg_plane(const ResizeGradJobs& j, int p, long long in_px, long long out_px) {
  const int P = j.planes[0] + j.planes[1];
  const int t = p / P, r = p - t * P;
  const int job = r >= j.planes[0] ? 1 : 0;      // uniform over the block
  const int pl = job ? r - j.planes[0] : r;
  TgPlane o;
  const float* b = job ? nullptr : j.srcb[t];
  o.src = j.src[job][t] + pl * out_px;
  o.srcb = b ? b + pl * out_px : nullptr;
  o.dst = j.dst[job][t] + pl * in_px;
  o.mul = j.mul[job];
  o.accumulate = j.accumulate[job];
  return o;
}

// Any geometry, any alignment: one thread per input node, which finds the rows and columns that reach it once and then
// walks the planes (grid y).
__global__ __launch_bounds__(TG_THREADS) void resize_grad_gather_kernel(ResizeGradJobs jobs, int T, int Hin, int Win,
                                                                        int Hout, int Wout, float sh, float sw) {
#pragma clang fp contract(off)
  const int node = blockIdx.x * TG_THREADS + threadIdx.x;
  if (node >= Hin * Win) return;
  const int iy = node / Win, ix = node - iy * Win;
  const int ys = tg_lower(sh, Hin, Hout, iy - 1), ye = tg_lower(sh, Hin, Hout, iy + 1);
  const int xs = tg_lower(sw, Win, Wout, ix - 1), xe = tg_lower(sw, Win, Wout, ix + 1);
  const int total = T * (jobs.planes[0] + jobs.planes[1]);
  const long long in_px = (long long)Hin * Win, out_px = (long long)Hout * Wout;
  for (int p = blockIdx.y; p < total; p += gridDim.y) {
    const TgPlane pl = tg_plane(jobs, p, in_px, out_px);
    float acc = 0.f;
    for (int oy = ys; oy < ye; ++oy) {
      int y0, y1;
      float ly;
      tg_coord(sh, oy, Hin, y0, y1, ly);
      const float hy = 1.f - ly;
      const float* row = pl.src + (long long)oy * Wout;
      const float* rowb = pl.srcb ? pl.srcb + (long long)oy * Wout : nullptr;
      float r = 0.f;
      for (int q = xs >> 2; q <= ((xe - 1) >> 2); ++q) {
        float part = 0.f;
        for (int e = 0; e < 4; ++e) {
          const int ox = 4 * q + e;
          if (ox < xs || ox >= xe) continue;
          int x0, x1;
          float lx;
          tg_coord(sw, ox, Win, x0, x1, lx);
          const float hx = 1.f - lx;
          float g = row[ox];
          if (rowb) g = g + rowb[ox];
          if (x0 == ix) part = part + hx * g;
          if (x1 == ix) part = part + lx * g;
        }
        r = r + part;
      }
      if (y0 == iy) acc = acc + hy * r;
      if (y1 == iy) acc = acc + ly * r;
    }
    float v = pl.mul * acc;
    if (pl.accumulate) v = pl.dst[node] + v;
    pl.dst[node] = v;
  }
}

// The up-sampling adjoint (scale <= 1/4 along x, e.g. the x8 of the decoder), 16-byte aligned, no second addend: one
// workgroup walks whole planes.  A lane owns one quad of four output columns (its x taps and weights are built once) and
// reads it with one 16-byte load from each of 4 rows per step, the loads of the next step in flight while this one is
// reduced: quad partials -> LDS -> row sums r(oy, ix) -> LDS -> lane ix folds the rows in ascending order into the two
// input rows that are open (y0 and y0 + 1), and stores a row when the walk has passed it.
#define TG_ROWS_PER_LANE 4
__global__ __launch_bounds__(TG_THREADS) void resize_grad_rows_kernel(ResizeGradJobs jobs, int T, int Hin, int Win,
                                                                      int Hout, int Wout, float sh, float sw, int qpr, int rp) {
#pragma clang fp contract(off)
  __shared__ float4 s_part[1024];      // [row slot][quad]: partials of nodes a, a + 1, a + 2 (a = x0 of the quad's first column)
  __shared__ float s_row[1024];        // [row slot][ix]
  __shared__ int s_a[TG_THREADS];
  const int tid = threadIdx.x;
  const int quad = tid % qpr, rslot = tid / qpr;
  const bool loader = rslot < rp;
  const int RS = TG_ROWS_PER_LANE * rp;                  // rows per step
  int k0[4], k1[4];
  float hx[4], lx[4];
  {
    int a = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      int x0, x1;
      tg_coord(sw, 4 * quad + e, Win, x0, x1, lx[e]);
      if (e == 0) a = x0;
      k0[e] = x0 - a;
      k1[e] = x1 - a;
      hx[e] = 1.f - lx[e];
    }
    if (rslot == 0) s_a[quad] = a;
  }
  // the items (row slot, ix) this thread sums in stage 2, and the quads that reach node ix
  int qlo[TG_ROWS_PER_LANE], qhi[TG_ROWS_PER_LANE];
  const int items = RS * Win;
#pragma unroll
  for (int m = 0; m < TG_ROWS_PER_LANE; ++m) {
    const int item = tid + TG_THREADS * m;
    const int ix = item % Win;
    qlo[m] = tg_lower(sw, Win, Wout, ix - 1) >> 2;
    qhi[m] = (tg_lower(sw, Win, Wout, ix + 1) - 1) >> 2;
  }
  __syncthreads();
  const int total = T * (jobs.planes[0] + jobs.planes[1]);
  const long long in_px = (long long)Hin * Win, out_px = (long long)Hout * Wout;
  const int nsteps = (Hout + RS - 1) / RS;
  for (int p = blockIdx.x; p < total; p += gridDim.x) {
    const TgPlane pl = tg_plane(jobs, p, in_px, out_px);
    int cur = 0;
    float accA = 0.f, accB = 0.f;                        // nodes (cur, ix) and (cur + 1, ix) of lane ix < Win
    float4 v[TG_ROWS_PER_LANE];
#pragma unroll
    for (int j = 0; j < TG_ROWS_PER_LANE; ++j) {
      const int oy = j * rp + rslot;
      v[j] = (loader && oy < Hout) ? *reinterpret_cast<const float4*>(pl.src + (long long)oy * Wout + 4 * quad) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int step = 0; step < nsteps; ++step) {
      if (loader) {
#pragma unroll
        for (int j = 0; j < TG_ROWS_PER_LANE; ++j) {
          const float g[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
          float pk[3] = {0.f, 0.f, 0.f};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float th = hx[e] * g[e], tl = lx[e] * g[e];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
              pk[k] = pk[k] + (k0[e] == k ? th : 0.f);
              pk[k] = pk[k] + (k1[e] == k ? tl : 0.f);
            }
          }
          s_part[(j * rp + rslot) * qpr + quad] = make_float4(pk[0], pk[1], pk[2], 0.f);
        }
      }
      if (step + 1 < nsteps) {
#pragma unroll
        for (int j = 0; j < TG_ROWS_PER_LANE; ++j) {
          const int oy = (step + 1) * RS + j * rp + rslot;
          v[j] = (loader && oy < Hout) ? *reinterpret_cast<const float4*>(pl.src + (long long)oy * Wout + 4 * quad) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
      }
      __syncthreads();
#pragma unroll
      for (int m = 0; m < TG_ROWS_PER_LANE; ++m) {
        const int item = tid + TG_THREADS * m;
        if (item < items) {
          const int slot = item / Win, ix = item - slot * Win;
          float r = 0.f;
          for (int q = qlo[m]; q <= qhi[m]; ++q) {
            const int k = ix - s_a[q];
            const float4 s = s_part[slot * qpr + q];
            r = r + (k == 0 ? s.x : k == 1 ? s.y : s.z);
          }
          s_row[item] = r;
        }
      }
      __syncthreads();
      if (tid < Win) {
        for (int slot = 0; slot < RS; ++slot) {
          const int oy = step * RS + slot;
          if (oy >= Hout) break;
          int y0, y1;
          float ly;
          tg_coord(sh, oy, Hin, y0, y1, ly);
          const float hy = 1.f - ly;
          const float r = s_row[slot * Win + tid];
          while (cur < y0) {
            float o = pl.mul * accA;
            float* d = pl.dst + (long long)cur * Win + tid;
            if (pl.accumulate) o = *d + o;
            *d = o;
            accA = accB; accB = 0.f; ++cur;
          }
          accA = accA + hy * r;
          if (y1 > y0) accB = accB + ly * r; else accA = accA + ly * r;
        }
      }
    }
    if (tid < Win) {
      while (cur < Hin) {
        float o = pl.mul * accA;
        float* d = pl.dst + (long long)cur * Win + tid;
        if (pl.accumulate) o = *d + o;
        *d = o;
        accA = accB; accB = 0.f; ++cur;
      }
    }
    // s_part is rewritten before the next barrier by lanes that have passed the second one; s_row is rewritten after
    // the next first barrier, which the folding lanes reach only after their last read of it
  }
}

static bool tg_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

extern "C" int scf_resize_bilinear_grad(const float* const* g, const float* const* g_add, float* const* out, int64_t planes,
                                        float mul, int accumulate, const float* const* g1, float* const* out1,
                                        int64_t planes1, float mul1, int accumulate1, int T, int Hin, int Win, int Hout,
                                        int Wout, scf_stream_t stream) {
  if (!g || !out || planes <= 0 || planes1 < 0 || (planes1 > 0 && (!g1 || !out1)) || T <= 0 || Hin <= 0 || Win <= 0 ||
      Hout <= 0 || Wout <= 0)
    return SCF_EINVAL;
  if (T > TG_MAX_T) return SCF_EUNSUPPORTED;
  const long long total = (long long)T * (planes + planes1);
  if (total > 0x7fffffffLL || (long long)Hin * Win > 0x7fffffffLL || (long long)Hout * Wout > 0x7fffffffLL ||
      planes + planes1 > 0x7fffffffLL)
    return SCF_EUNSUPPORTED;
  ResizeGradJobs jobs = {};
  jobs.planes[0] = (int)planes; jobs.mul[0] = mul; jobs.accumulate[0] = accumulate ? 1 : 0;
  jobs.planes[1] = (int)planes1; jobs.mul[1] = mul1; jobs.accumulate[1] = accumulate1 ? 1 : 0;
  bool aligned = (Wout & 3) == 0, has_add = false;
  for (int t = 0; t < T; ++t) {
    if (!g[t] || !out[t] || (planes1 > 0 && (!g1[t] || !out1[t]))) return SCF_EINVAL;
    jobs.src[0][t] = g[t]; jobs.srcb[t] = g_add ? g_add[t] : nullptr; jobs.dst[0][t] = out[t];
    has_add = has_add || jobs.srcb[t];
    aligned = aligned && tg_aligned16(g[t]);
    if (planes1 > 0) {
      jobs.src[1][t] = g1[t]; jobs.dst[1][t] = out1[t];
      aligned = aligned && tg_aligned16(g1[t]);
    }
  }
  const float sh = Hout > 1 ? (float)(Hin - 1) / (float)(Hout - 1) : 0.f;
  const float sw = Wout > 1 ? (float)(Win - 1) / (float)(Wout - 1) : 0.f;
  hipStream_t st = scf_stream(stream);
  const int qpr = Wout / 4;
  if (aligned && !has_add && sw <= 0.25f && qpr >= 1 && qpr <= TG_THREADS && Win <= qpr && Hin * (long long)Win <= 0x7fffffffLL) {
    // a few workgroups per CU, each walking planes (the lesson at the top of resample.hip)
    long long grid = 4LL * scf_cu_count();
    grid = grid > total ? total : grid;
    scf_launch(resize_grad_rows_kernel, dim3((unsigned)grid), dim3(TG_THREADS), 0, st, jobs, T, Hin, Win, Hout, Wout, sh, sw, qpr,
               TG_THREADS / qpr);
    return scf_launch_status();
  }
  const long long gx = scf_cdiv((long long)Hin * Win, TG_THREADS);
  if (gx > 0x7fffffffLL) return SCF_EUNSUPPORTED;
  long long gy = scf_cdiv(8LL * scf_cu_count(), gx);
  gy = gy < 1 ? 1 : gy > total ? total : gy > 65535 ? 65535 : gy;
  scf_launch(resize_grad_gather_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(TG_THREADS), 0, st, jobs, T, Hin, Win, Hout, Wout, sh,
             sw);
  return scf_launch_status();
}

// ================================================================================================ re-projection sums
// flow = (qx / qz - x, qy / qz - y), q = K (R P + t), P the object-frame point of the pixel (pose.hip).  Per foreground
// pixel, in fp32:  g_q = (gu / qz, gv / qz, -(gu qx + gv qy) / (qz qz)),  g_p = K^T g_q;  per (iteration, sample), in fp64:
// words [0, 9) = sum g_p (x) P (row-major, d / dR), words [9, 12) = sum g_p (d / dt).  A block folds lane -> wave (shuffle
// tree) -> waves in order (LDS) and writes its 12 words; scf_pose_tail_grad adds the blocks of a sample in block order.
#define TG_WORDS 12
struct ReprojGradK {
  const float* depth; const float* K; const float* R0; const float* t0;
  const float* R[TG_MAX_T]; const float* t[TG_MAX_T]; const float* g[TG_MAX_T];
  int N, H, W, tiles;
};

static int tg_tiles(long long hw) {
  const long long t = scf_cdiv(hw, 4 * TG_THREADS);
  return (int)(t < 1 ? 1 : t > 16 ? 16 : t);
}

__device__ __forceinline__ double tg_wave_sum(double s) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
  return s;
}

__global__ __launch_bounds__(TG_THREADS) void reproject_flow_grad_kernel(ReprojGradK k, double* ws) {
  __shared__ PoseMats s;
  __shared__ double s_red[TG_WAVES][TG_WORDS];
  const int tile = blockIdx.x, n = blockIdx.y, ti = blockIdx.z, tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  double* out = ws + (((long long)ti * k.N + n) * k.tiles + tile) * TG_WORDS;
  const float* g = k.g[ti];
  if (!g) {                                    // no cotangent for this iteration: exact zeros (uniform over the block)
    if (tid < TG_WORDS) out[tid] = 0.0;
    return;
  }
  load_mats(&s, k.K, k.R0, k.t0, k.R[ti], k.t[ti], n);
  const int hw = k.H * k.W;
  const float* dp = k.depth + (long long)n * hw;
  const float* gx = g + (long long)n * 2 * hw;
  const float* gy = gx + hw;
  double acc[TG_WORDS];
#pragma unroll
  for (int i = 0; i < TG_WORDS; ++i) acc[i] = 0.0;
  for (int idx = tile * TG_THREADS + tid; idx < hw; idx += k.tiles * TG_THREADS) {
    const float d = dp[idx];
    if (d > 0.f) {                             // the forward's decision: a NaN depth is background
      const int yi = idx / k.W, xi = idx - yi * k.W;
      float P[3];
      unproject(s, (float)xi, (float)yi, d, P[0], P[1], P[2]);
      const float px = s.R[0] * P[0] + s.R[1] * P[1] + s.R[2] * P[2] + s.t[0];
      const float py = s.R[3] * P[0] + s.R[4] * P[1] + s.R[5] * P[2] + s.t[1];
      const float pz = s.R[6] * P[0] + s.R[7] * P[1] + s.R[8] * P[2] + s.t[2];
      const float qx = s.K[0] * px + s.K[1] * py + s.K[2] * pz;
      const float qy = s.K[3] * px + s.K[4] * py + s.K[5] * pz;
      const float qz = s.K[6] * px + s.K[7] * py + s.K[8] * pz;
      const float gu = gx[idx], gv = gy[idx];
      const float a = gu / qz, b = gv / qz;
      const float c = -(gu * qx + gv * qy) / (qz * qz);
      float gp[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) gp[j] = s.K[j] * a + s.K[3 + j] * b + s.K[6 + j] * c;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) acc[3 * i + j] += (double)(gp[i] * P[j]);
        acc[9 + i] += (double)gp[i];
      }
    }
  }
#pragma unroll
  for (int i = 0; i < TG_WORDS; ++i) {
    const double v = tg_wave_sum(acc[i]);
    if (lane == 0) s_red[wave][i] = v;
  }
  __syncthreads();
  if (tid < TG_WORDS) {
    double v = s_red[0][tid];
    for (int w = 1; w < TG_WAVES; ++w) v += s_red[w][tid];
    out[tid] = v;
  }
}

extern "C" int64_t scf_tail_grad_workspace_bytes(int N, int H, int W, int T) {
  if (N <= 0 || H <= 0 || W <= 0 || T <= 0 || T > TG_MAX_T || (int64_t)H * W > 0x7fffffffLL) return SCF_EINVAL;
  return (int64_t)T * N * tg_tiles((long long)H * W) * TG_WORDS * 8;
}

extern "C" int scf_reproject_flow_grad(const float* depth, const float* K, const float* R0, const float* t0,
                                       const float* const* R, const float* const* t, const float* const* g_flow, int T, int N,
                                       int H, int W, void* workspace, scf_stream_t stream) {
  if (!depth || !K || !R0 || !t0 || !R || !t || !g_flow || !workspace || T <= 0 || N <= 0 || H <= 0 || W <= 0) return SCF_EINVAL;
  if (T > TG_MAX_T || N > 65535 || (int64_t)H * W > 0x7fffffffLL) return SCF_EUNSUPPORTED;
  ReprojGradK k = {};
  k.depth = depth; k.K = K; k.R0 = R0; k.t0 = t0; k.N = N; k.H = H; k.W = W; k.tiles = tg_tiles((long long)H * W);
  for (int i = 0; i < T; ++i) {
    if (g_flow[i] && (!R[i] || !t[i])) return SCF_EINVAL;
    k.R[i] = R[i]; k.t[i] = t[i]; k.g[i] = g_flow[i];
  }
  scf_launch(reproject_flow_grad_kernel, dim3((unsigned)k.tiles, (unsigned)N, (unsigned)T), dim3(TG_THREADS), 0, scf_stream(stream), k,
             static_cast<double*>(workspace));
  return scf_launch_status();
}

// ================================================================================================ pose scan
// R_i = Rd(d_rot_i) R_{i-1}, t_i = compose(d_trans_i, t_{i-1}) (pose.hip, pose_update_one).  One thread per sample walks
// i = T-1 .. 0 in fp64 on the fp32 values the forward stored:  G = g(loss)_i + g(re-projection)_i + carry, then the
// backward of the ortho6d construction and of the translation compose, each output rounded to fp32 once.
struct PoseTailK {
  const float* d_rot[TG_MAX_T]; const float* d_trans[TG_MAX_T];
  const float* R[TG_MAX_T]; const float* t[TG_MAX_T];        // R_i, t_i: entry i - 1 is the input of iteration i
  const float* gR[TG_MAX_T]; const float* gt[TG_MAX_T];      // NULL entries: no cotangent
  float* g_drot[TG_MAX_T]; float* g_dtrans[TG_MAX_T];
  const float* R0; const float* t0; const double* sums;
  int tiles, T, N, flags, label_mode;
};

__device__ __forceinline__ void tg_cross(const double* u, const double* v, double* o) {
  o[0] = u[1] * v[2] - u[2] * v[1];
  o[1] = u[2] * v[0] - u[0] * v[2];
  o[2] = u[0] * v[1] - u[1] * v[0];
}

// backward of F.normalize (v / max(|v|, eps)): g / den, and through the norm only where it is not clamped
__device__ __forceinline__ void tg_normalize_bwd(const double* v, double nrm, double den, const double* g, double* gv) {
  const double dot = g[0] * v[0] + g[1] * v[1] + g[2] * v[2];
  const double gden = -dot / (den * den);
  for (int i = 0; i < 3; ++i) {
    gv[i] = g[i] / den;
    if (nrm >= 1e-12) gv[i] += v[i] * (gden / nrm);
  }
}

__global__ __launch_bounds__(64) void pose_tail_grad_kernel(PoseTailK k) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= k.N) return;
  const bool detach_pose = (k.flags & SCF_TAIL_DETACH_POSE) != 0, detach_depth = (k.flags & SCF_TAIL_DETACH_DEPTH_FOR_XY) != 0;
  const bool linear = (k.label_mode & SCF_POSE_DEPTH_LINEAR) != 0;
  double cR[9], ct[3];
  for (int j = 0; j < 9; ++j) cR[j] = 0.0;
  for (int j = 0; j < 3; ++j) ct[j] = 0.0;
  for (int i = k.T - 1; i >= 0; --i) {
    double G[9], Gt[3];
    for (int j = 0; j < 9; ++j) G[j] = k.gR[i] ? (double)k.gR[i][(long long)n * 9 + j] : 0.0;
    for (int j = 0; j < 3; ++j) Gt[j] = k.gt[i] ? (double)k.gt[i][(long long)n * 3 + j] : 0.0;
    if (k.sums) {
      double s[TG_WORDS];
      for (int j = 0; j < TG_WORDS; ++j) s[j] = 0.0;
      const double* w = k.sums + ((long long)i * k.N + n) * k.tiles * TG_WORDS;
      for (int tile = 0; tile < k.tiles; ++tile)
        for (int j = 0; j < TG_WORDS; ++j) s[j] += w[tile * TG_WORDS + j];
      for (int j = 0; j < 9; ++j) G[j] += s[j];
      for (int j = 0; j < 3; ++j) Gt[j] += s[9 + j];
    }
    for (int j = 0; j < 9; ++j) G[j] += cR[j];
    for (int j = 0; j < 3; ++j) Gt[j] += ct[j];
    const float* Rp32 = i == 0 ? k.R0 : k.R[i - 1];
    const float* tp32 = i == 0 ? k.t0 : k.t[i - 1];
    double Rp[9], tp[3], a[3], b[3], dt[3];
    for (int j = 0; j < 9; ++j) Rp[j] = (double)Rp32[(long long)n * 9 + j];
    for (int j = 0; j < 3; ++j) {
      tp[j] = (double)tp32[(long long)n * 3 + j];
      a[j] = (double)k.d_rot[i][(long long)n * 6 + j];
      b[j] = (double)k.d_rot[i][(long long)n * 6 + 3 + j];
      dt[j] = (double)k.d_trans[i][(long long)n * 3 + j];
    }
    // ---- rotation: x = normalize(a), z = normalize(x X b), y = z X x, Rd = [x y z] (columns)
    const double na = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]), da = na > 1e-12 ? na : 1e-12;
    double x[3], zp[3], z[3], y[3];
    for (int j = 0; j < 3; ++j) x[j] = a[j] / da;
    tg_cross(x, b, zp);
    const double nz = sqrt(zp[0] * zp[0] + zp[1] * zp[1] + zp[2] * zp[2]), dz = nz > 1e-12 ? nz : 1e-12;
    for (int j = 0; j < 3; ++j) z[j] = zp[j] / dz;
    tg_cross(z, x, y);
    double gx[3], gy[3], gz[3];                       // columns of g_Rd = G R_{i-1}^T
    for (int r = 0; r < 3; ++r) {
      gx[r] = G[r * 3] * Rp[0] + G[r * 3 + 1] * Rp[1] + G[r * 3 + 2] * Rp[2];
      gy[r] = G[r * 3] * Rp[3] + G[r * 3 + 1] * Rp[4] + G[r * 3 + 2] * Rp[5];
      gz[r] = G[r * 3] * Rp[6] + G[r * 3 + 1] * Rp[7] + G[r * 3 + 2] * Rp[8];
    }
    double tmp[3], gzp[3], ga[3], gb[3];
    tg_cross(x, gy, tmp);                             // y = z X x: g_z += x X g_y, g_x += g_y X z
    for (int j = 0; j < 3; ++j) gz[j] += tmp[j];
    tg_cross(gy, z, tmp);
    for (int j = 0; j < 3; ++j) gx[j] += tmp[j];
    tg_normalize_bwd(zp, nz, dz, gz, gzp);
    tg_cross(b, gzp, tmp);                            // zp = x X b: g_x += b X g_zp, g_b = g_zp X x
    for (int j = 0; j < 3; ++j) gx[j] += tmp[j];
    tg_cross(gzp, x, gb);
    tg_normalize_bwd(a, na, da, gx, ga);
    for (int j = 0; j < 3; ++j) {
      k.g_drot[i][(long long)n * 6 + j] = (float)ga[j];
      k.g_drot[i][(long long)n * 6 + 3 + j] = (float)gb[j];
    }
    // ---- translation: vz = tz / exp(dz) | tz (dz + 1); vx = vz (dx / 10 + tx / tz), vy likewise (vz detached there under detach_depth)
    const double ez = linear ? 0.0 : exp(dt[2]);
    const double vz = linear ? tp[2] * (dt[2] + 1.0) : tp[2] / ez;
    const double u = dt[0] / 10.0 + tp[0] / tp[2], v = dt[1] / 10.0 + tp[1] / tp[2];
    const double gvz = Gt[2] + (detach_depth ? 0.0 : Gt[0] * u + Gt[1] * v);
    const double gu = Gt[0] * vz, gv = Gt[1] * vz;
    const double gdz = linear ? gvz * tp[2] : -gvz * vz;
    k.g_dtrans[i][(long long)n * 3 + 0] = (float)(gu / 10.0);
    k.g_dtrans[i][(long long)n * 3 + 1] = (float)(gv / 10.0);
    k.g_dtrans[i][(long long)n * 3 + 2] = (float)gdz;
    if (detach_pose) continue;                        // the next pose was built on a detached copy: no carry
    const double Rd[9] = {x[0], y[0], z[0], x[1], y[1], z[1], x[2], y[2], z[2]};
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) cR[r * 3 + c] = Rd[r] * G[c] + Rd[3 + r] * G[3 + c] + Rd[6 + r] * G[6 + c];     // Rd^T G
    ct[0] = gu / tp[2];
    ct[1] = gv / tp[2];
    ct[2] = -(gu * tp[0] + gv * tp[1]) / (tp[2] * tp[2]) + (linear ? gvz * (dt[2] + 1.0) : gvz / ez);
  }
}

extern "C" int scf_pose_tail_grad(const float* const* d_rot, const float* const* d_trans, const float* R0, const float* t0,
                                  const float* const* R, const float* const* t, const float* const* g_R,
                                  const float* const* g_t, const void* reproject_sums, int H, int W, int flags, int label_mode,
                                  float* const* g_d_rot, float* const* g_d_trans, int T, int N, scf_stream_t stream) {
  if (!d_rot || !d_trans || !R0 || !t0 || !R || !t || !g_d_rot || !g_d_trans || T <= 0 || N <= 0) return SCF_EINVAL;
  if ((flags & ~(SCF_TAIL_DETACH_POSE | SCF_TAIL_DETACH_DEPTH_FOR_XY)) || (label_mode & ~(SCF_POSE_LABEL_PER_SAMPLE | SCF_POSE_DEPTH_LINEAR)))
    return SCF_EINVAL;
  if (reproject_sums && (H <= 0 || W <= 0)) return SCF_EINVAL;
  if (T > TG_MAX_T) return SCF_EUNSUPPORTED;
  PoseTailK k = {};
  for (int i = 0; i < T; ++i) {
    if (!d_rot[i] || !d_trans[i] || !g_d_rot[i] || !g_d_trans[i] || (i + 1 < T && (!R[i] || !t[i]))) return SCF_EINVAL;
    k.d_rot[i] = d_rot[i]; k.d_trans[i] = d_trans[i]; k.R[i] = R[i]; k.t[i] = t[i];
    k.gR[i] = g_R ? g_R[i] : nullptr; k.gt[i] = g_t ? g_t[i] : nullptr;
    k.g_drot[i] = g_d_rot[i]; k.g_dtrans[i] = g_d_trans[i];
  }
  k.R0 = R0; k.t0 = t0; k.sums = static_cast<const double*>(reproject_sums);
  k.tiles = reproject_sums ? tg_tiles((long long)H * W) : 0;
  k.T = T; k.N = N; k.flags = flags; k.label_mode = label_mode;
  scf_launch(pose_tail_grad_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, scf_stream(stream), k);
  return scf_launch_status();
}
