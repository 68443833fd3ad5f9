// The train pipeline's object patches for gfx950: pose jitter, a random crop ratio, colour augmentation before the resize,
// and the ground-truth mask, batched over objects.  It restates the train_pipeline of configs/refine_datasets/ycbv_real.py,
//   LoadMasks -> PoseJitter -> ComputeBbox -> Crop(size_range=(lo, hi)) -> RandomHSV -> RandomNoise -> RandomSmooth ->
//   Resize -> Pad -> RemapPose(keep_intrinsic=False) -> Normalize
// (datasets/pipelines/jitter.py:51-109, color_transform.py:76-133), which the reference runs object by object on the CPU with
// numpy, scipy, cv2 and mmcv.  None of them is used or needed; the semantics below are the contract, and
// tests/test_patches_train_host.py restates them in numpy (patch_train_reference).  Agreement with cv2 (cvtColor, blur,
// resize) is UNVERIFIED: cv2 is not a dependency.  patch.hip states items 1-6 of the val path; they run here as they stand.
//
// A. Random numbers: scf_rng.h.  Every draw is hash(seed, sample_id, stream, counter); sample_id = id_base + n, or
//    sample_ids[n].  Everything that reaches an integer or a uniform is bit-exact against the restatement; only the
//    transcendental part of a normal draw (ln, sqrt, cos) is not.
// B. PoseJitter (scf_pose_jitter), fp64 throughout.  Try t = 0 .. max_tries - 1 makes six normal draws z_i (stream JITTER,
//    counter 8 t + i): angles a_i = angle[0] + angle[1] z_i in degrees (i = 0..2), translation noise
//    (x[0] + x[1] z_3, y[0] + y[1] z_4, z[0] + z[1] z_5).  dR = Rx(a_2) Ry(a_1) Rz(a_0) -- scipy's
//    from_euler('zyx', [a_0, a_1, a_2]), lower case = extrinsic axes -- R_ref = dR R_gt, t_ref = t_gt + noise.
//      rotation error    acos(clip((tr(R_ref R_gt^T) - 1) / 2, -1, 1)) in degrees (the reference inverts R_gt)
//      translation error |noise|
//      ADD               mean |(R_gt - R_ref) X + (t_gt - t_ref)| / diameter[label] over every vertex_stride-th vertex of
//                        the class (the deterministic stand-in for the reference's 1000 random vertices, as the box's),
//                        summed per thread and then through a fixed tree: the same bits on every run
//    A try is rejected when a given limit (>= 0; negative = none) is exceeded; the first accepted try wins.  When none is,
//    R_ref = R_gt, t_ref = t_gt, the errors are 0, ok = 0, tries = max_tries: the kernel cannot loop for ever.  With a mesh,
//    a label outside [0, num_classes) gives the same identity result with tries = 0, and so does an empty class while
//    add_limit is set.  Without a mesh (only allowed without add_limit) labels are not read and add_error is NaN; with a
//    mesh and no add_limit the accepted try's ADD is still reported.
//    Two facts about the reference: its __call__ unpacks jitter()'s last two results in the wrong order (jitter.py:79
//    against :93), so init_rot_error holds the translation norm and init_trans_error the angle -- rot_error / trans_error
//    are written that way unless fix_error_swap_quirk is set; and its constructor cannot run with add_limit set
//    (mesh_vertices is read before assignment, jitter.py:45), so the shipped train_pipeline's add_limit never ran there.
// C. Per-object draws (scf_patch_boxes_train), fp64: size_ratio = lo + (hi - lo) u (stream CROP); gate_x on when
//    u <= p_x (streams GATE_*; the reference skips when random() > p); gains a, b, c = float32((2 u - 1) ratio_x + 1)
//    (stream HSV, counters 0..2); sigma = u noise_ratio (stream SIGMA) and s255 = float32(sigma 255);
//    k = 2 min(int(u m), m - 1) + 1 with m = max_kernel_size / 2 + 1 (stream SMOOTH), 1 when the gate is off.  m is the
//    length of the reference's own list [2 i + 1 for i in range(max_kernel_size // 2 + 1)] (color_transform.py:125): an
//    EVEN max_kernel_size therefore also draws k = max_kernel_size + 1 (4 gives {1, 3, 5}), as the reference does.
//    draws (N,8) fp64 = (size_ratio, a, b, c, sigma, k, hsv on, noise on).  Items 1-5 of patch.hip then run on the box of
//    the pose handed in (the jittered one) with size_ratio per object.
// D. Pixels (scf_patch_extract_train), on the crop patch of ph x pw pixels, Crop's fill pixels included:
//    a. source: the frame's BGR byte, or crop_pad_val.
//    b. RandomHSV.  BGR -> HSV in integers (8 bit, H in [0, 180)): v = max, d = v - min,
//         s = (d sdiv[v] + 2048) >> 12, sdiv[i] = rint((255 << 12) / i)  (fp64 quotient, ties to even; sdiv[0] = 0)
//         h' = g - b when v == r, else b - r + 2 d when v == g, else r - g + 4 d
//         h = (h' hdiv[d] + 2048) >> 12 (arithmetic shift), hdiv[i] = rint((180 << 12) / (6 i)), + 180 when negative
//       gains in fp32: x = float(h) a, clipped to 179 ONLY WHEN a >= 1 (the reference's rule), truncated; s and v likewise
//       with b, c and 255.  HSV -> BGR in fp32, every operation separately rounded:
//         s = S (1/255), v = V (1/255), hh = H (6/180) (fp32 constants), sector = floor(hh), f = hh - sector,
//         tab = (v, v (1 - s), v (1 - s f), v (1 - s (1 - f))), (b, g, r) = tab[{1,3,0},{1,0,2},{3,0,1},{0,2,1},{0,1,3},
//         {2,1,0}][sector], byte = rint(255 x) saturated.
//    c. RandomNoise: z from hash(.., NOISE, (y pw + x) 3 + c) with u1, u2 rounded to fp32,
//       z = sqrtf(-2 logf(u1)) cosf(float32(2 pi) u2), byte = trunc(clip(float(byte) + z s255, 0, 255)) in fp32.
//    d. RandomSmooth: k x k box mean over the patch, BORDER_REFLECT_101 (index -i -> i, n - 1 + i -> n - 1 - i, repeated
//       until inside; a side of 1 pixel clamps), integer sum S, byte = (S + k^2 / 2) / k^2 (k^2 is odd: no ties).
//    e. items 3, 4 and 6 of patch.hip on the augmented patch.
//    f. mask (N,Hf,Wf) uint8, nonzero = object: crop with fill 0, nearest resize src = min(floor(d (src / dst)), src - 1)
//       per axis in fp64 (the record's src / dst), pad with mask_pad_val; out (N,H,W) bytes 0 / 1.  An invalid object's mask
//       is all mask_pad_val.
//    With k = 1, both gates off and no masks the result is scf_patch_extract's, bit for bit.
//
// Layout.  pose_jitter_kernel: one workgroup per object, every thread repeats the draws (uniform control flow), the ADD sum
// is the only block-wide step.  patch_draw_kernel: one thread per object.  patch_extract_train_kernel: one block per
// 16 x 64 output tile, one thread per four consecutive columns of a row (the stores of patch_extract_kernel).  Two routes:
//   LDS     the tile's source footprint (its rows and columns of taps, plus k / 2 on every side) is staged in LDS after
//           steps a-c as packed BGR words, summed horizontally (three 16-bit planes), then vertically into the blurred
//           bytes, which the four taps per output pixel read.  50 KiB of dynamic LDS + 2 KiB of tables per block: three
//           blocks per CU of 160 KiB.
//   direct  a footprint that does not fit (strong down-scaling, huge crops): each thread evaluates its taps' k^2
//           neighbourhoods itself.  Same integers, same bits.
// The route is a function of (ph, pw, new_h, new_w, k) alone -- scf_patch_train_route, the kernel's own formula on the host
// -- through an upper bound of the footprint: cap = min(src, (tile - 1) src / dst + 4) per axis (the taps of `tile`
// consecutive outputs span at most (tile - 1) src/dst + 1 source pixels, + 1 for the fp32 rounding of the coordinate while
// src <= 2^20, + 1 for the second tap, + 1 for counting both ends); larger patches take the direct route.
#include "patch_common.h"
#include "scf_rng.h"

#pragma clang fp contract(off)

#define PT_THREADS 256
#define PT_TH 16
#define PT_TW 64
#define PT_LDS_BYTES 51200
#define PT_MAX_K 15
#define PT_MAX_SIDE (1 << 20)
#define JIT_THREADS 256
#define PT_PI 3.14159265358979323846

struct PatchAug {            // 64 bytes per object, after the N PatchRec records
  double ratio, sigma;
  uint64_t sample_id;
  float a, b, c, s255;
  int k, hsv_on, noise_on;
  int reserved[3];
};
static_assert(sizeof(PatchAug) == 64, "PatchAug is 64 bytes");

__host__ __device__ static inline int pt_cap(int src, int dst, int tile) {
  const int64_t c = ((int64_t)(tile - 1) * src) / dst + 4;
  return c < src ? (int)c : src;
}
__host__ __device__ static inline int64_t pt_lds_need(int fh, int fw, int r) {
  const int64_t ah = fh + 2 * r, aw = fw + 2 * r;
  return 4 * ah * aw + (r ? 6 * ah * fw + 8 : 0);
}
__host__ __device__ static inline int pt_route(int ph, int pw, int new_h, int new_w, int k) {
  if (ph > PT_MAX_SIDE || pw > PT_MAX_SIDE) return 1;
  return pt_lds_need(pt_cap(ph, new_h, PT_TH), pt_cap(pw, new_w, PT_TW), k / 2) <= PT_LDS_BYTES ? 0 : 1;
}

// -------------------------------------------------------------------------------------------- jitter
struct JitterCfg {
  double angle[2], x[2], y[2], z[2];
  double angle_limit, trans_limit, add_limit;
  uint64_t seed;
  int max_tries, fix_swap, stride;
};

__device__ __forceinline__ double jit_normal(uint64_t seed, uint64_t sid, uint64_t counter) {
  const uint64_t h = scf_rng_hash(seed, sid, SCF_RNG_JITTER, counter);
  return sqrt(-2.0 * log(scf_rng_u1(h))) * cos((2.0 * PT_PI) * scf_rng_u2(h));
}

__global__ void __launch_bounds__(JIT_THREADS) pose_jitter_kernel(const float* verts, const int* vert_offset, int num_classes,
                                                                  const float* diam, const int* labels, const float* Rg,
                                                                  const float* tg, JitterCfg c, int64_t id_base,
                                                                  const int64_t* sample_ids, float* R_ref, float* t_ref,
                                                                  float* add_err, float* rot_err, float* trans_err, int* ok,
                                                                  int* tries) {
  __shared__ double part[JIT_THREADS];
  const int n = blockIdx.x, tid = threadIdx.x;
  const uint64_t sid = (uint64_t)(sample_ids ? sample_ids[n] : id_base + n);
  double R[9], t[3];
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = (double)Rg[9 * (int64_t)n + i];
#pragma unroll
  for (int i = 0; i < 3; ++i) t[i] = (double)tg[3 * (int64_t)n + i];
  int vbase = 0, nv = 0;
  bool usable = true;
  double d = 1.0;
  if (verts) {
    const int l = labels[n];
    if (l >= 0 && l < num_classes) {
      vbase = vert_offset[l];
      nv = max(vert_offset[l + 1] - vbase, 0);
      d = (double)diam[l];
    } else {
      usable = false;
    }
    if (nv == 0 && c.add_limit >= 0) usable = false;
  }
  const bool with_add = verts && nv > 0;
  double Rr[9], tr[3], e_rot = 0.0, e_trans = 0.0, e_add = 0.0;
  bool found = false;
  int t_used = 0;
  for (int tr_i = 0; usable && tr_i < c.max_tries && !found; ++tr_i) {
    t_used = tr_i + 1;
    double z[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) z[i] = jit_normal(c.seed, sid, (uint64_t)tr_i * 8 + i);
    const double a0 = (c.angle[0] + c.angle[1] * z[0]) * (PT_PI / 180.0);
    const double a1 = (c.angle[0] + c.angle[1] * z[1]) * (PT_PI / 180.0);
    const double a2 = (c.angle[0] + c.angle[1] * z[2]) * (PT_PI / 180.0);
    const double nz[3] = {c.x[0] + c.x[1] * z[3], c.y[0] + c.y[1] * z[4], c.z[0] + c.z[1] * z[5]};
    const double cz = cos(a0), sz = sin(a0), cy = cos(a1), sy = sin(a1), cx = cos(a2), sx = sin(a2);
    // Rx(a2) Ry(a1) Rz(a0)
    const double D[9] = {cy * cz, -cy * sz, sy,
                         sx * sy * cz + cx * sz, -sx * sy * sz + cx * cz, -sx * cy,
                         -cx * sy * cz + sx * sz, cx * sy * sz + sx * cz, cx * cy};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) Rr[3 * i + j] = D[3 * i] * R[j] + D[3 * i + 1] * R[3 + j] + D[3 * i + 2] * R[6 + j];
    double trace = 0.0;                                   // tr(R_ref R_gt^T) = sum of the element-wise products
#pragma unroll
    for (int i = 0; i < 9; ++i) trace += Rr[i] * R[i];
    e_rot = acos(fmin(fmax((trace - 1.0) / 2.0, -1.0), 1.0)) * (180.0 / PT_PI);
    e_trans = sqrt(nz[0] * nz[0] + nz[1] * nz[1] + nz[2] * nz[2]);
#pragma unroll
    for (int i = 0; i < 3; ++i) tr[i] = t[i] + nz[i];
    bool rej = (c.angle_limit >= 0 && e_rot > c.angle_limit) || (c.trans_limit >= 0 && e_trans > c.trans_limit);
    if (!rej && with_add) {                               // uniform: every thread holds the same values
      double s = 0.0;
      for (int64_t i = (int64_t)tid * c.stride; i < nv; i += (int64_t)JIT_THREADS * c.stride) {
        const float* X = verts + 3 * (vbase + i);
        const double x = X[0], y = X[1], w = X[2];
        const double dx = (R[0] - Rr[0]) * x + (R[1] - Rr[1]) * y + (R[2] - Rr[2]) * w + (t[0] - tr[0]);
        const double dy = (R[3] - Rr[3]) * x + (R[4] - Rr[4]) * y + (R[5] - Rr[5]) * w + (t[1] - tr[1]);
        const double dz = (R[6] - Rr[6]) * x + (R[7] - Rr[7]) * y + (R[8] - Rr[8]) * w + (t[2] - tr[2]);
        s += sqrt(dx * dx + dy * dy + dz * dz);
      }
      __syncthreads();                                    // the previous try's readers are done
      part[tid] = s;
      __syncthreads();
      for (int o = JIT_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) part[tid] += part[tid + o];
        __syncthreads();
      }
      const int64_t used = ((int64_t)nv + c.stride - 1) / c.stride;
      e_add = part[0] / (double)used / d;
      rej = c.add_limit >= 0 && e_add > c.add_limit;
    }
    found = !rej;
  }
  if (tid != 0) return;
  if (!found) {
#pragma unroll
    for (int i = 0; i < 9; ++i) Rr[i] = R[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) tr[i] = t[i];
    e_rot = e_trans = e_add = 0.0;
  }
  for (int i = 0; i < 9; ++i) R_ref[9 * (int64_t)n + i] = found ? (float)Rr[i] : Rg[9 * (int64_t)n + i];
  for (int i = 0; i < 3; ++i) t_ref[3 * (int64_t)n + i] = found ? (float)tr[i] : tg[3 * (int64_t)n + i];
  add_err[n] = (found && !with_add) ? NAN : (float)e_add;
  rot_err[n] = (float)(c.fix_swap ? e_rot : e_trans);
  trans_err[n] = (float)(c.fix_swap ? e_trans : e_rot);
  ok[n] = found ? 1 : 0;
  tries[n] = t_used;
}

// --------------------------------------------------------------------------------------------- draws
struct DrawCfg {
  double lo, hi, hsv_ratio[3], hsv_p, noise_p, smooth_p, noise_ratio;
  uint64_t seed;
  int kinds;                 // max_kernel_size / 2 + 1
};

__global__ void patch_draw_kernel(int N, DrawCfg c, int64_t id_base, const int64_t* sample_ids, double* draws, PatchAug* augs) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const uint64_t sid = (uint64_t)(sample_ids ? sample_ids[n] : id_base + n);
  PatchAug a;
  a.sample_id = sid;
  a.ratio = c.lo + (c.hi - c.lo) * scf_rng_uniform(c.seed, sid, SCF_RNG_CROP, 0);
  a.hsv_on = scf_rng_uniform(c.seed, sid, SCF_RNG_GATE_HSV, 0) <= c.hsv_p;
  a.noise_on = scf_rng_uniform(c.seed, sid, SCF_RNG_GATE_NOISE, 0) <= c.noise_p;
  const bool smooth_on = scf_rng_uniform(c.seed, sid, SCF_RNG_GATE_SMOOTH, 0) <= c.smooth_p;
  float g[3];
  for (int i = 0; i < 3; ++i)
    g[i] = (float)((2.0 * scf_rng_uniform(c.seed, sid, SCF_RNG_HSV, i) - 1.0) * c.hsv_ratio[i] + 1.0);
  a.a = g[0]; a.b = g[1]; a.c = g[2];
  a.sigma = scf_rng_uniform(c.seed, sid, SCF_RNG_SIGMA, 0) * c.noise_ratio;
  a.s255 = (float)(a.sigma * 255.0);
  const int idx = min((int)(scf_rng_uniform(c.seed, sid, SCF_RNG_SMOOTH, 0) * (double)c.kinds), c.kinds - 1);
  a.k = smooth_on ? 2 * idx + 1 : 1;
  for (int i = 0; i < 3; ++i) a.reserved[i] = 0;
  augs[n] = a;
  double* o = draws + 8 * (int64_t)n;
  o[0] = a.ratio; o[1] = a.a; o[2] = a.b; o[3] = a.c; o[4] = a.sigma; o[5] = a.k; o[6] = a.hsv_on; o[7] = a.noise_on;
}

// ------------------------------------------------------------------------------------------- extract
struct AugCtx {              // what steps a-c need for one object
  const uint8_t* frame;
  int Hf, Wf, x1, y1, pw, ph;
  int fill[3];
  int hsv_on, noise_on;
  float a, b, c, s255;
  uint64_t seed, sid;
  const int* sdiv;
  const int* hdiv;
};

__device__ __forceinline__ int pt_reflect(int i, int n) {
  if (n == 1) return 0;
  while ((unsigned)i >= (unsigned)n) i = i < 0 ? -i : 2 * n - 2 - i;
  return i;
}

__device__ __forceinline__ int pt_gain(int v, float g, float top) {
  float x = (float)v * g;
  if (g >= 1.f) x = fminf(x, top);
  return (int)x;
}

__device__ __forceinline__ int pt_byte(float x) {
  return (int)fminf(fmaxf(rintf(255.f * x), 0.f), 255.f);
}

// steps a-c for patch pixel (py, px), both inside the patch -> b | g << 8 | r << 16
__device__ __forceinline__ uint32_t pt_aug_pixel(const AugCtx& q, int py, int px) {
  int v[3];
  patch_tap(q.frame, q.Hf, q.Wf, q.y1 + py, q.x1 + px, q.fill, v);
  if (q.hsv_on) {
    const int b = v[0], g = v[1], r = v[2];
    const int vmax = max(b, max(g, r)), vmin = min(b, min(g, r)), diff = vmax - vmin;
    const int vr = vmax == r ? -1 : 0, vg = vmax == g ? -1 : 0;
    const int s = (diff * q.sdiv[vmax] + (1 << 11)) >> 12;
    int h = (vr & (g - b)) + (~vr & ((vg & (b - r + 2 * diff)) + (~vg & (r - g + 4 * diff))));
    h = (h * q.hdiv[diff] + (1 << 11)) >> 12;
    h += h < 0 ? 180 : 0;
    const int H2 = pt_gain(h, q.a, 179.f), S2 = pt_gain(s, q.b, 255.f), V2 = pt_gain(vmax, q.c, 255.f);
    const float sf = (float)S2 * (1.f / 255.f), vf = (float)V2 * (1.f / 255.f);
    const float hh = (float)H2 * (6.f / 180.f);
    const float fl = floorf(hh);
    int sector = (int)fl;
    float f = hh - fl;
    if ((unsigned)sector >= 6u) { sector = 0; f = 0.f; }
    float tab[4];
    tab[0] = vf;
    tab[1] = vf * (1.f - sf);
    tab[2] = vf * (1.f - sf * f);
    tab[3] = vf * (1.f - sf * (1.f - f));
    int ib, ig, ir;
    switch (sector) {
      case 0: ib = 1; ig = 3; ir = 0; break;
      case 1: ib = 1; ig = 0; ir = 2; break;
      case 2: ib = 3; ig = 0; ir = 1; break;
      case 3: ib = 0; ig = 2; ir = 1; break;
      case 4: ib = 0; ig = 1; ir = 3; break;
      default: ib = 2; ig = 1; ir = 0; break;
    }
    float xb = tab[0], xg = tab[0], xr = tab[0];
#pragma unroll
    for (int i = 1; i < 4; ++i) {
      xb = ib == i ? tab[i] : xb;
      xg = ig == i ? tab[i] : xg;
      xr = ir == i ? tab[i] : xr;
    }
    v[0] = pt_byte(xb); v[1] = pt_byte(xg); v[2] = pt_byte(xr);
  }
  if (q.noise_on) {
    const uint64_t key = ((uint64_t)py * (uint64_t)q.pw + (uint64_t)px) * 3ull;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const uint64_t h = scf_rng_hash(q.seed, q.sid, SCF_RNG_NOISE, key + ch);
      const float u1 = (float)scf_rng_u1(h), u2 = (float)scf_rng_u2(h);
      const float z = sqrtf(-2.f * logf(u1)) * cosf(6.2831855f * u2);
      const float x = fminf(fmaxf((float)v[ch] + z * q.s255, 0.f), 255.f);
      v[ch] = (int)x;
    }
  }
  return (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16);
}

// step d for patch pixel (y, x) on the direct route
__device__ __forceinline__ uint32_t pt_blur_direct(const AugCtx& q, int y, int x, int r) {
  if (r == 0) return pt_aug_pixel(q, y, x);
  int s0 = 0, s1 = 0, s2 = 0;
  for (int dy = -r; dy <= r; ++dy) {
    const int yy = pt_reflect(y + dy, q.ph);
    for (int dx = -r; dx <= r; ++dx) {
      const uint32_t w = pt_aug_pixel(q, yy, pt_reflect(x + dx, q.pw));
      s0 += w & 255; s1 += (w >> 8) & 255; s2 += (w >> 16) & 255;
    }
  }
  const int kk = (2 * r + 1) * (2 * r + 1), half = kk >> 1;
  return (uint32_t)((s0 + half) / kk) | ((uint32_t)((s1 + half) / kk) << 8) | ((uint32_t)((s2 + half) / kk) << 16);
}

// items 3, 4 and 6 and the mask for one thread's four columns; LDS: the taps come from the staged, blurred footprint
template <bool VEC, bool LDS>
__device__ __forceinline__ void pt_emit(const AugCtx& q, const PatchRec& rec, const PatchPix& p, const uint32_t* lds, int fy0,
                                        int fx0, int bstride, int r, bool have, int ty, int tx, int tid, int n, int Hf, int Wf,
                                        const uint8_t* masks, int mask_pad, float* out, uint8_t* mask_out) {
  const int pw = q.pw, ph = q.ph;
  const int Y = ty * PT_TH + tid / (PT_TW / 4), X0 = tx * PT_TW + (tid % (PT_TW / 4)) * 4;
  if (Y >= p.H || X0 >= p.W) return;                      // after the last barrier
  const int dy = Y - rec.top;
  const bool row_in = have && dy >= 0 && dy < rec.new_h;
  int iy = 0, b0 = 0, b1 = 0;
  if (row_in) patch_coef(dy, rec.ry, ph, iy, b0, b1);
  const int iy1 = min(iy + 1, ph - 1);
  int my = 0;
  if (row_in && mask_out) my = min((int)floor((double)dy * rec.ry), ph - 1);
  auto column = [&](int j, int* val, int& mv) {
    const int dx = X0 + j - rec.left;
    val[0] = p.pad[0]; val[1] = p.pad[1]; val[2] = p.pad[2];
    mv = mask_pad;
    if (row_in && dx >= 0 && dx < rec.new_w && X0 + j < p.W) {
      int ix, a0, a1;
      patch_coef(dx, rec.rx, pw, ix, a0, a1);
      const int ix1 = min(ix + 1, pw - 1);
      uint32_t t00, t01, t10, t11;
      if constexpr (LDS) {
        const uint32_t* row0 = lds + (iy - fy0) * bstride - fx0;
        const uint32_t* row1 = lds + (iy1 - fy0) * bstride - fx0;
        t00 = row0[ix]; t01 = row0[ix1]; t10 = row1[ix]; t11 = row1[ix1];
      } else {
        t00 = pt_blur_direct(q, iy, ix, r);
        t01 = pt_blur_direct(q, iy, ix1, r);
        t10 = pt_blur_direct(q, iy1, ix, r);
        t11 = pt_blur_direct(q, iy1, ix1, r);
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int sh = 8 * c;
        val[c] = patch_blend((t00 >> sh) & 255, (t01 >> sh) & 255, (t10 >> sh) & 255, (t11 >> sh) & 255, a0, a1, b0, b1);
      }
      if (mask_out) {
        const int mx = min((int)floor((double)dx * rec.rx), pw - 1);
        const int fy = rec.y1 + my, fx = rec.x1 + mx;
        mv = 0;
        if ((unsigned)fy < (unsigned)Hf && (unsigned)fx < (unsigned)Wf)
          mv = masks[((int64_t)n * Hf + fy) * Wf + fx] != 0;
      }
    }
  };
  const int64_t HW = (int64_t)p.H * p.W;
  float* dst = out + (int64_t)n * 3 * HW + (int64_t)Y * p.W + X0;
  uint8_t* md = mask_out ? mask_out + (int64_t)n * HW + (int64_t)Y * p.W + X0 : nullptr;
  if constexpr (!LDS) {                                   // the slow route: one column at a time, scalar stores
    for (int j = 0; j < 4 && X0 + j < p.W; ++j) {
      int val[3], mv;
      column(j, val, mv);
      for (int c = 0; c < 3; ++c) {
        const int oc = p.to_rgb ? 2 - c : c;
        dst[oc * HW + j] = patch_norm(p, val[c], oc);
      }
      if (md) md[j] = (uint8_t)mv;
    }
    return;
  }
  float res[3][4];
  uint8_t mres[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    int val[3], mv;
    column(j, val, mv);
    mres[j] = (uint8_t)mv;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int oc = p.to_rgb ? 2 - c : c;
      res[oc][j] = patch_norm(p, val[c], oc);
    }
  }
  patch_store4<VEC>(p, res, X0, HW, dst);
  if (md) {
    if constexpr (VEC) {
      *reinterpret_cast<uchar4*>(md) = make_uchar4(mres[0], mres[1], mres[2], mres[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (X0 + j < p.W) md[j] = mres[j];
    }
  }
}

template <bool VEC>
__global__ void __launch_bounds__(PT_THREADS) patch_extract_train_kernel(const uint8_t* frames, int F, int Hf, int Wf,
                                                                         const int* frame_index, const uint8_t* masks,
                                                                         const PatchRec* recs, const PatchAug* augs,
                                                                         PatchPix p, int mask_pad, uint64_t seed, float* out,
                                                                         uint8_t* mask_out) {
  extern __shared__ uint32_t lds[];
  __shared__ int sdiv[256], hdiv[256];
  const int n = blockIdx.y, tid = threadIdx.x;
  const int tiles_x = (p.W + PT_TW - 1) / PT_TW;
  const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
  const PatchRec rec = recs[n];
  const PatchAug aug = augs[n];
  const int fi = frame_index[n];
  const bool live = rec.valid && fi >= 0 && fi < F;
  const int pw = rec.x2 - rec.x1 + 1, ph = rec.y2 - rec.y1 + 1;
  const int r = aug.k / 2;
  AugCtx q;
  q.frame = frames + (int64_t)(live ? fi : 0) * Hf * Wf * 3;
  q.Hf = Hf; q.Wf = Wf; q.x1 = rec.x1; q.y1 = rec.y1; q.pw = pw; q.ph = ph;
  q.fill[0] = p.crop_pad[0]; q.fill[1] = p.crop_pad[1]; q.fill[2] = p.crop_pad[2];
  q.hsv_on = aug.hsv_on; q.noise_on = aug.noise_on;
  q.a = aug.a; q.b = aug.b; q.c = aug.c; q.s255 = aug.s255;
  q.seed = seed; q.sid = aug.sample_id;
  q.sdiv = sdiv; q.hdiv = hdiv;
  if (live && aug.hsv_on) {                              // block-uniform: the tables are read by step b alone
    sdiv[tid] = tid ? (int)rint((double)(255 << 12) / (double)tid) : 0;
    hdiv[tid] = tid ? (int)rint((double)(180 << 12) / (6.0 * (double)tid)) : 0;
  }
  __syncthreads();

  // the tile's destination rows / columns inside the resized patch (block-uniform)
  const int dy0 = max(ty * PT_TH - rec.top, 0), dy1 = min(min(ty * PT_TH + PT_TH, p.H) - 1 - rec.top, rec.new_h - 1);
  const int dx0 = max(tx * PT_TW - rec.left, 0), dx1 = min(min(tx * PT_TW + PT_TW, p.W) - 1 - rec.left, rec.new_w - 1);
  const bool have = live && dy0 <= dy1 && dx0 <= dx1;
  int fy0 = 0, fx0 = 0, fh = 0, fw = 0, bstride = 0;
  bool use_lds = false;
  if (have) {
    int i, c0, c1;
    patch_coef(dy0, rec.ry, ph, fy0, c0, c1);
    patch_coef(dy1, rec.ry, ph, i, c0, c1);
    fh = min(i + 1, ph - 1) - fy0 + 1;
    patch_coef(dx0, rec.rx, pw, fx0, c0, c1);
    patch_coef(dx1, rec.rx, pw, i, c0, c1);
    fw = min(i + 1, pw - 1) - fx0 + 1;
    use_lds = pt_route(ph, pw, rec.new_h, rec.new_w, aug.k) == 0 && fh <= pt_cap(ph, rec.new_h, PT_TH) &&
              fw <= pt_cap(pw, rec.new_w, PT_TW);       // the last two always hold (the bound of the header comment)
  }
  if (use_lds) {
    const int ah = fh + 2 * r, aw = fw + 2 * r;
    for (int idx = tid; idx < ah * aw; idx += PT_THREADS) {
      const int ay = idx / aw, ax = idx - ay * aw;
      lds[idx] = pt_aug_pixel(q, pt_reflect(fy0 - r + ay, ph), pt_reflect(fx0 - r + ax, pw));
    }
    __syncthreads();
    bstride = aw;
    if (r) {
      unsigned short* hs = reinterpret_cast<unsigned short*>(lds + ah * aw);
      const int hn = ah * fw;
      for (int idx = tid; idx < hn; idx += PT_THREADS) {
        const int ay = idx / fw, x = idx - ay * fw;
        int s0 = 0, s1 = 0, s2 = 0;
        for (int d = 0; d <= 2 * r; ++d) {
          const uint32_t w = lds[ay * aw + x + d];
          s0 += w & 255; s1 += (w >> 8) & 255; s2 += (w >> 16) & 255;
        }
        hs[idx] = (unsigned short)s0; hs[hn + idx] = (unsigned short)s1; hs[2 * hn + idx] = (unsigned short)s2;
      }
      __syncthreads();
      const int kk = aug.k * aug.k, half = kk >> 1;
      for (int idx = tid; idx < fh * fw; idx += PT_THREADS) {
        const int y = idx / fw, x = idx - y * fw;
        int s0 = 0, s1 = 0, s2 = 0;
        for (int d = 0; d <= 2 * r; ++d) {
          const int j = (y + d) * fw + x;
          s0 += hs[j]; s1 += hs[hn + j]; s2 += hs[2 * hn + j];
        }
        lds[idx] = (uint32_t)((s0 + half) / kk) | ((uint32_t)((s1 + half) / kk) << 8) | ((uint32_t)((s2 + half) / kk) << 16);
      }
      __syncthreads();
      bstride = fw;
    }
  }

  if (use_lds || !have)                                  // a tile of padding alone reads no tap: the vector stores
    pt_emit<VEC, true>(q, rec, p, lds, fy0, fx0, bstride, r, have, ty, tx, tid, n, Hf, Wf, masks, mask_pad, out, mask_out);
  else
    pt_emit<VEC, false>(q, rec, p, lds, fy0, fx0, bstride, r, have, ty, tx, tid, n, Hf, Wf, masks, mask_pad, out, mask_out);
}

// ------------------------------------------------------------------------------------------------ host
static bool unit(double p) { return p >= 0 && p <= 1; }

static bool aug_params_ok(const scf_patch_aug_params* a) {
  if (!a) return false;
  const double* pairs[4] = {a->jitter_angle, a->jitter_x, a->jitter_y, a->jitter_z};
  for (int i = 0; i < 4; ++i)
    if (!isfinite(pairs[i][0]) || !isfinite(pairs[i][1]) || pairs[i][1] < 0) return false;
  if (isnan(a->angle_limit) || isnan(a->translation_limit) || isnan(a->add_limit)) return false;
  if (!(a->size_range[0] > 0) || !(a->size_range[1] >= a->size_range[0]) || !isfinite(a->size_range[1])) return false;
  for (int i = 0; i < 3; ++i)
    if (!(a->hsv_ratio[i] >= 0) || !(a->hsv_ratio[i] < 1)) return false;
  if (!unit(a->hsv_p) || !unit(a->noise_p) || !unit(a->smooth_p)) return false;
  if (!(a->noise_ratio >= 0) || !isfinite(a->noise_ratio)) return false;
  if (a->max_tries < 1 || a->max_tries > 4096) return false;
  if (a->max_kernel_size < 1 || a->max_kernel_size > PT_MAX_K) return false;
  return true;
}

extern "C" int scf_pose_jitter(const scf_mesh_store* mesh, const float* diameters, const int32_t* labels, const float* R_gt,
                               const float* t_gt, int N, int vertex_stride, const scf_patch_aug_params* aug, int64_t id_base,
                               const int64_t* sample_ids, float* R_ref, float* t_ref, float* add_error, float* rot_error,
                               float* trans_error, int32_t* ok, int32_t* tries, scf_stream_t stream) {
  if (!aug_params_ok(aug) || N <= 0 || vertex_stride <= 0) return SCF_EINVAL;
  if (!R_gt || !t_gt || !R_ref || !t_ref || !add_error || !rot_error || !trans_error || !ok || !tries) return SCF_EINVAL;
  if (mesh && (!mesh->verts || !mesh->vert_offset || mesh->num_classes <= 0 || !diameters || !labels)) return SCF_EINVAL;
  if (!mesh && aug->add_limit >= 0) return SCF_EINVAL;
  JitterCfg c;
  for (int i = 0; i < 2; ++i) {
    c.angle[i] = aug->jitter_angle[i]; c.x[i] = aug->jitter_x[i]; c.y[i] = aug->jitter_y[i]; c.z[i] = aug->jitter_z[i];
  }
  c.angle_limit = aug->angle_limit; c.trans_limit = aug->translation_limit; c.add_limit = aug->add_limit;
  c.seed = aug->seed; c.max_tries = aug->max_tries; c.fix_swap = aug->fix_error_swap_quirk != 0; c.stride = vertex_stride;
  scf_launch(pose_jitter_kernel, dim3(N), dim3(JIT_THREADS), 0, scf_stream(stream), mesh ? mesh->verts : (const float*)nullptr,
             mesh ? (const int*)mesh->vert_offset : (const int*)nullptr, mesh ? (int)mesh->num_classes : 0, diameters,
             (const int*)labels, R_gt, t_gt, c, id_base, sample_ids, R_ref, t_ref, add_error, rot_error, trans_error,
             (int*)ok, (int*)tries);
  return scf_launch_status();
}

extern "C" int64_t scf_patch_train_workspace_bytes(int N) {
  if (N <= 0) return SCF_EINVAL;
  return (int64_t)N * (int64_t)(sizeof(PatchRec) + sizeof(PatchAug));
}

extern "C" int scf_patch_train_route(int ph, int pw, int new_h, int new_w, int k) {
  if (ph <= 0 || pw <= 0 || new_h <= 0 || new_w <= 0 || k < 1 || k > PT_MAX_K || k % 2 == 0) return SCF_EINVAL;
  return pt_route(ph, pw, new_h, new_w, k);
}

extern "C" int scf_patch_boxes_train(const scf_mesh_store* mesh, const int32_t* labels, const float* R, const float* t,
                                     const float* K, const int32_t* crop_in, int N, int frame_h, int frame_w,
                                     const scf_patch_params* p, const scf_patch_aug_params* aug, int64_t id_base,
                                     const int64_t* sample_ids, double* draws, float* box, int32_t* crop, float* scale,
                                     float* transform_matrix, float* k, int32_t* valid, void* workspace,
                                     scf_stream_t stream) {
  if (!aug_params_ok(aug) || !patch_params_ok(p) || !draws || !workspace || N <= 0) return SCF_EINVAL;
  DrawCfg c;
  c.lo = aug->size_range[0]; c.hi = aug->size_range[1];
  for (int i = 0; i < 3; ++i) c.hsv_ratio[i] = aug->hsv_ratio[i];
  c.hsv_p = aug->hsv_p; c.noise_p = aug->noise_p; c.smooth_p = aug->smooth_p; c.noise_ratio = aug->noise_ratio;
  c.seed = aug->seed; c.kinds = aug->max_kernel_size / 2 + 1;
  PatchAug* augs = reinterpret_cast<PatchAug*>(static_cast<char*>(workspace) + (int64_t)N * sizeof(PatchRec));
  scf_launch(patch_draw_kernel, dim3((unsigned)scf_cdiv(N, 64)), dim3(64), 0, scf_stream(stream), N, c, id_base, sample_ids,
             draws, augs);
  if (scf_launch_status() != SCF_OK) return SCF_ELAUNCH;
  return scf_patch_boxes_ratio(mesh, labels, R, t, K, crop_in, draws, 8, N, frame_h, frame_w, p, box, crop, scale,
                               transform_matrix, k, valid, workspace, stream);
}

extern "C" int scf_patch_extract_train(const uint8_t* frames, int F, int frame_h, int frame_w, const int32_t* frame_index,
                                       const uint8_t* masks, int N, const void* workspace, const scf_patch_params* p,
                                       const scf_patch_aug_params* aug, float* out, uint8_t* mask_out, scf_stream_t stream) {
  if (!aug_params_ok(aug) || !patch_extract_args_ok(p, frames, frame_index, workspace, out, N, F, frame_h, frame_w)) return SCF_EINVAL;
  if ((masks == nullptr) != (mask_out == nullptr)) return SCF_EINVAL;
  const PatchPix x = patch_pix(p);
  const int64_t tiles = scf_cdiv(p->out_w, PT_TW) * scf_cdiv(p->out_h, PT_TH);
  const dim3 grid((unsigned)tiles, N);
  const PatchRec* recs = static_cast<const PatchRec*>(workspace);
  const PatchAug* augs = reinterpret_cast<const PatchAug*>(static_cast<const char*>(workspace) + (int64_t)N * sizeof(PatchRec));
  const bool vec = p->out_w % 4 == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)mask_out & 3) == 0;
  const int mask_pad = aug->mask_pad_val != 0;
  if (vec)
    scf_launch(patch_extract_train_kernel<true>, grid, dim3(PT_THREADS), PT_LDS_BYTES, scf_stream(stream), frames, F, frame_h,
               frame_w, (const int*)frame_index, masks, recs, augs, x, mask_pad, (uint64_t)aug->seed, out, mask_out);
  else
    scf_launch(patch_extract_train_kernel<false>, grid, dim3(PT_THREADS), PT_LDS_BYTES, scf_stream(stream), frames, F, frame_h,
               frame_w, (const int*)frame_index, masks, recs, augs, x, mask_pad, (uint64_t)aug->seed, out, mask_out);
  return scf_launch_status();
}
