// What patch.hip and patch_train.hip share: the per-object record, items 2, 3 and 5 for one object (patch_finish), the
// resize coefficients, the frame tap and the blend of item 3, item 6 for one value, the three plane stores of four columns,
// and on the host the check of scf_patch_params, of the extract entries' arguments and the PatchPix they launch with.
// patch.hip states the semantics.
#pragma once
#include "scf_common.h"
#include <math.h>

// nothing in this file may fuse a multiplication into an addition: the coordinate and geometry arithmetic is
// compared bit for bit with a restatement that rounds each operation
#pragma clang fp contract(off)

#define PATCH_THREADS 256
#define PATCH_BOX_THREADS 1024
#define PATCH_BOX_WAVES (PATCH_BOX_THREADS / SCF_WAVE)
#define PATCH_MAX_OUT 8192
#define PATCH_MAX_FRAME 16384
#define PATCH_EDGE_LIMIT 536870912.0     // 2^29

struct PatchRec {          // 64 bytes per object
  double rx, ry;           // src / dst per axis: pw / new_w, ph / new_h
  int x1, y1, x2, y2;      // crop rectangle, ends inclusive
  int new_w, new_h, left, top;
  int valid;
  int reserved[3];
};
static_assert(sizeof(PatchRec) == 64, "PatchRec is 64 bytes");

struct PatchGeo {          // what items 2, 3 and 5 read of scf_patch_params
  double aspect, ratio, min_expand;
  int out_h, out_w, resize, stride, keep_ratio, clip_border, fix_quirk, center;
};

struct PatchPix {          // what items 3, 4 and 6 read
  int crop_pad[3], pad[3];
  float mean[3], inv_std[3];
  int to_rgb, H, W;
};

// items 2 (from a box), 3 and 5 for one object; box == nullptr: rect holds a caller-supplied rectangle
static __device__ void patch_finish(const PatchGeo& g, bool ok, const float* box, const int* rect, const float* K, int Hf,
                             int Wf, int* crop, float* scale, float* tm, float* kout, int* valid, PatchRec* rec) {
  int x1 = 0, y1 = 0, x2 = 0, y2 = 0;
  if (ok && box) {
    const float xcf = (box[0] + box[2]) / 2.f, ycf = (box[1] + box[3]) / 2.f;
    const double xc = xcf, yc = ycf;
    double bw = (double)(box[2] - box[0]), bh = (double)(box[3] - box[1]);
    if (!g.keep_ratio) {
      bw = fmax(bw, bh * g.aspect);
      bh = fmax(bw / g.aspect, bh);
    }
    const double sw = bw * g.ratio, sh = bh * g.ratio;
    if (g.min_expand > 0) {
      bw = fmax(bw + 2 * g.min_expand, sw);
      bh = fmax(bh + 2 * g.min_expand, sh);
    } else {
      bw = sw;
      bh = sh;
    }
    double ex1 = xc - bw / 2, ex2 = xc + bw / 2, ey1 = yc - bh / 2;
    double ey2 = ((g.clip_border && !g.fix_quirk) ? (double)box[3] : yc) + bh / 2;
    if (g.clip_border) {
      ex1 = fmin(fmax(ex1, 0.0), (double)Wf);
      ex2 = fmin(fmax(ex2, 0.0), (double)Wf);
      ey1 = fmin(fmax(ey1, 0.0), (double)Hf);
      ey2 = fmin(fmax(ey2, 0.0), (double)Hf);
    }
    ok = fabs(ex1) < PATCH_EDGE_LIMIT && fabs(ex2) < PATCH_EDGE_LIMIT && fabs(ey1) < PATCH_EDGE_LIMIT &&
         fabs(ey2) < PATCH_EDGE_LIMIT;                       // false for NaN and inf too
    if (ok) {
      x1 = (int)ex1; x2 = (int)ex2; y1 = (int)ey1; y2 = (int)ey2;
    }
  } else if (ok) {
    x1 = rect[0]; y1 = rect[1]; x2 = rect[2]; y2 = rect[3];
    ok = x1 > -(int)PATCH_EDGE_LIMIT && y1 > -(int)PATCH_EDGE_LIMIT && x2 < (int)PATCH_EDGE_LIMIT &&
         y2 < (int)PATCH_EDGE_LIMIT;
  }
  ok = ok && x2 >= x1 && y2 >= y1;
  int new_w = 0, new_h = 0, left = 0, top = 0;
  double s = 1.0, rx = 1.0, ry = 1.0;
  if (ok) {
    const int pw = x2 - x1 + 1, ph = y2 - y1 + 1;
    s = (double)g.resize / (double)max(ph, pw);
    new_w = (int)((double)pw * s + 0.5);
    new_h = (int)((double)ph * s + 0.5);
    ok = new_w >= 1 && new_h >= 1 && new_w <= g.out_w && new_h <= g.out_h;
    if (ok) {
      rx = (double)pw / (double)new_w;
      ry = (double)ph / (double)new_h;
      if (g.center) {
        top = (int)((double)g.out_h / 2 - (double)new_h / 2);
        left = (int)((double)g.out_w / 2 - (double)new_w / 2);
      }
    }
  }
  if (!ok) {
    x1 = y1 = x2 = y2 = new_w = new_h = left = top = 0;
    s = rx = ry = 1.0;
  }
  const double tx = ok ? s * (double)(-x1) + (double)left : 0.0;
  const double ty = ok ? s * (double)(-y1) + (double)top : 0.0;
  crop[0] = x1; crop[1] = y1; crop[2] = x2; crop[3] = y2;
  *scale = (float)s;
  *valid = ok ? 1 : 0;
  tm[0] = (float)s; tm[1] = 0.f; tm[2] = (float)tx;
  tm[3] = 0.f; tm[4] = (float)s; tm[5] = (float)ty;
  tm[6] = 0.f; tm[7] = 0.f; tm[8] = 1.f;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double k0 = K[j], k1 = K[3 + j], k2 = K[6 + j];
    kout[j] = (float)(s * k0 + tx * k2);
    kout[3 + j] = (float)(s * k1 + ty * k2);
    kout[6 + j] = K[6 + j];
  }
  rec->rx = rx; rec->ry = ry;
  rec->x1 = x1; rec->y1 = y1; rec->x2 = x2; rec->y2 = y2;
  rec->new_w = new_w; rec->new_h = new_h; rec->left = left; rec->top = top;
  rec->valid = ok ? 1 : 0;
  rec->reserved[0] = rec->reserved[1] = rec->reserved[2] = 0;
}

// one axis of item 3: source index and the two fixed-point coefficients for destination index d
__device__ __forceinline__ void patch_coef(int d, double ratio, int src, int& i, int& a0, int& a1) {
  float f = (float)(((double)d + 0.5) * ratio - 0.5);
  const float fl = floorf(f);
  i = (int)fl;
  f -= fl;
  if (i < 0) { i = 0; f = 0.f; }
  if (i >= src - 1) { i = src - 1; f = 0.f; }
  a0 = (int)rintf((1.f - f) * 2048.f);
  a1 = (int)rintf(f * 2048.f);
}

// pixel (y, x) of the frame, or the crop fill outside it
__device__ __forceinline__ void patch_tap(const uint8_t* frame, int Hf, int Wf, int y, int x, const int* fill, int* o) {
  if ((unsigned)y < (unsigned)Hf && (unsigned)x < (unsigned)Wf) {
    const uint8_t* p = frame + ((int64_t)y * Wf + x) * 3;
    o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
  } else {
    o[0] = fill[0]; o[1] = fill[1]; o[2] = fill[2];
  }
}

// one channel of item 3 from its four taps: the two unshifted horizontal sums, then the vertical pass (one expression:
// with the sums named, the scalar-store patch_extract_kernel takes a VGPR more)
__device__ __forceinline__ int patch_blend(int p00, int p01, int p10, int p11, int a0, int a1, int b0, int b1) {
  return min((((b0 * ((p00 * a0 + p01 * a1) >> 4)) >> 16) + ((b1 * ((p10 * a0 + p11 * a1) >> 4)) >> 16) + 2) >> 2, 255);
}

// item 6 for one value that lands in output channel oc (the channel loop around it stays in the kernels: behind a call
// patch_extract_kernel takes two SGPRs more)
__device__ __forceinline__ float patch_norm(const PatchPix& p, int v, int oc) { return ((float)v - p.mean[oc]) * p.inv_std[oc]; }

// the three plane stores of four consecutive columns from X0, res[output channel][column]; dst: column X0 of the row in
// plane 0
template <bool VEC>
__device__ __forceinline__ void patch_store4(const PatchPix& p, const float (&res)[3][4], int X0, int64_t HW, float* dst) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if constexpr (VEC) {
      *reinterpret_cast<float4*>(dst + c * HW) = make_float4(res[c][0], res[c][1], res[c][2], res[c][3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (X0 + j < p.W) dst[c * HW + j] = res[c][j];
    }
  }
}

static bool patch_params_ok(const scf_patch_params* p) {
  if (!p) return false;
  if (p->out_h <= 0 || p->out_w <= 0 || p->out_h > PATCH_MAX_OUT || p->out_w > PATCH_MAX_OUT) return false;
  if (p->resize <= 0 || p->resize > p->out_h || p->resize > p->out_w) return false;
  if (p->vertex_stride <= 0) return false;
  if (!(p->aspect_ratio > 0) || !(p->size_ratio > 0) || !(p->min_expand >= 0)) return false;
  if (!isfinite(p->aspect_ratio) || !isfinite(p->size_ratio) || !isfinite(p->min_expand)) return false;
  for (int c = 0; c < 3; ++c) {
    if (p->crop_pad_val[c] < 0 || p->crop_pad_val[c] > 255 || p->pad_val[c] < 0 || p->pad_val[c] > 255) return false;
    if (!isfinite(p->mean[c]) || !isfinite(p->std[c]) || !(p->std[c] != 0.f)) return false;
  }
  return true;
}

// what scf_patch_extract and scf_patch_extract_train check alike
static bool patch_extract_args_ok(const scf_patch_params* p, const void* frames, const void* frame_index, const void* workspace,
                                  const void* out, int N, int F, int frame_h, int frame_w) {
  if (!patch_params_ok(p) || !frames || !frame_index || !workspace || !out) return false;
  if (N <= 0 || N > 65535 || F <= 0) return false;
  return frame_h > 0 && frame_w > 0 && frame_h <= PATCH_MAX_FRAME && frame_w <= PATCH_MAX_FRAME;
}

static PatchPix patch_pix(const scf_patch_params* p) {
  PatchPix x;
  for (int c = 0; c < 3; ++c) {
    x.crop_pad[c] = p->crop_pad_val[c];
    x.pad[c] = p->pad_val[c];
    x.mean[c] = p->mean[c];
    x.inv_std[c] = (float)(1.0 / (double)p->std[c]);
  }
  x.to_rgb = p->to_rgb != 0;
  x.H = p->out_h;
  x.W = p->out_w;
  return x;
}


// patch.hip: scf_patch_boxes with an optional per-object size ratio read on the device (not part of the C ABI)
int scf_patch_boxes_ratio(const scf_mesh_store* mesh, const int32_t* labels, const float* R, const float* t,
                          const float* K, const int32_t* crop_in, const double* ratios, int ratio_stride, int N,
                          int frame_h, int frame_w, const scf_patch_params* p, float* box, int32_t* crop, float* scale,
                          float* transform_matrix, float* k, int32_t* valid, void* workspace, scf_stream_t stream);
