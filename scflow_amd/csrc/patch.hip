// Object patches from full frames for gfx950: box, crop, resize, pad, intrinsics and normalisation, batched over
// objects.  It restates the val_pipeline of configs/refine_datasets/ycbv_*.py, which the reference runs object by
// object on the CPU through cv2 / mmcv 1.3.16:
//   ComputeBbox -> Crop(size_range=(r, r), clip_border, pad_val) -> Resize(S, keep_ratio=True) ->
//   Pad((H, W), center, pad_val) -> RemapPose(keep_intrinsic=False) ('adapt_intrinsic') -> Normalize(mean, std, to_rgb)
// (datasets/pipelines/formatting.py:41-90, geometry_transform.py:155-500, datasets/pose.py:18-66; mmcv's imcrop,
// imrescale / rescale_size, impad, imnormalize).  Neither cv2 nor mmcv is used or needed; the semantics below are the
// contract, and tests/test_patches_host.py restates them in numpy (patch_reference), bit for bit.
//
// 1. Box.  For object n with class labels[n], every vertex_stride-th vertex X of the class (all of them at 1):
//      X_c = R X + t,  p = K X_c (the full 3 x 3 product),  u = p.x / (p.z + 1e-8),  v = p.y / (p.z + 1e-8)
//    in fp32, every multiplication and addition separately rounded (no fused multiply-add in this file).  The box is
//    (min u, min v, max u, max v), fp32 values.  The reference draws 1000 random vertices per mesh at construction;
//    taking every (vertex_stride-th) vertex is the deterministic stand-in, so its boxes are supersets of the
//    reference's on the same mesh.  An object is INVALID when its label is outside [0, num_classes), its class mesh
//    is empty, any used vertex has p.z <= 0 (or NaN), or the box is not finite.
// 2. Crop rectangle.  xc = (x1 + x2) / 2, yc = (y1 + y2) / 2, bw = x2 - x1, bh = y2 - y1 in fp32 from the fp32 box;
//    everything after that in fp64.  Without keep_ratio: bw = max(bw, bh * aspect), then bh = max(bw / aspect, bh).
//    Both are scaled by size_ratio; with min_expand > 0 each becomes max(old + 2 min_expand, scaled).
//      clip_border = 0:  crop_x1 = trunc(xc - bw/2), crop_x2 = trunc(xc + bw/2), y likewise (trunc: toward zero)
//      clip_border = 1:  the four edges are clipped to [0, Wf] / [0, Hf] before truncation, and the lower edge is
//                        y2 + bh/2 with y2 the BOX's lower edge, as geometry_transform.py:251 writes it;
//                        fix_clip_border_quirk != 0 uses yc + bh/2 instead.
//    The patch is (crop_y2 - crop_y1 + 1) x (crop_x2 - crop_x1 + 1), ends inclusive; pixels outside the frame are
//    crop_pad_val.  A rectangle wholly outside the frame gives an all-crop_pad_val patch (mmcv's imcrop clips such a
//    rectangle to the frame's first or last row / column and pastes that sliver instead; not reproduced).  An edge
//    that is not finite or not within +-2^29 makes the object invalid.  Caller-supplied rectangles (crop_in) enter
//    here in place of items 1 and 2; one with x2 < x1 or y2 < y1 is invalid.
// 3. Resize.  s = S / max(ph, pw) in fp64; new_w = int(pw s + 0.5), new_h = int(ph s + 0.5); an object whose new_w or
//    new_h is 0 is invalid (cv2.resize raises there).  Interpolation is OpenCV's generic 8-bit INTER_LINEAR: per axis,
//    for destination index d,
//      f = float32((d + 0.5) (src / dst) - 0.5)        quotient, product and difference in fp64, separately rounded
//      i = floor(f), f -= i;  i < 0: i = 0, f = 0;  i >= src - 1: i = src - 1, f = 0
//      a0 = rint((1 - f) 2048), a1 = rint(f 2048)      fp32, ties to even
//    the horizontal sums S0 = p(i_y, i_x) a0 + p(i_y, i_x + 1) a1 and S1 (row i_y + 1) stay unshifted integers, and
//      value = (((b0 (S0 >> 4)) >> 16) + ((b1 (S1 >> 4)) >> 16) + 2) >> 2.
//    (cv2 forms the ratio as 1 / (dst / src), which may differ from src / dst in the last bit; with cv2 absent that is
//    unverified, and the form above is the contract.)
// 4. Pad to (H, W) with pad_val per channel.  center: top = int(H/2 - new_h/2), left = int(W/2 - new_w/2); else 0, 0.
// 5. Intrinsics.  transform_matrix = P S C with C the translation by (-crop_x1, -crop_y1), S = diag(s, s, 1), P the
//    translation by (left, top), i.e. [[s, 0, left - s crop_x1], [0, s, top - s crop_y1], [0, 0, 1]];
//    k = transform_matrix K.  Both in fp64 from the fp32 K, rounded once to fp32.  Poses pass through
//    ('adapt_intrinsic'); ori_k = K.
// 6. Normalize.  The frame is read as BGR; to_rgb swaps channels 0 and 2.  out = (float32(value) - mean_c)
//    float32(1.0 / std_c) with c the OUTPUT channel, written NCHW.  crop_pad_val and pad_val are indexed by the
//    FRAME's channel order.  An invalid object gets an all-pad_val patch (normalised), valid = 0, crop rectangle 0,
//    scale 1, an identity transform_matrix and k = K: the kernels cannot raise.  A frame_index outside [0, F) also
//    gives an all-pad_val patch.
//
// Layout (no atomics, nothing through the host):
//   patch_box_kernel      one workgroup of 1024 threads per object: fp32 projection of the class's vertices (the
//                         scf_mesh_store layout), min / max through wave shuffles and LDS, then thread 0 does items
//                         2, 3 and 5 and writes a 64-byte record.
//   patch_extract_kernel  reads the record; one thread per four consecutive output columns of one row, so the three
//                         plane stores of a wave are contiguous 16-byte stores (1 KiB per instruction); every output
//                         pixel is written once.  The taps are plain byte loads of the HWC frame: neighbouring
//                         pixels share cache lines and the frame stays in L2.  The job is bound by the fp32 store.
#include "patch_common.h"

__device__ __forceinline__ float wave_min(float v) {
  for (int o = SCF_WAVE / 2; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
  for (int o = SCF_WAVE / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// ------------------------------------------------------------------------------------------------- box
__global__ void __launch_bounds__(PATCH_BOX_THREADS) patch_box_kernel(const float* verts, const int* vert_offset,
                                                                  int num_classes, const int* labels, const float* Rs,
                                                                  const float* ts, const float* Ks, const int* crop_in,
                                                                  const double* ratios, int ratio_stride, int Hf, int Wf,
                                                                  PatchGeo g, float* box_out, int* crop,
                                                                  float* scale, float* tm, float* kout, int* valid,
                                                                  PatchRec* recs) {
  __shared__ float part[4][PATCH_BOX_WAVES];
  const int n = blockIdx.x, tid = threadIdx.x;
  const float* K = Ks + 9 * (int64_t)n;
  if (ratios) g.ratio = ratios[(int64_t)n * ratio_stride];   // the train pipeline's per-object Crop ratio (patch_train.hip)
  if (crop_in) {                                       // caller-supplied rectangle: items 3 and 5 only
    if (tid < 4 && box_out) box_out[4 * (int64_t)n + tid] = 0.f;
    if (tid == 0)
      patch_finish(g, true, nullptr, crop_in + 4 * (int64_t)n, K, Hf, Wf, crop + 4 * (int64_t)n, scale + n,
                   tm + 9 * (int64_t)n, kout + 9 * (int64_t)n, valid + n, recs + n);
    return;
  }
  int vbase = 0, nv = 0;
  const int l = labels[n];
  if (l >= 0 && l < num_classes) {
    vbase = vert_offset[l];
    nv = max(vert_offset[l + 1] - vbase, 0);
  }
  const float* R = Rs + 9 * (int64_t)n;
  const float* t = ts + 3 * (int64_t)n;
  float r[9], k[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) { r[i] = R[i]; k[i] = K[i]; }
  const float t0 = t[0], t1 = t[1], t2 = t[2];
  float umin = INFINITY, umax = -INFINITY, vmin = INFINITY, vmax = -INFINITY;
  int bad = 0;
  for (int64_t i = (int64_t)tid * g.stride; i < nv; i += (int64_t)PATCH_BOX_THREADS * g.stride) {
    const float* X = verts + 3 * (vbase + i);
    const float x = X[0], y = X[1], z = X[2];
    const float cx = r[0] * x + r[1] * y + r[2] * z + t0;
    const float cy = r[3] * x + r[4] * y + r[5] * z + t1;
    const float cz = r[6] * x + r[7] * y + r[8] * z + t2;
    const float px = k[0] * cx + k[1] * cy + k[2] * cz;
    const float py = k[3] * cx + k[4] * cy + k[5] * cz;
    const float pz = k[6] * cx + k[7] * cy + k[8] * cz;
    if (!(pz > 0.f)) bad = 1;
    const float u = px / (pz + 1e-8f), v = py / (pz + 1e-8f);
    umin = fminf(umin, u); umax = fmaxf(umax, u);
    vmin = fminf(vmin, v); vmax = fmaxf(vmax, v);
  }
  bad = __syncthreads_or(bad);
  umin = wave_min(umin); vmin = wave_min(vmin); umax = wave_max(umax); vmax = wave_max(vmax);
  if ((tid & (SCF_WAVE - 1)) == 0) {
    const int w = tid / SCF_WAVE;
    part[0][w] = umin; part[1][w] = vmin; part[2][w] = umax; part[3][w] = vmax;
  }
  __syncthreads();
  if (tid != 0) return;
  float box[4] = {part[0][0], part[1][0], part[2][0], part[3][0]};
  for (int w = 1; w < PATCH_BOX_WAVES; ++w) {
    box[0] = fminf(box[0], part[0][w]); box[1] = fminf(box[1], part[1][w]);
    box[2] = fmaxf(box[2], part[2][w]); box[3] = fmaxf(box[3], part[3][w]);
  }
  const bool ok = nv > 0 && !bad && isfinite(box[0]) && isfinite(box[1]) && isfinite(box[2]) && isfinite(box[3]);
  if (box_out)
    for (int j = 0; j < 4; ++j) box_out[4 * (int64_t)n + j] = ok ? box[j] : 0.f;
  patch_finish(g, ok, box, nullptr, K, Hf, Wf, crop + 4 * (int64_t)n, scale + n, tm + 9 * (int64_t)n,
               kout + 9 * (int64_t)n, valid + n, recs + n);
}

// --------------------------------------------------------------------------------------------- extract
template <bool VEC>
__global__ void __launch_bounds__(PATCH_THREADS) patch_extract_kernel(const uint8_t* frames, int F, int Hf, int Wf,
                                                                      const int* frame_index, const PatchRec* recs,
                                                                      PatchPix p, float* out) {
  const int n = blockIdx.y;
  const int groups = (p.W + 3) / 4;
  const int64_t id = (int64_t)blockIdx.x * PATCH_THREADS + threadIdx.x;
  if (id >= (int64_t)groups * p.H) return;
  const int Y = (int)(id / groups), X0 = (int)(id % groups) * 4;
  const PatchRec rec = recs[n];
  const int fi = frame_index[n];
  const bool live = rec.valid && fi >= 0 && fi < F;
  const uint8_t* frame = frames + (int64_t)(live ? fi : 0) * Hf * Wf * 3;
  const int pw = rec.x2 - rec.x1 + 1, ph = rec.y2 - rec.y1 + 1;
  const int dy = Y - rec.top;
  const bool row_in = live && dy >= 0 && dy < rec.new_h;
  int iy = 0, b0 = 0, b1 = 0;
  if (row_in) patch_coef(dy, rec.ry, ph, iy, b0, b1);
  const int iy1 = min(iy + 1, ph - 1);
  float res[3][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int dx = X0 + j - rec.left;
    int val[3] = {p.pad[0], p.pad[1], p.pad[2]};
    if (row_in && dx >= 0 && dx < rec.new_w && X0 + j < p.W) {
      int ix, a0, a1;
      patch_coef(dx, rec.rx, pw, ix, a0, a1);
      const int ix1 = min(ix + 1, pw - 1);
      int t00[3], t01[3], t10[3], t11[3];
      patch_tap(frame, Hf, Wf, rec.y1 + iy, rec.x1 + ix, p.crop_pad, t00);
      patch_tap(frame, Hf, Wf, rec.y1 + iy, rec.x1 + ix1, p.crop_pad, t01);
      patch_tap(frame, Hf, Wf, rec.y1 + iy1, rec.x1 + ix, p.crop_pad, t10);
      patch_tap(frame, Hf, Wf, rec.y1 + iy1, rec.x1 + ix1, p.crop_pad, t11);
#pragma unroll
      for (int c = 0; c < 3; ++c) val[c] = patch_blend(t00[c], t01[c], t10[c], t11[c], a0, a1, b0, b1);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int oc = p.to_rgb ? 2 - c : c;
      res[oc][j] = patch_norm(p, val[c], oc);
    }
  }
  const int64_t HW = (int64_t)p.H * p.W;
  patch_store4<VEC>(p, res, X0, HW, out + (int64_t)n * 3 * HW + (int64_t)Y * p.W + X0);
}

// ------------------------------------------------------------------------------------------------ host
extern "C" int64_t scf_patch_workspace_bytes(int N) {
  if (N <= 0) return SCF_EINVAL;
  return (int64_t)N * (int64_t)sizeof(PatchRec);
}

// scf_patch_boxes with an optional per-object size ratio on the device (ratios[n * ratio_stride], fp64; nullptr: p->size_ratio
// for every object).  scf_patch_boxes_train (patch_train.hip) enters here; declared in patch_common.h.
int scf_patch_boxes_ratio(const scf_mesh_store* mesh, const int32_t* labels, const float* R, const float* t,
                          const float* K, const int32_t* crop_in, const double* ratios, int ratio_stride, int N,
                          int frame_h, int frame_w, const scf_patch_params* p, float* box, int32_t* crop, float* scale,
                          float* transform_matrix, float* k, int32_t* valid, void* workspace, scf_stream_t stream) {
  if (!patch_params_ok(p) || !K || !crop || !scale || !transform_matrix || !k || !valid || !workspace) return SCF_EINVAL;
  if (N <= 0 || frame_h <= 0 || frame_w <= 0 || frame_h > PATCH_MAX_FRAME || frame_w > PATCH_MAX_FRAME) return SCF_EINVAL;
  if (!crop_in) {
    if (!mesh || !labels || !R || !t) return SCF_EINVAL;
    if (!mesh->verts || !mesh->vert_offset || mesh->num_classes <= 0) return SCF_EINVAL;
  }
  PatchGeo g{p->aspect_ratio, p->size_ratio, p->min_expand, p->out_h, p->out_w, p->resize, p->vertex_stride,
             p->keep_ratio != 0, p->clip_border != 0, p->fix_clip_border_quirk != 0, p->center != 0};
  scf_launch(patch_box_kernel, dim3(N), dim3(PATCH_BOX_THREADS), 0, scf_stream(stream),
             crop_in ? (const float*)nullptr : mesh->verts, crop_in ? (const int*)nullptr : (const int*)mesh->vert_offset,
             crop_in ? 0 : (int)mesh->num_classes, (const int*)labels, R, t, K, (const int*)crop_in, ratios, ratio_stride, frame_h, frame_w, g,
             box, (int*)crop, scale, transform_matrix, k, (int*)valid, (PatchRec*)workspace);
  return scf_launch_status();
}

extern "C" int scf_patch_boxes(const scf_mesh_store* mesh, const int32_t* labels, const float* R, const float* t,
                               const float* K, const int32_t* crop_in, int N, int frame_h, int frame_w,
                               const scf_patch_params* p, float* box, int32_t* crop, float* scale,
                               float* transform_matrix, float* k, int32_t* valid, void* workspace,
                               scf_stream_t stream) {
  return scf_patch_boxes_ratio(mesh, labels, R, t, K, crop_in, nullptr, 0, N, frame_h, frame_w, p, box, crop, scale,
                               transform_matrix, k, valid, workspace, stream);
}

extern "C" int scf_patch_extract(const uint8_t* frames, int F, int frame_h, int frame_w, const int32_t* frame_index,
                                 int N, const void* workspace, const scf_patch_params* p, float* out,
                                 scf_stream_t stream) {
  if (!patch_extract_args_ok(p, frames, frame_index, workspace, out, N, F, frame_h, frame_w)) return SCF_EINVAL;
  const PatchPix x = patch_pix(p);
  const int64_t threads = (int64_t)((p->out_w + 3) / 4) * p->out_h;
  const dim3 grid((unsigned)scf_cdiv(threads, PATCH_THREADS), N);
  const bool vec = p->out_w % 4 == 0 && ((uintptr_t)out & 15) == 0;
  if (vec)
    scf_launch(patch_extract_kernel<true>, grid, dim3(PATCH_THREADS), 0, scf_stream(stream), frames, F, frame_h, frame_w,
               (const int*)frame_index, (const PatchRec*)workspace, x, out);
  else
    scf_launch(patch_extract_kernel<false>, grid, dim3(PATCH_THREADS), 0, scf_stream(stream), frames, F, frame_h, frame_w,
               (const int*)frame_index, (const PatchRec*)workspace, x, out);
  return scf_launch_status();
}
