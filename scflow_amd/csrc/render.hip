// Mesh renderer for gfx950: hard z-buffer rasterisation (one face per pixel) and Phong shading, batched over
// samples.  It restates what Renderer.forward (models/utils/rendering.py) asks pytorch3d for under the shipped
// configuration (configs/refine_datasets/ycbv_real.py:148-164): shader_type='Phong', soft_blending=False,
// faces_per_pixel=1, blur_radius=0, render_mask=False, background (.5, .5, .5).  No pytorch3d bit parity is
// claimed; the semantics below are the contract.
//
// Camera.  OpenCV R, t, K per sample: X_c = R X + t, u = fx X_c.x / X_c.z + cx, v = fy X_c.y / X_c.z + cy (K's
// skew entry is not read, as in cameras_from_opencv_projection).  The z-buffer holds X_c.z; znear / zfar play no
// part in hard rasterisation and are not computed.
//
// Pixel sampling points.  cameras_from_opencv_projection maps u to NDC with scale = (S-1)/2, c0 = (W-1)/2
// (S = min(H, W)), and pytorch3d samples pixel centres on a flipped non-square NDC grid (PixToNonSquareNdc):
// column c sits at x_ndc = (W - 2c - 1) / S.  Hence output column c samples
//   u(c) = (W-1)/2 - (S-1)(W-2c-1)/(2S)        (256 x 256: u(c) = c 255/256 + 255/512, not u = c)
// and row r samples v(r) by the same formula with H.  pixel_coord() is that formula, shared with the host entry
// scf_render_pixel_coord.  Both axes are flipped, an orientation-preserving map, so screen barycentrics taken in
// the (u, v) plane equal pytorch3d's NDC ones.
//
// Coverage.  A pixel is covered by a face when all three screen barycentrics of its sampling point are >= 0
// (edge functions evaluated with each edge's endpoints in a canonical order, so that two faces sharing an edge
// leave no crack between them).
// Faces of zero (or non-finite) screen area, faces whose three vertices all have z <= 0 and faces with a vertex
// index outside their mesh are skipped; a hit whose perspective-correct z is <= 0 (or not finite) is discarded.
// Back faces are not culled (pytorch3d's default).
//
// Depth test.  z = 1 / (b0/z0 + b1/z1 + b2/z2), i.e. 1/z interpolated linearly in screen space (exact on the
// face's plane).  The hit is the lexicographic minimum of (z, face index).  Every pixel evaluates every face of its
// sample and nothing depends on the other samples of the batch, so results are deterministic and a sample gives
// the same bits alone or in any batch.
//
// Outputs.  zbuf = z of the hit or -1 (pytorch3d's background value); pix_to_face = the face index within the
// sample's own mesh or -1 (pytorch3d returns an index into the packed batch); RGBA (alpha = covered) and / or
// NCHW RGB through a per-channel (x - mean) / std, the normalisation BaseRefiner.format_data_test applies.
//
// Shading: pytorch3d's phong_shading followed by hard_rgb_blend, in the object (world) frame, with the
// perspective-correct barycentrics B_i = (b_i/z_i) / sum_j (b_j/z_j).  Position p, vertex normal n and vertex
// colour (TexturesVertex, in [0, 1]) are interpolated; normalisation is x / max(|x|, 1e-6);
//   colour = (ambient + diffuse) * texel + specular
//   ambient = a_L,  diffuse = d_L relu(n.l),  specular = s_L (relu(v.(2 (n.l) n - l)) [n.l > 0])^64
//   l = light - p,  v = cam - p,  cam = -R^T t;  material colours 1, shininess 64.
// Light colours: default_lights -> pytorch3d PointLights defaults (ambient .5, diffuse .3, specular .2), otherwise
// ambient .8, diffuse .5, specular 1.  Light location, as rendering.py:191-207 writes it:
//   seperate_lights:                   R (0, 0, max(zmin_n - 400, 0)), zmin_n = min camera z over sample n's vertices
//   not seperate, default_lights:      (0, 1, 0)
//   not seperate, not default_lights:  R (0, 0, znear / 4), znear = floor(min_n zmin_n / 100) 100 over the batch
// Background pixels get background_color.  Vertex normals are whatever the mesh store holds (scflow_amd/mesh.py:
// the PLY's nx ny nz when present, else the normalised area-weighted sum of face normals).
//
// Precision.  Projections, barycentrics, depth and shading are fp64.  The face records the rasteriser streams
// are fp32 (projected vertices, 1/z); the winner of each pixel is re-projected from the fp32 inputs in fp64 for
// the depth it reports and for shading, so only the coverage decision sees the fp32 record (an error of about
// 1e-5 px at 256 px).
//
// Layout (no global atomics):
//   render_zmin_kernel    one workgroup per sample: min camera z over the sample's vertices (only when a light
//                         position needs it).
//   render_setup_kernel   one thread per (sample, face): the fp32 record and a pixel bounding box clipped to the
//                         image (int16 x4, empty = (32767, -1)).
//   render_raster_kernel  one workgroup of 256 threads per (sample, 16 x 16 pixel tile), one pixel per thread.  The
//                         sample's faces stream through in chunks of 256: each thread tests one face's box against
//                         the tile, the overlapping ones are compacted IN ORDER into LDS (ballot + popcount per
//                         wave, wave offsets through LDS), then every pixel tests them against its best (z, face)
//                         kept in registers.  The winner is shaded and written straight to the output planes.
#include "scf_common.h"
#include <math.h>

#define RENDER_TILE 16
#define RENDER_THREADS (RENDER_TILE * RENDER_TILE)
#define RENDER_WAVES (RENDER_THREADS / SCF_WAVE)
#define RENDER_MAX_SIZE 8192

// image-plane coordinate sampled by pixel `i` along an axis of `size` pixels; `smin` = min(H, W)
__host__ __device__ __forceinline__ double pixel_coord(int i, int size, int smin) {
  return 0.5 * (size - 1) - (double)(smin - 1) * (double)(size - 2 * i - 1) / (2.0 * smin);
}

struct MeshArgs {
  const float* verts;
  const float* normals;
  const float* colors;
  const int* faces;
  const int* vert_offset;
  const int* face_offset;
  int num_classes;
  int max_faces;
};

// the sample's mesh: vertex base / count and face base / count; an out-of-range label is the empty mesh
__device__ __forceinline__ void sample_mesh(const MeshArgs& m, const int* labels, int n, int& vbase, int& nv,
                                            int& fbase, int& nf) {
  const int l = labels[n];
  vbase = nv = fbase = nf = 0;
  if (l < 0 || l >= m.num_classes) return;
  vbase = m.vert_offset[l];
  nv = m.vert_offset[l + 1] - vbase;
  fbase = m.face_offset[l];
  nf = min(m.face_offset[l + 1] - fbase, m.max_faces);
  if (nv < 0 || nf < 0) nv = nf = 0;
}

__device__ __forceinline__ void cam_point(const float* R, const float* t, const float* X, double* c) {
  const double x = X[0], y = X[1], z = X[2];
#pragma unroll
  for (int i = 0; i < 3; ++i) c[i] = (double)R[3 * i] * x + (double)R[3 * i + 1] * y + (double)R[3 * i + 2] * z + (double)t[i];
}

// ------------------------------------------------------------------------------------------------ zmin
__global__ void __launch_bounds__(RENDER_THREADS) render_zmin_kernel(MeshArgs m, const int* labels, const float* Rs,
                                                                     const float* ts, double* zmin) {
  __shared__ double part[RENDER_WAVES];
  const int n = blockIdx.x;
  int vbase, nv, fbase, nf;
  sample_mesh(m, labels, n, vbase, nv, fbase, nf);
  const float* R = Rs + 9 * (int64_t)n;
  const float* t = ts + 3 * (int64_t)n;
  double z = INFINITY;
  for (int i = threadIdx.x; i < nv; i += RENDER_THREADS) {
    double c[3];
    cam_point(R, t, m.verts + 3 * (int64_t)(vbase + i), c);
    z = fmin(z, c[2]);
  }
  for (int o = SCF_WAVE / 2; o > 0; o >>= 1) z = fmin(z, __shfl_xor(z, o));
  if ((threadIdx.x & (SCF_WAVE - 1)) == 0) part[threadIdx.x / SCF_WAVE] = z;
  __syncthreads();
  if (threadIdx.x == 0) {
    double r = part[0];
    for (int w = 1; w < RENDER_WAVES; ++w) r = fmin(r, part[w]);
    zmin[n] = r;
  }
}

// ----------------------------------------------------------------------------------------------- setup
// column range [lo, hi] whose sampling points can fall in [a, b] (widened by one pixel: the box only culls, the
// barycentric test decides); NaN bounds open the range to the whole axis
__device__ __forceinline__ void pixel_range(double a, double b, int size, int smin, int& lo, int& hi) {
  const double c0 = 0.5 * (size - 1) - (double)(smin - 1) * (double)(size - 1) / (2.0 * smin);  // u(0)
  const double step = (double)(smin - 1) / (double)smin;                                        // u(c+1) - u(c)
  double l = step > 0 ? floor((a - c0) / step) - 1 : -1.0;
  double h = step > 0 ? ceil((b - c0) / step) + 1 : (double)size;
  l = fmax(l, -1.0);                 // fmax / fmin return the other operand for a NaN
  h = fmin(h, (double)size);
  lo = max((int)l, 0);
  hi = min((int)h, size - 1);
}

__global__ void __launch_bounds__(256) render_setup_kernel(MeshArgs m, const int* labels, const float* Rs,
                                                           const float* ts, const float* Ks, int H, int W,
                                                           short4* boxes, float4* recs) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  const int n = blockIdx.y;
  if (f >= m.max_faces) return;
  const int64_t slot = (int64_t)n * m.max_faces + f;
  const short4 empty = make_short4(32767, -1, 32767, -1);
  int vbase, nv, fbase, nf;
  sample_mesh(m, labels, n, vbase, nv, fbase, nf);
  if (f >= nf) { boxes[slot] = empty; return; }
  const int* fi = m.faces + 3 * (int64_t)(fbase + f);
  const int i0 = fi[0], i1 = fi[1], i2 = fi[2];
  if (i0 < 0 || i0 >= nv || i1 < 0 || i1 >= nv || i2 < 0 || i2 >= nv) { boxes[slot] = empty; return; }
  const float* R = Rs + 9 * (int64_t)n;
  const float* t = ts + 3 * (int64_t)n;
  const float* K = Ks + 9 * (int64_t)n;
  double c[3][3];
  cam_point(R, t, m.verts + 3 * (int64_t)(vbase + i0), c[0]);
  cam_point(R, t, m.verts + 3 * (int64_t)(vbase + i1), c[1]);
  cam_point(R, t, m.verts + 3 * (int64_t)(vbase + i2), c[2]);
  if (c[0][2] <= 0 && c[1][2] <= 0 && c[2][2] <= 0) { boxes[slot] = empty; return; }
  const double fx = K[0], cx = K[2], fy = K[4], cy = K[5];
  float u[3], v[3], iz[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    u[k] = (float)(fx * c[k][0] / c[k][2] + cx);
    v[k] = (float)(fy * c[k][1] / c[k][2] + cy);
    iz[k] = (float)(1.0 / c[k][2]);
  }
  // the area the rasteriser will see (fp32 record, fp64 arithmetic)
  const double area = ((double)u[2] - u[0]) * ((double)v[1] - v[0]) - ((double)v[2] - v[0]) * ((double)u[1] - u[0]);
  if (!(area != 0.0) || !isfinite(area)) { boxes[slot] = empty; return; }
  const int smin = min(H, W);
  int c0, c1, r0, r1;
  pixel_range(fmin(fmin((double)u[0], (double)u[1]), (double)u[2]), fmax(fmax((double)u[0], (double)u[1]), (double)u[2]),
              W, smin, c0, c1);
  pixel_range(fmin(fmin((double)v[0], (double)v[1]), (double)v[2]), fmax(fmax((double)v[0], (double)v[1]), (double)v[2]),
              H, smin, r0, r1);
  if (c0 > c1 || r0 > r1) { boxes[slot] = empty; return; }
  boxes[slot] = make_short4((short)c0, (short)c1, (short)r0, (short)r1);
  float4* r = recs + 3 * slot;
  r[0] = make_float4(u[0], v[0], u[1], v[1]);
  r[1] = make_float4(u[2], v[2], iz[0], iz[1]);
  r[2] = make_float4(iz[2], area > 0 ? 1.f : -1.f, 0.f, 0.f);
}

// ---------------------------------------------------------------------------------------------- raster
struct RenderOut {
  float* zbuf;
  int* p2f;
  float* rgba;
  float* rgb;
  float bg[3], mean[3], stdv[3];
  int default_lights, seperate_lights;
};

// edge function (p - a) x (b - a), evaluated with the endpoints in a canonical order: the two faces sharing an edge
// get exactly opposite values, so a sampling point on a shared edge is never missed by both (no cracks)
__device__ __forceinline__ double edge_fn(double au, double av, double bu, double bv, double x, double y) {
  if (au > bu || (au == bu && av > bv)) return -((x - bu) * (av - bv) - (y - bv) * (au - bu));
  return (x - au) * (bv - av) - (y - av) * (bu - au);
}

__device__ __forceinline__ void normalize3(double* a) {
  const double l = fmax(sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]), 1e-6);
  a[0] /= l; a[1] /= l; a[2] /= l;
}

__global__ void __launch_bounds__(RENDER_THREADS) render_raster_kernel(MeshArgs m, const int* labels, const float* Rs,
                                                                       const float* ts, const float* Ks, int N, int H,
                                                                       int W, const short4* boxes, const float4* recs,
                                                                       const double* zmin, RenderOut o) {
  __shared__ float4 lrec[RENDER_THREADS][3];
  __shared__ int lface[RENDER_THREADS];
  __shared__ int wcnt[RENDER_WAVES];
  const int n = blockIdx.y;
  const int tiles_x = (W + RENDER_TILE - 1) / RENDER_TILE;
  const int tx0 = (blockIdx.x % tiles_x) * RENDER_TILE, ty0 = (blockIdx.x / tiles_x) * RENDER_TILE;
  const int tid = threadIdx.x, lane = tid & (SCF_WAVE - 1), wid = tid / SCF_WAVE;
  const int px = tx0 + (tid % RENDER_TILE), py = ty0 + (tid / RENDER_TILE);
  const bool in_img = px < W && py < H;
  const int smin = min(H, W);
  const double x = pixel_coord(px, W, smin), y = pixel_coord(py, H, smin);
  int vbase, nv, fbase, nf;
  sample_mesh(m, labels, n, vbase, nv, fbase, nf);
  const int64_t base = (int64_t)n * m.max_faces;

  double bz = INFINITY;
  int bf = -1;
  for (int f0 = 0; f0 < nf; f0 += RENDER_THREADS) {
    const int f = f0 + tid;
    bool hit = false;
    if (f < nf) {
      const short4 b = boxes[base + f];
      hit = b.x <= tx0 + RENDER_TILE - 1 && b.y >= tx0 && b.z <= ty0 + RENDER_TILE - 1 && b.w >= ty0;
    }
    const unsigned long long mask = __ballot(hit);
    if (lane == 0) wcnt[wid] = __popcll(mask);
    __syncthreads();
    int off = 0, total = 0;
#pragma unroll
    for (int w = 0; w < RENDER_WAVES; ++w) {
      off += w < wid ? wcnt[w] : 0;
      total += wcnt[w];
    }
    if (hit) {
      const int s = off + __popcll(mask & ((1ull << lane) - 1));
      const float4* r = recs + 3 * (base + f);
      lrec[s][0] = r[0];
      lrec[s][1] = r[1];
      lrec[s][2] = r[2];
      lface[s] = f;
    }
    __syncthreads();
    if (in_img) {
      for (int k = 0; k < total; ++k) {
        const float4 a = lrec[k][0], b = lrec[k][1], c = lrec[k][2];
        const double u0 = a.x, v0 = a.y, u1 = a.z, v1 = a.w, u2 = b.x, v2 = b.y;
        const double w0 = edge_fn(u1, v1, u2, v2, x, y);
        const double w1 = edge_fn(u2, v2, u0, v0, x, y);
        const double w2 = edge_fn(u0, v0, u1, v1, x, y);
        const double sg = c.y;
        if (!(w0 * sg >= 0 && w1 * sg >= 0 && w2 * sg >= 0)) continue;
        const double s = w0 + w1 + w2;
        if (s == 0.0) continue;
        const double q = (w0 * (double)b.z + w1 * (double)b.w + w2 * (double)c.x) / s;
        const double z = 1.0 / q;
        if (!(z > 0) || !(z < INFINITY)) continue;
        const int fk = lface[k];
        if (z < bz || (z == bz && fk < bf)) { bz = z; bf = fk; }
      }
    }
    __syncthreads();
  }
  if (!in_img) return;

  const int64_t HW = (int64_t)H * W, pix = (int64_t)py * W + px;
  float rgb[3] = {o.bg[0], o.bg[1], o.bg[2]};
  float zout = -1.f;
  if (bf >= 0) {
    // re-project the winner in fp64 from the fp32 inputs: depth and shading barycentrics at full precision
    const float* R = Rs + 9 * (int64_t)n;
    const float* t = ts + 3 * (int64_t)n;
    const float* K = Ks + 9 * (int64_t)n;
    const int* fi = m.faces + 3 * (int64_t)(fbase + bf);
    const int64_t vi[3] = {vbase + (int64_t)fi[0], vbase + (int64_t)fi[1], vbase + (int64_t)fi[2]};
    const double fx = K[0], cx = K[2], fy = K[4], cy = K[5];
    double u[3], v[3], iz[3];
    for (int k = 0; k < 3; ++k) {
      double c[3];
      cam_point(R, t, m.verts + 3 * vi[k], c);
      u[k] = fx * c[0] / c[2] + cx;
      v[k] = fy * c[1] / c[2] + cy;
      iz[k] = 1.0 / c[2];
    }
    const double w0 = (x - u[1]) * (v[2] - v[1]) - (y - v[1]) * (u[2] - u[1]);
    const double w1 = (x - u[2]) * (v[0] - v[2]) - (y - v[2]) * (u[0] - u[2]);
    const double w2 = (x - u[0]) * (v[1] - v[0]) - (y - v[0]) * (u[1] - u[0]);
    double B[3] = {w0 * iz[0], w1 * iz[1], w2 * iz[2]};
    const double q = B[0] + B[1] + B[2];
    double z = (w0 + w1 + w2) / q;
    if (!(z > 0) || !(z < INFINITY)) z = bz;          // only reachable within rounding of an edge or z = 0
    B[0] /= q; B[1] /= q; B[2] /= q;
    zout = (float)z;
    double p[3] = {0, 0, 0}, nr[3] = {0, 0, 0}, col[3] = {0, 0, 0};
    for (int k = 0; k < 3; ++k) {
      for (int j = 0; j < 3; ++j) {
        p[j] += B[k] * (double)m.verts[3 * vi[k] + j];
        nr[j] += B[k] * (double)m.normals[3 * vi[k] + j];
        col[j] += B[k] * (double)m.colors[3 * vi[k] + j];
      }
    }
    // light position and colours (rendering.py:191-207)
    double L[3] = {0.0, 1.0, 0.0};
    const double la = o.default_lights ? 0.5 : 0.8, ld = o.default_lights ? 0.3 : 0.5, ls = o.default_lights ? 0.2 : 1.0;
    if (o.seperate_lights || !o.default_lights) {
      double zl;
      if (o.seperate_lights) {
        zl = fmax(zmin[n] - 400.0, 0.0);
      } else {
        double zb = INFINITY;
        for (int i = 0; i < N; ++i) zb = fmin(zb, zmin[i]);
        zl = floor(zb / 100.0) * 100.0 / 4.0;
      }
      L[0] = (double)R[2] * zl; L[1] = (double)R[5] * zl; L[2] = (double)R[8] * zl;
    }
    const double cam[3] = {-((double)R[0] * t[0] + (double)R[3] * t[1] + (double)R[6] * t[2]),
                           -((double)R[1] * t[0] + (double)R[4] * t[1] + (double)R[7] * t[2]),
                           -((double)R[2] * t[0] + (double)R[5] * t[1] + (double)R[8] * t[2])};
    double l[3] = {L[0] - p[0], L[1] - p[1], L[2] - p[2]};
    double vd[3] = {cam[0] - p[0], cam[1] - p[1], cam[2] - p[2]};
    normalize3(nr);
    normalize3(l);
    normalize3(vd);
    const double cosang = nr[0] * l[0] + nr[1] * l[1] + nr[2] * l[2];
    const double diffuse = ld * fmax(cosang, 0.0);
    double spec = 0.0;
    if (cosang > 0) {
      double a = 0.0;
      for (int j = 0; j < 3; ++j) a += vd[j] * (2.0 * cosang * nr[j] - l[j]);
      a = fmax(a, 0.0);
      for (int i = 0; i < 6; ++i) a *= a;                // a^64
      spec = ls * a;
    }
    for (int j = 0; j < 3; ++j) rgb[j] = (float)((la + diffuse) * col[j] + spec);
  }
  o.zbuf[n * HW + pix] = zout;
  if (o.p2f) o.p2f[n * HW + pix] = bf;
  if (o.rgba) {
    float4* dst = reinterpret_cast<float4*>(o.rgba) + n * HW + pix;
    *dst = make_float4(rgb[0], rgb[1], rgb[2], bf >= 0 ? 1.f : 0.f);
  }
  if (o.rgb) {
#pragma unroll
    for (int j = 0; j < 3; ++j) o.rgb[(n * 3 + j) * HW + pix] = (rgb[j] - o.mean[j]) / o.stdv[j];
  }
}

// ------------------------------------------------------------------------------------------------ host
static int64_t render_ws_layout(int N, int max_faces, int64_t* off_boxes, int64_t* off_recs) {
  const int64_t a = ((int64_t)N * 8 + 255) / 256 * 256;
  const int64_t nb = (int64_t)N * max_faces * 8;
  const int64_t b = a + (nb + 255) / 256 * 256;
  *off_boxes = a;
  *off_recs = b;
  return b + (int64_t)N * max_faces * 48;
}

extern "C" double scf_render_pixel_coord(int index, int size, int other) {
  if (size <= 0 || other <= 0) return NAN;
  return pixel_coord(index, size, size < other ? size : other);
}

extern "C" int64_t scf_render_workspace_bytes(int N, int max_faces) {
  if (N <= 0 || max_faces <= 0) return SCF_EINVAL;
  int64_t ob, orr;
  return render_ws_layout(N, max_faces, &ob, &orr);
}

extern "C" int scf_render_mesh(const scf_mesh_store* mesh, const int32_t* labels, const float* R, const float* t,
                               const float* K, int N, const scf_render_params* p, float* zbuf, int32_t* pix_to_face,
                               float* rgba, float* rgb_nchw, void* workspace, scf_stream_t stream) {
  if (!mesh || !p || !labels || !R || !t || !K || !zbuf || !workspace || N <= 0) return SCF_EINVAL;
  if (!mesh->verts || !mesh->normals || !mesh->colors || !mesh->faces || !mesh->vert_offset || !mesh->face_offset ||
      mesh->num_classes <= 0 || mesh->max_faces <= 0)
    return SCF_EINVAL;
  if (p->H <= 0 || p->W <= 0 || p->H > RENDER_MAX_SIZE || p->W > RENDER_MAX_SIZE) return SCF_EINVAL;
  if ((int64_t)N * ((p->W + RENDER_TILE - 1) / RENDER_TILE) > 0x7fffffffLL) return SCF_EINVAL;
  if ((int64_t)N > 65535 || (mesh->max_faces + 255) / 256 > 0x7fffffff) return SCF_EINVAL;
  if (rgb_nchw)
    for (int j = 0; j < 3; ++j)
      if (!(p->norm_std[j] != 0.f)) return SCF_EINVAL;
  MeshArgs m{mesh->verts, mesh->normals, mesh->colors, (const int*)mesh->faces, (const int*)mesh->vert_offset,
             (const int*)mesh->face_offset, mesh->num_classes, mesh->max_faces};
  int64_t ob, orr;
  render_ws_layout(N, mesh->max_faces, &ob, &orr);
  char* ws = (char*)workspace;
  double* zmin = (double*)ws;
  short4* boxes = (short4*)(ws + ob);
  float4* recs = (float4*)(ws + orr);
  hipStream_t st = scf_stream(stream);
  if (p->seperate_lights || !p->default_lights) {
    scf_launch(render_zmin_kernel, dim3(N), dim3(RENDER_THREADS), 0, st, m, (const int*)labels, R, t, zmin);
    const int e = scf_launch_status();
    if (e != SCF_OK) return e;
  }
  scf_launch(render_setup_kernel, dim3((mesh->max_faces + 255) / 256, N), dim3(256), 0, st, m, (const int*)labels, R, t,
             K, (int)p->H, (int)p->W, boxes, recs);
  int e = scf_launch_status();
  if (e != SCF_OK) return e;
  RenderOut o{zbuf, (int*)pix_to_face, rgba, rgb_nchw, {p->background[0], p->background[1], p->background[2]},
              {p->norm_mean[0], p->norm_mean[1], p->norm_mean[2]}, {p->norm_std[0], p->norm_std[1], p->norm_std[2]},
              p->default_lights, p->seperate_lights};
  const int tiles = ((p->W + RENDER_TILE - 1) / RENDER_TILE) * ((p->H + RENDER_TILE - 1) / RENDER_TILE);
  scf_launch(render_raster_kernel, dim3(tiles, N), dim3(RENDER_THREADS), 0, st, m, (const int*)labels, R, t, K, N,
             (int)p->H, (int)p->W, (const short4*)boxes, (const float4*)recs, (const double*)zmin, o);
  return scf_launch_status();
}
