// Pose helpers shared by pose.hip (dense re-projection / un-projection) and pnp.hip (correspondence
// extraction): one definition, so both un-project a pixel with the same instructions.
#pragma once
#include "scf_common.h"

// 3x3 inverse in fp64 (adjugate), rounded to fp32.  The reference uses torch.inverse (fp32
// LU); both are within a few fp32 ulp of the true inverse.
__device__ inline void inv3x3(const float* m, float* o) {
  const double a = m[0], b = m[1], c = m[2], d = m[3], e = m[4], f = m[5], g = m[6], h = m[7],
               i = m[8];
  const double A = e * i - f * h, B = -(d * i - f * g), C = d * h - e * g;
  const double det = a * A + b * B + c * C;
  const double id = 1.0 / det;
  o[0] = (float)(A * id);
  o[1] = (float)(-(b * i - c * h) * id);
  o[2] = (float)((b * f - c * e) * id);
  o[3] = (float)(B * id);
  o[4] = (float)((a * i - c * g) * id);
  o[5] = (float)(-(a * f - c * d) * id);
  o[6] = (float)(C * id);
  o[7] = (float)(-(a * h - b * g) * id);
  o[8] = (float)((a * e - b * d) * id);
}

struct PoseMats {
  float Kinv[9], R0inv[9], t0[3], K[9], R[9], t[3];
};

__device__ inline void load_mats(PoseMats* s, const float* K, const float* R0, const float* t0,
                                 const float* R, const float* t, int n) {
  const int tid = threadIdx.x;
  if (tid == 0) inv3x3(K + 9 * n, s->Kinv);
  if (tid == 64) inv3x3(R0 + 9 * n, s->R0inv);
  if (tid >= 128 && tid < 137) {
    s->K[tid - 128] = K[9 * n + tid - 128];
    if (R) s->R[tid - 128] = R[9 * n + tid - 128];
  }
  if (tid >= 192 && tid < 195) {
    s->t0[tid - 192] = t0[3 * n + tid - 192];
    if (t) s->t[tid - 192] = t[3 * n + tid - 192];
  }
  __syncthreads();
}

// object-frame point of pixel (x, y) with depth d: lift_2d_to_3d, pose.py:26-41
__device__ __forceinline__ void unproject(const PoseMats& s, float x, float y, float d, float& X,
                                          float& Y, float& Z) {
  const float hx = x * d, hy = y * d, hz = d;
  const float cx = s.Kinv[0] * hx + s.Kinv[1] * hy + s.Kinv[2] * hz - s.t0[0];
  const float cy = s.Kinv[3] * hx + s.Kinv[4] * hy + s.Kinv[5] * hz - s.t0[1];
  const float cz = s.Kinv[6] * hx + s.Kinv[7] * hy + s.Kinv[8] * hz - s.t0[2];
  X = s.R0inv[0] * cx + s.R0inv[1] * cy + s.R0inv[2] * cz;
  Y = s.R0inv[3] * cx + s.R0inv[4] * cy + s.R0inv[5] * cz;
  Z = s.R0inv[6] * cx + s.R0inv[7] * cy + s.R0inv[8] * cz;
}
