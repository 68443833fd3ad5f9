// Window centre and bilinear weights of one (query, level) of the multi-scale correlation lookup: the one definition
// the forward (corr_lookup.hip) and its adjoint with respect to the pyramid (corr_lookup_grad.hip) share.
#pragma once
#include "scf_common.h"

// Window centre of one (query, level) and its bilinear weights -- shared by the LDS-DMA kernel and
// the generic kernel so that both are the same arithmetic.  Reference: corr_lookup.py:127 (centre /
// 2^l), :64-67 (normalise with max(size-1, 1), grid_sample de-normalises with size-1).
//   * along a size-1 axis every tap lands exactly on index 0 (flat: centre := R, weights 1 | 0);
//   * a centre far outside any map is clamped to +-30000: all taps read zero padding;
//   * NaN / inf flow, or a centre whose normalisation overflows fp32 (|c| * 2 = inf): the reference's
//     grid_sample returns NaN for every tap of that query (torch CPU) -- reproduced by NaN weights
//     on an all-padding window (0 * NaN = NaN).
struct LkCentre {
  float x0f, y0f;       // floor of the (clamped) centre
  int x0, y0;           // map coordinates of window column / row 0
  float nw, ne, sw, se;
};
template <int R_>
__device__ __forceinline__ LkCentre lk_centre(float qx, float qy, float inv, bool flat_x, bool flat_y, int r_rt = 0) {
  const int R = R_ > 0 ? R_ : r_rt;
  const float cxu = qx * inv, cyu = qy * inv;               // exact power-of-two scaling
  const bool bad = !(fabsf(cxu * 2.f) < __builtin_inff()) || !(fabsf(cyu * 2.f) < __builtin_inff());
  float cx = flat_x ? (float)R : cxu;
  float cy = flat_y ? (float)R : cyu;
  cx = fminf(fmaxf(cx, -30000.f), 30000.f);                 // far outside any map -> all taps 0
  cy = fminf(fmaxf(cy, -30000.f), 30000.f);
  if (bad) { cx = -30000.f; cy = -30000.f; }
  LkCentre c;
  c.x0f = floorf(cx); c.y0f = floorf(cy);
  c.x0 = (int)c.x0f - R; c.y0 = (int)c.y0f - R;
  const float tx = cx - c.x0f, ty = cy - c.y0f;
  const float wx0 = (c.x0f + 1.f) - cx, wy0 = (c.y0f + 1.f) - cy;   // grid_sample: (x_se - x)
  const float nanv = __builtin_nanf("");
  c.nw = bad ? nanv : wx0 * wy0; c.ne = bad ? nanv : tx * wy0;
  c.sw = bad ? nanv : wx0 * ty;  c.se = bad ? nanv : tx * ty;
  return c;
}
