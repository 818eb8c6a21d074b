// The descriptor arithmetic of oetr_keypoint_select (include/oetr_keypoint_select.h), the ONE copy: k_ks_emit
// (keypoint_select.hip) uses it on the device and tools/keypoint_select_hostmath.cpp compiles it for the host, where
// tests/test_keypoint_select_cpu.py holds it to the numpy specification before any device run.  float32, every product
// and sum rounded on its own, division and sqrt correctly rounded.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define KS_FN __host__ __device__ __forceinline__
#else
#define KS_FN inline
#endif

namespace oetr {
namespace ks {

// a NaN score is loaded as -inf
KS_FN float load_score(float s) { return s != s ? -INFINITY : s; }

// SuperPoint's sample_descriptors coordinate followed by grid_sample's align_corners=True un-normalisation;
// n: the descriptor map's w (or h)
KS_FN float coordinate(float kp, int n, int cell) {
#pragma clang fp contract(off)
  const float half = (float)(cell * 0.5);
  const float den = (float)((double)n * cell - cell * 0.5 - 0.5);
  const float t = (kp - half) + 0.5f;
  const float g = (t / den) * 2.0f - 1.0f;
  return ((g + 1.0f) / 2.0f) * (float)(n - 1);
}

// The four taps of one keypoint: weights, whether each lies inside the map (decided on the floats, so a NaN or
// infinite coordinate has no tap), and the cell indices (0 where outside).
struct Taps {
  float w_nw, w_ne, w_sw, w_se;
  bool nw, ne, sw, se;
  int x0, x1, y0, y1;
};

KS_FN Taps taps(float x, float y, int w, int h, int cell) {
#pragma clang fp contract(off)
  const float ix = coordinate(x, w, cell), iy = coordinate(y, h, cell);
  const float x0 = floorf(ix), y0 = floorf(iy);
  const float x1 = x0 + 1.0f, y1 = y0 + 1.0f;
  const float wx1 = ix - x0, wx0 = x1 - ix, wy1 = iy - y0, wy0 = y1 - iy;
  const bool in_x0 = x0 >= 0.0f && x0 <= (float)(w - 1), in_x1 = x1 >= 0.0f && x1 <= (float)(w - 1);
  const bool in_y0 = y0 >= 0.0f && y0 <= (float)(h - 1), in_y1 = y1 >= 0.0f && y1 <= (float)(h - 1);
  Taps t;
  t.w_nw = wx0 * wy0, t.w_ne = wx1 * wy0, t.w_sw = wx0 * wy1, t.w_se = wx1 * wy1;
  t.nw = in_x0 && in_y0, t.ne = in_x1 && in_y0, t.sw = in_x0 && in_y1, t.se = in_x1 && in_y1;
  t.x0 = in_x0 ? (int)x0 : 0, t.x1 = in_x1 ? (int)x1 : 0;
  t.y0 = in_y0 ? (int)y0 : 0, t.y1 = in_y1 ? (int)y1 : 0;
  return t;
}

// one channel: f points at element (d, 0, 0) of the map; sy, sx: its row and column strides in elements
KS_FN float interpolate(const Taps& t, const float* f, int64_t sy, int64_t sx) {
#pragma clang fp contract(off)
  const float t_nw = t.nw ? f[t.y0 * sy + t.x0 * sx] * t.w_nw : 0.0f;
  const float t_ne = t.ne ? f[t.y0 * sy + t.x1 * sx] * t.w_ne : 0.0f;
  const float t_sw = t.sw ? f[t.y1 * sy + t.x0 * sx] * t.w_sw : 0.0f;
  const float t_se = t.se ? f[t.y1 * sy + t.x1 * sx] * t.w_se : 0.0f;
  return ((t_nw + t_ne) + t_sw) + t_se;
}

// a partial sum of squares takes one more channel
KS_FN float add_square(float partial, float v) {
#pragma clang fp contract(off)
  return partial + v * v;
}

// one step of the fixed tree: p[j] += p[j + stride]
KS_FN float tree_step(float mine, float other) {
#pragma clang fp contract(off)
  return mine + other;
}

KS_FN float norm_of(float ss) {
  const float n = sqrtf(ss);
  return n < 1e-12f ? 1e-12f : n;
}

}  // namespace ks
}  // namespace oetr
