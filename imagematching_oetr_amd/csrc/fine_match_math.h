// The arithmetic of oetr_fine_refine (include/oetr_fine_match.h), the ONE copy: the kernels of fine_match.hip use it on
// the device and tools/fine_match_hostmath.cpp compiles it for the host, where tests/test_fine_match_cpu.py holds it to
// the numpy specification tests/fine_match_oracle.py bit for bit before any device run.  float32; every product, sum
// and quotient is rounded on its own except where fmaf is written.  e(x) is dual_softmax_math.h's, included, not
// restated.
#pragma once
#include "../../include/oetr_fine_match.h"
#include "dual_softmax_math.h"

namespace oetr {
namespace fm {

// the partial sums of a dot product: channel c belongs to partial (c / 4) % PARTIALS
constexpr int PARTIALS = OETR_FINE_MATCH_PARTIALS;
constexpr float VAR_MIN = 1e-10f;

DS_FN int partial_of(int c) { return (c >> 2) % PARTIALS; }

// G[k] = float32((2 k - (W - 1)) / (W - 1)), W in {3, 5, 7}
DS_FN float grid(int W, int k) {
  constexpr float g3[3] = OETR_FINE_MATCH_G3, g5[5] = OETR_FINE_MATCH_G5, g7[7] = OETR_FINE_MATCH_G7;
  return W == 3 ? g3[k] : (W == 5 ? g5[k] : g7[k]);
}

// the rounded square of G[k]
DS_FN float grid2(int W, int k) {
#pragma clang fp contract(off)
  const float g = grid(W, k);
  return g * g;
}

// float32(1 / sqrt(C)), formed in double: computed on the host, once per call
inline float scale_of(int C) { return (float)(1.0 / std::sqrt((double)C)); }

// float32((W / 2) * fine_cell): one rounding
DS_FN float radius_of(int W, float fine_cell) {
#pragma clang fp contract(off)
  return (float)(W / 2) * fine_cell;
}

// four more channels of one partial: ascending c
DS_FN float chain4(float acc, float a0, float a1, float a2, float a3, float b0, float b1, float b2, float b3) {
  acc = fmaf(a0, b0, acc);
  acc = fmaf(a1, b1, acc);
  acc = fmaf(a2, b2, acc);
  return fmaf(a3, b3, acc);
}

// one node of the fixed tree of adjacent pairs; float addition commutes
DS_FN float tree_node(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}

// t = s * scale, one rounding
DS_FN float t_of(float s, float scale) {
#pragma clang fp contract(off)
  return s * scale;
}

DS_FN bool candidate(float t) { return ds::finite(t); }

// the running maximum of the candidates (-inf: none yet); exact, whatever the order
DS_FN float max_push(float m, float t) { return candidate(t) && t > m ? t : m; }

// q = e(t - m_), +0 for what is no candidate
DS_FN float q_of(float t, float m) {
#pragma clang fp contract(off)
  return candidate(t) ? ds::e(t - m) : 0.0f;
}

// Z: ascending r from +0
DS_FN float sum_q(const float* q, int n) {
#pragma clang fp contract(off)
  float z = 0.0f;
  for (int r = 0; r < n; ++r) z = z + q[r];
  return z;
}

DS_FN float heat_of(float q, float Z) {
#pragma clang fp contract(off)
  return q / Z;
}

// one of the four serial sums over the heat: which = 0: x (G[kx]), 1: y (G[ky]), 2: xx, 3: yy (the rounded squares)
DS_FN float moment(const float* heat, int W, int which) {
  float acc = 0.0f;
  for (int ky = 0, r = 0; ky < W; ++ky)
    for (int kx = 0; kx < W; ++kx, ++r) {
      const int k = (which & 1) ? ky : kx;
      acc = fmaf(heat[r], which < 2 ? grid(W, k) : grid2(W, k), acc);
    }
  return acc;
}

struct Expec {
  float x, y, sd;
};

// var = second moment - mean * mean: the product rounded, the difference rounded; the square roots correctly rounded
DS_FN Expec finish(float x, float y, float xx, float yy) {
#pragma clang fp contract(off)
  const float px = x * x, py = y * y;
  float vx = xx - px, vy = yy - py;
  vx = vx > VAR_MIN ? vx : VAR_MIN;
  vy = vy > VAR_MIN ? vy : VAR_MIN;
  return {x, y, sqrtf(vx) + sqrtf(vy)};
}

// a match without a candidate
DS_FN Expec none() { return {0.0f, 0.0f, NAN}; }

// keypoint + v * radius: the product rounded, the sum rounded
DS_FN float refined(float kp, float v, float radius) {
#pragma clang fp contract(off)
  const float d = v * radius;
  return kp + d;
}

}  // namespace fm
}  // namespace oetr
