// The arithmetic of oetr_dual_softmax_match (include/oetr_dual_softmax.h), the ONE copy: the kernels of
// dual_softmax.hip use it on the device and tools/dual_softmax_hostmath.cpp compiles it for the host, where
// tests/test_dual_softmax_cpu.py holds it to the numpy specification tests/dual_softmax_oracle.py bit for bit before
// any device run.  float32; every product, sum and quotient is rounded on its own except where fmaf is written.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define DS_FN __host__ __device__ __forceinline__
#else
#define DS_FN inline
#endif

namespace oetr {
namespace ds {

// e(x) = 0 below this: exp(-87) = 1.6e-38 is still a normal float32, so e never returns a subnormal
constexpr float E_CUT = -87.0f;
constexpr float E_LOG2E = 1.44269502162933349609375f;          // float32(1 / ln 2)
constexpr float E_LN2_HI = 0.693359375f;                       // 355 / 512: n * E_LN2_HI is exact for |n| <= 126
constexpr float E_LN2_LO = -2.12194440e-4f;                    // float32(ln 2 - 355 / 512)
// 1 + r + r^2 / 2 + ... to r^7 on |r| <= ln 2 / 2 (the coefficients of Cephes' expf), Horner from E_C7 down
constexpr float E_C7 = 1.9875691500e-4f, E_C6 = 1.3981999507e-3f, E_C5 = 8.3334519073e-3f, E_C4 = 4.1665795894e-2f,
                E_C3 = 1.6666665459e-1f, E_C2 = 0.5f;
// a softmax factor below this power of two is no candidate: a product of two factors is then never subnormal
constexpr float Q_MIN = 0x1p-62f;
// the partial sums of a row: see slot()
constexpr int PARTIALS = 8;

DS_FN bool finite(float t) { return t - t == 0.0f; }           // false for NaN, +inf, -inf

// The float32 exponential of the specification for x <= 0 (x finite or -inf): n = rint(x * log2e), r = x - n ln 2 in
// two fmaf, the polynomial in seven fmaf, n added to the exponent field.  x >= E_CUT gives n >= -126 and, where
// n = -126, a polynomial value >= 1: the result is normal.  e(0) = 1 exactly.
DS_FN float e(float x) {
#pragma clang fp contract(off)
  if (!(x >= E_CUT)) return 0.0f;
  const float n = rintf(x * E_LOG2E);
  float r = fmaf(n, -E_LN2_HI, x);
  r = fmaf(n, -E_LN2_LO, r);
  float p = E_C7;
  p = fmaf(p, r, E_C6);
  p = fmaf(p, r, E_C5);
  p = fmaf(p, r, E_C4);
  p = fmaf(p, r, E_C3);
  p = fmaf(p, r, E_C2);
  p = fmaf(p, r, 1.0f);
  p = fmaf(p, r, 1.0f);
  int32_t bits;
  memcpy(&bits, &p, 4);
  bits += (int32_t)n * (1 << 23);
  memcpy(&p, &bits, 4);
  return p;
}

// t = s * scale, one rounding
DS_FN float scaled(float s, float scale) {
#pragma clang fp contract(off)
  return s * scale;
}

// The partial sum that column j of a row belongs to.  Within a tile of 128 columns, jj = j % 128: the 64-column half
// kh = jj / 64, the lane half hh = (jj / 4) % 2 and the 32-column accumulator a = (jj / 32) % 2 - the three things a
// lane of the kernel does not walk - so a partial is one register that takes its columns in ASCENDING j.
DS_FN int slot(int j) { return ((j >> 6) & 1) * 4 + ((j >> 2) & 1) * 2 + ((j >> 5) & 1); }

// one more term of a partial sum
DS_FN float add_term(float partial, float term) {
#pragma clang fp contract(off)
  return partial + term;
}

// one node of the fixed tree ((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7)); float addition commutes
DS_FN float tree_node(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}

// one softmax factor e(t - m) / Z
DS_FN float factor(float t, float m, float Z) {
#pragma clang fp contract(off)
  return e(t - m) / Z;
}

// The confidence of one element from its two factors, or -1 where it is no candidate (a confidence is never negative).
DS_FN float confidence(float t, float m, float Z, float c, float Y) {
#pragma clang fp contract(off)
  if (!finite(t)) return -1.0f;
  const float q0 = factor(t, m, Z), q1 = factor(t, c, Y);
  if (!(q0 >= Q_MIN) || !(q1 >= Q_MIN)) return -1.0f;
  return q0 * q1;
}

// the running (maximum, lowest index that attains it) of one query; i = -1: no candidate yet
struct Best {
  float v;
  int i;
};

DS_FN Best best_empty() { return {-1.0f, -1}; }

DS_FN void best_push(Best& b, float conf, int j) {
  if (conf < 0.0f) return;
  if (conf > b.v || (conf == b.v && (unsigned)j < (unsigned)b.i)) b.v = conf, b.i = j;
}

// the union of two disjoint column sets; an empty side (v = -1, i = -1: the largest unsigned) loses
DS_FN Best best_merge(const Best& a, const Best& b) {
  return (a.v > b.v || (a.v == b.v && (unsigned)a.i < (unsigned)b.i)) ? a : b;
}

// the running maximum of the finite t of one query (-inf: none yet)
DS_FN float max_push(float m, float t) { return finite(t) && t > m ? t : m; }

// token i of an h x w grid in raster order lies at least `border` cells from every edge
DS_FN bool inside(int i, int h, int w, int border) {
  const int row = i / w, col = i - row * w;
  return row >= border && row < h - border && col >= border && col < w - border;
}

}  // namespace ds
}  // namespace oetr
