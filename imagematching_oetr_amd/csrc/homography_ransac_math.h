// The arithmetic of the homography entry (include/oetr_homography_ransac.h), one copy for every kernel of
// homography_ransac.hip: tests/homography_ransac_oracle.py LITERALLY - float64, every operation rounded on its own in
// the order and with the parentheses written there, IEEE division and square root, no contraction into FMAs, every
// decision a comparison.  Plain C++ (no HIP types), so the same text also compiles for the host
// (tools/homography_ransac_hostmath.cpp).  The sampler's bits, det3 and the small helpers are pose_ransac_math.h's.
// Arrays are indexed by compile-time constants after unrolling: nothing here needs scratch memory.
#pragma once
#include <cstdint>

#include "pose_ransac_math.h"

namespace oetr {
namespace hr {

using pr::abs64;
using pr::det3;
using pr::finite64;
using pr::nan64;
using pr::sqrt_rn;

constexpr int SAMPLE = 4;                 // rows of a minimal sample
constexpr int TERMS = 28;                 // sums of the refit's normal equations
constexpr int CLASSES = 256;              // partial sums of each: the list position modulo 256
constexpr int MAX_SIDE = 8192;            // OETR_COVIS_MAX_SIDE

// ------------------------------------------------------------------ normalisation
struct Frames {
  double c1x, c1y, s1, c2x, c2y, s2;
};

// W1, H1, W2, H2 whole numbers in 1..MAX_SIDE (false for NaN): P[9..12] of the parameter block.
PR_FN bool sizes_ok(const double* P) {
  bool ok = true;
#pragma unroll
  for (int k = 9; k < 13; ++k) {
    const double s = P[k];
    ok = ok && s >= 1.0 && s <= (double)MAX_SIDE && s == __builtin_rint(s);
  }
  return ok;
}

PR_FN Frames frames(const double* P) {
#pragma clang fp contract(off)
  Frames f;
  f.c1x = (P[9] - 1.0) / 2.0, f.c1y = (P[10] - 1.0) / 2.0, f.s1 = (P[9] + P[10]) / 2.0;
  f.c2x = (P[11] - 1.0) / 2.0, f.c2y = (P[12] - 1.0) / 2.0, f.s2 = (P[11] + P[12]) / 2.0;
  return f;
}

PR_FN void normalise(const Frames& f, double u1, double v1, double u2, double v2, double& x1, double& y1, double& x2,
                     double& y2) {
#pragma clang fp contract(off)
  x1 = (u1 - f.c1x) / f.s1, y1 = (v1 - f.c1y) / f.s1;
  x2 = (u2 - f.c2x) / f.s2, y2 = (v2 - f.c2y) / f.s2;
}

PR_FN double thr_sq(const Frames& f, double px_thr) {
#pragma clang fp contract(off)
  const double thr_n = px_thr / f.s2;
  return thr_n * thr_n;
}

// ------------------------------------------------------------------ sampling
// 4 distinct rows of a list of `len` >= 4 rows, ascending; every idx[j] < len.  pr::sample7's construction.
PR_FN void sample4(uint32_t seed, uint32_t pair_id, uint32_t h, uint32_t len, uint32_t (&idx)[SAMPLE]) {
#pragma unroll
  for (int j = 0; j < SAMPLE; ++j) {
    const uint64_t range = (uint64_t)(len - (uint32_t)j);
    uint32_t v = (uint32_t)(((uint64_t)pr::draw_bits(seed, pair_id, h, (uint32_t)j) * range) >> 32);   // < len - j
#pragma unroll
    for (int i = 0; i < j; ++i)
      if (v >= idx[i]) v += 1u;                                     // steps past the rows already chosen: < len
    idx[j] = v;
#pragma unroll
    for (int i = j; i > 0; --i) {                                   // keeps them ascending
      const uint32_t lo = idx[i - 1] < idx[i] ? idx[i - 1] : idx[i];
      const uint32_t hi = idx[i - 1] < idx[i] ? idx[i] : idx[i - 1];
      idx[i - 1] = lo;
      idx[i] = hi;
    }
  }
}

// ------------------------------------------------------------------ the 4-point solver
PR_FN bool finite_model(const double (&h)[9]) {
  bool fin = true;
#pragma unroll
  for (int k = 0; k < 9; ++k) fin = fin && finite64(h[k]);
  return fin;
}

PR_FN double a2_of(const double (&h)[9], double x, double y) {
#pragma clang fp contract(off)
  return (h[6] * x + h[7] * y) + h[8];
}

// h scaled by 1 / sqrt(sum of squares), then negated when a2 of the row (x, y) is negative.
PR_FN void unit_and_sign(double (&h)[9], double x, double y) {
#pragma clang fp contract(off)
  double ss = h[0] * h[0];
#pragma unroll
  for (int k = 1; k < 9; ++k) ss = ss + h[k] * h[k];
  const double scale = 1.0 / sqrt_rn(ss);
#pragma unroll
  for (int k = 0; k < 9; ++k) h[k] = h[k] * scale;
  const bool neg = a2_of(h, x, y) < 0.0;
#pragma unroll
  for (int k = 0; k < 9; ++k) h[k] = neg ? -h[k] : h[k];
}

// [d1 p1 | d2 p2 | d3 p3] of four points (x, y, 1), as rows.
PR_FN void basis(const double (&x)[SAMPLE], const double (&y)[SAMPLE], double (&A)[3][3]) {
#pragma clang fp contract(off)
  double d[3];
  d[0] = det3(x[3], y[3], 1.0, x[1], y[1], 1.0, x[2], y[2], 1.0);
  d[1] = det3(x[0], y[0], 1.0, x[3], y[3], 1.0, x[2], y[2], 1.0);
  d[2] = det3(x[0], y[0], 1.0, x[1], y[1], 1.0, x[3], y[3], 1.0);
#pragma unroll
  for (int c = 0; c < 3; ++c) A[0][c] = d[c] * x[c], A[1][c] = d[c] * y[c], A[2][c] = d[c] * 1.0;
}

// X[r] = (x1, y1, x2, y2) of the sample's row r, normalised.  out = the model (row major) or all NaN.
PR_FN void solve4(const double (&X)[SAMPLE][4], double (&out)[9]) {
#pragma clang fp contract(off)
  double xa[SAMPLE], ya[SAMPLE], xb[SAMPLE], yb[SAMPLE];
#pragma unroll
  for (int r = 0; r < SAMPLE; ++r) xa[r] = X[r][0], ya[r] = X[r][1], xb[r] = X[r][2], yb[r] = X[r][3];
  double a[3][3], B[3][3], adj[3][3];
  basis(xa, ya, a);
  basis(xb, yb, B);
  adj[0][0] = a[1][1] * a[2][2] - a[1][2] * a[2][1];
  adj[0][1] = a[0][2] * a[2][1] - a[0][1] * a[2][2];
  adj[0][2] = a[0][1] * a[1][2] - a[0][2] * a[1][1];
  adj[1][0] = a[1][2] * a[2][0] - a[1][0] * a[2][2];
  adj[1][1] = a[0][0] * a[2][2] - a[0][2] * a[2][0];
  adj[1][2] = a[0][2] * a[1][0] - a[0][0] * a[1][2];
  adj[2][0] = a[1][0] * a[2][1] - a[1][1] * a[2][0];
  adj[2][1] = a[0][1] * a[2][0] - a[0][0] * a[2][1];
  adj[2][2] = a[0][0] * a[1][1] - a[0][1] * a[1][0];
  double h[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) h[3 * i + j] = (B[i][0] * adj[0][j] + B[i][1] * adj[1][j]) + B[i][2] * adj[2][j];
  unit_and_sign(h, xa[0], ya[0]);
  bool ok = finite_model(h);
#pragma unroll
  for (int r = 0; r < SAMPLE; ++r) ok = ok && a2_of(h, xa[r], ya[r]) > 0.0;      // the orientation test
#pragma unroll
  for (int k = 0; k < 9; ++k) out[k] = ok ? h[k] : nan64();
}

// ------------------------------------------------------------------ scoring
// a2 > 0 and the squared transfer error in picture 2 below the threshold, without the division; false for NaN.
PR_FN bool inlier(const double (&h)[9], double x1, double y1, double x2, double y2, double thr_sq) {
#pragma clang fp contract(off)
  const double a0 = (h[0] * x1 + h[1] * y1) + h[2];
  const double a1 = (h[3] * x1 + h[4] * y1) + h[5];
  const double a2 = (h[6] * x1 + h[7] * y1) + h[8];
  const double dx = x2 * a2 - a0, dy = y2 * a2 - a1;
  // both comparisons always (a bitwise and): a short-circuit here becomes a branch per row in the scoring loop, which
  // keeps the rows of an unrolled loop from overlapping
  const bool front = a2 > 0.0, near = dx * dx + dy * dy < thr_sq * (a2 * a2);
  return front & near;
}

// ------------------------------------------------------------------ the refit
// acc[k] = acc[k] + term k of one row (tests/homography_ransac_oracle.py: row_terms).
PR_FN void add_row_terms(double (&acc)[TERMS], double x, double y, double x2, double y2) {
#pragma clang fp contract(off)
  const double mx = -(x2 * x), my = -(x2 * y), nx = -(y2 * x), ny = -(y2 * y);
  const double t[TERMS] = {x * x,  x * y,  x,      y * y,  y,                          //
                           x * mx, x * my, y * mx, y * my, mx, my,                    //
                           x * nx, x * ny, y * nx, y * ny, nx, ny,                    //
                           mx * mx + nx * nx, mx * my + nx * ny, my * my + ny * ny,   //
                           x * x2, y * x2, x2,     x * y2, y * y2, y2,                //
                           mx * x2 + nx * y2, my * x2 + ny * y2};
#pragma unroll
  for (int k = 0; k < TERMS; ++k) acc[k] = acc[k] + t[k];
}

// The augmented 8 x 9 system of the normal equations, element e = 9 * row + column: the index of its sum, NORMAL_N
// for the count of the rows, NORMAL_ZERO for a structural zero.
constexpr int NORMAL_N = 28, NORMAL_ZERO = 29;
PR_FN int normal_index(int e) {
  constexpr signed char M[72] = {0,  1,  2,  29, 29, 29, 5,  6,  20,   //
                                 1,  3,  4,  29, 29, 29, 7,  8,  21,   //
                                 2,  4,  28, 29, 29, 29, 9,  10, 22,   //
                                 29, 29, 29, 0,  1,  2,  11, 12, 23,   //
                                 29, 29, 29, 1,  3,  4,  13, 14, 24,   //
                                 29, 29, 29, 2,  4,  28, 15, 16, 25,   //
                                 5,  7,  9,  11, 13, 15, 17, 18, 26,   //
                                 6,  8,  10, 12, 14, 16, 18, 19, 27};
  return M[e];
}

// Gauss-Jordan with partial pivoting, pr::solve7's rule, in the two steps every form of the elimination shares.
// The pivot row of column c: the largest |entry| among rows c .. 7 (col[r] = A[r][c]; diag = A[c][c]), the lowest row
// on a tie; ok turns false for a zero or NaN pivot.
PR_FN int gj_pivot(double diag, const double (&col)[8], int c, bool& ok) {
  double best = abs64(diag);
  int piv = c;
#pragma unroll
  for (int r = 1; r < 8; ++r) {
    const double v = abs64(col[r]);
    const bool take = r > c && v > best;                            // the lowest index wins a tie
    best = take ? v : best;
    piv = take ? r : piv;
  }
  ok = ok && (best > 0.0);                                          // false for a NaN pivot, too
  return piv;
}

// After the row swap, the new element (r, k) for k > c: the pivot row is divided by d = A[c][c]; every other row
// subtracts f = A[r][c] times the DIVIDED element a_ck / d.
PR_FN double gj_element(bool pivot_row, double a_rk, double a_ck, double d, double f) {
#pragma clang fp contract(off)
  const double t = a_ck / d;
  return pivot_row ? t : a_rk - f * t;
}

// The normal equations from the 28 sums and the count n, solved serially: cand = the 8 unknowns and 1.  Row swaps by
// selects, compile-time indices.  (k_hr_finish runs the same two steps spread over the lanes of a workgroup.)
PR_FN bool solve8(const double (&S)[TERMS], double n, double (&cand)[9]) {
#pragma clang fp contract(off)
  double A[8][9];
#pragma unroll
  for (int e = 0; e < 72; ++e) {
    const int at = normal_index(e);
    A[e / 9][e % 9] = at == NORMAL_N ? n : (at == NORMAL_ZERO ? 0.0 : S[at < TERMS ? at : 0]);
  }
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    double col[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) col[r] = A[r][c];
    const int piv = gj_pivot(A[c][c], col, c, ok);
#pragma unroll
    for (int r = c + 1; r < 8; ++r) {
      const bool sw = piv == r;
#pragma unroll
      for (int k = c; k < 9; ++k) {
        const double u = A[c][k], w = A[r][k];
        A[c][k] = sw ? w : u;
        A[r][k] = sw ? u : w;
      }
    }
    const double d = A[c][c];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      if (r == c) continue;
      const double f = A[r][c];
#pragma unroll
      for (int k = c + 1; k < 9; ++k) A[r][k] = gj_element(false, A[r][k], A[c][k], d, f);
    }
#pragma unroll
    for (int k = c + 1; k < 9; ++k) A[c][k] = gj_element(true, A[c][k], A[c][k], d, 0.0);
  }
#pragma unroll
  for (int r = 0; r < 8; ++r) cand[r] = A[r][8];
  cand[8] = 1.0;
  return ok;
}

// ------------------------------------------------------------------ delivery and errors
// T2^-1 Hn T1 in pixel coordinates up to scale, of unit Frobenius norm, the sign kept.
PR_FN void deliver(const double (&h)[9], const Frames& f, double (&H)[9]) {
#pragma clang fp contract(off)
  double g[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    g[r][0] = h[3 * r], g[r][1] = h[3 * r + 1];
    g[r][2] = (f.s1 * h[3 * r + 2] - h[3 * r] * f.c1x) - h[3 * r + 1] * f.c1y;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    H[c] = f.s2 * g[0][c] + f.c2x * g[2][c];
    H[3 + c] = f.s2 * g[1][c] + f.c2y * g[2][c];
    H[6 + c] = g[2][c];
  }
  double ss = H[0] * H[0];
#pragma unroll
  for (int k = 1; k < 9; ++k) ss = ss + H[k] * H[k];
  const double scale = 1.0 / sqrt_rn(ss);
#pragma unroll
  for (int k = 0; k < 9; ++k) H[k] = H[k] * scale;
}

// The squared distance between the corner (x, y) warped by H and by G; NaN where a divisor is 0.
PR_FN double corner_sq(const double (&H)[9], const double* G, double x, double y) {
#pragma clang fp contract(off)
  const double a0 = (H[0] * x + H[1] * y) + H[2], a1 = (H[3] * x + H[4] * y) + H[5], a2 = (H[6] * x + H[7] * y) + H[8];
  const double b0 = (G[0] * x + G[1] * y) + G[2], b1 = (G[3] * x + G[4] * y) + G[5], b2 = (G[6] * x + G[7] * y) + G[8];
  const double pu = a0 / a2, pv = a1 / a2, qu = b0 / b2, qv = b1 / b2;
  const double d = (pu - qu) * (pu - qu) + (pv - qv) * (pv - qv);
  return (a2 == 0.0 || b2 == 0.0) ? nan64() : d;
}

}  // namespace hr
}  // namespace oetr
