// The arithmetic of the pose-refit entry (include/oetr_pose_refit.h) that pose_ransac_math.h and
// homography_ransac_math.h do not already hold: tests/pose_refit_oracle.py LITERALLY - float64, every operation
// rounded on its own in the order and with the parentheses written there, no contraction into FMAs, every decision a
// comparison.  Sampson's test, the decomposition, the depths and the cosines are pr::'s, the two steps of the
// elimination are hr::gj_pivot / hr::gj_element: the arithmetic stays one copy.  Added here: a row's 44 terms, the
// held entry, the assembly of the 8 x 9 system and the candidate's scaling - and the normalisation of a row, which
// pose_ransac.hip keeps to itself.  Plain C++ (no HIP types), so the same text also compiles for the host
// (tools/pose_refit_hostmath.cpp).
#pragma once
#include <cstdint>

#include "homography_ransac_math.h"
#include "pose_ransac_math.h"

namespace oetr {
namespace rf {

using pr::abs64;
using pr::nan64;
using pr::sqrt_rn;

constexpr int TERMS = 44;                 // floating-point sums of one round
constexpr int PRODUCTS = 36;              // of them, sums of products: the upper triangle of the leading 8 x 8
constexpr int MIN_ROWS = 8;               // a round needs that many inlier rows
constexpr int CLASSES = hr::CLASSES;      // partial sums of each: the list position modulo 256

// ------------------------------------------------------------------ normalisation (pro.normalise)
PR_FN void normalise(const double* P, double u1, double v1, double u2, double v2, double& x1, double& y1, double& x2,
                     double& y2) {
#pragma clang fp contract(off)
  x1 = (u1 - P[2]) / P[0], y1 = (v1 - P[3]) / P[1];
  x2 = (u2 - P[6]) / P[4], y2 = (v2 - P[7]) / P[5];
}

PR_FN double thr_sq(const double* P, double px_thr) {
#pragma clang fp contract(off)
  const double thr_n = px_thr / ((P[0] + P[5]) / 2.0);           // the reference's f_mean: K0[0,0] and K1[1,1] only
  return thr_n * thr_n;
}

// ------------------------------------------------------------------ the sums
// acc[k] = acc[k] + term k of one row (row_terms): w_i * w_j for i <= j < 8, row major, then w_0 .. w_7.
PR_FN void add_row_terms(double (&acc)[TERMS], double x1, double y1, double x2, double y2) {
#pragma clang fp contract(off)
  const double w[8] = {x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1};
  int at = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
#pragma unroll
    for (int j = i; j < 8; ++j) {
      acc[at] = acc[at] + w[i] * w[j];
      ++at;
    }
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[PRODUCTS + i] = acc[PRODUCTS + i] + w[i];
}

// Where M[i][j] lives among the sums (0 <= i, j <= 8); TERMS for M[8][8], the count of the rows.
PR_FN int moment_index(int i, int j) {
  const int lo = i < j ? i : j, hi = i < j ? j : i;
  if (hi == 8) return lo == 8 ? TERMS : PRODUCTS + lo;
  return (8 * lo - (lo * (lo - 1)) / 2) + (hi - lo);
}

// ------------------------------------------------------------------ the system
// The held entry: the largest |F[i]|, the lowest index on a tie.
PR_FN int held_entry(const double (&F)[9]) {
  double best = abs64(F[0]);
  int k = 0;
#pragma unroll
  for (int i = 1; i < 9; ++i) {
    const double v = abs64(F[i]);
    const bool take = v > best;
    best = take ? v : best;
    k = take ? i : k;
  }
  return k;
}

// Unknown r (0..7) of the system is entry `entry_of(r, k)` of the model: the entries without k, ascending.
PR_FN int entry_of(int r, int k) { return r + (r >= k ? 1 : 0); }

// Element e = 9 * row + column of the augmented 8 x 9 system: rows and columns of M without k, the right-hand side
// -M[:, k].  S: the 44 sums (any memory the caller can index at run time), n: the count.
PR_FN double system_element(const double* S, double n, int k, int e) {
  const int r = e / 9, c = e - 9 * r;
  const int at = moment_index(entry_of(r, k), c == 8 ? k : entry_of(c, k));
  const double v = at == TERMS ? n : S[at < TERMS ? at : 0];
  return c == 8 ? -v : v;
}

// The candidate (the eight solutions with 1 at k) scaled by 1 / sqrt(sum of squares, added in entry order).
PR_FN void scale_candidate(double (&cand)[9]) {
#pragma clang fp contract(off)
  double ss = cand[0] * cand[0];
#pragma unroll
  for (int i = 1; i < 9; ++i) ss = ss + cand[i] * cand[i];
  const double scale = 1.0 / sqrt_rn(ss);
#pragma unroll
  for (int i = 0; i < 9; ++i) cand[i] = cand[i] * scale;
}

}  // namespace rf
}  // namespace oetr
