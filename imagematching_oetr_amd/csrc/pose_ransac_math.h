// The arithmetic of the relative-pose entry (include/oetr_pose_ransac.h), one copy for every kernel of
// pose_ransac.hip: tests/pose_ransac_oracle.py LITERALLY - float64, every operation rounded on its own in the order
// and with the parentheses written there, IEEE division and square root, no contraction into FMAs, every decision a
// comparison.  Plain C++ (no HIP types), so the same text also compiles for the host.  Arrays are indexed by
// compile-time constants after unrolling: nothing here needs scratch memory.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define PR_FN __host__ __device__ __forceinline__
#else
#define PR_FN inline
#endif

namespace oetr {
namespace pr {

constexpr int SAMPLE = 7;                 // rows of a minimal sample
constexpr int ROOTS = 3;                  // models of a hypothesis
constexpr int BISECTIONS = 80;            // per root, fixed
constexpr int SWEEPS = 10;                // of the one-sided Jacobi SVD, fixed

PR_FN double nan64() { return __builtin_nan(""); }
// the specification's np.sqrt: correctly rounded
PR_FN double sqrt_rn(double x) { return __builtin_sqrt(x); }
PR_FN double abs64(double x) { return __builtin_fabs(x); }
PR_FN bool finite64(double x) { return (x - x) == 0.0; }

// ------------------------------------------------------------------ sampling
PR_FN uint32_t mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

PR_FN uint32_t draw_bits(uint32_t seed, uint32_t pair_id, uint32_t h, uint32_t j) {
  uint32_t x = mix32(seed + 0x9e3779b9u);
  x = mix32(x ^ pair_id);
  x = mix32(x ^ h);
  return mix32(x ^ j);
}

// 7 distinct rows of a list of `len` >= 7 rows, ascending; every idx[j] < len.
PR_FN void sample7(uint32_t seed, uint32_t pair_id, uint32_t h, uint32_t len, uint32_t (&idx)[SAMPLE]) {
#pragma unroll
  for (int j = 0; j < SAMPLE; ++j) {
    const uint64_t range = (uint64_t)(len - (uint32_t)j);
    uint32_t v = (uint32_t)(((uint64_t)draw_bits(seed, pair_id, h, (uint32_t)j) * range) >> 32);   // < len - j
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

// ------------------------------------------------------------------ the 7-point solver
PR_FN double det3(double a0, double a1, double a2, double b0, double b1, double b2, double c0, double c1, double c2) {
#pragma clang fp contract(off)
  return (a0 * (b1 * c2 - b2 * c1) - a1 * (b0 * c2 - b2 * c0)) + a2 * (b0 * c1 - b1 * c0);
}

PR_FN double cubic(double a, double b, double c, double x) {
#pragma clang fp contract(off)
  return ((x + a) * x + b) * x + c;
}

// X[r] = (x1, y1, x2, y2) of the sample's row r, normalised.  out[root] = a model (row major) or all NaN.
PR_FN void solve7(const double (&X)[SAMPLE][4], double (&out)[ROOTS][9]) {
#pragma clang fp contract(off)
  double A[SAMPLE][9];
#pragma unroll
  for (int r = 0; r < SAMPLE; ++r) {
    const double x1 = X[r][0], y1 = X[r][1], x2 = X[r][2], y2 = X[r][3];
    A[r][0] = x2 * x1, A[r][1] = x2 * y1, A[r][2] = x2;
    A[r][3] = y2 * x1, A[r][4] = y2 * y1, A[r][5] = y2;
    A[r][6] = x1, A[r][7] = y1, A[r][8] = 1.0;
  }
  bool ok = true;
#pragma unroll
  for (int c = 0; c < SAMPLE; ++c) {
    double best = abs64(A[c][c]);
    int piv = c;
#pragma unroll
    for (int r = c + 1; r < SAMPLE; ++r) {
      const double v = abs64(A[r][c]);
      const bool take = v > best;                                   // the lowest index wins a tie
      best = take ? v : best;
      piv = take ? r : piv;
    }
    ok = ok && (best > 0.0);                                        // false for a NaN pivot, too
#pragma unroll
    for (int r = c + 1; r < SAMPLE; ++r) {
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
    for (int k = c + 1; k < 9; ++k) A[c][k] = A[c][k] / d;
#pragma unroll
    for (int r = 0; r < SAMPLE; ++r) {
      if (r == c) continue;
      const double f = A[r][c];
#pragma unroll
      for (int k = c + 1; k < 9; ++k) A[r][k] = A[r][k] - f * A[c][k];
    }
  }
  // the two null vectors, and F(l) = F2 + l * D with D = F1 - F2
  double F2[9], D[9];
#pragma unroll
  for (int r = 0; r < SAMPLE; ++r) {
    const double f1 = -A[r][7], f2 = -A[r][8];
    F2[r] = f2;
    D[r] = f1 - f2;
  }
  F2[7] = 0.0, F2[8] = 1.0;
  D[7] = 1.0, D[8] = -1.0;

  const double c0 = det3(F2[0], F2[1], F2[2], F2[3], F2[4], F2[5], F2[6], F2[7], F2[8]);
  const double c3 = det3(D[0], D[1], D[2], D[3], D[4], D[5], D[6], D[7], D[8]);
  const double c1 = (det3(D[0], D[1], D[2], F2[3], F2[4], F2[5], F2[6], F2[7], F2[8]) +
                     det3(F2[0], F2[1], F2[2], D[3], D[4], D[5], F2[6], F2[7], F2[8])) +
                    det3(F2[0], F2[1], F2[2], F2[3], F2[4], F2[5], D[6], D[7], D[8]);
  const double c2 = (det3(F2[0], F2[1], F2[2], D[3], D[4], D[5], D[6], D[7], D[8]) +
                     det3(D[0], D[1], D[2], F2[3], F2[4], F2[5], D[6], D[7], D[8])) +
                    det3(D[0], D[1], D[2], D[3], D[4], D[5], F2[6], F2[7], F2[8]);

  const bool at_infinity = c3 == 0.0;                               // the root at infinity: F = D alone
  const double a = c2 / c3, b = c1 / c3, c = c0 / c3;               // monic
  double big = abs64(a);
  big = abs64(b) > big ? abs64(b) : big;
  big = abs64(c) > big ? abs64(c) : big;
  const double M = 1.0 + big;                                       // Cauchy's bound on every root
  const double disc = a * a - 3.0 * b;
  const bool three = disc > 0.0;                                    // two turning points l1 < l2
  const double sq = sqrt_rn(three ? disc : 0.0);
  const double l1 = (-a - sq) / 3.0, l2 = (-a + sq) / 3.0;
  const double p1 = cubic(a, b, c, l1), p2 = cubic(a, b, c, l2);
  const bool has1 = three ? p1 >= 0.0 : true;                       // in [-M, l1] (monotone cubic: in [-M, M])
  const bool has2 = three && p1 > 0.0 && p2 < 0.0;                  // in [l1, l2], falling
  const bool has3 = three && p2 <= 0.0;                             // in [l2, M]
  double lo[ROOTS] = {-M, l1, l2};
  double hi[ROOTS] = {three ? l1 : M, l2, M};
  for (int it = 0; it < BISECTIONS; ++it) {
#pragma unroll
    for (int k = 0; k < ROOTS; ++k) {
      const double mid = 0.5 * (lo[k] + hi[k]);
      const double pm = cubic(a, b, c, mid);
      const bool upper = k == 1 ? pm < 0.0 : pm > 0.0;              // the root lies below mid
      hi[k] = upper ? mid : hi[k];
      lo[k] = upper ? lo[k] : mid;
    }
  }
  const double r1 = 0.5 * (lo[0] + hi[0]), r2 = 0.5 * (lo[1] + hi[1]), r3 = 0.5 * (lo[2] + hi[2]);
  // the real roots in ascending order (has2 implies has1 and has3)
  double root[ROOTS];
  bool have[ROOTS];
  root[0] = has1 ? r1 : r3;
  have[0] = has1 || has3;
  root[1] = has2 ? r2 : r3;
  have[1] = has1 && (has2 || has3);
  root[2] = r3;
  have[2] = has1 && has2 && has3;
#pragma unroll
  for (int s = 0; s < ROOTS; ++s) {
    const bool use = ok && (at_infinity ? s == 0 : have[s]);
    double F[9];
    bool fin = use;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      F[k] = at_infinity ? D[k] : F2[k] + root[s] * D[k];
      fin = fin && finite64(F[k]);
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) out[s][k] = fin ? F[k] : nan64();
  }
}

// ------------------------------------------------------------------ scoring
// Sampson's test of one row under F without the division; false for NaN and for a zero denominator.
PR_FN bool inlier(const double (&F)[9], double x1, double y1, double x2, double y2, double thr_sq) {
#pragma clang fp contract(off)
  const double a0 = (F[0] * x1 + F[1] * y1) + F[2];
  const double a1 = (F[3] * x1 + F[4] * y1) + F[5];
  const double a2 = (F[6] * x1 + F[7] * y1) + F[8];
  const double b0 = (F[0] * x2 + F[3] * y2) + F[6];
  const double b1 = (F[1] * x2 + F[4] * y2) + F[7];
  const double s = (x2 * a0 + y2 * a1) + a2;
  return s * s < thr_sq * ((a0 * a0 + a1 * a1) + (b0 * b0 + b1 * b1));
}

PR_FN bool finite_model(const double (&F)[9]) {
  bool fin = true;
#pragma unroll
  for (int k = 0; k < 9; ++k) fin = fin && finite64(F[k]);
  return fin;
}

// ------------------------------------------------------------------ decomposition
// F -> the two rotations (row major, determinant +1) and the unit translation of the essential-matrix decomposition,
// through a one-sided Jacobi SVD F V = U S with a fixed number of sweeps.
PR_FN void decompose(const double (&F)[9], double (&R1)[9], double (&R2)[9], double (&t)[3]) {
#pragma clang fp contract(off)
  double a[3][3], v[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) a[i][j] = F[3 * i + j], v[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < SWEEPS; ++sweep) {
#pragma unroll
    for (int pq = 0; pq < 3; ++pq) {
      const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;           // (0,1) (0,2) (1,2)
      const double alpha = (a[0][p] * a[0][p] + a[1][p] * a[1][p]) + a[2][p] * a[2][p];
      const double beta = (a[0][q] * a[0][q] + a[1][q] * a[1][q]) + a[2][q] * a[2][q];
      const double gamma = (a[0][p] * a[0][q] + a[1][p] * a[1][q]) + a[2][p] * a[2][q];
      const bool rot = gamma != 0.0;
      const double zeta = (beta - alpha) / (2.0 * gamma);
      const double tm = 1.0 / (abs64(zeta) + sqrt_rn(1.0 + zeta * zeta));
      const double tt = zeta < 0.0 ? -tm : tm;
      const double cc = 1.0 / sqrt_rn(1.0 + tt * tt);
      const double c = rot ? cc : 1.0, s = rot ? cc * tt : 0.0;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const double ap = a[i][p], aq = a[i][q], vp = v[i][p], vq = v[i][q];
        a[i][p] = c * ap - s * aq;
        a[i][q] = s * ap + c * aq;
        v[i][p] = c * vp - s * vq;
        v[i][q] = s * vp + c * vq;
      }
    }
  }
  double n[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) n[j] = (a[0][j] * a[0][j] + a[1][j] * a[1][j]) + a[2][j] * a[2][j];
  // the two largest singular values first: three compare-and-swaps of columns
#pragma unroll
  for (int pq = 0; pq < 3; ++pq) {
    const int p = pq == 1 ? 1 : 0, q = pq == 1 ? 2 : 1;             // (0,1) (1,2) (0,1)
    const bool sw = n[p] < n[q];
    const double np_ = n[p], nq_ = n[q];
    n[p] = sw ? nq_ : np_;
    n[q] = sw ? np_ : nq_;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const double ap = a[i][p], aq = a[i][q], vp = v[i][p], vq = v[i][q];
      a[i][p] = sw ? aq : ap;
      a[i][q] = sw ? ap : aq;
      v[i][p] = sw ? vq : vp;
      v[i][q] = sw ? vp : vq;
    }
  }
  const double s1 = sqrt_rn(n[0]), s2 = sqrt_rn(n[1]);
  double u1[3], u2[3], u3[3], v1[3], v2[3], v3[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) u1[i] = a[i][0] / s1, u2[i] = a[i][1] / s2, v1[i] = v[i][0], v2[i] = v[i][1];
  // the third columns as cross products: both determinants +1
  u3[0] = u1[1] * u2[2] - u1[2] * u2[1];
  u3[1] = u1[2] * u2[0] - u1[0] * u2[2];
  u3[2] = u1[0] * u2[1] - u1[1] * u2[0];
  v3[0] = v1[1] * v2[2] - v1[2] * v2[1];
  v3[1] = v1[2] * v2[0] - v1[0] * v2[2];
  v3[2] = v1[0] * v2[1] - v1[1] * v2[0];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      R1[3 * i + j] = (u2[i] * v1[j] - u1[i] * v2[j]) + u3[i] * v3[j];       // U W V^T
      R2[3 * i + j] = (u1[i] * v2[j] - u2[i] * v1[j]) + u3[i] * v3[j];       // U W^T V^T
    }
    t[i] = u3[i];
  }
}

// The depths (z1, z2) of one row under (R, t): the least-squares solution of z2 * x2 - z1 * R x1 = t.
PR_FN void depths(const double (&R)[9], const double (&t)[3], double x1, double y1, double x2, double y2, double& z1,
                  double& z2) {
#pragma clang fp contract(off)
  const double r0 = (R[0] * x1 + R[1] * y1) + R[2];
  const double r1 = (R[3] * x1 + R[4] * y1) + R[5];
  const double r2 = (R[6] * x1 + R[7] * y1) + R[8];
  const double A = (x2 * x2 + y2 * y2) + 1.0;
  const double B = (x2 * r0 + y2 * r1) + r2;
  const double C = (r0 * r0 + r1 * r1) + r2 * r2;
  const double Dd = (x2 * t[0] + y2 * t[1]) + t[2];
  const double E = (r0 * t[0] + r1 * t[1]) + r2 * t[2];
  const double det = A * C - B * B;
  z2 = (Dd * C - B * E) / det;
  z1 = (B * Dd - A * E) / det;
}

// cos_R = (trace(R_gt^T R) - 1) / 2 and cos_t = (t . t_gt) / (|t| |t_gt|), unclipped.
PR_FN void cosines(const double* Rg, const double* tg, const double (&R)[9], const double (&t)[3], double& cos_r,
                   double& cos_t) {
#pragma clang fp contract(off)
  double tr = Rg[0] * R[0];
#pragma unroll
  for (int k = 1; k < 9; ++k) tr = tr + Rg[k] * R[k];
  cos_r = (tr - 1.0) / 2.0;
  const double dot = (t[0] * tg[0] + t[1] * tg[1]) + t[2] * tg[2];
  const double tt = (t[0] * t[0] + t[1] * t[1]) + t[2] * t[2];
  const double gg = (tg[0] * tg[0] + tg[1] * tg[1]) + tg[2] * tg[2];
  cos_t = dot / (sqrt_rn(tt) * sqrt_rn(gg));
}

}  // namespace pr
}  // namespace oetr
