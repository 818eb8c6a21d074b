// The arithmetic of oetr_pose_refit on the HOST: imagematching_oetr_amd/csrc/pose_refit_math.h (with pose_ransac_math.h
// and homography_ransac_math.h) - the one copy the kernel uses - compiled as plain C++, with the kernel's loops restated
// serially (a loop over the 256 "threads" of the workgroup, the butterfly over an array, the elimination's two steps
// over the 72 elements).  tests/test_pose_refit_cpu.py loads it and compares every round's candidate and count and
// every output with the numpy specification bit for bit, so a slip between the specification and the headers shows on
// a machine without a GPU.  One pair per call.
//
// Build (tools/README.md):  make -C imagematching_oetr_amd/csrc hostmath-pose_refit
#include <cstdint>
#include <stddef.h>

#include <vector>

#include "../imagematching_oetr_amd/csrc/pose_refit_math.h"

using namespace oetr;

namespace {

struct Rows {
  const double* P;
  const float *k1, *k2;
  void at(int j, double& x1, double& y1, double& x2, double& y2) const {
    rf::normalise(P, (double)k1[2 * j], (double)k1[2 * j + 1], (double)k2[2 * j], (double)k2[2 * j + 1], x1, y1, x2, y2);
  }
};

int count_inliers(const Rows& rows, int len, const double (&F)[9], double thr_sq) {
  int c = 0;
  for (int j = 0; j < len; ++j) {
    double x1, y1, x2, y2;
    rows.at(j, x1, y1, x2, y2);
    c += pr::inlier(F, x1, y1, x2, y2, thr_sq) ? 1 : 0;
  }
  return c;
}

// The fixed tree over 256 partial sums.
double tree_sum(const double* partials) {
#pragma clang fp contract(off)
  double v[rf::CLASSES], w[rf::CLASSES];
  for (int i = 0; i < rf::CLASSES; ++i) v[i] = partials[i];
  for (int o = 1; o < 64; o <<= 1) {
    for (int i = 0; i < rf::CLASSES; ++i) w[i] = v[i] + v[i ^ o];
    for (int i = 0; i < rf::CLASSES; ++i) v[i] = w[i];
  }
  return (v[0] + v[64]) + (v[128] + v[192]);
}

// The kernel's elimination: every "thread" e < 72 computes its element from the matrix of the step before.
bool eliminate(double (&A)[8][9]) {
  bool ok = true;
  for (int c = 0; c < 8; ++c) {
    double col[8], B[8][9];
    for (int r = 0; r < 8; ++r) col[r] = A[r][c];
    const int piv = hr::gj_pivot(A[c][c], col, c, ok);
    for (int e = 0; e < 72; ++e) {
      const int er = e / 9, ek = e - 9 * er;
      const int from = er == c ? piv : (er == piv ? c : er);
      const double mine = A[from][ek], a_ck = A[piv][ek], d = A[piv][c], f = A[from][c];
      B[er][ek] = ek > c ? hr::gj_element(er == c, mine, a_ck, d, f) : mine;
    }
    for (int r = 0; r < 8; ++r)
      for (int k = 0; k < 9; ++k) A[r][k] = B[r][k];
  }
  return ok;
}

}  // namespace

extern "C" {

double rf_host_tree_sum(const double* partials) { return tree_sum(partials); }

int rf_host_held_entry(const double* F) {
  double f[9];
  for (int k = 0; k < 9; ++k) f[k] = F[k];
  return rf::held_entry(f);
}

// One pair.  candidates [refit_iters][9] and candidate_counts [refit_iters]: every round's candidate and its count
// (-1: not finite), in order; *n_candidates of them are written.
void rf_host_refit(const double* P, const float* k1, const float* k2, int len, const double* model_in, double px_thr,
                   int refit_iters, double* model, double* pose, double* cosines, int32_t* counts, uint8_t* inliers,
                   double* candidates, int32_t* candidate_counts, int32_t* n_candidates) {
  const Rows rows{P, k1, k2};
  const double thr_sq = rf::thr_sq(P, px_thr);
  double cur[9];
  for (int k = 0; k < 9; ++k) cur[k] = model_in[k];
  const bool posed = len > 0 && pr::finite_model(cur);
  int count_in = 0, count = 0, accepted = 0, made = 0;               // the kernel's: no counting pass of its own
  for (int round = 0; posed && round < refit_iters; ++round) {
    std::vector<double> partial(rf::TERMS * rf::CLASSES, 0.0);     // [term][class]
    int n = 0;
    for (int tid = 0; tid < rf::CLASSES; ++tid) {
      double acc[rf::TERMS];
      for (int k = 0; k < rf::TERMS; ++k) acc[k] = 0.0;
      for (int j = tid; j < len; j += rf::CLASSES) {
        double x1, y1, x2, y2;
        rows.at(j, x1, y1, x2, y2);
        if (pr::inlier(cur, x1, y1, x2, y2, thr_sq)) {
          rf::add_row_terms(acc, x1, y1, x2, y2);
          n += 1;
        }
      }
      for (int k = 0; k < rf::TERMS; ++k) partial[(size_t)k * rf::CLASSES + tid] = acc[k];
    }
    double S[rf::TERMS];
    for (int k = 0; k < rf::TERMS; ++k) S[k] = tree_sum(&partial[(size_t)k * rf::CLASSES]);
    if (round == 0) count_in = count = n;
    if (n < rf::MIN_ROWS) break;
    const int held = rf::held_entry(cur);
    double A[8][9];
    for (int e = 0; e < 72; ++e) A[e / 9][e % 9] = rf::system_element(S, (double)n, held, e);
    if (!eliminate(A)) break;
    double cand[9];
    for (int i = 0; i < 9; ++i) {
      const int row = i - ((i >= held && i > 0) ? 1 : 0);
      cand[i] = i == held ? 1.0 : A[row][8];
    }
    rf::scale_candidate(cand);
    for (int k = 0; k < 9; ++k) candidates[9 * made + k] = cand[k];
    if (!pr::finite_model(cand)) {
      candidate_counts[made++] = -1;
      break;
    }
    const int c = count_inliers(rows, len, cand, thr_sq);
    candidate_counts[made++] = c;
    if (c < count) break;
    for (int k = 0; k < 9; ++k) cur[k] = cand[k];
    count = c;
    accepted += 1;
  }
  *n_candidates = made;

  double R1[9], R2[9], t[3];
  pr::decompose(cur, R1, R2, t);
  int votes[4] = {0, 0, 0, 0}, delivered = 0;
  for (int j = 0; j < len; ++j) {
    double x1, y1, x2, y2;
    rows.at(j, x1, y1, x2, y2);
    const bool in = posed && pr::inlier(cur, x1, y1, x2, y2, thr_sq);
    inliers[j] = in ? 1 : 0;
    if (in) {
      delivered += 1;
      double z1, z2;
      pr::depths(R1, t, x1, y1, x2, y2, z1, z2);
      votes[0] += (z1 > 0.0 && z2 > 0.0) ? 1 : 0;
      votes[1] += (-z1 > 0.0 && -z2 > 0.0) ? 1 : 0;
      pr::depths(R2, t, x1, y1, x2, y2, z1, z2);
      votes[2] += (z1 > 0.0 && z2 > 0.0) ? 1 : 0;
      votes[3] += (-z1 > 0.0 && -z2 > 0.0) ? 1 : 0;
    }
  }
  int chosen = 0, most = votes[0];
  for (int c = 1; c < 4; ++c)
    if (votes[c] > most) most = votes[c], chosen = c;
  double R[9], tc[3];
  for (int k = 0; k < 9; ++k) R[k] = chosen < 2 ? R1[k] : R2[k];
  for (int k = 0; k < 3; ++k) tc[k] = (chosen & 1) ? -t[k] : t[k];
  double cos_r, cos_t;
  pr::cosines(P + 8, P + 17, R, tc, cos_r, cos_t);
  for (int k = 0; k < 9; ++k) model[k] = posed ? cur[k] : pr::nan64(), pose[k] = posed ? R[k] : pr::nan64();
  for (int k = 0; k < 3; ++k) pose[9 + k] = posed ? tc[k] : pr::nan64();
  cosines[0] = posed ? cos_r : pr::nan64();
  cosines[1] = posed ? cos_t : pr::nan64();
  counts[0] = len, counts[1] = posed ? (refit_iters > 0 ? count_in : delivered) : 0, counts[2] = posed ? accepted : -1;
  counts[3] = posed ? delivered : 0;
  counts[4] = posed ? most : 0;
}

}  // extern "C"
