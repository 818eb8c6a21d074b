// The arithmetic of oetr_homography_ransac on the HOST: imagematching_oetr_amd/csrc/homography_ransac_math.h - the one
// copy the kernels use - compiled as plain C++, with the kernels' loops restated serially (a loop over the 256
// "threads" of the finishing workgroup, the butterfly over an array).  tests/test_homography_ransac_cpu.py loads it
// and compares every output with the numpy specification bit for bit, so a slip between the specification and the
// header shows on a machine without a GPU.  One pair per call.
//
// Build (tools/README.md):  make -C imagematching_oetr_amd/csrc hostmath-homography_ransac
#include <cstdint>
#include <stddef.h>

#include <vector>

#include "../imagematching_oetr_amd/csrc/homography_ransac_math.h"

using namespace oetr;

namespace {

struct Rows {
  const hr::Frames& f;
  const float *k1, *k2;
  void at(int j, double& x1, double& y1, double& x2, double& y2) const {
    hr::normalise(f, (double)k1[2 * j], (double)k1[2 * j + 1], (double)k2[2 * j], (double)k2[2 * j + 1], x1, y1, x2, y2);
  }
};

int count_inliers(const Rows& rows, int len, const double (&h)[9], double thr_sq, uint8_t* mark) {
  int c = 0;
  for (int j = 0; j < len; ++j) {
    double x1, y1, x2, y2;
    rows.at(j, x1, y1, x2, y2);
    const bool in = hr::inlier(h, x1, y1, x2, y2, thr_sq);
    c += in ? 1 : 0;
    if (mark) mark[j] = in ? 1 : 0;
  }
  return c;
}

}  // namespace

extern "C" {

// The fixed tree over 256 partial sums.
double hr_host_tree_sum(const double* partials) {
#pragma clang fp contract(off)
  double v[hr::CLASSES], w[hr::CLASSES];
  for (int i = 0; i < hr::CLASSES; ++i) v[i] = partials[i];
  for (int o = 1; o < 64; o <<= 1) {
    for (int i = 0; i < hr::CLASSES; ++i) w[i] = v[i] + v[i ^ o];
    for (int i = 0; i < hr::CLASSES; ++i) v[i] = w[i];
  }
  return (v[0] + v[64]) + (v[128] + v[192]);
}

void hr_host_sample(uint32_t seed, uint32_t pair_id, int n_hyp, uint32_t len, int64_t* idx) {
  for (int h = 0; h < n_hyp; ++h) {
    uint32_t s[hr::SAMPLE];
    hr::sample4(seed, pair_id, (uint32_t)h, len, s);
    for (int j = 0; j < hr::SAMPLE; ++j) idx[hr::SAMPLE * h + j] = s[j];
  }
}

// One pair.  models_in NULL: n_models hypotheses are sampled and solved.  models [n_models][9] and model_counts
// [n_models] are written either way (the workspace's view).
void hr_host_estimate(const double* P, const float* k1, const float* k2, int len, int n_models, uint32_t seed,
                      uint32_t pair_id, double px_thr, int refit_iters, const double* models_in, double* models,
                      int32_t* model_counts, double* model, double* H_out, double* corner_sq, int32_t* counts,
                      uint8_t* inliers) {
  const bool sized = hr::sizes_ok(P);
  const hr::Frames f = hr::frames(P);
  const Rows rows{f, k1, k2};
  const double thr_sq = hr::thr_sq(f, px_thr);
  for (int m = 0; m < n_models; ++m) {
    double out[9];
    if (models_in) {
      for (int k = 0; k < 9; ++k) out[k] = models_in[9 * m + k];
    } else if (len >= hr::SAMPLE && sized) {
      uint32_t idx[hr::SAMPLE];
      hr::sample4(seed, pair_id, (uint32_t)m, (uint32_t)len, idx);
      double X[hr::SAMPLE][4];
      for (int j = 0; j < hr::SAMPLE; ++j) rows.at((int)idx[j], X[j][0], X[j][1], X[j][2], X[j][3]);
      hr::solve4(X, out);
    } else {
      for (int k = 0; k < 9; ++k) out[k] = hr::nan64();
    }
    for (int k = 0; k < 9; ++k) models[9 * m + k] = out[k];
    model_counts[m] = (sized && hr::finite_model(out)) ? count_inliers(rows, len, out, thr_sq, nullptr) : -1;
  }
  int best = -1, at = -1, finite = 0;
  for (int m = 0; m < n_models; ++m) {
    finite += model_counts[m] >= 0 ? 1 : 0;
    if (model_counts[m] > best) best = model_counts[m], at = m;
  }
  const int selected = (sized && best >= 0) ? at : -1;
  const bool found = selected >= 0;
  double cur[9];
  for (int k = 0; k < 9; ++k) cur[k] = found ? models[9 * selected + k] : hr::nan64();
  int count = found ? best : 0, accepted = 0;
  for (int round = 0; found && round < refit_iters; ++round) {
    std::vector<double> partial(hr::TERMS * hr::CLASSES, 0.0);     // [term][class]
    int n = 0, first = INT32_MAX;
    for (int tid = 0; tid < hr::CLASSES; ++tid) {
      double acc[hr::TERMS];
      for (int k = 0; k < hr::TERMS; ++k) acc[k] = 0.0;
      for (int j = tid; j < len; j += hr::CLASSES) {
        double x1, y1, x2, y2;
        rows.at(j, x1, y1, x2, y2);
        if (hr::inlier(cur, x1, y1, x2, y2, thr_sq)) {
          hr::add_row_terms(acc, x1, y1, x2, y2);
          n += 1;
          first = j < first ? j : first;
        }
      }
      for (int k = 0; k < hr::TERMS; ++k) partial[(size_t)k * hr::CLASSES + tid] = acc[k];
    }
    double S[hr::TERMS];
    for (int k = 0; k < hr::TERMS; ++k) S[k] = hr_host_tree_sum(&partial[(size_t)k * hr::CLASSES]);
    if (n < hr::SAMPLE) break;
    double cand[9];
    bool ok = hr::solve8(S, (double)n, cand);
    double fx, fy, fx2, fy2;
    rows.at(first, fx, fy, fx2, fy2);
    hr::unit_and_sign(cand, fx, fy);
    ok = ok && hr::finite_model(cand);
    if (!ok) break;
    const int c = count_inliers(rows, len, cand, thr_sq, nullptr);
    if (c < count) break;
    for (int k = 0; k < 9; ++k) cur[k] = cand[k];
    count = c;
    accepted += 1;
  }
  for (int j = 0; j < len; ++j) inliers[j] = 0;
  if (found) count_inliers(rows, len, cur, thr_sq, inliers);
  double H[9];
  hr::deliver(cur, f, H);
  const double w = P[9] - 1.0, h = P[10] - 1.0;
  for (int k = 0; k < 9; ++k) model[k] = cur[k], H_out[k] = found ? H[k] : hr::nan64();
  corner_sq[0] = found ? hr::corner_sq(H, P, 0.0, 0.0) : hr::nan64();
  corner_sq[1] = found ? hr::corner_sq(H, P, w, 0.0) : hr::nan64();
  corner_sq[2] = found ? hr::corner_sq(H, P, w, h) : hr::nan64();
  corner_sq[3] = found ? hr::corner_sq(H, P, 0.0, h) : hr::nan64();
  counts[0] = sized ? len : -1, counts[1] = sized ? finite : -1, counts[2] = selected;
  counts[3] = sized ? (found ? best : 0) : -1, counts[4] = sized ? count : -1, counts[5] = sized ? accepted : -1;
}

}  // extern "C"
