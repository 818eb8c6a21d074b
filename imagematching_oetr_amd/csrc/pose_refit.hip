// A least-squares refit of relative poses on their inliers (include/oetr_pose_refit.h).  The kernel runs
// tests/pose_refit_oracle.py LITERALLY; the arithmetic is pose_refit_math.h on top of pose_ransac_math.h and
// homography_ransac_math.h (float64, every operation rounded on its own, no contraction into FMAs, IEEE division and
// square root).
//
// k_pr_refit: ONE kernel, one workgroup of 256 threads per pair, the shape of k_hr_finish.  Every thread holds the
// current model in registers; every value a decision rests on is uniform over the workgroup.  A round: thread t adds
// the 44 terms of the inlier rows t, t + 256, ... of the list (the 256 partial sums of the specification, in
// registers), the partials are summed by the specified tree - an xor butterfly of lane shuffles within each of the four
// waves, the four wave values through LDS as (w0 + w1) + (w2 + w3) -, the 8 x 9 system is assembled and eliminated in
// LDS with one thread per element (hr::gj_pivot / hr::gj_element: every thread takes the same pivot decisions from the
// same LDS values), the candidate is scored over all rows by all threads, the counts added as integers, and accepted
// or not.  model_in's own inliers cost no pass: the first round counts them as it adds their terms.  Then k_pr_pose's
// tail: the decomposition by every thread alike, ONE pass over the rows that writes `inliers`, counts the delivered
// model's inliers and takes the four cheirality votes through integer LDS atomics, the outputs by thread 0.  Every output element is
// written by exactly one thread.
#include <string>

#include "../../include/oetr_pose_refit.h"
#include "common.h"
#include "pose_refit_math.h"

namespace oetr {

constexpr int RF_PARAMS = OETR_MATCH_SCORE_PARAM_DOUBLES;
constexpr int RF_THREADS = 256;                                    // rf::CLASSES
constexpr int RF_WAVES = RF_THREADS / 64;
constexpr int RF_COUNTERS = OETR_POSE_REFIT_COUNTERS;
static_assert(RF_THREADS == rf::CLASSES && RF_WAVES == 4, "the refit's tree is written for four waves of 64");

// The list of pair p: first row and length, both offsets clamped into [0, n_matches] (start + len <= n_matches).
__device__ __forceinline__ void rf_list(const int32_t* __restrict__ offsets, int p, int n_matches, int& start, int& len) {
  int a = offsets[p], b = offsets[p + 1];
  a = a < 0 ? 0 : (a > n_matches ? n_matches : a);
  b = b < 0 ? 0 : (b > n_matches ? n_matches : b);
  start = a;
  len = b > a ? b - a : 0;
}

// Row m < n_matches, normalised: (x1, y1, x2, y2).
__device__ __forceinline__ void rf_row(const double* __restrict__ P, const float* __restrict__ k1,
                                       const float* __restrict__ k2, int m, double& x1, double& y1, double& x2,
                                       double& y2) {
  const size_t at = 2 * (size_t)m;
  rf::normalise(P, (double)k1[at], (double)k1[at + 1], (double)k2[at], (double)k2[at + 1], x1, y1, x2, y2);
}

// The sum of an int over the workgroup.  `s`: RF_WAVES ints of LDS nobody else uses between the two barriers inside.
__device__ __forceinline__ int rf_sum_int(int v, int* s) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();                                                  // the last readers of `s` are through
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  return (s[0] + s[1]) + (s[2] + s[3]);
}

// The inliers of F over the rows of the list, over the workgroup.
__device__ __forceinline__ int rf_count(const double (&F)[9], const double* __restrict__ P,
                                        const float* __restrict__ k1, const float* __restrict__ k2, int start, int len,
                                        double thr_sq, int* s) {
  int c = 0;
  for (int j = (int)threadIdx.x; j < len; j += RF_THREADS) {
    double x1, y1, x2, y2;
    rf_row(P, k1, k2, start + j, x1, y1, x2, y2);
    c += pr::inlier(F, x1, y1, x2, y2, thr_sq) ? 1 : 0;
  }
  return rf_sum_int(c, s);
}

__global__ __launch_bounds__(RF_THREADS) void k_pr_refit(
    const double* __restrict__ params, const int32_t* __restrict__ offsets, int n_pairs, const float* __restrict__ k1,
    const float* __restrict__ k2, int n_matches, const double* __restrict__ model_in, double px_thr, int refit_iters,
    double* __restrict__ model, double* __restrict__ pose, double* __restrict__ cosines, int32_t* __restrict__ counts,
    uint8_t* __restrict__ inliers) {
#pragma clang fp contract(off)
  __shared__ double s_sum[RF_WAVES][rf::TERMS], s_tot[rf::TERMS], s_A[8][9];
  __shared__ int s_int[RF_WAVES], s_votes[5];                       // four cheirality votes, the delivered model's inliers
  const int p = blockIdx.x, tid = threadIdx.x;
  const double* __restrict__ P = params + (size_t)p * RF_PARAMS;
  int start, len;
  rf_list(offsets, p, n_matches, start, len);
  const double thr_sq = rf::thr_sq(P, px_thr);
  if (tid < 5) s_votes[tid] = 0;
  __syncthreads();                                                  // before the last pass adds to them, rounds or none

  double cur[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) cur[k] = model_in[9 * (size_t)p + k];
  const bool posed = len > 0 && pr::finite_model(cur);              // uniform over the workgroup
  // The inliers of model_in need no pass of their own: the first round counts them while it adds their terms, and
  // without a round the delivered model IS model_in, whose inliers the last pass counts.
  int count_in = 0, count = 0, accepted = 0;

  // the refit: a fixed number of rounds, every decision uniform over the workgroup
#pragma nounroll
  for (int round = 0; posed && round < refit_iters; ++round) {
    double acc[rf::TERMS];
#pragma unroll
    for (int k = 0; k < rf::TERMS; ++k) acc[k] = 0.0;
    int n = 0;
    for (int j = tid; j < len; j += RF_THREADS) {                   // partial sum `tid`: positions tid, tid + 256, ...
      double x1, y1, x2, y2;
      rf_row(P, k1, k2, start + j, x1, y1, x2, y2);
      if (pr::inlier(cur, x1, y1, x2, y2, thr_sq)) {
        rf::add_row_terms(acc, x1, y1, x2, y2);
        n += 1;
      }
    }
    // the tree: an xor butterfly within the wave (all 64 lanes end equal), then (w0 + w1) + (w2 + w3)
#pragma unroll
    for (int k = 0; k < rf::TERMS; ++k) {
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) acc[k] = acc[k] + __shfl_xor(acc[k], o, 64);
    }
    __syncthreads();                                                // the last round's readers of s_sum are through
    if ((tid & 63) == 0) {
#pragma unroll
      for (int k = 0; k < rf::TERMS; ++k) s_sum[tid >> 6][k] = acc[k];
    }
    __syncthreads();
    if (tid < rf::TERMS) s_tot[tid] = (s_sum[0][tid] + s_sum[1][tid]) + (s_sum[2][tid] + s_sum[3][tid]);
    n = rf_sum_int(n, s_int);                                       // (its barriers publish s_tot, too)
    if (round == 0) count_in = count = n;                           // later rounds: n == count, the candidate's score
    if (n < rf::MIN_ROWS) break;
    // the system and its elimination, spread over the workgroup: thread e < 72 owns element (e / 9, e % 9); the matrix
    // lives in LDS between the steps; every thread takes the same pivot decisions from the same LDS values
    const int held = rf::held_entry(cur);                           // 0 <= held < 9
    const bool owner = tid < 72;
    const int er = owner ? tid / 9 : 0, ek = owner ? tid - 9 * er : 0;
    double a = rf::system_element(s_tot, (double)n, held, owner ? tid : 0);      // indices 0..43 of s_tot
    bool ok = true;
#pragma nounroll
    for (int c = 0; c < 8; ++c) {
      if (owner) s_A[er][ek] = a;
      __syncthreads();
      double col[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) col[r] = s_A[r][c];
      const int piv = hr::gj_pivot(s_A[c][c], col, c, ok);          // c <= piv < 8
      // after the swap of rows c and piv: row c is the old row piv
      const int from = er == c ? piv : (er == piv ? c : er);
      const double mine = s_A[from][ek], a_ck = s_A[piv][ek], d = s_A[piv][c], f = s_A[from][c];
      a = ek > c ? hr::gj_element(er == c, mine, a_ck, d, f) : mine;
      __syncthreads();                                              // every read of this step is through
    }
    if (owner) s_A[er][ek] = a;
    __syncthreads();
    if (!ok) break;                                                 // a zero or NaN pivot: no candidate
    double cand[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      const int row = i - ((i >= held && i > 0) ? 1 : 0);               // 0..7 whatever `held`: unknown i, or i - 1 past it
      cand[i] = i == held ? 1.0 : s_A[row][8];
    }
    rf::scale_candidate(cand);
    if (!pr::finite_model(cand)) break;
    const int c = rf_count(cand, P, k1, k2, start, len, thr_sq, s_int);
    if (c < count) break;
#pragma unroll
    for (int k = 0; k < 9; ++k) cur[k] = cand[k];
    count = c;
    accepted += 1;
  }

  // k_pr_pose's tail under the delivered model
  double R1[9], R2[9], t[3];
  pr::decompose(cur, R1, R2, t);
  int votes[4] = {0, 0, 0, 0}, delivered = 0;
  for (int j = tid; j < len; j += RF_THREADS) {
    double x1, y1, x2, y2;
    rf_row(P, k1, k2, start + j, x1, y1, x2, y2);
    const bool in = posed && pr::inlier(cur, x1, y1, x2, y2, thr_sq);
    if (inliers) inliers[(size_t)(start + j)] = in ? 1 : 0;
    if (in) {
      delivered += 1;
      double z1, z2;
      pr::depths(R1, t, x1, y1, x2, y2, z1, z2);
      votes[0] += (z1 > 0.0 && z2 > 0.0) ? 1 : 0;
      votes[1] += (-z1 > 0.0 && -z2 > 0.0) ? 1 : 0;                 // (R1, -t): both depths change sign, exactly
      pr::depths(R2, t, x1, y1, x2, y2, z1, z2);
      votes[2] += (z1 > 0.0 && z2 > 0.0) ? 1 : 0;
      votes[3] += (-z1 > 0.0 && -z2 > 0.0) ? 1 : 0;
    }
  }
  // rows outside every list: before the first list and after the last one (the offsets are non-decreasing)
  if (inliers && p == 0)
    for (int j = tid; j < start; j += RF_THREADS) inliers[(size_t)j] = 0;
  if (inliers && p == n_pairs - 1)
    for (int j = start + len + tid; j < n_matches; j += RF_THREADS) inliers[(size_t)j] = 0;
#pragma unroll
  for (int c = 0; c < 4; ++c)
    if (votes[c]) atomicAdd(&s_votes[c], votes[c]);
  if (delivered) atomicAdd(&s_votes[4], delivered);
  __syncthreads();
  if (tid != 0) return;

  int chosen = 0, most = s_votes[0];
#pragma unroll
  for (int c = 1; c < 4; ++c)
    if (s_votes[c] > most) most = s_votes[c], chosen = c;
  double R[9], tc[3];
#pragma unroll
  for (int k = 0; k < 9; ++k) R[k] = chosen < 2 ? R1[k] : R2[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) tc[k] = (chosen & 1) ? -t[k] : t[k];
  double cos_r, cos_t;
  pr::cosines(P + 8, P + 17, R, tc, cos_r, cos_t);
  double* mo = model + 9 * (size_t)p;
  double* po = pose + 12 * (size_t)p;
#pragma unroll
  for (int k = 0; k < 9; ++k) mo[k] = posed ? cur[k] : pr::nan64(), po[k] = posed ? R[k] : pr::nan64();
#pragma unroll
  for (int k = 0; k < 3; ++k) po[9 + k] = posed ? tc[k] : pr::nan64();
  cosines[2 * (size_t)p] = posed ? cos_r : pr::nan64();
  cosines[2 * (size_t)p + 1] = posed ? cos_t : pr::nan64();
  int32_t* co = counts + RF_COUNTERS * (size_t)p;
  delivered = s_votes[4];                                           // == count whenever a round ran
  co[0] = len, co[1] = posed ? (refit_iters > 0 ? count_in : delivered) : 0, co[2] = posed ? accepted : -1;
  co[3] = posed ? delivered : 0;
  co[4] = posed ? most : 0;
}

}  // namespace oetr

using namespace oetr;

extern "C" {

int oetr_pose_refit_abi_version(void) { return OETR_POSE_REFIT_ABI_VERSION; }

// The host code dereferences none of its pointer arguments and reads nothing from the device.
oetr_status oetr_pose_refit(const double* params, const int32_t* offsets, int n_pairs, const float* k1, const float* k2,
                            int64_t n_matches, const double* model_in, double px_thr, int refit_iters, double* model,
                            double* pose, double* cosines, int32_t* counts, uint8_t* inliers, void* stream) {
  const char* me = "oetr_pose_refit";
  if (!params || !offsets) return entry_fail(me, OETR_ERR_BAD_ARG, "NULL parameter / offsets pointer");
  if (!model_in) return entry_fail(me, OETR_ERR_BAD_ARG, "NULL model_in pointer");
  if (!model || !pose || !cosines || !counts)
    return entry_fail(me, OETR_ERR_BAD_ARG, "NULL model / pose / cosines / counts output");
  if (n_matches != 0 && (!k1 || !k2)) return entry_fail(me, OETR_ERR_BAD_ARG, "NULL keypoint pointer");
  if (n_pairs <= 0) return entry_fail(me, OETR_ERR_BAD_ARG, "need n_pairs > 0");
  if (n_matches < 0) return entry_fail(me, OETR_ERR_BAD_ARG, "need n_matches >= 0");
  if (refit_iters < 0 || refit_iters > OETR_POSE_REFIT_MAX_ITERS)
    return entry_fail(me, OETR_ERR_BAD_ARG, "need 0 <= refit_iters <= " + std::to_string(OETR_POSE_REFIT_MAX_ITERS));
  if (!(px_thr > 0.0) || !(px_thr - px_thr == 0.0))
    return entry_fail(me, OETR_ERR_BAD_ARG, "need a finite px_thr > 0");
  if (n_matches > (int64_t)INT32_MAX)
    return entry_fail(me, OETR_ERR_BAD_SHAPE, "need n_matches <= " + std::to_string(INT32_MAX) + " (the offsets are int32)");
  hipLaunchKernelGGL(k_pr_refit, dim3((unsigned)n_pairs), dim3(RF_THREADS), 0, static_cast<hipStream_t>(stream), params,
                     offsets, n_pairs, k1, k2, (int)n_matches, model_in, px_thr, refit_iters, model, pose, cosines,
                     counts, inliers);
  return entry_hip(me, hipGetLastError(), "k_pr_refit");
}

}  // extern "C"
