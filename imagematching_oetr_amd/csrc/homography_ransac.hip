// Homographies from match lists by RANSAC with a refit (include/oetr_homography_ransac.h).  The kernels run
// tests/homography_ransac_oracle.py LITERALLY; the one copy of the arithmetic is homography_ransac_math.h (float64,
// every operation rounded on its own, no contraction into FMAs, IEEE division and square root).
//
// k_hr_solve: one thread per (pair, hypothesis), 64-thread workgroups.  The sampler, the four rows' loads and
// normalisation, the closed-form 4-point solver; one model into the workspace, an absent one all NaN.
//
// k_hr_score, the hot one: the shape of k_pr_score.  A workgroup is (pair, tile of 256 models), a thread holds ONE
// model in registers and walks the pair's rows.  The rows are staged through LDS in tiles of 256: widened and
// normalised ONCE per tile, then read back as broadcasts.  The inlier count lives in a register: no atomics, one int32
// store per model.
//
// k_hr_finish: one workgroup of 256 threads per pair.  Argmax over the pair's model counts (the lowest number on a
// tie) through LDS; then the refit rounds, every value of which is uniform over the workgroup: thread t adds the
// terms of the inlier rows t, t + 256, ... of the list (the 256 partial sums of the specification), the partials are
// summed by the specified tree - an xor butterfly of lane shuffles within each of the four waves, the four wave values
// through LDS as (w0 + w1) + (w2 + w3) -, the 8 x 9 system is eliminated in LDS with one thread per element (the two
// steps of hr::solve8, spread over the lanes: the registers of a serial elimination would leave one wave per SIMD), the
// candidate is scored over all rows and accepted or not.  One last pass writes `inliers` under the delivered model;
// thread 0 writes the rest.
#include <string>

#include "../../include/oetr_homography_ransac.h"
#include "common.h"
#include "homography_ransac_math.h"

namespace oetr {

constexpr int HR_PARAMS = OETR_HOMOGRAPHY_PARAM_DOUBLES;
constexpr int HR_SOLVE_THREADS = 64;
constexpr int HR_THREADS = 256;                                    // models per tile, rows per LDS tile, hr::CLASSES
constexpr int HR_WAVES = HR_THREADS / 64;
constexpr int HR_COUNTERS = OETR_HOMOGRAPHY_RANSAC_COUNTERS;
static_assert(HR_THREADS == hr::CLASSES && HR_WAVES == 4, "the refit's tree is written for four waves of 64");

// The list of pair p: first row and length, both offsets clamped into [0, n_matches] (start + len <= n_matches).
__device__ __forceinline__ void hr_list(const int32_t* __restrict__ offsets, int p, int n_matches, int& start, int& len) {
  int a = offsets[p], b = offsets[p + 1];
  a = a < 0 ? 0 : (a > n_matches ? n_matches : a);
  b = b < 0 ? 0 : (b > n_matches ? n_matches : b);
  start = a;
  len = b > a ? b - a : 0;
}

// Row m < n_matches, normalised: (x1, y1, x2, y2).
__device__ __forceinline__ void hr_row(const hr::Frames& f, const float* __restrict__ k1, const float* __restrict__ k2,
                                       int m, double& x1, double& y1, double& x2, double& y2) {
  const size_t at = 2 * (size_t)m;
  hr::normalise(f, (double)k1[at], (double)k1[at + 1], (double)k2[at], (double)k2[at + 1], x1, y1, x2, y2);
}

__global__ __launch_bounds__(HR_SOLVE_THREADS) void k_hr_solve(
    const double* __restrict__ params, const int32_t* __restrict__ offsets, const int32_t* __restrict__ pair_ids,
    int n_pairs, const float* __restrict__ k1, const float* __restrict__ k2, int n_matches, int n_hyp, uint32_t seed,
    double* __restrict__ models) {
  const int64_t at = (int64_t)blockIdx.x * HR_SOLVE_THREADS + (int64_t)threadIdx.x;
  if (at >= (int64_t)n_pairs * n_hyp) return;                       // n_pairs * n_hyp <= INT32_MAX (host check)
  const int p = (int)(at / n_hyp), h = (int)(at - (int64_t)p * n_hyp);
  const double* __restrict__ P = params + (size_t)p * HR_PARAMS;
  int start, len;
  hr_list(offsets, p, n_matches, start, len);
  double out[9];
  if (len >= hr::SAMPLE && hr::sizes_ok(P)) {
    const uint32_t id = pair_ids ? (uint32_t)pair_ids[p] : (uint32_t)p;
    uint32_t idx[hr::SAMPLE];
    hr::sample4(seed, id, (uint32_t)h, (uint32_t)len, idx);         // idx[j] < len: start + idx[j] < n_matches
    const hr::Frames f = hr::frames(P);
    double X[hr::SAMPLE][4];
#pragma unroll
    for (int j = 0; j < hr::SAMPLE; ++j) hr_row(f, k1, k2, start + (int)idx[j], X[j][0], X[j][1], X[j][2], X[j][3]);
    hr::solve4(X, out);
  } else {
#pragma unroll
    for (int k = 0; k < 9; ++k) out[k] = hr::nan64();
  }
  double* dst = models + (size_t)at * 9;                            // model h of pair p
#pragma unroll
  for (int k = 0; k < 9; ++k) dst[k] = out[k];
}

// grid: x = pair * tiles + tile
__global__ __launch_bounds__(HR_THREADS) void k_hr_score(
    const double* __restrict__ params, const int32_t* __restrict__ offsets, int n_pairs, const float* __restrict__ k1,
    const float* __restrict__ k2, int n_matches, const double* __restrict__ models, int n_models, int tiles,
    double px_thr, int32_t* __restrict__ model_counts) {
  __shared__ __attribute__((aligned(32))) double rows[HR_THREADS][4];
  const int p = (int)blockIdx.x / tiles, tile = (int)blockIdx.x - p * tiles;
  const int m = tile * HR_THREADS + (int)threadIdx.x;
  const bool mine = m < n_models;
  const double* __restrict__ P = params + (size_t)p * HR_PARAMS;
  const bool sized = hr::sizes_ok(P);                               // uniform over the workgroup
  int start, len;
  hr_list(offsets, p, n_matches, start, len);
  if (!sized) len = 0;
  const hr::Frames f = hr::frames(P);
  const double thr_sq = hr::thr_sq(f, px_thr);
  double h[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) h[k] = mine ? models[((size_t)p * n_models + (size_t)m) * 9 + k] : hr::nan64();
  int count = 0;
  for (int base = 0; base < len; base += HR_THREADS) {              // uniform over the workgroup
    __syncthreads();
    const int j = base + (int)threadIdx.x;
    double x1 = hr::nan64(), y1 = x1, x2 = x1, y2 = x1;
    if (j < len) hr_row(f, k1, k2, start + j, x1, y1, x2, y2);
    rows[threadIdx.x][0] = x1, rows[threadIdx.x][1] = y1, rows[threadIdx.x][2] = x2, rows[threadIdx.x][3] = y2;
    __syncthreads();
    const int n = len - base < HR_THREADS ? len - base : HR_THREADS;
#pragma unroll 8
    for (int r = 0; r < n; ++r) count += hr::inlier(h, rows[r][0], rows[r][1], rows[r][2], rows[r][3], thr_sq) ? 1 : 0;
  }
  if (mine) model_counts[(size_t)p * n_models + (size_t)m] = (sized && hr::finite_model(h)) ? count : -1;
}

// An int over the workgroup: the sum (MIN false) or the minimum (MIN true).  `s`: HR_WAVES ints of LDS nobody else
// uses between the two barriers inside.
template <bool MIN>
__device__ __forceinline__ int hr_reduce_int(int v, int* s) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int w = __shfl_xor(v, o, 64);
    v = MIN ? (w < v ? w : v) : v + w;
  }
  __syncthreads();                                                  // the last readers of `s` are through
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  const int a = s[0], b = s[1], c = s[2], d = s[3];
  if (MIN) return (a < b ? a : b) < (c < d ? c : d) ? (a < b ? a : b) : (c < d ? c : d);
  return (a + b) + (c + d);
}

__global__ __launch_bounds__(HR_THREADS) void k_hr_finish(
    const double* __restrict__ params, const int32_t* __restrict__ offsets, int n_pairs, const float* __restrict__ k1,
    const float* __restrict__ k2, int n_matches, const double* __restrict__ models, int n_models,
    const int32_t* __restrict__ model_counts, double px_thr, int refit_iters, double* __restrict__ model,
    double* __restrict__ H_out, double* __restrict__ corner_sq, int32_t* __restrict__ counts,
    uint8_t* __restrict__ inliers) {
#pragma clang fp contract(off)
  __shared__ int s_best[HR_THREADS], s_at[HR_THREADS], s_finite[HR_THREADS];
  __shared__ double s_sum[HR_WAVES][hr::TERMS], s_tot[hr::TERMS], s_A[8][9];
  __shared__ int s_int[HR_WAVES];
  const int p = blockIdx.x, tid = threadIdx.x;
  const double* __restrict__ P = params + (size_t)p * HR_PARAMS;
  const bool sized = hr::sizes_ok(P);                               // uniform over the workgroup
  int start, len;
  hr_list(offsets, p, n_matches, start, len);

  // the model with the most inliers, the lowest number on a tie; a non-finite model (-1) never wins
  int best = -1, at = INT32_MAX, finite = 0;
  for (int m = tid; m < n_models; m += HR_THREADS) {                // ascending: a later equal count does not replace
    const int c = model_counts[(size_t)p * n_models + (size_t)m];
    finite += c >= 0 ? 1 : 0;
    if (c > best) best = c, at = m;
  }
  s_best[tid] = best, s_at[tid] = at, s_finite[tid] = finite;
  __syncthreads();
  for (int half = HR_THREADS / 2; half > 0; half >>= 1) {
    if (tid < half) {
      const int b = s_best[tid + half], a = s_at[tid + half];
      if (b > s_best[tid] || (b == s_best[tid] && a < s_at[tid])) s_best[tid] = b, s_at[tid] = a;
      s_finite[tid] += s_finite[tid + half];
    }
    __syncthreads();
  }
  best = s_best[0];
  finite = s_finite[0];
  const int selected = (sized && best >= 0) ? s_at[0] : -1;         // uniform over the workgroup; < n_models
  const bool found = selected >= 0;

  const hr::Frames f = hr::frames(P);
  const double thr_sq = hr::thr_sq(f, px_thr);
  double cur[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) cur[k] = found ? models[((size_t)p * n_models + (size_t)selected) * 9 + k] : hr::nan64();
  int count = found ? best : 0, accepted = 0;

  // the refit: a fixed number of rounds, every decision uniform over the workgroup
#pragma nounroll
  for (int round = 0; found && round < refit_iters; ++round) {
    double acc[hr::TERMS];
#pragma unroll
    for (int k = 0; k < hr::TERMS; ++k) acc[k] = 0.0;
    int n = 0, first = INT32_MAX;
    for (int j = tid; j < len; j += HR_THREADS) {                   // partial sum `tid`: positions tid, tid + 256, ...
      double x1, y1, x2, y2;
      hr_row(f, k1, k2, start + j, x1, y1, x2, y2);
      if (hr::inlier(cur, x1, y1, x2, y2, thr_sq)) {
        hr::add_row_terms(acc, x1, y1, x2, y2);
        n += 1;
        first = j < first ? j : first;
      }
    }
    // the tree: an xor butterfly within the wave (all 64 lanes end equal), then (w0 + w1) + (w2 + w3)
#pragma unroll
    for (int k = 0; k < hr::TERMS; ++k) {
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) acc[k] = acc[k] + __shfl_xor(acc[k], o, 64);
    }
    __syncthreads();                                                // the last round's readers of s_sum are through
    if ((tid & 63) == 0) {
#pragma unroll
      for (int k = 0; k < hr::TERMS; ++k) s_sum[tid >> 6][k] = acc[k];
    }
    __syncthreads();
    if (tid < hr::TERMS) s_tot[tid] = (s_sum[0][tid] + s_sum[1][tid]) + (s_sum[2][tid] + s_sum[3][tid]);
    n = hr_reduce_int<false>(n, s_int);
    first = hr_reduce_int<true>(first, s_int);                      // (its barriers publish s_tot, too)
    if (n < hr::SAMPLE) break;                                      // first < len from here on
    // the elimination, spread over the workgroup: thread e < 72 owns element (e / 9, e % 9) of the 8 x 9 system; the
    // matrix lives in LDS between the steps; every thread takes the same pivot decisions from the same LDS values
    const bool owner = tid < 72;
    const int er = owner ? tid / 9 : 0, ek = owner ? tid - 9 * er : 0;
    const int src = hr::normal_index(owner ? tid : 0);
    double a = src == hr::NORMAL_N ? (double)n : (src == hr::NORMAL_ZERO ? 0.0 : s_tot[src]);
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
    double cand[9];
#pragma unroll
    for (int r = 0; r < 8; ++r) cand[r] = s_A[r][8];
    cand[8] = 1.0;
    double fx, fy, fx2, fy2;
    hr_row(f, k1, k2, start + first, fx, fy, fx2, fy2);
    hr::unit_and_sign(cand, fx, fy);
    ok = ok && hr::finite_model(cand);
    if (!ok) break;
    int c = 0;
    for (int j = tid; j < len; j += HR_THREADS) {
      double x1, y1, x2, y2;
      hr_row(f, k1, k2, start + j, x1, y1, x2, y2);
      c += hr::inlier(cand, x1, y1, x2, y2, thr_sq) ? 1 : 0;
    }
    c = hr_reduce_int<false>(c, s_int);
    if (c < count) break;
#pragma unroll
    for (int k = 0; k < 9; ++k) cur[k] = cand[k];
    count = c;
    accepted += 1;
  }

  if (inliers) {
    for (int j = tid; j < len; j += HR_THREADS) {
      double x1, y1, x2, y2;
      hr_row(f, k1, k2, start + j, x1, y1, x2, y2);
      inliers[(size_t)(start + j)] = (found && hr::inlier(cur, x1, y1, x2, y2, thr_sq)) ? 1 : 0;
    }
    // rows outside every list: before the first list and after the last one (the offsets are non-decreasing)
    if (p == 0)
      for (int j = tid; j < start; j += HR_THREADS) inliers[(size_t)j] = 0;
    if (p == n_pairs - 1)
      for (int j = start + len + tid; j < n_matches; j += HR_THREADS) inliers[(size_t)j] = 0;
  }
  if (tid != 0) return;

  double H[9];
  hr::deliver(cur, f, H);
  const double w = P[9] - 1.0, h = P[10] - 1.0;
  double* mo = model + 9 * (size_t)p;
  double* ho = H_out + 9 * (size_t)p;
#pragma unroll
  for (int k = 0; k < 9; ++k) mo[k] = cur[k], ho[k] = found ? H[k] : hr::nan64();
  double* co = corner_sq + 4 * (size_t)p;
  co[0] = found ? hr::corner_sq(H, P, 0.0, 0.0) : hr::nan64();
  co[1] = found ? hr::corner_sq(H, P, w, 0.0) : hr::nan64();
  co[2] = found ? hr::corner_sq(H, P, w, h) : hr::nan64();
  co[3] = found ? hr::corner_sq(H, P, 0.0, h) : hr::nan64();
  int32_t* cn = counts + HR_COUNTERS * (size_t)p;
  cn[0] = sized ? len : -1, cn[1] = sized ? finite : -1, cn[2] = selected;
  cn[3] = sized ? (found ? best : 0) : -1, cn[4] = sized ? count : -1, cn[5] = sized ? accepted : -1;
}

}  // namespace oetr

using namespace oetr;

extern "C" {

int oetr_homography_ransac_abi_version(void) { return OETR_HOMOGRAPHY_RANSAC_ABI_VERSION; }

size_t oetr_homography_ransac_workspace_bytes(int n_pairs, int n_models) {
  if (n_pairs <= 0 || n_models <= 0) return 0;
  return (size_t)n_pairs * (size_t)n_models * (9 * sizeof(double) + sizeof(int32_t));
}

// The host code dereferences none of its pointer arguments and reads nothing from the device.
oetr_status oetr_homography_ransac(const double* params, const int32_t* offsets, const int32_t* pair_ids, int n_pairs,
                                   const float* k1, const float* k2, int64_t n_matches, int n_hyp, uint32_t seed,
                                   double px_thr, int refit_iters, const double* models_in, int n_models_in,
                                   void* workspace, size_t workspace_bytes, double* model, double* H, double* corner_sq,
                                   int32_t* counts, uint8_t* inliers, void* stream) {
  const char* me = "oetr_homography_ransac";
  if (!params || !offsets) return entry_fail(me, OETR_ERR_BAD_ARG, "NULL parameter / offsets pointer");
  if (!model || !H || !corner_sq || !counts)
    return entry_fail(me, OETR_ERR_BAD_ARG, "NULL model / H / corner_sq / counts output");
  if (n_matches != 0 && (!k1 || !k2)) return entry_fail(me, OETR_ERR_BAD_ARG, "NULL keypoint pointer");
  if (n_pairs <= 0) return entry_fail(me, OETR_ERR_BAD_ARG, "need n_pairs > 0");
  if (n_matches < 0) return entry_fail(me, OETR_ERR_BAD_ARG, "need n_matches >= 0");
  if (!models_in && (n_hyp < 1 || n_hyp > OETR_HOMOGRAPHY_RANSAC_MAX_HYPOTHESES))
    return entry_fail(me, OETR_ERR_BAD_ARG,
                      "need 1 <= n_hyp <= " + std::to_string(OETR_HOMOGRAPHY_RANSAC_MAX_HYPOTHESES));
  if (models_in && (n_models_in < 1 || n_models_in > OETR_HOMOGRAPHY_RANSAC_MAX_MODELS))
    return entry_fail(me, OETR_ERR_BAD_ARG,
                      "need 1 <= n_models_in <= " + std::to_string(OETR_HOMOGRAPHY_RANSAC_MAX_MODELS));
  if (refit_iters < 0 || refit_iters > OETR_HOMOGRAPHY_RANSAC_MAX_REFIT)
    return entry_fail(me, OETR_ERR_BAD_ARG,
                      "need 0 <= refit_iters <= " + std::to_string(OETR_HOMOGRAPHY_RANSAC_MAX_REFIT));
  if (!(px_thr > 0.0) || !(px_thr - px_thr == 0.0))
    return entry_fail(me, OETR_ERR_BAD_ARG, "need a finite px_thr > 0");
  if (n_matches > (int64_t)INT32_MAX)
    return entry_fail(me, OETR_ERR_BAD_SHAPE, "need n_matches <= " + std::to_string(INT32_MAX) + " (the offsets are int32)");
  const int n_models = models_in ? n_models_in : n_hyp;
  if ((int64_t)n_pairs * n_models > (int64_t)INT32_MAX)
    return entry_fail(me, OETR_ERR_BAD_SHAPE, "need n_pairs * n_models <= " + std::to_string(INT32_MAX));
  const size_t need = oetr_homography_ransac_workspace_bytes(n_pairs, n_models);
  if (!workspace || workspace_bytes < need)
    return entry_fail(me, OETR_ERR_BAD_ARG,
                      "workspace NULL or smaller than oetr_homography_ransac_workspace_bytes(n_pairs, n_models) = " +
                          std::to_string(need));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int n = (int)n_matches;
  double* ws_models = static_cast<double*>(workspace);
  int32_t* model_counts = reinterpret_cast<int32_t*>(ws_models + (size_t)n_pairs * n_models * 9);
  const double* models = models_in ? models_in : ws_models;
  if (!models_in) {
    const unsigned blocks = (unsigned)(((int64_t)n_pairs * n_hyp + HR_SOLVE_THREADS - 1) / HR_SOLVE_THREADS);
    hipLaunchKernelGGL(k_hr_solve, dim3(blocks), dim3(HR_SOLVE_THREADS), 0, s, params, offsets, pair_ids, n_pairs, k1,
                       k2, n, n_hyp, seed, ws_models);
    if (oetr_status rc = entry_hip(me, hipGetLastError(), "k_hr_solve")) return rc;
  }
  const int tiles = (n_models + HR_THREADS - 1) / HR_THREADS;       // n_pairs * tiles <= n_pairs * n_models
  hipLaunchKernelGGL(k_hr_score, dim3((unsigned)(n_pairs * tiles)), dim3(HR_THREADS), 0, s, params, offsets, n_pairs,
                     k1, k2, n, models, n_models, tiles, px_thr, model_counts);
  if (oetr_status rc = entry_hip(me, hipGetLastError(), "k_hr_score")) return rc;
  hipLaunchKernelGGL(k_hr_finish, dim3((unsigned)n_pairs), dim3(HR_THREADS), 0, s, params, offsets, n_pairs, k1, k2, n,
                     models, n_models, model_counts, px_thr, refit_iters, model, H, corner_sq, counts, inliers);
  return entry_hip(me, hipGetLastError(), "k_hr_finish");
}

}  // extern "C"
