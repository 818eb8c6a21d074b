// Relative pose from match lists by RANSAC (include/oetr_pose_ransac.h).  The kernels run tests/pose_ransac_oracle.py
// LITERALLY; the one copy of the arithmetic is pose_ransac_math.h (float64, every operation rounded on its own, no
// contraction into FMAs, IEEE division and square root).
//
// k_pr_solve: one thread per (pair, hypothesis), 64-thread workgroups.  The sampler, the seven rows' loads and
// normalisation, the 7-point solver; up to 3 models into the workspace, absent ones all NaN.  The 7 x 9 system is
// eliminated with compile-time indices and row swaps by selects, so it stays in registers.  Not the hot kernel.
//
// k_pr_score, the hot one: a workgroup is (pair, tile of 256 models), a thread holds ONE model in registers and walks
// the pair's rows.  The rows are staged through LDS in tiles of 256: widened and normalised ONCE per tile, then read
// back as broadcasts (every lane the same address, two ds_read_b128 per row).  The inlier count lives in a register:
// no atomics, one int32 store per model.
//
// k_pr_pose: one workgroup per pair.  Argmax over the pair's model counts (the lowest number on a tie) through LDS;
// the decomposition, computed by every thread alike (wave-uniform values: no broadcast step needed); ONE pass over the
// rows that scores them again under the selected model, writes `inliers`, and takes the four cheirality votes of the
// inlier rows, summed by integer LDS atomics; then the choice, pose, cosines and counts by thread 0.
#include <string>

#include "../../include/oetr_pose_ransac.h"
#include "common.h"
#include "pose_ransac_math.h"

namespace oetr {

constexpr int PR_PARAMS = OETR_MATCH_SCORE_PARAM_DOUBLES;
constexpr int PR_SOLVE_THREADS = 64;
constexpr int PR_THREADS = 256;                                    // k_pr_score: models per tile, rows per LDS tile
constexpr int PR_COUNTERS = OETR_POSE_RANSAC_COUNTERS;

// The list of pair p: first row and length, both offsets clamped into [0, n_matches] (start + len <= n_matches).
__device__ __forceinline__ void pr_list(const int32_t* __restrict__ offsets, int p, int n_matches, int& start, int& len) {
  int a = offsets[p], b = offsets[p + 1];
  a = a < 0 ? 0 : (a > n_matches ? n_matches : a);
  b = b < 0 ? 0 : (b > n_matches ? n_matches : b);
  start = a;
  len = b > a ? b - a : 0;
}

// Row m < n_matches, normalised: (x1, y1, x2, y2).
__device__ __forceinline__ void pr_row(const double* __restrict__ P, const float* __restrict__ k1,
                                       const float* __restrict__ k2, int m, double& x1, double& y1, double& x2,
                                       double& y2) {
#pragma clang fp contract(off)
  const size_t at = 2 * (size_t)m;
  const double u1 = (double)k1[at], v1 = (double)k1[at + 1], u2 = (double)k2[at], v2 = (double)k2[at + 1];
  x1 = (u1 - P[2]) / P[0], y1 = (v1 - P[3]) / P[1];
  x2 = (u2 - P[6]) / P[4], y2 = (v2 - P[7]) / P[5];
}

__device__ __forceinline__ double pr_thr_sq(const double* __restrict__ P, double px_thr) {
#pragma clang fp contract(off)
  const double thr_n = px_thr / ((P[0] + P[5]) / 2.0);
  return thr_n * thr_n;
}

__global__ __launch_bounds__(PR_SOLVE_THREADS) void k_pr_solve(
    const double* __restrict__ params, const int32_t* __restrict__ offsets, const int32_t* __restrict__ pair_ids,
    int n_pairs, const float* __restrict__ k1, const float* __restrict__ k2, int n_matches, int n_hyp, uint32_t seed,
    double* __restrict__ models) {
  const int64_t at = (int64_t)blockIdx.x * PR_SOLVE_THREADS + (int64_t)threadIdx.x;
  if (at >= (int64_t)n_pairs * n_hyp) return;                       // n_pairs * 3 * n_hyp <= INT32_MAX (host check)
  const int p = (int)(at / n_hyp), h = (int)(at - (int64_t)p * n_hyp);
  int start, len;
  pr_list(offsets, p, n_matches, start, len);
  double out[pr::ROOTS][9];
  if (len >= pr::SAMPLE) {
    const uint32_t id = pair_ids ? (uint32_t)pair_ids[p] : (uint32_t)p;
    uint32_t idx[pr::SAMPLE];
    pr::sample7(seed, id, (uint32_t)h, (uint32_t)len, idx);         // idx[j] < len: start + idx[j] < n_matches
    const double* __restrict__ P = params + (size_t)p * PR_PARAMS;
    double X[pr::SAMPLE][4];
#pragma unroll
    for (int j = 0; j < pr::SAMPLE; ++j) pr_row(P, k1, k2, start + (int)idx[j], X[j][0], X[j][1], X[j][2], X[j][3]);
    pr::solve7(X, out);
  } else {
#pragma unroll
    for (int s = 0; s < pr::ROOTS; ++s)
#pragma unroll
      for (int k = 0; k < 9; ++k) out[s][k] = pr::nan64();
  }
  double* dst = models + (size_t)at * (pr::ROOTS * 9);              // model 3 * h + root of pair p
#pragma unroll
  for (int s = 0; s < pr::ROOTS; ++s)
#pragma unroll
    for (int k = 0; k < 9; ++k) dst[9 * s + k] = out[s][k];
}

// grid: x = pair * tiles + tile
__global__ __launch_bounds__(PR_THREADS) void k_pr_score(
    const double* __restrict__ params, const int32_t* __restrict__ offsets, int n_pairs, const float* __restrict__ k1,
    const float* __restrict__ k2, int n_matches, const double* __restrict__ models, int n_models, int tiles,
    double px_thr, int32_t* __restrict__ model_counts) {
  __shared__ __attribute__((aligned(32))) double rows[PR_THREADS][4];
  const int p = (int)blockIdx.x / tiles, tile = (int)blockIdx.x - p * tiles;
  const int m = tile * PR_THREADS + (int)threadIdx.x;
  const bool mine = m < n_models;
  const double* __restrict__ P = params + (size_t)p * PR_PARAMS;
  int start, len;
  pr_list(offsets, p, n_matches, start, len);
  const double thr_sq = pr_thr_sq(P, px_thr);
  double F[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) F[k] = mine ? models[((size_t)p * n_models + (size_t)m) * 9 + k] : pr::nan64();
  int count = 0;
  for (int base = 0; base < len; base += PR_THREADS) {              // uniform over the workgroup
    __syncthreads();
    const int j = base + (int)threadIdx.x;
    double x1 = pr::nan64(), y1 = x1, x2 = x1, y2 = x1;
    if (j < len) pr_row(P, k1, k2, start + j, x1, y1, x2, y2);
    rows[threadIdx.x][0] = x1, rows[threadIdx.x][1] = y1, rows[threadIdx.x][2] = x2, rows[threadIdx.x][3] = y2;
    __syncthreads();
    const int n = len - base < PR_THREADS ? len - base : PR_THREADS;
#pragma unroll 4
    for (int r = 0; r < n; ++r) count += pr::inlier(F, rows[r][0], rows[r][1], rows[r][2], rows[r][3], thr_sq) ? 1 : 0;
  }
  if (mine) model_counts[(size_t)p * n_models + (size_t)m] = pr::finite_model(F) ? count : -1;
}

__global__ __launch_bounds__(PR_THREADS) void k_pr_pose(
    const double* __restrict__ params, const int32_t* __restrict__ offsets, int n_pairs, const float* __restrict__ k1,
    const float* __restrict__ k2, int n_matches, const double* __restrict__ models, int n_models,
    const int32_t* __restrict__ model_counts, double px_thr, double* __restrict__ model, double* __restrict__ pose,
    double* __restrict__ cosines, int32_t* __restrict__ counts, uint8_t* __restrict__ inliers) {
  __shared__ int s_best[PR_THREADS], s_at[PR_THREADS], s_finite[PR_THREADS];
  __shared__ int s_votes[4];
  const int p = blockIdx.x, tid = threadIdx.x;
  const double* __restrict__ P = params + (size_t)p * PR_PARAMS;
  int start, len;
  pr_list(offsets, p, n_matches, start, len);

  // the model with the most inliers, the lowest number on a tie; a non-finite model (-1) never wins
  int best = -1, at = INT32_MAX, finite = 0;
  for (int m = tid; m < n_models; m += PR_THREADS) {                // ascending: a later equal count does not replace
    const int c = model_counts[(size_t)p * n_models + (size_t)m];
    finite += c >= 0 ? 1 : 0;
    if (c > best) best = c, at = m;
  }
  s_best[tid] = best, s_at[tid] = at, s_finite[tid] = finite;
  if (tid < 4) s_votes[tid] = 0;
  __syncthreads();
  for (int half = PR_THREADS / 2; half > 0; half >>= 1) {
    if (tid < half) {
      const int b = s_best[tid + half], a = s_at[tid + half];
      if (b > s_best[tid] || (b == s_best[tid] && a < s_at[tid])) s_best[tid] = b, s_at[tid] = a;
      s_finite[tid] += s_finite[tid + half];
    }
    __syncthreads();
  }
  best = s_best[0];
  finite = s_finite[0];
  const int selected = best >= 0 ? s_at[0] : -1;                    // uniform over the workgroup; < n_models
  const bool posed = selected >= 0;

  double F[9], R1[9], R2[9], t[3];
#pragma unroll
  for (int k = 0; k < 9; ++k) F[k] = posed ? models[((size_t)p * n_models + (size_t)selected) * 9 + k] : pr::nan64();
  pr::decompose(F, R1, R2, t);
  const double thr_sq = pr_thr_sq(P, px_thr);

  int votes[4] = {0, 0, 0, 0};
  for (int j = tid; j < len; j += PR_THREADS) {
    double x1, y1, x2, y2;
    pr_row(P, k1, k2, start + j, x1, y1, x2, y2);
    const bool in = posed && pr::inlier(F, x1, y1, x2, y2, thr_sq);
    if (inliers) inliers[(size_t)(start + j)] = in ? 1 : 0;
    if (in) {
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
    for (int j = tid; j < start; j += PR_THREADS) inliers[(size_t)j] = 0;
  if (inliers && p == n_pairs - 1)
    for (int j = start + len + tid; j < n_matches; j += PR_THREADS) inliers[(size_t)j] = 0;
#pragma unroll
  for (int c = 0; c < 4; ++c)
    if (votes[c]) atomicAdd(&s_votes[c], votes[c]);
  __syncthreads();
  if (tid != 0) return;

  int cand = 0, most = s_votes[0];
#pragma unroll
  for (int c = 1; c < 4; ++c)
    if (s_votes[c] > most) most = s_votes[c], cand = c;
  double R[9], tc[3];
#pragma unroll
  for (int k = 0; k < 9; ++k) R[k] = cand < 2 ? R1[k] : R2[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) tc[k] = (cand & 1) ? -t[k] : t[k];
  double cos_r, cos_t;
  pr::cosines(P + 8, P + 17, R, tc, cos_r, cos_t);
  double* mo = model + 9 * (size_t)p;
  double* po = pose + 12 * (size_t)p;
#pragma unroll
  for (int k = 0; k < 9; ++k) mo[k] = F[k], po[k] = posed ? R[k] : pr::nan64();
#pragma unroll
  for (int k = 0; k < 3; ++k) po[9 + k] = posed ? tc[k] : pr::nan64();
  cosines[2 * (size_t)p] = posed ? cos_r : pr::nan64();
  cosines[2 * (size_t)p + 1] = posed ? cos_t : pr::nan64();
  int32_t* co = counts + PR_COUNTERS * (size_t)p;
  co[0] = len, co[1] = finite, co[2] = selected, co[3] = posed ? best : 0, co[4] = posed ? most : 0;
}

__global__ void k_pr_sqrt(const double* __restrict__ in, double* __restrict__ out, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + (int64_t)threadIdx.x;
  if (i < n) out[i] = pr::sqrt_rn(in[i]);
}

}  // namespace oetr

using namespace oetr;

extern "C" {

int oetr_pose_ransac_abi_version(void) { return OETR_POSE_RANSAC_ABI_VERSION; }

size_t oetr_pose_ransac_workspace_bytes(int n_pairs, int n_models) {
  if (n_pairs <= 0 || n_models <= 0) return 0;
  return (size_t)n_pairs * (size_t)n_models * (9 * sizeof(double) + sizeof(int32_t));
}

// The host code dereferences none of its pointer arguments and reads nothing from the device.
oetr_status oetr_pose_ransac(const double* params, const int32_t* offsets, const int32_t* pair_ids, int n_pairs,
                             const float* k1, const float* k2, int64_t n_matches, int n_hyp, uint32_t seed,
                             double px_thr, const double* models_in, int n_models_in, void* workspace,
                             size_t workspace_bytes, double* model, double* pose, double* cosines, int32_t* counts,
                             uint8_t* inliers, void* stream) {
  const char* me = "oetr_pose_ransac";
  if (!params || !offsets) return entry_fail(me, OETR_ERR_BAD_ARG, "NULL parameter / offsets pointer");
  if (!model || !pose || !cosines || !counts)
    return entry_fail(me, OETR_ERR_BAD_ARG, "NULL model / pose / cosines / counts output");
  if (n_matches != 0 && (!k1 || !k2)) return entry_fail(me, OETR_ERR_BAD_ARG, "NULL keypoint pointer");
  if (n_pairs <= 0) return entry_fail(me, OETR_ERR_BAD_ARG, "need n_pairs > 0");
  if (n_matches < 0) return entry_fail(me, OETR_ERR_BAD_ARG, "need n_matches >= 0");
  if (!models_in && (n_hyp < 1 || n_hyp > OETR_POSE_RANSAC_MAX_HYPOTHESES))
    return entry_fail(me, OETR_ERR_BAD_ARG, "need 1 <= n_hyp <= " + std::to_string(OETR_POSE_RANSAC_MAX_HYPOTHESES));
  if (models_in && (n_models_in < 1 || n_models_in > OETR_POSE_RANSAC_MAX_MODELS))
    return entry_fail(me, OETR_ERR_BAD_ARG, "need 1 <= n_models_in <= " + std::to_string(OETR_POSE_RANSAC_MAX_MODELS));
  if (!(px_thr > 0.0) || !(px_thr - px_thr == 0.0))
    return entry_fail(me, OETR_ERR_BAD_ARG, "need a finite px_thr > 0");
  if (n_matches > (int64_t)INT32_MAX)
    return entry_fail(me, OETR_ERR_BAD_SHAPE, "need n_matches <= " + std::to_string(INT32_MAX) + " (the offsets are int32)");
  const int n_models = models_in ? n_models_in : pr::ROOTS * n_hyp;
  if ((int64_t)n_pairs * n_models > (int64_t)INT32_MAX)
    return entry_fail(me, OETR_ERR_BAD_SHAPE, "need n_pairs * n_models <= " + std::to_string(INT32_MAX));
  const size_t need = oetr_pose_ransac_workspace_bytes(n_pairs, n_models);
  if (!workspace || workspace_bytes < need)
    return entry_fail(me, OETR_ERR_BAD_ARG,
                      "workspace NULL or smaller than oetr_pose_ransac_workspace_bytes(n_pairs, n_models) = " +
                          std::to_string(need));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int n = (int)n_matches;
  double* ws_models = static_cast<double*>(workspace);
  int32_t* model_counts = reinterpret_cast<int32_t*>(ws_models + (size_t)n_pairs * n_models * 9);
  const double* models = models_in ? models_in : ws_models;
  if (!models_in) {
    const unsigned blocks = (unsigned)(((int64_t)n_pairs * n_hyp + PR_SOLVE_THREADS - 1) / PR_SOLVE_THREADS);
    hipLaunchKernelGGL(k_pr_solve, dim3(blocks), dim3(PR_SOLVE_THREADS), 0, s, params, offsets, pair_ids, n_pairs, k1,
                       k2, n, n_hyp, seed, ws_models);
    if (oetr_status rc = entry_hip(me, hipGetLastError(), "k_pr_solve")) return rc;
  }
  const int tiles = (n_models + PR_THREADS - 1) / PR_THREADS;       // n_pairs * tiles <= n_pairs * n_models
  hipLaunchKernelGGL(k_pr_score, dim3((unsigned)(n_pairs * tiles)), dim3(PR_THREADS), 0, s, params, offsets, n_pairs,
                     k1, k2, n, models, n_models, tiles, px_thr, model_counts);
  if (oetr_status rc = entry_hip(me, hipGetLastError(), "k_pr_score")) return rc;
  hipLaunchKernelGGL(k_pr_pose, dim3((unsigned)n_pairs), dim3(PR_THREADS), 0, s, params, offsets, n_pairs, k1, k2, n,
                     models, n_models, model_counts, px_thr, model, pose, cosines, counts, inliers);
  return entry_hip(me, hipGetLastError(), "k_pr_pose");
}

oetr_status oetr_pose_ransac_sqrt(const double* in, double* out, int64_t n, void* stream) {
  const char* me = "oetr_pose_ransac_sqrt";
  if (!in || !out) return entry_fail(me, OETR_ERR_BAD_ARG, "NULL pointer");
  if (n <= 0 || n > (int64_t)INT32_MAX) return entry_fail(me, OETR_ERR_BAD_ARG, "need 0 < n <= " + std::to_string(INT32_MAX));
  hipLaunchKernelGGL(k_pr_sqrt, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), in,
                     out, n);
  return entry_hip(me, hipGetLastError(), "k_pr_sqrt");
}

}  // extern "C"
