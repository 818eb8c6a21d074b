// Keypoint repeatability against depth and pose (include/oetr_keypoint_score.h): the reference's pose_evaluate ->
// get_projected_kp / unnormalize_keypoints / get_repeatability for many pairs over a depth-map set, both directions,
// in one call.
//
// k_keypoint_nearest: workgroup = (query tile of 256 source keypoints, direction, pair), flattened into blockIdx.x;
// one thread owns one source keypoint.  The pair's two indices, two table rows, four offsets and 20 parameters depend
// on blockIdx alone: wave-uniform (scalar) loads.  The thread projects its keypoint itself - one depth pixel, three
// float64 divisions, tests/keypoint_score_oracle.py::project LITERALLY: float64, every operation rounded on its own
// in the order and with the parentheses written there (no contraction into FMAs) - so there is no buffer of projected
// points.  The depth read and the projection are depth_pose.h's, the one copy match_row of match_score.hip runs
// too: a keypoint scored through either entry gives the same bits.  The target picture's keypoints go through LDS
// in tiles of 256, widened to float64 once; in the inner loop every lane reads the same LDS address (a broadcast: no
// bank conflict), and the running minimum is taken with a strict "<" in ascending index order: the lowest index wins
// a tie, a NaN never wins.
// A workgroup in which no row is kept skips the loop.
//
// Nothing is dereferenced on the strength of device data alone: the map indices are tested against n_maps, the
// table rows as in k_match_score, a picture's keypoint rows against n_keypoints and max_kp (keypoint_rows), a depth
// pixel in float64 against its map's H, W before the conversion to an integer.
//
// Counters: one ballot and one popcount per wave for the kept rows and for each threshold, one atomicAdd per
// non-zero count from the wave's first lane.  Integer atomics commute: the counters do not depend on arrival order.
// clear_i32 (match_score.hip's k_clear_i32) zeroes the counters before, k_keypoint_finish (one thread per pair and
// direction) afterwards writes the source picture's keypoint count, or -1 throughout for a pair that is not vouched for.
#include <cmath>
#include <string>

#include "../../include/oetr_keypoint_score.h"
#include "common.h"
#include "depth_pose.h"

namespace oetr {

constexpr int KP_THREADS = 256;                                     // the query tile: one thread per source keypoint
constexpr int KP_TARGET_TILE = 256;                                 // target keypoints staged in LDS at a time
constexpr int KP_PARAMS = OETR_MATCH_SCORE_PARAM_DOUBLES;
constexpr int KP_MAX_THR = OETR_KEYPOINT_SCORE_MAX_THRESHOLDS;
constexpr int KP_HEAD = OETR_KEYPOINT_SCORE_HEAD_COUNTERS;

struct KpThresholds {
  double th[KP_MAX_THR];
};

// The keypoint rows [first, first + count) of picture k, or false when they are not vouched for: every row then lies
// in [0, n_keypoints) and count in [0, max_kp].  k is in [0, n_maps): reads kp_offsets[k], kp_offsets[k + 1].
__device__ __forceinline__ bool keypoint_rows(const int32_t* __restrict__ kp_offsets, int k, int n_keypoints,
                                              int max_kp, int& first, int& count) {
  const int lo = kp_offsets[k], hi = kp_offsets[k + 1];
  first = lo;
  count = 0;
  if (lo < 0 || hi > n_keypoints || hi < lo) return false;         // 0 <= lo <= hi <= n_keypoints: no overflow below
  count = hi - lo;
  return count <= max_kp;
}

struct KpPair {
  oetr_covis_map m1, m2;
  int first1, count1, first2, count2;
};

// Everything pair p reads through, or false when the pair must not be dereferenced.
__device__ __forceinline__ bool keypoint_pair(const oetr_covis_map* __restrict__ maps, int n_maps,
                                              const int32_t* __restrict__ kp_offsets, int n_keypoints, int max_kp,
                                              const int32_t* __restrict__ idx1, const int32_t* __restrict__ idx2,
                                              int p, KpPair& out) {
  const int i1 = idx1[p], i2 = idx2[p];
  if (!pair_maps(maps, n_maps, idx1, idx2, p, out.m1, out.m2)) return false;          // i1, i2 in [0, n_maps)
  const bool rows1 = keypoint_rows(kp_offsets, i1, n_keypoints, max_kp, out.first1, out.count1);
  const bool rows2 = keypoint_rows(kp_offsets, i2, n_keypoints, max_kp, out.first2, out.count2);
  return rows1 && rows2;
}

__global__ __launch_bounds__(KP_THREADS) void k_keypoint_nearest(
    const oetr_covis_map* __restrict__ maps, int n_maps, const float2* __restrict__ keypoints, int n_keypoints,
    const int32_t* __restrict__ kp_offsets, const int32_t* __restrict__ idx1, const int32_t* __restrict__ idx2,
    const double* __restrict__ params, int tiles, KpThresholds thr, int n_thr, int max_kp,
    int32_t* __restrict__ counts, int32_t* __restrict__ nearest, double* __restrict__ dist_sq) {
#pragma clang fp contract(off)
  __shared__ double2 target[KP_TARGET_TILE];
  // blockIdx.x = tile + tiles * (side + 2 * pair), below 2^31 (checked on the host)
  const int tile = (int)(blockIdx.x % (unsigned)tiles);
  const int rest = (int)(blockIdx.x / (unsigned)tiles);
  const int side = rest & 1, p = rest >> 1;
  const int a = tile * KP_THREADS + (int)threadIdx.x;               // at most ceil(max_kp / 256) * 256 - 1 <= INT32_MAX
  const bool in_width = a < max_kp;
  const size_t out_at = ((size_t)p * 2 + (size_t)side) * (size_t)max_kp + (size_t)a;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);

  KpPair pair;
  const bool vouched = keypoint_pair(maps, n_maps, kp_offsets, n_keypoints, max_kp, idx1, idx2, p, pair);
  const int n_src = vouched ? (side ? pair.count2 : pair.count1) : 0;
  if (tile * KP_THREADS >= n_src) {                                 // workgroup-uniform: only padding rows here
    if (in_width) {
      if (nearest) nearest[out_at] = -1;
      if (dist_sq) dist_sq[out_at] = nan;
    }
    return;
  }
  const int first_src = side ? pair.first2 : pair.first1, first_dst = side ? pair.first1 : pair.first2;
  const int n_dst = side ? pair.count1 : pair.count2;
  const oetr_covis_map src = side ? pair.m2 : pair.m1, dst = side ? pair.m1 : pair.m2;
  const double* __restrict__ P = params + (size_t)p * KP_PARAMS;

  const bool active = a < n_src;                                    // n_src <= max_kp: an active row is in the width
  bool kept = false;
  double pu = nan, pv = nan;
  if (active) {
    const float2 k = keypoints[(size_t)first_src + (size_t)a];      // first_src + a < first_src + n_src <= n_keypoints
    const double u = (double)k.x, v = (double)k.y;
    const double d = depth_at(src, u, v);
    if (side) project21(P, u, v, d, pu, pv); else project12(P, u, v, d, pu, pv);
    kept = d != 0.0 && pu < (double)dst.W && pv < (double)dst.H;    // the reference's test: no lower bound; NaN fails
  }

  double best = __longlong_as_double(0x7ff0000000000000ll);         // +inf
  int best_at = -1;
  if (__syncthreads_or(kept ? 1 : 0)) {                             // workgroup-uniform
    for (int base = 0; base < n_dst; base += KP_TARGET_TILE) {
      const int m = min(KP_TARGET_TILE, n_dst - base);
      __syncthreads();                                              // the previous tile has been read
      if ((int)threadIdx.x < m) {
        const float2 k = keypoints[(size_t)first_dst + (size_t)base + (size_t)threadIdx.x];   // < first_dst + n_dst
        target[threadIdx.x] = make_double2((double)k.x, (double)k.y);
      }
      __syncthreads();
      for (int b = 0; b < m; ++b) {
        const double2 t = target[b];                                // one address for the whole wave: a broadcast
        const double du = pu - t.x, dv = pv - t.y;
        const double d = du * du + dv * dv;
        if (d < best) {
          best = d;
          best_at = base + b;
        }
      }
    }
  }

  if (in_width) {
    if (nearest) nearest[out_at] = kept ? best_at : -1;
    if (dist_sq) dist_sq[out_at] = kept ? best : nan;
  }

  // counters 1 .. 1 + n_thr (counter 0, the keypoint count, is k_keypoint_finish's).  Every lane arrives here.
  int32_t* c = counts + ((size_t)p * 2 + (size_t)side) * (size_t)(KP_HEAD + n_thr);
  const bool first_lane = (threadIdx.x & 63) == 0;
  const int n_kept = __popcll(__ballot(kept));
  if (n_kept == 0) return;                                          // wave-uniform
  if (first_lane) atomicAdd(c + 1, n_kept);
#pragma unroll
  for (int k = 0; k < KP_MAX_THR; ++k) {
    if (k < n_thr) {
      const double th = thr.th[k];
      const int n = __popcll(__ballot(kept && best < th * th));     // false for a NaN threshold
      if (first_lane && n) atomicAdd(c + KP_HEAD + k, n);
    }
  }
}

// one thread per pair and direction; the vouching test k_keypoint_nearest made, made again
__global__ void k_keypoint_finish(const oetr_covis_map* __restrict__ maps, int n_maps, int n_keypoints,
                                  const int32_t* __restrict__ kp_offsets, const int32_t* __restrict__ idx1,
                                  const int32_t* __restrict__ idx2, int n_pairs, int n_thr, int max_kp,
                                  int32_t* __restrict__ counts) {
  const unsigned at = blockIdx.x * blockDim.x + threadIdx.x;
  if (at >= 2u * (unsigned)n_pairs) return;
  const int p = (int)(at >> 1), side = (int)(at & 1u);
  int32_t* c = counts + (size_t)at * (size_t)(KP_HEAD + n_thr);
  KpPair pair;
  if (!keypoint_pair(maps, n_maps, kp_offsets, n_keypoints, max_kp, idx1, idx2, p, pair)) {
    for (int k = 0; k < KP_HEAD + n_thr; ++k) c[k] = -1;
    return;
  }
  c[0] = side ? pair.count2 : pair.count1;
}

namespace {

constexpr const char* ME = "oetr_keypoint_repeatability";

}  // namespace
}  // namespace oetr

using namespace oetr;

extern "C" {

int oetr_keypoint_score_abi_version(void) { return OETR_KEYPOINT_SCORE_ABI_VERSION; }

// The host code dereferences none of its device-pointer arguments (thresholds is host memory) and reads nothing from
// the device.
oetr_status oetr_keypoint_repeatability(const oetr_covis_map* maps, int n_maps, const float* keypoints,
                                        int64_t n_keypoints, const int32_t* kp_offsets, const int32_t* idx1,
                                        const int32_t* idx2, const double* params, int n_pairs,
                                        const double* thresholds, int n_thresholds, int max_kp, int32_t* counts,
                                        int32_t* nearest, double* dist_sq, void* stream) {
  if (!maps || !kp_offsets || !idx1 || !idx2 || !params)
    return entry_fail(ME, OETR_ERR_BAD_ARG, "NULL map table / offsets / index / parameter pointer");
  if (!counts) return entry_fail(ME, OETR_ERR_BAD_ARG, "NULL counts output");
  if (n_maps <= 0 || n_pairs <= 0) return entry_fail(ME, OETR_ERR_BAD_ARG, "need n_maps > 0 and n_pairs > 0");
  if (n_keypoints < 0 || max_kp < 0) return entry_fail(ME, OETR_ERR_BAD_ARG, "need n_keypoints >= 0 and max_kp >= 0");
  if (n_keypoints != 0 && !keypoints) return entry_fail(ME, OETR_ERR_BAD_ARG, "NULL keypoint pointer");
  if (n_thresholds < 0 || n_thresholds > KP_MAX_THR)
    return entry_fail(ME, OETR_ERR_BAD_ARG, "need 0 <= n_thresholds <= " + std::to_string(KP_MAX_THR));
  if (n_thresholds != 0 && !thresholds) return entry_fail(ME, OETR_ERR_BAD_ARG, "NULL thresholds");
  if (n_keypoints > (int64_t)INT32_MAX)
    return entry_fail(ME, OETR_ERR_BAD_SHAPE, "need n_keypoints <= " + std::to_string(INT32_MAX) + " (the offsets are int32)");
  const int per_side = KP_HEAD + n_thresholds;
  const int64_t n_counters = 2 * (int64_t)n_pairs * per_side;
  const int64_t tiles = ((int64_t)max_kp + KP_THREADS - 1) / KP_THREADS;
  const int64_t blocks = 2 * (int64_t)n_pairs * tiles;
  if (n_counters > (int64_t)INT32_MAX || blocks > (int64_t)INT32_MAX)
    return entry_fail(ME, OETR_ERR_BAD_SHAPE, "more than " + std::to_string(INT32_MAX) + " counters or workgroups (2 * "
                         "n_pairs * ceil(max_kp / 256))");
  hipStream_t s = static_cast<hipStream_t>(stream);
  KpThresholds thr;
  for (int k = 0; k < KP_MAX_THR; ++k) thr.th[k] = k < n_thresholds ? thresholds[k] : 0.0;
  // cleared by a kernel, not by a memset node: see clear_i32 (match_score.hip)
  if (oetr_status rc = entry_hip(ME, clear_i32(counts, n_counters, s), "k_clear_i32")) return rc;
  if (blocks > 0) {
    hipLaunchKernelGGL(k_keypoint_nearest, dim3((unsigned)blocks), dim3(KP_THREADS), 0, s, maps, n_maps,
                       reinterpret_cast<const float2*>(keypoints), (int)n_keypoints, kp_offsets, idx1, idx2, params,
                       (int)tiles, thr, n_thresholds, max_kp, counts, nearest, dist_sq);
    if (oetr_status rc = entry_hip(ME, hipGetLastError(), "k_keypoint_nearest")) return rc;
  }
  hipLaunchKernelGGL(k_keypoint_finish, dim3((unsigned)((2 * (int64_t)n_pairs + 255) / 256)), dim3(256), 0, s, maps,
                     n_maps, (int)n_keypoints, kp_offsets, idx1, idx2, n_pairs, n_thresholds, max_kp, counts);
  return entry_hip(ME, hipGetLastError(), "k_keypoint_finish");
}

}  // extern "C"
