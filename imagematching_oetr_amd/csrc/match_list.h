// The match-list device code the entries that score one row per thread share: oetr_match_score (match_score.hip)
// and oetr_homography_match_score (homography.hip).  A call's rows are cut into lists by int32 offsets[n_pairs + 1],
// assumed non-decreasing: list p owns the rows offsets[p] .. offsets[p+1]-1, a row outside every list is scored by
// nobody.  ONE copy of the search, of the wave-level row -> list step, of the list-length rule and of the prologue of
// the per-pair counters, so that both entries give a call's rows the same membership.  pr_list (pose_ransac.hip),
// asm_range (match_assembly.hip) and keypoint_rows (keypoint_score.hip) look alike and stay where they are: they answer
// malformed offsets differently (each offset clamped on its own / the end clamped up to the start / the pair refused).
#pragma once
#include "common.h"

namespace oetr {

// The largest p in [0, n_pairs) with offsets[p] <= m, or -1: the number of such entries, less one.  Reads
// offsets[0 .. n_pairs-1] only.
__device__ __forceinline__ int find_list(const int32_t* __restrict__ offsets, int n_pairs, int m) {
  int lo = 0, hi = n_pairs;
  while (lo < hi) {
    const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);     // lo <= mid < hi <= n_pairs
    if (offsets[mid] <= m) lo = mid + 1; else hi = mid;
  }
  return lo - 1;
}

// The list of row m (`active`: m is a row of the call) of a THREADS-wide workgroup that takes one row per thread:
// p, or -1 for a row in no list, and the wave-uniform p0, the list of the wave's FIRST row (-1: none).  p0 is searched
// once per wave with wave-uniform (scalar) loads; rows ascend with the lane, so for non-decreasing offsets a later row
// m < offsets[p0 + 1] belongs to p0 too: offsets[p0] <= row0 <= m and every later offset is > m.  Only a lane past
// that boundary searches for itself.  A wave with __ballot(active && p != p0) == 0 may load its pair's data by p0.
template <int THREADS>
__device__ __forceinline__ void wave_find_list(const int32_t* __restrict__ offsets, int n_pairs, int n_matches,
                                               bool active, int m, int& p0, int& p) {
  const int64_t row0 = (int64_t)blockIdx.x * THREADS + (int64_t)__builtin_amdgcn_readfirstlane((int)threadIdx.x);
  int end0 = 0;
  p0 = -1;
  if (row0 < (int64_t)n_matches) {
    p0 = __builtin_amdgcn_readfirstlane(find_list(offsets, n_pairs, (int)row0));
    if (p0 >= 0) end0 = offsets[p0 + 1];                            // p0 + 1 <= n_pairs
  }
  p = -1;
  if (active) {
    if (p0 >= 0 && m < end0) {
      p = p0;
    } else {
      p = find_list(offsets, n_pairs, m);
      if (p >= 0 && !(m < offsets[p + 1])) p = -1;
    }
  }
}

// The length of list p as the counters report it: clamped into [0, n_matches], whatever the offsets hold.
__device__ __forceinline__ int32_t list_length(const int32_t* __restrict__ offsets, int p, int n_matches) {
  const long long len = (long long)offsets[p + 1] - (long long)offsets[p];
  return (int32_t)(len < 0 ? 0 : (len > (long long)n_matches ? (long long)n_matches : len));
}

// What a wave's lanes count for.  `counted`: the pair a lane's row counts for, or -1.  any: some lane counts; first:
// the pair of the lowest such lane; one_pair: every counting lane counts for `first`, so the wave can add ballots'
// popcounts from one lane where it would otherwise add per lane.  Every lane of the wave must arrive.
struct WaveCounted {
  bool any, one_pair;
  int first;
};

__device__ __forceinline__ WaveCounted wave_counted(int counted) {
  const unsigned long long counting = __ballot(counted >= 0);
  WaveCounted w = {counting != 0ull, false, -1};
  if (!w.any) return w;                                             // wave-uniform
  w.first = __shfl(counted, __ffsll((long long)counting) - 1, 64);
  w.one_pair = __ballot(counted >= 0 && counted != w.first) == 0ull;
  return w;
}

}  // namespace oetr
