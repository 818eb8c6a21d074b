// The depth-and-pose device code the evaluation entries share: oetr_covis_boxes_indexed (covis.hip),
// oetr_match_score (match_score.hip) and oetr_keypoint_repeatability (keypoint_score.hip).  ONE copy of
// the test that vouches for a pair's two table rows, of the half-to-even depth read and of the two
// projections, so that a keypoint scored through either scoring entry gives the same bits and a
// correction is made once.  The projections are tests/keypoint_score_oracle.py::project (the second half
// of tests/match_score_oracle.py::score) LITERALLY: float64, every operation rounded on its own in the
// order and with the parentheses written there - `fp contract(off)` in every function that does float64
// arithmetic, whatever the flags of the file that includes it.
#pragma once
#include "../../include/oetr_covis_set.h"
#include "common.h"

namespace oetr {

// A table row a call may dereference: a pointer and sides within 1..OETR_COVIS_MAX_SIDE.
__device__ __forceinline__ bool map_usable(const oetr_covis_map& m) {
  return m.depth != nullptr && m.H >= 1 && m.H <= OETR_COVIS_MAX_SIDE && m.W >= 1 && m.W <= OETR_COVIS_MAX_SIDE;
}

// Both table rows of pair p, or false when the pair must not be dereferenced: an index outside [0, n_maps)
// (a and b are then not written) or a row that fails `usable` - map_usable, or an entry's stricter test.
template <class Usable>
__device__ __forceinline__ bool pair_maps(const oetr_covis_map* __restrict__ maps, int n_maps,
                                          const int32_t* __restrict__ idx1, const int32_t* __restrict__ idx2, int p,
                                          oetr_covis_map& a, oetr_covis_map& b, Usable usable) {
  const int i1 = idx1[p], i2 = idx2[p];
  if (i1 < 0 || i1 >= n_maps || i2 < 0 || i2 >= n_maps) return false;
  a = maps[i1];
  b = maps[i2];
  return usable(a) && usable(b);
}

__device__ __forceinline__ bool pair_maps(const oetr_covis_map* __restrict__ maps, int n_maps,
                                          const int32_t* __restrict__ idx1, const int32_t* __restrict__ idx2, int p,
                                          oetr_covis_map& a, oetr_covis_map& b) {
  return pair_maps(maps, n_maps, idx1, idx2, p, a, b, [](const oetr_covis_map& m) { return map_usable(m); });
}

// Depth at (rint(v), rint(u)), half to even, 0 outside the map.  The range test is made in float64 on the rounded
// coordinates: NaN and +-inf fail it, -0 passes; only then is anything converted to an integer.
__device__ __forceinline__ double depth_at(const oetr_covis_map& m, double u, double v) {
#pragma clang fp contract(off)
  const double c = rint(u), r = rint(v);
  if (!(c >= 0.0 && c < (double)m.W && r >= 0.0 && r < (double)m.H)) return 0.0;
  return (double)m.depth[(size_t)(int)r * (size_t)m.W + (size_t)(int)c];
}

// P: a pair's 20 doubles (include/oetr_match_score.h).  reverse=False of the oracle's project: the keypoint
// (u, v) of picture 1, at depth d, in picture 2.
__device__ __forceinline__ void project12(const double* __restrict__ P, double u, double v, double d, double& pu,
                                          double& pv) {
#pragma clang fp contract(off)
  const double fx1 = P[0], fy1 = P[1], cx1 = P[2], cy1 = P[3], fx2 = P[4], fy2 = P[5], cx2 = P[6], cy2 = P[7];
  const double R00 = P[8], R01 = P[9], R02 = P[10], R10 = P[11], R11 = P[12], R12 = P[13], R20 = P[14],
               R21 = P[15], R22 = P[16];
  const double t0 = P[17], t1 = P[18], t2 = P[19];
  const double x1 = (u - cx1) / fx1, y1 = (v - cy1) / fy1;
  const double X1 = x1 * d, Y1 = y1 * d;
  const double p0 = ((R00 * X1 + R01 * Y1) + R02 * d) + t0;
  const double p1 = ((R10 * X1 + R11 * Y1) + R12 * d) + t1;
  const double p2 = ((R20 * X1 + R21 * Y1) + R22 * d) + t2;
  pu = fx2 * (p0 / p2) + cx2;
  pv = fy2 * (p1 / p2) + cy2;
}

// ... reverse=True: a keypoint of picture 2 in picture 1, under R^T and R^T t.
__device__ __forceinline__ void project21(const double* __restrict__ P, double u, double v, double d, double& pu,
                                          double& pv) {
#pragma clang fp contract(off)
  const double fx1 = P[0], fy1 = P[1], cx1 = P[2], cy1 = P[3], fx2 = P[4], fy2 = P[5], cx2 = P[6], cy2 = P[7];
  const double R00 = P[8], R01 = P[9], R02 = P[10], R10 = P[11], R11 = P[12], R12 = P[13], R20 = P[14],
               R21 = P[15], R22 = P[16];
  const double t0 = P[17], t1 = P[18], t2 = P[19];
  const double x2 = (u - cx2) / fx2, y2 = (v - cy2) / fy2;
  const double m0 = (R00 * t0 + R10 * t1) + R20 * t2;
  const double m1 = (R01 * t0 + R11 * t1) + R21 * t2;
  const double m2 = (R02 * t0 + R12 * t1) + R22 * t2;
  const double X2 = x2 * d, Y2 = y2 * d;
  const double q0 = ((R00 * X2 + R10 * Y2) + R20 * d) - m0;
  const double q1 = ((R01 * X2 + R11 * Y2) + R21 * d) - m1;
  const double q2 = ((R02 * X2 + R12 * Y2) + R22 * d) - m2;
  pu = fx1 * (q0 / q2) + cx1;
  pv = fy1 * (q1 / q2) + cy1;
}

}  // namespace oetr
