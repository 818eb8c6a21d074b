/* Scoring matches against depth and pose, by index over a SET of depth maps: an extension of liboetr_hip.so.
 *
 * The chain boxes -> crops -> matcher -> keypoints mapped back is judged by whether its matches are correct: the
 * reference's validation_error / compute_epipolar_error (thresholded at 5e-4), get_episym, and pose_evaluate ->
 * get_projected_kp / get_truesym.  oetr_match_score computes those per-match quantities, a flag byte per match
 * and five counters per pair for MANY match lists in one call, reading the depth maps in place through the
 * device table of a depth-map set (oetr_covis_map, include/oetr_covis_set.h: the same table, no second type).
 *
 * The arithmetic is the float64 program tests/match_score_oracle.py::score, operation by operation in the order
 * written there (no contraction into FMAs), with the reference's kept quirks (the UNSQUARED denominators of
 * compute_epipolar_error, ys = ys2 in get_truesym, no positive-depth test, half-to-even rounding of the depth
 * look-up) and its one departure (distances are delivered SQUARED).
 *
 * This header extends include/oetr_hip.h (same library, same status codes, same oetr_last_error) and carries a
 * version of its own; OETR_ABI_VERSION and the versions of the other extensions do not change. */
#ifndef OETR_MATCH_SCORE_H_
#define OETR_MATCH_SCORE_H_

#include "oetr_covis_set.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OETR_MATCH_SCORE_ABI_VERSION 1

/* float64 per pair in `params`: fx fy cx cy of camera 1, fx fy cx cy of camera 2, R (row major), t of T_1to2 */
#define OETR_MATCH_SCORE_PARAM_DOUBLES 20
/* counters per pair: matches, epi_ref < epi_thr, episym < sym_thr, both depths, both depths and
 * reproj21_sq < px_thr^2 */
#define OETR_MATCH_SCORE_COUNTERS 5

/* flag bits of one match */
#define OETR_MATCH_DEPTH1 1  /* map 1 has depth under keypoint 1 */
#define OETR_MATCH_DEPTH2 2  /* map 2 has depth under keypoint 2 */
#define OETR_MATCH_EPI 4     /* epi_ref < epi_thr */
#define OETR_MATCH_EPISYM 8  /* episym < sym_thr */
#define OETR_MATCH_REPROJ 16 /* both depths and reproj21_sq < px_thr * px_thr */

int oetr_match_score_abi_version(void);

/* n_pairs match lists over the maps of a set, concatenated: list p is the rows offsets[p] .. offsets[p+1]-1 of
 * k1 / k2 (float32 (u, v) in the original pictures; widened to float64, which is exact), scored for depth map
 * maps[idx1[p]] against maps[idx2[p]] under params[p].  Per row m: values[0..3][m] = epi_ref, episym,
 * reproj12_sq, reproj21_sq (values is float64 [4][n_matches]; NULL: not stored), flags[m] (the bits above);
 * per pair counts[p][0..4].  A threshold that is NaN is OFF: its flag is never set and its counter reads -1.
 *
 * n_matches is a HOST value: it sets the grid (one thread per row) and bounds every row access.  The host code
 * dereferences none of the pointers and learns nothing from device memory.
 *
 * Memory safety does not depend on device data.  The thread of row m < n_matches reads only k1[m], k2[m],
 * offsets[0..n_pairs], idx1[p], idx2[p], params[p], the two table rows, and a depth pixel whose rounded
 * coordinates passed the range test in float64 against that row's H, W; it writes only row m of values and
 * flags, and adds to counts[p].
 *
 * Row m belongs to the largest p with offsets[p] <= m (binary search: offsets are assumed non-decreasing) and
 * is scored only if also m < offsets[p+1].  A row that belongs to no list - before offsets[0], at or after
 * offsets[n_pairs] - gets flags = 0 and NaN values.  Offsets that are not non-decreasing give UNSPECIFIED
 * flags, values and counters, but never a read or a write out of bounds.
 *
 * A pair is NEVER DEREFERENCED when for either side the index is outside [0, n_maps), the map's pointer is NULL
 * or its H or W is outside 1..OETR_COVIS_MAX_SIDE (the rule of oetr_covis_boxes_indexed without max_pixels: the
 * grid is over matches): its rows get flags = 0 and NaN values, all five of its counters read -1, and the other
 * pairs of the call are unaffected.
 *
 * counts[p][0] = offsets[p+1] - offsets[p] clamped to [0, n_matches]; counts[p][3] counts the rows with both
 * depths whatever the thresholds.
 *
 * The call only enqueues on `stream`: one kernel that clears counts, the scoring kernel (none for
 * n_matches == 0, which is legal) and a finishing kernel over pairs.  It needs no workspace (the counters
 * accumulate in counts itself), reads nothing back, allocates nothing, and can be captured into a HIP graph as
 * three nodes in a line; a replay sees whatever the buffers hold at replay time.  The counters are integer
 * atomics: results are bit-identical from run to run and do not depend on the order of the pair list.
 *
 * Checked on the host before anything is enqueued: NULL maps / idx1 / idx2 / params / offsets / counts, NULL k1 /
 * k2 / flags unless n_matches == 0 (no row, nothing to point at), n_maps <= 0, n_pairs <= 0, n_matches < 0
 * -> OETR_ERR_BAD_ARG; n_matches > INT32_MAX (the offsets are int32) or n_pairs > INT32_MAX / 5
 * -> OETR_ERR_BAD_SHAPE. */
oetr_status oetr_match_score(const oetr_covis_map *maps, int n_maps, const int32_t *idx1, const int32_t *idx2,
                             const double *params, const int32_t *offsets, int n_pairs, const float *k1,
                             const float *k2, int64_t n_matches, double epi_thr, double sym_thr, double px_thr,
                             double *values, uint8_t *flags, int32_t *counts, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* OETR_MATCH_SCORE_H_ */
