/* Keypoint repeatability against depth and pose, by index over a SET of depth maps: an extension of liboetr_hip.so.
 *
 * oetr_match_score (include/oetr_match_score.h) says what share of a matcher's matches is correct.  The counterpart
 * - of the keypoints that COULD have been matched, how many have a partner in the other picture at all - is the
 * reference's repeatability (pose_evaluate, dloc/evaluate/utils/evaluation.py:135-179; get_repeatability,
 * utils.py:214-236): every keypoint of one picture is projected into the other with depth and pose, the ones that
 * have a depth and land inside the other picture are kept, and each kept one looks for the nearest keypoint of the
 * other picture - an N x M table of squared distances per pair and direction.  oetr_keypoint_repeatability does that
 * for MANY pairs of an image set in one call, both directions, reading the depth maps in place through the device
 * table of a depth-map set (oetr_covis_map, include/oetr_covis_set.h: the same table, no second type) and the
 * keypoints of every image from ONE concatenated array.  The nearest neighbour it finds is also the ground-truth
 * correspondence between the two keypoint sets.
 *
 * The arithmetic is the float64 program tests/keypoint_score_oracle.py, operation by operation in the order
 * written there (no contraction into FMAs), with the reference's kept quirks (the kept-row test has no lower bound
 * and no positive-depth test, a NaN depth counts as a depth, half-to-even rounding of the depth look-up) and its
 * departures (a target keypoint with a non-finite coordinate never wins, where the reference's amin would return
 * NaN for every row; an empty target set gives -1 / +inf, where the reference raises).
 *
 * This header extends include/oetr_hip.h (same library, same status codes, same oetr_last_error) and carries a
 * version of its own; OETR_ABI_VERSION and the versions of the other extensions do not change. */
#ifndef OETR_KEYPOINT_SCORE_H_
#define OETR_KEYPOINT_SCORE_H_

#include "oetr_match_score.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OETR_KEYPOINT_SCORE_ABI_VERSION 1

/* thresholds per call, at most */
#define OETR_KEYPOINT_SCORE_MAX_THRESHOLDS 8
/* counters per pair and direction BEFORE the thresholds': keypoints of the source picture, kept rows */
#define OETR_KEYPOINT_SCORE_HEAD_COUNTERS 2

int oetr_keypoint_score_abi_version(void);

/* For p in [0, n_pairs) and both directions s (0: picture idx1[p] -> picture idx2[p], 1: the other way round):
 * every keypoint a of the source picture is projected into the target picture under params[p]
 * (OETR_MATCH_SCORE_PARAM_DOUBLES float64, the layout of oetr_match_score.h; direction 1 uses R^T and R^T t,
 * recomputed), KEPT when its depth d != 0 and its projection (pu, pv) has pu < W and pv < H of the target map (NaN
 * fails), and a kept row gets
 *     dist_sq[p][s][a] = min over b of (pu - u[b]) * (pu - u[b]) + (pv - v[b]) * (pv - v[b])
 * over the target picture's keypoints and nearest[p][s][a] = the smallest b that attains it (strict "<" in
 * ascending order from +inf / -1: a NaN or infinite distance never wins; no target keypoint: -1 / +inf).  Rows that
 * are not kept, and rows a at or past the source picture's keypoint count, hold -1 / NaN.  nearest is int32
 * [n_pairs][2][max_kp], dist_sq float64 [n_pairs][2][max_kp]; either may be NULL (not stored).
 *
 * counts is int32 [n_pairs][2][2 + n_thresholds]: the source picture's keypoints, the kept rows, and for each
 * threshold the kept rows with dist_sq < th * th (float64; false for a NaN threshold).
 *
 * keypoints is device float32 [n_keypoints][2], 8-byte aligned, (u, v) in the original pictures (widened to float64,
 * which is exact); picture k of the set owns the rows kp_offsets[k] .. kp_offsets[k+1] - 1 (kp_offsets: device int32
 * [n_maps + 1]).  thresholds is HOST memory (n_thresholds doubles, read during the call; NULL for none).
 *
 * n_keypoints and max_kp are HOST values.  max_kp is the largest keypoint count per picture the caller vouches
 * for: it sets the grid (one thread per source keypoint up to max_kp, times two directions, times pairs) and is
 * the padded width of nearest and dist_sq.  The host code dereferences none of the device pointers and learns
 * nothing from device memory.
 *
 * Memory safety does not depend on device data that has not been tested.  A pair is NEVER DEREFERENCED - its
 * nearest / dist_sq rows hold -1 / NaN, all of its counters in both directions read -1, the other pairs of the call
 * are unaffected - when for either of its sides the index is outside [0, n_maps), the map's pointer is NULL, its H
 * or W is outside 1..OETR_COVIS_MAX_SIDE, or the picture's keypoint rows are not vouched for: kp_offsets[k] < 0,
 * kp_offsets[k+1] > n_keypoints, or a count kp_offsets[k+1] - kp_offsets[k] that is negative or exceeds max_kp.
 * Every keypoint row that is read therefore lies in [0, n_keypoints), every output row in [0, max_kp), and a depth
 * pixel is read only when its rounded coordinates passed the range test in float64 against that map's H, W.
 * kp_offsets that are not non-decreasing may give UNSPECIFIED scores (pictures sharing rows) but never a read or a
 * write out of bounds.
 *
 * The call only enqueues on `stream`: one kernel that clears counts, the scoring kernel (none for max_kp == 0,
 * which is legal) and a finishing kernel over pairs.  It needs no workspace (the counters accumulate in counts
 * itself), reads nothing back, allocates nothing, and can be captured into a HIP graph as three nodes in a line; a
 * replay sees whatever the buffers hold at replay time.  The counters are integer atomics and every row is one
 * thread's: results are bit-identical from run to run and do not depend on the order of the pair list.
 *
 * Checked on the host before anything is enqueued: NULL maps / kp_offsets / idx1 / idx2 / params / counts, NULL
 * keypoints unless n_keypoints == 0, NULL thresholds unless n_thresholds == 0, n_maps <= 0, n_pairs <= 0,
 * n_keypoints < 0, max_kp < 0, n_thresholds outside 0..OETR_KEYPOINT_SCORE_MAX_THRESHOLDS -> OETR_ERR_BAD_ARG;
 * n_keypoints > INT32_MAX (the offsets are int32), or more than INT32_MAX counters, workgroups
 * (2 * n_pairs * ceil(max_kp / 256)) -> OETR_ERR_BAD_SHAPE. */
oetr_status oetr_keypoint_repeatability(const oetr_covis_map *maps, int n_maps, const float *keypoints,
                                        int64_t n_keypoints, const int32_t *kp_offsets, const int32_t *idx1,
                                        const int32_t *idx2, const double *params, int n_pairs,
                                        const double *thresholds, int n_thresholds, int max_kp, int32_t *counts,
                                        int32_t *nearest, double *dist_sq, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* OETR_KEYPOINT_SCORE_H_ */
