/* Scoring matches and overlap boxes against a HOMOGRAPHY: an extension of liboetr_hip.so.
 *
 * Every other ground truth of the evaluation chain comes from depth maps and poses (include/oetr_covis.h,
 * oetr_covis_set.h, oetr_match_score.h, oetr_keypoint_score.h).  The reference has a second protocol that needs
 * neither, the planar one on HPatches: dloc/evaluate/eval_hpatches.py computes h_evaluate(H_gt, kpts0, kpts1, matches)
 * per pair and accumulates mean(dist <= thr) for thr = 1 .. 15.  oetr_homography_match_score computes those distances
 * and the per-threshold counters for MANY match lists in one call; oetr_homography_boxes computes the overlap boxes
 * of many pairs of pictures related by a homography, with the outputs of oetr_covis_boxes.
 *
 * The arithmetic is the float64 program tests/homography_oracle.py (score / overlap_box), operation by operation in
 * the order written there (no contraction into FMAs, IEEE division, rint for the landing pixel).  Its one departure
 * from h_evaluate is the project's standing one: the distance is delivered SQUARED and compared with thr * thr.  The
 * BOXES are this project's own statement - the reference has no overlap boxes under a homography: they are
 * numpy_overlap_box (include/oetr_covis.h) with the depth-and-pose warp replaced by H.
 *
 * H maps pixel coordinates of picture 1 to picture 2; pixel centres sit at INTEGER coordinates (the convention of
 * HPatches' H_1_k files and of h_evaluate).
 *
 * This header extends include/oetr_hip.h (same library, same status codes, same oetr_last_error) and carries a
 * version of its own; OETR_ABI_VERSION and the versions of the other extensions do not change. */
#ifndef OETR_HOMOGRAPHY_H_
#define OETR_HOMOGRAPHY_H_

#include "oetr_covis.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OETR_HOMOGRAPHY_ABI_VERSION 1

/* float64 per pair in `params`: H row major in [0..8], then W1, H1, W2, H2 as whole numbers in [9..12]; [13..15] are
 * reserved and ignored.  The match scoring reads [0..8] only. */
#define OETR_HOMOGRAPHY_PARAM_DOUBLES 16
#define OETR_HOMOGRAPHY_MAX_THRESHOLDS 16

int oetr_homography_abi_version(void);

/* n_pairs match lists, concatenated: list p is the rows offsets[p] .. offsets[p+1]-1 of k1 / k2 (float32 (x, y);
 * widened to float64, which is exact), scored under the H of params[p].  Per row m, with (x, y) = k1[m] and
 * (x2, y2) = k2[m]:
 *     a_r = (h_r0 * x + h_r1 * y) + h_r2   for r = 0, 1, 2
 *     pu = a0 / a2,  pv = a1 / a2
 *     dist_sq[m] = (x2 - pu) * (x2 - pu) + (y2 - pv) * (y2 - pv)       (dist_sq NULL: not stored)
 * and per pair counts[p][0] = the list's length, counts[p][1 + t] = its rows with dist_sq <= thresholds[t] *
 * thresholds[t].  A NaN dist_sq or a NaN threshold fails that comparison; a row with a2 == 0 or a non-finite H gives
 * inf or NaN and is not special-cased, as in the reference; an empty list counts 0 at every threshold (the reference's
 * dist = [inf] substitute).
 *
 * `thresholds` is a HOST array of n_thresholds doubles, read DURING THE CALL: the squares go into the scoring
 * kernel's arguments, so a captured graph node carries the thresholds of its capture, whatever the array holds later.
 *
 * n_matches is a HOST value: it sets the grid (one thread per row) and bounds every row access.  The host code
 * dereferences none of the device pointers and learns nothing from device memory.
 *
 * Memory safety does not depend on device data.  The thread of row m < n_matches reads only k1[m], k2[m],
 * offsets[0..n_pairs] and params[p][0..8] with p in [0, n_pairs) by construction of the search; it writes only
 * dist_sq[m], and adds to counts[p].
 *
 * Row m belongs to the largest p with offsets[p] <= m (binary search: offsets are assumed non-decreasing) and is
 * scored only if also m < offsets[p+1].  A row that belongs to no list - before offsets[0], at or after
 * offsets[n_pairs] - gets a NaN dist_sq and is counted nowhere.  Offsets that are not non-decreasing give UNSPECIFIED
 * values and counters, but never a read or a write out of bounds.  counts[p][0] = offsets[p+1] - offsets[p] clamped
 * to [0, n_matches].
 *
 * The call only enqueues on `stream`: one kernel that clears counts and writes the list lengths, and the scoring
 * kernel (none for n_matches == 0, which is legal).  It needs no workspace (the counters accumulate in counts itself,
 * summed inside a wave over the lanes of one pair before the integer atomics), reads nothing back, allocates nothing,
 * and can be captured into a HIP graph as two nodes in a line; a replay scores whatever the buffers hold at replay
 * time.  Integer atomics commute: results are bit-identical from run to run.
 *
 * Checked on the host before anything is enqueued: NULL params / offsets / counts, NULL k1 / k2 unless
 * n_matches == 0, NULL thresholds unless n_thresholds == 0, n_thresholds outside 0..OETR_HOMOGRAPHY_MAX_THRESHOLDS,
 * n_pairs <= 0, n_matches < 0 -> OETR_ERR_BAD_ARG; n_matches > INT32_MAX (the offsets are int32) or
 * n_pairs > INT32_MAX / 17 -> OETR_ERR_BAD_SHAPE. */
oetr_status oetr_homography_match_score(const double *params, const int32_t *offsets, int n_pairs, const float *k1,
                                        const float *k2, int64_t n_matches, const double *thresholds, int n_thresholds,
                                        double *dist_sq, int32_t *counts, void *stream);

/* Bytes of workspace oetr_homography_boxes needs for n_pairs pairs (0 for n_pairs <= 0). */
size_t oetr_homography_workspace_bytes(int n_pairs);

/* Overlap boxes of n_pairs pairs of pictures under their homographies.  For every pixel (u, v) of picture 1
 * (0 <= u < W1, 0 <= v < H1), with a0, a1, a2 as above: the pixel is KEPT when a2 > 0 (it lies on picture 2's side of
 * the horizon line) and its landing pixel i = rint(a0 / a2), j = rint(a1 / a2) (half to even) has 0 <= i < W2 and
 * 0 <= j < H2 - tested in float64 before any conversion, false for NaN.  count[p] = the kept pixels (count NULL: not
 * stored), box1[p] = (min u, min v, max u, max v) and box2[p] = (min i, min j, max i, max j) over them as float32,
 * valid[p] = count > 0; the boxes are zeros when not valid.  These are the outputs of oetr_covis_boxes.
 *
 * The per-pixel evaluation is deliberate: the boxes are defined over the integer pixel set, and the brute-force
 * count is what makes them exact.
 *
 * The call reads ONLY the parameter blocks - no image memory at all - so memory safety does not depend on device
 * data.  max_h1 / max_w1 are HOST values that set the grid.  A pair is NEVER EVALUATED, and reports count = -1,
 * valid = 0 and zero boxes with the other pairs of the call unaffected, when its W1, H1, W2, H2 are not whole numbers
 * in 1..OETR_COVIS_MAX_SIDE, or H1 > max_h1, or W1 > max_w1.
 *
 * The call only enqueues on `stream`: a kernel that clears the workspace (which may hold anything on entry), the
 * pixel kernel, and a finishing kernel that decodes the workspace.  The reductions are made within the wave and the
 * workgroup first, then by integer min / max / add atomics into the workspace: results are bit-identical from run to
 * run.  Nothing is read back or allocated; the call can be captured into a HIP graph.
 *
 * Checked on the host before anything is enqueued: NULL params, NULL box1 / box2 / valid, n_pairs <= 0, workspace
 * NULL or smaller than oetr_homography_workspace_bytes(n_pairs) -> OETR_ERR_BAD_ARG; n_pairs > INT32_MAX / 17,
 * max_h1 or max_w1 outside 1..OETR_COVIS_MAX_SIDE -> OETR_ERR_BAD_SHAPE. */
oetr_status oetr_homography_boxes(const double *params, int n_pairs, int max_h1, int max_w1, void *workspace,
                                  size_t workspace_bytes, float *box1, float *box2, uint8_t *valid, int32_t *count,
                                  void *stream);

#ifdef __cplusplus
}
#endif
#endif /* OETR_HOMOGRAPHY_H_ */
