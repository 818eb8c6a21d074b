/* A least-squares refit of relative poses on their inliers, on the device: an extension of liboetr_hip.so.
 *
 * oetr_pose_ransac (include/oetr_pose_ransac.h) delivers the bare model of a minimal 7-point sample.
 * oetr_pose_refit takes such a model per pair - the one oetr_pose_ransac selected, or any other - and the same match
 * lists, runs a FIXED number of least-squares rounds on the model's inliers and delivers what oetr_pose_ransac
 * delivers: the model, the pose, the two cosines of the pose error, counters and the inlier marks.  oetr_pose_ransac,
 * its header and its results do not change.
 *
 * The arithmetic is the float64 program tests/pose_refit_oracle.py, operation by operation in the order written there
 * (no contraction into FMAs, IEEE division and square root, every decision a comparison, every sum in a specified
 * order).  It is THE PROJECT'S OWN STATEMENT: no parity with cv2 is claimed.  No Hartley normalisation, no projection
 * onto the essential manifold, no second threshold, no non-linear minimisation, no adaptive termination.
 *
 * Per pair, with the 20 doubles of OETR_MATCH_SCORE_PARAM_DOUBLES, its list of rows (u, v) and model_in[p] (9 doubles,
 * row major, in the normalised coordinates of oetr_pose_ransac):
 *   start    a non-finite model_in or a list of 0 rows: no pose.  Otherwise F = model_in as given (no rescaling) and
 *            count = its inliers over ALL rows under oetr_pose_ransac's test;
 *   round    (refit_iters times) the inlier rows of F, fewer than 8: stop; w = (x2 x1, x2 y1, x2, y2 x1, y2 y1, y2,
 *            x1, y1, 1) per row; the upper triangle of M = sum w w^T, each of its 44 floating-point sums taken as 256
 *            partial sums by the row's position in the list modulo 256 and one fixed tree over them; the entry k of F
 *            of largest magnitude (the lowest on a tie) is held at 1; the 8 x 9 system (M without row and column k,
 *            right-hand side -M[:, k]) is eliminated by Gauss-Jordan with partial pivoting, a zero or NaN pivot: stop;
 *            the candidate is scaled to unit norm and scored over ALL rows; it replaces F iff it is finite and has at
 *            least as many inliers, otherwise F stays and the rounds stop;
 *   deliver  decomposition, cheirality votes over the inlier rows of the delivered F, cosines: as oetr_pose_ransac.
 * The delivered model never has fewer inliers than model_in.  With refit_iters = 0 and model_in = the model of
 * oetr_pose_ransac, model, pose, cosines, inliers and counts[3..4] are bit for bit those of oetr_pose_ransac.
 *
 * This header extends include/oetr_hip.h (same library, same status codes, same oetr_last_error) and carries a
 * version of its own; OETR_ABI_VERSION and the versions of the other extensions do not change. */
#ifndef OETR_POSE_REFIT_H_
#define OETR_POSE_REFIT_H_

#include "oetr_match_score.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OETR_POSE_REFIT_ABI_VERSION 1
#define OETR_POSE_REFIT_MAX_ITERS 8
#define OETR_POSE_REFIT_COUNTERS 5

int oetr_pose_refit_abi_version(void);

/* n_pairs match lists, concatenated as oetr_pose_ransac takes them and oetr_assemble_matches leaves them: list p is the
 * rows offsets[p] .. offsets[p+1]-1 of k1 / k2 (float32 (u, v) in the original pictures, widened exactly), both offsets
 * clamped into [0, n_matches].  n_matches is a HOST value that bounds every row access.  Offsets that are not
 * non-decreasing give UNSPECIFIED results, but never an access out of bounds.  model_in: float64 [n_pairs][9].
 *
 * Outputs: model[p] the delivered F, pose[p] = R (row major) then t of the chosen candidate, cosines[p], and
 * counts[p] = { the list's length, the inliers of model_in, the rounds accepted (0..refit_iters; -1: no pose), the
 * inliers of the delivered model, the votes of the chosen candidate }.  A pair without a pose has NaN model, pose and
 * cosines and 0 inliers and votes; counts[p][2] < 0 exactly then.  inliers[m] (NULL: not stored) is 1 for the inlier
 * rows of the delivered models and 0 for every other row below n_matches.  No output may overlap an input.
 *
 * The call only enqueues on `stream`: ONE kernel, one workgroup per pair, whatever the lists hold.  It needs no
 * workspace, reads nothing back, allocates nothing, uses no memset node and no floating-point atomics: results are
 * bit-identical from run to run, and the call can be captured into a HIP graph.
 *
 * Checked on the host before anything is enqueued: NULL params / offsets / model_in / model / pose / cosines / counts,
 * NULL k1 / k2 unless n_matches == 0, n_pairs <= 0, n_matches < 0, refit_iters outside 0..8, px_thr not finite or
 * <= 0 -> OETR_ERR_BAD_ARG; n_matches > INT32_MAX -> OETR_ERR_BAD_SHAPE. */
oetr_status oetr_pose_refit(const double *params, const int32_t *offsets, int n_pairs, const float *k1, const float *k2,
                            int64_t n_matches, const double *model_in, double px_thr, int refit_iters, double *model,
                            double *pose, double *cosines, int32_t *counts, uint8_t *inliers, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* OETR_POSE_REFIT_H_ */
