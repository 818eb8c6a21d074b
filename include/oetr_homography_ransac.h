/* Homographies from match lists, by RANSAC with a refit on the device: an extension of liboetr_hip.so.
 *
 * The planar protocol (include/oetr_homography.h) scores matches and boxes against a homography GIVEN from outside.
 * The reference also ESTIMATES a planar transform from the matches: pr_evaluate / pr_evaluate_cv
 * (dloc/evaluate/utils/evaluation.py) fit a similarity or affine map by skimage.measure.ransac or cv2.estimateAffine*
 * per pair on the host and carry landmarks across with homo_trans.  oetr_homography_ransac estimates a FULL
 * homography for MANY match lists in one call, refits it on its inliers, and delivers the four squared corner
 * distances to H_gt; the square roots and the mean stay with the caller.
 *
 * The arithmetic is the float64 program tests/homography_ransac_oracle.py, operation by operation in the order written
 * there (no contraction into FMAs, IEEE division and square root, every decision a comparison, the order of every sum
 * of the refit included).  It is THE PROJECT'S OWN STATEMENT: no parity with skimage or cv2 is claimed.
 *
 * Per pair, with the 16 doubles of OETR_HOMOGRAPHY_PARAM_DOUBLES (H_gt row major in [0..8], then W1, H1, W2, H2) and
 * its list of rows (u, v):
 *   normalise  side i: c_i = ((W_i - 1) / 2, (H_i - 1) / 2), s_i = (W_i + H_i) / 2, x = (u - c.x) / s, y = (v - c.y) / s;
 *              thr_n = px_thr / s_2.  H_gt is not needed for the estimate: NaN there means "no ground truth" (the
 *              estimate is made, corner_sq is NaN).  A pair whose sizes are not whole numbers in
 *              1..OETR_COVIS_MAX_SIDE is not estimated: its six counters read -1;
 *   sample     hypothesis h draws 4 distinct rows with the counter-based generator of oetr_pose_ransac, of
 *              (seed, pair_id, h, draw); pair_id = pair_ids[p], or p when pair_ids is NULL; a list of fewer than 4
 *              rows has no hypotheses;
 *   solve      the closed form through the projective bases of the two quadruples, Hn = B adj(A), scaled to unit
 *              norm, signed so that a2 of the first sample row is not negative; one model per hypothesis, absent
 *              (all NaN) when an entry is not finite or a sample row has a2 <= 0.  No other conditioning test;
 *   score      with a_r = (h_r0 x + h_r1 y) + h_r2, a row is an inlier iff a2 > 0 and
 *              (x2 a2 - a0)^2 + (y2 a2 - a1)^2 < thr_n^2 (a2 a2); a model with a non-finite entry scores -1;
 *   select     most inliers, the lowest model number on a tie; no finite model: no homography;
 *   refit      refit_iters rounds: the normal equations of the DLT with h22 = 1 over the inlier rows of the current
 *              model, every sum in the specified order (256 partial sums by list position modulo 256, then a fixed
 *              tree), Gauss-Jordan with partial pivoting; the candidate is scored over all rows and accepted iff it is
 *              finite and has at least the inliers of the current model, otherwise the rounds stop;
 *   deliver    model[p] = Hn, the matrix that was scored; H[p] = T2^-1 Hn T1 in pixel coordinates, unit Frobenius
 *              norm - what oetr_homography_match_score and oetr_homography_boxes take in [0..8] of their blocks;
 *   errors     corner_sq[p][c]: the squared distance between corner c of picture 1 - (0,0), (W1-1,0), (W1-1,H1-1),
 *              (0,H1-1) - warped by H and by H_gt; NaN without a model or ground truth, or where a divisor is 0.
 *
 * This header extends include/oetr_hip.h (same library, same status codes, same oetr_last_error) and carries a
 * version of its own; OETR_ABI_VERSION and the versions of the other extensions do not change. */
#ifndef OETR_HOMOGRAPHY_RANSAC_H_
#define OETR_HOMOGRAPHY_RANSAC_H_

#include "oetr_homography.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OETR_HOMOGRAPHY_RANSAC_ABI_VERSION 1
#define OETR_HOMOGRAPHY_RANSAC_MAX_HYPOTHESES 4096
#define OETR_HOMOGRAPHY_RANSAC_MAX_MODELS 4096
#define OETR_HOMOGRAPHY_RANSAC_MAX_REFIT 4
#define OETR_HOMOGRAPHY_RANSAC_COUNTERS 6

int oetr_homography_ransac_abi_version(void);

/* Bytes of workspace for n_pairs pairs of n_models models each (n_models = n_hyp, or n_models_in): the models as
 * float64 [n_pairs][n_models][9], then their inlier counts as int32 [n_pairs][n_models].  0 when either is <= 0. */
size_t oetr_homography_ransac_workspace_bytes(int n_pairs, int n_models);

/* n_pairs match lists, concatenated as oetr_match_score takes them and oetr_assemble_matches leaves them: list p is the
 * rows offsets[p] .. offsets[p+1]-1 of k1 / k2 (float32 (u, v) in the original pictures, widened exactly), both offsets
 * clamped into [0, n_matches].  n_matches is a HOST value that bounds every row access.  Offsets that are not
 * non-decreasing give UNSPECIFIED results, but never an access out of bounds.
 *
 * models_in NULL: n_hyp hypotheses per pair are sampled and solved (n_models = n_hyp; n_models_in is ignored).
 * models_in non-NULL (float64 [n_pairs][n_models_in][9], in NORMALISED coordinates): sampling and solving are skipped
 * and the caller's models are scored, selected and refitted (n_hyp and seed are ignored); the models part of the
 * workspace is left alone.
 *
 * Outputs: model[p] the delivered Hn, H[p], corner_sq[p], and counts[p] = { the list's length, the finite models, the
 * number of the selected model or -1, the inliers of the selected minimal model, the inliers of the delivered model,
 * the refit rounds accepted }.  A pair without a homography has NaN model, H and corner_sq and 0 in its last three
 * counters.  inliers[m] (NULL: not stored) is 1 for the inlier rows of the DELIVERED models and 0 for every other row
 * below n_matches.  Every output element is written by exactly one thread.
 *
 * The call only enqueues on `stream`: the solving kernel (not with models_in), the scoring kernel and the finishing
 * kernel, in a line, whatever the lists hold.  It reads nothing back, allocates nothing, uses no memset node and no
 * floating-point atomics: results are bit-identical from run to run, and the call can be captured into a HIP graph.
 *
 * Memory safety rests on host values and on values tested on the device: sample indices lie below the clamped list
 * length by construction of the sampler, a model number forms an address only after the compare against n_models.
 *
 * Checked on the host before anything is enqueued: NULL params / offsets / workspace / model / H / corner_sq / counts,
 * NULL k1 / k2 unless n_matches == 0, n_pairs <= 0, n_matches < 0, n_hyp outside 1..4096 (models_in NULL), n_models_in
 * outside 1..4096 (otherwise), refit_iters outside 0..4, px_thr not finite or <= 0, workspace smaller than
 * oetr_homography_ransac_workspace_bytes -> OETR_ERR_BAD_ARG; n_matches > INT32_MAX, n_pairs * n_models > INT32_MAX
 * -> OETR_ERR_BAD_SHAPE. */
oetr_status oetr_homography_ransac(const double *params, const int32_t *offsets, const int32_t *pair_ids, int n_pairs,
                                   const float *k1, const float *k2, int64_t n_matches, int n_hyp, uint32_t seed,
                                   double px_thr, int refit_iters, const double *models_in, int n_models_in,
                                   void *workspace, size_t workspace_bytes, double *model, double *H, double *corner_sq,
                                   int32_t *counts, uint8_t *inliers, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* OETR_HOMOGRAPHY_RANSAC_H_ */
