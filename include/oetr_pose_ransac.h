/* Relative pose from match lists, by RANSAC on the device: an extension of liboetr_hip.so.
 *
 * The reference's evaluation reports AUC@5/10/20 of the pose error first (dloc/evaluate/eval_megadepth.py); its
 * validation_error -> estimate_pose -> compute_pose_error (dloc/evaluate/utils/evaluation.py) runs
 * cv2.findEssentialMat(RANSAC) and cv2.recoverPose per pair on the host.  oetr_pose_ransac estimates the relative
 * pose of MANY match lists in one call and delivers the two cosines of the pose error; the arccos stays with the
 * caller.
 *
 * The arithmetic is the float64 program tests/pose_ransac_oracle.py, operation by operation in the order written there
 * (no contraction into FMAs, IEEE division and square root, every decision a comparison).  It is THE PROJECT'S OWN
 * STATEMENT, not OpenCV's: a 7-point minimal solver, a fixed number of hypotheses that are all scored, no adaptive
 * termination, no local optimisation, no pose below 7 matches.  No parity with cv2 is claimed.
 *
 * Per pair, with the 20 doubles of OETR_MATCH_SCORE_PARAM_DOUBLES (fx fy cx cy of both cameras, R row major and t of
 * T_1to2) and its list of rows (u, v):
 *   normalise  x = (u - cx) / fx, y = (v - cy) / fy on both sides; thr_n = px_thr / ((fx1 + fy2) / 2) (the reference's
 *              f_mean quirk is kept);
 *   sample     hypothesis h draws 7 distinct rows with a counter-based generator of (seed, pair_id, h, draw);
 *              pair_id = pair_ids[p], or p when pair_ids is NULL; a list of fewer than 7 rows has no hypotheses;
 *   solve      the 7-point algorithm: up to 3 models per hypothesis, numbered 3 * h + root, absent ones all NaN;
 *   score      a row is an inlier of F iff s * s < thr_n^2 * ((a0^2 + a1^2) + (b0^2 + b1^2)) with a = F x1,
 *              b = F^T x2, s = x2 . a; a model with a non-finite entry scores -1;
 *   select     most inliers, the lowest model number on a tie; no finite model: no pose;
 *   decompose  (R1, +t), (R1, -t), (R2, +t), (R2, -t); the candidate with the most inlier rows of positive depth on
 *              both sides wins, the lowest number on a tie;
 *   errors     cosines[p] = { (trace(R_gt^T R) - 1) / 2, (t . t_gt) / (|t| |t_gt|) }, unclipped.
 *
 * This header extends include/oetr_hip.h (same library, same status codes, same oetr_last_error) and carries a
 * version of its own; OETR_ABI_VERSION and the versions of the other extensions do not change. */
#ifndef OETR_POSE_RANSAC_H_
#define OETR_POSE_RANSAC_H_

#include "oetr_match_score.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OETR_POSE_RANSAC_ABI_VERSION 1
#define OETR_POSE_RANSAC_MAX_HYPOTHESES 4096
#define OETR_POSE_RANSAC_MAX_MODELS 12288          /* 3 * OETR_POSE_RANSAC_MAX_HYPOTHESES */
#define OETR_POSE_RANSAC_COUNTERS 5

int oetr_pose_ransac_abi_version(void);

/* Bytes of workspace for n_pairs pairs of n_models models each (n_models = 3 * n_hyp, or n_models_in): the models
 * as float64 [n_pairs][n_models][9], then their inlier counts as int32 [n_pairs][n_models].  0 when either is <= 0. */
size_t oetr_pose_ransac_workspace_bytes(int n_pairs, int n_models);

/* n_pairs match lists, concatenated as oetr_match_score takes them and oetr_assemble_matches leaves them: list p is the
 * rows offsets[p] .. offsets[p+1]-1 of k1 / k2 (float32 (u, v) in the original pictures, widened exactly), both offsets
 * clamped into [0, n_matches].  n_matches is a HOST value that bounds every row access.  Offsets that are not
 * non-decreasing give UNSPECIFIED results, but never an access out of bounds.
 *
 * models_in NULL: n_hyp hypotheses per pair are sampled and solved (n_models = 3 * n_hyp; n_models_in is ignored).
 * models_in non-NULL (float64 [n_pairs][n_models_in][9]): sampling and solving are skipped and the caller's models are
 * scored, selected and decomposed (n_hyp and seed are ignored); the models part of the workspace is left alone.
 *
 * Outputs: model[p] the selected F, pose[p] = R (row major) then t of the chosen candidate, cosines[p], and
 * counts[p] = { the list's length, the finite models, the number of the selected model or -1, its inliers, the votes
 * of the chosen candidate }.  A pair without a pose has NaN model, pose and cosines and 0 inliers and votes.
 * inliers[m] (NULL: not stored) is 1 for the inlier rows of the selected models and 0 for every other row below
 * n_matches.
 *
 * The call only enqueues on `stream`: the solving kernel (not with models_in), the scoring kernel and the pose
 * kernel, in a line, whatever the lists hold.  It reads nothing back, allocates nothing, uses no memset node and no
 * floating-point atomics: results are bit-identical from run to run, and the call can be captured into a HIP graph.
 *
 * Memory safety rests on host values and on values tested on the device: sample indices lie below the clamped list
 * length by construction of the sampler, a model number forms an address only after the compare against n_models.
 *
 * Checked on the host before anything is enqueued: NULL params / offsets / workspace / model / pose / cosines /
 * counts, NULL k1 / k2 unless n_matches == 0, n_pairs <= 0, n_matches < 0, n_hyp outside 1..4096 (models_in NULL),
 * n_models_in outside 1..12288 (otherwise), px_thr not finite or <= 0, workspace smaller than
 * oetr_pose_ransac_workspace_bytes -> OETR_ERR_BAD_ARG; n_matches > INT32_MAX, n_pairs * n_models > INT32_MAX ->
 * OETR_ERR_BAD_SHAPE. */
oetr_status oetr_pose_ransac(const double *params, const int32_t *offsets, const int32_t *pair_ids, int n_pairs,
                             const float *k1, const float *k2, int64_t n_matches, int n_hyp, uint32_t seed,
                             double px_thr, const double *models_in, int n_models_in, void *workspace,
                             size_t workspace_bytes, double *model, double *pose, double *cosines, int32_t *counts,
                             uint8_t *inliers, void *stream);

/* A test hook: out[i] = the device's float64 square root of in[i], the one the kernels use, for 0 <= i < n. */
oetr_status oetr_pose_ransac_sqrt(const double *in, double *out, int64_t n, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* OETR_POSE_RANSAC_H_ */
