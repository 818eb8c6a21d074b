/* Assembling matcher output into origin-frame match lists: an extension of liboetr_hip.so.
 *
 * Between the batched crop step (include/oetr_crop_batch.h) and the scoring of matches (include/oetr_match_score.h)
 * stands the tail of the reference's process() (dloc/core/overlap_features.py:118-155): keypoints found in the crops
 * are mapped back into the original pictures, (keypoints / ratio + bbox[:2]) * scales, and the matcher's matches0 is
 * turned into lists, valid = matches > -1, index0 = nonzero(valid), index1 = matches[valid], mconf = conf[valid].
 * oetr_assemble_matches does both for ALL pairs of a call, reading the geometry records oetr_overlap_crop_batch left
 * on the device (oetr_crop_info, include/oetr_hip.h: the same struct, no second one), and adds the reference's
 * selection of the pairs to run again without crops (fewer than 30 matches, overlap_features.py:215).
 *
 * The arithmetic is the numpy program tests/match_assembly_oracle.py, operation by operation, with the reference's
 * dtypes: q = float32(k / float32(ratio)) (the correctly rounded float32 quotient, denormals kept),
 * t = float32(q + sbox), origin = float64(t) * scale; nothing is contracted.
 *
 * This header extends include/oetr_hip.h (same library, same status codes, same oetr_last_error) and carries a
 * version of its own; OETR_ABI_VERSION and the versions of the other extensions do not change. */
#ifndef OETR_MATCH_ASSEMBLY_H_
#define OETR_MATCH_ASSEMBLY_H_

#include "oetr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OETR_MATCH_ASSEMBLY_ABI_VERSION 1
/* counters per pair: K0 (keypoints of side 0), K1, matches kept, matches rejected */
#define OETR_MATCH_ASSEMBLY_COUNTERS 4

int oetr_match_assembly_abi_version(void);

/* Bytes of device scratch for a call of n_pairs pairs (the kept count of every pair, between the counting and the
 * scanning launch).  0 for n_pairs < 1.  No GPU needed. */
size_t oetr_match_assembly_workspace_bytes(int n_pairs);

/* n_pairs pairs, their keypoints concatenated per side: side i of pair p owns rows off_i[p] .. off_i[p+1]-1 of kp_i.
 *
 *   info      device [n_pairs]          the pairs' geometry records; read: valid, ratio[i][0..1], sbox[i][0..1]
 *   scales    device float64 [n_pairs][2][2]   the reader's scales0 / scales1 (sx, sy) of each pair
 *   kp0, kp1  device float32 [n_kp0][2], [n_kp1][2]   keypoints in CROP coordinates
 *   off0, off1  device int32 [n_pairs+1]   non-decreasing row offsets
 *   matches   device [n_kp0], int32 (match_bytes 4) or int64 (match_bytes 8): the matcher's matches0, aligned with
 *             kp0.  Row a of pair p holds b, an index WITHIN side 1 of pair p, or a negative value for no match
 *   conf      device float32 [n_kp0] (matching_scores0) or NULL; mconf must be NULL exactly when conf is
 *   min_matches   the selection's bound (>= 0); few / n_few both NULL switch the selection off
 *
 * Alignment: rows move as whole vectors, so kp0, kp1, k1 and k2 must be 8-byte aligned, origin0 and origin1 16-byte
 * aligned and matches aligned to match_bytes (any fresh device allocation is; a view that starts at an odd float is
 * not).
 *
 * Outputs (device):
 *   origin0 float64 [n_kp0][2], origin1 float64 [n_kp1][2]   every keypoint in its original picture.  A row that no
 *             pair owns (before off_i[0], from off_i[n_pairs] on) and a row of a pair with valid == -1 reads NaN
 *   index0, index1 int32 [n_kp0]; k1, k2 float32 [n_kp0][2]; mconf float32 [n_kp0]
 *             the lists, pair after pair, in each pair in ascending a: every a with 0 <= matches[a] < K1_p gives
 *             index0 = a, index1 = b = matches[a], k1 = float32(origin0[off0[p]+a]), k2 = float32(origin1[off1[p]+b])
 *             (round to nearest even), mconf = conf[off0[p]+a].  Duplicated b are kept.  n_kp0 rows are the upper
 *             bound; rows from offsets[n_pairs] on are WRITTEN by every call: -1 in index0 / index1, NaN elsewhere
 *   offsets   int32 [n_pairs+1]   list p is the rows offsets[p] .. offsets[p+1]-1; offsets[n_pairs] is the total
 *   counts    int32 [n_pairs][4]  K0, K1, kept, rejected.  Rejected: matches[a] >= K1_p (for int64 this includes every
 *             positive value beyond int32); such a match is dropped and kp1 is never dereferenced with it.  A negative
 *             value of any size is "no match", as in the reference's matches > -1.  A pair with valid == -1 (no crops
 *             were made) gives an empty list and four -1
 *   few       int32 [n_pairs], n_few int32 [1]   the numbers of the pairs with kept < min_matches or valid == -1, in
 *             list order; few[n_few ..] reads -1
 *
 * Three launches whatever n_pairs and the keypoint counts are: a count per pair, one workgroup that scans the counts
 * into offsets and compacts few, and the emitting launch (one workgroup per pair walks its rows in order).  The order
 * of every output is decided by arithmetic: two calls give the same bits.  No workgroup waits on another.
 *
 * Memory safety does not depend on device data: off_i[p] is clamped into [0, n_kp_i] and off_i[p+1] into
 * [that, n_kp_i] before use, K1_p is the clamped length, a match index is tested with one unsigned compare against
 * K1_p before any address is formed from it, and a list row is written only below n_kp0.  Offsets that are not
 * non-decreasing give UNSPECIFIED results, but never a read or a write out of bounds.
 *
 * The call only enqueues on `stream`: it reads nothing back, allocates nothing, borrows every pointer, and can be
 * captured into a HIP graph (a replay sees what the buffers hold at replay time).  n_kp0 == 0 and n_kp1 == 0 are
 * legal (the pointers to rows may then be NULL).
 *
 * Checked on the host before anything is enqueued: NULL info / scales / off0 / off1 / offsets / counts / workspace,
 * NULL kp0 / matches / origin0 / index0 / index1 / k1 / k2 unless n_kp0 == 0, NULL kp1 / origin1 unless n_kp1 == 0,
 * conf without mconf or mconf without conf, few without n_few or n_few without few, n_pairs <= 0, n_kp0 < 0,
 * n_kp1 < 0, min_matches < 0, match_bytes other than 4 or 8, a pointer that misses the alignment above
 * -> OETR_ERR_BAD_ARG; n_kp0 or n_kp1 > INT32_MAX (the offsets are int32) or n_pairs > INT32_MAX / 4
 * -> OETR_ERR_BAD_SHAPE; workspace_bytes smaller than
 * oetr_match_assembly_workspace_bytes(n_pairs) -> OETR_ERR_WORKSPACE. */
oetr_status oetr_assemble_matches(const oetr_crop_info *info, const double *scales, int n_pairs, const float *kp0,
                                  const int32_t *off0, int64_t n_kp0, const float *kp1, const int32_t *off1,
                                  int64_t n_kp1, const void *matches, int match_bytes, const float *conf,
                                  int min_matches, void *workspace, size_t workspace_bytes, double *origin0,
                                  double *origin1, int32_t *index0, int32_t *index1, float *k1, float *k2,
                                  float *mconf, int32_t *offsets, int32_t *counts, int32_t *few, int32_t *n_few,
                                  void *stream);

#ifdef __cplusplus
}
#endif
#endif /* OETR_MATCH_ASSEMBLY_H_ */
