/* Matching two descriptor sets by nearest neighbours: an extension of liboetr_hip.so.
 *
 * oetr_assemble_matches (include/oetr_match_assembly.h) starts from a matcher's matches0.  The reference's own matcher
 * is dloc/core/matchers/nearest_neighbor.py: sim = einsum('bdn,bdm->bnm'), topk(2) per row and per column, a ratio
 * test and a distance threshold on 2 * (1 - sim), then the mutual check.  oetr_nn_match does that for ALL pairs of a
 * call, from the joined descriptors and the offsets oetr_assemble_matches takes, and never stores a similarity matrix.
 *
 * The arithmetic is the numpy program tests/nn_match_oracle.py, bit for bit:
 *   sim[i][j]   one float32 fmaf chain, acc = 0; for d = 0 .. D-1: acc = fmaf(desc0[i][d], desc1[j][d], acc) - the
 *               f32-input MFMA of gfx950 is that chain - so direction 1's similarity is the transpose, bit for bit
 *   top two     NaN and -inf are no candidates; b1 = the largest candidate, i1 = the LOWEST index that attains it (-1
 *               without a candidate), b2 = the second largest counting multiplicity (-inf with fewer than two)
 *   find_nn     float32, nothing contracted: d0 = 2 * (1 - b1), d1 = 2 * (1 - b2), mask = i1 >= 0,
 *               mask &= d0 <= ratio_sq * d1 (ratio test on), mask &= d0 <= distance_sq (distance test on),
 *               m = mask ? i1 : -1, score = mask ? (b1 + 1) / 2 : 0
 *   mutual      matches0[i] = m0[i] when m0[i] > -1 and m1[m0[i]] == i, else -1; scores0 stays direction 0's score
 *               BEFORE the mutual check, as the reference returns it
 * Two departures from the reference, both where it leaves the result open: torch's topk does not say which of two
 * tied maxima it returns (here: the lowest index), and its topk(2) raises for a side of one row (here b2 = -inf, so
 * the ratio test passes).
 *
 * This header extends include/oetr_hip.h (same library, same status codes, same oetr_last_error) and carries a
 * version of its own; OETR_ABI_VERSION and the versions of the other extensions do not change. */
#ifndef OETR_NN_MATCH_H_
#define OETR_NN_MATCH_H_

#include "oetr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OETR_NN_MATCH_ABI_VERSION 1
/* counters per pair: K0, K1, rows of side 0 that pass find_nn, rows of side 0 matched after the mutual check (equal
 * to the third when the mutual check is off) */
#define OETR_NN_MATCH_COUNTERS 4
/* the flag word */
#define OETR_NN_MATCH_RATIO 1u    /* the ratio test is on: ratio_sq is read */
#define OETR_NN_MATCH_DISTANCE 2u /* the distance test is on: distance_sq is read */
#define OETR_NN_MATCH_MUTUAL 4u   /* the mutual check is on */
#define OETR_NN_MATCH_MIN_D 4
#define OETR_NN_MATCH_MAX_D 512

int oetr_nn_match_abi_version(void);

/* Bytes of device scratch a call with n_kp1 rows on side 1 needs when it is given no matches1 output (direction 1's
 * matches live there).  0 for n_kp1 < 1.  No GPU needed. */
size_t oetr_nn_match_workspace_bytes(int64_t n_kp1);

/* n_pairs pairs, their descriptors concatenated per side: side i of pair p owns rows off_i[p] .. off_i[p+1]-1.
 *
 *   desc0, desc1   device float32 [n_kp0][D], [n_kp1][D], keypoint-major, 16-byte aligned; D % 4 == 0, 4 <= D <= 512
 *   off0, off1     device int32 [n_pairs+1], non-decreasing: what oetr_assemble_matches takes
 *   max_k0, max_k1 the largest per-pair row counts the caller vouches for (they size the grid).  A pair whose clamped
 *                  count exceeds one of them is never dereferenced: its counters read four -1, its rows -1 / 0
 *   ratio_sq       float32(ratio_threshold^2), read when flags has OETR_NN_MATCH_RATIO
 *   distance_sq    float32(distance_threshold^2), read when flags has OETR_NN_MATCH_DISTANCE
 *   workspace      device scratch of oetr_nn_match_workspace_bytes(n_kp1) bytes; may be NULL when matches1 is given or
 *                  n_kp1 == 0
 *
 * Outputs (device):
 *   matches0  int32 [n_kp0]    row a of pair p: an index WITHIN side 1 of pair p, or -1 - what oetr_assemble_matches
 *                              reads as `matches` with match_bytes 4
 *   scores0   float32 [n_kp0]  matching_scores0
 *   matches1  int32 [n_kp1] or NULL   direction 1 after find_nn, before any mutual check
 *   counts    int32 [n_pairs][4]
 * Rows that no pair owns are written -1 / 0 by every call.
 *
 * Three launches whatever the sizes are: one that writes -1 / 0 to every row; the top-two launch, in which a workgroup
 * owns one pair, one direction and 64 query rows, walks the other side in tiles of 128 rows, contracts over D with
 * v_mfma_f32_32x32x2_f32 (every (i, j) accumulator is ONE chain over ascending d: no split over D) and keeps each
 * query's running top two in registers under the order (value descending, index ascending); and one workgroup per pair
 * for the mutual check and the counters.  Pairs ride on the x dimension of the grid only.  No floating-point atomics,
 * no order that depends on scheduling, no workgroup waits on another: two calls give the same bits.
 *
 * Memory safety does not depend on device data: off_i[p] is clamped into [0, n_kp_i] and off_i[p+1] into
 * [that, n_kp_i] before use, and a match index passes one unsigned compare against K1 before an address is formed
 * from it.  Offsets that are not non-decreasing give UNSPECIFIED results, never an access out of bounds.
 *
 * The call only enqueues on `stream`: it reads nothing back, allocates nothing, borrows every pointer, and can be
 * captured into a HIP graph.  n_kp0 == 0 and n_kp1 == 0 are legal (the pointers to rows may then be NULL), and so are
 * pairs with K = 0.
 *
 * Checked on the host before anything is enqueued: NULL off0 / off1 / counts, NULL desc0 / matches0 / scores0 unless
 * n_kp0 == 0, NULL desc1 unless n_kp1 == 0, NULL workspace without matches1 unless n_kp1 == 0, n_pairs <= 0,
 * n_kp0 < 0, n_kp1 < 0, max_k0 < 0, max_k1 < 0, D outside [4, 512] or not a multiple of 4, unknown flag bits,
 * desc0 / desc1 off 16 bytes, matches0 / scores0 / matches1 / counts / workspace off 4 bytes -> OETR_ERR_BAD_ARG;
 * n_kp0 or n_kp1 > INT32_MAX, n_pairs > INT32_MAX / 4, or more than INT32_MAX workgroups
 * (n_pairs * (ceil(max_k0 / 64) + ceil(max_k1 / 64)), each term at least 1) -> OETR_ERR_BAD_SHAPE; workspace_bytes
 * smaller than oetr_nn_match_workspace_bytes(n_kp1) when the workspace is used -> OETR_ERR_WORKSPACE. */
oetr_status oetr_nn_match(const float *desc0, const int32_t *off0, int64_t n_kp0, const float *desc1,
                          const int32_t *off1, int64_t n_kp1, int n_pairs, int D, int max_k0, int max_k1,
                          float ratio_sq, float distance_sq, unsigned flags, void *workspace, size_t workspace_bytes,
                          int32_t *matches0, float *scores0, int32_t *matches1, int32_t *counts, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* OETR_NN_MATCH_H_ */
