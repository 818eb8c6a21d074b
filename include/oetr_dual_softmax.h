/* Matching two dense feature grids by a dual softmax: an extension of liboetr_hip.so.
 *
 * The coarse matching head of a detector-free matcher (the reference's `direct` branch, dloc/core/matchers/loftr.py)
 * works on two 1/8-resolution feature grids: a similarity matrix, a softmax along both axes, a threshold, border
 * removal and the mutual-maximum test.  oetr_dual_softmax_match does that for ALL pairs of a call, from the joined
 * token rows and the offsets oetr_assemble_matches takes, and never stores a similarity or confidence matrix.
 *
 * The arithmetic is THE PROJECT'S OWN STATEMENT, modelled on LoFTR's published coarse matching; that code lives in a
 * third_party/ tree outside the reference checkout, so no parity with it is claimed.  It is the numpy program
 * tests/dual_softmax_oracle.py, bit for bit (csrc/dual_softmax_math.h is its one C++ copy):
 *   s[i][j]     one float32 fmaf chain, acc = 0; for d = 0 .. D-1: acc = fmaf(feat0[i][d], feat1[j][d], acc) - what the
 *               f32-input MFMA of gfx950 computes - so direction 1's similarity is the transpose, bit for bit
 *   t[i][j]     s[i][j] * scale, one rounding; scale is ONE float32, float32(1 / (D * temperature)).  A non-finite t
 *               (NaN, +inf, -inf) is no candidate: it enters no maximum and no sum and is nobody's match
 *   e(x)        for x <= 0: 0 where x < -87 (so e never returns a subnormal); else n = rint(x * float32(1 / ln 2)),
 *               r = fmaf(n, -ln2_lo, fmaf(n, -0.693359375, x)), p = the degree-7 polynomial of dual_softmax_math.h by
 *               Horner in seven fmaf, and n added to p's exponent field by integer arithmetic.  e(0) = 1 exactly
 *   m[i], Z[i]  m = the maximum of the row's candidates (exact, order-free); Z = the sum of e(t - m) over them in the
 *               STATED order: OETR_DUAL_SOFTMAX_PARTIALS = 8 partial sums by position - column j belongs to partial
 *               4 * ((j / 64) % 2) + 2 * ((j / 4) % 2) + (j / 32) % 2, each partial adds its columns in ascending j
 *               from +0 - then the tree ((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7)).  c[j], Y[j]: the same
 *               down column j (the row statistics of direction 1)
 *   conf[i][j]  (e(t - m[i]) / Z[i]) * (e(t - c[j]) / Y[j]): two divisions and one product, each rounded.  A factor
 *               below 2^-62 makes the element NO CANDIDATE, so no product is ever subnormal (a subnormal quotient is
 *               below 2^-62 whether or not the hardware flushes it)
 *   decision    j*(i) = the LOWEST index that attains the maximum confidence among row i's candidates, or -1 without
 *               one; i*(j) likewise.  matches0[i] = j* when conf[i][j*] > threshold, i*(j*) == i, token i lies in
 *               [border_rm, h0 - border_rm) x [border_rm, w0 - border_rm) of its grid and j* does in its own; else -1
 *
 * This header extends include/oetr_hip.h (same library, same status codes, same oetr_last_error) and carries a
 * version of its own; OETR_ABI_VERSION and the versions of the other extensions do not change. */
#ifndef OETR_DUAL_SOFTMAX_H_
#define OETR_DUAL_SOFTMAX_H_

#include "oetr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OETR_DUAL_SOFTMAX_ABI_VERSION 1
/* counters per pair: L (rows of side 0), S (rows of side 1), rows whose maximum confidence is over the threshold with
 * both tokens off the border, rows matched (the mutual test too) */
#define OETR_DUAL_SOFTMAX_COUNTERS 4
/* partial sums of every row and column sum, see above */
#define OETR_DUAL_SOFTMAX_PARTIALS 8
#define OETR_DUAL_SOFTMAX_MIN_D 4
#define OETR_DUAL_SOFTMAX_MAX_D 512

int oetr_dual_softmax_abi_version(void);

/* Bytes of device scratch a call with n_tok0 / n_tok1 rows needs: two floats (maximum, sum) per token of either side,
 * and direction 1's matches when the call is given no matches1 output.  Negative counts read as 0.  No GPU needed. */
size_t oetr_dual_softmax_workspace_bytes(int64_t n_tok0, int64_t n_tok1);

/* n_pairs pairs, their token rows concatenated per side: side i of pair p owns rows off_i[p] .. off_i[p+1]-1, the
 * tokens of an h x w grid in raster order.
 *
 *   feat0, feat1   device float32 [n_tok0][D], [n_tok1][D], token-major, 16-byte aligned; D % 4 == 0, 4 <= D <= 512
 *   off0, off1     device int32 [n_pairs+1], non-decreasing: what oetr_assemble_matches takes
 *   grids0, grids1 device int32 [n_pairs][2] = (h, w).  A pair with h < 0, w < 0 or h * w != its row count on either
 *                  side is never dereferenced: its counters read four -1, its rows -1 / 0 / NaN
 *   max_k0, max_k1 the largest per-pair row counts the caller vouches for (they size the grid); a pair beyond one of
 *                  them is treated likewise
 *   scale          float32(1 / (D * temperature)), finite and > 0
 *   threshold      finite and >= 0
 *   border_rm      >= 0; a grid narrower than 2 * border_rm + 1 matches nothing
 *   cell           >= 1: the pixels per token of the keypoints
 *   workspace      device scratch of oetr_dual_softmax_workspace_bytes(n_tok0, n_tok1) bytes, 8-byte aligned
 *
 * Outputs (device):
 *   matches0   int32 [n_tok0]      row a of pair p: an index WITHIN side 1 of pair p, or -1
 *   scores0    float32 [n_tok0]    the row's maximum confidence BEFORE the tests, 0 without a candidate
 *   matches1   int32 [n_tok1] or NULL   direction 1's argmax before the tests
 *   keypoints0, keypoints1  float32 [n_tok][2] = (col * cell, row * cell) of every token
 *   counts     int32 [n_pairs][4]
 * Rows that no pair owns are written -1 / 0 / NaN by every call.
 *
 * Five launches whatever the sizes are: one that writes -1 / 0 / NaN to every row; three sweeps, in each of which a
 * workgroup owns one pair, one direction and 64 query rows, walks the other side in tiles of 128 rows in ascending
 * order and contracts over D with v_mfma_f32_32x32x2_f32 (every (i, j) accumulator is ONE chain over ascending d) - the
 * first keeps each query's maximum and writes its keypoint, the second its sum, the third, reading the other side's
 * maxima and sums from the workspace, the maximum confidence and the lowest index that attains it; and one workgroup
 * per pair for the tests and the counters.  The sweeps are ordered by the launch boundary alone.  Pairs ride on the x
 * dimension of the grid only.  No floating-point atomics, no order that depends on scheduling, no workgroup waits on
 * another: two calls give the same bits.
 *
 * Memory safety does not depend on device data: off_i[p] is clamped into [0, n_tok_i] and off_i[p+1] into
 * [that, n_tok_i] before use, and a match index passes one unsigned compare against S before an address is formed
 * from it.  Offsets that are not non-decreasing give UNSPECIFIED results, never an access out of bounds.
 *
 * The call only enqueues on `stream`: it reads nothing back, allocates nothing, borrows every pointer, and can be
 * captured into a HIP graph.  n_tok0 == 0 and n_tok1 == 0 are legal (the pointers to rows may then be NULL), and so
 * are pairs with no rows.
 *
 * Checked on the host before anything is enqueued: NULL off0 / off1 / grids0 / grids1 / counts, NULL feat0 / matches0
 * / scores0 / keypoints0 unless n_tok0 == 0, NULL feat1 / keypoints1 unless n_tok1 == 0, NULL workspace unless
 * n_tok0 == 0 and n_tok1 == 0, n_pairs <= 0, n_tok0 < 0, n_tok1 < 0, max_k0 < 0, max_k1 < 0, D outside [4, 512] or not
 * a multiple of 4, scale not finite or <= 0, threshold not finite or < 0, border_rm < 0, cell < 1, feat0 / feat1 off
 * 16 bytes, workspace / keypoints0 / keypoints1 off 8 bytes, the other pointers off 4 bytes -> OETR_ERR_BAD_ARG;
 * n_tok0 or n_tok1 > INT32_MAX, n_pairs > INT32_MAX / 4, or more than INT32_MAX workgroups
 * (n_pairs * (ceil(max_k0 / 64) + ceil(max_k1 / 64)), each term at least 1) -> OETR_ERR_BAD_SHAPE; workspace_bytes
 * smaller than what the call uses -> OETR_ERR_WORKSPACE. */
oetr_status oetr_dual_softmax_match(const float *feat0, const int32_t *off0, const int32_t *grids0, int64_t n_tok0,
                                    const float *feat1, const int32_t *off1, const int32_t *grids1, int64_t n_tok1,
                                    int n_pairs, int D, int max_k0, int max_k1, float scale, float threshold,
                                    int border_rm, int cell, void *workspace, size_t workspace_bytes,
                                    int32_t *matches0, float *scores0, int32_t *matches1, float *keypoints0,
                                    float *keypoints1, int32_t *counts, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* OETR_DUAL_SOFTMAX_H_ */
