/* Refining dense matches to sub-pixel: the two device stages that bracket the fine network of a detector-free
 * matcher.  An extension of liboetr_hip.so.
 *
 * oetr_dual_softmax_match (include/oetr_dual_softmax.h) leaves every dense match on a cell corner of the 1/8-resolution
 * grid.  The matcher the reference calls in its `direct` branch (dloc/core/matchers/loftr.py) returns the FINE-level
 * result: per coarse match a W x W window of 1/2-resolution features around both cells, a small network on the
 * windows, the correlation of window 0's centre feature with window 1, a softmax over the W * W positions, its
 * spatial expectation and the expectation's standard deviation.  oetr_fine_windows builds the match list and gathers
 * the windows from the matcher's output as it lies on the device - no unfold of the whole fine maps, no nonzero, no
 * read-back; oetr_fine_refine is the expectation head.  The network between them stays torch.  A fused kernel that
 * skips the window buffers is NOT built.
 *
 * The arithmetic of the head is THE PROJECT'S OWN STATEMENT, modelled on LoFTR's published fine matching; that code
 * lives in a third_party/ tree outside the reference checkout, so no parity with it is claimed.  It is the numpy
 * program tests/fine_match_oracle.py, bit for bit (csrc/fine_match_math.h is its one C++ copy).  Per match m, with
 * WW = W * W, float32, every operation rounded on its own except where fmaf is written:
 *   s[r]     the dot product of win0[m][WW / 2][:] with win1[m][r][:] in a STATED order: OETR_FINE_MATCH_PARTIALS = 16
 *            partial sums, channel c belongs to partial (c / 4) % 16, each partial is an fmaf chain over its channels
 *            in ascending c from +0; then the fixed tree of adjacent pairs ((p0 + p1) + (p2 + p3)) + ...
 *   t[r]     s[r] * float32(1 / sqrt(C)), one rounding.  A non-finite t (NaN, +inf, -inf) is no candidate: it enters
 *            no maximum and no sum, and its heat is +0
 *   m_       the maximum of the candidates;  q[r] = e(t[r] - m_) with the e(x) of oetr_dual_softmax.h
 *   Z        the sum of q in ascending r from +0;  heat[r] = q[r] / Z
 *   G[k]     float32((2 k - (W - 1)) / (W - 1)), the tables below; gx[r] = G[r % W], gy[r] = G[r / W]
 *   x        acc = +0; for r ascending: acc = fmaf(heat[r], gx[r], acc).  y with gy; xx, yy with the ROUNDED squares
 *            float32(G[k] * G[k])
 *   var_x    xx - x * x: the product rounded, the difference rounded;  var_y likewise
 *   std      sqrt(max(var_x, 1e-10f)) + sqrt(max(var_y, 1e-10f)), the square roots correctly rounded
 *   without a candidate: x = y = 0, std = NaN, and the pair's third counter counts the match
 *   radius   float32((W / 2) * fine_cell);  mkpts1 = keypoints1[j] + (x, y) * radius: the product rounded, the sum
 *            rounded;  mkpts0 = keypoints0[a]
 *
 * This header extends include/oetr_hip.h (same library, same status codes, same oetr_last_error) and carries a
 * version of its own; OETR_ABI_VERSION and the versions of the other extensions do not change. */
#ifndef OETR_FINE_MATCH_H_
#define OETR_FINE_MATCH_H_

#include "oetr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OETR_FINE_MATCH_ABI_VERSION 1
/* counters per pair of oetr_fine_windows: matched, kept (matched minus those dropped at the list's capacity) */
#define OETR_FINE_MATCH_WINDOW_COUNTERS 2
/* counters per pair of oetr_fine_refine: matched, kept, kept matches without a candidate */
#define OETR_FINE_MATCH_COUNTERS 3
/* partial sums of every dot product, see above */
#define OETR_FINE_MATCH_PARTIALS 16
#define OETR_FINE_MATCH_MIN_C 4
#define OETR_FINE_MATCH_MAX_C 512
#define OETR_FINE_MATCH_MAX_STRIDE 8
#define OETR_FINE_MATCH_MAX_W 7
/* G[k] = float32((2 k - (W - 1)) / (W - 1)) for W = 3, 5, 7 */
#define OETR_FINE_MATCH_G3 {-1.0f, 0.0f, 1.0f}
#define OETR_FINE_MATCH_G5 {-1.0f, -0.5f, 0.0f, 0.5f, 1.0f}
#define OETR_FINE_MATCH_G7 {-1.0f, -0.666666686534881591796875f, -0.3333333432674407958984375f, 0.0f, \
                            0.3333333432674407958984375f, 0.666666686534881591796875f, 1.0f}

int oetr_fine_match_abi_version(void);

/* Bytes of device scratch oetr_fine_windows needs for n_pairs pairs (one int32 per pair).  n_pairs < 1 reads as 0.
 * No GPU needed. */
size_t oetr_fine_match_workspace_bytes(int n_pairs);

/* The match list of a dual-softmax result and the fine windows of its matches.
 *
 * The coarse side, as oetr_dual_softmax_match leaves it:
 *   matches0       device int32 [n_tok0]: token a of pair p -> an index within side 1 of pair p, or anything else
 *   off0, off1     device int32 [n_pairs+1]; grids0, grids1 device int32 [n_pairs][2] = (h, w);  max_k0
 * The fine side:
 *   fine0, fine1   device float32 [n_fine0][C], [n_fine1][C]: the fine maps as joined token rows in raster order,
 *                  16-byte aligned; C % 4 == 0, 4 <= C <= 512
 *   foff0, foff1   device int32 [n_pairs+1];  fgrids0, fgrids1 device int32 [n_pairs][2] = (hf, wf)
 *   W              3, 5 or 7;  stride 1 .. 8: the fine cells per coarse cell
 *   max_matches    >= 0: the capacity M_cap of the list; max_matches * W * W <= INT32_MAX
 *   workspace      device scratch of oetr_fine_match_workspace_bytes(n_pairs) bytes, 4-byte aligned
 *
 * A pair is VOUCHED FOR when on both sides its coarse grid multiplies to its coarse rows and its fine grid to its fine
 * rows (no entry negative) and its side-0 rows are at most max_k0.  Any other pair is never dereferenced and its
 * counters read -1.  The fine grid need not be stride times the coarse one: what lies outside it reads as zero.
 *
 * The list: every side-0 token a of a vouched pair with 0 <= matches0[a] < S_p, pair after pair, ascending a.  A match
 * whose list position is >= M_cap is dropped and counted.
 *
 * Outputs (device):
 *   rows      int32 [M_cap][3] = (pair, index within side 0, index within side 1)
 *   moffsets  int32 [n_pairs+1]: pair p owns list rows moffsets[p] .. moffsets[p+1]-1
 *   counts    int32 [n_pairs][2] = matched, kept
 *   win0, win1  float32 [M_cap][W*W][C]: element r = ky * W + kx of a token at coarse (row, col) is fine token
 *             (row * stride + ky - W / 2, col * stride + kx - W / 2) of its own side's fine map, +0 outside that map:
 *             unfold(kernel W, stride, padding W / 2)
 * Every row of rows, win0 and win1 is written exactly once by every call; rows from moffsets[n_pairs] on read -1 / +0.
 *
 * Four launches whatever the sizes are, ordered by the launch boundary alone: one workgroup per pair counts its
 * matches; ONE workgroup scans the counts into moffsets; one workgroup per pair walks its side-0 rows in order and
 * places each match by arithmetic (the 64-bit ballot, a popcount prefix, wave totals, a running base); and the window
 * copy, a grid-stride loop over the M_cap list rows in which 16, 32 or 64 lanes own a window row and move it with
 * 16-byte loads and stores (it also writes the -1 / +0 rows past the list: there is no clearing launch).  No atomics,
 * no workgroup waits on another: two calls give the same bits.
 *
 * Memory safety does not depend on device data: offsets are clamped as in oetr_dual_softmax_match, a match index and
 * every entry of a list row pass one unsigned compare before an address is formed from them.
 *
 * The call only enqueues on `stream`: it reads nothing back, allocates nothing, borrows every pointer, and can be
 * captured into a HIP graph.
 *
 * Checked on the host before anything is enqueued: NULL off0 / off1 / grids0 / grids1 / foff0 / foff1 / fgrids0 /
 * fgrids1 / moffsets / counts / workspace, NULL matches0 unless n_tok0 == 0, NULL fine0 / fine1 unless that side has
 * no fine rows, NULL rows / win0 / win1 unless max_matches == 0, n_pairs <= 0, a negative row count, max_k0 < 0,
 * max_matches < 0, W not in {3, 5, 7}, stride outside [1, 8], C outside [4, 512] or not a multiple of 4, fine0 / fine1
 * / win0 / win1 off 16 bytes, the other pointers off 4 bytes -> OETR_ERR_BAD_ARG; a row count > INT32_MAX,
 * n_pairs > INT32_MAX / 3, max_matches > INT32_MAX / (W * W) -> OETR_ERR_BAD_SHAPE; workspace_bytes too small ->
 * OETR_ERR_WORKSPACE. */
oetr_status oetr_fine_windows(const int32_t *matches0, const int32_t *off0, const int32_t *off1, const int32_t *grids0,
                              const int32_t *grids1, int64_t n_tok0, int64_t n_tok1, int n_pairs, int max_k0,
                              const float *fine0, const int32_t *foff0, const int32_t *fgrids0, int64_t n_fine0,
                              const float *fine1, const int32_t *foff1, const int32_t *fgrids1, int64_t n_fine1, int C,
                              int W, int stride, int64_t max_matches, void *workspace, size_t workspace_bytes,
                              int32_t *rows, int32_t *moffsets, int32_t *counts, float *win0, float *win1,
                              void *stream);

/* The expectation head on the windows of a match list (the arithmetic above).
 *
 *   win0, win1     device float32 [max_matches][W*W][C], 16-byte aligned: oetr_fine_windows' windows, or whatever a
 *                  network made of them
 *   rows, moffsets, wcounts   oetr_fine_windows' list, its offsets and its counters [n_pairs][2]
 *   keypoints0, keypoints1    device float32 [n_tok0][2], [n_tok1][2], 8-byte aligned, with off0 / off1 [n_pairs+1]
 *   fine_cell      finite and > 0: the pixels per fine token
 *
 * Outputs (device):
 *   expec          float32 [max_matches][3] = (x, y, std), x and y in [-1, 1]
 *   mkpts0, mkpts1 float32 [max_matches][2]
 *   keypoints1_f   float32 [n_tok1][2]: a copy of keypoints1 with the refined position at every matched token
 *   counts         int32 [n_pairs][3] = matched, kept, kept matches without a candidate; three -1 where wcounts does
 * Rows past the list read NaN.  A list row whose entries are out of range (it cannot come from oetr_fine_windows)
 * reads NaN and touches nothing else.  Two matches onto one side-1 token cannot come from oetr_dual_softmax_match; if
 * they are given, that token's refined position is that of one of them, unspecified which.
 *
 * Three launches: the copy of keypoints1; the head, a grid-stride loop of one workgroup per list row in which 16 lanes
 * own a window row (16-byte loads, four shuffle levels) and one wave does the softmax and the expectation; one
 * workgroup per pair for the counters.  Only enqueues; reads nothing back; allocates nothing; can be captured.
 *
 * Checked on the host: NULL moffsets / wcounts / off0 / off1 / counts, NULL rows / win0 / win1 / expec / mkpts0 /
 * mkpts1 unless max_matches == 0, NULL keypoints0 unless n_tok0 == 0, NULL keypoints1 / keypoints1_f unless
 * n_tok1 == 0, n_pairs <= 0, a negative row count, max_matches < 0, W, C as above, fine_cell not finite or <= 0,
 * win0 / win1 off 16 bytes, the keypoint rows off 8 bytes, the other pointers off 4 bytes -> OETR_ERR_BAD_ARG; the
 * same limits -> OETR_ERR_BAD_SHAPE. */
oetr_status oetr_fine_refine(const float *win0, const float *win1, const int32_t *rows, const int32_t *moffsets,
                             const int32_t *wcounts, int n_pairs, int64_t max_matches, const float *keypoints0,
                             const int32_t *off0, int64_t n_tok0, const float *keypoints1, const int32_t *off1,
                             int64_t n_tok1, int C, int W, float fine_cell, float *expec, float *mkpts0, float *mkpts1,
                             float *keypoints1_f, int32_t *counts, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* OETR_FINE_MATCH_H_ */
