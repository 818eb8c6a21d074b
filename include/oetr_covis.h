/* Co-visibility extension of liboetr_hip.so: ground-truth overlap boxes from depth maps and poses.
 *
 * The reference scores a predicted box against the bounding box of the pixels two views see in
 * common (numpy_overlap_box, src/datasets/utils.py:140-202): every pixel of depth map 1 that has a
 * depth is un-projected, moved into camera 2 with the two poses, projected, and kept when it lands
 * inside image 2 at a depth within 0.5 of that image's depth map.  oetr_covis_boxes is that function
 * for a batch of pairs, on the device, in float64 and in the reference's order of operations.
 *
 * Two quirks of the reference are KEPT (its outputs are the parity target):
 *   - the landing pixel is trunc(u2), trunc(v2) TOWARDS ZERO (astype(int)), so -1 < u2 < 0 lands on
 *     column 0; a non-finite projection (a point on or behind the camera plane) is outside;
 *   - the depth test |Z - depth2[j, i]| < 0.5 is literal: a landing pixel WITHOUT depth (0) passes
 *     when the point is closer than 0.5 to camera 2.
 * One is DEPARTED from: the reference tests the landing column against the map's HEIGHT and the row
 * against its WIDTH (i < h, j < w), which for a non-square map indexes depth2 out of range or drops a
 * strip.  This entry tests i < W, j < H.  For square maps - all the reference's dataset emits - the
 * two are the same test, and parity with the reference is claimed for square maps only.
 *
 * This header extends include/oetr_hip.h (same library, same status codes, same oetr_last_error)
 * and carries a version of its own; OETR_ABI_VERSION does not change. */
#ifndef OETR_COVIS_H_
#define OETR_COVIS_H_

#include "oetr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OETR_COVIS_ABI_VERSION 1

/* One pair's parameter block: OETR_COVIS_PARAM_DOUBLES float64 values,
 *     [ 0..15]  T = pose2 * inverse(pose1), 4 x 4, row-major (world-to-camera poses)
 *     [16..19]  K1: fx, fy, cx, cy  (K1[0][0], K1[1][1], K1[0][2], K1[1][2])
 *     [20..28]  K2, 3 x 3, row-major (the whole matrix: the projection divides by its third row)
 *     [29..30]  bbox1  (row, col): offset of map 1's crop in the resized image
 *     [31..32]  ratio1 (row, col): resize factors of image 1
 *     [33..34]  bbox2  (row, col)
 *     [35..36]  ratio2 (row, col)
 *     [37..39]  reserved (ignored) */
#define OETR_COVIS_PARAM_DOUBLES 40
#define OETR_COVIS_MAX_SIDE 8192

int oetr_covis_abi_version(void);

/* Bytes of workspace oetr_covis_boxes needs for n_pairs pairs (0 for n_pairs <= 0).  Needs no GPU.
 * The workspace may hold anything on entry: every call initialises what it uses. */
size_t oetr_covis_workspace_bytes(int n_pairs);

/* For p in [0, n_pairs), with depth1[p] / depth2[p] float32 [H][W] (0: no depth) and params[p] as above:
 *     source pixels   (u, v) with depth1[v][u] = Z > 0
 *                     x = (u + bbox1[1] + 0.5) / ratio1[1],  X = (x - cx) * (Z / fx)   (y, Y likewise)
 *     transform       (X, Y, Z, 1) by T, divided by the fourth component -> (Xc, Yc, Zc)
 *     projection      K2 (Xc, Yc, Zc), divided by the third component;
 *                     u2 = . * ratio2[1] - bbox2[1] - 0.5,  v2 = . * ratio2[0] - bbox2[0] - 0.5
 *     landing pixel   i = trunc(u2), j = trunc(v2); inside: 0 <= i < W, 0 <= j < H
 *     inlier          inside and |Zc - depth2[j][i]| < 0.5
 *     count[p]        number of inliers (int32; may be NULL)
 *     valid[p]        count > 0 (uint8)
 *     box1[p]         (min u, min v, max u, max v) over the inliers, float32; zeros when not valid
 *     box2[p]         (min i, min j, max i, max j) over the inliers, float32; zeros when not valid
 *     mask1[p][v][u] = 1, mask2[p][j][i] = 1 for every inlier (uint8 [H][W], cleared by the call);
 *                     both NULL (no masks) or both set.
 * All pointers are device memory owned by the caller.  The call only enqueues on `stream` (kernels
 * alone: the clears are kernels too, no memset node), reads nothing back and can be captured into a HIP graph; the
 * reductions are integer atomics, so the results are bit-identical from run to run.
 *
 * Checked on the host before anything is enqueued: NULL depth / params / workspace / box / valid
 * pointers, exactly one mask pointer, n_pairs <= 0, workspace_bytes < oetr_covis_workspace_bytes(n_pairs)
 * -> OETR_ERR_BAD_ARG; H or W outside 1..OETR_COVIS_MAX_SIDE -> OETR_ERR_BAD_SHAPE. */
oetr_status oetr_covis_boxes(const float *depth1, const float *depth2, const double *params,
                             int n_pairs, int H, int W, void *workspace, size_t workspace_bytes,
                             float *box1, float *box2, uint8_t *valid, int32_t *count,
                             uint8_t *mask1, uint8_t *mask2, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* OETR_COVIS_H_ */
