/* Keypoints selected and descriptors sampled from an extractor network's dense maps: an extension of liboetr_hip.so.
 *
 * oetr_nn_match (include/oetr_nn_match.h) and oetr_assemble_matches (include/oetr_match_assembly.h) start from
 * keypoints, scores and descriptors.  An extractor network delivers a dense score map and a dense descriptor map per
 * image; the head behind it - non-maximum suppression, a threshold, a border, the best max_keypoints, descriptors
 * sampled at the keypoints and normalised - is oetr_keypoint_select, for ALL images of a call (mixed sizes) in a fixed
 * number of launches.  Its outputs are the joined keypoints / scores / descriptors / offsets the two entries above take.
 *
 * The statement is this project's own, modelled on SuperPoint's published post-processing (simple_nms, remove_borders,
 * top_k_keypoints, sample_descriptors); it is the numpy program tests/keypoint_select_oracle.py, bit for bit:
 *   loading      a NaN score is loaded as -inf
 *   pool(X)      the maximum over the (2r+1)^2 window, positions outside the map not counted
 *   NMS          M = (S == pool(S)); twice: supp = pool(M) > 0, S' = supp ? 0 : S, M |= (S' == pool(S')) & !supp;
 *                N = M ? S : 0
 *   candidates   N > threshold, border <= y < H - border, border <= x < W - border
 *   selection    at most max_keypoints candidates: all, in raster order (y * W + x ascending); more: the
 *                max_keypoints best in descending score order, a tie to the LOWER raster index
 *   keypoint     (x, y) as float32
 *   descriptor   float32, every product and sum rounded on its own, division and sqrt correctly rounded:
 *                t = (x - cell/2) + 0.5; g = (t / float(w*cell - cell/2 - 0.5)) * 2 - 1; ix = ((g + 1) / 2) * (w - 1)
 *                (iy likewise with h); x0 = floor(ix), x1 = x0 + 1, wx1 = ix - x0, wx0 = x1 - ix (y likewise); a tap
 *                is inside when 0 <= its x <= w-1 and 0 <= its y <= h-1 (so a NaN coordinate has no tap); term =
 *                inside ? F[d][y][x] * (wx * wy) : 0 for nw, ne, sw, se; v[d] = ((nw + ne) + sw) + se;
 *                ss: 64 partial sums, partial j over the channels d = j (mod 64) ascending of v[d] * v[d], then
 *                p[j] += p[j + stride] for stride 32, 16, 8, 4, 2, 1; n = sqrt(ss), n = n < 1e-12 ? 1e-12 : n;
 *                out[d] = v[d] / n
 *
 * This header extends include/oetr_hip.h (same library, same status codes, same oetr_last_error) and carries a
 * version of its own; OETR_ABI_VERSION and the versions of the other extensions do not change. */
#ifndef OETR_KEYPOINT_SELECT_H_
#define OETR_KEYPOINT_SELECT_H_

#include "oetr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OETR_KEYPOINT_SELECT_ABI_VERSION 1
/* counters per map: candidates, kept; two -1 for a map whose record is unusable (below) */
#define OETR_KEYPOINT_SELECT_COUNTERS 2
#define OETR_KEYPOINT_SELECT_MAX_RADIUS 8
#define OETR_KEYPOINT_SELECT_MAX_KEYPOINTS 4096
#define OETR_KEYPOINT_SELECT_MIN_D 4
#define OETR_KEYPOINT_SELECT_MAX_D 512
#define OETR_KEYPOINT_SELECT_MAX_SIDE 8192
/* a map's first pixel in the workspace planes is a multiple of this */
#define OETR_KEYPOINT_SELECT_PIXEL_ALIGN 64

/* One record per image of the device table.  Strides count ELEMENTS (floats), so an NCHW and a channels-last
 * descriptor map both go in without a copy; the score map's x stride is 1. */
typedef struct oetr_keypoint_map {
  const float *scores;      /* device [H][W], row y at scores + y * score_stride */
  int32_t H, W;             /* 1 <= H, W <= OETR_KEYPOINT_SELECT_MAX_SIDE */
  int64_t score_stride;
  const float *desc;        /* device, element (d, y, x) at desc + d * desc_stride[0] + y * desc_stride[1] + x * desc_stride[2] */
  int32_t h, w;             /* 1 <= h, w <= OETR_KEYPOINT_SELECT_MAX_SIDE */
  int64_t desc_stride[3];
  int64_t pixel_offset;     /* of the map's H * W pixels in the workspace planes: a multiple of
                               OETR_KEYPOINT_SELECT_PIXEL_ALIGN, the ranges of two maps disjoint, all below total_pixels */
} oetr_keypoint_map;

int oetr_keypoint_select_abi_version(void);

/* Bytes of device scratch for a call whose maps' pixel ranges end below total_pixels, with n_maps maps and
 * max_keypoints kept at most.  0 for arguments the call would refuse.  No GPU needed. */
size_t oetr_keypoint_select_workspace_bytes(int64_t total_pixels, int n_maps, int max_keypoints);

/*   maps            device oetr_keypoint_map[n_maps]
 *   max_pixels      the largest H * W the caller vouches for (it sizes the grids)
 *   total_pixels    the end of the last map's pixel range in the workspace planes
 *   D               descriptor channels of every map: D % 4 == 0, 4 <= D <= 512
 *   nms_radius      0 .. 8;  threshold >= 0;  remove_borders >= 0;  1 <= max_keypoints <= 4096;  cell >= 1
 *
 * Outputs (device), n_maps * max_keypoints rows of capacity:
 *   keypoints    float32 [rows][2]   (x, y), 8-byte aligned
 *   scores       float32 [rows]
 *   descriptors  float32 [rows][D]
 *   offsets      int32 [n_maps+1]    map b owns rows offsets[b] .. offsets[b+1]-1
 *   counts       int32 [n_maps][2]   candidates, kept
 * Rows from offsets[n_maps] on are written -1 (keypoints) / NaN (scores) / 0 (descriptors) by every call.
 *
 * Thirteen launches whatever the sizes are: ten elementwise passes of the NMS (the maximum is separable: rows, then
 * columns; byte masks and one float plane in the workspace), one workgroup per map that compacts the candidates in
 * raster order (ballot / popcount prefix), finds the cut by a radix select and sorts at most 4096 64-bit keys, one
 * workgroup that scans the kept counts into offsets, and one wave per kept keypoint that samples and normalises.  Maps
 * ride on the x dimension of the grids only.  No atomic decides an order, no workgroup waits on another: two calls
 * give the same bits.
 *
 * A record whose H, W, h or w lies outside [1, 8192], whose H * W exceeds max_pixels, or whose pixel range is
 * misaligned or does not end below total_pixels is never dereferenced: the map keeps nothing and its counters read
 * two -1.  The pointers and strides of a usable record are the caller's responsibility.
 *
 * The call only enqueues on `stream`: it reads nothing back, allocates nothing, borrows every pointer, and can be
 * captured into a HIP graph.
 *
 * Checked on the host before anything is enqueued: NULL maps / workspace / keypoints / scores / descriptors / offsets /
 * counts, n_maps <= 0, max_pixels < 1, total_pixels < 1, D outside [4, 512] or not a multiple of 4, nms_radius outside
 * [0, 8], a threshold that is negative or NaN, remove_borders < 0, max_keypoints outside [1, 4096], cell < 1, maps off
 * 8 bytes, keypoints off 8 bytes, scores / descriptors / offsets / counts / workspace off 4 bytes -> OETR_ERR_BAD_ARG;
 * max_pixels > 8192 * 8192, total_pixels > 2^40, n_maps * max_keypoints > INT32_MAX -> OETR_ERR_BAD_SHAPE;
 * workspace_bytes smaller than oetr_keypoint_select_workspace_bytes(...) -> OETR_ERR_WORKSPACE. */
oetr_status oetr_keypoint_select(const oetr_keypoint_map *maps, int n_maps, int64_t max_pixels, int64_t total_pixels,
                                 int D, int nms_radius, float threshold, int remove_borders, int max_keypoints,
                                 int cell, void *workspace, size_t workspace_bytes, float *keypoints, float *scores,
                                 float *descriptors, int32_t *offsets, int32_t *counts, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* OETR_KEYPOINT_SELECT_H_ */
