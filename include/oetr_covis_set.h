/* Co-visibility boxes by index over a SET of depth maps, and pair mining: an extension of liboetr_hip.so.
 *
 * oetr_covis_boxes (include/oetr_covis.h) takes one stacked depth tensor per side, so every pair of a call
 * carries its own two maps and all maps share one shape.  The jobs the boxes are used for are pair LISTS over
 * an image SET - scoring a list of pairs, mining training pairs from a scene (the reference's
 * src/utils/megadepth_preprocess.py) - where a map serves many pairs and the maps have their native, differing
 * sizes.  oetr_covis_boxes_indexed reads the maps in place through a device table and takes the pairs as two
 * index arrays; oetr_covis_select is the reference's mining criterion on the resulting boxes.
 *
 * The per-pixel arithmetic is the ONE copy oetr_covis_boxes runs (csrc/covis.hip: covis_block), with both kept
 * quirks of the reference (truncation towards zero, the literal depth test) and the same DEPARTURE from it:
 * map 1 is H1 x W1, map 2 is H2 x W2, and the landing pixel is tested as 0 <= i < W2, 0 <= j < H2 where the
 * reference compares the column with the height and the row with the width.  For square maps of one size the
 * two are the same test, and parity with the reference is claimed for those only.
 *
 * There are NO MASKS in this entry: a mask per pair is per-pair memory of the size of a map again, which is what
 * the entry exists to avoid.  Callers that need masks stack the maps and call oetr_covis_boxes.
 *
 * This header extends include/oetr_hip.h (same library, same status codes, same oetr_last_error) and carries a
 * version of its own; OETR_ABI_VERSION and OETR_COVIS_ABI_VERSION do not change. */
#ifndef OETR_COVIS_SET_H_
#define OETR_COVIS_SET_H_

#include "oetr_covis.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OETR_COVIS_SET_ABI_VERSION 1

/* One depth map of the set: float32 [H][W] in device memory (0: no depth).  16 bytes.  The table is a DEVICE
 * array of these; the host never reads it. */
typedef struct oetr_covis_map {
  const float *depth;
  int32_t H, W;
} oetr_covis_map;

int oetr_covis_set_abi_version(void);

/* Bytes of workspace oetr_covis_boxes_indexed needs for n_pairs pairs (0 for n_pairs <= 0).  Needs no GPU.
 * The workspace may hold anything on entry: every call initialises what it uses. */
size_t oetr_covis_set_workspace_bytes(int n_pairs);

/* For p in [0, n_pairs): the results of oetr_covis_boxes for depth map maps[idx1[p]] (H1 x W1) against
 * maps[idx2[p]] (H2 x W2) under params[p] (OETR_COVIS_PARAM_DOUBLES float64, the layout of oetr_covis.h):
 * count[p] (int32, may be NULL), valid[p] (uint8), box1[p] / box2[p] (float32 [4]; zeros when not valid).
 * idx1 / idx2 are device int32 [n_pairs].  The same map may serve any number of pairs, on either side.
 *
 * max_pixels is the largest H * W the caller vouches for; it sets the grid (blocks of 2048 source pixels up to
 * max_pixels, times pairs), so it is a host value while the table is not.
 *
 * A pair is NEVER DEREFERENCED - and gets zero boxes, valid = 0, count = -1 - when for either of its sides the
 * index is outside [0, n_maps), the map's pointer is NULL, its H or W is outside 1..OETR_COVIS_MAX_SIDE, or its
 * H * W exceeds max_pixels.  The other pairs of the call are unaffected.
 *
 * The call only enqueues on `stream` (a clearing kernel and two more, one more kernel per 65535 pairs; no memset node),
 * reads nothing back, allocates nothing and can be captured into a HIP graph; a replay sees the table, the
 * indices and the parameters the buffers hold at replay time.  The reductions are integer atomics, so the
 * results are bit-identical from run to run and do not depend on the order of the list.
 *
 * Checked on the host before anything is enqueued: NULL maps / idx / params / workspace / box / valid pointers,
 * n_maps <= 0, n_pairs <= 0, workspace_bytes < oetr_covis_set_workspace_bytes(n_pairs) -> OETR_ERR_BAD_ARG;
 * max_pixels outside 1..OETR_COVIS_MAX_SIDE^2 -> OETR_ERR_BAD_SHAPE. */
oetr_status oetr_covis_boxes_indexed(const oetr_covis_map *maps, int n_maps, const int32_t *idx1,
                                     const int32_t *idx2, const double *params, int n_pairs, int64_t max_pixels,
                                     void *workspace, size_t workspace_bytes, float *box1, float *box2,
                                     uint8_t *valid, int32_t *count, void *stream);

/* The reference's mining criterion (src/utils/megadepth_preprocess.py:71-92, 199-200) on n_pairs boxes, in
 * float64.  With w1 = box1[2] - box1[0], h1 = box1[3] - box1[1] and w2, h2 likewise, and max(a, b) Python's
 * (b > a ? b : a, so a NaN first argument stays):
 *     scale_diff[p] = max(max(w1 / w2, w2 / w1), max(h1 / h2, h2 / h1))
 * A zero width or height gives inf or NaN exactly as numpy's division does.  Pair p is KEPT when
 *     valid[p] && max(box1[p]) > 0 && max(box2[p]) > 0 && scale_diff[p] > min_scale_diff
 * (false for a NaN scale_diff).  kept (int32 [n_pairs]) receives the kept pair numbers in ascending order, cut
 * at `limit` entries (limit <= 0: no cut), and -1 in every entry after them; n_kept (one int32) the number of
 * entries written.  scale_diff (float64 [n_pairs]) may be NULL.  The order does not depend on scheduling: one
 * workgroup scans the list in chunks.  All pointers are device memory.  `workspace` is reserved: this version
 * uses none, and NULL / 0 are accepted.  Enqueue only, capturable, no host read.
 *
 * Checked on the host: NULL box1 / box2 / valid / kept / n_kept, n_pairs <= 0, a NaN min_scale_diff
 * -> OETR_ERR_BAD_ARG. */
oetr_status oetr_covis_select(const float *box1, const float *box2, const uint8_t *valid, int n_pairs,
                              double min_scale_diff, int limit, int32_t *kept, int32_t *n_kept,
                              double *scale_diff, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* OETR_COVIS_SET_H_ */
