/* Batched box -> crop extension of liboetr_hip.so: the crop step for a whole chunk of pairs in one call.
 *
 * oetr_overlap_crop (include/oetr_hip.h) crops ONE pair: three launches, one of them a single thread,
 * and the reference it restates is hard-wired to bbox[0].  Every stage before it works on 8-32 pairs
 * per call.  oetr_overlap_crop_batch is the same step for n pairs: a constant number of launches
 * whatever n is (2 for size_divisor == 1, 3 otherwise), images of different sizes inside one call, no
 * allocation, and the n geometry records next to each other in one device array.
 *
 * Pair k of a call produces the oetr_crop_info and the pixels oetr_overlap_crop produces for that pair
 * alone, bit for bit: both entries are built on one copy of the arithmetic (csrc/crop_sample.h).
 *
 * This header extends include/oetr_hip.h (same library, same status codes, same oetr_last_error, the
 * same oetr_crop_info) and carries a version of its own; OETR_ABI_VERSION does not change. */
#ifndef OETR_CROP_BATCH_H_
#define OETR_CROP_BATCH_H_

#include "oetr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OETR_CROP_BATCH_ABI_VERSION 1
#define OETR_CROP_BATCH_MAX_PAIRS 32767   /* two sides of a pair per grid plane */

int oetr_crop_batch_abi_version(void);

typedef struct {            /* one per pair; DEVICE memory, filled by the caller; 48 bytes */
  const float *image[2];    /* [channels][h][w], the matcher's images; an image may appear in any number of pairs */
  int32_t h[2], w[2];
  float   scale[2][2];      /* overlap_scales (sx, sy) of each side */
} oetr_crop_pair;

/* Floats per output slot: channels x ceil(max_h/d)*d x ceil(max_w/d)*d with d = size_divisor, the two
 * rounded sizes in *cap_h / *cap_w (either may be NULL).  0 on bad arguments (a size < 1).  No GPU needed. */
size_t oetr_crop_batch_capacity(int channels, int max_h, int max_w, int size_divisor, int *cap_h, int *cap_w);

/*   pairs         device [n]        the table above; max_h / max_w bound every image of the call
 *   box1/box2     device [n][4]     the OETR boxes of the n pairs, OETR input frame (forward_dummy's
 *                                   outputs as they are; any float is taken: the box domain, below)
 *   keep_aspect, size_divisor, gate_mode     as for oetr_overlap_crop, one setting for the call
 *   tmp           n*2*capacity floats of scratch between the two resize passes; may be NULL when
 *                 size_divisor == 1 (nothing is resized twice then)
 *   out           [n][2][capacity]: crop (k, i) densely packed [channels][out_h][out_w] at the START of
 *                 slot (k, i); the rest of a slot is not written
 *   capacity_floats   floats per slot, at least oetr_crop_batch_capacity()
 *   info          device [n], written by the first launch
 *
 * info[k] is exactly what oetr_overlap_crop writes for pair k, for EVERY box: valid = 1 (crops made),
 * valid = 0 for a failed gate (both images copied into their slots bit for bit) and valid = -1 (no crops:
 * nothing read from the pair's images, nothing written to its tmp / out slots).  valid = -1 is the one
 * rule of include/oetr_hip.h (THE BOX DOMAIN): a pair with a scaled coordinate that does not truncate into
 * [0, 2^31) - negative, NaN, infinite, huge - tested in float before any conversion and before the gate
 * (all integer fields and ratios zero, sbox the scaled floats); or, inside the domain, a crop that is
 * empty or does not fit (new_* / out_* zeroed).  A record with valid = 1 therefore has box >= 0: no
 * kernel forms an address from a negative origin.  The "fits" test is made against the pair's OWN
 * capacity - its two image sizes rounded up to size_divisor, what oetr_overlap_crop_capacity gives for it
 * - not the slot's.  The host never reads the table, so what it cannot check is reported from the device:
 * a pair with an image larger than max_h x max_w, a size < 1 or a NULL image gets valid = -1 and is never
 * dereferenced.
 *
 * Enqueue-only: no device-to-host copy, no synchronisation, no allocation; the caller owns every
 * buffer, and the call can be captured into a HIP graph (a replay sees the boxes and the table the
 * buffers hold at replay time).
 *
 * Checked on the host before any HIP call (so the checks work without a GPU): NULL pairs / box / out /
 * info, n < 1 or > OETR_CROP_BATCH_MAX_PAIRS, channels / max_h / max_w < 1, size_divisor < 1, gate_mode
 * outside {0, 1}, tmp == NULL with size_divisor > 1 -> OETR_ERR_BAD_ARG; capacity_floats smaller than
 * oetr_crop_batch_capacity() -> OETR_ERR_WORKSPACE. */
oetr_status oetr_overlap_crop_batch(const oetr_crop_pair *pairs, int n, int channels, int max_h, int max_w,
                                    const float *box1, const float *box2, int keep_aspect, int size_divisor,
                                    int gate_mode, float *tmp, float *out, size_t capacity_floats,
                                    oetr_crop_info *info, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* OETR_CROP_BATCH_H_ */
