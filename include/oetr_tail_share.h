/* Encoder tail sharing: one switch (and the tests' view of what it did) of liboetr_hip.so.
 *
 * With 64-row encoder workgroups an image of L tokens ends in a tile of L % 64 rows.  Where that is 1..16 rows
 * in BOTH images of the pairs (400 tokens per image: 16), the library runs a pair's two ragged last tiles in ONE
 * workgroup, as rows 0.. and 16.. of one 32-row MFMA tile: one workgroup per pair fewer in each of the nine
 * encoder launches of a forward call (13 instead of 14 at 400 tokens), every output bit-identical - the same
 * products in the same MFMA k-slots, exact zeros elsewhere.  It applies to OETR_DTYPE_F32_SPLIT_F16 and
 * OETR_DTYPE_F32_SPLIT_QK16 with linear attention; every other setting and shape runs as before.
 *
 * This header extends include/oetr_hip.h (same library, same status codes, same oetr_last_error);
 * OETR_ABI_VERSION does not change. */
#ifndef OETR_TAIL_SHARE_H_
#define OETR_TAIL_SHARE_H_

#include "oetr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* -1 (default): automatic - shared wherever the shape allows it.  0: off (tests compare both paths in one
 * build).  Anything else: OETR_ERR_BAD_ARG.  Mutates the handle like the setters of oetr_hip.h: call it
 * outside concurrent forward calls. */
oetr_status oetr_set_tail_share(oetr_handle h, int mode);

/* Tests only: workgroups of each encoder launch of the handle's most recent call (0 before the first; -1:
 * NULL handle) - N x (tiles of image 1 + tiles of image 2), or N fewer where the tails were shared. */
int oetr_debug_encoder_grid(oetr_handle h);

#ifdef __cplusplus
}
#endif

#endif /* OETR_TAIL_SHARE_H_ */
