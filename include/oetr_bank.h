/* Feature-bank extension of liboetr_hip.so: the hot path fed from per-image token rows
 * that outlive a call.
 *
 * The trunk and the neck of one image depend on that image alone, so a pair LIST over an
 * image SET (retrieval shortlists, SfM pair files, exhaustive matching) needs them once per
 * image, not once per pair.  A BANK is plain caller-owned device memory,
 *
 *     float bank[bank_images][L][256]        (token-major, L = hf * wf)
 *
 * holding exactly the rows oetr_neck_forward_tokens writes for one image after another.  The
 * library owns nothing new: the entries below gather a batch of pairs out of one or two banks
 * by index, on the device, and run the existing token-resident forward path on them.
 *
 * This header extends include/oetr_hip.h (same library, same status codes, same
 * oetr_last_error) and carries a version of its own; OETR_ABI_VERSION does not change. */
#ifndef OETR_BANK_H_
#define OETR_BANK_H_

#include "oetr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OETR_BANK_ABI_VERSION 1

/* Status-word bit (beside OETR_FLAG_F16_RANGE / OETR_FLAG_EXCHANGE): a pair index was outside
 * its bank.  The row was taken from the nearest valid image instead, so that call's outputs
 * are INVALID.  A caller bug, not something a re-run in another precision repairs. */
#define OETR_FLAG_INDEX 4u

int oetr_bank_abi_version(void);

/* One launch (k_bank_gather): for p in [0, n_pairs)
 *     tokens1[p] = bank1[idx1[p]]   (L1 x 256 floats)
 *     tokens2[p] = bank2[idx2[p]]   (L2 x 256 floats)
 * idx1 / idx2: DEVICE int32 [n_pairs].  The host never reads them, so the call is
 * enqueue-only and can be captured into a HIP graph; a replay sees the indices the buffers
 * hold at replay time.  bank2 may equal bank1.  An index outside [0, bankK_images) is CLAMPED
 * into range - never dereferenced as given - and OETR_FLAG_INDEX is OR-ed into *status_word
 * (device uint32; NULL: not reported).  tokens1 / tokens2 must not overlap the banks.
 *
 * Checked on the host before anything is enqueued: NULL bank / index / token pointers,
 * n_pairs <= 0, bankK_images <= 0 -> OETR_ERR_BAD_ARG; L1 or L2 outside 1..OETR_MAX_TOKENS,
 * or more than 2^22 token rows in all -> OETR_ERR_BAD_SHAPE. */
oetr_status oetr_bank_gather(const float *bank1, int bank1_images, const int32_t *idx1,
                             const float *bank2, int bank2_images, const int32_t *idx2,
                             int n_pairs, int L1, int L2, float *tokens1, float *tokens2,
                             uint32_t *status_word, void *stream);

/* The gather above into the workspace's token buffers (those oetr_token_buffers reports for
 * the shape), with the workspace's own status word, followed by oetr_forward_tokens - or, with
 * a non-NULL flag_slot, oetr_forward_tokens_flagslot - on them.  L1 = hf1 * wf1, L2 = hf2 * wf2.
 * The position tables must already be in the workspace, as for oetr_forward_tokens.  Every
 * argument is validated before the gather is enqueued (as above, plus the handle, the box
 * pointers, the shape and the workspace as oetr_forward_tokens validates them). */
oetr_status oetr_forward_bank(oetr_handle h, const float *bank1, int bank1_images,
                              const int32_t *idx1, const float *bank2, int bank2_images,
                              const int32_t *idx2, int n_pairs, int hf1, int wf1, int hf2, int wf2,
                              int img_h1, int img_w1, int img_h2, int img_w2, void *workspace,
                              size_t workspace_bytes, float *box1, float *box2,
                              uint32_t *flag_slot, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* OETR_BANK_H_ */
