// Feature bank (include/oetr_bank.h): a batch of pairs assembled, by index, from per-image token
// rows that outlive a call, and the token-resident forward path on the result.
//
// k_bank_gather is a pure copy of 2 N L rows of 1 KB.  A wave moves whole rows: one 16-byte load and
// one 16-byte store per lane and row (64 lanes x 16 B = the row), BANK_ROWS consecutive rows of one
// image per wave, all their loads issued before the first store.  The image index is a wave-uniform
// value read once per row block.  Both sides of the batch go in the one launch, the grid is sized from
// the row count (8 pairs of 20x20 tokens: 16 images x 25 workgroups of 16 rows over 256 CUs), no LDS.
#include <string>

#include "../../include/oetr_bank.h"
#include "common.h"

namespace oetr {

constexpr int BANK_ROWS = 4;                 // rows per wave, in flight together
constexpr int BANK_WAVES = 4;                // waves per workgroup
constexpr uint32_t FLAG_INDEX = 4u;          // == OETR_FLAG_INDEX
static_assert(FLAG_INDEX == OETR_FLAG_INDEX, "status bit");
static_assert(C * sizeof(float) == 64 * sizeof(f32x4), "a wave moves one row per instruction");

// (plain fields, selected by side with scalar selects: indexing arrays of a kernel argument by a run-time side makes
//  every field a scalar load of its own, one after the other, in front of the index load the row addresses wait for)
struct BankGather {
  const float *bank1, *bank2;
  const int32_t *idx1, *idx2;
  float *tokens1, *tokens2;
  int images1, images2;    // bank images per side (indices are clamped into [0, images))
  int L1, L2;              // token rows per image
  int n_pairs;
  uint32_t* flags;         // status word (may be NULL)
};

// grid: x = blocks of BANK_WAVES x BANK_ROWS rows inside one image (sized for the larger side; consecutive workgroups
// take consecutive rows), y = side * n_pairs + pair
__global__ __launch_bounds__(64 * BANK_WAVES) void k_bank_gather(const BankGather p) {
  // one row block per wave; everything up to the row pointers is wave-uniform (scalar registers)
  const int side = (int)blockIdx.y >= p.n_pairs;
  const int pair = (int)blockIdx.y - (side ? p.n_pairs : 0);
  const int L = side ? p.L2 : p.L1;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int row0 = ((int)blockIdx.x * BANK_WAVES + wave) * BANK_ROWS;
  if (row0 >= L) return;
  const int given = (side ? p.idx2 : p.idx1)[pair];
  const int last = (side ? p.images2 : p.images1) - 1;
  const int img = given < 0 ? 0 : (given > last ? last : given);     // never dereferenced as given
  const int lane = threadIdx.x & 63;
  if (given != img && row0 == 0 && p.flags && lane == 0) atomicOr(p.flags, FLAG_INDEX);
  const f32x4* src = reinterpret_cast<const f32x4*>((side ? p.bank2 : p.bank1) + ((size_t)img * L + row0) * C) + lane;
  f32x4* dst = reinterpret_cast<f32x4*>((side ? p.tokens2 : p.tokens1) + ((size_t)pair * L + row0) * C) + lane;
  if (L - row0 >= BANK_ROWS) {      // a full block: every load in flight before the first store
    f32x4 v[BANK_ROWS];
#pragma unroll
    for (int r = 0; r < BANK_ROWS; ++r) v[r] = src[(size_t)r * (C / 4)];
#pragma unroll
    for (int r = 0; r < BANK_ROWS; ++r) dst[(size_t)r * (C / 4)] = v[r];
  } else {                          // an image's last block when L is no multiple of BANK_ROWS
    for (int r = 0; r < L - row0; ++r) dst[(size_t)r * (C / 4)] = src[(size_t)r * (C / 4)];
  }
}

namespace {

// host-side validation of a gather's arguments (`who`: the entry point, for the message)
oetr_status bank_check(const char* who, const float* bank1, int bank1_images, const int32_t* idx1,
                       const float* bank2, int bank2_images, const int32_t* idx2, int n_pairs, long L1,
                       long L2) {
  if (!bank1 || !bank2 || !idx1 || !idx2)
    return entry_fail(who, OETR_ERR_BAD_ARG, "NULL bank / index pointer");
  if (n_pairs <= 0 || bank1_images <= 0 || bank2_images <= 0)
    return entry_fail(who, OETR_ERR_BAD_ARG, "need n_pairs > 0 and bank images > 0");
  if (L1 < 1 || L2 < 1 || L1 > OETR_MAX_TOKENS || L2 > OETR_MAX_TOKENS)
    return entry_fail(who, OETR_ERR_BAD_SHAPE, "need 1 <= L <= " + std::to_string(OETR_MAX_TOKENS));
  if ((long)n_pairs * (L1 + L2) > (1L << 30) / C)      // (the bound of a workspace: 32-bit row counts stay safe)
    return entry_fail(who, OETR_ERR_BAD_SHAPE, "more than 2^22 token rows");
  return OETR_OK;
}

oetr_status launch_bank_gather(const float* bank1, int bank1_images, const int32_t* idx1, const float* bank2,
                               int bank2_images, const int32_t* idx2, int n_pairs, int L1, int L2,
                               float* tokens1, float* tokens2, uint32_t* status_word, hipStream_t s) {
  constexpr int wg_rows = BANK_WAVES * BANK_ROWS;
  constexpr int max_pairs = 32767;      // 2 x pairs is the grid's y extent (at most 65535): more pairs, more launches
  const int Lmax = L1 > L2 ? L1 : L2;
  for (int p0 = 0; p0 < n_pairs; p0 += max_pairs) {
    BankGather p;
    p.bank1 = bank1; p.bank2 = bank2;
    p.idx1 = idx1 + p0; p.idx2 = idx2 + p0;
    p.tokens1 = tokens1 + (size_t)p0 * L1 * C; p.tokens2 = tokens2 + (size_t)p0 * L2 * C;
    p.images1 = bank1_images; p.images2 = bank2_images;
    p.L1 = L1; p.L2 = L2;
    p.n_pairs = n_pairs - p0 < max_pairs ? n_pairs - p0 : max_pairs;
    p.flags = status_word;
    const dim3 grid((unsigned)((Lmax + wg_rows - 1) / wg_rows), (unsigned)(2 * p.n_pairs));
    hipLaunchKernelGGL(k_bank_gather, grid, dim3(64 * BANK_WAVES), 0, s, p);
    const hipError_t e = hipGetLastError();             // (under the kernel's name: both entries launch it from here)
    if (e != hipSuccess) return entry_fail("k_bank_gather", OETR_ERR_HIP, hipGetErrorString(e));
  }
  return OETR_OK;
}

}  // namespace
}  // namespace oetr

using namespace oetr;

extern "C" {

int oetr_bank_abi_version(void) { return OETR_BANK_ABI_VERSION; }

oetr_status oetr_bank_gather(const float* bank1, int bank1_images, const int32_t* idx1,
                             const float* bank2, int bank2_images, const int32_t* idx2,
                             int n_pairs, int L1, int L2, float* tokens1, float* tokens2,
                             uint32_t* status_word, void* stream) {
  if (!tokens1 || !tokens2) return entry_fail("oetr_bank_gather", OETR_ERR_BAD_ARG, "NULL token buffer");
  if (oetr_status rc = bank_check("oetr_bank_gather", bank1, bank1_images, idx1, bank2, bank2_images, idx2,
                                  n_pairs, L1, L2))
    return rc;
  return launch_bank_gather(bank1, bank1_images, idx1, bank2, bank2_images, idx2, n_pairs, L1, L2, tokens1,
                            tokens2, status_word, static_cast<hipStream_t>(stream));
}

oetr_status oetr_forward_bank(oetr_handle h, const float* bank1, int bank1_images, const int32_t* idx1,
                              const float* bank2, int bank2_images, const int32_t* idx2, int n_pairs,
                              int hf1, int wf1, int hf2, int wf2, int img_h1, int img_w1, int img_h2,
                              int img_w2, void* workspace, size_t workspace_bytes, float* box1, float* box2,
                              uint32_t* flag_slot, void* stream) {
  // everything oetr_forward_tokens would refuse is refused here, before the gather is enqueued
  if (!h || !box1 || !box2) return entry_fail("oetr_forward_bank", OETR_ERR_BAD_ARG, "NULL handle / box output");
  if (hf1 <= 0 || wf1 <= 0 || hf2 <= 0 || wf2 <= 0)
    return entry_fail("oetr_forward_bank", OETR_ERR_BAD_SHAPE, "empty token grid");
  if (oetr_status rc = bank_check("oetr_forward_bank", bank1, bank1_images, idx1, bank2, bank2_images, idx2,
                                  n_pairs, (long)hf1 * wf1, (long)hf2 * wf2))
    return rc;
  if (img_h1 < hf1 || img_h2 < hf2 || img_w1 <= 0 || img_w2 <= 0)
    return entry_fail("oetr_forward_bank", OETR_ERR_BAD_SHAPE, "image size smaller than the token grid");
  float *tokens1, *tokens2, *pos1, *pos2;
  if (oetr_status rc = oetr_token_buffers(h, n_pairs, hf1, wf1, hf2, wf2, workspace, workspace_bytes, &tokens1,
                                          &tokens2, &pos1, &pos2))
    return rc;                                  // shape / workspace size and alignment
  // the workspace opens with its status word (OETR_WORKSPACE_STATUS_BYTES)
  if (oetr_status rc = launch_bank_gather(bank1, bank1_images, idx1, bank2, bank2_images, idx2, n_pairs,
                                          hf1 * wf1, hf2 * wf2, tokens1, tokens2,
                                          static_cast<uint32_t*>(workspace), static_cast<hipStream_t>(stream)))
    return rc;
  if (flag_slot)
    return oetr_forward_tokens_flagslot(h, n_pairs, hf1, wf1, hf2, wf2, img_h1, img_w1, img_h2, img_w2,
                                        workspace, workspace_bytes, box1, box2, flag_slot, stream);
  return oetr_forward_tokens(h, n_pairs, hf1, wf1, hf2, wf2, img_h1, img_w1, img_h2, img_w2, workspace,
                             workspace_bytes, box1, box2, stream);
}

}  // extern "C"
