// Assembling matcher output into origin-frame match lists (include/oetr_match_assembly.h): the tail of the
// reference's process() - keypoints mapped back into the original pictures, matches0 turned into lists - for all
// pairs of a call, with the geometry records oetr_overlap_crop_batch left on the device.
//
// Three launches, ordered by the launch boundary alone (no workgroup waits on another):
//   k_asm_count   one workgroup per pair: kept / rejected matches of the pair -> counts[p][0..3], workspace[p].
//   k_asm_scan    ONE workgroup: exclusive scan of the kept counts into offsets (chunks of 1024 pairs, a running
//                 base carried across chunks), and the ordered compaction of the pair numbers with too few matches.
//   k_asm_emit    one workgroup per pair walks the pair's rows of side 0 in order, 1024 at a time: origin0 of the row,
//                 the 64-bit ballot of "kept" with a popcount prefix inside the wave, wave totals through LDS, a
//                 running base across chunks - so list row = offsets[p] + (number of kept rows before it), decided
//                 by arithmetic.  A kept row also converts kp1[off1[p] + b] with asm_origin, the ONE copy of the
//                 arithmetic, which the same workgroup then uses for its origin1 rows.  Rows of the list outputs from
//                 offsets[P] on are written -1 / NaN by the workgroup whose side-0 rows have those numbers (the
//                 first / last workgroup also take the rows before off0[0] / from off0[P] on), so the tail is tiled
//                 exactly once and is disjoint from every kept row (those lie below offsets[P]).
//
// Nothing is dereferenced on the strength of device data alone: asm_range clamps the offsets into [0, n], K1 is the
// clamped length, a match index passes ONE unsigned compare against K1 before it forms an address (a negative value
// and, for int64, anything beyond int32 fail it as a huge unsigned number), and a list row is written only when
// (unsigned)row < n_kp0.
#include <string>
#include <type_traits>

#include "../../include/oetr_match_assembly.h"
#include "common.h"

namespace oetr {

// 1024 threads: a pair of 2048 rows is two chunks with one barrier each.  With 256 threads (eight chunks) 256 pairs
// took 25.1 us instead of 18.4 us and 1024 pairs 46.1 us instead of 46.9 us (one run of the probe per build, DESIGN
// 9.3h; profiles/match_assembly_probe.json has the shipped form).
constexpr int ASM_THREADS = 1024;
constexpr int ASM_WAVES = ASM_THREADS / 64;
constexpr int ASM_SCAN_THREADS = 1024;
constexpr int ASM_SCAN_WAVES = ASM_SCAN_THREADS / 64;
constexpr int ASM_COUNTERS = OETR_MATCH_ASSEMBLY_COUNTERS;

struct AsmRange {
  int s, e;
};

// rows off[p] .. off[p+1]-1, clamped: 0 <= s <= e <= n whatever the device holds
__device__ __forceinline__ AsmRange asm_range(const int32_t* __restrict__ off, int p, int n) {
  int s = off[p], e = off[p + 1];
  s = s < 0 ? 0 : (s > n ? n : s);
  e = e < s ? s : (e > n ? n : e);
  return {s, e};
}

// 0 <= v < K1 as one unsigned compare (K1 >= 0); rejected: v >= K1
template <typename M>
__device__ __forceinline__ bool asm_keep(M v, int K1, bool& rejected) {
  using U = std::make_unsigned_t<M>;
  const bool keep = (U)v < (U)K1;
  rejected = !keep && v >= 0;
  return keep;
}

struct AsmSide {
  float rx, ry, bx, by;
  double sx, sy;
};

__device__ __forceinline__ AsmSide asm_side(const oetr_crop_info* __restrict__ g, const double* __restrict__ scales,
                                            int p, int i) {
  AsmSide s;
  s.rx = (float)g->ratio[i][0], s.ry = (float)g->ratio[i][1];      // the reference's float32 [1,2] ratio
  s.bx = g->sbox[i][0], s.by = g->sbox[i][1];
  s.sx = scales[(size_t)p * 4 + 2 * i], s.sy = scales[(size_t)p * 4 + 2 * i + 1];
  return s;
}

// The one copy of the arithmetic: (k / ratio + bbox[:2]) in float32, each operation rounded on its own (the quotient
// is the correctly rounded one: v_div_scale / v_div_fmas / v_div_fixup, denormals kept), times the float64 scale.
__device__ __forceinline__ double2 asm_origin(const AsmSide& s, float2 k) {
#pragma clang fp contract(off)
  const float qx = k.x / s.rx, qy = k.y / s.ry;
  const float tx = qx + s.bx, ty = qy + s.by;
  return make_double2((double)tx * s.sx, (double)ty * s.sy);
}

__device__ __forceinline__ double2 asm_nan2() {
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  return make_double2(nan, nan);
}

template <typename M>
__global__ __launch_bounds__(ASM_THREADS) void k_asm_count(const oetr_crop_info* __restrict__ info,
                                                           const int32_t* __restrict__ off0, int n0,
                                                           const int32_t* __restrict__ off1, int n1,
                                                           const M* __restrict__ matches, int32_t* __restrict__ kept_ws,
                                                           int32_t* __restrict__ counts) {
  __shared__ int s_kept[ASM_WAVES], s_rej[ASM_WAVES];
  const int p = (int)blockIdx.x, tid = (int)threadIdx.x;
  int32_t* c = counts + (size_t)p * ASM_COUNTERS;
  if (info[p].valid < 0) {                                          // wave-uniform: no crops were made
    if (tid == 0) {
      c[0] = c[1] = c[2] = c[3] = -1;
      kept_ws[p] = 0;
    }
    return;
  }
  const AsmRange r0 = asm_range(off0, p, n0), r1 = asm_range(off1, p, n1);
  const int K1 = r1.e - r1.s;
  int kept = 0, rej = 0;
  for (int64_t r = (int64_t)r0.s + tid; r < (int64_t)r0.e; r += ASM_THREADS) {   // 64-bit: r0.e may be INT32_MAX
    bool rejected;
    kept += asm_keep<M>(matches[r], K1, rejected) ? 1 : 0;
    rej += rejected ? 1 : 0;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    kept += __shfl_xor(kept, d, 64);
    rej += __shfl_xor(rej, d, 64);
  }
  if ((tid & 63) == 0) s_kept[tid >> 6] = kept, s_rej[tid >> 6] = rej;
  __syncthreads();
  if (tid == 0) {
    kept = rej = 0;
#pragma unroll
    for (int w = 0; w < ASM_WAVES; ++w) kept += s_kept[w], rej += s_rej[w];
    c[0] = r0.e - r0.s, c[1] = K1, c[2] = kept, c[3] = rej;
    kept_ws[p] = kept;
  }
}

// One workgroup.  offsets[p] = min(sum of kept[0..p), n0): saturated in 64 bits, so non-decreasing and inside the
// list outputs whatever the offsets of the inputs were.  few: the pairs whose kept counter (-1 for a pair without
// crops) is below min_matches, in list order; few == NULL: no selection.
__global__ __launch_bounds__(ASM_SCAN_THREADS) void k_asm_scan(const int32_t* __restrict__ kept_ws,
                                                               const int32_t* __restrict__ counts, int n_pairs, int n0,
                                                               int min_matches, int32_t* __restrict__ offsets,
                                                               int32_t* __restrict__ few, int32_t* __restrict__ n_few) {
  __shared__ long long s_sum[2][ASM_SCAN_WAVES];
  __shared__ int s_few[2][ASM_SCAN_WAVES];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  long long base = 0;
  int few_base = 0, buf = 0;
  for (int c = 0; c < n_pairs; c += ASM_SCAN_THREADS, buf ^= 1) {  // uniform trip count
    const int p = c + tid;                                          // c + tid <= INT32_MAX / 4 + 1023
    const bool active = p < n_pairs;
    const long long k = active ? (long long)kept_ws[p] : 0;
    long long incl = k;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const long long up = __shfl_up(incl, d, 64);
      if (lane >= d) incl += up;
    }
    const bool is_few = active && few != nullptr && counts[(size_t)p * ASM_COUNTERS + 2] < min_matches;
    const unsigned long long fb = __ballot(is_few);
    if (lane == 63) s_sum[buf][wave] = incl;
    if (lane == 0) s_few[buf][wave] = __popcll(fb);
    __syncthreads();                                                // two buffers: one barrier per chunk
    long long before = 0, total = 0;
    int few_before = 0, few_total = 0;
#pragma unroll
    for (int w = 0; w < ASM_SCAN_WAVES; ++w) {
      const long long t = s_sum[buf][w];
      const int f = s_few[buf][w];
      if (w < wave) before += t, few_before += f;
      total += t, few_total += f;
    }
    if (active) {
      const long long at = base + before + incl - k;
      offsets[p] = (int32_t)(at < (long long)n0 ? at : (long long)n0);
    }
    if (is_few) few[few_base + few_before + __popcll(fb & ((1ull << lane) - 1ull))] = p;   // < n_pairs entries
    base += total;
    few_base += few_total;
  }
  if (tid == 0) {
    offsets[n_pairs] = (int32_t)(base < (long long)n0 ? base : (long long)n0);
    if (n_few) n_few[0] = few_base;
  }
  if (few)
    for (int i = few_base + tid; i < n_pairs; i += ASM_SCAN_THREADS) few[i] = -1;
}

template <typename M>
__global__ __launch_bounds__(ASM_THREADS) void k_asm_emit(
    const oetr_crop_info* __restrict__ info, const double* __restrict__ scales, int n_pairs,
    const float* __restrict__ kp0, const int32_t* __restrict__ off0, int n0, const float* __restrict__ kp1,
    const int32_t* __restrict__ off1, int n1, const M* __restrict__ matches, const float* __restrict__ conf,
    const int32_t* __restrict__ offsets, double* __restrict__ origin0, double* __restrict__ origin1,
    int32_t* __restrict__ index0, int32_t* __restrict__ index1, float* __restrict__ k1, float* __restrict__ k2,
    float* __restrict__ mconf) {
  __shared__ int s_tot[2][ASM_WAVES];
  const int p = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const oetr_crop_info* g = info + p;
  const bool ok = g->valid >= 0;                                    // wave-uniform
  const AsmRange r0 = asm_range(off0, p, n0), r1 = asm_range(off1, p, n1);
  const int K1 = r1.e - r1.s;
  const AsmSide side0 = asm_side(g, scales, p, 0), side1 = asm_side(g, scales, p, 1);
  const float2* kp0v = reinterpret_cast<const float2*>(kp0);
  const float2* kp1v = reinterpret_cast<const float2*>(kp1);
  double2* o0v = reinterpret_cast<double2*>(origin0);
  double2* o1v = reinterpret_cast<double2*>(origin1);
  float2* k1v = reinterpret_cast<float2*>(k1);
  float2* k2v = reinterpret_cast<float2*>(k2);
  const float nanf = __int_as_float(0x7fc00000);
  int total = offsets[n_pairs], first = offsets[p];                 // k_asm_scan's: inside [0, n0]; clamped all the same
  total = total < 0 ? 0 : (total > n0 ? n0 : total);
  first = first < 0 ? 0 : (first > n0 ? n0 : first);
  unsigned base = (unsigned)first;                                  // <= n0 + K0 < 2^32

  // side 0: the pair's rows, with the rows before the first pair's / after the last pair's
  const int lo = p == 0 ? 0 : r0.s, hi = p == n_pairs - 1 ? n0 : r0.e;
  int buf = 0;
  for (int64_t c = lo; c < (int64_t)hi; c += ASM_THREADS, buf ^= 1) {   // uniform trip count; 64-bit: hi may be INT32_MAX
    const int64_t r64 = c + tid;
    const bool in = r64 < (int64_t)hi;
    const int r = in ? (int)r64 : lo;
    const bool own = in && ok && r >= r0.s && r < r0.e;
    double2 o = asm_nan2();
    bool keep = false;
    int b = 0;
    if (own) {
      o = asm_origin(side0, kp0v[r]);
      const M v = matches[r];
      bool rejected;
      keep = asm_keep<M>(v, K1, rejected);
      b = keep ? (int)v : 0;                                        // 0 <= b < K1 <= n1
    }
    if (in) o0v[r] = o;
    const unsigned long long kb = __ballot(keep);
    if (lane == 0) s_tot[buf][wave] = __popcll(kb);
    __syncthreads();                                                // two buffers: one barrier per chunk
    unsigned before = 0, chunk = 0;
#pragma unroll
    for (int w = 0; w < ASM_WAVES; ++w) {
      const unsigned t = (unsigned)s_tot[buf][w];
      if (w < wave) before += t;
      chunk += t;
    }
    if (keep) {
      const unsigned dst = base + before + (unsigned)__popcll(kb & ((1ull << lane) - 1ull));
      if (dst < (unsigned)n0) {
        const double2 o2 = asm_origin(side1, kp1v[(size_t)r1.s + (size_t)b]);
        index0[dst] = r - r0.s;
        index1[dst] = b;
        k1v[dst] = make_float2((float)o.x, (float)o.y);
        k2v[dst] = make_float2((float)o2.x, (float)o2.y);
        if (conf) mconf[dst] = conf[r];
      }
    }
    if (in && r >= total) {                                         // the tail of the list outputs
      index0[r] = -1;
      index1[r] = -1;
      k1v[r] = make_float2(nanf, nanf);
      k2v[r] = make_float2(nanf, nanf);
      if (conf) mconf[r] = nanf;
    }
    base += chunk;
  }

  // side 1 likewise
  const int lo1 = p == 0 ? 0 : r1.s, hi1 = p == n_pairs - 1 ? n1 : r1.e;
  for (int64_t r = (int64_t)lo1 + tid; r < (int64_t)hi1; r += ASM_THREADS) {
    const bool own = ok && r >= r1.s && r < r1.e;
    o1v[r] = own ? asm_origin(side1, kp1v[r]) : asm_nan2();
  }
}

namespace {

constexpr const char* ME = "oetr_assemble_matches";

bool asm_aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

template <typename M>
oetr_status asm_launch(const oetr_crop_info* info, const double* scales, int n_pairs, const float* kp0,
                       const int32_t* off0, int n0, const float* kp1, const int32_t* off1, int n1, const void* matches,
                       const float* conf, int min_matches, int32_t* kept_ws, double* origin0, double* origin1,
                       int32_t* index0, int32_t* index1, float* k1, float* k2, float* mconf, int32_t* offsets,
                       int32_t* counts, int32_t* few, int32_t* n_few, hipStream_t s) {
  const M* m = static_cast<const M*>(matches);
  hipLaunchKernelGGL(k_asm_count<M>, dim3((unsigned)n_pairs), dim3(ASM_THREADS), 0, s, info, off0, n0, off1, n1, m,
                     kept_ws, counts);
  if (oetr_status rc = entry_hip(ME, hipGetLastError(), "k_asm_count")) return rc;
  hipLaunchKernelGGL(k_asm_scan, dim3(1), dim3(ASM_SCAN_THREADS), 0, s, kept_ws, counts, n_pairs, n0, min_matches,
                     offsets, few, n_few);
  if (oetr_status rc = entry_hip(ME, hipGetLastError(), "k_asm_scan")) return rc;
  hipLaunchKernelGGL(k_asm_emit<M>, dim3((unsigned)n_pairs), dim3(ASM_THREADS), 0, s, info, scales, n_pairs, kp0, off0,
                     n0, kp1, off1, n1, m, conf, offsets, origin0, origin1, index0, index1, k1, k2, mconf);
  return entry_hip(ME, hipGetLastError(), "k_asm_emit");
}

}  // namespace
}  // namespace oetr

using namespace oetr;

extern "C" {

int oetr_match_assembly_abi_version(void) { return OETR_MATCH_ASSEMBLY_ABI_VERSION; }

size_t oetr_match_assembly_workspace_bytes(int n_pairs) {
  if (n_pairs < 1) return 0;
  return (((size_t)n_pairs * sizeof(int32_t)) + 255) / 256 * 256;
}

// The host code dereferences none of its pointer arguments and reads nothing from the device.
oetr_status oetr_assemble_matches(const oetr_crop_info* info, const double* scales, int n_pairs, const float* kp0,
                                  const int32_t* off0, int64_t n_kp0, const float* kp1, const int32_t* off1,
                                  int64_t n_kp1, const void* matches, int match_bytes, const float* conf,
                                  int min_matches, void* workspace, size_t workspace_bytes, double* origin0,
                                  double* origin1, int32_t* index0, int32_t* index1, float* k1, float* k2,
                                  float* mconf, int32_t* offsets, int32_t* counts, int32_t* few, int32_t* n_few,
                                  void* stream) {
  if (!info || !scales || !off0 || !off1)
    return entry_fail(ME, OETR_ERR_BAD_ARG, "NULL geometry record / scales / off0 / off1 pointer");
  if (!offsets || !counts) return entry_fail(ME, OETR_ERR_BAD_ARG, "NULL offsets / counts output");
  if (!workspace) return entry_fail(ME, OETR_ERR_BAD_ARG, "NULL workspace");
  if (n_pairs <= 0) return entry_fail(ME, OETR_ERR_BAD_ARG, "need n_pairs > 0");
  if (n_kp0 < 0 || n_kp1 < 0) return entry_fail(ME, OETR_ERR_BAD_ARG, "need n_kp0 >= 0 and n_kp1 >= 0");
  if (match_bytes != 4 && match_bytes != 8)
    return entry_fail(ME, OETR_ERR_BAD_ARG, "match_bytes must be 4 (int32) or 8 (int64), got " + std::to_string(match_bytes));
  if (min_matches < 0) return entry_fail(ME, OETR_ERR_BAD_ARG, "need min_matches >= 0 (few = n_few = NULL: no selection)");
  if ((few == nullptr) != (n_few == nullptr)) return entry_fail(ME, OETR_ERR_BAD_ARG, "few and n_few go together");
  if (n_kp0 != 0 && (!kp0 || !matches)) return entry_fail(ME, OETR_ERR_BAD_ARG, "NULL kp0 / matches pointer");
  if (n_kp0 != 0 && (!origin0 || !index0 || !index1 || !k1 || !k2))
    return entry_fail(ME, OETR_ERR_BAD_ARG, "NULL origin0 / index0 / index1 / k1 / k2 output");
  if (n_kp1 != 0 && (!kp1 || !origin1)) return entry_fail(ME, OETR_ERR_BAD_ARG, "NULL kp1 / origin1 pointer");
  if (n_kp0 != 0 && (conf == nullptr) != (mconf == nullptr))
    return entry_fail(ME, OETR_ERR_BAD_ARG, "conf and mconf go together");
  if (!asm_aligned(kp0, 8) || !asm_aligned(kp1, 8) || !asm_aligned(k1, 8) || !asm_aligned(k2, 8) ||
      !asm_aligned(origin0, 16) || !asm_aligned(origin1, 16) || !asm_aligned(matches, (uintptr_t)match_bytes))
    return entry_fail(ME, OETR_ERR_BAD_ARG, "keypoint rows must be 8-byte aligned, origin rows 16-byte, matches to their size");
  if (n_pairs > INT32_MAX / ASM_COUNTERS)
    return entry_fail(ME, OETR_ERR_BAD_SHAPE, "need n_pairs <= " + std::to_string(INT32_MAX / ASM_COUNTERS));
  if (n_kp0 > (int64_t)INT32_MAX || n_kp1 > (int64_t)INT32_MAX)
    return entry_fail(ME, OETR_ERR_BAD_SHAPE, "need n_kp0, n_kp1 <= " + std::to_string(INT32_MAX) + " (the offsets are int32)");
  if (workspace_bytes < oetr_match_assembly_workspace_bytes(n_pairs))
    return entry_fail(ME, OETR_ERR_WORKSPACE, "workspace of " + std::to_string(workspace_bytes) + " bytes, need " +
                                            std::to_string(oetr_match_assembly_workspace_bytes(n_pairs)));
  hipStream_t s = static_cast<hipStream_t>(stream);
  int32_t* kept_ws = static_cast<int32_t*>(workspace);
  const int n0 = (int)n_kp0, n1 = (int)n_kp1;
  if (match_bytes == 4)
    return asm_launch<int32_t>(info, scales, n_pairs, kp0, off0, n0, kp1, off1, n1, matches, conf, min_matches, kept_ws,
                               origin0, origin1, index0, index1, k1, k2, mconf, offsets, counts, few, n_few, s);
  return asm_launch<int64_t>(info, scales, n_pairs, kp0, off0, n0, kp1, off1, n1, matches, conf, min_matches, kept_ws,
                             origin0, origin1, index0, index1, k1, k2, mconf, offsets, counts, few, n_few, s);
}

}  // extern "C"
