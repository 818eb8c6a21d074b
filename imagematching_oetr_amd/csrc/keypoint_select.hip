// Keypoints selected and descriptors sampled from dense maps (include/oetr_keypoint_select.h): the head behind an
// extractor network - simple_nms, the threshold, the border, the best max_keypoints, sample_descriptors - for all maps
// of a call, of mixed sizes.  The statement is the header's; tests/keypoint_select_oracle.py is its numpy form.
//
// Thirteen launches, ordered by the launch boundary alone (no workgroup waits on another):
//   k_ks_nms<0..5>  ten elementwise passes (0, 1, then 2..5 twice).  The window maximum is separable, rows then
//                   columns, so a pass reads 2r+1 neighbours of one plane and writes its own pixel of another:
//                     0  A = rowmax(S)                      1  M = (S == colmax(A))
//                     2  Bm = rowmax(M)                     3  supp = colmax(Bm)
//                     4  A = rowmax(supp ? 0 : S)           5  M |= ((supp ? 0 : S) == colmax(A)) & !supp
//                   A (float), M, Bm, supp (bytes) are planes of the workspace; a map's pixels start at its
//                   pixel_offset.  A block owns one map (grid x) and 2048 of its pixels (grid y).  A tiled form
//                   with the 5r halo in LDS would hold 2 floats + 2 bytes per cell: 125 KB for a 32^2 tile at r = 8.
//   k_ks_select     one workgroup per map: walks the pixels in raster order, 4096 at a time, and compacts the
//                   candidates' raster indices into the map's part of plane A (free by now) - the position is the
//                   popcount prefix inside the wave, the wave totals through LDS, a running base across chunks.  With
//                   more than max_keypoints candidates: a radix select over the scores' bit patterns (positive floats
//                   order as unsigned integers; four 8-bit histogram passes whose LDS atomics only COUNT), the ties at
//                   the cut taken in raster order by the same prefix, then a bitonic sort of at most 4096 keys
//                   (score bits << 32 | ~index, descending: 32 KB of LDS).
//   k_ks_scan       ONE workgroup: exclusive scan of the kept counts into offsets.
//   k_ks_emit       one wave per keypoint slot: the keypoint, its score, the four taps with lanes over d (coalesced for
//                   channels-last maps), the 64 partial sums of squares - lane j holds partial j - and the fixed tree
//                   by wave shuffles; the arithmetic is keypoint_select_math.h, which the host compiles too.  The wave
//                   of slot b * k + i also writes the tail row of that number.
//
// Nothing of a record is dereferenced before ks_view has checked its sizes and its pixel range against the call's
// bounds; a raster index read back from the workspace is clamped below H * W before it forms an address.
#include <string>

#include "../../include/oetr_keypoint_select.h"
#include "common.h"
#include "keypoint_select_math.h"

namespace oetr {

constexpr int KS_THREADS = 256;
constexpr int KS_PIX_PER_BLOCK = 2048;
constexpr int KS_SEL_THREADS = 1024;
constexpr int KS_SEL_WAVES = KS_SEL_THREADS / 64;
constexpr int KS_SEL_CHUNK = KS_SEL_THREADS * 4;
constexpr int KS_MAX_K = OETR_KEYPOINT_SELECT_MAX_KEYPOINTS;
constexpr int KS_COUNTERS = OETR_KEYPOINT_SELECT_COUNTERS;
constexpr int KS_MAX_SIDE = OETR_KEYPOINT_SELECT_MAX_SIDE;
constexpr int KS_EMIT_WAVES = 4;
constexpr int KS_MAX_D_PER_LANE = OETR_KEYPOINT_SELECT_MAX_D / 64;

struct KsView {
  bool ok;
  int H, W, HW;
};

// the sizes of a record, checked: ok means 1 <= H, W, h, w <= 8192, H * W <= max_pixels and the pixel range
// [pixel_offset, pixel_offset + H * W) aligned and inside [0, total_pixels)
__device__ __forceinline__ KsView ks_view(const oetr_keypoint_map& m, int64_t max_pixels, int64_t total_pixels) {
  KsView v;
  v.H = m.H, v.W = m.W;
  bool ok = m.H >= 1 && m.H <= KS_MAX_SIDE && m.W >= 1 && m.W <= KS_MAX_SIDE && m.h >= 1 && m.h <= KS_MAX_SIDE &&
            m.w >= 1 && m.w <= KS_MAX_SIDE;
  const int64_t hw = ok ? (int64_t)m.H * m.W : 0;
  ok = ok && hw <= max_pixels && m.pixel_offset >= 0 && (m.pixel_offset % OETR_KEYPOINT_SELECT_PIXEL_ALIGN) == 0 &&
       m.pixel_offset <= total_pixels - hw;
  v.ok = ok;
  v.HW = ok ? (int)hw : 0;
  return v;
}

__device__ __forceinline__ float ks_score(const oetr_keypoint_map& m, int y, int x) {
  return ks::load_score(m.scores[(int64_t)y * m.score_stride + x]);   // a NaN score is loaded as -inf
}

// One pass of the NMS (the table above).  The maximum is a compare and a select, so the value kept is a copy of an
// input, bit for bit.
template <int PASS>
__global__ __launch_bounds__(KS_THREADS) void k_ks_nms(const oetr_keypoint_map* __restrict__ maps, int64_t max_pixels,
                                                       int64_t total_pixels, int r, float* __restrict__ A,
                                                       uint8_t* __restrict__ M, uint8_t* __restrict__ Bm,
                                                       uint8_t* __restrict__ supp) {
  const oetr_keypoint_map m = maps[blockIdx.x];
  const KsView v = ks_view(m, max_pixels, total_pixels);
  const int64_t first = (int64_t)blockIdx.y * KS_PIX_PER_BLOCK;
  if (!v.ok || first >= (int64_t)v.HW) return;
  const int H = v.H, W = v.W;
  const int end = (int)first + KS_PIX_PER_BLOCK < v.HW ? (int)first + KS_PIX_PER_BLOCK : v.HW;
  float* a = A + m.pixel_offset;
  uint8_t* mk = M + m.pixel_offset;
  uint8_t* bm = Bm + m.pixel_offset;
  uint8_t* sp = supp + m.pixel_offset;
  for (int i = (int)first + (int)threadIdx.x; i < end; i += KS_THREADS) {
    const int y = i / W, x = i - y * W;
    const int x_lo = x - r < 0 ? 0 : x - r, x_hi = x + r > W - 1 ? W - 1 : x + r;
    const int y_lo = y - r < 0 ? 0 : y - r, y_hi = y + r > H - 1 ? H - 1 : y + r;
    if (PASS == 0 || PASS == 4) {
      float best = -INFINITY;
      for (int xx = x_lo; xx <= x_hi; ++xx) {
        float s = ks_score(m, y, xx);
        if (PASS == 4 && sp[y * W + xx]) s = 0.0f;
        best = s > best ? s : best;
      }
      a[i] = best;
    } else if (PASS == 1 || PASS == 5) {
      float best = -INFINITY;
      for (int yy = y_lo; yy <= y_hi; ++yy) {
        const float t = a[yy * W + x];
        best = t > best ? t : best;
      }
      const float s = ks_score(m, y, x);
      if (PASS == 1) {
        mk[i] = s == best ? 1 : 0;
      } else if (!sp[i] && s == best) {
        mk[i] = 1;
      }
    } else if (PASS == 2) {
      uint8_t any = 0;
      for (int xx = x_lo; xx <= x_hi; ++xx) any |= mk[y * W + xx];
      bm[i] = any;
    } else {
      uint8_t any = 0;
      for (int yy = y_lo; yy <= y_hi; ++yy) any |= bm[yy * W + x];
      sp[i] = any;
    }
  }
}

// the position of a thread's `n` entries among those of the workgroup's threads in order, and the workgroup's total:
// an inclusive scan inside the wave, the wave totals through `s_tot` (one barrier; the caller alternates two buffers)
__device__ __forceinline__ int ks_prefix(int n, int* s_tot, int& total) {
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  int incl = n;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int up = __shfl_up(incl, d, 64);
    if (lane >= d) incl += up;
  }
  if (lane == 63) s_tot[wave] = incl;
  __syncthreads();
  int before = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < KS_SEL_WAVES; ++w) {
    const int t = s_tot[w];
    if (w < wave) before += t;
    total += t;
  }
  return before + incl - n;
}

__device__ __forceinline__ unsigned ks_bits_at(const oetr_keypoint_map& m, const KsView& v, int idx) {
  idx = (unsigned)idx < (unsigned)v.HW ? idx : 0;
  const int y = idx / v.W, x = idx - y * v.W;
  return __float_as_uint(ks_score(m, y, x));
}

__global__ __launch_bounds__(KS_SEL_THREADS) void k_ks_select(const oetr_keypoint_map* __restrict__ maps,
                                                              int64_t max_pixels, int64_t total_pixels, float threshold,
                                                              int border, int k, float* __restrict__ A,
                                                              const uint8_t* __restrict__ M, int32_t* __restrict__ sel,
                                                              int32_t* __restrict__ counts) {
  __shared__ unsigned long long s_keys[KS_MAX_K];
  __shared__ unsigned s_hist[256];
  __shared__ int s_tot[2][KS_SEL_WAVES], s_tot2[2][KS_SEL_WAVES];
  __shared__ unsigned s_prefix;
  __shared__ int s_need;
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
  const oetr_keypoint_map m = maps[b];
  const KsView v = ks_view(m, max_pixels, total_pixels);
  int32_t* out = sel + (int64_t)b * k;
  if (!v.ok) {                                                      // uniform
    if (tid == 0) counts[(int64_t)b * KS_COUNTERS] = counts[(int64_t)b * KS_COUNTERS + 1] = -1;
    return;
  }
  const int H = v.H, W = v.W, HW = v.HW;
  int32_t* list = reinterpret_cast<int32_t*>(A + m.pixel_offset);  // HW entries: the map's part of plane A
  const uint8_t* mk = M + m.pixel_offset;

  // the candidates' raster indices, in raster order
  int C = 0, buf = 0;
  for (int c = 0; c < HW; c += KS_SEL_CHUNK, buf ^= 1) {            // uniform trip count
    const int i0 = c + tid * 4;                                     // < HW + 4096: no overflow
    bool cand[4] = {false, false, false, false};
    int n = 0;
    if (i0 < HW) {
      // four mask bytes in one load: pixel_offset and i0 are multiples of 4, and the plane is padded to 256 bytes
      const unsigned four = *reinterpret_cast<const unsigned*>(mk + i0);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int i = i0 + j;
        if (i < HW && ((four >> (8 * j)) & 0xffu)) {
          const int y = i / W, x = i - y * W;
          cand[j] = y >= border && y < H - border && x >= border && x < W - border && ks_score(m, y, x) > threshold;
          n += cand[j] ? 1 : 0;
        }
      }
    }
    int total;
    int pos = C + ks_prefix(n, s_tot[buf], total);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (cand[j]) list[pos++] = i0 + j;                            // pos <= the number of pixels before i0 + j
    C += total;
  }
  __syncthreads();                                                  // the list is read by other threads from here on

  if (C <= k) {
    for (int i = tid; i < C; i += KS_SEL_THREADS) out[i] = list[i];
    if (tid == 0) counts[(int64_t)b * KS_COUNTERS] = C, counts[(int64_t)b * KS_COUNTERS + 1] = C;
    return;
  }

  // the k-th largest bit pattern: four 8-bit digits from the top; s_need: how many are still to be taken among the
  // entries that share the digits found so far
  if (tid == 0) s_prefix = 0u, s_need = k;
  for (int shift = 24; shift >= 0; shift -= 8) {
    if (tid < 256) s_hist[tid] = 0u;
    __syncthreads();
    const unsigned prefix = s_prefix;
    for (int i = tid; i < C; i += KS_SEL_THREADS) {
      const unsigned bits = ks_bits_at(m, v, list[i]);
      if (((unsigned long long)bits >> (shift + 8)) == ((unsigned long long)prefix >> (shift + 8)))
        atomicAdd(&s_hist[(bits >> shift) & 255u], 1u);             // counts only: the sum does not depend on the order
    }
    __syncthreads();
    if (tid == 0) {
      int need = s_need, above = 0, bin = 255;
      for (; bin > 0; --bin) {
        const int h = (int)s_hist[bin];
        if (above + h >= need) break;
        above += h;
      }
      s_prefix = prefix | ((unsigned)bin << shift);
      s_need = need - above;
    }
    __syncthreads();
  }
  const unsigned cut = s_prefix;
  const int ties = s_need < 1 ? 1 : (s_need > k ? k : s_need);      // 1 <= ties <= k by construction
  const int greater = k - ties;

  // entries above the cut go to slots [0, greater), the first `ties` entries at the cut (raster order) behind them
  int g_base = 0, e_base = 0;
  buf = 0;
  for (int c = 0; c < C; c += KS_SEL_THREADS, buf ^= 1) {           // uniform trip count
    const int i = c + tid;
    int idx = 0;
    unsigned bits = 0u;
    if (i < C) idx = list[i], bits = ks_bits_at(m, v, idx);
    const bool gt = i < C && bits > cut, eq = i < C && bits == cut;
    int g_total, e_total;
    const int g_pos = g_base + ks_prefix(gt ? 1 : 0, s_tot[buf], g_total);
    const int e_pos = e_base + ks_prefix(eq ? 1 : 0, s_tot2[buf], e_total);
    const unsigned long long key = ((unsigned long long)bits << 32) | (unsigned long long)(0xffffffffu - (unsigned)idx);
    if (gt && g_pos < greater) s_keys[g_pos] = key;
    if (eq && e_pos < ties) s_keys[greater + e_pos] = key;
    g_base += g_total, e_base += e_total;
  }
  int n = 1;
  while (n < k) n <<= 1;                                            // <= 4096
  for (int i = k + tid; i < n; i += KS_SEL_THREADS) s_keys[i] = 0ull;   // below every key: a candidate's bits are > 0

  // bitonic sort, descending
  for (int size = 2; size <= n; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int t = tid; t < (n >> 1); t += KS_SEL_THREADS) {
        const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
        const bool descending = (lo & size) == 0;
        const unsigned long long x = s_keys[lo], y = s_keys[hi];
        if ((x < y) == descending) s_keys[lo] = y, s_keys[hi] = x;
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < k; i += KS_SEL_THREADS) out[i] = (int32_t)(0xffffffffu - (unsigned)(s_keys[i] & 0xffffffffull));
  if (tid == 0) counts[(int64_t)b * KS_COUNTERS] = C, counts[(int64_t)b * KS_COUNTERS + 1] = k;
}

// One workgroup.  offsets[b] = the kept counts of the maps before b; a count is clamped into [0, k], so the offsets
// are non-decreasing and end at most at n_maps * k.
__global__ __launch_bounds__(KS_SEL_THREADS) void k_ks_scan(const int32_t* __restrict__ counts, int n_maps, int k,
                                                            int32_t* __restrict__ offsets) {
  __shared__ int s_tot[2][KS_SEL_WAVES];
  const int tid = (int)threadIdx.x;
  int base = 0, buf = 0;
  for (int c = 0; c < n_maps; c += KS_SEL_THREADS, buf ^= 1) {      // uniform trip count
    const int b = c + tid;
    int kept = b < n_maps ? counts[(int64_t)b * KS_COUNTERS + 1] : 0;
    kept = kept < 0 ? 0 : (kept > k ? k : kept);
    int total;
    const int at = base + ks_prefix(kept, s_tot[buf], total);
    if (b < n_maps) offsets[b] = at;
    base += total;
  }
  if (tid == 0) offsets[n_maps] = base;
}

__global__ __launch_bounds__(KS_EMIT_WAVES * 64) void k_ks_emit(
    const oetr_keypoint_map* __restrict__ maps, int n_maps, int64_t max_pixels, int64_t total_pixels, int D, int k,
    int cell, const int32_t* __restrict__ sel, const int32_t* __restrict__ counts, const int32_t* __restrict__ offsets,
    float* __restrict__ keypoints, float* __restrict__ scores, float* __restrict__ descriptors) {
  const int b = (int)blockIdx.x, lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const int i = (int)blockIdx.y * KS_EMIT_WAVES + wave;
  if (i >= k) return;                                               // wave-uniform
  const int rows = n_maps * k;                                      // <= INT32_MAX (checked on the host)
  const oetr_keypoint_map m = maps[b];
  const KsView v = ks_view(m, max_pixels, total_pixels);
  int kept = v.ok ? counts[(int64_t)b * KS_COUNTERS + 1] : 0;
  kept = kept < 0 ? 0 : (kept > k ? k : kept);
  int total = offsets[n_maps], first = offsets[b];                  // k_ks_scan's: inside [0, rows]; clamped all the same
  total = total < 0 ? 0 : (total > rows ? rows : total);
  first = first < 0 ? 0 : (first > rows ? rows : first);
  const int slot = b * k + i;
  float2* kpv = reinterpret_cast<float2*>(keypoints);

  if (i < kept && first + i < rows) {                               // wave-uniform
    const int row = first + i;
    int idx = sel[slot];
    idx = (unsigned)idx < (unsigned)v.HW ? idx : 0;
    const int y = idx / v.W, x = idx - y * v.W;
    if (lane == 0) {
      kpv[row] = make_float2((float)x, (float)y);
      scores[row] = ks_score(m, y, x);
    }
    const ks::Taps taps = ks::taps((float)x, (float)y, m.w, m.h, cell);
    float val[KS_MAX_D_PER_LANE];
    float part = 0.0f;                                              // partial `lane` of the 64
#pragma unroll
    for (int j = 0; j < KS_MAX_D_PER_LANE; ++j) {
      const int d = lane + 64 * j;
      val[j] = 0.0f;
      if (d < D) {
        val[j] = ks::interpolate(taps, m.desc + (int64_t)d * m.desc_stride[0], m.desc_stride[1], m.desc_stride[2]);
        part = ks::add_square(part, val[j]);
      }
    }
#pragma unroll
    for (int stride = 32; stride >= 1; stride >>= 1) part = ks::tree_step(part, __shfl_down(part, stride, 64));
    const float norm = ks::norm_of(__shfl(part, 0, 64));
    float* o = descriptors + (int64_t)row * D;
#pragma unroll
    for (int j = 0; j < KS_MAX_D_PER_LANE; ++j) {
      const int d = lane + 64 * j;
      if (d < D) o[d] = val[j] / norm;
    }
  }
  if (slot >= total) {                                              // the tail: disjoint from every kept row
    if (lane == 0) {
      kpv[slot] = make_float2(-1.0f, -1.0f);
      scores[slot] = __int_as_float(0x7fc00000);
    }
    float* o = descriptors + (int64_t)slot * D;
    for (int d = lane; d < D; d += 64) o[d] = 0.0f;
  }
}

namespace {

constexpr const char* ME = "oetr_keypoint_select";
constexpr int64_t KS_MAX_TOTAL_PIXELS = (int64_t)1 << 40;
constexpr int KS_MAX_MAPS = 1 << 21;                                // 1024 threads a map stay below 2^32 threads a launch

bool ks_aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

size_t ks_plane(int64_t total_pixels) { return ((size_t)total_pixels + 255) / 256 * 256; }

}  // namespace
}  // namespace oetr

using namespace oetr;

extern "C" {

int oetr_keypoint_select_abi_version(void) { return OETR_KEYPOINT_SELECT_ABI_VERSION; }

size_t oetr_keypoint_select_workspace_bytes(int64_t total_pixels, int n_maps, int max_keypoints) {
  if (total_pixels < 1 || total_pixels > KS_MAX_TOTAL_PIXELS || n_maps < 1 || n_maps > KS_MAX_MAPS ||
      max_keypoints < 1 || max_keypoints > KS_MAX_K || (int64_t)n_maps * max_keypoints > (int64_t)INT32_MAX)
    return 0;
  // plane A (float), the three byte planes, the selected raster indices
  return ks_plane(total_pixels) * (sizeof(float) + 3) + (size_t)n_maps * (size_t)max_keypoints * sizeof(int32_t);
}

// The host code dereferences none of its pointer arguments and reads nothing from the device.
oetr_status oetr_keypoint_select(const oetr_keypoint_map* maps, int n_maps, int64_t max_pixels, int64_t total_pixels,
                                 int D, int nms_radius, float threshold, int remove_borders, int max_keypoints,
                                 int cell, void* workspace, size_t workspace_bytes, float* keypoints, float* scores,
                                 float* descriptors, int32_t* offsets, int32_t* counts, void* stream) {
  if (!maps || !workspace) return entry_fail(ME, OETR_ERR_BAD_ARG, "NULL maps / workspace pointer");
  if (!keypoints || !scores || !descriptors || !offsets || !counts)
    return entry_fail(ME, OETR_ERR_BAD_ARG, "NULL keypoints / scores / descriptors / offsets / counts output");
  if (n_maps <= 0) return entry_fail(ME, OETR_ERR_BAD_ARG, "need n_maps > 0");
  if (max_pixels < 1 || total_pixels < 1) return entry_fail(ME, OETR_ERR_BAD_ARG, "need max_pixels >= 1 and total_pixels >= 1");
  if (D < OETR_KEYPOINT_SELECT_MIN_D || D > OETR_KEYPOINT_SELECT_MAX_D || D % 4)
    return entry_fail(ME, OETR_ERR_BAD_ARG, "need D % 4 == 0 and 4 <= D <= 512, got " + std::to_string(D));
  if (nms_radius < 0 || nms_radius > OETR_KEYPOINT_SELECT_MAX_RADIUS)
    return entry_fail(ME, OETR_ERR_BAD_ARG, "need 0 <= nms_radius <= 8, got " + std::to_string(nms_radius));
  if (!(threshold >= 0.0f)) return entry_fail(ME, OETR_ERR_BAD_ARG, "need threshold >= 0");
  if (remove_borders < 0) return entry_fail(ME, OETR_ERR_BAD_ARG, "need remove_borders >= 0");
  if (max_keypoints < 1 || max_keypoints > KS_MAX_K)
    return entry_fail(ME, OETR_ERR_BAD_ARG, "need 1 <= max_keypoints <= 4096, got " + std::to_string(max_keypoints));
  if (cell < 1) return entry_fail(ME, OETR_ERR_BAD_ARG, "need cell >= 1");
  if (!ks_aligned(maps, 8) || !ks_aligned(keypoints, 8) || !ks_aligned(scores, 4) || !ks_aligned(descriptors, 4) ||
      !ks_aligned(offsets, 4) || !ks_aligned(counts, 4) || !ks_aligned(workspace, 4))
    return entry_fail(ME, OETR_ERR_BAD_ARG, "maps and keypoints must be 8-byte aligned, the other buffers 4-byte");
  if (max_pixels > (int64_t)KS_MAX_SIDE * KS_MAX_SIDE)
    return entry_fail(ME, OETR_ERR_BAD_SHAPE, "need max_pixels <= 8192 * 8192");
  if (total_pixels > KS_MAX_TOTAL_PIXELS) return entry_fail(ME, OETR_ERR_BAD_SHAPE, "need total_pixels <= 2^40");
  if (n_maps > KS_MAX_MAPS) return entry_fail(ME, OETR_ERR_BAD_SHAPE, "need n_maps <= " + std::to_string(KS_MAX_MAPS));
  if ((int64_t)n_maps * max_keypoints > (int64_t)INT32_MAX)
    return entry_fail(ME, OETR_ERR_BAD_SHAPE, "need n_maps * max_keypoints <= " + std::to_string(INT32_MAX));
  const size_t need = oetr_keypoint_select_workspace_bytes(total_pixels, n_maps, max_keypoints);
  if (workspace_bytes < need)
    return entry_fail(ME, OETR_ERR_WORKSPACE,
                      "workspace of " + std::to_string(workspace_bytes) + " bytes, need " + std::to_string(need));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t plane = ks_plane(total_pixels);
  float* A = static_cast<float*>(workspace);
  uint8_t* M = reinterpret_cast<uint8_t*>(A + plane);
  uint8_t* Bm = M + plane;
  uint8_t* supp = Bm + plane;
  int32_t* sel = reinterpret_cast<int32_t*>(supp + plane);
  const int k = max_keypoints, r = nms_radius;
  const dim3 nms_grid((unsigned)n_maps, (unsigned)((max_pixels + KS_PIX_PER_BLOCK - 1) / KS_PIX_PER_BLOCK));   // y <= 32768
#define KS_NMS(PASS)                                                                                                   \
  hipLaunchKernelGGL(k_ks_nms<PASS>, nms_grid, dim3(KS_THREADS), 0, s, maps, max_pixels, total_pixels, r, A, M, Bm, supp); \
  if (oetr_status rc = entry_hip(ME, hipGetLastError(), "k_ks_nms")) return rc
  KS_NMS(0);
  KS_NMS(1);
  for (int round = 0; round < 2; ++round) {
    KS_NMS(2);
    KS_NMS(3);
    KS_NMS(4);
    KS_NMS(5);
  }
#undef KS_NMS
  hipLaunchKernelGGL(k_ks_select, dim3((unsigned)n_maps), dim3(KS_SEL_THREADS), 0, s, maps, max_pixels, total_pixels,
                     threshold, remove_borders, k, A, M, sel, counts);
  if (oetr_status rc = entry_hip(ME, hipGetLastError(), "k_ks_select")) return rc;
  hipLaunchKernelGGL(k_ks_scan, dim3(1), dim3(KS_SEL_THREADS), 0, s, counts, n_maps, k, offsets);
  if (oetr_status rc = entry_hip(ME, hipGetLastError(), "k_ks_scan")) return rc;
  hipLaunchKernelGGL(k_ks_emit, dim3((unsigned)n_maps, (unsigned)((k + KS_EMIT_WAVES - 1) / KS_EMIT_WAVES)),
                     dim3(KS_EMIT_WAVES * 64), 0, s, maps, n_maps, max_pixels, total_pixels, D, k, cell, sel, counts,
                     offsets, keypoints, scores, descriptors);
  return entry_hip(ME, hipGetLastError(), "k_ks_emit");
}

}  // extern "C"
