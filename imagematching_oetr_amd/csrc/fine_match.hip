// Refining dense matches to sub-pixel (include/oetr_fine_match.h): the match list and fine windows of a dual-softmax
// result, and the expectation head on the windows - the two device stages that bracket the fine network.  The head is
// bit for bit the numpy program tests/fine_match_oracle.py (fine_match_math.h is its one C++ copy).
//
// oetr_fine_windows, four launches ordered by the launch boundary alone (no workgroup waits on another, no atomics):
//   k_fw_count    one workgroup per pair: its matches -> workspace[p] (-1: the pair is not vouched for).
//   k_fw_scan     ONE workgroup: exclusive scan of the counts into moffsets, saturated at the capacity (chunks of 1024
//                 pairs, a running base carried across chunks), and both counters of every pair.
//   k_fw_emit     one workgroup per pair walks the pair's rows of side 0 in order, 1024 at a time: the 64-bit ballot of
//                 "matched" with a popcount prefix inside the wave, wave totals through LDS, a running base across
//                 chunks - so list row = moffsets[p] + (number of matches before it), decided by arithmetic.  This is
//                 match_assembly.hip's walk, restated here, not shared: that file is left untouched.
//   k_fw_gather   the window copy, a grid-stride loop over ALL M_cap list rows: 16, 32 or 64 lanes own a window row of
//                 C floats and move it with 16-byte loads and stores; a list row from moffsets[P] on gets -1 and +0
//                 windows from the same loop, so every row is written exactly once and there is no clearing launch.
// oetr_fine_refine, three launches:
//   k_fr_copy     keypoints1_f = keypoints1.
//   k_fr_head     a grid-stride loop of one workgroup per list row: 16 lanes own a window row of win1 and its dot
//                 product with the centre row of win0 - lane l is the specification's partial l, four shuffle levels
//                 are its tree; wave 0 then does the softmax, five serial sums are five lanes' work (Z on every lane,
//                 the four moments on lanes 0 .. 3), and lane 0 writes the row and the refined keypoint.
//   k_fr_count    one workgroup per pair: the counters.
//
// Nothing is dereferenced on the strength of device data alone: fm_range clamps the offsets into [0, n], a pair that
// is not vouched for is left before any of its rows is read, a match index passes ONE unsigned compare against S
// before it is kept, every entry of a list row passes one before it forms an address, and a fine token is read only
// inside its grid, which multiplies to the clamped row count.
#include <cmath>
#include <string>

#include "../../include/oetr_fine_match.h"
#include "common.h"
#include "fine_match_math.h"

namespace oetr {

constexpr int FM_THREADS = 1024;           // k_fw_count, k_fw_emit, k_fw_scan: match_assembly.hip's choice
constexpr int FM_WAVES = FM_THREADS / 64;
constexpr int FM_ROW_THREADS = 256;        // k_fw_gather, k_fr_head: one list row per workgroup and step
constexpr int FM_MAX_GROUPS = 16384;       // of the two grid-stride loops over the list
constexpr int FM_WCOUNTERS = OETR_FINE_MATCH_WINDOW_COUNTERS;
constexpr int FM_COUNTERS = OETR_FINE_MATCH_COUNTERS;
constexpr int FM_MAX_WW = OETR_FINE_MATCH_MAX_W * OETR_FINE_MATCH_MAX_W;
static_assert(FM_MAX_WW <= 64, "one wave holds a window's positions");
static_assert(fm::PARTIALS == 16, "16 lanes own a window row");

struct FmRange {
  int s, e;
};

// rows off[p] .. off[p+1]-1, clamped: 0 <= s <= e <= n whatever the device holds
__device__ __forceinline__ FmRange fm_range(const int32_t* __restrict__ off, int p, int n) {
  int s = off[p], e = off[p + 1];
  s = s < 0 ? 0 : (s > n ? n : s);
  e = e < s ? s : (e > n ? n : e);
  return {s, e};
}

struct FmGrid {
  int h, w;
};

__device__ __forceinline__ FmGrid fm_grid(const int32_t* __restrict__ grids, int p) {
  return {grids[2 * (size_t)p], grids[2 * (size_t)p + 1]};
}

__device__ __forceinline__ bool fm_multiplies(FmGrid g, FmRange r) {
  return g.h >= 0 && g.w >= 0 && (int64_t)g.h * g.w == (int64_t)(r.e - r.s);
}

// what oetr_fine_windows knows of the sides
struct FmSides {
  const int32_t* off[2];
  const int32_t* grids[2];
  const int32_t* foff[2];
  const int32_t* fgrids[2];
  int n_tok[2], n_fine[2];
  int n_pairs, max_k0;
};

struct FmPair {
  FmRange r[2], f[2];
  FmGrid g[2], fg[2];
  bool ok;                                 // vouched for
};

__device__ __forceinline__ FmPair fm_pair(const FmSides& a, int p) {
  FmPair q;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    q.r[i] = fm_range(a.off[i], p, a.n_tok[i]);
    q.f[i] = fm_range(a.foff[i], p, a.n_fine[i]);
    q.g[i] = fm_grid(a.grids[i], p);
    q.fg[i] = fm_grid(a.fgrids[i], p);
  }
  q.ok = q.r[0].e - q.r[0].s <= a.max_k0 && fm_multiplies(q.g[0], q.r[0]) && fm_multiplies(q.g[1], q.r[1]) &&
         fm_multiplies(q.fg[0], q.f[0]) && fm_multiplies(q.fg[1], q.f[1]);
  return q;
}

// 0 <= v < K1 as one unsigned compare (K1 >= 0)
__device__ __forceinline__ bool fm_matched(int v, int K1) { return (unsigned)v < (unsigned)K1; }

__device__ __forceinline__ int fm_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

__global__ __launch_bounds__(FM_THREADS) void k_fw_count(const FmSides a, const int32_t* __restrict__ matches0,
                                                         int32_t* __restrict__ matched_ws) {
  __shared__ int s_n[FM_WAVES];
  const int p = (int)blockIdx.x, tid = (int)threadIdx.x;
  const FmPair q = fm_pair(a, p);
  if (!q.ok) {                                                      // uniform: none of its rows is read
    if (tid == 0) matched_ws[p] = -1;
    return;
  }
  const int K1 = q.r[1].e - q.r[1].s;
  int n = 0;
  for (int64_t r = (int64_t)q.r[0].s + tid; r < (int64_t)q.r[0].e; r += FM_THREADS)   // 64-bit: e may be INT32_MAX
    n += fm_matched(matches0[r], K1) ? 1 : 0;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) n += __shfl_xor(n, d, 64);
  if ((tid & 63) == 0) s_n[tid >> 6] = n;
  __syncthreads();
  if (tid == 0) {
    n = 0;
#pragma unroll
    for (int w = 0; w < FM_WAVES; ++w) n += s_n[w];
    matched_ws[p] = n;
  }
}

// One workgroup.  moffsets[p] = min(sum of matched[0..p), cap): saturated in 64 bits, so non-decreasing and inside the
// list whatever the inputs were; kept[p] = moffsets[p+1] - moffsets[p].
__global__ __launch_bounds__(FM_THREADS) void k_fw_scan(const int32_t* __restrict__ matched_ws, int n_pairs, int cap,
                                                        int32_t* __restrict__ moffsets, int32_t* __restrict__ counts) {
  __shared__ long long s_sum[2][FM_WAVES];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  long long base = 0;
  int buf = 0;
  for (int c = 0; c < n_pairs; c += FM_THREADS, buf ^= 1) {         // uniform trip count
    const int p = c + tid;                                          // <= INT32_MAX / 3 + 1023
    const bool active = p < n_pairs;
    const int matched = active ? matched_ws[p] : 0;
    const long long k = matched > 0 ? (long long)matched : 0;
    long long incl = k;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const long long up = __shfl_up(incl, d, 64);
      if (lane >= d) incl += up;
    }
    if (lane == 63) s_sum[buf][wave] = incl;
    __syncthreads();                                                // two buffers: one barrier per chunk
    long long before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < FM_WAVES; ++w) {
      const long long t = s_sum[buf][w];
      if (w < wave) before += t;
      total += t;
    }
    if (active) {
      const long long at = base + before + incl - k, end = at + k;
      const int lo = (int)(at < (long long)cap ? at : (long long)cap);
      const int hi = (int)(end < (long long)cap ? end : (long long)cap);
      moffsets[p] = lo;
      counts[(size_t)p * FM_WCOUNTERS] = matched < 0 ? -1 : matched;
      counts[(size_t)p * FM_WCOUNTERS + 1] = matched < 0 ? -1 : hi - lo;
    }
    base += total;
  }
  if (tid == 0) moffsets[n_pairs] = (int32_t)(base < (long long)cap ? base : (long long)cap);
}

__global__ __launch_bounds__(FM_THREADS) void k_fw_emit(const FmSides a, const int32_t* __restrict__ matches0, int cap,
                                                        const int32_t* __restrict__ moffsets,
                                                        int32_t* __restrict__ rows) {
  __shared__ int s_tot[2][FM_WAVES];
  const int p = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const FmPair q = fm_pair(a, p);
  if (!q.ok) return;                                                // uniform: before any barrier
  const int K0 = q.r[0].e - q.r[0].s, K1 = q.r[1].e - q.r[1].s;
  unsigned base = (unsigned)fm_clamp(moffsets[p], cap);             // k_fw_scan's: inside [0, cap]; clamped all the same
  int buf = 0;
  for (int c = 0; c < K0 && base < (unsigned)cap; c += FM_THREADS, buf ^= 1) {   // uniform; base + K0 < 2^32
    const int i = c + tid;                                          // K0 <= INT32_MAX: c + tid may wrap, then i < 0
    const bool in = i >= 0 && i < K0;
    const int v = in ? matches0[(size_t)q.r[0].s + (size_t)i] : -1;
    const bool keep = in && fm_matched(v, K1);
    const unsigned long long kb = __ballot(keep);
    if (lane == 0) s_tot[buf][wave] = __popcll(kb);
    __syncthreads();                                                // two buffers: one barrier per chunk
    unsigned before = 0, chunk = 0;
#pragma unroll
    for (int w = 0; w < FM_WAVES; ++w) {
      const unsigned t = (unsigned)s_tot[buf][w];
      if (w < wave) before += t;
      chunk += t;
    }
    if (keep) {
      const unsigned dst = base + before + (unsigned)__popcll(kb & ((1ull << lane) - 1ull));
      if (dst < (unsigned)cap) {                                    // else: dropped, and counted by k_fw_scan
        int32_t* row = rows + (size_t)dst * 3;
        row[0] = p, row[1] = i, row[2] = v;
      }
    }
    base += chunk;
    if (c > INT32_MAX - FM_THREADS) break;                          // uniform: the next c would wrap
  }
}

// A list row as the launches after k_fw_emit read it: every entry passes one unsigned compare.
struct FmRow {
  int p, a, j;
};

__device__ __forceinline__ FmRow fm_row(const int32_t* __restrict__ rows, int64_t m) {
  const int32_t* row = rows + (size_t)m * 3;
  return {row[0], row[1], row[2]};
}

__global__ __launch_bounds__(FM_ROW_THREADS) void k_fw_gather(const FmSides a, const float* __restrict__ fine0,
                                                              const float* __restrict__ fine1, int C4, int W, int stride,
                                                              int cap, int lpr_shift,
                                                              const int32_t* __restrict__ moffsets,
                                                              int32_t* __restrict__ rows, float* __restrict__ win0,
                                                              float* __restrict__ win1) {
  const int tid = (int)threadIdx.x, WW = W * W;
  const int lpr = 1 << lpr_shift, l = tid & (lpr - 1), unit = tid >> lpr_shift, units = FM_ROW_THREADS >> lpr_shift;
  const int total = fm_clamp(moffsets[a.n_pairs], cap);
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int m = (int)blockIdx.x; m < cap; m += (int)gridDim.x) {     // cap * WW <= INT32_MAX
    bool live = m < total;                                          // uniform
    FmRow t = {-1, 0, 0};
    // per side: the coarse grid's width, the fine grid and its first row (scalars: a record indexed by the side at
    // run time would live in scratch memory)
    int gw0 = 1, gw1 = 1, fh0 = 0, fh1 = 0, fw0 = 0, fw1 = 0, first0 = 0, first1 = 0;
    if (live) {
      t = fm_row(rows, m);
      live = (unsigned)t.p < (unsigned)a.n_pairs;
      if (live) {
        const FmPair q = fm_pair(a, t.p);
        live = q.ok && (unsigned)t.a < (unsigned)(q.r[0].e - q.r[0].s) && (unsigned)t.j < (unsigned)(q.r[1].e - q.r[1].s);
        gw0 = q.g[0].w, gw1 = q.g[1].w;                             // g.h * g.w == K > token >= 0: g.w >= 1
        fh0 = q.fg[0].h, fw0 = q.fg[0].w, fh1 = q.fg[1].h, fw1 = q.fg[1].w;
        first0 = q.f[0].s, first1 = q.f[1].s;
      }
    } else if (tid < 3) {
      rows[(size_t)m * 3 + tid] = -1;                               // past the list
    }
    for (int u = unit; u < 2 * WW; u += units) {
      const int side = u >= WW ? 1 : 0, r = u - side * WW;
      const int ky = r / W, kx = r - ky * W;
      const float4* src = nullptr;
      if (live) {
        const int gw = side ? gw1 : gw0, fh = side ? fh1 : fh0, fw = side ? fw1 : fw0;
        const int token = side ? t.j : t.a, first = side ? first1 : first0;
        const int row = token / gw, col = token - row * gw;
        const int64_t fy = (int64_t)row * stride + ky - W / 2, fx = (int64_t)col * stride + kx - W / 2;
        if (fy >= 0 && fy < (int64_t)fh && fx >= 0 && fx < (int64_t)fw)   // fy * fw + fx < fh * fw == its fine rows
          src = reinterpret_cast<const float4*>((side ? fine1 : fine0) +
                                                ((size_t)first + (size_t)(fy * fw + fx)) * (size_t)(4 * C4));
      }
      float4* dst = reinterpret_cast<float4*>((side ? win1 : win0) + ((size_t)m * WW + r) * (size_t)(4 * C4));
      for (int c = l; c < C4; c += lpr) {
        float4 v = zero;
        if (src) v = src[c];
        dst[c] = v;
      }
    }
  }
}

__global__ __launch_bounds__(FM_ROW_THREADS) void k_fr_copy(const float2* __restrict__ kp1, int n1,
                                                            float2* __restrict__ kp1f) {
  const int64_t step = (int64_t)gridDim.x * FM_ROW_THREADS;
  for (int64_t r = (int64_t)blockIdx.x * FM_ROW_THREADS + threadIdx.x; r < (int64_t)n1; r += step) kp1f[r] = kp1[r];
}

__global__ __launch_bounds__(FM_ROW_THREADS) void k_fr_head(
    const float* __restrict__ win0, const float* __restrict__ win1, const int32_t* __restrict__ rows,
    const int32_t* __restrict__ moffsets, int n_pairs, int cap, const float2* __restrict__ kp0,
    const int32_t* __restrict__ off0, int n0, const float2* __restrict__ kp1, const int32_t* __restrict__ off1, int n1,
    int C4, int W, float scale, float radius, float* __restrict__ expec, float2* __restrict__ mkpts0,
    float2* __restrict__ mkpts1, float2* __restrict__ kp1f) {
  __shared__ float s_s[64], s_q[64], s_heat[64], s_mom[4];
  const int tid = (int)threadIdx.x, WW = W * W, l = tid & 15, group = tid >> 4;
  const int total = fm_clamp(moffsets[n_pairs], cap);
  const float2 nan2 = make_float2(NAN, NAN);
  for (int m = (int)blockIdx.x; m < cap; m += (int)gridDim.x) {
    bool live = m < total;                                          // uniform, as everything below that decides a path
    FmRow t = {-1, 0, 0};
    FmRange r0 = {0, 0}, r1 = {0, 0};
    if (live) {
      t = fm_row(rows, m);
      live = (unsigned)t.p < (unsigned)n_pairs;
      if (live) {
        r0 = fm_range(off0, t.p, n0), r1 = fm_range(off1, t.p, n1);
        live = (unsigned)t.a < (unsigned)(r0.e - r0.s) && (unsigned)t.j < (unsigned)(r1.e - r1.s);
      }
    }
    if (!live) {                                                    // past the list, or a row nobody could have listed
      if (tid == 0) {
        expec[(size_t)m * 3] = expec[(size_t)m * 3 + 1] = expec[(size_t)m * 3 + 2] = NAN;
        mkpts0[m] = mkpts1[m] = nan2;
      }
      continue;
    }
    const float4* centre = reinterpret_cast<const float4*>(win0 + ((size_t)m * WW + WW / 2) * (size_t)(4 * C4));
    for (int r = group; r < WW; r += FM_ROW_THREADS / 16) {
      const float4* row = reinterpret_cast<const float4*>(win1 + ((size_t)m * WW + r) * (size_t)(4 * C4));
      float acc = 0.0f;                                             // partial l: its channels in ascending c
      for (int c = l; c < C4; c += 16) {
        const float4 x = centre[c], y = row[c];
        acc = fm::chain4(acc, x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w);
      }
#pragma unroll
      for (int d = 1; d < 16; d <<= 1) acc = fm::tree_node(acc, __shfl_xor(acc, d, 64));   // adjacent pairs
      if (l == 0) s_s[r] = acc;
    }
    __syncthreads();
    bool has = false;
    if (tid < 64) {
      const float tt = tid < WW ? fm::t_of(s_s[tid], scale) : NAN;
      float mx = fm::max_push(-INFINITY, tt);
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) {
        const float other = __shfl_xor(mx, d, 64);
        mx = other > mx ? other : mx;
      }
      has = mx > -INFINITY;                                         // a candidate is finite
      s_q[tid] = has ? fm::q_of(tt, mx) : 0.0f;
    }
    __syncthreads();
    if (tid < 64) {
      const float Z = fm::sum_q(s_q, WW);                           // every lane: the same serial sum
      s_heat[tid] = has && tid < WW ? fm::heat_of(s_q[tid], Z) : 0.0f;
    }
    __syncthreads();
    if (tid < 4) s_mom[tid] = fm::moment(s_heat, W, tid);
    __syncthreads();
    if (tid == 0) {
      const fm::Expec e = has ? fm::finish(s_mom[0], s_mom[1], s_mom[2], s_mom[3]) : fm::none();
      expec[(size_t)m * 3] = e.x, expec[(size_t)m * 3 + 1] = e.y, expec[(size_t)m * 3 + 2] = e.sd;
      const float2 k1 = kp1[(size_t)r1.s + (size_t)t.j];
      const float2 fine = make_float2(fm::refined(k1.x, e.x, radius), fm::refined(k1.y, e.y, radius));
      mkpts0[m] = kp0[(size_t)r0.s + (size_t)t.a];
      mkpts1[m] = fine;
      kp1f[(size_t)r1.s + (size_t)t.j] = fine;
    }
  }
}

__global__ __launch_bounds__(FM_ROW_THREADS) void k_fr_count(const int32_t* __restrict__ moffsets,
                                                             const int32_t* __restrict__ wcounts, int cap,
                                                             const float* __restrict__ expec,
                                                             int32_t* __restrict__ counts) {
  __shared__ int s_n[FM_ROW_THREADS / 64];
  const int p = (int)blockIdx.x, tid = (int)threadIdx.x;
  int32_t* c = counts + (size_t)p * FM_COUNTERS;
  const int matched = wcounts[(size_t)p * FM_WCOUNTERS], kept = wcounts[(size_t)p * FM_WCOUNTERS + 1];
  if (matched < 0) {                                                // uniform: the pair was not vouched for
    if (tid == 0) c[0] = c[1] = c[2] = -1;
    return;
  }
  const FmRange r = fm_range(moffsets, p, cap);
  int n = 0;
  for (int m = r.s + tid; m < r.e; m += FM_ROW_THREADS) n += expec[(size_t)m * 3 + 2] != expec[(size_t)m * 3 + 2] ? 1 : 0;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) n += __shfl_xor(n, d, 64);
  if ((tid & 63) == 0) s_n[tid >> 6] = n;
  __syncthreads();
  if (tid == 0) {
    n = 0;
#pragma unroll
    for (int w = 0; w < FM_ROW_THREADS / 64; ++w) n += s_n[w];
    c[0] = matched, c[1] = kept, c[2] = n;
  }
}

namespace {

constexpr const char* WINDOWS = "oetr_fine_windows";
constexpr const char* REFINE = "oetr_fine_refine";

bool fm_aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// what both entries refuse alike; "" = nothing
std::string fm_bad_sizes(int C, int W) {
  if (W != 3 && W != 5 && W != 7) return "need W in {3, 5, 7}, got " + std::to_string(W);
  if (C < OETR_FINE_MATCH_MIN_C || C > OETR_FINE_MATCH_MAX_C || C % 4 != 0)
    return "need C % 4 == 0 and 4 <= C <= 512, got " + std::to_string(C);
  return "";
}

unsigned fm_list_groups(int64_t cap) { return (unsigned)(cap > FM_MAX_GROUPS ? FM_MAX_GROUPS : cap); }

}  // namespace
}  // namespace oetr

using namespace oetr;

extern "C" {

int oetr_fine_match_abi_version(void) { return OETR_FINE_MATCH_ABI_VERSION; }

size_t oetr_fine_match_workspace_bytes(int n_pairs) {
  if (n_pairs < 1) return 0;
  return (((size_t)n_pairs * sizeof(int32_t)) + 255) / 256 * 256;
}

// The host code dereferences none of its pointer arguments and reads nothing from the device.
oetr_status oetr_fine_windows(const int32_t* matches0, const int32_t* off0, const int32_t* off1, const int32_t* grids0,
                              const int32_t* grids1, int64_t n_tok0, int64_t n_tok1, int n_pairs, int max_k0,
                              const float* fine0, const int32_t* foff0, const int32_t* fgrids0, int64_t n_fine0,
                              const float* fine1, const int32_t* foff1, const int32_t* fgrids1, int64_t n_fine1, int C,
                              int W, int stride, int64_t max_matches, void* workspace, size_t workspace_bytes,
                              int32_t* rows, int32_t* moffsets, int32_t* counts, float* win0, float* win1,
                              void* stream) {
  const char* ME = WINDOWS;
  if (!off0 || !off1 || !grids0 || !grids1)
    return entry_fail(ME, OETR_ERR_BAD_ARG, "NULL off0 / off1 / grids0 / grids1 pointer");
  if (!foff0 || !foff1 || !fgrids0 || !fgrids1)
    return entry_fail(ME, OETR_ERR_BAD_ARG, "NULL foff0 / foff1 / fgrids0 / fgrids1 pointer");
  if (!moffsets || !counts) return entry_fail(ME, OETR_ERR_BAD_ARG, "NULL moffsets / counts output");
  if (!workspace) return entry_fail(ME, OETR_ERR_BAD_ARG, "NULL workspace");
  if (n_pairs <= 0) return entry_fail(ME, OETR_ERR_BAD_ARG, "need n_pairs > 0");
  if (n_tok0 < 0 || n_tok1 < 0 || n_fine0 < 0 || n_fine1 < 0)
    return entry_fail(ME, OETR_ERR_BAD_ARG, "need n_tok0, n_tok1, n_fine0, n_fine1 >= 0");
  if (max_k0 < 0) return entry_fail(ME, OETR_ERR_BAD_ARG, "need max_k0 >= 0");
  if (max_matches < 0) return entry_fail(ME, OETR_ERR_BAD_ARG, "need max_matches >= 0");
  if (const std::string bad = fm_bad_sizes(C, W); !bad.empty()) return entry_fail(ME, OETR_ERR_BAD_ARG, bad);
  if (stride < 1 || stride > OETR_FINE_MATCH_MAX_STRIDE)
    return entry_fail(ME, OETR_ERR_BAD_ARG, "need 1 <= stride <= 8, got " + std::to_string(stride));
  if (n_tok0 != 0 && !matches0) return entry_fail(ME, OETR_ERR_BAD_ARG, "NULL matches0 pointer");
  if ((n_fine0 != 0 && !fine0) || (n_fine1 != 0 && !fine1))
    return entry_fail(ME, OETR_ERR_BAD_ARG, "NULL fine0 / fine1 pointer");
  if (max_matches != 0 && (!rows || !win0 || !win1))
    return entry_fail(ME, OETR_ERR_BAD_ARG, "NULL rows / win0 / win1 output");
  if (!fm_aligned(fine0, 16) || !fm_aligned(fine1, 16) || !fm_aligned(win0, 16) || !fm_aligned(win1, 16))
    return entry_fail(ME, OETR_ERR_BAD_ARG, "fine0 / fine1 / win0 / win1 rows must be 16-byte aligned");
  if (!fm_aligned(matches0, 4) || !fm_aligned(off0, 4) || !fm_aligned(off1, 4) || !fm_aligned(grids0, 4) ||
      !fm_aligned(grids1, 4) || !fm_aligned(foff0, 4) || !fm_aligned(foff1, 4) || !fm_aligned(fgrids0, 4) ||
      !fm_aligned(fgrids1, 4) || !fm_aligned(workspace, 4) || !fm_aligned(rows, 4) || !fm_aligned(moffsets, 4) ||
      !fm_aligned(counts, 4))
    return entry_fail(ME, OETR_ERR_BAD_ARG, "matches0 / offsets / grids / workspace / rows / moffsets / counts must be "
                                            "4-byte aligned");
  if (n_pairs > INT32_MAX / FM_COUNTERS)
    return entry_fail(ME, OETR_ERR_BAD_SHAPE, "need n_pairs <= " + std::to_string(INT32_MAX / FM_COUNTERS));
  if (n_tok0 > (int64_t)INT32_MAX || n_tok1 > (int64_t)INT32_MAX || n_fine0 > (int64_t)INT32_MAX ||
      n_fine1 > (int64_t)INT32_MAX)
    return entry_fail(ME, OETR_ERR_BAD_SHAPE, "need n_tok0, n_tok1, n_fine0, n_fine1 <= " + std::to_string(INT32_MAX) +
                                              " (the offsets are int32)");
  if (max_matches > (int64_t)(INT32_MAX / (W * W)))
    return entry_fail(ME, OETR_ERR_BAD_SHAPE, "need max_matches <= " + std::to_string(INT32_MAX / (W * W)) +
                                              " (INT32_MAX / (W * W)); split the call");
  if (workspace_bytes < oetr_fine_match_workspace_bytes(n_pairs))
    return entry_fail(ME, OETR_ERR_WORKSPACE, "workspace of " + std::to_string(workspace_bytes) + " bytes, need " +
                                              std::to_string(oetr_fine_match_workspace_bytes(n_pairs)));
  hipStream_t s = static_cast<hipStream_t>(stream);
  FmSides a;
  a.off[0] = off0, a.off[1] = off1;
  a.grids[0] = grids0, a.grids[1] = grids1;
  a.foff[0] = foff0, a.foff[1] = foff1;
  a.fgrids[0] = fgrids0, a.fgrids[1] = fgrids1;
  a.n_tok[0] = (int)n_tok0, a.n_tok[1] = (int)n_tok1;
  a.n_fine[0] = (int)n_fine0, a.n_fine[1] = (int)n_fine1;
  a.n_pairs = n_pairs, a.max_k0 = max_k0;
  const int cap = (int)max_matches;
  int32_t* matched_ws = static_cast<int32_t*>(workspace);
  hipLaunchKernelGGL(k_fw_count, dim3((unsigned)n_pairs), dim3(FM_THREADS), 0, s, a, matches0, matched_ws);
  if (oetr_status rc = entry_hip(ME, hipGetLastError(), "k_fw_count")) return rc;
  hipLaunchKernelGGL(k_fw_scan, dim3(1), dim3(FM_THREADS), 0, s, matched_ws, n_pairs, cap, moffsets, counts);
  if (oetr_status rc = entry_hip(ME, hipGetLastError(), "k_fw_scan")) return rc;
  if (cap == 0) return OETR_OK;                                     // no list row to write
  hipLaunchKernelGGL(k_fw_emit, dim3((unsigned)n_pairs), dim3(FM_THREADS), 0, s, a, matches0, cap, moffsets, rows);
  if (oetr_status rc = entry_hip(ME, hipGetLastError(), "k_fw_emit")) return rc;
  const int C4 = C / 4;
  const int lpr_shift = C4 <= 16 ? 4 : (C4 <= 32 ? 5 : 6);          // 16 lanes, a half-wave or a wave per window row
  hipLaunchKernelGGL(k_fw_gather, dim3(fm_list_groups(max_matches)), dim3(FM_ROW_THREADS), 0, s, a, fine0, fine1, C4, W,
                     stride, cap, lpr_shift, moffsets, rows, win0, win1);
  return entry_hip(ME, hipGetLastError(), "k_fw_gather");
}

oetr_status oetr_fine_refine(const float* win0, const float* win1, const int32_t* rows, const int32_t* moffsets,
                             const int32_t* wcounts, int n_pairs, int64_t max_matches, const float* keypoints0,
                             const int32_t* off0, int64_t n_tok0, const float* keypoints1, const int32_t* off1,
                             int64_t n_tok1, int C, int W, float fine_cell, float* expec, float* mkpts0, float* mkpts1,
                             float* keypoints1_f, int32_t* counts, void* stream) {
  const char* ME = REFINE;
  if (!moffsets || !wcounts || !off0 || !off1)
    return entry_fail(ME, OETR_ERR_BAD_ARG, "NULL moffsets / wcounts / off0 / off1 pointer");
  if (!counts) return entry_fail(ME, OETR_ERR_BAD_ARG, "NULL counts output");
  if (n_pairs <= 0) return entry_fail(ME, OETR_ERR_BAD_ARG, "need n_pairs > 0");
  if (n_tok0 < 0 || n_tok1 < 0) return entry_fail(ME, OETR_ERR_BAD_ARG, "need n_tok0 >= 0 and n_tok1 >= 0");
  if (max_matches < 0) return entry_fail(ME, OETR_ERR_BAD_ARG, "need max_matches >= 0");
  if (const std::string bad = fm_bad_sizes(C, W); !bad.empty()) return entry_fail(ME, OETR_ERR_BAD_ARG, bad);
  if (!std::isfinite(fine_cell) || !(fine_cell > 0.0f))
    return entry_fail(ME, OETR_ERR_BAD_ARG, "need a finite fine_cell > 0, got " + std::to_string(fine_cell));
  if (max_matches != 0 && (!rows || !win0 || !win1 || !expec || !mkpts0 || !mkpts1))
    return entry_fail(ME, OETR_ERR_BAD_ARG, "NULL rows / win0 / win1 / expec / mkpts0 / mkpts1 pointer");
  if (n_tok0 != 0 && !keypoints0) return entry_fail(ME, OETR_ERR_BAD_ARG, "NULL keypoints0 pointer");
  if (n_tok1 != 0 && (!keypoints1 || !keypoints1_f))
    return entry_fail(ME, OETR_ERR_BAD_ARG, "NULL keypoints1 / keypoints1_f pointer");
  if (!fm_aligned(win0, 16) || !fm_aligned(win1, 16))
    return entry_fail(ME, OETR_ERR_BAD_ARG, "win0 / win1 rows must be 16-byte aligned");
  if (!fm_aligned(keypoints0, 8) || !fm_aligned(keypoints1, 8) || !fm_aligned(keypoints1_f, 8) ||
      !fm_aligned(mkpts0, 8) || !fm_aligned(mkpts1, 8))
    return entry_fail(ME, OETR_ERR_BAD_ARG, "keypoints0 / keypoints1 / keypoints1_f / mkpts0 / mkpts1 must be 8-byte aligned");
  if (!fm_aligned(rows, 4) || !fm_aligned(moffsets, 4) || !fm_aligned(wcounts, 4) || !fm_aligned(off0, 4) ||
      !fm_aligned(off1, 4) || !fm_aligned(expec, 4) || !fm_aligned(counts, 4))
    return entry_fail(ME, OETR_ERR_BAD_ARG, "rows / moffsets / wcounts / off0 / off1 / expec / counts must be 4-byte aligned");
  if (n_pairs > INT32_MAX / FM_COUNTERS)
    return entry_fail(ME, OETR_ERR_BAD_SHAPE, "need n_pairs <= " + std::to_string(INT32_MAX / FM_COUNTERS));
  if (n_tok0 > (int64_t)INT32_MAX || n_tok1 > (int64_t)INT32_MAX)
    return entry_fail(ME, OETR_ERR_BAD_SHAPE, "need n_tok0, n_tok1 <= " + std::to_string(INT32_MAX) + " (the offsets are int32)");
  if (max_matches > (int64_t)(INT32_MAX / (W * W)))
    return entry_fail(ME, OETR_ERR_BAD_SHAPE, "need max_matches <= " + std::to_string(INT32_MAX / (W * W)) +
                                              " (INT32_MAX / (W * W)); split the call");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int cap = (int)max_matches, n0 = (int)n_tok0, n1 = (int)n_tok1;
  const int64_t copy_groups = (n_tok1 + FM_ROW_THREADS - 1) / FM_ROW_THREADS;
  if (n1 > 0) {
    hipLaunchKernelGGL(k_fr_copy, dim3((unsigned)(copy_groups > 4096 ? 4096 : copy_groups)), dim3(FM_ROW_THREADS), 0, s,
                       reinterpret_cast<const float2*>(keypoints1), n1, reinterpret_cast<float2*>(keypoints1_f));
    if (oetr_status rc = entry_hip(ME, hipGetLastError(), "k_fr_copy")) return rc;
  }
  if (cap > 0) {
    hipLaunchKernelGGL(k_fr_head, dim3(fm_list_groups(max_matches)), dim3(FM_ROW_THREADS), 0, s, win0, win1, rows,
                       moffsets, n_pairs, cap, reinterpret_cast<const float2*>(keypoints0), off0, n0,
                       reinterpret_cast<const float2*>(keypoints1), off1, n1, C / 4, W, fm::scale_of(C),
                       fm::radius_of(W, fine_cell), expec, reinterpret_cast<float2*>(mkpts0),
                       reinterpret_cast<float2*>(mkpts1), reinterpret_cast<float2*>(keypoints1_f));
    if (oetr_status rc = entry_hip(ME, hipGetLastError(), "k_fr_head")) return rc;
  }
  hipLaunchKernelGGL(k_fr_count, dim3((unsigned)n_pairs), dim3(FM_ROW_THREADS), 0, s, moffsets, wcounts, cap, expec,
                     counts);
  return entry_hip(ME, hipGetLastError(), "k_fr_count");
}

}  // extern "C"
