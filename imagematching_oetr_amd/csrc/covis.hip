// Co-visibility boxes (include/oetr_covis.h): the reference's numpy_overlap_box (src/datasets/utils.py:140-202)
// for a batch of pairs - ground-truth overlap boxes, inlier counts and masks from depth maps, intrinsics and poses.
//
// k_covis_warp streams depth map 1: a workgroup of 256 threads takes COVIS_PIX consecutive pixels of one pair (a
// strip of rows; consecutive lanes read consecutive floats), each thread COVIS_PER_THREAD of them, all loads issued
// before the arithmetic.  A pixel with depth is un-projected, transformed, projected, truncated and depth-tested in
// float64 with every operation rounded on its own, in the reference's order (no contraction into FMAs: trunc() and
// "< 0.5" are discontinuous, and the parity target is a float64 numpy program).  The pair's 37 parameters are
// wave-uniform loads.  Per thread: eight box bounds and a count in registers, all kept as MAXIMA of non-negative codes
// (a minimum m is kept as SIDE - m, a maximum M as M + 1; 0 = nothing seen), so that the all-zero accumulator the
// call's clear leaves (clear_acc: a kernel, not a memset node) is the neutral element.  Wave reduction by __shfl_xor over 64 lanes, one LDS step per workgroup, then one set
// of integer atomicMax / atomicAdd per workgroup that saw an inlier: integer atomics commute, the result does not
// depend on arrival order.  k_covis_finish (one thread per pair) decodes the accumulators into float32 boxes, the
// valid byte and the count.  Masks are plain byte stores of 1 into memory the call cleared.
//
// The set entry (include/oetr_covis_set.h) runs the SAME per-pixel code - covis_block, the one copy - from
// k_covis_warp_indexed: the two maps of a pair come from a device table by index and have sizes of their own, all
// of it wave-uniform loads before the first pixel is touched; a pair the table does not vouch for is left alone.
// k_covis_select is the reference's mining criterion (scale_diff > threshold) as an ordered compaction by ONE
// workgroup, so the kept list is in list order whatever the scheduling.
#include <cmath>
#include <string>

#include "../../include/oetr_covis_set.h"
#include "common.h"
#include "depth_pose.h"

namespace oetr {

constexpr int COVIS_THREADS = 256;
constexpr int COVIS_PER_THREAD = 8;
constexpr int COVIS_PIX = COVIS_THREADS * COVIS_PER_THREAD;      // pixels per workgroup
constexpr int COVIS_ACC = 16;                                    // int32 per pair in the workspace (64 B; 9 used)
constexpr int SIDE = OETR_COVIS_MAX_SIDE;
enum { A_MINU, A_MINV, A_MAXU, A_MAXV, A_MINI, A_MINJ, A_MAXI, A_MAXJ, A_COUNT, A_USED };

// One workgroup's COVIS_PIX source pixels of one pair, from `block` * COVIS_PIX on: map 1 is d1 [H1][W1], map 2 is
// d2 [H2][W2], P the pair's parameter block, acc its accumulators, m1 / m2 its masks (both nullptr: none).  Every
// argument is wave-uniform.  The one copy of the per-pixel arithmetic: both entries run it.
__device__ __forceinline__ void covis_block(const float* __restrict__ d1, int H1, int W1,
                                            const float* __restrict__ d2, int H2, int W2,
                                            const double* __restrict__ P, int block, int* __restrict__ acc,
                                            uint8_t* __restrict__ m1, uint8_t* __restrict__ m2) {
#pragma clang fp contract(off)
  const int n_pix = H1 * W1;                                      // <= 2^26
  const int first = block * COVIS_PIX + (int)threadIdx.x;

  float z[COVIS_PER_THREAD];
#pragma unroll
  for (int k = 0; k < COVIS_PER_THREAD; ++k) {
    const int idx = first + k * COVIS_THREADS;
    z[k] = idx < n_pix ? d1[idx] : 0.0f;
  }

  const double fx = P[16], fy = P[17], cx = P[18], cy = P[19];
  const double b1r = P[29], b1c = P[30], r1r = P[31], r1c = P[32];
  const double b2r = P[33], b2c = P[34], r2r = P[35], r2c = P[36];

  int best[A_USED];
#pragma unroll
  for (int a = 0; a < A_USED; ++a) best[a] = 0;

#pragma unroll
  for (int k = 0; k < COVIS_PER_THREAD; ++k) {
    if (!(z[k] > 0.0f)) continue;                                 // no depth (0, negative, NaN) or past the map
    const int idx = first + k * COVIS_THREADS;
    const int v = idx / W1, u = idx - v * W1;
    const double Z = (double)z[k];
    const double x = ((double)u + b1c + 0.5) / r1c;
    const double y = ((double)v + b1r + 0.5) / r1r;
    const double X = (x - cx) * (Z / fx);
    const double Y = (y - cy) * (Z / fy);
    double q[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) q[r] = ((P[4 * r] * X + P[4 * r + 1] * Y) + P[4 * r + 2] * Z) + P[4 * r + 3];
    // a rigid T has the last row (0, 0, 0, 1) and q[3] is exactly 1: x / 1.0 is x for every x (inf and NaN too), so
    // the three divisions are skipped without changing a bit of the result
    double Xc = q[0], Yc = q[1], Zc = q[2];
    if (q[3] != 1.0) { Xc = q[0] / q[3]; Yc = q[1] / q[3]; Zc = q[2] / q[3]; }
    double h[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) h[r] = (P[20 + 3 * r] * Xc + P[21 + 3 * r] * Yc) + P[22 + 3 * r] * Zc;
    const double u2 = (h[0] / h[2]) * r2c - b2c - 0.5;
    const double v2 = (h[1] / h[2]) * r2r - b2r - 0.5;
    // trunc(u2) in [0, W2) <=> -1 < u2 < W2 (false for NaN; +-inf and anything beyond int are outside)
    if (!(u2 > -1.0 && u2 < (double)W2 && v2 > -1.0 && v2 < (double)H2)) continue;
    const int i = (int)u2, j = (int)v2;                           // towards zero; 0 <= i < W2, 0 <= j < H2
    const double Z2 = (double)d2[(size_t)j * W2 + i];
    if (!(fabs(Zc - Z2) < 0.5)) continue;
    best[A_MINU] = max(best[A_MINU], SIDE - u);
    best[A_MINV] = max(best[A_MINV], SIDE - v);
    best[A_MAXU] = max(best[A_MAXU], u + 1);
    best[A_MAXV] = max(best[A_MAXV], v + 1);
    best[A_MINI] = max(best[A_MINI], SIDE - i);
    best[A_MINJ] = max(best[A_MINJ], SIDE - j);
    best[A_MAXI] = max(best[A_MAXI], i + 1);
    best[A_MAXJ] = max(best[A_MAXJ], j + 1);
    best[A_COUNT] += 1;
    if (m1) {
      m1[(size_t)idx] = 1;
      m2[(size_t)j * W2 + i] = 1;
    }
  }

  // wave: butterfly over 64 lanes
#pragma unroll
  for (int a = 0; a < A_USED; ++a) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const int other = __shfl_xor(best[a], off, 64);
      best[a] = a == A_COUNT ? best[a] + other : max(best[a], other);
    }
  }
  // workgroup: one LDS step, then one atomic per accumulator
  __shared__ int part[COVIS_THREADS / 64][A_USED];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int a = 0; a < A_USED; ++a) part[wave][a] = best[a];
  }
  __syncthreads();
  if (threadIdx.x < A_USED) {
    const int a = threadIdx.x;
    int r = part[0][a];
    int n = part[0][A_COUNT];
    for (int w = 1; w < COVIS_THREADS / 64; ++w) {
      r = a == A_COUNT ? r + part[w][a] : max(r, part[w][a]);
      n += part[w][A_COUNT];
    }
    if (n > 0) {
      int* dst = acc + a;
      if (a == A_COUNT) atomicAdd(dst, r); else atomicMax(dst, r);
    }
  }
}

// grid: x = blocks of COVIS_PIX pixels of one map, y = pair
__global__ __launch_bounds__(COVIS_THREADS) void k_covis_warp(const float* __restrict__ depth1,
                                                              const float* __restrict__ depth2,
                                                              const double* __restrict__ params, int H, int W,
                                                              int* __restrict__ acc, uint8_t* __restrict__ mask1,
                                                              uint8_t* __restrict__ mask2) {
  const int pair = blockIdx.y;
  const size_t map = (size_t)pair * (size_t)(H * W);
  covis_block(depth1 + map, H, W, depth2 + map, H, W, params + (size_t)pair * OETR_COVIS_PARAM_DOUBLES,
              (int)blockIdx.x, acc + (size_t)pair * COVIS_ACC, mask1 ? mask1 + map : nullptr,
              mask2 ? mask2 + map : nullptr);
}

// Both rows of pair `pair`, or false when the pair must not be dereferenced (include/oetr_covis_set.h): depth_pose.h's
// test, with no more pixels in a map than the caller vouched for (asked after the sides: H * W <= SIDE * SIDE).
__device__ __forceinline__ bool covis_pair_maps(const oetr_covis_map* __restrict__ maps, int n_maps,
                                                const int32_t* __restrict__ idx1, const int32_t* __restrict__ idx2,
                                                int pair, int max_pixels, oetr_covis_map& a, oetr_covis_map& b) {
  return pair_maps(maps, n_maps, idx1, idx2, pair, a, b,
                   [=](const oetr_covis_map& m) { return map_usable(m) && m.H * m.W <= max_pixels; });
}

// grid: x = blocks of COVIS_PIX pixels up to max_pixels, y = pair.  The indices and the two table rows are
// wave-uniform (scalar) loads; a block past its pair's own H1 * W1 leaves right after them.
__global__ __launch_bounds__(COVIS_THREADS) void k_covis_warp_indexed(const oetr_covis_map* __restrict__ maps,
                                                                      int n_maps, const int32_t* __restrict__ idx1,
                                                                      const int32_t* __restrict__ idx2,
                                                                      const double* __restrict__ params,
                                                                      int max_pixels, int* __restrict__ acc) {
  const int pair = blockIdx.y;
  oetr_covis_map a, b;
  if (!covis_pair_maps(maps, n_maps, idx1, idx2, pair, max_pixels, a, b)) return;
  if ((int)blockIdx.x * COVIS_PIX >= a.H * a.W) return;
  covis_block(a.depth, a.H, a.W, b.depth, b.H, b.W, params + (size_t)pair * OETR_COVIS_PARAM_DOUBLES,
              (int)blockIdx.x, acc + (size_t)pair * COVIS_ACC, nullptr, nullptr);
}

// Pair p's accumulators decoded into its outputs; a pair that was never dereferenced reports count = -1.
__device__ __forceinline__ void covis_decode(const int* __restrict__ acc, int p, bool dereferenced,
                                             float* __restrict__ box1, float* __restrict__ box2,
                                             uint8_t* __restrict__ valid, int32_t* __restrict__ count) {
  const int* a = acc + (size_t)p * COVIS_ACC;
  const int n = dereferenced ? a[A_COUNT] : -1;
  const bool ok = n > 0;
  float* b1 = box1 + 4 * (size_t)p;
  float* b2 = box2 + 4 * (size_t)p;
  b1[0] = ok ? (float)(SIDE - a[A_MINU]) : 0.0f;
  b1[1] = ok ? (float)(SIDE - a[A_MINV]) : 0.0f;
  b1[2] = ok ? (float)(a[A_MAXU] - 1) : 0.0f;
  b1[3] = ok ? (float)(a[A_MAXV] - 1) : 0.0f;
  b2[0] = ok ? (float)(SIDE - a[A_MINI]) : 0.0f;
  b2[1] = ok ? (float)(SIDE - a[A_MINJ]) : 0.0f;
  b2[2] = ok ? (float)(a[A_MAXI] - 1) : 0.0f;
  b2[3] = ok ? (float)(a[A_MAXJ] - 1) : 0.0f;
  valid[p] = ok ? 1 : 0;
  if (count) count[p] = n;
}

// one thread per pair
__global__ void k_covis_finish(const int* __restrict__ acc, int n_pairs, float* __restrict__ box1,
                               float* __restrict__ box2, uint8_t* __restrict__ valid, int32_t* __restrict__ count) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pairs) return;
  covis_decode(acc, p, true, box1, box2, valid, count);
}

// one thread per pair; the test k_covis_warp_indexed made, made again
__global__ void k_covis_finish_indexed(const oetr_covis_map* __restrict__ maps, int n_maps,
                                       const int32_t* __restrict__ idx1, const int32_t* __restrict__ idx2,
                                       int max_pixels, const int* __restrict__ acc, int n_pairs,
                                       float* __restrict__ box1, float* __restrict__ box2,
                                       uint8_t* __restrict__ valid, int32_t* __restrict__ count) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pairs) return;
  oetr_covis_map a, b;
  covis_decode(acc, p, covis_pair_maps(maps, n_maps, idx1, idx2, p, max_pixels, a, b), box1, box2, valid, count);
}

constexpr int SELECT_THREADS = 256;

// Python's max(a, b): a unless b > a (a NaN first argument stays, a NaN second one is dropped)
__device__ __forceinline__ double py_max(double a, double b) { return b > a ? b : a; }

// ONE workgroup: chunks of SELECT_THREADS pairs in list order; within a chunk the kept pairs are numbered by a
// ballot per wave and a running sum over the waves, so the kept list is ascending whatever the scheduling.
__global__ __launch_bounds__(SELECT_THREADS) void k_covis_select(const float* __restrict__ box1,
                                                                 const float* __restrict__ box2,
                                                                 const uint8_t* __restrict__ valid, int n_pairs,
                                                                 double min_scale_diff, int limit,
                                                                 int32_t* __restrict__ kept, int32_t* __restrict__ n_kept,
                                                                 double* __restrict__ scale_diff) {
  constexpr int WAVES = SELECT_THREADS / 64;
  __shared__ int wave_kept[WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int cut = limit > 0 ? limit : n_pairs;
  int total = 0;                                                  // kept so far (uncut); the same in every thread
  for (int base = 0; base < n_pairs; base += SELECT_THREADS) {
    const int p = base + (int)threadIdx.x;
    bool keep = false;
    if (p < n_pairs) {
      const float* a = box1 + 4 * (size_t)p;
      const float* b = box2 + 4 * (size_t)p;
      const double a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3], b0 = b[0], b1 = b[1], b2 = b[2], b3 = b[3];
      const double w_diff = py_max((a2 - a0) / (b2 - b0), (b2 - b0) / (a2 - a0));
      const double h_diff = py_max((a3 - a1) / (b3 - b1), (b3 - b1) / (a3 - a1));
      const double sd = py_max(w_diff, h_diff);
      if (scale_diff) scale_diff[p] = sd;
      const double top_a = fmax(fmax(a0, a1), fmax(a2, a3)), top_b = fmax(fmax(b0, b1), fmax(b2, b3));
      keep = valid[p] != 0 && top_a > 0.0 && top_b > 0.0 && sd > min_scale_diff;
    }
    const unsigned long long votes = __ballot(keep);
    if (lane == 0) wave_kept[wave] = __popcll(votes);
    __syncthreads();
    int before = total, chunk = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
      if (w < wave) before += wave_kept[w];
      chunk += wave_kept[w];
    }
    const int at = before + __popcll(votes & ((1ull << lane) - 1ull));
    if (keep && at < cut) kept[at] = p;
    total += chunk;
    __syncthreads();                                              // wave_kept is rewritten by the next chunk
  }
  const int written = total < cut ? total : cut;
  for (int k = written + (int)threadIdx.x; k < n_pairs; k += SELECT_THREADS) kept[k] = -1;
  if (threadIdx.x == 0) *n_kept = written;
}

constexpr int CLEAR_THREADS = 256;
constexpr unsigned CLEAR_MAX_BLOCKS = 4096;                       // past that a thread stores more than once

// a[0 .. n) = 0 and b[0 .. n) = 0 (grid y: 0 = a, 1 = b): the byte-sized sibling of k_clear_i32 for the two masks,
// a kernel for the same reason (see clear_i32 in match_score.hip).  16-byte stores over each array's aligned body,
// grid-stride; byte stores on the at most 15 bytes before and the at most 15 bytes after it.
__global__ __launch_bounds__(CLEAR_THREADS) void k_clear_u8_pair(uint8_t* __restrict__ a, uint8_t* __restrict__ b,
                                                                 size_t n) {
  uint8_t* __restrict__ p = blockIdx.y == 0 ? a : b;
  const size_t to_aligned = (size_t)((16u - (unsigned)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u);
  const size_t head = to_aligned < n ? to_aligned : n;            // bytes before the first 16-byte boundary
  const size_t body = (n - head) / 16;                            // whole 16-byte words: head + 16 * body <= n
  const size_t tail = head + 16 * body;                           // n - tail <= 15
  uint4* __restrict__ q = reinterpret_cast<uint4*>(p + head);
  const size_t tid = (size_t)blockIdx.x * CLEAR_THREADS + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * CLEAR_THREADS;
  for (size_t i = tid; i < body; i += stride) q[i] = make_uint4(0u, 0u, 0u, 0u);
  if (tid < head) p[tid] = 0;                                     // the grid has at least CLEAR_THREADS threads
  if (tid < n - tail) p[tail + tid] = 0;
}

namespace {

constexpr int COVIS_MAX_GRID_Y = 65535;                           // the grid's y extent: more pairs, more launches

// The accumulators of n_pairs pairs zeroed by the library's clearing kernel, not by a memset node: captured into a
// graph, hipMemsetAsync(acc, 0, 192) left a foreign 16-byte pattern in the accumulators on the graph's second replay
// after device copies between the replays (tests/test_gpu_covis.py: the ragged-clears test; the fault clear_i32 in
// match_score.hip records).  One launch up to INT32_MAX / COVIS_ACC pairs, clear_i32's int count.
hipError_t clear_acc(int* acc, int n_pairs, hipStream_t s) {
  constexpr int64_t chunk = INT32_MAX / COVIS_ACC;
  for (int64_t p0 = 0; p0 < (int64_t)n_pairs; p0 += chunk) {
    const int64_t n = (int64_t)n_pairs - p0 < chunk ? (int64_t)n_pairs - p0 : chunk;
    if (hipError_t e = clear_i32(acc + p0 * COVIS_ACC, n * COVIS_ACC, s)) return e;
  }
  return hipSuccess;
}

hipError_t clear_masks(uint8_t* mask1, uint8_t* mask2, size_t n, hipStream_t s) {
  const size_t words = n / 16 + 1;
  const size_t want = (words + CLEAR_THREADS - 1) / CLEAR_THREADS;
  const unsigned blocks = (unsigned)(want < CLEAR_MAX_BLOCKS ? want : CLEAR_MAX_BLOCKS);
  hipLaunchKernelGGL(k_clear_u8_pair, dim3(blocks, 2), dim3(CLEAR_THREADS), 0, s, mask1, mask2, n);
  return hipGetLastError();
}

}  // namespace
}  // namespace oetr

using namespace oetr;

extern "C" {

int oetr_covis_abi_version(void) { return OETR_COVIS_ABI_VERSION; }

size_t oetr_covis_workspace_bytes(int n_pairs) {
  return n_pairs > 0 ? (size_t)n_pairs * COVIS_ACC * sizeof(int) : 0;
}

oetr_status oetr_covis_boxes(const float* depth1, const float* depth2, const double* params, int n_pairs,
                             int H, int W, void* workspace, size_t workspace_bytes, float* box1, float* box2,
                             uint8_t* valid, int32_t* count, uint8_t* mask1, uint8_t* mask2, void* stream) {
  const char* me = "oetr_covis_boxes";
  if (!depth1 || !depth2 || !params) return entry_fail(me, OETR_ERR_BAD_ARG, "NULL depth / parameter pointer");
  if (!box1 || !box2 || !valid) return entry_fail(me, OETR_ERR_BAD_ARG, "NULL box / valid output");
  if ((mask1 == nullptr) != (mask2 == nullptr))
    return entry_fail(me, OETR_ERR_BAD_ARG, "mask1 and mask2 must both be NULL or both be set");
  if (n_pairs <= 0) return entry_fail(me, OETR_ERR_BAD_ARG, "need n_pairs > 0");
  if (H < 1 || W < 1 || H > SIDE || W > SIDE)
    return entry_fail(me, OETR_ERR_BAD_SHAPE, "need 1 <= H, W <= " + std::to_string(SIDE));
  const size_t need = oetr_covis_workspace_bytes(n_pairs);
  if (!workspace || workspace_bytes < need)
    return entry_fail(me, OETR_ERR_BAD_ARG, "workspace NULL or smaller than oetr_covis_workspace_bytes(n_pairs) = " +
                                            std::to_string(need));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t n_pix = (size_t)H * W;
  int* acc = static_cast<int*>(workspace);
  if (oetr_status rc = entry_hip(me, clear_acc(acc, n_pairs, s), "k_clear_i32")) return rc;
  if (mask1) {
    if (oetr_status rc = entry_hip(me, clear_masks(mask1, mask2, n_pix * n_pairs, s), "k_clear_u8_pair")) return rc;
  }
  constexpr int max_pairs = COVIS_MAX_GRID_Y;
  const unsigned blocks = (unsigned)((n_pix + COVIS_PIX - 1) / COVIS_PIX);
  for (int p0 = 0; p0 < n_pairs; p0 += max_pairs) {
    const int n = n_pairs - p0 < max_pairs ? n_pairs - p0 : max_pairs;
    const size_t off = (size_t)p0 * n_pix;
    hipLaunchKernelGGL(k_covis_warp, dim3(blocks, (unsigned)n), dim3(COVIS_THREADS), 0, s, depth1 + off,
                       depth2 + off, params + (size_t)p0 * OETR_COVIS_PARAM_DOUBLES, H, W,
                       acc + (size_t)p0 * COVIS_ACC, mask1 ? mask1 + off : nullptr, mask2 ? mask2 + off : nullptr);
    if (oetr_status rc = entry_hip(me, hipGetLastError(), "k_covis_warp")) return rc;
  }
  hipLaunchKernelGGL(k_covis_finish, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, s, acc, n_pairs, box1,
                     box2, valid, count);
  return entry_hip(me, hipGetLastError(), "k_covis_finish");
}

int oetr_covis_set_abi_version(void) { return OETR_COVIS_SET_ABI_VERSION; }

size_t oetr_covis_set_workspace_bytes(int n_pairs) { return oetr_covis_workspace_bytes(n_pairs); }

oetr_status oetr_covis_boxes_indexed(const oetr_covis_map* maps, int n_maps, const int32_t* idx1,
                                     const int32_t* idx2, const double* params, int n_pairs, int64_t max_pixels,
                                     void* workspace, size_t workspace_bytes, float* box1, float* box2,
                                     uint8_t* valid, int32_t* count, void* stream) {
  const char* me = "oetr_covis_boxes_indexed";
  if (!maps || !idx1 || !idx2 || !params) return entry_fail(me, OETR_ERR_BAD_ARG, "NULL map table / index / parameter pointer");
  if (!box1 || !box2 || !valid) return entry_fail(me, OETR_ERR_BAD_ARG, "NULL box / valid output");
  if (n_maps <= 0 || n_pairs <= 0) return entry_fail(me, OETR_ERR_BAD_ARG, "need n_maps > 0 and n_pairs > 0");
  if (max_pixels < 1 || max_pixels > (int64_t)SIDE * SIDE)
    return entry_fail(me, OETR_ERR_BAD_SHAPE, "need 1 <= max_pixels <= " + std::to_string((int64_t)SIDE * SIDE));
  const size_t need = oetr_covis_set_workspace_bytes(n_pairs);
  if (!workspace || workspace_bytes < need)
    return entry_fail(me, OETR_ERR_BAD_ARG, "workspace NULL or smaller than oetr_covis_set_workspace_bytes(n_pairs) = " +
                                            std::to_string(need));
  hipStream_t s = static_cast<hipStream_t>(stream);
  int* acc = static_cast<int*>(workspace);
  if (oetr_status rc = entry_hip(me, clear_acc(acc, n_pairs, s), "k_clear_i32")) return rc;
  const int max_pix = (int)max_pixels;
  const unsigned blocks = (unsigned)((max_pix + COVIS_PIX - 1) / COVIS_PIX);
  for (int p0 = 0; p0 < n_pairs; p0 += COVIS_MAX_GRID_Y) {
    const int n = n_pairs - p0 < COVIS_MAX_GRID_Y ? n_pairs - p0 : COVIS_MAX_GRID_Y;
    hipLaunchKernelGGL(k_covis_warp_indexed, dim3(blocks, (unsigned)n), dim3(COVIS_THREADS), 0, s, maps, n_maps,
                       idx1 + p0, idx2 + p0, params + (size_t)p0 * OETR_COVIS_PARAM_DOUBLES, max_pix,
                       acc + (size_t)p0 * COVIS_ACC);
    if (oetr_status rc = entry_hip(me, hipGetLastError(), "k_covis_warp_indexed")) return rc;
  }
  hipLaunchKernelGGL(k_covis_finish_indexed, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, s, maps, n_maps,
                     idx1, idx2, max_pix, acc, n_pairs, box1, box2, valid, count);
  return entry_hip(me, hipGetLastError(), "k_covis_finish_indexed");
}

oetr_status oetr_covis_select(const float* box1, const float* box2, const uint8_t* valid, int n_pairs,
                              double min_scale_diff, int limit, int32_t* kept, int32_t* n_kept, double* scale_diff,
                              void* workspace, size_t workspace_bytes, void* stream) {
  const char* me = "oetr_covis_select";
  (void)workspace; (void)workspace_bytes;                         // reserved (include/oetr_covis_set.h)
  if (!box1 || !box2 || !valid) return entry_fail(me, OETR_ERR_BAD_ARG, "NULL box / valid input");
  if (!kept || !n_kept) return entry_fail(me, OETR_ERR_BAD_ARG, "NULL kept / n_kept output");
  if (n_pairs <= 0) return entry_fail(me, OETR_ERR_BAD_ARG, "need n_pairs > 0");
  if (std::isnan(min_scale_diff)) return entry_fail(me, OETR_ERR_BAD_ARG, "min_scale_diff is NaN");
  hipLaunchKernelGGL(k_covis_select, dim3(1), dim3(SELECT_THREADS), 0, static_cast<hipStream_t>(stream), box1, box2,
                     valid, n_pairs, min_scale_diff, limit, kept, n_kept, scale_diff);
  return entry_hip(me, hipGetLastError(), "k_covis_select");
}

}  // extern "C"
