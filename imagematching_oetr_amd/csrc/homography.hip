// Scoring matches and overlap boxes against a homography (include/oetr_homography.h): the planar sibling of the
// depth-and-pose entries.  Both kernels run tests/homography_oracle.py LITERALLY: float64, every operation rounded on
// its own in the order and with the parentheses written there (no contraction into FMAs: rint() and the "<=" tests
// are discontinuous and the parity target is a float64 numpy program), IEEE division.
//
// k_homography_score: one thread per match row, 256-thread workgroups, the row -> list step of match_list.h.  A wave
// whose rows all lie in the list of its first row - the common case - takes the nine doubles of H by scalar loads,
// as it took that list, so a row's vector loads are its two keypoints.  Per row 6 v_mul_f64, 9 v_add_f64 and two
// divisions.  The squared thresholds travel in the kernel's arguments.  Counters: a wave whose counted rows all belong to one pair
// takes one ballot and one popcount per threshold, lane t keeping threshold t's count, and issues ONE atomic
// instruction on the pair's adjacent counters (one instruction per threshold, all from lane 0, cost twice the whole
// call; summing the workgroup's four waves through LDS first, and 8-byte keypoint loads, gained nothing measurable:
// DESIGN 9.3i); a wave that straddles lists falls back to per-lane atomicAdd.  k_homography_init (one thread per
// counter) writes the list lengths and zeroes the rest beforehand - a kernel, not a memset node: see clear_i32 in
// match_score.hip.
//
// k_homography_warp: the structure of k_covis_warp (covis.hip) without a depth map - a workgroup of 256 threads takes
// HOM_PIX consecutive pixels of one pair, each thread HOM_PER_THREAD of them; it reads the pair's 13 parameters
// (wave-uniform) and NOTHING else.  Eight box bounds and a count per thread, kept as MAXIMA of non-negative codes
// (a minimum m as SIDE - m, a maximum M as M + 1; 0 = nothing seen) so that zero is the neutral element; butterfly
// over the wave, one LDS step per workgroup, then one set of integer atomicMax / atomicAdd per workgroup that kept a
// pixel.  k_homography_finish (one thread per pair) decodes the accumulators.  A pair whose sizes fail hom_sizes is
// left alone by both kernels.
#include <cmath>
#include <string>

#include "../../include/oetr_homography.h"
#include "common.h"
#include "match_list.h"

namespace oetr {

constexpr int HOM_THREADS = 256;
constexpr int HOM_PARAMS = OETR_HOMOGRAPHY_PARAM_DOUBLES;
constexpr int HOM_MAX_THR = OETR_HOMOGRAPHY_MAX_THRESHOLDS;
constexpr int HOM_PER_THREAD = 8;
constexpr int HOM_PIX = HOM_THREADS * HOM_PER_THREAD;            // pixels per workgroup
constexpr int HOM_ACC = 16;                                      // int32 per pair in the workspace (64 B; 9 used)
constexpr int HOM_SIDE = OETR_COVIS_MAX_SIDE;
constexpr int HOM_MAX_GRID_Y = 65535;                            // the grid's y extent: more pairs, more launches
enum { B_MINU, B_MINV, B_MAXU, B_MAXV, B_MINI, B_MINJ, B_MAXI, B_MAXJ, B_COUNT, B_USED };

struct HomThresholds {
  double sq[HOM_MAX_THR];                                        // thr * thr, NaN past n_thresholds
};

// One row of tests/homography_oracle.py::score under the H at P.  The one copy of the arithmetic; inlined twice (H by
// scalar loads / by per-lane loads).
__device__ __forceinline__ double hom_row(const double* __restrict__ P, double x, double y, double x2, double y2) {
#pragma clang fp contract(off)
  const double a0 = (P[0] * x + P[1] * y) + P[2];
  const double a1 = (P[3] * x + P[4] * y) + P[5];
  const double a2 = (P[6] * x + P[7] * y) + P[8];
  const double pu = a0 / a2, pv = a1 / a2;
  return (x2 - pu) * (x2 - pu) + (y2 - pv) * (y2 - pv);
}

__global__ __launch_bounds__(HOM_THREADS) void k_homography_score(
    const double* __restrict__ params, const int32_t* __restrict__ offsets, int n_pairs, const float* __restrict__ k1,
    const float* __restrict__ k2, int n_matches, HomThresholds thr, int n_thr, double* __restrict__ dist_sq,
    int32_t* __restrict__ counts) {
  const int64_t row = (int64_t)blockIdx.x * HOM_THREADS + (int64_t)threadIdx.x;
  const bool active = row < (int64_t)n_matches;
  const int m = active ? (int)row : 0;

  // the keypoints depend on the row alone: their loads go out before the search
  float x = 0.0f, y = 0.0f, x2 = 0.0f, y2 = 0.0f;
  if (active) {
    const size_t at = 2 * (size_t)m;
    x = k1[at], y = k1[at + 1], x2 = k2[at], y2 = k2[at + 1];
  }

  int p0, p;                                                        // the wave's first row's list, this row's
  wave_find_list<HOM_THREADS>(offsets, n_pairs, n_matches, active, m, p0, p);

  double d = __longlong_as_double(0x7ff8000000000000ll);
  if (__ballot(active && p != p0) == 0ull) {
    // every active row of the wave is in list p0: H by scalar loads
    if (p0 >= 0 && active) d = hom_row(params + (size_t)p0 * HOM_PARAMS, (double)x, (double)y, (double)x2, (double)y2);
  } else if (p >= 0) {
    d = hom_row(params + (size_t)p * HOM_PARAMS, (double)x, (double)y, (double)x2, (double)y2);
  }
  if (active && dist_sq) dist_sq[(size_t)m] = d;

  // bit t: dist_sq <= thr_t^2 (false for a NaN on either side).  Every lane of the wave arrives here.
  const int counted = active ? p : -1;                              // the pair this row counts for, or none
  unsigned hits = 0u;
#pragma unroll
  for (int t = 0; t < HOM_MAX_THR; ++t)
    if (t < n_thr && counted >= 0 && d <= thr.sq[t]) hits |= 1u << t;

  const int stride = 1 + n_thr;
  const WaveCounted w = wave_counted(counted);
  if (!w.any) return;                                               // wave-uniform
  if (w.one_pair) {
    // lane t keeps the wave's count of threshold t: ONE atomic instruction per wave, on adjacent counters
    const int lane = threadIdx.x & 63;
    int mine = 0;
#pragma unroll
    for (int t = 0; t < HOM_MAX_THR; ++t) {
      if (t < n_thr) {                                              // wave-uniform
        const int n = __popcll(__ballot((hits >> t) & 1u));
        if (lane == t) mine = n;
      }
    }
    if (mine) atomicAdd(counts + (size_t)w.first * stride + 1 + lane, mine);   // mine != 0 only for lane < n_thr
  } else if (counted >= 0) {
    int32_t* c = counts + (size_t)counted * stride;
    for (int t = 0; t < n_thr; ++t)
      if ((hits >> t) & 1u) atomicAdd(c + 1 + t, 1);
  }
}

// One thread per counter: counts[p][0] = the list length clamped to [0, n_matches], the rest 0.
__global__ void k_homography_init(const int32_t* __restrict__ offsets, int n_pairs, int n_matches, int stride,
                                  int32_t* __restrict__ counts) {
  const unsigned at = blockIdx.x * blockDim.x + threadIdx.x;
  if (at >= (unsigned)(n_pairs * stride)) return;                   // n_pairs * stride <= INT32_MAX (host check)
  const int p = (int)(at / (unsigned)stride), k = (int)(at - (unsigned)p * (unsigned)stride);
  counts[at] = k == 0 ? list_length(offsets, p, n_matches) : 0;
}

// The sizes of the pair at P, or false when the pair must not be evaluated: W1, H1, W2, H2 not whole numbers in
// 1..OETR_COVIS_MAX_SIDE (false for NaN), or picture 1 larger than the grid the host vouched for.
__device__ __forceinline__ bool hom_sizes(const double* __restrict__ P, int max_h1, int max_w1, int& W1, int& H1,
                                          int& W2, int& H2) {
  const double w1 = P[9], h1 = P[10], w2 = P[11], h2 = P[12];
  auto side = [](double s) { return s >= 1.0 && s <= (double)HOM_SIDE && s == rint(s); };
  if (!(side(w1) && side(h1) && side(w2) && side(h2))) return false;
  W1 = (int)w1, H1 = (int)h1, W2 = (int)w2, H2 = (int)h2;
  return H1 <= max_h1 && W1 <= max_w1;
}

// grid: x = blocks of HOM_PIX pixels up to max_h1 * max_w1, y = pair.  Everything loaded is wave-uniform.
__global__ __launch_bounds__(HOM_THREADS) void k_homography_warp(const double* __restrict__ params, int max_h1,
                                                                 int max_w1, int* __restrict__ acc_all) {
#pragma clang fp contract(off)
  const int pair = blockIdx.y;
  const double* __restrict__ P = params + (size_t)pair * HOM_PARAMS;
  int W1, H1, W2, H2;
  if (!hom_sizes(P, max_h1, max_w1, W1, H1, W2, H2)) return;
  const int n_pix = H1 * W1;                                      // <= 2^26
  if ((int)blockIdx.x * HOM_PIX >= n_pix) return;
  const int first = (int)blockIdx.x * HOM_PIX + (int)threadIdx.x;
  const double h00 = P[0], h01 = P[1], h02 = P[2], h10 = P[3], h11 = P[4], h12 = P[5], h20 = P[6], h21 = P[7],
               h22 = P[8];
  const double w2 = (double)W2, h2 = (double)H2;

  int best[B_USED];
#pragma unroll
  for (int a = 0; a < B_USED; ++a) best[a] = 0;

#pragma unroll
  for (int k = 0; k < HOM_PER_THREAD; ++k) {
    const int idx = first + k * HOM_THREADS;
    if (idx >= n_pix) continue;
    const int v = idx / W1, u = idx - v * W1;
    const double x = (double)u, y = (double)v;
    const double a0 = (h00 * x + h01 * y) + h02;
    const double a1 = (h10 * x + h11 * y) + h12;
    const double a2 = (h20 * x + h21 * y) + h22;
    if (!(a2 > 0.0)) continue;                                    // beyond the horizon line (or NaN)
    const double fi = rint(a0 / a2), fj = rint(a1 / a2);          // half to even
    if (!(fi >= 0.0 && fi < w2 && fj >= 0.0 && fj < h2)) continue;   // false for NaN; +-inf are outside
    const int i = (int)fi, j = (int)fj;                           // 0 <= i < W2, 0 <= j < H2
    best[B_MINU] = max(best[B_MINU], HOM_SIDE - u);
    best[B_MINV] = max(best[B_MINV], HOM_SIDE - v);
    best[B_MAXU] = max(best[B_MAXU], u + 1);
    best[B_MAXV] = max(best[B_MAXV], v + 1);
    best[B_MINI] = max(best[B_MINI], HOM_SIDE - i);
    best[B_MINJ] = max(best[B_MINJ], HOM_SIDE - j);
    best[B_MAXI] = max(best[B_MAXI], i + 1);
    best[B_MAXJ] = max(best[B_MAXJ], j + 1);
    best[B_COUNT] += 1;
  }

  // wave: butterfly over 64 lanes
#pragma unroll
  for (int a = 0; a < B_USED; ++a) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const int other = __shfl_xor(best[a], off, 64);
      best[a] = a == B_COUNT ? best[a] + other : max(best[a], other);
    }
  }
  // workgroup: one LDS step, then one atomic per accumulator
  __shared__ int part[HOM_THREADS / 64][B_USED];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int a = 0; a < B_USED; ++a) part[wave][a] = best[a];
  }
  __syncthreads();
  if (threadIdx.x < B_USED) {
    const int a = threadIdx.x;
    int r = part[0][a];
    int n = part[0][B_COUNT];
    for (int w = 1; w < HOM_THREADS / 64; ++w) {
      r = a == B_COUNT ? r + part[w][a] : max(r, part[w][a]);
      n += part[w][B_COUNT];
    }
    if (n > 0) {
      int* dst = acc_all + (size_t)pair * HOM_ACC + a;
      if (a == B_COUNT) atomicAdd(dst, r); else atomicMax(dst, r);
    }
  }
}

// one thread per pair; the test k_homography_warp made, made again
__global__ void k_homography_finish(const double* __restrict__ params, int max_h1, int max_w1,
                                    const int* __restrict__ acc, int n_pairs, float* __restrict__ box1,
                                    float* __restrict__ box2, uint8_t* __restrict__ valid,
                                    int32_t* __restrict__ count) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pairs) return;
  int W1, H1, W2, H2;
  const bool evaluated = hom_sizes(params + (size_t)p * HOM_PARAMS, max_h1, max_w1, W1, H1, W2, H2);
  const int* a = acc + (size_t)p * HOM_ACC;
  const int n = evaluated ? a[B_COUNT] : -1;
  const bool ok = n > 0;
  float* b1 = box1 + 4 * (size_t)p;
  float* b2 = box2 + 4 * (size_t)p;
  b1[0] = ok ? (float)(HOM_SIDE - a[B_MINU]) : 0.0f;
  b1[1] = ok ? (float)(HOM_SIDE - a[B_MINV]) : 0.0f;
  b1[2] = ok ? (float)(a[B_MAXU] - 1) : 0.0f;
  b1[3] = ok ? (float)(a[B_MAXV] - 1) : 0.0f;
  b2[0] = ok ? (float)(HOM_SIDE - a[B_MINI]) : 0.0f;
  b2[1] = ok ? (float)(HOM_SIDE - a[B_MINJ]) : 0.0f;
  b2[2] = ok ? (float)(a[B_MAXI] - 1) : 0.0f;
  b2[3] = ok ? (float)(a[B_MAXJ] - 1) : 0.0f;
  valid[p] = ok ? 1 : 0;
  if (count) count[p] = n;
}

}  // namespace oetr

using namespace oetr;

extern "C" {

int oetr_homography_abi_version(void) { return OETR_HOMOGRAPHY_ABI_VERSION; }

// The host code dereferences none of its device pointer arguments and reads nothing from the device; `thresholds`
// is host memory and is read here.
oetr_status oetr_homography_match_score(const double* params, const int32_t* offsets, int n_pairs, const float* k1,
                                        const float* k2, int64_t n_matches, const double* thresholds, int n_thresholds,
                                        double* dist_sq, int32_t* counts, void* stream) {
  const char* me = "oetr_homography_match_score";
  if (!params || !offsets) return entry_fail(me, OETR_ERR_BAD_ARG, "NULL parameter / offsets pointer");
  if (!counts) return entry_fail(me, OETR_ERR_BAD_ARG, "NULL counts output");
  if (n_matches != 0 && (!k1 || !k2)) return entry_fail(me, OETR_ERR_BAD_ARG, "NULL keypoint pointer");
  if (n_thresholds < 0 || n_thresholds > HOM_MAX_THR)
    return entry_fail(me, OETR_ERR_BAD_ARG, "need 0 <= n_thresholds <= " + std::to_string(HOM_MAX_THR));
  if (n_thresholds != 0 && !thresholds) return entry_fail(me, OETR_ERR_BAD_ARG, "NULL thresholds");
  if (n_pairs <= 0) return entry_fail(me, OETR_ERR_BAD_ARG, "need n_pairs > 0");
  if (n_matches < 0) return entry_fail(me, OETR_ERR_BAD_ARG, "need n_matches >= 0");
  if (n_pairs > INT32_MAX / (1 + HOM_MAX_THR))
    return entry_fail(me, OETR_ERR_BAD_SHAPE, "need n_pairs <= " + std::to_string(INT32_MAX / (1 + HOM_MAX_THR)));
  if (n_matches > (int64_t)INT32_MAX)
    return entry_fail(me, OETR_ERR_BAD_SHAPE, "need n_matches <= " + std::to_string(INT32_MAX) + " (the offsets are int32)");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int n = (int)n_matches;
  HomThresholds thr;
  for (int t = 0; t < HOM_MAX_THR; ++t) thr.sq[t] = t < n_thresholds ? thresholds[t] * thresholds[t] : std::nan("");
  const int stride = 1 + n_thresholds;
  const int n_counters = n_pairs * stride;                          // n_pairs <= INT32_MAX / 17, checked above
  hipLaunchKernelGGL(k_homography_init, dim3((unsigned)(((int64_t)n_counters + 255) / 256)), dim3(256), 0, s, offsets,
                     n_pairs, n, stride, counts);
  if (oetr_status rc = entry_hip(me, hipGetLastError(), "k_homography_init")) return rc;
  if (n > 0) {
    const unsigned blocks = (unsigned)(((int64_t)n + HOM_THREADS - 1) / HOM_THREADS);
    hipLaunchKernelGGL(k_homography_score, dim3(blocks), dim3(HOM_THREADS), 0, s, params, offsets, n_pairs, k1, k2, n,
                       thr, n_thresholds, dist_sq, counts);
    if (oetr_status rc = entry_hip(me, hipGetLastError(), "k_homography_score")) return rc;
  }
  return OETR_OK;
}

size_t oetr_homography_workspace_bytes(int n_pairs) {
  return n_pairs > 0 ? (size_t)n_pairs * HOM_ACC * sizeof(int) : 0;
}

oetr_status oetr_homography_boxes(const double* params, int n_pairs, int max_h1, int max_w1, void* workspace,
                                  size_t workspace_bytes, float* box1, float* box2, uint8_t* valid, int32_t* count,
                                  void* stream) {
  const char* me = "oetr_homography_boxes";
  if (!params) return entry_fail(me, OETR_ERR_BAD_ARG, "NULL parameter pointer");
  if (!box1 || !box2 || !valid) return entry_fail(me, OETR_ERR_BAD_ARG, "NULL box / valid output");
  if (n_pairs <= 0) return entry_fail(me, OETR_ERR_BAD_ARG, "need n_pairs > 0");
  if (n_pairs > INT32_MAX / (1 + HOM_MAX_THR))
    return entry_fail(me, OETR_ERR_BAD_SHAPE, "need n_pairs <= " + std::to_string(INT32_MAX / (1 + HOM_MAX_THR)));
  if (max_h1 < 1 || max_w1 < 1 || max_h1 > HOM_SIDE || max_w1 > HOM_SIDE)
    return entry_fail(me, OETR_ERR_BAD_SHAPE, "need 1 <= max_h1, max_w1 <= " + std::to_string(HOM_SIDE));
  const size_t need = oetr_homography_workspace_bytes(n_pairs);
  if (!workspace || workspace_bytes < need)
    return entry_fail(me, OETR_ERR_BAD_ARG, "workspace NULL or smaller than oetr_homography_workspace_bytes(n_pairs) = " +
                                            std::to_string(need));
  hipStream_t s = static_cast<hipStream_t>(stream);
  int* acc = static_cast<int*>(workspace);
  // n_pairs * 16 <= INT32_MAX, checked above; cleared by a kernel, not by a memset node: see clear_i32 (match_score.hip)
  if (oetr_status rc = entry_hip(me, clear_i32(acc, (int64_t)n_pairs * HOM_ACC, s), "k_clear_i32")) return rc;
  const int max_pix = max_h1 * max_w1;                              // <= 2^26
  const unsigned blocks = (unsigned)((max_pix + HOM_PIX - 1) / HOM_PIX);
  for (int p0 = 0; p0 < n_pairs; p0 += HOM_MAX_GRID_Y) {
    const int n = n_pairs - p0 < HOM_MAX_GRID_Y ? n_pairs - p0 : HOM_MAX_GRID_Y;
    hipLaunchKernelGGL(k_homography_warp, dim3(blocks, (unsigned)n), dim3(HOM_THREADS), 0, s,
                       params + (size_t)p0 * HOM_PARAMS, max_h1, max_w1, acc + (size_t)p0 * HOM_ACC);
    if (oetr_status rc = entry_hip(me, hipGetLastError(), "k_homography_warp")) return rc;
  }
  hipLaunchKernelGGL(k_homography_finish, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, s, params, max_h1,
                     max_w1, acc, n_pairs, box1, box2, valid, count);
  return entry_hip(me, hipGetLastError(), "k_homography_finish");
}

}  // extern "C"
