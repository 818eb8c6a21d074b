// Dual-softmax matching of dense feature grids (include/oetr_dual_softmax.h): the coarse matching head of a
// detector-free matcher for all pairs of a call, bit for bit the numpy program tests/dual_softmax_oracle.py.  No
// similarity or confidence matrix goes to global memory: the tile of similarities is recomputed by each sweep.
//
// Five launches, ordered by the launch boundary alone (no workgroup waits on another):
//   k_ds_clear      every row of matches0 / scores0 / direction 1's matches / the keypoints reads -1 / 0 / NaN: the rows
//                   no pair owns and the rows of the pairs that are not matched keep that.
//   k_ds_sweep<1>   k_nn_top2's decomposition (nn_match.hip): one workgroup = one pair, one direction, 64 query rows;
//                   it walks the other side in tiles of 128 key rows in ASCENDING order and D in steps of 64 columns
//                   staged through LDS; wave (qh, kh) of the four owns the 32 query rows qh and the 64 key rows kh of
//                   the tile as two 32x32 accumulators of v_mfma_f32_32x32x2_f32 with the KEYS as the A operand, so a
//                   lane has its query on the lane and 16 keys per accumulator in its registers.  Each (i, j) is ONE
//                   chain over ascending d.  Sweep 1 keeps the maximum of the query's finite t = s * scale and writes
//                   the query's keypoint;
//   k_ds_sweep<2>   the sum of e(t - m): a lane's two accumulators are two of the specification's eight partial sums
//                   (dual_softmax_math.h: slot), which take their columns in ascending j because a lane walks its
//                   registers and the tiles in that order; the tree's three levels are the lane's two accumulators,
//                   the two lane halves and the two key waves;
//   k_ds_sweep<3>   the confidence of every element from the query's (m, Z) and, staged per tile, the keys' (c, Y) of
//                   the workspace, and the running (maximum, lowest index) under an order that makes the merges free
//                   of the walk.
//   k_ds_decide     one workgroup per pair: threshold, borders and the mutual test in place on matches0, the counters.
// Direction 1 is the same kernel with the sides swapped: fmaf and the product of the two factors commute, so it
// recomputes bit-equal values.
//
// The staging (ds_fetch / ds_store) and the tile walk restate nn_match.hip's; that file is left untouched, so
// match_descriptors' device code cannot move.
//
// Nothing is dereferenced on the strength of device data alone: ds_range clamps the offsets into [0, n], a pair
// beyond max_k0 / max_k1 or whose grid does not multiply to its row count is left before any row is read, rows are
// loaded and written below the clamped K only, and a match index passes ONE unsigned compare against S before it
// forms an address.
#include <cmath>
#include <string>

#include "../../include/oetr_dual_softmax.h"
#include "common.h"
#include "dual_softmax_math.h"

namespace oetr {

constexpr int DS_THREADS = 256;
constexpr int DS_QT = 64;            // query rows of a workgroup
constexpr int DS_KT = 128;           // key rows of a tile
constexpr int DS_DC = 64;            // columns of D per staging step
// An odd row stride: the 32 rows that one lane group of a ds_read_b32 reads at one column fall into 32 banks.
constexpr int DS_LD = DS_DC + 1;
constexpr int DS_COUNTERS = OETR_DUAL_SOFTMAX_COUNTERS;
static_assert(ds::PARTIALS == OETR_DUAL_SOFTMAX_PARTIALS, "the header states the partial sums of the arithmetic");

using ds_f32x16 = __attribute__((ext_vector_type(16))) float;

struct DsRange {
  int s, e;
};

// rows off[p] .. off[p+1]-1, clamped: 0 <= s <= e <= n whatever the device holds
__device__ __forceinline__ DsRange ds_range(const int32_t* __restrict__ off, int p, int n) {
  int s = off[p], e = off[p + 1];
  s = s < 0 ? 0 : (s > n ? n : s);
  e = e < s ? s : (e > n ? n : e);
  return {s, e};
}

struct DsGrid {
  int h, w;
};

__device__ __forceinline__ DsGrid ds_grid(const int32_t* __restrict__ grids, int p) {
  return {grids[2 * (size_t)p], grids[2 * (size_t)p + 1]};
}

// the pair is matched: within max_k*, and each grid multiplies to its side's row count
__device__ __forceinline__ bool ds_vouched(int K0, int K1, int max_k0, int max_k1, DsGrid g0, DsGrid g1) {
  return K0 <= max_k0 && K1 <= max_k1 && g0.h >= 0 && g0.w >= 0 && g1.h >= 0 && g1.w >= 0 &&
         (int64_t)g0.h * g0.w == (int64_t)K0 && (int64_t)g1.h * g1.w == (int64_t)K1;
}

struct DsArgs {
  const float* feat[2];
  const int32_t* off[2];
  const int32_t* grids[2];
  int n[2], max_k[2], tiles[2];
  int D, cell;
  float scale;
  float2* stats[2];                  // (maximum, sum) of every token as a query
  float* keypoints[2];
  int32_t* matches0;
  float* scores0;
  int32_t* m1;
};

__global__ __launch_bounds__(DS_THREADS) void k_ds_clear(int32_t* __restrict__ matches0, float* __restrict__ scores0,
                                                         float2* __restrict__ kp0, int n0, int32_t* __restrict__ m1,
                                                         float2* __restrict__ kp1, int n1) {
  const int64_t step = (int64_t)gridDim.x * DS_THREADS;
  const float2 none = make_float2(NAN, NAN);
  for (int64_t r = (int64_t)blockIdx.x * DS_THREADS + threadIdx.x; r < (int64_t)n0; r += step) {
    matches0[r] = -1;
    scores0[r] = 0.0f;
    kp0[r] = none;
  }
  for (int64_t r = (int64_t)blockIdx.x * DS_THREADS + threadIdx.x; r < (int64_t)n1; r += step) {
    m1[r] = -1;
    kp1[r] = none;
  }
}

// ROWS x DS_DC floats of the rows row0 .. of a side (g: the side's first row of the pair, K its rows) from column d0 on,
// as ROWS / 16 float4 per thread; rows from K on and columns from D on read 0
template <int ROWS>
__device__ __forceinline__ void ds_fetch(float4 (&v)[ROWS / 16], const float* __restrict__ g, int K, int row0, int D,
                                         int d0, int tid) {
  const int d = d0 + 4 * (tid & 15);
#pragma unroll
  for (int i = 0; i < ROWS / 16; ++i) {
    const int r = row0 + (tid >> 4) + 16 * i;
    v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < K && d < D) v[i] = *reinterpret_cast<const float4*>(g + (size_t)r * (size_t)D + d);   // D % 4 == 0
  }
}

template <int ROWS>
__device__ __forceinline__ void ds_store(float* __restrict__ s, const float4 (&v)[ROWS / 16], int tid) {
#pragma unroll
  for (int i = 0; i < ROWS / 16; ++i) {
    float* dst = s + ((tid >> 4) + 16 * i) * DS_LD + 4 * (tid & 15);
    dst[0] = v[i].x, dst[1] = v[i].y, dst[2] = v[i].z, dst[3] = v[i].w;
  }
}

// What a lane keeps of its query over the walk, and what it does with one complete similarity.
template <int SWEEP>
struct DsLane;

template <>
struct DsLane<1> {
  float m = -INFINITY;
  __device__ __forceinline__ void take(int, float t, int, float2) { m = ds::max_push(m, t); }
};

template <>
struct DsLane<2> {
  float my_m = 0.0f, z[2] = {0.0f, 0.0f};
  __device__ __forceinline__ void take(int a, float t, int, float2) {
    if (ds::finite(t)) z[a] = ds::add_term(z[a], ds::e(t - my_m));
  }
};

template <>
struct DsLane<3> {
  float my_m = 0.0f, my_Z = 1.0f;
  ds::Best best = ds::best_empty();
  __device__ __forceinline__ void take(int, float t, int j, float2 key) {
    ds::best_push(best, ds::confidence(t, my_m, my_Z, key.x, key.y), j);
  }
};

// Three workgroups per CU, as many as the LDS holds (k_nn_top2's choice, nn_match.hip).
template <int SWEEP>
__global__ __launch_bounds__(DS_THREADS, 3) void k_ds_sweep(const DsArgs a) {
  __shared__ float s_q[DS_QT * DS_LD];
  __shared__ float s_k[DS_KT * DS_LD];
  __shared__ float2 s_key[DS_KT];                                   // sweep 3: the tile's keys' (c, Y)
  __shared__ float s_v[2][DS_QT];
  __shared__ int s_i[2][DS_QT];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int per_pair = a.tiles[0] + a.tiles[1];
  const int p = (int)(blockIdx.x / (unsigned)per_pair);
  const int rem = (int)(blockIdx.x - (unsigned)p * (unsigned)per_pair);
  const int dir = rem >= a.tiles[0] ? 1 : 0;                        // direction 1: side 1 asks, side 0 answers
  const int q0 = (dir ? rem - a.tiles[0] : rem) * DS_QT;
  const DsRange r0 = ds_range(a.off[0], p, a.n[0]), r1 = ds_range(a.off[1], p, a.n[1]);
  const DsGrid g0 = ds_grid(a.grids[0], p), g1 = ds_grid(a.grids[1], p);
  if (!ds_vouched(r0.e - r0.s, r1.e - r1.s, a.max_k[0], a.max_k[1], g0, g1)) return;   // nothing of it is read
  const DsRange rq = dir ? r1 : r0, rk = dir ? r0 : r1;
  const int Kq = rq.e - rq.s, Kk = rk.e - rk.s, D = a.D;
  if (q0 >= Kq) return;                                             // uniform: before any barrier
  const float* gq = a.feat[dir] + (size_t)rq.s * (size_t)D;
  const float* gk = a.feat[dir ^ 1] + (size_t)rk.s * (size_t)D;
  float2* stats_q = a.stats[dir] + rq.s;                            // rows below Kq
  const float2* stats_k = a.stats[dir ^ 1] + rk.s;                  // rows below Kk

  const int r = lane & 31, h = lane >> 5, qh = wave & 1, kh = wave >> 1;
  const float* lq = s_q + (qh * 32 + r) * DS_LD + h;                // column d of the step: k slot h of MFMA d / 2
  const float* lk = s_k + (kh * 64 + r) * DS_LD + h;
  DsLane<SWEEP> mine;
  if constexpr (SWEEP >= 2) {
    const int q = q0 + qh * 32 + r;
    if (q < Kq) {
      const float2 st = stats_q[q];
      mine.my_m = st.x;
      if constexpr (SWEEP == 3) mine.my_Z = st.y;
    }
  }
  ds_f32x16 acc0 = {}, acc1 = {};
  const int chunks = (D + DS_DC - 1) / DS_DC;
  const int steps = ((Kk + DS_KT - 1) / DS_KT) * chunks;            // (key tile, chunk of D), the chunks in order
  float4 vq[DS_QT / 16], vk[DS_KT / 16];
  if (steps > 0) {
    ds_fetch<DS_QT>(vq, gq, Kq, q0, D, 0, tid);
    ds_fetch<DS_KT>(vk, gk, Kk, 0, D, 0, tid);
  }
  int kt = 0, c = 0;
  for (int s = 0; s < steps; ++s) {
    ds_store<DS_QT>(s_q, vq, tid);
    ds_store<DS_KT>(s_k, vk, tid);
    if constexpr (SWEEP == 3) {
      if (c == 0 && tid < DS_KT) {                                  // the tile's keys: rows below Kk only
        const int j = kt * DS_KT + tid;
        s_key[tid] = j < Kk ? stats_k[j] : make_float2(0.0f, 1.0f);
      }
    }
    __syncthreads();
    const int len = D - c * DS_DC < DS_DC ? D - c * DS_DC : DS_DC;   // a multiple of 4
    const bool last_chunk = c == chunks - 1;
    const int k0 = kt * DS_KT;
    if (last_chunk) c = 0, ++kt; else ++c;
    if (s + 1 < steps) {                                            // the next step's rows, in flight under the MFMAs
      ds_fetch<DS_QT>(vq, gq, Kq, q0, D, c * DS_DC, tid);
      ds_fetch<DS_KT>(vk, gk, Kk, kt * DS_KT, D, c * DS_DC, tid);
    }
    if (k0 + kh * 64 < Kk) {                                        // wave-uniform: this wave's key rows exist
      auto two_columns = [&](int d) {
        const float q = lq[d];
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(lk[d], q, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(lk[32 * DS_LD + d], q, acc1, 0, 0, 0);
      };
      if (len == DS_DC) {
#pragma unroll
        for (int d = 0; d < DS_DC; d += 2) two_columns(d);
      } else {
        for (int d = 0; d < len; d += 4) two_columns(d), two_columns(d + 2);
      }
    }
    if (last_chunk) {                                               // the tile's similarities are complete
      const int jj0 = kh * 64 + 4 * h;
#pragma unroll
      for (int g = 0; g < 16; ++g) {                                // ascending j within either accumulator
        const int jj = jj0 + (g & 3) + 8 * (g >> 2);                // the accumulator's row: (g & 3) + 8 (g >> 2) + 4 h
        const int j = k0 + jj;
        float2 key0 = make_float2(0.0f, 1.0f), key1 = key0;
        if constexpr (SWEEP == 3) key0 = s_key[jj], key1 = s_key[jj + 32];
        if (j < Kk) mine.take(0, ds::scaled(acc0[g], a.scale), j, key0);
        if (j + 32 < Kk) mine.take(1, ds::scaled(acc1[g], a.scale), j + 32, key1);
      }
      acc0 = ds_f32x16{};
      acc1 = ds_f32x16{};
    }
    __syncthreads();
  }
  // the query's other lane half, then the other key wave
  const int q = qh * 32 + r;
  const size_t row = (size_t)(q0 + tid);                            // of the pair's asking side, for tid < DS_QT
  const bool writer = tid < DS_QT && q0 + tid < Kq;
  if constexpr (SWEEP == 1) {
    const float other = __shfl_xor(mine.m, 32, 64);
    const float m = other > mine.m ? other : mine.m;
    if (h == 0) s_v[kh][q] = m;
    __syncthreads();
    if (writer) {
      stats_q[row].x = s_v[1][tid] > s_v[0][tid] ? s_v[1][tid] : s_v[0][tid];
      const DsGrid g = dir ? g1 : g0;                               // g.h * g.w == Kq > row: g.w >= 1
      const int y = (int)row / g.w, x = (int)row - y * g.w;
      reinterpret_cast<float2*>(a.keypoints[dir])[(size_t)rq.s + row] =
          make_float2((float)((int64_t)x * a.cell), (float)((int64_t)y * a.cell));
    }
  } else if constexpr (SWEEP == 2) {
    float z = ds::tree_node(mine.z[0], mine.z[1]);
    z = ds::tree_node(z, __shfl_xor(z, 32, 64));
    if (h == 0) s_v[kh][q] = z;
    __syncthreads();
    if (writer) stats_q[row].y = ds::tree_node(s_v[0][tid], s_v[1][tid]);
  } else {
    const ds::Best other = {__shfl_xor(mine.best.v, 32, 64), __shfl_xor(mine.best.i, 32, 64)};
    const ds::Best b = ds::best_merge(mine.best, other);
    if (h == 0) s_v[kh][q] = b.v, s_i[kh][q] = b.i;
    __syncthreads();
    if (writer) {
      const ds::Best t = ds::best_merge(ds::Best{s_v[0][tid], s_i[0][tid]}, ds::Best{s_v[1][tid], s_i[1][tid]});
      const size_t out = (size_t)rq.s + row;                        // < n of the asking side
      if (dir) {
        a.m1[out] = t.i;
      } else {
        a.matches0[out] = t.i;
        a.scores0[out] = t.i >= 0 ? t.v : 0.0f;
      }
    }
  }
}

__global__ __launch_bounds__(DS_THREADS) void k_ds_decide(const int32_t* __restrict__ off0, int n0,
                                                          const int32_t* __restrict__ off1, int n1,
                                                          const int32_t* __restrict__ grids0,
                                                          const int32_t* __restrict__ grids1, int max_k0, int max_k1,
                                                          float threshold, int border, int32_t* __restrict__ matches0,
                                                          const float* __restrict__ scores0,
                                                          const int32_t* __restrict__ m1, int32_t* __restrict__ counts) {
  __shared__ int s_over[DS_THREADS / 64], s_kept[DS_THREADS / 64];
  const int p = (int)blockIdx.x, tid = (int)threadIdx.x;
  int32_t* c = counts + (size_t)p * DS_COUNTERS;
  const DsRange r0 = ds_range(off0, p, n0), r1 = ds_range(off1, p, n1);
  const DsGrid g0 = ds_grid(grids0, p), g1 = ds_grid(grids1, p);
  const int K0 = r0.e - r0.s, K1 = r1.e - r1.s;
  if (!ds_vouched(K0, K1, max_k0, max_k1, g0, g1)) {                // uniform: not matched
    if (tid == 0) c[0] = c[1] = c[2] = c[3] = -1;
    return;
  }
  int over = 0, kept = 0;
  for (int i = tid; i < K0; i += DS_THREADS) {
    const size_t row = (size_t)r0.s + (size_t)i;
    const int j = matches0[row];
    bool pass = (unsigned)j < (unsigned)K1;                         // before j forms an address; K1 >= 1: g1.w >= 1
    pass = pass && scores0[row] > threshold && ds::inside(i, g0.h, g0.w, border) && ds::inside(j, g1.h, g1.w, border);
    const bool keep = pass && m1[(size_t)r1.s + (size_t)j] == i;
    if (!keep) matches0[row] = -1;
    over += pass ? 1 : 0;
    kept += keep ? 1 : 0;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    over += __shfl_xor(over, d, 64);
    kept += __shfl_xor(kept, d, 64);
  }
  if ((tid & 63) == 0) s_over[tid >> 6] = over, s_kept[tid >> 6] = kept;
  __syncthreads();
  if (tid == 0) {
    over = kept = 0;
#pragma unroll
    for (int w = 0; w < DS_THREADS / 64; ++w) over += s_over[w], kept += s_kept[w];
    c[0] = K0, c[1] = K1, c[2] = over, c[3] = kept;
  }
}

namespace {

constexpr const char* ME = "oetr_dual_softmax_match";

bool ds_aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

int ds_tiles(int max_k) { return max_k < 1 ? 1 : (int)(((int64_t)max_k + DS_QT - 1) / DS_QT); }

size_t ds_padded(size_t bytes) { return (bytes + 255) / 256 * 256; }

size_t ds_stats_bytes(int64_t n) { return n < 1 ? 0 : ds_padded((size_t)n * sizeof(float2)); }

}  // namespace
}  // namespace oetr

using namespace oetr;

extern "C" {

int oetr_dual_softmax_abi_version(void) { return OETR_DUAL_SOFTMAX_ABI_VERSION; }

size_t oetr_dual_softmax_workspace_bytes(int64_t n_tok0, int64_t n_tok1) {
  return ds_stats_bytes(n_tok0) + ds_stats_bytes(n_tok1) +
         (n_tok1 < 1 ? 0 : ds_padded((size_t)n_tok1 * sizeof(int32_t)));
}

// The host code dereferences none of its pointer arguments and reads nothing from the device.
oetr_status oetr_dual_softmax_match(const float* feat0, const int32_t* off0, const int32_t* grids0, int64_t n_tok0,
                                    const float* feat1, const int32_t* off1, const int32_t* grids1, int64_t n_tok1,
                                    int n_pairs, int D, int max_k0, int max_k1, float scale, float threshold,
                                    int border_rm, int cell, void* workspace, size_t workspace_bytes,
                                    int32_t* matches0, float* scores0, int32_t* matches1, float* keypoints0,
                                    float* keypoints1, int32_t* counts, void* stream) {
  if (!off0 || !off1) return entry_fail(ME, OETR_ERR_BAD_ARG, "NULL off0 / off1 pointer");
  if (!grids0 || !grids1) return entry_fail(ME, OETR_ERR_BAD_ARG, "NULL grids0 / grids1 pointer");
  if (!counts) return entry_fail(ME, OETR_ERR_BAD_ARG, "NULL counts output");
  if (n_pairs <= 0) return entry_fail(ME, OETR_ERR_BAD_ARG, "need n_pairs > 0");
  if (n_tok0 < 0 || n_tok1 < 0) return entry_fail(ME, OETR_ERR_BAD_ARG, "need n_tok0 >= 0 and n_tok1 >= 0");
  if (max_k0 < 0 || max_k1 < 0) return entry_fail(ME, OETR_ERR_BAD_ARG, "need max_k0 >= 0 and max_k1 >= 0");
  if (D < OETR_DUAL_SOFTMAX_MIN_D || D > OETR_DUAL_SOFTMAX_MAX_D || D % 4 != 0)
    return entry_fail(ME, OETR_ERR_BAD_ARG, "need D % 4 == 0 and 4 <= D <= 512, got " + std::to_string(D));
  if (!std::isfinite(scale) || !(scale > 0.0f))
    return entry_fail(ME, OETR_ERR_BAD_ARG, "need a finite scale > 0, got " + std::to_string(scale));
  if (!std::isfinite(threshold) || !(threshold >= 0.0f))
    return entry_fail(ME, OETR_ERR_BAD_ARG, "need a finite threshold >= 0, got " + std::to_string(threshold));
  if (border_rm < 0) return entry_fail(ME, OETR_ERR_BAD_ARG, "need border_rm >= 0");
  if (cell < 1) return entry_fail(ME, OETR_ERR_BAD_ARG, "need cell >= 1");
  if (n_tok0 != 0 && (!feat0 || !matches0 || !scores0 || !keypoints0))
    return entry_fail(ME, OETR_ERR_BAD_ARG, "NULL feat0 / matches0 / scores0 / keypoints0 pointer");
  if (n_tok1 != 0 && (!feat1 || !keypoints1)) return entry_fail(ME, OETR_ERR_BAD_ARG, "NULL feat1 / keypoints1 pointer");
  if ((n_tok0 != 0 || n_tok1 != 0) && !workspace)
    return entry_fail(ME, OETR_ERR_BAD_ARG, "NULL workspace (the maxima and sums of every token live there)");
  if (!ds_aligned(feat0, 16) || !ds_aligned(feat1, 16))
    return entry_fail(ME, OETR_ERR_BAD_ARG, "feature rows must be 16-byte aligned");
  if (!ds_aligned(workspace, 8) || !ds_aligned(keypoints0, 8) || !ds_aligned(keypoints1, 8))
    return entry_fail(ME, OETR_ERR_BAD_ARG, "workspace / keypoints0 / keypoints1 must be 8-byte aligned");
  if (!ds_aligned(matches0, 4) || !ds_aligned(scores0, 4) || !ds_aligned(matches1, 4) || !ds_aligned(counts, 4) ||
      !ds_aligned(off0, 4) || !ds_aligned(off1, 4) || !ds_aligned(grids0, 4) || !ds_aligned(grids1, 4))
    return entry_fail(ME, OETR_ERR_BAD_ARG, "off / grids / matches0 / scores0 / matches1 / counts must be 4-byte aligned");
  if (n_pairs > INT32_MAX / DS_COUNTERS)
    return entry_fail(ME, OETR_ERR_BAD_SHAPE, "need n_pairs <= " + std::to_string(INT32_MAX / DS_COUNTERS));
  if (n_tok0 > (int64_t)INT32_MAX || n_tok1 > (int64_t)INT32_MAX)
    return entry_fail(ME, OETR_ERR_BAD_SHAPE, "need n_tok0, n_tok1 <= " + std::to_string(INT32_MAX) + " (the offsets are int32)");
  const int t0 = ds_tiles(max_k0), t1 = ds_tiles(max_k1);
  const int64_t groups = (int64_t)n_pairs * ((int64_t)t0 + (int64_t)t1);
  if (groups > (int64_t)INT32_MAX)
    return entry_fail(ME, OETR_ERR_BAD_SHAPE, std::to_string(groups) + " workgroups (n_pairs * tiles of 64 rows of max_k0 "
                                            "and max_k1): need <= " + std::to_string(INT32_MAX) + "; split the call");
  const size_t need = ds_stats_bytes(n_tok0) + ds_stats_bytes(n_tok1) +
                      (matches1 || n_tok1 < 1 ? 0 : ds_padded((size_t)n_tok1 * sizeof(int32_t)));
  if (workspace_bytes < need)
    return entry_fail(ME, OETR_ERR_WORKSPACE, "workspace of " + std::to_string(workspace_bytes) + " bytes, need " +
                                            std::to_string(need));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int n0 = (int)n_tok0, n1 = (int)n_tok1;
  char* ws = static_cast<char*>(workspace);
  DsArgs a;
  a.stats[0] = reinterpret_cast<float2*>(ws);
  a.stats[1] = reinterpret_cast<float2*>(ws + ds_stats_bytes(n_tok0));
  int32_t* m1 = matches1 ? matches1 : reinterpret_cast<int32_t*>(ws + ds_stats_bytes(n_tok0) + ds_stats_bytes(n_tok1));
  const int64_t most = n_tok0 > n_tok1 ? n_tok0 : n_tok1;
  const int64_t clear_groups = (most + DS_THREADS - 1) / DS_THREADS;
  hipLaunchKernelGGL(k_ds_clear, dim3((unsigned)(clear_groups < 1 ? 1 : (clear_groups > 4096 ? 4096 : clear_groups))),
                     dim3(DS_THREADS), 0, s, matches0, scores0, reinterpret_cast<float2*>(keypoints0), n0, m1,
                     reinterpret_cast<float2*>(keypoints1), n1);
  if (oetr_status rc = entry_hip(ME, hipGetLastError(), "k_ds_clear")) return rc;
  a.feat[0] = feat0, a.feat[1] = feat1;
  a.off[0] = off0, a.off[1] = off1;
  a.grids[0] = grids0, a.grids[1] = grids1;
  a.n[0] = n0, a.n[1] = n1;
  a.max_k[0] = max_k0, a.max_k[1] = max_k1;
  a.tiles[0] = t0, a.tiles[1] = t1;
  a.D = D, a.cell = cell;
  a.scale = scale;
  a.keypoints[0] = keypoints0, a.keypoints[1] = keypoints1;
  a.matches0 = matches0, a.scores0 = scores0, a.m1 = m1;
  hipLaunchKernelGGL(k_ds_sweep<1>, dim3((unsigned)groups), dim3(DS_THREADS), 0, s, a);
  if (oetr_status rc = entry_hip(ME, hipGetLastError(), "k_ds_sweep<1>")) return rc;
  hipLaunchKernelGGL(k_ds_sweep<2>, dim3((unsigned)groups), dim3(DS_THREADS), 0, s, a);
  if (oetr_status rc = entry_hip(ME, hipGetLastError(), "k_ds_sweep<2>")) return rc;
  hipLaunchKernelGGL(k_ds_sweep<3>, dim3((unsigned)groups), dim3(DS_THREADS), 0, s, a);
  if (oetr_status rc = entry_hip(ME, hipGetLastError(), "k_ds_sweep<3>")) return rc;
  hipLaunchKernelGGL(k_ds_decide, dim3((unsigned)n_pairs), dim3(DS_THREADS), 0, s, off0, n0, off1, n1, grids0, grids1,
                     max_k0, max_k1, threshold, border_rm, matches0, scores0, m1, counts);
  return entry_hip(ME, hipGetLastError(), "k_ds_decide");
}

}  // extern "C"
