// Nearest-neighbour matching of descriptor sets (include/oetr_nn_match.h): the reference's find_nn / mutual_check /
// NearestNeighbor (dloc/core/matchers/nearest_neighbor.py) for all pairs of a call, bit for bit the numpy program
// tests/nn_match_oracle.py.  No similarity matrix goes to global memory.
//
// Three launches, ordered by the launch boundary alone (no workgroup waits on another):
//   k_nn_clear    every row of matches0 / scores0 / direction 1's matches reads -1 / 0: the rows no pair owns and the
//                 rows of the pairs beyond max_k0 / max_k1 keep that.
//   k_nn_top2     one workgroup = one pair, one direction, 64 query rows.  It walks the other side in tiles of 128 key
//                 rows and D in steps of 64 columns staged through LDS; wave (qh, kh) of the four owns the 32 query
//                 rows qh and the 64 key rows kh of the tile as two 32x32 accumulators of v_mfma_f32_32x32x2_f32, with
//                 the KEYS as the A operand: an accumulator then has its query on the lane and 16 keys in its
//                 registers, so a lane keeps the running top two of ITS query with no lane traffic.  Each (i, j)
//                 accumulator is fed by ONE chain over ascending d (the MFMA's two k slots are d, d + 1; the steps over
//                 D run in order into the same registers): the similarity is the specification's fmaf chain, and
//                 direction 1 - the same kernel with the sides swapped - recomputes bit-equal values because fmaf
//                 commutes.  The running top two live under the order (value descending, index ascending), which makes
//                 the merge across the two lane halves and the two key waves independent of the order of the walk.
//                 Reducing both directions from one tile would halve the FLOPs; it needs a top two per COLUMN across
//                 workgroups and is not built.
//   k_nn_mutual   one workgroup per pair: the mutual check in place on matches0 (a row reads its own entry and
//                 direction 1's matches only) and the pair's four counters.
//
// Nothing is dereferenced on the strength of device data alone: nn_range clamps the offsets into [0, n], a pair
// beyond max_k0 / max_k1 is left before any row is read, rows are loaded and written below the clamped K only, and a
// match index passes ONE unsigned compare against K1 before it forms an address.
#include <string>

#include "../../include/oetr_nn_match.h"
#include "common.h"

namespace oetr {

constexpr int NN_THREADS = 256;
constexpr int NN_QT = 64;            // query rows of a workgroup
constexpr int NN_KT = 128;           // key rows of a tile
constexpr int NN_DC = 64;            // columns of D per staging step
// An odd row stride: the 32 rows that one lane group of a ds_read_b32 reads at one column fall into 32 banks.
constexpr int NN_LD = NN_DC + 1;
constexpr int NN_COUNTERS = OETR_NN_MATCH_COUNTERS;
constexpr unsigned NN_FLAGS = OETR_NN_MATCH_RATIO | OETR_NN_MATCH_DISTANCE | OETR_NN_MATCH_MUTUAL;

using nn_f32x16 = __attribute__((ext_vector_type(16))) float;

struct NnRange {
  int s, e;
};

// rows off[p] .. off[p+1]-1, clamped: 0 <= s <= e <= n whatever the device holds
__device__ __forceinline__ NnRange nn_range(const int32_t* __restrict__ off, int p, int n) {
  int s = off[p], e = off[p + 1];
  s = s < 0 ? 0 : (s > n ? n : s);
  e = e < s ? s : (e > n ? n : e);
  return {s, e};
}

// The running top two of one query: b1 the largest candidate, i1 the lowest index that attains it (-1: none yet),
// b2 the second largest counting multiplicity.
struct NnTop {
  float b1, b2;
  int i1;
};

__device__ __forceinline__ NnTop nn_empty() { return {-INFINITY, -INFINITY, -1}; }

// one more similarity; NaN and -inf are no candidates
__device__ __forceinline__ void nn_push(NnTop& t, float s, int j) {
  if (!(s > -INFINITY)) return;
  if (s > t.b1 || (s == t.b1 && j < t.i1)) {
    t.b2 = t.b1;
    t.b1 = s;
    t.i1 = j;
  } else if (s > t.b2) {
    t.b2 = s;
  }
}

// The top two of the union of two disjoint key sets.  An empty side (i1 = -1, b1 = -inf) loses every comparison: its
// index is the largest unsigned number.
__device__ __forceinline__ NnTop nn_merge(const NnTop& a, const NnTop& b) {
  const bool a_first = a.b1 > b.b1 || (a.b1 == b.b1 && (unsigned)a.i1 < (unsigned)b.i1);
  const NnTop& w = a_first ? a : b;
  const NnTop& l = a_first ? b : a;
  return {w.b1, w.b2 > l.b1 ? w.b2 : l.b1, w.i1};
}

// find_nn of the specification in float32, one rounding per operation
__device__ __forceinline__ void nn_decide(const NnTop& t, unsigned flags, float ratio_sq, float distance_sq, int& m,
                                          float& score) {
#pragma clang fp contract(off)
  const float d0 = 2.0f * (1.0f - t.b1), d1 = 2.0f * (1.0f - t.b2);
  bool mask = t.i1 >= 0;
  if (flags & OETR_NN_MATCH_RATIO) {
    const float bound = ratio_sq * d1;
    mask = mask && d0 <= bound;
  }
  if (flags & OETR_NN_MATCH_DISTANCE) mask = mask && d0 <= distance_sq;
  const float half = (t.b1 + 1.0f) / 2.0f;
  m = mask ? t.i1 : -1;
  score = mask ? half : 0.0f;
}

struct NnArgs {
  const float* desc[2];
  const int32_t* off[2];
  int n[2], max_k[2], tiles[2];
  int D;
  unsigned flags;
  float ratio_sq, distance_sq;
  int32_t* matches0;
  float* scores0;
  int32_t* m1;
};

__global__ __launch_bounds__(NN_THREADS) void k_nn_clear(int32_t* __restrict__ matches0, float* __restrict__ scores0,
                                                         int n0, int32_t* __restrict__ m1, int n1) {
  const int64_t step = (int64_t)gridDim.x * NN_THREADS;
  for (int64_t r = (int64_t)blockIdx.x * NN_THREADS + threadIdx.x; r < (int64_t)n0; r += step) {
    matches0[r] = -1;
    scores0[r] = 0.0f;
  }
  for (int64_t r = (int64_t)blockIdx.x * NN_THREADS + threadIdx.x; r < (int64_t)n1; r += step) m1[r] = -1;
}

// ROWS x NN_DC floats of the rows row0 .. of a side (g: the side's first row of the pair, K its rows) from column d0 on,
// as ROWS / 16 float4 per thread; rows from K on and columns from D on read 0
template <int ROWS>
__device__ __forceinline__ void nn_fetch(float4 (&v)[ROWS / 16], const float* __restrict__ g, int K, int row0, int D,
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
__device__ __forceinline__ void nn_store(float* __restrict__ s, const float4 (&v)[ROWS / 16], int tid) {
#pragma unroll
  for (int i = 0; i < ROWS / 16; ++i) {
    float* dst = s + ((tid >> 4) + 16 * i) * NN_LD + 4 * (tid & 15);
    dst[0] = v[i].x, dst[1] = v[i].y, dst[2] = v[i].z, dst[3] = v[i].w;
  }
}

// Three workgroups per CU, as many as the LDS holds: held to 168 registers the kernel spills 8 bytes per lane, and
// the probe's cells ran 11.43 -> 10.35 ms and 6.64 -> 5.87 ms against the two workgroups of the free allocation
// (138 VGPRs + 65 AGPRs; one run of tools/nn_match_probe.py per build).
__global__ __launch_bounds__(NN_THREADS, 3) void k_nn_top2(const NnArgs a) {
  __shared__ float s_q[NN_QT * NN_LD];
  __shared__ float s_k[NN_KT * NN_LD];
  __shared__ float s_b1[2][NN_QT], s_b2[2][NN_QT];
  __shared__ int s_i1[2][NN_QT];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int per_pair = a.tiles[0] + a.tiles[1];
  const int p = (int)(blockIdx.x / (unsigned)per_pair);
  const int rem = (int)(blockIdx.x - (unsigned)p * (unsigned)per_pair);
  const int dir = rem >= a.tiles[0] ? 1 : 0;                        // direction 1: side 1 asks, side 0 answers
  const int q0 = (dir ? rem - a.tiles[0] : rem) * NN_QT;
  const NnRange r0 = nn_range(a.off[0], p, a.n[0]), r1 = nn_range(a.off[1], p, a.n[1]);
  if (r0.e - r0.s > a.max_k[0] || r1.e - r1.s > a.max_k[1]) return;   // not vouched for: nothing of it is read
  const NnRange rq = dir ? r1 : r0, rk = dir ? r0 : r1;
  const int Kq = rq.e - rq.s, Kk = rk.e - rk.s, D = a.D;
  if (q0 >= Kq) return;                                             // uniform: before any barrier
  const float* gq = a.desc[dir] + (size_t)rq.s * (size_t)D;
  const float* gk = a.desc[dir ^ 1] + (size_t)rk.s * (size_t)D;

  const int r = lane & 31, h = lane >> 5, qh = wave & 1, kh = wave >> 1;
  const float* lq = s_q + (qh * 32 + r) * NN_LD + h;                // column d of the step: k slot h of MFMA d / 2
  const float* lk = s_k + (kh * 64 + r) * NN_LD + h;
  NnTop top = nn_empty();
  nn_f32x16 acc0 = {}, acc1 = {};
  const int chunks = (D + NN_DC - 1) / NN_DC;
  const int steps = ((Kk + NN_KT - 1) / NN_KT) * chunks;            // (key tile, chunk of D), the chunks in order
  float4 vq[NN_QT / 16], vk[NN_KT / 16];
  if (steps > 0) {
    nn_fetch<NN_QT>(vq, gq, Kq, q0, D, 0, tid);
    nn_fetch<NN_KT>(vk, gk, Kk, 0, D, 0, tid);
  }
  int kt = 0, c = 0;
  for (int s = 0; s < steps; ++s) {
    nn_store<NN_QT>(s_q, vq, tid);
    nn_store<NN_KT>(s_k, vk, tid);
    __syncthreads();
    const int len = D - c * NN_DC < NN_DC ? D - c * NN_DC : NN_DC;   // a multiple of 4
    const bool last_chunk = c == chunks - 1;
    const int k0 = kt * NN_KT;
    if (last_chunk) c = 0, ++kt; else ++c;
    if (s + 1 < steps) {                                            // the next step's rows, in flight under the MFMAs
      nn_fetch<NN_QT>(vq, gq, Kq, q0, D, c * NN_DC, tid);
      nn_fetch<NN_KT>(vk, gk, Kk, kt * NN_KT, D, c * NN_DC, tid);
    }
    if (k0 + kh * 64 < Kk) {                                        // wave-uniform: this wave's key rows exist
      auto two_columns = [&](int d) {
        const float q = lq[d];
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(lk[d], q, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(lk[32 * NN_LD + d], q, acc1, 0, 0, 0);
      };
      if (len == NN_DC) {
#pragma unroll
        for (int d = 0; d < NN_DC; d += 2) two_columns(d);
      } else {
        for (int d = 0; d < len; d += 4) two_columns(d), two_columns(d + 2);
      }
    }
    if (last_chunk) {                                               // the tile's similarities are complete
      const int j0 = k0 + kh * 64 + 4 * h;
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        const int j = j0 + (g & 3) + 8 * (g >> 2);                  // the accumulator's row: (g & 3) + 8 (g >> 2) + 4 h
        if (j < Kk) nn_push(top, acc0[g], j);
        if (j + 32 < Kk) nn_push(top, acc1[g], j + 32);
      }
      acc0 = nn_f32x16{};
      acc1 = nn_f32x16{};
    }
    __syncthreads();
  }
  // the query's other lane half, then the other key wave
  NnTop other = {__shfl_xor(top.b1, 32, 64), __shfl_xor(top.b2, 32, 64), __shfl_xor(top.i1, 32, 64)};
  top = nn_merge(top, other);
  if (h == 0) {
    const int q = qh * 32 + r;
    s_b1[kh][q] = top.b1, s_b2[kh][q] = top.b2, s_i1[kh][q] = top.i1;
  }
  __syncthreads();
  if (tid < NN_QT && q0 + tid < Kq) {
    const NnTop t = nn_merge(NnTop{s_b1[0][tid], s_b2[0][tid], s_i1[0][tid]},
                             NnTop{s_b1[1][tid], s_b2[1][tid], s_i1[1][tid]});
    int m;
    float score;
    nn_decide(t, a.flags, a.ratio_sq, a.distance_sq, m, score);
    const size_t row = (size_t)rq.s + (size_t)(q0 + tid);           // < n of the asking side
    if (dir) {
      a.m1[row] = m;
    } else {
      a.matches0[row] = m;
      a.scores0[row] = score;
    }
  }
}

__global__ __launch_bounds__(NN_THREADS) void k_nn_mutual(const int32_t* __restrict__ off0, int n0,
                                                          const int32_t* __restrict__ off1, int n1, int max_k0,
                                                          int max_k1, unsigned flags, int32_t* __restrict__ matches0,
                                                          const int32_t* __restrict__ m1, int32_t* __restrict__ counts) {
  __shared__ int s_pass[NN_THREADS / 64], s_kept[NN_THREADS / 64];
  const int p = (int)blockIdx.x, tid = (int)threadIdx.x;
  int32_t* c = counts + (size_t)p * NN_COUNTERS;
  const NnRange r0 = nn_range(off0, p, n0), r1 = nn_range(off1, p, n1);
  const int K0 = r0.e - r0.s, K1 = r1.e - r1.s;
  if (K0 > max_k0 || K1 > max_k1) {                                 // uniform: not vouched for
    if (tid == 0) c[0] = c[1] = c[2] = c[3] = -1;
    return;
  }
  const bool mutual = (flags & OETR_NN_MATCH_MUTUAL) != 0;
  int pass = 0, kept = 0;
  for (int i = tid; i < K0; i += NN_THREADS) {
    const size_t row = (size_t)r0.s + (size_t)i;
    const int m = matches0[row];
    const bool ok = (unsigned)m < (unsigned)K1;                     // before m forms an address
    bool keep = ok;
    if (mutual && ok) {
      keep = m1[(size_t)r1.s + (size_t)m] == i;
      if (!keep) matches0[row] = -1;
    }
    pass += ok ? 1 : 0;
    kept += keep ? 1 : 0;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    pass += __shfl_xor(pass, d, 64);
    kept += __shfl_xor(kept, d, 64);
  }
  if ((tid & 63) == 0) s_pass[tid >> 6] = pass, s_kept[tid >> 6] = kept;
  __syncthreads();
  if (tid == 0) {
    pass = kept = 0;
#pragma unroll
    for (int w = 0; w < NN_THREADS / 64; ++w) pass += s_pass[w], kept += s_kept[w];
    c[0] = K0, c[1] = K1, c[2] = pass, c[3] = kept;
  }
}

namespace {

constexpr const char* ME = "oetr_nn_match";

bool nn_aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

int nn_tiles(int max_k) { return max_k < 1 ? 1 : (int)(((int64_t)max_k + NN_QT - 1) / NN_QT); }

}  // namespace
}  // namespace oetr

using namespace oetr;

extern "C" {

int oetr_nn_match_abi_version(void) { return OETR_NN_MATCH_ABI_VERSION; }

size_t oetr_nn_match_workspace_bytes(int64_t n_kp1) {
  if (n_kp1 < 1) return 0;
  return (((size_t)n_kp1 * sizeof(int32_t)) + 255) / 256 * 256;
}

// The host code dereferences none of its pointer arguments and reads nothing from the device.
oetr_status oetr_nn_match(const float* desc0, const int32_t* off0, int64_t n_kp0, const float* desc1,
                          const int32_t* off1, int64_t n_kp1, int n_pairs, int D, int max_k0, int max_k1,
                          float ratio_sq, float distance_sq, unsigned flags, void* workspace, size_t workspace_bytes,
                          int32_t* matches0, float* scores0, int32_t* matches1, int32_t* counts, void* stream) {
  if (!off0 || !off1) return entry_fail(ME, OETR_ERR_BAD_ARG, "NULL off0 / off1 pointer");
  if (!counts) return entry_fail(ME, OETR_ERR_BAD_ARG, "NULL counts output");
  if (n_pairs <= 0) return entry_fail(ME, OETR_ERR_BAD_ARG, "need n_pairs > 0");
  if (n_kp0 < 0 || n_kp1 < 0) return entry_fail(ME, OETR_ERR_BAD_ARG, "need n_kp0 >= 0 and n_kp1 >= 0");
  if (max_k0 < 0 || max_k1 < 0) return entry_fail(ME, OETR_ERR_BAD_ARG, "need max_k0 >= 0 and max_k1 >= 0");
  if (D < OETR_NN_MATCH_MIN_D || D > OETR_NN_MATCH_MAX_D || D % 4 != 0)
    return entry_fail(ME, OETR_ERR_BAD_ARG, "need D % 4 == 0 and 4 <= D <= 512, got " + std::to_string(D));
  if (flags & ~NN_FLAGS) return entry_fail(ME, OETR_ERR_BAD_ARG, "unknown flag bits in " + std::to_string(flags));
  if (n_kp0 != 0 && (!desc0 || !matches0 || !scores0))
    return entry_fail(ME, OETR_ERR_BAD_ARG, "NULL desc0 / matches0 / scores0 pointer");
  if (n_kp1 != 0 && !desc1) return entry_fail(ME, OETR_ERR_BAD_ARG, "NULL desc1 pointer");
  if (n_kp1 != 0 && !matches1 && !workspace)
    return entry_fail(ME, OETR_ERR_BAD_ARG, "NULL workspace (direction 1's matches need it, or a matches1 output)");
  if (!nn_aligned(desc0, 16) || !nn_aligned(desc1, 16))
    return entry_fail(ME, OETR_ERR_BAD_ARG, "descriptor rows must be 16-byte aligned");
  if (!nn_aligned(matches0, 4) || !nn_aligned(scores0, 4) || !nn_aligned(matches1, 4) || !nn_aligned(counts, 4) ||
      !nn_aligned(workspace, 4))
    return entry_fail(ME, OETR_ERR_BAD_ARG, "matches0 / scores0 / matches1 / counts / workspace must be 4-byte aligned");
  if (n_pairs > INT32_MAX / NN_COUNTERS)
    return entry_fail(ME, OETR_ERR_BAD_SHAPE, "need n_pairs <= " + std::to_string(INT32_MAX / NN_COUNTERS));
  if (n_kp0 > (int64_t)INT32_MAX || n_kp1 > (int64_t)INT32_MAX)
    return entry_fail(ME, OETR_ERR_BAD_SHAPE, "need n_kp0, n_kp1 <= " + std::to_string(INT32_MAX) + " (the offsets are int32)");
  const int t0 = nn_tiles(max_k0), t1 = nn_tiles(max_k1);
  const int64_t groups = (int64_t)n_pairs * ((int64_t)t0 + (int64_t)t1);
  if (groups > (int64_t)INT32_MAX)
    return entry_fail(ME, OETR_ERR_BAD_SHAPE, std::to_string(groups) + " workgroups (n_pairs * tiles of 64 rows of max_k0 "
                                            "and max_k1): need <= " + std::to_string(INT32_MAX) + "; split the call");
  if (n_kp1 != 0 && !matches1 && workspace_bytes < oetr_nn_match_workspace_bytes(n_kp1))
    return entry_fail(ME, OETR_ERR_WORKSPACE, "workspace of " + std::to_string(workspace_bytes) + " bytes, need " +
                                            std::to_string(oetr_nn_match_workspace_bytes(n_kp1)));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int n0 = (int)n_kp0, n1 = (int)n_kp1;
  int32_t* m1 = matches1 ? matches1 : static_cast<int32_t*>(workspace);
  const int64_t most = n_kp0 > n_kp1 ? n_kp0 : n_kp1;
  const int64_t clear_groups = (most + NN_THREADS - 1) / NN_THREADS;
  hipLaunchKernelGGL(k_nn_clear, dim3((unsigned)(clear_groups < 1 ? 1 : (clear_groups > 4096 ? 4096 : clear_groups))),
                     dim3(NN_THREADS), 0, s, matches0, scores0, n0, m1, n1);
  if (oetr_status rc = entry_hip(ME, hipGetLastError(), "k_nn_clear")) return rc;
  NnArgs a;
  a.desc[0] = desc0, a.desc[1] = desc1;
  a.off[0] = off0, a.off[1] = off1;
  a.n[0] = n0, a.n[1] = n1;
  a.max_k[0] = max_k0, a.max_k[1] = max_k1;
  a.tiles[0] = t0, a.tiles[1] = t1;
  a.D = D;
  a.flags = flags;
  a.ratio_sq = ratio_sq, a.distance_sq = distance_sq;
  a.matches0 = matches0, a.scores0 = scores0, a.m1 = m1;
  hipLaunchKernelGGL(k_nn_top2, dim3((unsigned)groups), dim3(NN_THREADS), 0, s, a);
  if (oetr_status rc = entry_hip(ME, hipGetLastError(), "k_nn_top2")) return rc;
  hipLaunchKernelGGL(k_nn_mutual, dim3((unsigned)n_pairs), dim3(NN_THREADS), 0, s, off0, n0, off1, n1, max_k0, max_k1,
                     flags, matches0, m1, counts);
  return entry_hip(ME, hipGetLastError(), "k_nn_mutual");
}

}  // extern "C"
