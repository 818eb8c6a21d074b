// Scoring matches against depth and pose (include/oetr_match_score.h): the reference's compute_epipolar_error,
// get_episym and get_projected_kp + get_truesym for many match lists over a depth-map set, in one call.
//
// k_match_score: one thread per match row, 256-thread workgroups.  The row finds its list (match_list.h), makes the
// vouching test of k_covis_warp_indexed on its pair's two table rows (without max_pixels: the grid is over matches)
// and then runs tests/match_score_oracle.py::score LITERALLY: float64, every operation rounded on its own in the order and with
// the parentheses written there (no contraction into FMAs: rint() and the "<" tests are discontinuous and the
// parity target is a float64 numpy program).  E = [t]x R, m = R^T t and px_thr * px_thr are computed per thread
// with the same individual operations.  Twelve float64 divisions per row.  A wave whose rows all lie in the list of
// its first row - the common case - takes its two indices, two table rows and 20 parameters by scalar loads, as it
// took that list, so that a row's chain of dependent VECTOR loads is its keypoints and its two depth pixels.  (A
// search and the pair's data per lane, 16 dependent vector loads, cost 6.4x a copy of the call's bytes;
// profiles/match_score_probe.json has what this form costs.)  A wave that straddles lists loads per lane.
// Nothing is dereferenced on the strength of device data alone: a row index is below the host's n_matches, a pair
// number inside [0, n_pairs) by construction of the search, a map index tested against n_maps, a depth pixel
// tested in float64 against its row's H, W before the conversion to an integer.
//
// Counters: a wave whose counted rows all belong to one pair takes one ballot and one popcount per flag and
// issues one atomicAdd per non-zero counter; a wave that straddles lists falls back to per-lane atomicAdd.
// Integer atomics commute: the counters do not depend on arrival order.  k_clear_i32 zeroes the counters before,
// k_match_finish (one thread per pair) afterwards writes the list length, -1 for a threshold that is off, and -1 throughout
// for a pair that is not vouched for.
#include <cmath>
#include <string>

#include "../../include/oetr_match_score.h"
#include "common.h"
#include "depth_pose.h"
#include "match_list.h"

namespace oetr {

constexpr int MATCH_THREADS = 256;
constexpr int MATCH_PARAMS = OETR_MATCH_SCORE_PARAM_DOUBLES;
constexpr int MATCH_COUNTERS = OETR_MATCH_SCORE_COUNTERS;

struct MatchRow {
  double epi, sym, r12, r21;
  unsigned flag;
};

// One row of tests/match_score_oracle.py::score under the 20 doubles at P, the two maps of its pair.  The one copy
// of the arithmetic; inlined twice (pair data by scalar loads / by per-lane loads).
__device__ __forceinline__ MatchRow match_row(const oetr_covis_map& ma, const oetr_covis_map& mb,
                                              const double* __restrict__ P, double u1, double v1, double u2,
                                              double v2, double epi_thr, double sym_thr, double px_thr) {
#pragma clang fp contract(off)
  const double fx1 = P[0], fy1 = P[1], cx1 = P[2], cy1 = P[3], fx2 = P[4], fy2 = P[5], cx2 = P[6], cy2 = P[7];
  const double R00 = P[8], R01 = P[9], R02 = P[10], R10 = P[11], R11 = P[12], R12 = P[13], R20 = P[14],
               R21 = P[15], R22 = P[16];
  const double t0 = P[17], t1 = P[18], t2 = P[19];

  const double x1 = (u1 - cx1) / fx1, y1 = (v1 - cy1) / fy1;
  const double x2 = (u2 - cx2) / fx2, y2 = (v2 - cy2) / fy2;
  const double E00 = t1 * R20 - t2 * R10, E01 = t1 * R21 - t2 * R11, E02 = t1 * R22 - t2 * R12;
  const double E10 = t2 * R00 - t0 * R20, E11 = t2 * R01 - t0 * R21, E12 = t2 * R02 - t0 * R22;
  const double E20 = t0 * R10 - t1 * R00, E21 = t0 * R11 - t1 * R01, E22 = t0 * R12 - t1 * R02;
  const double a0 = (E00 * x1 + E01 * y1) + E02;
  const double a1 = (E10 * x1 + E11 * y1) + E12;
  const double a2 = (E20 * x1 + E21 * y1) + E22;
  const double b0 = (E00 * x2 + E10 * y2) + E20;
  const double b1 = (E01 * x2 + E11 * y2) + E21;
  const double s = (x2 * a0 + y2 * a1) + a2;
  const double s2 = s * s;
  MatchRow out;
  out.epi = s2 * (1.0 / (a0 + a1) + 1.0 / (b0 + b1));
  out.sym = s2 * (1.0 / (a0 * a0 + a1 * a1) + 1.0 / (b0 * b0 + b1 * b1));

  // each keypoint under its depth in the other picture (depth_pose.h), against its partner
  const double d1 = depth_at(ma, u1, v1), d2 = depth_at(mb, u2, v2);
  double pu, pv;
  project12(P, u1, v1, d1, pu, pv);
  const double e0 = pu - u2, e1 = pv - v2;
  out.r12 = e0 * e0 + e1 * e1;
  project21(P, u2, v2, d2, pu, pv);
  const double g0 = pu - u1, g1 = pv - v1;
  out.r21 = g0 * g0 + g1 * g1;

  const bool has1 = d1 != 0.0, has2 = d2 != 0.0;
  const bool both = has1 && has2;
  const bool ok_epi = out.epi < epi_thr, ok_sym = out.sym < sym_thr;   // false for a NaN threshold
  const bool ok_px = both && (out.r21 < px_thr * px_thr);
  out.flag = (has1 ? OETR_MATCH_DEPTH1 : 0) | (has2 ? OETR_MATCH_DEPTH2 : 0) | (ok_epi ? OETR_MATCH_EPI : 0) |
             (ok_sym ? OETR_MATCH_EPISYM : 0) | (ok_px ? OETR_MATCH_REPROJ : 0);
  return out;
}

__global__ __launch_bounds__(MATCH_THREADS) void k_match_score(
    const oetr_covis_map* __restrict__ maps, int n_maps, const int32_t* __restrict__ idx1,
    const int32_t* __restrict__ idx2, const double* __restrict__ params, const int32_t* __restrict__ offsets,
    int n_pairs, const float* __restrict__ k1, const float* __restrict__ k2, int n_matches, double epi_thr,
    double sym_thr, double px_thr, double* __restrict__ values, uint8_t* __restrict__ flags,
    int32_t* __restrict__ counts) {
  const int64_t row = (int64_t)blockIdx.x * MATCH_THREADS + (int64_t)threadIdx.x;
  const bool active = row < (int64_t)n_matches;
  const int m = active ? (int)row : 0;

  // the keypoints depend on the row alone: their loads go out before the search
  float u1 = 0.0f, v1 = 0.0f, u2 = 0.0f, v2 = 0.0f;
  if (active) {
    const size_t at = 2 * (size_t)m;
    u1 = k1[at], v1 = k1[at + 1], u2 = k2[at], v2 = k2[at + 1];
  }

  int p0, p;                                                        // the wave's first row's list, this row's
  wave_find_list<MATCH_THREADS>(offsets, n_pairs, n_matches, active, m, p0, p);

  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  MatchRow r = {nan, nan, nan, nan, 0u};
  int counted = -1;                                                 // the pair this row's flags count for, or none
  oetr_covis_map ma, mb;
  if (__ballot(active && p != p0) == 0ull) {
    // every active row of the wave is in list p0: indices, table rows and parameters by scalar loads
    if (p0 >= 0 && pair_maps(maps, n_maps, idx1, idx2, p0, ma, mb) && active) {
      r = match_row(ma, mb, params + (size_t)p0 * MATCH_PARAMS, (double)u1, (double)v1, (double)u2, (double)v2,
                    epi_thr, sym_thr, px_thr);
      counted = p0;
    }
  } else if (p >= 0 && pair_maps(maps, n_maps, idx1, idx2, p, ma, mb)) {
    r = match_row(ma, mb, params + (size_t)p * MATCH_PARAMS, (double)u1, (double)v1, (double)u2, (double)v2, epi_thr,
                  sym_thr, px_thr);
    counted = p;
  }
  const double epi = r.epi, sym = r.sym, r12 = r.r12, r21 = r.r21;
  const unsigned flag = r.flag;

  if (active) {
    if (values) {
      const size_t n = (size_t)n_matches;
      values[(size_t)m] = epi;
      values[n + (size_t)m] = sym;
      values[2 * n + (size_t)m] = r12;
      values[3 * n + (size_t)m] = r21;
    }
    flags[m] = (uint8_t)flag;
  }

  // counters 1..4 (counter 0, the list length, is k_match_finish's).  Every lane of the wave arrives here.
  const bool c_epi = (flag & OETR_MATCH_EPI) != 0, c_sym = (flag & OETR_MATCH_EPISYM) != 0;
  const bool c_both = (flag & 3u) == 3u, c_px = (flag & OETR_MATCH_REPROJ) != 0;
  const WaveCounted w = wave_counted(counted);
  if (!w.any) return;                                               // wave-uniform
  if (w.one_pair) {
    const int n_epi = __popcll(__ballot(c_epi)), n_sym = __popcll(__ballot(c_sym));
    const int n_both = __popcll(__ballot(c_both)), n_px = __popcll(__ballot(c_px));
    if ((threadIdx.x & 63) == 0) {
      int32_t* c = counts + (size_t)w.first * MATCH_COUNTERS;       // 0 <= first < n_pairs
      if (n_epi) atomicAdd(c + 1, n_epi);
      if (n_sym) atomicAdd(c + 2, n_sym);
      if (n_both) atomicAdd(c + 3, n_both);
      if (n_px) atomicAdd(c + 4, n_px);
    }
  } else if (counted >= 0) {
    int32_t* c = counts + (size_t)counted * MATCH_COUNTERS;
    if (c_epi) atomicAdd(c + 1, 1);
    if (c_sym) atomicAdd(c + 2, 1);
    if (c_both) atomicAdd(c + 3, 1);
    if (c_px) atomicAdd(c + 4, 1);
  }
}

// p[0 .. n) = 0, as a kernel of the library's own: see the note on hipMemsetAsync at clear_i32 below
__global__ void k_clear_i32(int32_t* __restrict__ p, int n) {
  const unsigned at = blockIdx.x * blockDim.x + threadIdx.x;
  if (at < (unsigned)n) p[at] = 0;
}

// one thread per pair; the vouching test k_match_score made, made again
__global__ void k_match_finish(const oetr_covis_map* __restrict__ maps, int n_maps, const int32_t* __restrict__ idx1,
                               const int32_t* __restrict__ idx2, const int32_t* __restrict__ offsets, int n_pairs,
                               int n_matches, double epi_thr, double sym_thr, double px_thr,
                               int32_t* __restrict__ counts) {
  const unsigned at = blockIdx.x * blockDim.x + threadIdx.x;
  if (at >= (unsigned)n_pairs) return;
  const int p = (int)at;
  int32_t* c = counts + (size_t)p * MATCH_COUNTERS;
  oetr_covis_map a, b;
  if (!pair_maps(maps, n_maps, idx1, idx2, p, a, b)) {
#pragma unroll
    for (int k = 0; k < MATCH_COUNTERS; ++k) c[k] = -1;
    return;
  }
  c[0] = list_length(offsets, p, n_matches);
  if (epi_thr != epi_thr) c[1] = -1;
  if (sym_thr != sym_thr) c[2] = -1;
  if (px_thr != px_thr) c[4] = -1;
}

// The entries' counters are cleared by a kernel, not by hipMemsetAsync: captured into a HIP graph as a memset node
// (280 bytes for 14 pairs), the clearing wrote a foreign 16-byte pattern over counts on the graph's SECOND replay,
// after device copies had run between the replays (tests/test_gpu_match_score.py, the capture test; the runtime's
// side of it was not examined).  A kernel node carries its arguments with it.  The kernel is launched from the file
// that defines it (the build is not relocatable), so the other entries reach it through this function.
hipError_t clear_i32(int32_t* p, int64_t n, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(k_clear_i32, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p, (int)n);
  return hipGetLastError();
}

namespace {

constexpr const char* ME = "oetr_match_score";

}  // namespace
}  // namespace oetr

using namespace oetr;

extern "C" {

int oetr_match_score_abi_version(void) { return OETR_MATCH_SCORE_ABI_VERSION; }

// The host code dereferences none of its pointer arguments and reads nothing from the device.
oetr_status oetr_match_score(const oetr_covis_map* maps, int n_maps, const int32_t* idx1, const int32_t* idx2,
                             const double* params, const int32_t* offsets, int n_pairs, const float* k1,
                             const float* k2, int64_t n_matches, double epi_thr, double sym_thr, double px_thr,
                             double* values, uint8_t* flags, int32_t* counts, void* stream) {
  if (!maps || !idx1 || !idx2 || !params || !offsets)
    return entry_fail(ME, OETR_ERR_BAD_ARG, "NULL map table / index / parameter / offsets pointer");
  if (!counts) return entry_fail(ME, OETR_ERR_BAD_ARG, "NULL counts output");
  if (n_matches != 0 && (!k1 || !k2)) return entry_fail(ME, OETR_ERR_BAD_ARG, "NULL keypoint pointer");
  if (n_matches != 0 && !flags) return entry_fail(ME, OETR_ERR_BAD_ARG, "NULL flags output");
  if (n_maps <= 0 || n_pairs <= 0) return entry_fail(ME, OETR_ERR_BAD_ARG, "need n_maps > 0 and n_pairs > 0");
  if (n_matches < 0) return entry_fail(ME, OETR_ERR_BAD_ARG, "need n_matches >= 0");
  if (n_pairs > INT32_MAX / MATCH_COUNTERS)
    return entry_fail(ME, OETR_ERR_BAD_SHAPE, "need n_pairs <= " + std::to_string(INT32_MAX / MATCH_COUNTERS));
  if (n_matches > (int64_t)INT32_MAX)
    return entry_fail(ME, OETR_ERR_BAD_SHAPE, "need n_matches <= " + std::to_string(INT32_MAX) + " (the offsets are int32)");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int n = (int)n_matches;
  // n_pairs <= INT32_MAX / 5, checked above
  if (oetr_status rc = entry_hip(ME, clear_i32(counts, (int64_t)n_pairs * MATCH_COUNTERS, s), "k_clear_i32")) return rc;
  if (n > 0) {
    const unsigned blocks = (unsigned)(((int64_t)n + MATCH_THREADS - 1) / MATCH_THREADS);
    hipLaunchKernelGGL(k_match_score, dim3(blocks), dim3(MATCH_THREADS), 0, s, maps, n_maps, idx1, idx2, params,
                       offsets, n_pairs, k1, k2, n, epi_thr, sym_thr, px_thr, values, flags, counts);
    if (oetr_status rc = entry_hip(ME, hipGetLastError(), "k_match_score")) return rc;
  }
  hipLaunchKernelGGL(k_match_finish, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, s, maps, n_maps, idx1,
                     idx2, offsets, n_pairs, n, epi_thr, sym_thr, px_thr, counts);
  return entry_hip(ME, hipGetLastError(), "k_match_finish");
}

}  // extern "C"
