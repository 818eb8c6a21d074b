// The box -> crop step for a whole chunk of pairs in one call (include/oetr_crop_batch.h), gfx950.
//
// crop.hip crops one pair with three launches; here n pairs of mixed image sizes are cropped by
//
//   k_crop_batch_geometry        one THREAD per pair: crop_geometry (crop_sample.h) -> info[k]
//   k_crop_batch_resize<1>       one launch for the batch: crop x255 -> bicubic -> tmp, or - for a side
//                                whose out size equals its new size (always when size_divisor == 1) -
//                                -> /255 -> out directly; the pass-through copy of a failed gate
//   k_crop_batch_resize<2>       only when size_divisor > 1: tmp -> bicubic -> /255 -> out for the
//                                sides pass 1 did not finish
//
// so a call is 2 launches for size_divisor == 1 and 3 otherwise, whatever n is.  Skipping the second
// resize of an equal-size side changes nothing: its cubic weights are exactly (0, 1, 0, 0), so crop.hip's
// second pass hands every finite value through and divides it by 255 - which pass 1 does here.
//
// Grid of a resize pass: x, y = 64 x 16 output tiles over the call's capacity, z = pair * 2 + side.  The
// sizes are data dependent, so every wave first reads its pair's record and table entry (the addresses
// depend on blockIdx alone: scalar loads) and leaves when its tile lies outside the side's size.  A wave
// is one row of 64 adjacent output pixels (coalesced stores); a thread takes 4 rows of one column and all
// channels, so the source column, the x weights and the two double steps sw/dw and sh/dh - wave-uniform
// quotients - are formed once per thread and serve 4 * channels pixels: no integer division and no
// double division per pixel.  The 16 taps of a pixel come out of L1 / L2 (neighbouring lanes read
// neighbouring or the same source pixels).
//
// info[k] is also the plan of the resize passes (origin, source and destination sizes): nothing private is
// kept in the caller's buffers, whose slots a crop may fill completely.
#include "../../include/oetr_crop_batch.h"
#include "common.h"
#include "crop_sample.h"

namespace oetr {

constexpr int CROP_TILE_W = 64, CROP_TILE_H = 16, CROP_ROWS = 4;   // 256 threads: 64 columns x 4 rows, 4 rows each

struct CropBatchLaunch {
  const oetr_crop_pair* pairs;
  int n, channels, max_h, max_w;
  const float* box[2];      // device [n][4]
  int keep_aspect, size_divisor, gate_mode;
  float* tmp;               // [n][2][capacity] or NULL
  float* out;               // [n][2][capacity]
  size_t capacity;          // floats per slot
  oetr_crop_info* info;     // device [n]
};

// crop_geometry's view of one pair of the table
struct CropBatchPair {
  int h[2], w[2];
  const float* box[2];
  float scale[2][2];
  int keep_aspect, size_divisor, gate_mode;
  int cap_h, cap_w;
};

__global__ __launch_bounds__(64) void k_crop_batch_geometry(CropBatchLaunch p) {
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= p.n) return;
  const oetr_crop_pair pr = p.pairs[k];
  CropBatchPair a;
  bool ok = true;
  for (int i = 0; i < 2; ++i) {
    a.h[i] = pr.h[i]; a.w[i] = pr.w[i];
    a.box[i] = p.box[i] + (size_t)k * 4;
    a.scale[i][0] = pr.scale[i][0]; a.scale[i][1] = pr.scale[i][1];
    if (!pr.image[i] || pr.h[i] < 1 || pr.w[i] < 1 || pr.h[i] > p.max_h || pr.w[i] > p.max_w) ok = false;
  }
  a.keep_aspect = p.keep_aspect; a.size_divisor = p.size_divisor; a.gate_mode = p.gate_mode;
  // the pair's OWN capacity (oetr_overlap_crop_capacity); none for an entry the call's bounds do not cover,
  // which makes the fits test fail: valid = -1
  const int d = p.size_divisor;
  a.cap_h = ok ? ((max(pr.h[0], pr.h[1]) + d - 1) / d) * d : 0;
  a.cap_w = ok ? ((max(pr.w[0], pr.w[1]) + d - 1) / d) * d : 0;
  oetr_crop_info g;
  crop_geometry(a, g);
  p.info[k] = g;
}

template <int PASS>
__global__ __launch_bounds__(256) void k_crop_batch_resize(CropBatchLaunch p) {
  const int k = blockIdx.z >> 1, im = blockIdx.z & 1;
  const oetr_crop_info& g = p.info[k];
  const oetr_crop_pair& pr = p.pairs[k];
  const int C = p.channels;
  const int tile_x = blockIdx.x * CROP_TILE_W, tile_y = blockIdx.y * CROP_TILE_H;
  const int dx = tile_x + (threadIdx.x & 63);
  const int dy0 = tile_y + (threadIdx.x >> 6);
  const size_t slot = ((size_t)k * 2 + im) * p.capacity;
  const int valid = g.valid;
  if (valid != 1) {
    // gate failed: the reference hands data['image0'/'image1'] back untouched - a plain copy, bit for bit
    if (PASS == 1 && valid == 0) {
      const int w = pr.w[im], h = pr.h[im];
      if (tile_x >= w || tile_y >= h || dx >= w) return;
      const float* image = pr.image[im];
      float* dst = p.out + slot;
      for (int r = 0; r < CROP_ROWS; ++r) {
        const int y = dy0 + r * CROP_ROWS;
        if (y >= h) break;
        for (int c = 0; c < C; ++c) {
          const size_t at = ((size_t)c * h + y) * w + dx;
          dst[at] = image[at];
        }
      }
    }
    return;
  }
  const int nw = g.new_w[im], nh = g.new_h[im];
  const bool direct = g.out_w[im] == nw && g.out_h[im] == nh;   // no second resize: pass 1 finishes the side
  int sw, sh, dw, dh, x0, y0, spitch;
  size_t splane;
  const float* src;
  float* dst;
  if (PASS == 1) {
    x0 = min(g.box[im][0], pr.w[im]); y0 = min(g.box[im][1], pr.h[im]);   // >= 0: crop_geometry's box domain
    sw = g.crop_w[im]; sh = g.crop_h[im];
    dw = nw; dh = nh;
    spitch = pr.w[im];
    splane = (size_t)pr.h[im] * pr.w[im];
    src = pr.image[im];
    dst = (direct ? p.out : p.tmp) + slot;
  } else {
    if (direct) return;
    x0 = y0 = 0;
    sw = nw; sh = nh;
    dw = g.out_w[im]; dh = g.out_h[im];
    spitch = sw;
    splane = (size_t)sw * sh;
    src = p.tmp + slot;
    dst = p.out + slot;
  }
  if (tile_x >= dw || tile_y >= dh || dx >= dw || sw <= 0 || sh <= 0) return;
  const double step_x = (double)sw / (double)dw, step_y = (double)sh / (double)dh;
  const float fx = crop_src_coord(dx, step_x);
  const int sx = (int)floorf(fx);
  float wx[4];
  cubic_weights(fx - (float)sx, wx);
  const float in_scale = PASS == 1 ? 255.0f : 1.0f;
  const size_t dplane = (size_t)dw * dh;
  for (int r = 0; r < CROP_ROWS; ++r) {
    const int dy = dy0 + r * CROP_ROWS;
    if (dy >= dh) break;
    const float fy = crop_src_coord(dy, step_y);
    const int sy = (int)floorf(fy);
    float wy[4];
    cubic_weights(fy - (float)sy, wy);
    for (int c = 0; c < C; ++c) {
      const float acc = crop_tap_sum(src + c * splane, spitch, x0, y0, sw, sh, sx, sy, wx, wy, in_scale);
      dst[c * dplane + (size_t)dy * dw + dx] = PASS == 1 && !direct ? acc : acc / 255.0f;
    }
  }
}

hipError_t launch_overlap_crop_batch(const CropBatchLaunch& p, int cap_h, int cap_w, hipStream_t s) {
  hipLaunchKernelGGL(k_crop_batch_geometry, dim3((unsigned)((p.n + 63) / 64)), dim3(64), 0, s, p);
  const dim3 grid((unsigned)((cap_w + CROP_TILE_W - 1) / CROP_TILE_W), (unsigned)((cap_h + CROP_TILE_H - 1) / CROP_TILE_H),
                  (unsigned)p.n * 2);
  hipLaunchKernelGGL((k_crop_batch_resize<1>), grid, dim3(256), 0, s, p);
  if (p.size_divisor > 1) hipLaunchKernelGGL((k_crop_batch_resize<2>), grid, dim3(256), 0, s, p);
  return hipGetLastError();
}

}  // namespace oetr

using namespace oetr;

extern "C" {

int oetr_crop_batch_abi_version(void) { return OETR_CROP_BATCH_ABI_VERSION; }

size_t oetr_crop_batch_capacity(int channels, int max_h, int max_w, int size_divisor, int* cap_h, int* cap_w) {
  if (channels <= 0 || max_h <= 0 || max_w <= 0 || size_divisor < 1) return 0;
  const long d = size_divisor;
  const long ch = ((max_h + d - 1) / d) * d, cw = ((max_w + d - 1) / d) * d;
  if (ch > INT32_MAX || cw > INT32_MAX) return 0;
  if (cap_h) *cap_h = (int)ch;
  if (cap_w) *cap_w = (int)cw;
  return (size_t)channels * (size_t)ch * (size_t)cw;
}

oetr_status oetr_overlap_crop_batch(const oetr_crop_pair* pairs, int n, int channels, int max_h, int max_w,
                                    const float* box1, const float* box2, int keep_aspect, int size_divisor,
                                    int gate_mode, float* tmp, float* out, size_t capacity_floats,
                                    oetr_crop_info* info, void* stream) {
  if (!pairs || !box1 || !box2 || !out || !info)
    return (oetr_status)set_last_error(OETR_ERR_BAD_ARG, "oetr_overlap_crop_batch: NULL argument");
  if (n < 1 || n > OETR_CROP_BATCH_MAX_PAIRS)
    return (oetr_status)set_last_error(OETR_ERR_BAD_ARG, "oetr_overlap_crop_batch: n outside 1..OETR_CROP_BATCH_MAX_PAIRS");
  int cap_h = 0, cap_w = 0;
  const size_t need = oetr_crop_batch_capacity(channels, max_h, max_w, size_divisor, &cap_h, &cap_w);
  if (need == 0 || (gate_mode != 0 && gate_mode != 1))
    return (oetr_status)set_last_error(OETR_ERR_BAD_ARG, "oetr_overlap_crop_batch: bad channels / max size / size_divisor / gate_mode");
  if (!tmp && size_divisor > 1)
    return (oetr_status)set_last_error(OETR_ERR_BAD_ARG, "oetr_overlap_crop_batch: tmp is NULL with size_divisor > 1");
  if (capacity_floats < need)
    return (oetr_status)set_last_error(OETR_ERR_WORKSPACE, "oetr_overlap_crop_batch: slots smaller than oetr_crop_batch_capacity()");
  if ((cap_h + CROP_TILE_H - 1) / CROP_TILE_H > 65535)
    return (oetr_status)set_last_error(OETR_ERR_BAD_ARG, "oetr_overlap_crop_batch: max_h beyond the grid");
  CropBatchLaunch p;
  p.pairs = pairs;
  p.n = n; p.channels = channels; p.max_h = max_h; p.max_w = max_w;
  p.box[0] = box1; p.box[1] = box2;
  p.keep_aspect = keep_aspect; p.size_divisor = size_divisor; p.gate_mode = gate_mode;
  p.tmp = tmp; p.out = out;
  p.capacity = capacity_floats;
  p.info = info;
  const hipError_t e = launch_overlap_crop_batch(p, cap_h, cap_w, static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return (oetr_status)set_last_error(OETR_ERR_HIP, hipGetErrorString(e));
  return OETR_OK;
}

}  // extern "C"
