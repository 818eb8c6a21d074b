// Device-side box -> crop step of the matching pipeline, gfx950.
//
// Reference: the overlap branch of Matching.forward (evaluation.py:82-170) and
// tensor_overlap_crop / patch_resize (dloc/core/utils/utils.py:476-564).  There every
// pair round-trips through the host: boxes are read back (.int(), Python slicing), the
// crops go to numpy, cv2.resize(INTER_CUBIC) runs on the CPU and the result is uploaded
// again.  Here the whole step is three launches on the caller's stream, with NO
// device-to-host copy: the boxes never leave the GPU.
//
//   k_crop_geometry (1 thread)   boxes x overlap_scales, int truncation, the gate,
//                                patch_resize in double (Python floats are doubles),
//                                rounding to size_divisor -> oetr_crop_info in HBM
//   k_crop_resize   (pass 1)     crop x255 -> bicubic -> tmp   [C][new_h][new_w]
//   k_crop_resize   (pass 2)     tmp -> bicubic -> /255 -> out [C][out_h][out_w]
//                                (the reference resizes a second time when the size is
//                                rounded up to a multiple of size_divisor; with equal
//                                sizes the cubic weights are exactly (0,1,0,0): a copy)
// When the gate fails the full images are passed through (evaluation.py:142-170): copied
// bit for bit, no resize passes.
//
// The sizes are data dependent, so the grids cover the caller's capacity and every
// thread reads the geometry first.  Bicubic = OpenCV's float path (a = -0.75, pixel
// centres (d + 0.5) * scale - 0.5, taps clamped to the border, horizontal then
// vertical); cv2 is not available in the build image: resize numerics are
// parity-unpinned (oracle/crop_oracle.py restates the same published algorithm).
//
// The arithmetic itself (geometry, cubic weights, source coordinate, tap sum) lives in crop_sample.h,
// shared with the batched entry (crop_batch.hip).
#include "../../include/oetr_hip.h"
#include "common.h"
#include "crop_sample.h"

namespace oetr {

struct CropLaunch {
  const float* image[2];   // [C][h][w]
  int h[2], w[2];
  int channels;
  const float* box[2];     // device [4] xyxy in the OETR input frame
  float scale[2][2];       // overlap_scales (sx, sy) per image
  int keep_aspect, size_divisor, gate_mode;
  int cap_h, cap_w;        // capacity of tmp / out per channel plane
  float* tmp[2];
  float* out[2];
  oetr_crop_info* info;
};

__global__ void k_crop_geometry(CropLaunch p) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  oetr_crop_info g;
  crop_geometry(p, g);   // crop_sample.h
  *p.info = g;
}

// One bicubic pass for both images (blockIdx.y = image, blockIdx.z = channel).
// PASS 1: src = the crop rectangle of the image, x255;  PASS 2: src = tmp, result /255.
template <int PASS>
__global__ __launch_bounds__(256) void k_crop_resize(CropLaunch p) {
  const int im = blockIdx.y, c = blockIdx.z;
  const oetr_crop_info& g = *p.info;
  if (g.valid != 1) {
    // gate failed: the reference hands data['image0'/'image1'] back untouched
    // (evaluation.py:142-170) - a plain copy, bit for bit, in the second pass only
    if (PASS == 2 && g.valid == 0) {
      const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
      const long npix = (long)p.w[im] * p.h[im];
      if (idx < npix) p.out[im][(size_t)c * npix + idx] = p.image[im][(size_t)c * npix + idx];
    }
    return;
  }
  int sw, sh, dw, dh, x0, y0, spitch;
  const float* src;
  float* dst;
  if (PASS == 1) {
    x0 = min(g.box[im][0], p.w[im]); y0 = min(g.box[im][1], p.h[im]);   // >= 0: crop_geometry's box domain
    sw = g.crop_w[im]; sh = g.crop_h[im];
    dw = g.new_w[im]; dh = g.new_h[im];
    spitch = p.w[im];
    src = p.image[im] + (size_t)c * p.h[im] * p.w[im];
    dst = p.tmp[im] + (size_t)c * dw * dh;
  } else {
    x0 = y0 = 0;
    sw = g.new_w[im]; sh = g.new_h[im];
    dw = g.out_w[im]; dh = g.out_h[im];
    spitch = sw;
    src = p.tmp[im] + (size_t)c * sw * sh;
    dst = p.out[im] + (size_t)c * dw * dh;
  }
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)dw * dh || sw <= 0 || sh <= 0) return;
  const int dy = (int)(idx / dw), dx = (int)(idx - (long)dy * dw);
  // fx = (float)((dx + 0.5) * scale_x - 0.5) with scale in double, as OpenCV computes it
  const float fx = crop_src_coord(dx, (double)sw / (double)dw);
  const float fy = crop_src_coord(dy, (double)sh / (double)dh);
  const int sx = (int)floorf(fx), sy = (int)floorf(fy);
  float wx[4], wy[4];
  cubic_weights(fx - (float)sx, wx);
  cubic_weights(fy - (float)sy, wy);
  const float in_scale = PASS == 1 ? 255.0f : 1.0f;
  const float acc = crop_tap_sum(src, spitch, x0, y0, sw, sh, sx, sy, wx, wy, in_scale);
  dst[idx] = PASS == 1 ? acc : acc / 255.0f;
}

hipError_t launch_overlap_crop(const CropLaunch& p, hipStream_t s) {
  hipLaunchKernelGGL(k_crop_geometry, dim3(1), dim3(64), 0, s, p);
  const long cap = (long)p.cap_h * p.cap_w;
  const dim3 grid((unsigned)((cap + 255) / 256), 2, p.channels);
  hipLaunchKernelGGL((k_crop_resize<1>), grid, dim3(256), 0, s, p);
  hipLaunchKernelGGL((k_crop_resize<2>), grid, dim3(256), 0, s, p);
  return hipGetLastError();
}

}  // namespace oetr

using namespace oetr;

extern "C" {

size_t oetr_overlap_crop_capacity(int channels, int h1, int w1, int h2, int w2, int size_divisor,
                                  int* cap_h, int* cap_w) {
  if (channels <= 0 || h1 <= 0 || w1 <= 0 || h2 <= 0 || w2 <= 0 || size_divisor < 1) return 0;
  const int d = size_divisor;
  const int ch = ((max(h1, h2) + d - 1) / d) * d, cw = ((max(w1, w2) + d - 1) / d) * d;
  if (cap_h) *cap_h = ch;
  if (cap_w) *cap_w = cw;
  return (size_t)channels * ch * cw;
}

oetr_status oetr_overlap_crop(const float* image1, const float* image2, int channels, int h1, int w1,
                              int h2, int w2, const float* box1, const float* box2,
                              const float scale1[2], const float scale2[2], int keep_aspect,
                              int size_divisor, int gate_mode, float* tmp, float* out1, float* out2,
                              size_t capacity_floats, oetr_crop_info* info, void* stream) {
  if (!image1 || !image2 || !box1 || !box2 || !scale1 || !scale2 || !tmp || !out1 || !out2 || !info)
    return (oetr_status)set_last_error(OETR_ERR_BAD_ARG, "oetr_overlap_crop: NULL argument");
  int cap_h = 0, cap_w = 0;
  const size_t need = oetr_overlap_crop_capacity(channels, h1, w1, h2, w2, size_divisor, &cap_h, &cap_w);
  if (need == 0 || (gate_mode != 0 && gate_mode != 1))
    return (oetr_status)set_last_error(OETR_ERR_BAD_ARG, "oetr_overlap_crop: bad shape / size_divisor / gate_mode");
  if (capacity_floats < need)
    return (oetr_status)set_last_error(OETR_ERR_WORKSPACE, "oetr_overlap_crop: buffers smaller than oetr_overlap_crop_capacity()");
  CropLaunch p;
  p.image[0] = image1; p.image[1] = image2;
  p.h[0] = h1; p.w[0] = w1; p.h[1] = h2; p.w[1] = w2;
  p.channels = channels;
  p.box[0] = box1; p.box[1] = box2;
  p.scale[0][0] = scale1[0]; p.scale[0][1] = scale1[1];
  p.scale[1][0] = scale2[0]; p.scale[1][1] = scale2[1];
  p.keep_aspect = keep_aspect; p.size_divisor = size_divisor; p.gate_mode = gate_mode;
  p.cap_h = cap_h; p.cap_w = cap_w;
  p.tmp[0] = tmp; p.tmp[1] = tmp + need;
  p.out[0] = out1; p.out[1] = out2;
  p.info = info;
  const hipError_t e = launch_overlap_crop(p, static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return (oetr_status)set_last_error(OETR_ERR_HIP, hipGetErrorString(e));
  return OETR_OK;
}

}  // extern "C"
