// The arithmetic of the box -> crop step, shared by its two entries: oetr_overlap_crop (crop.hip,
// one pair per call) and oetr_overlap_crop_batch (crop_batch.hip, n pairs per call).  ONE copy, so
// that pair k of a batched call is the per-pair call bit for bit: the geometry (boxes x
// overlap_scales, the box domain, int truncation, the gate, patch_resize in double, rounding to size_divisor),
// OpenCV's float bicubic weights, the source coordinate of an output pixel and the 4 x 4 tap sum.
// The expressions and the order of the products and sums are those crop.hip has always had (references
// to the reference's lines are in crop.hip's header comment).  What is NEW is that every rounding is
// pinned.  The tap sum used to be written with __fmul_rn / __fadd_rn, which are plain * and + to this
// compiler: under -ffp-contract=fast it fused SOME of the multiply-adds - which ones depended on the code
// around them (loop shape, SLP packing), so two kernels built from the same lines disagreed in the last
// bit.  The tap sum is now plain operators under `fp contract(off)` (every product and sum rounded on its
// own, as in the OpenCV C++ it restates and in the oracle), and the one fused step that is kept - the
// source coordinate - is written as the fma it always compiled to.
#pragma once
#include "../../include/oetr_hip.h"
#include "common.h"

namespace oetr {

// P: what the geometry needs of one pair, under these names (each entry passes its own struct):
//   int h[2], w[2]                              the matcher's images
//   const float* box[2]                         device [4] xyxy in the OETR input frame
//   float scale[2][2]                           overlap_scales (sx, sy) per image
//   int keep_aspect, size_divisor, gate_mode
//   int cap_h, cap_w                            capacity of tmp / out per channel plane
template <class P>
__device__ __forceinline__ void crop_geometry(const P& p, oetr_crop_info& g) {
  int bw[2], bh[2];
  bool inside = true;
  for (int i = 0; i < 2; ++i) {
    for (int j = 0; j < 4; ++j) {
      // bbox * overlap_scales in float32 (torch tensor product), then .int() truncation
      const float v = p.box[i][j] * p.scale[i][j & 1];
      g.sbox[i][j] = v;
      // THE BOX DOMAIN, tested in float ahead of the cast (include/oetr_hip.h): the truncation toward zero
      // must lie in [0, 2^31).  NaN fails both comparisons; -0.7 truncates to 0 and is inside.  Outside it
      // the cast would be undefined and a negative origin would address memory before the plane.
      const bool in_domain = v > -1.0f && v < 2147483648.0f;
      inside = inside && in_domain;
      g.box[i][j] = in_domain ? (int)v : 0;
    }
    bw[i] = g.box[i][2] - g.box[i][0];   // both in [0, 2^31): cannot overflow
    bh[i] = g.box[i][3] - g.box[i][1];
  }
  if (!inside) {
    // decided before the gate: valid = -1 whatever the gate would have said; every integer field and the
    // ratios zero, sbox the scaled floats as they are.  No resize kernel reads or writes for this pair.
    for (int i = 0; i < 2; ++i) {
      for (int j = 0; j < 4; ++j) g.box[i][j] = 0;
      g.crop_w[i] = g.crop_h[i] = g.new_w[i] = g.new_h[i] = g.out_w[i] = g.out_h[i] = 0;
      g.ratio[i][0] = g.ratio[i][1] = 0.0;
    }
    g.valid = -1;
    return;
  }
  int mn = min(min(bw[0], bh[0]), min(bw[1], bh[1]));
  bool valid = mn > 1;
  if (valid && p.gate_mode == 1) {   // 'pragueparks-val': integer floor_divide scores
    const int score = max(max(bw[0] / bw[1], bh[0] / bh[1]), max(bw[1] / bw[0], bh[1] / bh[0]));
    valid = score > 2;
  }
  // the larger-area image provides the target size (utils.py:525-534)
  const long a0 = (long)p.w[0] * p.h[0], a1 = (long)p.w[1] * p.h[1];
  const int ow = a0 >= a1 ? p.w[0] : p.w[1], oh = a0 >= a1 ? p.h[0] : p.h[1];
  for (int i = 0; i < 2; ++i) {
    if (!valid) {
      g.box[i][0] = 0; g.box[i][1] = 0; g.box[i][2] = p.w[i]; g.box[i][3] = p.h[i];
      g.sbox[i][0] = 0.f; g.sbox[i][1] = 0.f; g.sbox[i][2] = (float)p.w[i]; g.sbox[i][3] = (float)p.h[i];
      g.crop_w[i] = g.new_w[i] = g.out_w[i] = p.w[i];
      g.crop_h[i] = g.new_h[i] = g.out_h[i] = p.h[i];
      g.ratio[i][0] = g.ratio[i][1] = 1.0;
      continue;
    }
    // python slicing image[:, y1:y2, x1:x2] clamps at the border
    const int x1 = min(g.box[i][0], p.w[i]), x2 = min(g.box[i][2], p.w[i]);
    const int y1 = min(g.box[i][1], p.h[i]), y2 = min(g.box[i][3], p.h[i]);
    const int cw = max(0, x2 - x1), ch = max(0, y2 - y1);
    g.crop_w[i] = cw; g.crop_h[i] = ch;
    double rx, ry, nw, nh;
    if (p.keep_aspect) {   // patch_resize, extractor != 'disk'
      if ((double)ow / (double)cw > (double)oh / (double)ch) {
        rx = (double)oh / (double)ch; nw = rx * (double)cw; nh = (double)oh;
      } else {
        rx = (double)ow / (double)cw; nw = (double)ow; nh = rx * (double)ch;
      }
      ry = rx;
    } else {
      rx = (double)ow / (double)cw; ry = (double)oh / (double)ch; nw = (double)ow; nh = (double)oh;
    }
    g.ratio[i][0] = rx; g.ratio[i][1] = ry;
    g.new_w[i] = (int)nw; g.new_h[i] = (int)nh;
    g.out_w[i] = g.new_w[i]; g.out_h[i] = g.new_h[i];
    if (p.size_divisor > 1) {   // math.ceil(new / d) * d in double
      g.out_w[i] = (int)ceil((double)g.new_w[i] / p.size_divisor) * p.size_divisor;
      g.out_h[i] = (int)ceil((double)g.new_h[i] / p.size_divisor) * p.size_divisor;
    }
  }
  // A crop that does not fit the caller's capacity, or a degenerate one (the reference would
  // raise from cv2.resize there), cannot be produced: valid = -1, sizes zeroed - NOT the same
  // thing as a failed gate (valid = 0: the images pass through untouched).
  bool fits = true;
  for (int i = 0; i < 2; ++i)
    if (g.out_w[i] > p.cap_w || g.out_h[i] > p.cap_h || g.new_w[i] > p.cap_w || g.new_h[i] > p.cap_h ||
        g.new_w[i] <= 0 || g.new_h[i] <= 0)
      fits = false;
  if (!fits)
    for (int i = 0; i < 2; ++i) g.out_w[i] = g.out_h[i] = g.new_w[i] = g.new_h[i] = 0;
  g.valid = !fits ? -1 : (valid ? 1 : 0);
}

// OpenCV interpolateCubic (imgproc/resize.cpp), float32
__device__ __forceinline__ void cubic_weights(float t, float (&w)[4]) {
#pragma clang fp contract(off)   // separate multiplies and adds, like the C++ it restates
  const float a = -0.75f;
  w[0] = ((a * (t + 1.f) - 5.f * a) * (t + 1.f) + 8.f * a) * (t + 1.f) - 4.f * a;
  w[1] = ((a + 2.f) * t - (a + 3.f)) * t * t + 1.f;
  const float u = 1.f - t;
  w[2] = ((a + 2.f) * u - (a + 3.f)) * u * u + 1.f;
  w[3] = 1.f - w[0] - w[1] - w[2];
}

// Source coordinate of output pixel d: (float)((d + 0.5) * scale - 0.5) with scale = src / dst in
// double, as OpenCV computes it.  `scale` is that IEEE quotient wherever it was formed.  The multiply and
// the subtraction are ONE fused operation (what the expression has always compiled to), spelled out so
// that no kernel can get the other form.
__device__ __forceinline__ float crop_src_coord(int d, double scale) {
  return (float)__builtin_fma((double)d + 0.5, scale, -0.5);
}

// The 4 x 4 taps around (sx, sy), clamped to the sw x sh source rectangle whose corner is (x0, y0)
// of a plane with `spitch` floats per row; every source value is multiplied by in_scale first.
__device__ __forceinline__ float crop_tap_sum(const float* src, int spitch, int x0, int y0, int sw, int sh,
                                              int sx, int sy, const float (&wx)[4], const float (&wy)[4],
                                              const float in_scale) {
#pragma clang fp contract(off)   // every product and every sum rounded: the same bits in every kernel
  float acc = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int yy = min(max(sy - 1 + j, 0), sh - 1);
    const float* row = src + (size_t)(y0 + yy) * spitch + x0;
    float r = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int xx = min(max(sx - 1 + i, 0), sw - 1);
      r = r + (row[xx] * in_scale) * wx[i];   // hresize: S[..]*a0 + ... left to right
    }
    acc = acc + r * wy[j];                  // vresize: S0*b0 + S1*b1 + ...
  }
  return acc;
}

}  // namespace oetr
