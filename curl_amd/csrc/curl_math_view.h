// curl_math_view.h -- the encoder's input view as the reference makes it, on bytes: torchvision's Resize([size]) +
// CenterCrop((size, size)) of the decoded image (reference infer.py:32-41), which is Pillow's 8-bit antialiased bilinear
// resample -- fixed-point, rounded to bytes after each of its two passes -- followed by to_tensor and, for the mask, `> 0`.
//
// One header, three readers (as curl_math.h): the kernel (kernels/encoder_view.inc: tap sum, clip, header check), the library's
// host side (kernels/host_api_view.inc: geometry, the plan = the two coefficient tables) and the host twin
// (tests/twin/encoder_view_twin.cpp: all of it).  Restated from Pillow's and torchvision's behaviour:
//   geometry      the short side becomes `size`, the long one int(size * long / short); the crop margins are halved with
//                 Python's round(), so halves go to the EVEN integer
//   coefficients  float64, no contraction: a triangle of half-width max(in / out, 1) around (xx + 0.5) * in / out, normalised
//                 by its sum taken in index order, each weight rounded to 22 fractional bits
//   a pass        clip((2^21 + sum k[x] * byte[xmin + x]) >> 22, 0, 255): int32, products below 2^30, the sum below 2^31
// An axis with in == out needs no case of its own: its rows are {2^22, 0}, and (2^21 + 2^22 b) >> 22 = b.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "curl_math.h"

namespace curlm {

constexpr int kViewBits = 22;               // fractional bits of a coefficient: 32 - 8 - 2
constexpr int kViewMinSize = 8, kViewMaxSize = 1024;
constexpr int kViewMaxShrink = 64;          // min(H, W) / size beyond this is refused
constexpr int kViewMaxTaps = 160;           // ksize of the long axis at that limit: 2 ceil(64 * 8 / 7) + 1 = 149
constexpr int kViewHeaderInts = 16;         // the plan's header, in int32 (see ViewHeader)
constexpr int kViewStamp = 0x43565031;      // "CVP1"

// The plan a caller uploads: ViewHeader, then `size` rows {xmin, count, k[ksize_x]} for the cropped output columns
// left .. left + size - 1, then `size` rows {ymin, count, k[ksize_y]} for the cropped output rows; all int32.
struct ViewHeader {
  int stamp, H, W, size, ow, oh, top, left, ksize_x, ksize_y, zero[kViewHeaderInts - 10];
};
static_assert(sizeof(ViewHeader) == kViewHeaderInts * sizeof(int), "the header is sixteen int32");

struct ViewGeometry {
  int ow, oh, top, left;
};
// int(round(m / 2.0)) for a margin m >= 0 (torchvision's center_crop): Python rounds halves to even -- 1 -> 0, 3 -> 2
CURL_HD int view_half_margin(int m) {
  const int q = m >> 1;
  return (m & 1) ? q + (q & 1) : q;
}
// torchvision's Resize([size]): the short side becomes size, the long one int(size * long / short) (the quotient of two
// integers below 2^31 in float64 never rounds up to the next integer: it is the floor division)
CURL_HD ViewGeometry view_geometry(int H, int W, int size) {
  ViewGeometry g;
  if (W <= H) g.ow = size, g.oh = (int)(((int64_t)size * H) / W);
  else g.oh = size, g.ow = (int)(((int64_t)size * W) / H);
  g.top = view_half_margin(g.oh - size);
  g.left = view_half_margin(g.ow - size);
  return g;
}

struct ViewAxis {
  double scale, support, ss;  // in / out; max(scale, 1) (the bilinear filter's support is 1); 1 / support
  int ksize;
};
CURL_HD ViewAxis view_axis(int in, int out) {
#pragma clang fp contract(off)
  ViewAxis a;
  a.scale = (double)in / (double)out;
  a.support = a.scale < 1.0 ? 1.0 : a.scale;
  a.ss = 1.0 / a.support;
  a.ksize = (int)ceil(a.support) * 2 + 1;
  return a;
}
// Output sample xx of an axis of `in` samples: its first input sample, and k[0 .. ksize) (zero beyond the count, which is
// returned).  w: ksize doubles of scratch.
CURL_HD int view_coeffs(const ViewAxis& a, int in, int xx, int* xmin_out, int* k, double* w) {
#pragma clang fp contract(off)
  const double center = (xx + 0.5) * a.scale;
  int xmin = (int)(center - a.support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + a.support + 0.5);
  if (xmax > in) xmax = in;
  xmax -= xmin;
  double ww = 0.0;
  for (int x = 0; x < xmax; ++x) {
    double t = (x + xmin - center + 0.5) * a.ss;
    if (t < 0.0) t = -t;
    w[x] = t < 1.0 ? 1.0 - t : 0.0;
    ww += w[x];
  }
  for (int x = 0; x < a.ksize; ++x) {
    double p = x < xmax ? w[x] : 0.0;
    if (ww != 0.0) p = p / ww;
    k[x] = (int)(0.5 + p * (double)(1 << kViewBits));  // (a triangle's weights are never negative)
  }
  *xmin_out = xmin;
  return xmax;
}

CURL_HD int view_row_ints(int ksize) { return 2 + ksize; }
CURL_HD size_t view_plan_ints_of(int size, int ksize_x, int ksize_y) {
  return (size_t)kViewHeaderInts + (size_t)size * (size_t)(view_row_ints(ksize_x) + view_row_ints(ksize_y));
}
// what view_build_plan writes for this shape, in int32 (0: the shape is outside the limits above)
CURL_HD size_t view_plan_ints(int H, int W, int size) {
  if (H <= 0 || W <= 0 || size < kViewMinSize || size > kViewMaxSize) return 0;
  if ((int64_t)(H < W ? H : W) > (int64_t)kViewMaxShrink * size) return 0;
  const ViewGeometry g = view_geometry(H, W, size);
  const int kx = view_axis(W, g.ow).ksize, ky = view_axis(H, g.oh).ksize;
  if (kx > kViewMaxTaps || ky > kViewMaxTaps) return 0;
  return view_plan_ints_of(size, kx, ky);
}
// The plan of one shape into view_plan_ints(H, W, size) int32 of host memory (the caller has checked the shape).
inline void view_build_plan(int H, int W, int size, int* plan) {
  const ViewGeometry g = view_geometry(H, W, size);
  const ViewAxis ax = view_axis(W, g.ow), ay = view_axis(H, g.oh);
  ViewHeader h = {kViewStamp, H, W, size, g.ow, g.oh, g.top, g.left, ax.ksize, ay.ksize, {0}};
  *reinterpret_cast<ViewHeader*>(plan) = h;
  double w[kViewMaxTaps];
  int* row = plan + kViewHeaderInts;
  for (int i = 0; i < size; ++i, row += view_row_ints(ax.ksize)) row[1] = view_coeffs(ax, W, g.left + i, &row[0], row + 2, w);
  for (int i = 0; i < size; ++i, row += view_row_ints(ay.ksize)) row[1] = view_coeffs(ay, H, g.top + i, &row[0], row + 2, w);
}

// A pass, tap by tap.  The sum is carried unsigned (a foreign plan may hold anything: it wraps instead of overflowing);
// under a plan of view_build_plan both factors fit 24 bits and the sum stays below 2^31.
CURL_HD unsigned view_tap_start() { return 1u << (kViewBits - 1); }
CURL_HD unsigned view_tap(unsigned acc, int k, unsigned byte) { return acc + ((unsigned)k & 0xffffffu) * (byte & 0xffu); }
CURL_HD unsigned view_clip(unsigned acc) {
  const int v = (int)acc >> kViewBits;
  return (unsigned)(v < 0 ? 0 : v > 255 ? 255 : v);
}
// to_tensor of the view's byte; the mask view's `> 0`
CURL_HD float view_unit(unsigned byte) { return u8_to_unit((float)byte); }
CURL_HD float view_mask(unsigned byte) { return byte > 0u ? 1.0f : 0.0f; }

}  // namespace curlm
