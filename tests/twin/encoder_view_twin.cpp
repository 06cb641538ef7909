// encoder_view_twin.cpp -- TEST-ONLY host twin of the encoder's view from image bytes.
//
// Compiles curl_amd/csrc/curl_math_view.h (the header the gfx950 kernel and the library's host side include) for the host:
// the plan of a shape (view_build_plan: what curl_encoder_view_plan writes), and the two passes run FROM that plan as
// kernels/encoder_view.inc runs them -- the horizontal pass of every input row for the `size` cropped output columns,
// rounded to bytes, then the vertical pass on those bytes, to_tensor and the mask's `> 0`.  The product never loads this.
// With -DTWIN_MAIN it is a stand-alone program (for a sanitizer build): a few shapes on pseudo-random bytes, each printed as
// a sum; exit status 0 when every value lies in [0, 1].
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../curl_amd/csrc/curl_math_view.h"

using namespace curlm;

extern "C" {

// int32 of the plan of this shape (0: outside the limits); the plan itself, into view_plan_ints int32
size_t twin_view_plan_ints(int H, int W, int size) { return view_plan_ints(H, W, size); }
int twin_view_plan(int H, int W, int size, int* plan) {
  if (!view_plan_ints(H, W, size)) return -1;
  view_build_plan(H, W, size, plan);
  return 0;
}

// img [B,H,W,channels] (channels 3 | 4), mask [B,H,W] or NULL -> view_u8 [B,3,size,size] (the resampled bytes), view
// [B,3,size,size] = byte / 255, and for a mask mask_u8 [B,size,size], mask_view [B,1,size,size] = byte > 0
int twin_encoder_view(const uint8_t* img, int channels, const uint8_t* mask, uint8_t* view_u8, float* view, uint8_t* mask_u8,
                      float* mask_view, int B, int H, int W, int size) {
  const size_t n = view_plan_ints(H, W, size);
  if (!n || (channels != 3 && channels != 4)) return -1;
  std::vector<int> plan(n);
  view_build_plan(H, W, size, plan.data());
  const ViewHeader& h = *reinterpret_cast<const ViewHeader*>(plan.data());
  const int rix = view_row_ints(h.ksize_x), riy = view_row_ints(h.ksize_y);
  const int* const px = plan.data() + kViewHeaderInts;
  const int* const py = px + (size_t)size * rix;
  const size_t S2 = (size_t)size * size;
  std::vector<uint8_t> hb((size_t)H * size * 4);  // the horizontal pass: {r, g, b, mask} per (input row, output column)
  for (int b = 0; b < B; ++b) {
    const uint8_t* const ib = img + (size_t)b * H * W * channels;
    const uint8_t* const mb = mask ? mask + (size_t)b * H * W : nullptr;
    for (int y = 0; y < H; ++y)
      for (int c = 0; c < size; ++c) {
        const int* const kr = px + (size_t)c * rix;
        unsigned s[4] = {view_tap_start(), view_tap_start(), view_tap_start(), view_tap_start()};
        for (int x = 0; x < kr[1]; ++x) {
          const size_t p = (size_t)y * W + (size_t)(kr[0] + x);
          for (int ch = 0; ch < 3; ++ch) s[ch] = view_tap(s[ch], kr[2 + x], ib[p * channels + ch]);
          if (mb) s[3] = view_tap(s[3], kr[2 + x], mb[p]);
        }
        for (int ch = 0; ch < 4; ++ch) hb[((size_t)y * size + c) * 4 + ch] = (uint8_t)view_clip(s[ch]);
      }
    for (int r = 0; r < size; ++r)
      for (int c = 0; c < size; ++c) {
        const int* const kr = py + (size_t)r * riy;
        unsigned s[4] = {view_tap_start(), view_tap_start(), view_tap_start(), view_tap_start()};
        for (int y = 0; y < kr[1]; ++y)
          for (int ch = 0; ch < 4; ++ch) s[ch] = view_tap(s[ch], kr[2 + y], hb[((size_t)(kr[0] + y) * size + c) * 4 + ch]);
        const size_t o = (size_t)r * size + c;
        for (int ch = 0; ch < 3; ++ch) {
          const unsigned v = view_clip(s[ch]);
          view_u8[((size_t)b * 3 + ch) * S2 + o] = (uint8_t)v;
          view[((size_t)b * 3 + ch) * S2 + o] = view_unit(v);
        }
        if (mb) {
          const unsigned v = view_clip(s[3]);
          mask_u8[(size_t)b * S2 + o] = (uint8_t)v;
          mask_view[(size_t)b * S2 + o] = view_mask(v);
        }
      }
  }
  return 0;
}

}  // extern "C"

#ifdef TWIN_MAIN
int main() {
  const int shapes[][4] = {{40, 56, 32, 3}, {56, 40, 32, 4}, {32, 33, 32, 3}, {20, 27, 32, 3}, {641, 481, 32, 3}, {97, 1003, 16, 4}, {600, 8, 8, 3}, {512, 575, 8, 3}};
  uint32_t state = 12345u;
  auto byte = [&]() { return (uint8_t)((state = state * 1664525u + 1013904223u) >> 24); };
  int bad = 0;
  for (const auto& s : shapes) {
    const int B = 2, H = s[0], W = s[1], size = s[2], C = s[3];
    std::vector<uint8_t> img((size_t)B * H * W * C), mask((size_t)B * H * W), vu((size_t)B * 3 * size * size), mu((size_t)B * size * size);
    std::vector<float> v(vu.size()), m(mu.size());
    for (auto& x : img) x = byte();
    for (auto& x : mask) x = byte() < 26 ? byte() : 0;
    if (twin_encoder_view(img.data(), C, mask.data(), vu.data(), v.data(), mu.data(), m.data(), B, H, W, size)) return 2;
    double sum = 0.0;
    for (float x : v) bad += !(x >= 0.0f && x <= 1.0f), sum += x;
    for (float x : m) bad += !(x == 0.0f || x == 1.0f), sum += x;
    printf("%dx%dx%d -> %d: sum %.9g\n", H, W, C, size, sum);
  }
  return bad ? 1 : 0;
}
#endif
