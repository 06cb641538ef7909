// launch_plan_twin.cpp -- the host side of the C ABI (csrc/kernels/host_api.inc) run on a CPU with every kernel launch
// RECORDED instead of enqueued: which instantiation, grid, block, dynamic LDS and every kernel argument (as a digest; -v: in full).  The whole
// translation unit is compiled for the host only and linked without the HIP runtime; no device is ever opened.  The
// pointers are fixed fake addresses -- the host code never dereferences a device pointer.
//
// What it prints for a table of calls (every entry point, each side of every launch rule, every single-fault error) is
// compared with tests/data/launch_plan.txt by tests/test_launch_plan.py.  What it cannot see: a kernel's static LDS
// (hipFuncGetAttributes fails here, so static_lds<>() is 0 and lds_for_resident subtracts nothing).
//
//   launch_plan_twin [-v] <host_api.inc> <curl_hip.h>      (-v: kernel arguments in full instead of their digest)
// also checks its own coverage: every launch site of host_api.inc recorded, every declared entry point called.
#include <hip/hip_runtime.h>

#include <cxxabi.h>
#include <dlfcn.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <fstream>
#include <functional>
#include <regex>
#include <set>
#include <string>
#include <vector>
#include <type_traits>

static std::string g_out, g_call;     // the record; the launches of the call under way
static std::string* g_cur = &g_out;  // where outf writes
static bool g_verbose = false;        // -v: kernel arguments in full instead of their digest
static std::set<int> g_lines;
static std::set<std::string> g_called;
static int g_calls = 0, g_launches = 0;

__attribute__((format(printf, 1, 2))) static void outf(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  *g_cur += buf;
}

template <class... A>
static void record(int line, const void* kernel, dim3 grid, dim3 block, unsigned lds, const A&... args);

#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(k, g, b, l, s, ...) record(__LINE__, (const void*)(k), dim3(g), dim3(b), (unsigned)(l), __VA_ARGS__)
#define hipGetLastError() hipSuccess

#include "curl_kernels.hip"  // -I curl_amd/csrc (its own include of hip_runtime.h is guarded: the redefinitions hold)
#include "../../include/curl_hip_poly.h"

// what the host-only object still refers to: no-ops, so that no HIP runtime is linked
extern "C" {
void** __hipRegisterFatBinary(const void*) { return nullptr; }
void __hipRegisterFunction(void**, const void*, char*, const char*, unsigned, void*, void*, void*, void*, int*) {}
void __hipUnregisterFatBinary(void**) {}
hipError_t __hipPopCallConfiguration(dim3*, dim3*, size_t*, hipStream_t*) { return hipSuccess; }
hipError_t hipLaunchKernel(const void*, dim3, dim3, void**, size_t, hipStream_t) { return hipSuccess; }
hipError_t hipFuncGetAttributes(hipFuncAttributes*, const void*) { return hipErrorInvalidDeviceFunction; }
const char* hipGetErrorString(hipError_t) { return "hip error"; }
}

// ---------------------------------------------------------------------------------------------------------------
// printers: scalars as they are, the cases' fake pointers by name (IMG+4), every argument struct field by field (fields that
// are zero or NULL are left out)
// ---------------------------------------------------------------------------------------------------------------
static const char* const kPtrNames[] = {"0",    "IMG", "OUT", "GOUT", "GIMG", "RL", "RR",   "RH",    "REG", "WS",   "SCR",   "GL",    "GR",
                                        "GH",   "GREG", "COEF", "TGT", "LP", "LT",   "MASK",  "GCOEF", "AUX", "U8IN", "U8OUT", "WHITE", "SUMS"};
constexpr int kPtrShift = 36;  // the fake buffers lie 64 GiB apart: what a call derives from one (scratch + offset) keeps its name
static void put_ptr(const void* v) {
  const uint64_t a = (uint64_t)(uintptr_t)v, i = a >> kPtrShift, o = a & ((1ull << kPtrShift) - 1);
  if (i >= sizeof(kPtrNames) / sizeof(*kPtrNames)) outf("%p", v);
  else if (o) outf("%s+%llu", kPtrNames[i], (unsigned long long)o);
  else outf("%s", kPtrNames[i]);
}
template <class T>
struct no_printer : std::false_type {};
template <class T>
static void put(const T& v) {
  if constexpr (std::is_pointer_v<T> || std::is_null_pointer_v<T>) put_ptr((const void*)v);
  else if constexpr (std::is_same_v<T, float>) outf("%.9g", (double)v);
  else if constexpr (std::is_same_v<T, double>) outf("%.17g", v);
  else if constexpr (std::is_same_v<T, bool>) outf("%d", (int)v);
  else if constexpr (std::is_integral_v<T> && std::is_signed_v<T>) outf("%lld", (long long)v);
  else if constexpr (std::is_integral_v<T>) outf("%llu", (unsigned long long)v);
  else static_assert(no_printer<T>::value, "a kernel-argument struct without a printer: add one below");
}
#define FLD(f) (a.f ? (outf(" " #f "="), put(a.f)) : (void)0)
#define FLD3(f) outf(" " #f "=["), put(a.f[0]), outf(","), put(a.f[1]), outf(","), put(a.f[2]), outf("]")
static void put(const PrepArgs& a) { outf("Prep{"), FLD3(raw), FLD3(ncurves), FLD3(K), FLD(ws), FLD(reg_out), FLD(stride), outf(" }"); }
static void put(const StreamArgs& a) {
  outf("Stream{"), FLD(in), FLD(out), FLD(mask), FLD(coef), FLD(coef_stride), FLD(n), FLD(blocks_per_image), FLD(n_blocks), FLD(no_mem);
  FLD(W), FLD(H), FLD(op_flag), FLD(mask_first), FLD(white), FLD(units), FLD(segs), FLD(plane), FLD(off), FLD(row0), FLD(xcd_per), outf(" }");
}
static void put(const ChainArgs& a) {
  outf("Chain{"), FLD(in), FLD(out), FLD(knots), FLD(knot_stride), FLD(n_steps), FLD(K);
  for (int i = 0; i < CHAIN_MAX; ++i) outf(" step%d=(%d,%d,%d)", i, a.knot_off[i], a.cin[i], a.cout[i]);
  FLD(n), FLD(blocks_per_image), FLD(n_blocks), FLD(mode), outf(" }");
}
static void put_bwd(const BwdArgs& a) {
  FLD(in), FLD(gout), FLD(gin), FLD(mask), FLD(coef), FLD(partial), FLD(coef_stride), FLD(n), FLD(blocks_per_image), FLD(n_blocks);
  FLD(mask_first), FLD(stamp);
}
static void put(const BwdArgs& a) { outf("Bwd{"), put_bwd(a), outf(" }"); }
static void put(const PwlBwdArgs& a) { outf("PwlBwd{"), put_bwd(a), FLD(kl), FLD(kr), FLD(kh), outf(" }"); }
static void put(const KnotsBwdArgs& a) {
  outf("KnotsBwd{"), FLD(ws), FLD(partial), FLD(greg), FLD3(graw), FLD3(K), FLD(ws_stride), FLD(blocks_per_image), outf(" }");
}
static void put(const StageKnotsArgs& a) {
  outf("StageKnots{"), FLD(ws), FLD(partial), FLD(greg), FLD(graw), FLD(K), FLD(ws_stride), FLD(blocks_per_image), outf(" }");
}
static void put(const ConvBwdArgs& a) { outf("ConvBwd{"), FLD(in), FLD(gout), FLD(gin), FLD(n), outf(" }"); }
static void put(const LayerLossArgs& a) {
  outf("LayerLoss{"), FLD(img), FLD(tgt), FLD(mask), FLD(coef), FLD(out), FLD(partial), FLD(Lp), FLD(Lt), FLD(coef_stride), FLD(n);
  FLD(blocks_per_image), outf(" }");
}
static void put(const CoefGradArgs& a) {
  outf("CoefGrad{"), FLD(pxbuf), FLD(partial), FLD(HW), FLD(W), FLD(tiles), FLD(ppt), FLD(items), FLD(step_rows), FLD(step_cols), FLD(fW);
  FLD(fH), outf(" }");
}
static void put(const CoefGradStripArgs& a) {
  outf("CoefGradStrip{"), FLD(pxbuf), FLD(partial), FLD(HW), FLD(W), FLD(H), FLD(cw_log2), FLD(steps), FLD(n_cb), FLD(n_rt), FLD(items);
  FLD(fW), FLD(fH), outf(" }");
}
static void put(const PolyLayerGradArgs& a) {
  outf("PolyLayerGrad{"), FLD(img), FLD(gout), FLD(partial), FLD(HW), FLD(groups), FLD(tiles), FLD(steps), FLD(items), outf(" }");
}
static void put(const SsimArgs& a) {  // (without the window: ssim_window's floats are libm's, not a launch decision)
  outf("Ssim{"), FLD(a), FLD(b), FLD(a_next), FLD(b_next), FLD(partial), FLD(g_ssim), FLD(g_cs), FLD(d_mu), FLD(d_e11), FLD(d_e12);
  FLD(H), FLD(W), FLD(C), FLD(level), FLD(levels), FLD(radius), FLD(tiles_x), FLD(tiles), outf(" }");
}
static void put(const SsimGradArgs& a) {
  outf("SsimGrad{"), FLD(a), FLD(b), FLD(d_mu), FLD(d_e11), FLD(d_e12), FLD(g_below), FLD(g_out), FLD(H), FLD(W), FLD(radius);
  FLD(tiles_x), outf(" }");
}

template <class... A>
static void record(int line, const void* kernel, dim3 grid, dim3 block, unsigned lds, const A&... args) {
  g_lines.insert(line);
  ++g_launches;
  Dl_info info{};
  std::string name = "?";
  if (dladdr(kernel, &info) && info.dli_sname) {
    int status = 0;
    char* d = abi::__cxa_demangle(info.dli_sname, nullptr, nullptr, &status);
    name = (status == 0 && d) ? d : info.dli_sname;
    free(d);
  }
  // the kernel as `name<args>`: without the return type, the parameter list and the blanks
  name = name.substr(0, name.rfind('('));
  if (name.compare(0, 5, "void ") == 0) name.erase(0, 5);
  name.erase(std::remove(name.begin(), name.end(), ' '), name.end());
  // the arguments in full with -v, else as a 40-bit FNV-1a digest of that text
  std::string text;
  g_cur = &text;
  ((outf(" "), put(args)), ...);
  g_cur = &g_call;
  outf("%s@%d %s (%u,%u)x%u", g_call.empty() ? "" : " + ", line, name.c_str(), grid.x, grid.y, block.x);
  if (lds) outf(" lds=%u", lds);
  if (g_verbose) {
    outf(" |%s", text.c_str());
  } else {
    uint64_t h = 1469598103934665603ull;
    for (unsigned char ch : text) h = (h ^ ch) * 1099511628211ull;
    outf(" #%010llx", (unsigned long long)(h & 0xffffffffffull));
  }
  g_cur = &g_out;
}

// ---------------------------------------------------------------------------------------------------------------
// the calls
// ---------------------------------------------------------------------------------------------------------------
static float* P(unsigned i) { return (float*)(uintptr_t)((uint64_t)i << kPtrShift); }  // in kPtrNames' order
template <class T>
static T* off(T* p, int bytes) { return (T*)((char*)p + bytes); }
static float *const IMG = P(1), *const OUT = P(2), *const GOUT = P(3), *const GIMG = P(4), *const RL = P(5), *const RR = P(6),
             *const RH = P(7), *const REG = P(8), *const WS = P(9), *const SCR = P(10), *const GL = P(11), *const GR = P(12),
             *const GH = P(13), *const GREG = P(14), *const COEF = P(15), *const TGT = P(16), *const LP = P(17), *const LT = P(18),
             *const MASK = P(19), *const GCOEF = P(20), *const AUX = P(21);
static uint8_t *const U8IN = (uint8_t*)P(22), *const U8OUT = (uint8_t*)P(23), *const WHITE = (uint8_t*)P(24);
static double* const SUMS = (double*)P(25);
constexpr size_t BIG = (size_t)1 << 60;
#define UNROLL(u) ((unsigned)(u) << CURL_F_TUNE_UNROLL_SHIFT)
#define BLOCK(u) ((unsigned)(u) << CURL_F_TUNE_BLOCK_SHIFT)
#define XCD(u) ((unsigned)(u) << CURL_F_TUNE_XCD_SHIFT)
#define OCC(u) ((unsigned)(u) << CURL_F_TUNE_OCC_SHIFT)
#define PREP(u) ((unsigned)(u) << CURL_F_TUNE_PREP_SHIFT)

// A call that succeeds is one line: `fn: label => launch + launch ...`.  The calls that fail are gathered by outcome (return
// code, curl_last_error) and fault (the label without its `who: `), printed after the others with the entry points they hit.
struct Outcome {
  std::string what;
  std::vector<std::string> fns;
};
static std::vector<Outcome> g_failed;
static void call_done(const char* fn, const std::string& label, int rc) {
  ++g_calls;
  g_called.insert(fn);
  if (rc == 0) {
    outf("%s: %s%s", fn + 5, label.c_str(), g_call.empty() ? "" : " => ");
    g_out += g_call + "\n";
  } else {
    const size_t colon = label.find(": ");
    char what[400];
    snprintf(what, sizeof(what), "!%d \"%s\" [%s]", rc, curl_last_error(), label.c_str() + (colon == std::string::npos ? 0 : colon + 2));
    auto it = std::find_if(g_failed.begin(), g_failed.end(), [&](const Outcome& o) { return o.what == what; });
    if (it == g_failed.end()) it = g_failed.insert(g_failed.end(), Outcome{what, {}});
    it->fns.push_back(std::string(fn + 5) + (g_call.empty() ? "" : "(AFTER A LAUNCH)"));
  }
  g_call.clear();
}
static void print_failed() {
  for (const Outcome& o : g_failed) {
    g_out += o.what + ":";
    for (const std::string& fn : o.fns) g_out += " " + fn;
    g_out += "\n";
  }
}
#define CALL(label, fn, ...) call_done(#fn, label, fn(__VA_ARGS__))
static std::string g_size_fn;  // one line per size function: `name: (arguments)=bytes ...`
template <class... A>
static void size_call(const char* name, size_t (*fn)(A...), A... args) {
  ++g_calls;
  g_called.insert(name);
  if (g_size_fn != name) outf("%s%s:", g_size_fn.empty() ? "" : "\n", name + 5), g_size_fn = name;
  std::string text;
  g_cur = &text;
  ((outf(" "), put(args)), ...);
  g_cur = &g_out;
  outf(" (%s)=%zu", text.c_str() + 1, fn(args...));
}
#define SIZE(fn, ...) size_call(#fn, fn, __VA_ARGS__)
// ... or a copy of `base` with some changed: FROM(base, c.rows = 4)
#define FROM(base, ...) [&] { auto c = (base); __VA_ARGS__; return c; }()
// a call's arguments with some of them changed: WITH(Layer, c.B = 32, c.H = 256)
#define WITH(T, ...) [&] { T c; __VA_ARGS__; return c; }()

struct Shape {
  int B = 2, H = 32, W = 36;
};
static const Shape kCrops{32, 256, 256}, kFrames2{2, 1000, 1500}, kFrames3{3, 1000, 1500}, kFrames4{4, 1000, 1500}, kOdd{2, 255, 255},
    kFrame{1, 1000, 1500};

struct Layer {  // curl_layer_fwd_f32 and, with rows > 0, its slab form
  const float* img = IMG;
  const void* mask = MASK;
  int mk = 0;
  const float *rL = RL, *rR = RR, *rH = RH;
  float *out = OUT, *reg = REG;
  void* ws = WS;
  size_t wsb = BIG;
  int B = 2, H = 32, W = 36, row0 = 0, rows = 0, Kl = 16, Kr = 16, Kh = 16;
  unsigned flags = 0;
  Layer& shape(const Shape& s) { return B = s.B, H = s.H, W = s.W, *this; }
};
static void layer(const std::string& label, const Layer& c) {
  if (c.rows)
    CALL(label, curl_layer_fwd_slab_f32, c.img, c.mask, c.mk, c.rL, c.rR, c.rH, c.out, c.reg, c.ws, c.wsb, c.B, c.H, c.W, c.row0, c.rows,
         c.Kl, c.Kr, c.Kh, c.flags, nullptr);
  else
    CALL(label, curl_layer_fwd_f32, c.img, c.mask, c.mk, c.rL, c.rR, c.rH, c.out, c.reg, c.ws, c.wsb, c.B, c.H, c.W, c.Kl, c.Kr, c.Kh,
         c.flags, nullptr);
}
static void layer_u8(const std::string& label, const Layer& c, const uint8_t* in = U8IN, uint8_t* out = U8OUT, const uint8_t* white = WHITE) {
  CALL(label, curl_layer_fwd_u8hwc, in, c.mask, c.mk, c.rL, c.rR, c.rH, white, out, c.reg, c.ws, c.wsb, c.B, c.H, c.W, c.Kl, c.Kr, c.Kh,
       c.flags, nullptr);
}
struct LayerBwd : Layer {
  const float *gout = GOUT, *greg = GREG;
  float *gimg = GIMG, *gL = GL, *gR = GR, *gH = GH;
  void* scr = SCR;
  size_t scrb = BIG;
};
static void layer_bwd(const std::string& label, const LayerBwd& c, bool pwl = false) {
  if (pwl)
    CALL(label, curl_layer_pwl_bwd_f32, c.img, c.mask, c.mk, c.rL, c.rR, c.rH, c.gout, c.greg, c.gimg, c.gL, c.gR, c.gH, c.ws, c.wsb, c.scr,
         c.scrb, c.B, c.H, c.W, c.Kl, c.Kr, c.Kh, c.flags, nullptr);
  else
    CALL(label, curl_layer_bwd_f32, c.img, c.mask, c.mk, c.rL, c.rR, c.rH, c.gout, c.greg, c.gimg, c.gL, c.gR, c.gH, c.ws, c.wsb, c.scr,
         c.scrb, c.B, c.H, c.W, c.Kl, c.Kr, c.Kh, c.flags, nullptr);
}
struct LayerLoss : Layer {
  const float* tgt = TGT;
  double* sums = SUMS;
  float *Lp = LP, *Lt = LT;
  void* scr = SCR;
  size_t scrb = BIG;
};
static void layer_loss(const std::string& label, const LayerLoss& c) {
  CALL(label, curl_layer_loss_fwd_f32, c.img, c.mask, c.mk, c.rL, c.rR, c.rH, c.tgt, c.out, c.reg, c.sums, c.Lp, c.Lt, c.ws, c.wsb, c.scr,
       c.scrb, c.B, c.H, c.W, c.Kl, c.Kr, c.Kh, c.flags, nullptr);
}

// one knot segment: the adjust_* entries (no mask), the two stages, and the backward of all five
struct Seg {
  const float* img = IMG;
  const void* mask = MASK;
  int mk = 0;
  const float* raw = RL;
  float *out = OUT, *reg = REG;
  void* ws = WS;
  size_t wsb = BIG;
  int B = 2, H = 32, W = 36, K = 16;
  unsigned flags = 0;
  const float *gout = GOUT, *greg = GREG;
  float *gimg = GIMG, *graw = GL;
  void* scr = SCR;
  size_t scrb = BIG;
  Seg& shape(const Shape& s) { return B = s.B, H = s.H, W = s.W, *this; }
};
enum SegFn { RGB, LAB, HSV, LAB_STAGE, HSV_STAGE };
static const char* const kSegName[] = {"rgb", "lab", "hsv", "lab_stage", "hsv_stage"};
static void seg(SegFn f, const std::string& label, const Seg& c) {
  switch (f) {
    case RGB: CALL(label, curl_adjust_rgb_f32, c.img, c.raw, c.out, c.reg, c.ws, c.wsb, c.B, c.H, c.W, c.K, c.flags, nullptr); break;
    case LAB: CALL(label, curl_adjust_lab_f32, c.img, c.raw, c.out, c.reg, c.ws, c.wsb, c.B, c.H, c.W, c.K, c.flags, nullptr); break;
    case HSV: CALL(label, curl_adjust_hsv_f32, c.img, c.raw, c.out, c.reg, c.ws, c.wsb, c.B, c.H, c.W, c.K, c.flags, nullptr); break;
    case LAB_STAGE:
      CALL(label, curl_lab_stage_f32, c.img, c.mask, c.mk, c.raw, c.out, c.reg, c.ws, c.wsb, c.B, c.H, c.W, c.K, c.flags, nullptr);
      break;
    case HSV_STAGE:
      CALL(label, curl_hsv_stage_f32, c.img, c.mask, c.mk, c.raw, c.out, c.reg, c.ws, c.wsb, c.B, c.H, c.W, c.K, c.flags, nullptr);
      break;
  }
}
static void seg_bwd(SegFn f, const std::string& label, const Seg& c) {
#define SEG_BWD_ARGS c.gout, c.greg, c.gimg, c.graw, c.ws, c.wsb, c.scr, c.scrb, c.B, c.H, c.W, c.K, c.flags, nullptr
  switch (f) {
    case RGB: CALL(label, curl_adjust_rgb_bwd_f32, c.img, c.raw, SEG_BWD_ARGS); break;
    case LAB: CALL(label, curl_adjust_lab_bwd_f32, c.img, c.raw, SEG_BWD_ARGS); break;
    case HSV: CALL(label, curl_adjust_hsv_bwd_f32, c.img, c.raw, SEG_BWD_ARGS); break;
    case LAB_STAGE: CALL(label, curl_lab_stage_bwd_f32, c.img, c.mask, c.mk, c.raw, SEG_BWD_ARGS); break;
    case HSV_STAGE: CALL(label, curl_hsv_stage_bwd_f32, c.img, c.mask, c.mk, c.raw, SEG_BWD_ARGS); break;
  }
#undef SEG_BWD_ARGS
}

// the four converters, forward (in, out) and backward (in, grad_out, grad_in)
struct Conv {
  const float *in = IMG, *gout = GOUT;
  float* out = OUT;
  int B = 2, H = 32, W = 36;
  unsigned flags = 0;
  Conv& shape(const Shape& s) { return B = s.B, H = s.H, W = s.W, *this; }
};
static void conv(int which, const std::string& label, const Conv& c) {
  switch (which) {
    case 0: CALL(label, curl_rgb2lab_f32, c.in, c.out, c.B, c.H, c.W, c.flags, nullptr); break;
    case 1: CALL(label, curl_lab2rgb_f32, c.in, c.out, c.B, c.H, c.W, c.flags, nullptr); break;
    case 2: CALL(label, curl_rgb2hsv_f32, c.in, c.out, c.B, c.H, c.W, c.flags, nullptr); break;
    default: CALL(label, curl_hsv2rgb_f32, c.in, c.out, c.B, c.H, c.W, c.flags, nullptr); break;
  }
}
static void conv_bwd(int which, const std::string& label, const Conv& c) {
  switch (which) {
    case 0: CALL(label, curl_rgb2lab_bwd_f32, c.in, c.gout, c.out, c.B, c.H, c.W, c.flags, nullptr); break;
    case 1: CALL(label, curl_lab2rgb_bwd_f32, c.in, c.gout, c.out, c.B, c.H, c.W, c.flags, nullptr); break;
    case 2: CALL(label, curl_rgb2hsv_bwd_f32, c.in, c.gout, c.out, c.B, c.H, c.W, c.flags, nullptr); break;
    default: CALL(label, curl_hsv2rgb_bwd_f32, c.in, c.gout, c.out, c.B, c.H, c.W, c.flags, nullptr); break;
  }
}

constexpr int kPolyCounts[2][3] = {{4, 10, 20}, {6, 21, 56}};  // C(V + D, D) for V = 3 | 5, D = 1..3, said here on their own
struct Tri {  // the polynomial model: forward, slab (rows > 0), byte edge, backward
  const float *img = IMG, *coef = COEF, *gout = GOUT;
  float *out = OUT, *gcoef = GCOEF;
  void* scr = SCR;
  size_t scrb = BIG;
  int B = 2, H = 32, W = 36, row0 = 0, rows = 0, nc = 126;
  unsigned flags = 0;
  Tri& shape(const Shape& s) { return B = s.B, H = s.H, W = s.W, *this; }
};
static void tri(const std::string& label, const Tri& c) {
  if (c.rows) CALL(label, curl_trispace_fwd_slab_f32, c.img, c.coef, c.out, c.B, c.H, c.W, c.row0, c.rows, c.nc, c.flags, nullptr);
  else CALL(label, curl_trispace_fwd_f32, c.img, c.coef, c.out, c.B, c.H, c.W, c.nc, c.flags, nullptr);
}
static void tri_u8(const std::string& label, const Tri& c, const uint8_t* in = U8IN, uint8_t* out = U8OUT, const uint8_t* white = WHITE) {
  CALL(label, curl_trispace_fwd_u8hwc, in, c.coef, white, out, c.B, c.H, c.W, c.nc, c.flags, nullptr);
}
static void tri_bwd(const std::string& label, const Tri& c) {
  CALL(label, curl_trispace_bwd_f32, c.img, c.coef, c.gout, c.gcoef, c.scr, c.scrb, c.B, c.H, c.W, c.nc, c.flags, nullptr);
}
struct Poly {
  const float *img = IMG, *coef = COEF, *gout = GOUT;
  float *out = OUT, *gimg = GIMG, *gcoef = GCOEF;
  void* scr = SCR;
  size_t scrb = BIG;
  int B = 2, H = 32, W = 36, V = 5;
  unsigned flags = 0;
  Poly& shape(const Shape& s) { return B = s.B, H = s.H, W = s.W, *this; }
};
static void poly(const std::string& label, const Poly& c) { CALL(label, curl_poly_layer_f32, c.img, c.coef, c.out, c.B, c.H, c.W, c.V, nullptr); }
static void poly_bwd(const std::string& label, const Poly& c) {
  CALL(label, curl_poly_layer_bwd_f32, c.img, c.coef, c.gout, c.gimg, c.gcoef, c.scr, c.scrb, c.B, c.H, c.W, c.V, c.flags, nullptr);
}

// two images and a mask: PSNR, the loss terms and their backward, compose_white; MS-SSIM (C, window)
struct Pair {
  const float *a = IMG, *b = TGT;
  const void* mask = MASK;
  int mk = 0;
  float *res = OUT, *Lp = LP, *Lt = LT;
  double* sums = SUMS;
  const float *weights = AUX, *gLp = GL;
  void* scr = SCR;
  size_t scrb = BIG;
  int B = 2, C = 3, H = 32, W = 36, window = 11;
  Pair& shape(const Shape& s) { return B = s.B, H = s.H, W = s.W, *this; }
};
static void psnr(const std::string& label, const Pair& c) {
  CALL(label, curl_psnr_f32, c.a, c.b, c.mask, c.mk, c.res, c.scr, c.scrb, c.B, c.H, c.W, 1.0f, nullptr);
}
static void loss(const std::string& label, const Pair& c) {
  CALL(label, curl_loss_terms_f32, c.a, c.b, c.mask, c.mk, c.sums, c.Lp, c.Lt, c.scr, c.scrb, c.B, c.H, c.W, nullptr);
}
static void loss_bwd(const std::string& label, const Pair& c) {
  CALL(label, curl_loss_terms_bwd_f32, c.a, c.b, c.mask, c.mk, c.weights, c.gLp, c.res, c.B, c.H, c.W, nullptr);
}
static void compose(const std::string& label, const Pair& c, uint8_t* out = U8OUT) {
  CALL(label, curl_compose_white_u8hwc, c.a, c.mask, c.mk, out, c.B, c.H, c.W, nullptr);
}
static void msssim(const std::string& label, const Pair& c, bool bwd) {
  if (bwd) CALL(label, curl_msssim_bwd_f32, c.a, c.b, c.Lp, c.Lt, c.res, c.scr, c.scrb, c.B, c.C, c.H, c.W, c.window, nullptr);
  else CALL(label, curl_msssim_fwd_f32, c.a, c.b, c.Lp, c.Lt, c.scr, c.scrb, c.B, c.C, c.H, c.W, c.window, nullptr);
}

static std::string S(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
static std::string S(const char* fmt, ...) {
  char buf[256];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  return buf;
}

// the faults every image entry shares through check_img, on the call `go` makes from a mutable copy of `c`
template <class C, class Go>
static void img_faults(const char* who, C base, Go go) {
  go(S("%s: B = 0", who), FROM(base, c.B = 0));
  go(S("%s: H = 0", who), FROM(base, c.H = 0));
  go(S("%s: W = -1", who), FROM(base, c.W = -1));
  go(S("%s: H*W > 2^30", who), FROM(base, c.H = 32769, c.W = 32768));
  go(S("%s: B > 65535", who), FROM(base, c.B = 65536));
}
template <class C, class Go>
static void mask_faults(const char* who, C base, Go go) {
  go(S("%s: mask_kind 3", who), FROM(base, c.mk = 3));
  go(S("%s: mask_kind set, mask NULL", who), FROM(base, c.mk = 1, c.mask = nullptr));
}
template <class C, class Go>
static void ws_faults(const char* who, C base, Go go) {
  go(S("%s: workspace NULL", who), FROM(base, c.ws = nullptr));
  go(S("%s: workspace misaligned", who), FROM(base, c.ws = off(WS, 4)));
  go(S("%s: workspace too small", who), FROM(base, c.wsb = 64));
}
template <class C, class Go>
static void scratch_faults(const char* who, C base, Go go, bool alignment_checked) {
  go(S("%s: scratch NULL", who), FROM(base, c.scr = nullptr));
  go(S("%s: scratch off the 16-byte grid (%s)", who, alignment_checked ? "a fault" : "accepted"), FROM(base, c.scr = off(SCR, 4)));
  go(S("%s: scratch too small", who), FROM(base, c.scrb = 64));
}
static void tuning_faults(const char* who, unsigned allowed_extra, const std::function<void(const std::string&, unsigned)>& go) {
  go(S("%s: unknown flag bit", who), 0x80000000u);
  go(S("%s: PREP 3", who), PREP(3));
  for (unsigned bit : {CURL_F_EXACT_ORDER, CURL_F_PWL, CURL_F_RESIDUAL_ONLY, CURL_F_WS_READY, CURL_F_DIAG_SKIP_PREP})
    if (!(allowed_extra & bit)) go(S("%s: flag 0x%x not accepted here", who, bit), bit);
}

static void stream_cases() {
  // ---- launch_stream through the fused layer: self-prep, vector verdict, tuning fields, flags, slabs
  for (int mk = 0; mk < 3; ++mk) layer(S("float4, mask kind %d", mk), WITH(Layer, c.mk = mk));
  layer("self-prep at kSelfPrepMaxTiles: 32 crops = 2048 tiles", WITH(Layer, c.shape(kCrops), c.mk = 1));
  layer("self-prep above: two frames = 2930 tiles", WITH(Layer, c.shape(kFrames2), c.mk = 1));
  layer("scalar: H*W % 4 != 0, 32 crops of 255x255 (8160 scalar tiles: no self-prep)", WITH(Layer, c.shape(kOdd), c.B = 32));
  layer("scalar: H*W % 4 != 0, small", WITH(Layer, c.H = 33, c.W = 7, c.mk = 2));
  layer("scalar: img off the 16-byte grid", WITH(Layer, c.img = off(IMG, 4)));
  layer("scalar: out off the 16-byte grid", WITH(Layer, c.out = off(OUT, 8)));
  layer("scalar: float mask off its 16-byte grid", WITH(Layer, c.mk = 2, c.mask = off(MASK, 4)));
  layer("float4: uint8 mask on its 4-byte grid", WITH(Layer, c.mk = 1, c.mask = off(MASK, 4)));
  layer("scalar: uint8 mask off its 4-byte grid", WITH(Layer, c.mk = 1, c.mask = off(MASK, 2)));
  layer("float4: mask kind 0, the pointer's alignment is nobody's business", WITH(Layer, c.mk = 0, c.mask = off(MASK, 2)));
  for (unsigned u : {1u, 2u, 4u, 3u}) layer(S("UNROLL %u", u), WITH(Layer, c.shape(kFrame), c.flags = UNROLL(u)));
  for (unsigned b : {0u, 1u, 2u, 3u}) layer(S("BLOCK %u", b), WITH(Layer, c.shape(kFrame), c.flags = BLOCK(b) | PREP(1)));
  for (unsigned x : {0u, 1u, 2u, 3u}) {
    layer(S("XCD %u, blocks_per_image 9 (< 64)", x), WITH(Layer, c.H = 96, c.W = 96, c.flags = XCD(x)));
    layer(S("XCD %u, blocks_per_image 1465 (>= 64)", x), WITH(Layer, c.shape(kFrame), c.flags = XCD(x)));
  }
  for (unsigned k = 1; k <= 7; ++k) layer(S("OCC %u", k), WITH(Layer, c.shape(kFrame), c.flags = OCC(k)));
  for (unsigned p : {0u, 1u, 2u, 3u}) {
    layer(S("PREP %u, small launch", p), WITH(Layer, c.flags = PREP(p)));
    layer(S("PREP %u, large launch", p), WITH(Layer, c.shape(kFrames2), c.flags = PREP(p)));
  }
  layer("PREP 2 with a tile-shape request: the separate launch", WITH(Layer, c.flags = PREP(2) | UNROLL(1)));
  layer("NO_NT", WITH(Layer, c.flags = CURL_F_TUNE_NO_NT));
  layer("NO_NT on the scalar path", WITH(Layer, c.H = 33, c.W = 35, c.flags = CURL_F_TUNE_NO_NT));
  layer("DIAG_NO_MEM", WITH(Layer, c.flags = CURL_F_DIAG_NO_MEM));
  layer("DIAG_NO_MEM with MASK_FIRST, uint8 mask", WITH(Layer, c.mk = 1, c.flags = CURL_F_DIAG_NO_MEM | CURL_F_MASK_FIRST));
  for (int mk = 0; mk < 3; ++mk) {
    layer(S("MASK_FIRST, mask kind %d", mk), WITH(Layer, c.mk = mk, c.flags = CURL_F_MASK_FIRST));
    layer(S("PWL, mask kind %d", mk), WITH(Layer, c.mk = mk, c.flags = CURL_F_PWL));
    layer(S("EXACT_ORDER, mask kind %d", mk), WITH(Layer, c.mk = mk, c.flags = CURL_F_EXACT_ORDER));
  }
  layer("MASK_FIRST with UNROLL 2: the caller's tile shape stays", WITH(Layer, c.mk = 1, c.flags = CURL_F_MASK_FIRST | UNROLL(2)));
  layer("MASK_FIRST on the scalar path", WITH(Layer, c.mk = 1, c.H = 33, c.W = 35, c.flags = CURL_F_MASK_FIRST));
  layer("PWL with UNROLL 4 and OCC 3: one tile shape, no reservation on top of the table", WITH(Layer, c.flags = CURL_F_PWL | UNROLL(4) | OCC(3)));
  layer("PWL, scalar", WITH(Layer, c.H = 33, c.W = 35, c.flags = CURL_F_PWL));
  layer("PWL and EXACT_ORDER together", WITH(Layer, c.flags = CURL_F_PWL | CURL_F_EXACT_ORDER));
  layer("PWL with an uneven split", WITH(Layer, c.Kl = CURL_K_UNEVEN(16, 12), c.flags = CURL_F_PWL));
  layer("uneven splits, affine", WITH(Layer, c.Kl = CURL_K_UNEVEN(16, 12), c.Kh = CURL_K_UNEVEN(16, 2)));
  layer("DIAG_SKIP_PREP", WITH(Layer, c.flags = CURL_F_DIAG_SKIP_PREP));
  layer("DIAG_SKIP_PREP, large", WITH(Layer, c.shape(kFrames2), c.flags = CURL_F_DIAG_SKIP_PREP));
  layer("reg NULL", WITH(Layer, c.reg = nullptr));
  layer("slab, row0 * W a multiple of 4", WITH(Layer, c.row0 = 1, c.rows = 5));
  layer("slab, row0 * W not a multiple of 4 (W = 34, row0 = 1): scalar", WITH(Layer, c.W = 34, c.row0 = 1, c.rows = 4));
  layer("slab, rows * W not a multiple of 4 (W = 34, rows = 3): scalar", WITH(Layer, c.W = 34, c.row0 = 2, c.rows = 3));
  layer("slab of a large frame: self-prep counts the slab's tiles", WITH(Layer, c.shape(kFrames4), c.row0 = 100, c.rows = 200, c.mk = 1));
  layer("slab: the whole image", WITH(Layer, c.row0 = 0, c.rows = 32));
  // faults
  const auto go = [](const std::string& l, const Layer& c) { layer(l, c); };
  img_faults("layer", Layer(), go);
  mask_faults("layer", Layer(), go);
  ws_faults("layer", Layer(), go);
  layer("layer: img NULL", WITH(Layer, c.img = nullptr));
  layer("layer: out NULL", WITH(Layer, c.out = nullptr));
  layer("layer: rawL NULL", WITH(Layer, c.rL = nullptr));
  layer("layer: rawR NULL", WITH(Layer, c.rR = nullptr));
  layer("layer: rawH NULL", WITH(Layer, c.rH = nullptr));
  layer("layer: Kl = 1", WITH(Layer, c.Kl = 1));
  layer("layer: Kr = 257", WITH(Layer, c.Kr = 257));
  layer("layer: Kh negative", WITH(Layer, c.Kh = -16));
  layer("layer: Kh last curve of 1 knot", WITH(Layer, c.Kh = CURL_K_UNEVEN(16, 1)));
  layer("layer: Kl last curve longer than K", WITH(Layer, c.Kl = CURL_K_UNEVEN(16, 17)));
  layer("layer: EXACT_ORDER with an uneven split", WITH(Layer, c.Kr = CURL_K_UNEVEN(16, 12), c.flags = CURL_F_EXACT_ORDER));
  tuning_faults("layer", CURL_F_EXACT_ORDER | CURL_F_PWL | CURL_F_DIAG_SKIP_PREP, [](const std::string& l, unsigned f) { layer(l, WITH(Layer, c.flags = f)); });
  layer("layer: grid too large", WITH(Layer, c.B = 65535, c.H = 32768, c.W = 32768, c.flags = BLOCK(2) | PREP(1)));
  const auto slab = [](const std::string& l, const Layer& src) { layer(l, FROM(src, c.rows = 4)); };
  img_faults("layer slab", WITH(Layer, c.rows = 4), slab);
  layer("layer slab: row0 negative", WITH(Layer, c.row0 = -1, c.rows = 4));
  layer("layer slab: rows = 0 is the whole-image entry; rows = -1", WITH(Layer, c.rows = -1));
  layer("layer slab: row0 + rows > H", WITH(Layer, c.row0 = 30, c.rows = 3));
  layer("layer slab: mask NULL", WITH(Layer, c.rows = 4, c.mk = 2, c.mask = nullptr));
  layer("layer slab: workspace too small", WITH(Layer, c.rows = 4, c.wsb = 8));

  // ---- the byte edges: 4-byte-aligned images suffice for the vector path
  for (int mk = 0; mk < 3; ++mk) {
    layer_u8(S("float4, mask kind %d, white mask", mk), WITH(Layer, c.mk = mk));
    layer_u8(S("float4, mask kind %d, images on the 4-byte grid only", mk), WITH(Layer, c.mk = mk), off(U8IN, 4), off(U8OUT, 12), nullptr);
  }
  layer_u8("scalar: in off the 4-byte grid", Layer(), off(U8IN, 1));
  layer_u8("scalar: out off the 4-byte grid", Layer(), U8IN, off(U8OUT, 2));
  layer_u8("scalar: white mask off the 4-byte grid", Layer(), U8IN, U8OUT, off(WHITE, 3));
  layer_u8("scalar: float mask off its 16-byte grid", WITH(Layer, c.mk = 2, c.mask = off(MASK, 4)));
  layer_u8("scalar: H*W % 4 != 0", WITH(Layer, c.H = 33, c.W = 7));
  layer_u8("one frame", WITH(Layer, c.shape(kFrame), c.mk = 1));
  layer_u8("uneven split", WITH(Layer, c.Kr = CURL_K_UNEVEN(16, 5)));
  const auto go8 = [](const std::string& l, const Layer& c) { layer_u8(l, c); };
  img_faults("layer u8", Layer(), go8);
  mask_faults("layer u8", Layer(), go8);
  ws_faults("layer u8", Layer(), go8);
  layer_u8("layer u8: img NULL", Layer(), nullptr);
  layer_u8("layer u8: out NULL", Layer(), U8IN, nullptr);
  layer_u8("layer u8: rawR NULL", WITH(Layer, c.rR = nullptr));
  layer_u8("layer u8: Kl = 0", WITH(Layer, c.Kl = 0));
  layer_u8("layer u8: any flag", WITH(Layer, c.flags = CURL_F_MASK_FIRST));

  // ---- launch_stream through the other ops: Op::kResident, mask-first on a two-group op, the Lab stage's table forms
  for (SegFn f : {RGB, LAB, HSV, LAB_STAGE, HSV_STAGE}) {
    const char* n = kSegName[f];
    const bool stage = f >= LAB_STAGE;
    seg(f, S("%s: small (self-prep)", n), Seg());
    seg(f, S("%s: scalar", n), WITH(Seg, c.H = 33, c.W = 7));
    seg(f, S("%s: below kResidentMinTiles: three frames = 4395 tiles", n), WITH(Seg, c.shape(kFrames3)));
    seg(f, S("%s: at kResidentMinTiles: four frames = 5860 tiles", n), WITH(Seg, c.shape(kFrames4)));
    if (f == HSV_STAGE) {  // (what of the residency rule does not depend on the op)
      seg(f, S("%s: four frames, OCC 1 says no cap", n), WITH(Seg, c.shape(kFrames4), c.flags = OCC(1)));
      seg(f, S("%s: four frames, UNROLL 2 keeps the caller's shape", n), WITH(Seg, c.shape(kFrames4), c.flags = UNROLL(2)));
      seg(f, S("%s: four frames, scalar", n), WITH(Seg, c.shape(kFrames4), c.img = off(IMG, 4)));
      seg(f, S("%s: PREP 2 on four frames", n), WITH(Seg, c.shape(kFrames4), c.flags = PREP(2)));
    }
    seg(f, S("%s: uneven split", n), WITH(Seg, c.K = CURL_K_UNEVEN(16, 9)));
    if (stage)
      for (int mk = 1; mk < 3; ++mk) {
        seg(f, S("%s: mask kind %d", n, mk), WITH(Seg, c.mk = mk));
        seg(f, S("%s: MASK_FIRST, mask kind %d", n, mk), WITH(Seg, c.mk = mk, c.flags = CURL_F_MASK_FIRST | PREP(1)));
        seg(f, S("%s: MASK_FIRST, mask kind %d, four frames", n, mk), WITH(Seg, c.shape(kFrames4), c.mk = mk, c.flags = CURL_F_MASK_FIRST));
      }
    if (f != HSV_STAGE && f != LAB)  // (adjust_lab is adjust_rgb's code: adjust_common with three curves)
      for (unsigned fl : {CURL_F_EXACT_ORDER, CURL_F_PWL}) {
        seg(f, S("%s: flag 0x%x", n, fl), WITH(Seg, c.flags = fl, c.mk = stage ? 1 : 0));
        seg(f, S("%s: flag 0x%x, scalar", n, fl), WITH(Seg, c.H = 33, c.W = 35, c.flags = fl));
        seg(f, S("%s: flag 0x%x below the residency threshold", n, fl), WITH(Seg, c.shape(kFrames3), c.flags = fl));
        seg(f, S("%s: flag 0x%x at the residency threshold", n, fl), WITH(Seg, c.shape(kFrames4), c.flags = fl));
        seg(f, S("%s: flag 0x%x with UNROLL 4, BLOCK 1, OCC 2", n, fl), WITH(Seg, c.flags = fl | UNROLL(4) | BLOCK(1) | OCC(2)));
        seg(f, S("%s: flag 0x%x with an uneven split", n, fl), WITH(Seg, c.flags = fl, c.K = CURL_K_UNEVEN(16, 9)));
        seg(f, S("%s: flag 0x%x with UNROLL 3", n, fl), WITH(Seg, c.flags = fl | UNROLL(3)));
      }
    const auto gos = [f](const std::string& l, const Seg& c) { seg(f, l, c); };
    img_faults(n, Seg(), gos);
    ws_faults(n, Seg(), gos);
    if (stage) mask_faults(n, Seg(), gos);
    seg(f, S("%s: img NULL", n), WITH(Seg, c.img = nullptr));
    seg(f, S("%s: out NULL", n), WITH(Seg, c.out = nullptr));
    seg(f, S("%s: raw NULL", n), WITH(Seg, c.raw = nullptr));
    seg(f, S("%s: K = 1", n), WITH(Seg, c.K = 1));
    seg(f, S("%s: K = 300", n), WITH(Seg, c.K = 300));
    seg(f, S("%s: UNROLL 3", n), WITH(Seg, c.flags = UNROLL(3)));
    seg(f, S("%s: BLOCK 3", n), WITH(Seg, c.flags = BLOCK(3)));
    seg(f, S("%s: XCD 3", n), WITH(Seg, c.flags = XCD(3)));
    tuning_faults(n, f == HSV_STAGE ? 0 : (CURL_F_EXACT_ORDER | CURL_F_PWL), [f](const std::string& l, unsigned fl) { seg(f, l, WITH(Seg, c.flags = fl)); });
  }
  seg(HSV_STAGE, "hsv_stage: MASK_FIRST with UNROLL 4: the caller's shape stays", WITH(Seg, c.mk = 1, c.flags = CURL_F_MASK_FIRST | UNROLL(4) | PREP(1)));
  seg(HSV_STAGE, "hsv_stage: MASK_FIRST, uint8 mask: the flag rules the in-kernel collapse out", WITH(Seg, c.mk = 1, c.flags = CURL_F_MASK_FIRST));

  // ---- apply_curve: launch_chain modes 0, 1, 2 and its residency rule
  const auto curve = [](const std::string& l, const Seg& c, int cin = 0, int cout = 1) {
    CALL(l, curl_apply_curve_f32, c.img, c.raw, c.out, c.reg, c.B, c.H, c.W, c.K, cin, cout, c.flags, nullptr);
  };
  for (unsigned fl : {0u, CURL_F_EXACT_ORDER, CURL_F_PWL}) {
    curve(S("flags 0x%x", fl), WITH(Seg, c.flags = fl));
    curve(S("flags 0x%x, scalar", fl), WITH(Seg, c.H = 33, c.W = 35, c.flags = fl));
    curve(S("flags 0x%x, three frames", fl), WITH(Seg, c.shape(kFrames3), c.flags = fl));
    curve(S("flags 0x%x, four frames", fl), WITH(Seg, c.shape(kFrames4), c.flags = fl));
    if (fl == 0)
      for (unsigned u : {1u, 2u, 4u}) {
        curve(S("UNROLL %u, BLOCK 2 is ignored", u), WITH(Seg, c.flags = UNROLL(u) | BLOCK(2)));
        curve(S("UNROLL %u, scalar", u), WITH(Seg, c.H = 33, c.W = 35, c.flags = UNROLL(u)));
      }
  }
  curve("four frames, OCC 3", WITH(Seg, c.shape(kFrames4), c.flags = OCC(3)));
  curve("four frames, UNROLL 1", WITH(Seg, c.shape(kFrames4), c.flags = UNROLL(1)));
  curve("reg NULL", WITH(Seg, c.reg = nullptr));
  curve("65 images: two blocks of curve_reg_kernel", WITH(Seg, c.B = 65, c.H = 8, c.W = 8));
  img_faults("apply_curve", Seg(), [&](const std::string& l, const Seg& c) { curve(l, c); });
  curve("apply_curve: img NULL", WITH(Seg, c.img = nullptr));
  curve("apply_curve: C NULL", WITH(Seg, c.raw = nullptr));
  curve("apply_curve: K = 1", WITH(Seg, c.K = 1));
  curve("apply_curve: uneven K", WITH(Seg, c.K = CURL_K_UNEVEN(16, 9)));
  curve("apply_curve: channel_in 3", Seg(), 3, 0);
  curve("apply_curve: channel_out -1", Seg(), 0, -1);
  curve("apply_curve: UNROLL 5", WITH(Seg, c.flags = UNROLL(5)));
  curve("apply_curve: XCD 3", WITH(Seg, c.flags = XCD(3)));
  curve("apply_curve: BLOCK 3 is masked off", WITH(Seg, c.flags = BLOCK(3)));
  tuning_faults("apply_curve", CURL_F_EXACT_ORDER | CURL_F_PWL, [&](const std::string& l, unsigned fl) { curve(l, WITH(Seg, c.flags = fl)); });

  // ---- the converters
  for (int w = 0; w < 4; ++w) {
    conv(w, "float4", Conv());
    conv(w, "scalar", WITH(Conv, c.H = 33, c.W = 7));
    conv(w, "four frames: resident", WITH(Conv, c.shape(kFrames4)));
    if (w == 0) {
      conv(w, "three frames", WITH(Conv, c.shape(kFrames3)));
      conv(w, "four frames, BLOCK 1", WITH(Conv, c.shape(kFrames4), c.flags = BLOCK(1)));
      conv(w, "XCD 2, one frame", WITH(Conv, c.shape(kFrame), c.flags = XCD(2)));
    }
    const auto goc = [w](const std::string& l, const Conv& c) { conv(w, l, c); };
    img_faults("converter", Conv(), goc);
    conv(w, "converter: in NULL", WITH(Conv, c.in = nullptr));
    conv(w, "converter: out NULL", WITH(Conv, c.out = nullptr));
    conv(w, "converter: UNROLL 7", WITH(Conv, c.flags = UNROLL(7)));
    tuning_faults("converter", 0, [w](const std::string& l, unsigned fl) { conv(w, l, WITH(Conv, c.flags = fl)); });
    conv_bwd(w, "float4", Conv());
    conv_bwd(w, "scalar: H*W % 4 != 0", WITH(Conv, c.H = 33, c.W = 7));
    if (w == 0) conv_bwd(w, "scalar: grad_in off the grid", WITH(Conv, c.out = off(OUT, 4)));
    if (w == 0) conv_bwd(w, "one frame", WITH(Conv, c.shape(kFrame)));
    const auto gob = [w](const std::string& l, const Conv& c) { conv_bwd(w, l, c); };
    img_faults("converter bwd", Conv(), gob);
    conv_bwd(w, "converter bwd: in NULL", WITH(Conv, c.in = nullptr));
    conv_bwd(w, "converter bwd: grad_out NULL", WITH(Conv, c.gout = nullptr));
    conv_bwd(w, "converter bwd: grad_in NULL", WITH(Conv, c.out = nullptr));
    tuning_faults("converter bwd", 0, [w](const std::string& l, unsigned fl) { conv_bwd(w, l, WITH(Conv, c.flags = fl)); });
  }

  // ---- the polynomial model: row-tiled (126) and plain (35)
  for (int nc : {126, 35}) {
    tri(S("nc %d: float4", nc), WITH(Tri, c.nc = nc));
    tri(S("nc %d: W = 1500: two blocks of 192", nc), WITH(Tri, c.nc = nc, c.shape(kFrame)));
    tri(S("nc %d: W = 1028: 257 units", nc), WITH(Tri, c.nc = nc, c.H = 5, c.W = 1028));
    tri(S("nc %d: W %% 4 != 0 but H*W %% 4 == 0", nc), WITH(Tri, c.nc = nc, c.H = 4, c.W = 31));
    tri(S("nc %d: H*W %% 4 != 0", nc), WITH(Tri, c.nc = nc, c.H = 33, c.W = 7));
    tri(S("nc %d: W = 256", nc), WITH(Tri, c.nc = nc, c.H = 8, c.W = 256));
    tri(S("nc %d: residual only, UNROLL 4 and OCC 2 ignored", nc), WITH(Tri, c.nc = nc, c.flags = CURL_F_RESIDUAL_ONLY | UNROLL(4) | OCC(2)));
    tri(S("nc %d: BLOCK 1, XCD 2, one frame", nc), WITH(Tri, c.nc = nc, c.shape(kFrame), c.flags = BLOCK(1) | XCD(2)));
    tri(S("nc %d: slab row0 = 1", nc), WITH(Tri, c.nc = nc, c.row0 = 1, c.rows = 7));
    tri(S("nc %d: slab, row0 * W not a multiple of 4", nc), WITH(Tri, c.nc = nc, c.W = 34, c.row0 = 1, c.rows = 4));
    tri(S("nc %d: coeffs on the 8-byte grid", nc), WITH(Tri, c.nc = nc, c.coef = off(COEF, 8)));
    tri(S("nc %d: coeffs on the 4-byte grid", nc), WITH(Tri, c.nc = nc, c.coef = off(COEF, 4)));
    tri(S("nc %d: coeffs off the 4-byte grid", nc), WITH(Tri, c.nc = nc, c.coef = off(COEF, 2)));
    tri_u8(S("nc %d: float4, white mask", nc), WITH(Tri, c.nc = nc));
    tri_u8(S("nc %d: images on the 4-byte grid only, no white mask", nc), WITH(Tri, c.nc = nc), off(U8IN, 4), off(U8OUT, 8), nullptr);
    tri_u8(S("nc %d: scalar, in off the 4-byte grid", nc), WITH(Tri, c.nc = nc), off(U8IN, 2));
    tri_u8(S("nc %d: W = 1500", nc), WITH(Tri, c.nc = nc, c.shape(kFrame)));
    tri_u8(S("nc %d: W %% 4 != 0 but H*W %% 4 == 0", nc), WITH(Tri, c.nc = nc, c.H = 4, c.W = 31));
    tri_u8(S("nc %d: coeffs on the 4-byte grid", nc), WITH(Tri, c.nc = nc, c.coef = off(COEF, 4)));
  }
  const auto got = [](const std::string& l, const Tri& c) { tri(l, c); };
  img_faults("trispace", Tri(), got);
  img_faults("trispace slab", WITH(Tri, c.rows = 4), [](const std::string& l, const Tri& src) { tri(l, FROM(src, c.rows = 4)); });
  tri("trispace: img NULL", WITH(Tri, c.img = nullptr));
  tri("trispace: out NULL", WITH(Tri, c.out = nullptr));
  tri("trispace: coeffs NULL", WITH(Tri, c.coef = nullptr));
  tri("trispace: num_coeffs 56", WITH(Tri, c.nc = 56));
  tri("trispace: BLOCK 3", WITH(Tri, c.flags = BLOCK(3)));
  tri("trispace: XCD 3", WITH(Tri, c.flags = XCD(3)));
  tri("trispace rows: grid too large", WITH(Tri, c.B = 65535, c.H = 32768, c.W = 32768));
  tri("trispace rows: the row grid too large (the plain one fits)", WITH(Tri, c.B = 16, c.H = 1 << 28, c.W = 4));
  tri("trispace 35: grid too large", WITH(Tri, c.nc = 35, c.B = 65535, c.H = 32768, c.W = 32768, c.flags = BLOCK(2)));
  tuning_faults("trispace", CURL_F_RESIDUAL_ONLY, [](const std::string& l, unsigned fl) { tri(l, WITH(Tri, c.flags = fl)); });
  tri("trispace slab: row0 negative", WITH(Tri, c.row0 = -1, c.rows = 4));
  tri("trispace slab: rows negative", WITH(Tri, c.rows = -2));
  tri("trispace slab: row0 + rows > H", WITH(Tri, c.row0 = 31, c.rows = 2));
  tri("trispace slab: coeffs NULL", WITH(Tri, c.rows = 4, c.coef = nullptr));
  tri("trispace slab: num_coeffs 0", WITH(Tri, c.rows = 4, c.nc = 0));
  img_faults("trispace u8", Tri(), [](const std::string& l, const Tri& c) { tri_u8(l, c); });
  tri_u8("trispace u8: img NULL", Tri(), nullptr);
  tri_u8("trispace u8: out NULL", Tri(), U8IN, nullptr);
  tri_u8("trispace u8: coeffs NULL", WITH(Tri, c.coef = nullptr));
  tri_u8("trispace u8: num_coeffs 34", WITH(Tri, c.nc = 34));
  tri_u8("trispace u8: any flag", WITH(Tri, c.flags = CURL_F_RESIDUAL_ONLY));
  tri_u8("trispace u8: coeffs off the 8-byte grid", WITH(Tri, c.coef = off(COEF, 4)));

  // ---- orders 1-3 (curl_hip_poly.h): the order in the high half of num_coeffs, a kernel per (variables, order)
  for (int V : {5, 3})
    for (int D : {1, 2, 3}) tri(S("V %d order %d: float4", V, D), WITH(Tri, c.nc = CURL_POLY_COEFFS(kPolyCounts[V == 5][D - 1], D)));
  tri("V 5 order 2: scalar, H*W % 4 != 0", WITH(Tri, c.nc = CURL_POLY_COEFFS(21, 2), c.H = 33, c.W = 7));
  tri("V 5 order 3: slab row0 = 1", WITH(Tri, c.nc = CURL_POLY_COEFFS(56, 3), c.row0 = 1, c.rows = 7));
  tri("V 5 order 4 said in the high half: the row-tiled kernel", WITH(Tri, c.nc = CURL_POLY_COEFFS(126, 4)));
  tri_u8("V 5 order 1: float4, white mask", WITH(Tri, c.nc = CURL_POLY_COEFFS(6, 1)));
  tri_u8("V 3 order 2: float4, no white mask", WITH(Tri, c.nc = CURL_POLY_COEFFS(10, 2)), U8IN, U8OUT, nullptr);
  tri("trispace: order 5", WITH(Tri, c.nc = CURL_POLY_COEFFS(126, 5)));
  tri("trispace: order 0", WITH(Tri, c.nc = CURL_POLY_COEFFS(126, 0)));
  tri("trispace: a count of another order, CURL_POLY_COEFFS(56, 2)", WITH(Tri, c.nc = CURL_POLY_COEFFS(56, 2)));
  tri_u8("trispace u8: a plain 56, no order in the high half", WITH(Tri, c.nc = 56));
}

static void pointwise_cases() {
  // ---- the stand-alone polynomial layer
  for (int V : {5, 3}) {
    poly(S("V %d: float4", V), WITH(Poly, c.V = V));
    poly(S("V %d: scalar, H*W %% 4 != 0", V), WITH(Poly, c.V = V, c.H = 33, c.W = 7));
    poly(S("V %d: scalar, out off the grid", V), WITH(Poly, c.V = V, c.out = off(OUT, 4)));
    poly(S("V %d: one frame", V), WITH(Poly, c.V = V, c.shape(kFrame)));
  }
  img_faults("poly_layer", Poly(), [](const std::string& l, const Poly& c) { poly(l, c); });
  poly("poly_layer: img NULL", WITH(Poly, c.img = nullptr));
  poly("poly_layer: out NULL", WITH(Poly, c.out = nullptr));
  poly("poly_layer: coeffs NULL", WITH(Poly, c.coef = nullptr));
  poly("poly_layer: num_variables 4", WITH(Poly, c.V = 4));
  // degrees 1-3 (curl_hip_poly.h): the degree in the high half of num_variables
  for (int V : {5, 3})
    for (int D : {1, 2, 3}) poly(S("V %d degree %d: float4", V, D), WITH(Poly, c.V = CURL_POLY_VARS(V, D)));
  poly("V 3 degree 2: scalar, H*W % 4 != 0", WITH(Poly, c.V = CURL_POLY_VARS(3, 2), c.H = 33, c.W = 7));
  poly("V 5 degree 4 said in the high half", WITH(Poly, c.V = CURL_POLY_VARS(5, 4)));
  poly("poly_layer: degree 5", WITH(Poly, c.V = CURL_POLY_VARS(5, 5)));
  poly("poly_layer: degree 0", WITH(Poly, c.V = CURL_POLY_VARS(5, 0)));
  poly("poly_layer: 4 variables with a degree", WITH(Poly, c.V = CURL_POLY_VARS(4, 2)));

  // ---- the layout edges
  const auto ingress = [](const std::string& l, const Shape& s, int Cin, const uint8_t* in = U8IN, float* out = OUT) {
    CALL(l, curl_u8hwc_to_f32chw, in, out, s.B, s.H, s.W, Cin, nullptr);
  };
  const auto egress = [](const std::string& l, const Shape& s, const float* in = IMG, uint8_t* out = U8OUT) {
    CALL(l, curl_f32chw_to_u8hwc, in, out, s.B, s.H, s.W, nullptr);
  };
  for (int Cin : {3, 4}) {
    ingress(S("Cin %d: float4", Cin), Shape(), Cin);
    ingress(S("Cin %d: in on the 4-byte grid only", Cin), Shape(), Cin, off(U8IN, 4));
    ingress(S("Cin %d: in off the 4-byte grid", Cin), Shape(), Cin, off(U8IN, 2));
    ingress(S("Cin %d: out off the 16-byte grid", Cin), Shape(), Cin, U8IN, off(OUT, 4));
    ingress(S("Cin %d: H*W %% 4 != 0", Cin), Shape{2, 33, 7}, Cin);
    ingress(S("Cin %d: three frames, below 5632 tiles", Cin), kFrames3, Cin);
    ingress(S("Cin %d: four frames, at 5632 tiles: resident", Cin), kFrames4, Cin);
    ingress(S("Cin %d: 5632 tiles exactly (22 x 256 tiles of 1024 px)", Cin), Shape{22, 512, 512}, Cin);
    ingress(S("Cin %d: 5631 tiles", Cin), Shape{1, 5631, 1024}, Cin);
  }
  ingress("four frames, scalar: no reservation", kFrames4, 3, off(U8IN, 1));
  img_faults("ingress", Shape(), [&](const std::string& l, const Shape& s) { ingress(l, s, 3); });
  ingress("ingress: in NULL", Shape(), 3, nullptr);
  ingress("ingress: out NULL", Shape(), 3, U8IN, nullptr);
  ingress("ingress: Cin 2", Shape(), 2);
  egress("float4", Shape());
  egress("out on the 4-byte grid", Shape(), IMG, off(U8OUT, 4));
  egress("out off the 4-byte grid", Shape(), IMG, off(U8OUT, 1));
  egress("in off the 16-byte grid", Shape(), off(IMG, 8));
  egress("H*W % 4 != 0", Shape{2, 33, 7});
  egress("three frames", kFrames3);
  egress("four frames: resident", kFrames4);
  egress("four frames, scalar", kFrames4, IMG, off(U8OUT, 1));
  img_faults("egress", Shape(), [&](const std::string& l, const Shape& s) { egress(l, s); });
  egress("egress: in NULL", Shape(), nullptr);
  egress("egress: out NULL", Shape(), IMG, nullptr);

  // ---- compose_white, PSNR, the loss terms and their backward
  for (int mk = 0; mk < 3; ++mk) {
    if (mk) {
      compose(S("mask kind %d: float4", mk), WITH(Pair, c.mk = mk));
      compose(S("mask kind %d: scalar, H*W %% 4 != 0", mk), WITH(Pair, c.mk = mk, c.H = 33, c.W = 7));
      compose(S("mask kind %d: mask 4 bytes off", mk), WITH(Pair, c.mk = mk, c.mask = off(MASK, 4)));
      compose(S("mask kind %d: four frames: resident", mk), WITH(Pair, c.mk = mk, c.shape(kFrames4)));
      if (mk == 1) {
        compose("out on the 4-byte grid", WITH(Pair, c.mk = mk), off(U8OUT, 4));
        compose("out off the 4-byte grid", WITH(Pair, c.mk = mk), off(U8OUT, 3));
        compose("three frames", WITH(Pair, c.mk = mk, c.shape(kFrames3)));
        compose("four frames, scalar", WITH(Pair, c.mk = mk, c.shape(kFrames4), c.a = off(IMG, 4)));
      }
    }
    for (auto fn : {psnr, loss, loss_bwd}) {
      fn(S("mask kind %d: float4", mk), WITH(Pair, c.mk = mk));
      fn(S("mask kind %d: scalar, H*W %% 4 != 0", mk), WITH(Pair, c.mk = mk, c.H = 33, c.W = 7));
      fn(S("mask kind %d: mask 4 bytes off", mk), WITH(Pair, c.mk = mk, c.mask = off(MASK, 4)));
      fn(S("mask kind %d: four frames (PSNR: resident)", mk), WITH(Pair, c.mk = mk, c.shape(kFrames4)));
      if (mk != 1) continue;
      fn("b off the grid", WITH(Pair, c.mk = mk, c.b = off(TGT, 4)));
      fn("three frames", WITH(Pair, c.mk = mk, c.shape(kFrames3)));
      fn("four frames, scalar", WITH(Pair, c.mk = mk, c.shape(kFrames4), c.a = off(IMG, 4)));
    }
  }
  loss("L_pred and L_target NULL", WITH(Pair, c.Lp = nullptr, c.Lt = nullptr));
  loss("L_target off the grid: scalar", WITH(Pair, c.Lt = off(LT, 4)));
  loss_bwd("grad_L_pred NULL", WITH(Pair, c.gLp = nullptr));
  loss_bwd("grad_pred off the grid: scalar", WITH(Pair, c.res = off(OUT, 4)));
  loss_bwd("grad_L_pred off the grid: scalar", WITH(Pair, c.gLp = off(GL, 4)));
  const auto goc = [](const std::string& l, const Pair& src) { compose(l, FROM(src, c.mk = 1)); };
  img_faults("compose", Pair(), goc);
  compose("compose: in NULL", WITH(Pair, c.mk = 1, c.a = nullptr));
  compose("compose: out NULL", WITH(Pair, c.mk = 1), nullptr);
  compose("compose: mask kind 0", Pair());
  compose("compose: mask kind 3", WITH(Pair, c.mk = 3));
  compose("compose: mask NULL", WITH(Pair, c.mk = 2, c.mask = nullptr));
  for (auto fn : {psnr, loss, loss_bwd}) {
    const char* who = fn == psnr ? "psnr" : fn == loss ? "loss_terms" : "loss_terms_bwd";
    img_faults(who, Pair(), fn);
    mask_faults(who, Pair(), fn);
    fn(S("%s: a NULL", who), WITH(Pair, c.a = nullptr));
    fn(S("%s: b NULL", who), WITH(Pair, c.b = nullptr));
    if (fn != loss_bwd) scratch_faults(who, Pair(), fn, false);
  }
  psnr("psnr: output NULL", WITH(Pair, c.res = nullptr));
  loss("loss_terms: sums NULL", WITH(Pair, c.sums = nullptr));
  loss_bwd("loss_terms_bwd: weights NULL", WITH(Pair, c.weights = nullptr));
  loss_bwd("loss_terms_bwd: grad_pred NULL", WITH(Pair, c.res = nullptr));

  // ---- MS-SSIM
  for (bool bwd : {false, true}) {
    const char* who = bwd ? "msssim bwd" : "msssim fwd";
    for (int w : {1, 11}) {
      msssim(S("window %d, 2x3x32x32", w), WITH(Pair, c.W = 32, c.window = w), bwd);
      msssim(S("window %d, 2x1x70x100", w), WITH(Pair, c.C = 1, c.H = 70, c.W = 100, c.window = w), bwd);
    }
    const auto gom = [bwd](const std::string& l, const Pair& c) { msssim(l, c, bwd); };
    scratch_faults(who, WITH(Pair, c.W = 32), gom, true);
    msssim(S("%s: a NULL", who), WITH(Pair, c.W = 32, c.a = nullptr), bwd);
    msssim(S("%s: b NULL", who), WITH(Pair, c.W = 32, c.b = nullptr), bwd);
    msssim(S("%s: first [B,5] pointer NULL", who), WITH(Pair, c.W = 32, c.Lp = nullptr), bwd);
    msssim(S("%s: second [B,5] pointer NULL", who), WITH(Pair, c.W = 32, c.Lt = nullptr), bwd);
    if (bwd) msssim(S("%s: grad_a NULL", who), WITH(Pair, c.W = 32, c.res = nullptr), bwd);
    msssim(S("%s: B = 0", who), WITH(Pair, c.W = 32, c.B = 0), bwd);
    msssim(S("%s: C = 0", who), WITH(Pair, c.W = 32, c.C = 0), bwd);
    msssim(S("%s: H = 31", who), WITH(Pair, c.W = 32, c.H = 31), bwd);
    msssim(S("%s: W = 31", who), WITH(Pair, c.W = 31), bwd);
    msssim(S("%s: H*W > 2^30", who), WITH(Pair, c.H = 32769, c.W = 32768), bwd);
    msssim(S("%s: B*C > 65535", who), WITH(Pair, c.W = 32, c.B = 21846), bwd);
    msssim(S("%s: window 13", who), WITH(Pair, c.W = 32, c.window = 13), bwd);
    msssim(S("%s: window 4", who), WITH(Pair, c.W = 32, c.window = 4), bwd);
    msssim(S("%s: window 0", who), WITH(Pair, c.W = 32, c.window = 0), bwd);
  }

  // ---- the fused layer + loss forward: both sides of its self-prep rule
  for (int mk = 0; mk < 3; ++mk) {
    layer_loss(S("mask kind %d: float4, small", mk), WITH(LayerLoss, c.mk = mk));
    layer_loss(S("mask kind %d: scalar", mk), WITH(LayerLoss, c.mk = mk, c.H = 33, c.W = 7));
  }
  layer_loss("self-prep at 2048 tiles: the crop batch", WITH(LayerLoss, c.shape(kCrops), c.mk = 1));
  layer_loss("no self-prep above: 2 x 257 x 1024 px = 2056 tiles", WITH(LayerLoss, c.B = 8, c.H = 257, c.W = 1024, c.mk = 1));
  layer_loss("two frames", WITH(LayerLoss, c.shape(kFrames2)));
  layer_loss("PREP 1 on a small launch", WITH(LayerLoss, c.flags = PREP(1)));
  layer_loss("PREP 2 on two frames", WITH(LayerLoss, c.shape(kFrames2), c.flags = PREP(2)));
  layer_loss("L_target off the grid: scalar", WITH(LayerLoss, c.Lt = off(LT, 4)));
  layer_loss("L_pred off the grid: scalar", WITH(LayerLoss, c.Lp = off(LP, 4)));
  layer_loss("target off the grid: scalar", WITH(LayerLoss, c.tgt = off(TGT, 8)));
  layer_loss("L planes, reg NULL", WITH(LayerLoss, c.Lp = nullptr, c.Lt = nullptr, c.reg = nullptr));
  layer_loss("uneven splits", WITH(LayerLoss, c.Kl = CURL_K_UNEVEN(16, 3), c.Kr = CURL_K_UNEVEN(8, 7)));
  const auto gol = [](const std::string& l, const LayerLoss& c) { layer_loss(l, c); };
  img_faults("layer_loss", LayerLoss(), gol);
  mask_faults("layer_loss", LayerLoss(), gol);
  ws_faults("layer_loss", LayerLoss(), gol);
  scratch_faults("layer_loss", LayerLoss(), gol, false);
  layer_loss("layer_loss: img NULL", WITH(LayerLoss, c.img = nullptr));
  layer_loss("layer_loss: out NULL", WITH(LayerLoss, c.out = nullptr));
  layer_loss("layer_loss: target NULL", WITH(LayerLoss, c.tgt = nullptr));
  layer_loss("layer_loss: sums NULL", WITH(LayerLoss, c.sums = nullptr));
  layer_loss("layer_loss: rawH NULL", WITH(LayerLoss, c.rH = nullptr));
  layer_loss("layer_loss: Kl = 1", WITH(LayerLoss, c.Kl = 1));
  layer_loss("layer_loss: grid too large", WITH(LayerLoss, c.B = 65535, c.H = 32768, c.W = 32768, c.img = off(IMG, 4)));
  tuning_faults("layer_loss", 0, [](const std::string& l, unsigned fl) { layer_loss(l, WITH(LayerLoss, c.flags = fl)); });
}

static void backward_cases() {
  // ---- the fused layer, affine and piecewise-linear
  for (bool pwl : {false, true}) {
    const char* who = pwl ? "layer_pwl_bwd" : "layer_bwd";
    for (int mk = 0; mk < 3; ++mk)
      for (bool gimg : {true, false}) {  // (CURL_F_WS_READY where grad_img is NULL: the training step's call)
        const unsigned fl = gimg ? 0u : CURL_F_WS_READY;
        layer_bwd(S("mask kind %d, grad_img %d, flags 0x%x: float4", mk, gimg, fl), WITH(LayerBwd, c.mk = mk, c.gimg = gimg ? GIMG : nullptr, c.flags = fl), pwl);
        layer_bwd(S("mask kind %d, grad_img %d, flags 0x%x: scalar", mk, gimg, fl), WITH(LayerBwd, c.mk = mk, c.H = 33, c.W = 7, c.gimg = gimg ? GIMG : nullptr, c.flags = fl), pwl);
      }
    layer_bwd("MASK_FIRST, uint8 mask", WITH(LayerBwd, c.mk = 1, c.flags = CURL_F_MASK_FIRST), pwl);
    layer_bwd("grad_out off the grid: scalar", WITH(LayerBwd, c.gout = off(GOUT, 4)), pwl);
    layer_bwd("grad_img off the grid: scalar", WITH(LayerBwd, c.gimg = off(GIMG, 4)), pwl);
    layer_bwd("mask off its grid: scalar", WITH(LayerBwd, c.mk = 2, c.mask = off(MASK, 4)), pwl);
    layer_bwd("the crop batch", WITH(LayerBwd, c.shape(kCrops), c.mk = 1, c.gimg = nullptr, c.flags = CURL_F_WS_READY), pwl);
    layer_bwd("grad_reg NULL", WITH(LayerBwd, c.greg = nullptr), pwl);
    layer_bwd("uneven splits", WITH(LayerBwd, c.Kl = CURL_K_UNEVEN(16, 3), c.Kh = CURL_K_UNEVEN(16, 15)), pwl);
    if (pwl) {  // (its dynamic LDS follows the knot counts)
      for (int K : {2, 16, 256}) layer_bwd(S("K = %d", K), WITH(LayerBwd, c.Kl = K, c.Kr = K, c.Kh = K), pwl);
      layer_bwd("Kl, Kr, Kh = 4, 8, 32", WITH(LayerBwd, c.Kl = 4, c.Kr = 8, c.Kh = 32), pwl);
    }
    const auto gob = [pwl](const std::string& l, const LayerBwd& c) { layer_bwd(l, c, pwl); };
    img_faults(who, LayerBwd(), gob);
    mask_faults(who, LayerBwd(), gob);
    ws_faults(who, LayerBwd(), gob);
    scratch_faults(who, LayerBwd(), gob, true);
    layer_bwd(S("%s: img NULL", who), WITH(LayerBwd, c.img = nullptr), pwl);
    layer_bwd(S("%s: grad_out NULL", who), WITH(LayerBwd, c.gout = nullptr), pwl);
    layer_bwd(S("%s: rawL NULL", who), WITH(LayerBwd, c.rL = nullptr), pwl);
    layer_bwd(S("%s: grad_rawL NULL", who), WITH(LayerBwd, c.gL = nullptr), pwl);
    layer_bwd(S("%s: grad_rawR NULL", who), WITH(LayerBwd, c.gR = nullptr), pwl);
    layer_bwd(S("%s: grad_rawH NULL", who), WITH(LayerBwd, c.gH = nullptr), pwl);
    layer_bwd(S("%s: Kr = 1", who), WITH(LayerBwd, c.Kr = 1), pwl);
    layer_bwd(S("%s: Kh = 257", who), WITH(LayerBwd, c.Kh = 257), pwl);
    layer_bwd(S("%s: grid too large", who), WITH(LayerBwd, c.B = 65535, c.H = 32768, c.W = 32768, c.img = off(IMG, 4), c.Kl = 2, c.Kr = 2, c.Kh = 2), pwl);
    layer_bwd(S("%s: a tuning bit", who), WITH(LayerBwd, c.flags = UNROLL(2)), pwl);
    tuning_faults(who, CURL_F_WS_READY, [pwl](const std::string& l, unsigned fl) { layer_bwd(l, WITH(LayerBwd, c.flags = fl), pwl); });
  }

  // ---- one knot segment
  for (SegFn f : {RGB, LAB, HSV, LAB_STAGE, HSV_STAGE}) {
    const char* n = kSegName[f];
    const bool stage = f >= LAB_STAGE;
    for (int mk = 0; mk < (stage ? 3 : 1); ++mk)
      for (bool gimg : {true, false}) {
        const unsigned fl = gimg ? 0u : CURL_F_WS_READY;
        seg_bwd(f, S("%s bwd: mask kind %d, grad_img %d, flags 0x%x: float4", n, mk, gimg, fl), WITH(Seg, c.mk = mk, c.gimg = gimg ? GIMG : nullptr, c.flags = fl));
        seg_bwd(f, S("%s bwd: mask kind %d, grad_img %d, flags 0x%x: scalar", n, mk, gimg, fl), WITH(Seg, c.mk = mk, c.H = 33, c.W = 7, c.gimg = gimg ? GIMG : nullptr, c.flags = fl));
      }
    seg_bwd(f, S("%s bwd: MASK_FIRST", n), WITH(Seg, c.mk = stage ? 1 : 0, c.flags = CURL_F_MASK_FIRST));
    seg_bwd(f, S("%s bwd: uneven split", n), WITH(Seg, c.K = CURL_K_UNEVEN(16, 9)));
    seg_bwd(f, S("%s bwd: one frame, grad_reg NULL", n), WITH(Seg, c.shape(kFrame), c.greg = nullptr));
    const auto gos = [f](const std::string& l, const Seg& c) { seg_bwd(f, l, c); };
    img_faults(n, Seg(), gos);
    ws_faults(n, Seg(), gos);
    scratch_faults(n, Seg(), gos, true);
    if (stage) mask_faults(n, Seg(), gos);
    seg_bwd(f, S("%s bwd: img NULL", n), WITH(Seg, c.img = nullptr));
    seg_bwd(f, S("%s bwd: grad_out NULL", n), WITH(Seg, c.gout = nullptr));
    seg_bwd(f, S("%s bwd: raw NULL", n), WITH(Seg, c.raw = nullptr));
    seg_bwd(f, S("%s bwd: grad_raw NULL", n), WITH(Seg, c.graw = nullptr));
    seg_bwd(f, S("%s bwd: K = 1", n), WITH(Seg, c.K = 1));
    seg_bwd(f, S("%s bwd: grid too large", n), WITH(Seg, c.B = 65535, c.H = 32768, c.W = 32768, c.img = off(IMG, 4), c.K = 2));
    tuning_faults(n, CURL_F_WS_READY, [f](const std::string& l, unsigned fl) { seg_bwd(f, l, WITH(Seg, c.flags = fl)); });
  }

  // ---- the polynomial model's coefficient gradient
  for (int nc : {126, 35}) {
    tri_bwd(S("nc %d: float4 (W = 36: 64 columns)", nc), WITH(Tri, c.nc = nc));
    tri_bwd(S("nc %d: W = 100: 128 columns", nc), WITH(Tri, c.nc = nc, c.H = 16, c.W = 100));
    tri_bwd(S("nc %d: W = 200: 256 columns", nc), WITH(Tri, c.nc = nc, c.H = 16, c.W = 200));
    tri_bwd(S("nc %d: W = 1500, one frame", nc), WITH(Tri, c.nc = nc, c.shape(kFrame)));
    tri_bwd(S("nc %d: 64 crops: steps on the upper clamp", nc), WITH(Tri, c.nc = nc, c.shape(kCrops), c.B = 64));
    tri_bwd(S("nc %d: steps between the clamps: 8 x 512 x 512", nc), WITH(Tri, c.nc = nc, c.B = 8, c.H = 512, c.W = 512));
    tri_bwd(S("nc %d: W = 1028", nc), WITH(Tri, c.nc = nc, c.H = 5, c.W = 1028));
    tri_bwd(S("nc %d: H*W %% 4 != 0", nc), WITH(Tri, c.nc = nc, c.H = 33, c.W = 7));
    tri_bwd(S("nc %d: W %% 4 != 0, H*W %% 4 == 0", nc), WITH(Tri, c.nc = nc, c.H = 4, c.W = 31));
    tri_bwd(S("nc %d: grad_out off the grid", nc), WITH(Tri, c.nc = nc, c.gout = off(GOUT, 4)));
    tri_bwd(S("nc %d: residual only", nc), WITH(Tri, c.nc = nc, c.flags = CURL_F_RESIDUAL_ONLY));
    tri_bwd(S("nc %d: grid too large", nc), WITH(Tri, c.nc = nc, c.B = 65535, c.H = 32768, c.W = 32768));
  }
  const auto got = [](const std::string& l, const Tri& c) { tri_bwd(l, c); };
  img_faults("trispace_bwd", Tri(), got);
  scratch_faults("trispace_bwd", Tri(), got, true);
  tri_bwd("trispace_bwd: img NULL", WITH(Tri, c.img = nullptr));
  tri_bwd("trispace_bwd: grad_out NULL", WITH(Tri, c.gout = nullptr));
  tri_bwd("trispace_bwd: coeffs NULL", WITH(Tri, c.coef = nullptr));
  tri_bwd("trispace_bwd: grad_coeffs NULL", WITH(Tri, c.gcoef = nullptr));
  tri_bwd("trispace_bwd: num_coeffs 125", WITH(Tri, c.nc = 125));
  tri_bwd("trispace_bwd: coeffs off the 8-byte grid", WITH(Tri, c.coef = off(COEF, 4)));
  tri_bwd("trispace_bwd 35: coeffs off the 4-byte grid", WITH(Tri, c.nc = 35, c.coef = off(COEF, 1)));
  tuning_faults("trispace_bwd", CURL_F_RESIDUAL_ONLY, [](const std::string& l, unsigned fl) { tri_bwd(l, WITH(Tri, c.flags = fl)); });

  // ---- the stand-alone polynomial layer's backward
  for (int V : {5, 3}) {
    poly_bwd(S("V %d: both gradients", V), WITH(Poly, c.V = V));
    poly_bwd(S("V %d: grad_img alone, no scratch", V), WITH(Poly, c.V = V, c.gcoef = nullptr, c.scr = nullptr, c.scrb = 0));
    poly_bwd(S("V %d: grad_coeffs alone", V), WITH(Poly, c.V = V, c.gimg = nullptr));
    poly_bwd(S("V %d: scalar, H*W %% 4 != 0", V), WITH(Poly, c.V = V, c.H = 33, c.W = 7));
    poly_bwd(S("V %d: grad_img off the grid: its kernel scalar, the coefficient pass float4", V), WITH(Poly, c.V = V, c.gimg = off(GIMG, 4)));
    poly_bwd(S("V %d: grad_out off the grid: both scalar", V), WITH(Poly, c.V = V, c.gout = off(GOUT, 4)));
    poly_bwd(S("V %d: steps on the lower clamp (4): one frame", V), WITH(Poly, c.V = V, c.shape(kFrame)));
    poly_bwd(S("V %d: steps between the clamps (8): 8 x 1024 x 1024", V), WITH(Poly, c.V = V, c.B = 8, c.H = 1024, c.W = 1024));
    poly_bwd(S("V %d: steps on the upper clamp (16): 32 x 1024 x 1024", V), WITH(Poly, c.V = V, c.B = 32, c.H = 1024, c.W = 1024));
  }
  const auto gop = [](const std::string& l, const Poly& c) { poly_bwd(l, c); };
  img_faults("poly_layer_bwd", Poly(), gop);
  scratch_faults("poly_layer_bwd", Poly(), gop, true);
  poly_bwd("poly_layer_bwd: img NULL", WITH(Poly, c.img = nullptr));
  poly_bwd("poly_layer_bwd: grad_out NULL", WITH(Poly, c.gout = nullptr));
  poly_bwd("poly_layer_bwd: coeffs NULL", WITH(Poly, c.coef = nullptr));
  poly_bwd("poly_layer_bwd: both gradients NULL", WITH(Poly, c.gimg = nullptr, c.gcoef = nullptr));
  poly_bwd("poly_layer_bwd: num_variables 4", WITH(Poly, c.V = 4));
  poly_bwd("poly_layer_bwd: any flag", WITH(Poly, c.flags = CURL_F_WS_READY));
  poly_bwd("poly_layer_bwd: grid too large", WITH(Poly, c.B = 65535, c.H = 32768, c.W = 32768));
}

static void size_cases() {
#define SHAPES(fn, ...)                                                                                            \
  SIZE(fn, 2, 32, 36, ##__VA_ARGS__), SIZE(fn, 2, 33, 7, ##__VA_ARGS__), SIZE(fn, 32, 256, 256, ##__VA_ARGS__),    \
      SIZE(fn, 1, 1000, 1500, ##__VA_ARGS__), SIZE(fn, 0, 32, 36, ##__VA_ARGS__), SIZE(fn, 2, 0, 36, ##__VA_ARGS__), \
      SIZE(fn, 2, 32, -1, ##__VA_ARGS__)
  SHAPES(curl_layer_bwd_scratch_bytes);
  SHAPES(curl_psnr_scratch_bytes);
  SHAPES(curl_loss_terms_scratch_bytes);
  for (int K : {2, 16, 256}) SHAPES(curl_layer_pwl_bwd_scratch_bytes, K, K, K);
  SHAPES(curl_layer_pwl_bwd_scratch_bytes, 1, 16, 16), SHAPES(curl_layer_pwl_bwd_scratch_bytes, 16, 257, 16);
  SHAPES(curl_layer_pwl_bwd_scratch_bytes, 16, 16, 0);
  SHAPES(curl_trispace_bwd_scratch_bytes, 126), SHAPES(curl_trispace_bwd_scratch_bytes, 35), SHAPES(curl_trispace_bwd_scratch_bytes, 34);
  SIZE(curl_trispace_bwd_scratch_bytes, 64, 256, 256, 126), SIZE(curl_trispace_bwd_scratch_bytes, 8, 512, 512, 126);
  SIZE(curl_trispace_bwd_scratch_bytes, 2, 16, 100, 126), SIZE(curl_trispace_bwd_scratch_bytes, 2, 16, 200, 126);
  SHAPES(curl_poly_layer_bwd_scratch_bytes, 5), SHAPES(curl_poly_layer_bwd_scratch_bytes, 3), SHAPES(curl_poly_layer_bwd_scratch_bytes, 4);
  SIZE(curl_poly_layer_bwd_scratch_bytes, 8, 1024, 1024, 5), SIZE(curl_poly_layer_bwd_scratch_bytes, 32, 1024, 1024, 3);
  SIZE(curl_msssim_scratch_bytes, 2, 3, 32, 32), SIZE(curl_msssim_scratch_bytes, 2, 1, 70, 100), SIZE(curl_msssim_scratch_bytes, 32, 1, 256, 256);
  SIZE(curl_msssim_scratch_bytes, 0, 3, 32, 32), SIZE(curl_msssim_scratch_bytes, 2, 0, 32, 32), SIZE(curl_msssim_scratch_bytes, 2, 3, 0, 32);
  SIZE(curl_msssim_scratch_bytes, 2, 3, 32, -4);
  SIZE(curl_workspace_bytes, 2, 160), SIZE(curl_workspace_bytes, 32, 48), SIZE(curl_workspace_bytes, 1, 61), SIZE(curl_workspace_bytes, 1, 2560);
  SIZE(curl_workspace_bytes, 1, 0), SIZE(curl_workspace_bytes, 0, 160), SIZE(curl_workspace_bytes, 2, -1);
#undef SHAPES
}

// ---------------------------------------------------------------------------------------------------------------
// coverage: every launch site of host_api.inc recorded, every declared entry point called
// ---------------------------------------------------------------------------------------------------------------
// A launch site is the line on which a statement that names the launch macro ends (its `;`): that is the line __LINE__
// gives.  (host_api.inc writes no launch inside a macro of its own; one that did would be counted at its #define and fail
// the comparison with the lines recorded, which are those that expand it.)
static std::set<int> launch_sites(const char* path) {
  std::ifstream f(path);
  std::set<int> sites;
  std::string line;
  bool open = false;  // a launching statement has begun and its `;` is still to come
  for (int no = 1; std::getline(f, line); ++no) {
    size_t from = open ? 0 : line.find("hipLaunchKernelGGL");
    while (from != std::string::npos) {
      const size_t semi = line.find(';', from);
      open = semi == std::string::npos;
      if (open) break;
      sites.insert(no);
      from = line.find("hipLaunchKernelGGL", semi);
    }
  }
  return sites;
}
static std::set<std::string> declared_entries(const char* path) {
  std::ifstream f(path);
  std::set<std::string> names;
  std::string line;
  const std::regex decl(R"(^(?:int|size_t)\s+(curl_\w+)\s*\()");
  std::smatch m;
  while (std::getline(f, line))
    if (std::regex_search(line, m, decl) && m[1] != "curl_version") names.insert(m[1]);
  return names;
}

int main(int argc, char** argv) {
  if (argc > 1 && std::string(argv[1]) == "-v") g_verbose = true, --argc, ++argv;
  if (argc != 3) return fprintf(stderr, "usage: launch_plan_twin [-v] <host_api.inc> <curl_hip.h>\n"), 2;
  stream_cases();
  pointwise_cases();
  backward_cases();
  size_cases();
  g_out += "\n";
  print_failed();
  fputs(g_out.c_str(), stdout);
  int bad = 0;
  const std::set<int> sites = launch_sites(argv[1]);
  for (int l : sites)
    if (!g_lines.count(l)) ++bad, fprintf(stderr, "launch site never reached: %s:%d\n", argv[1], l);
  for (int l : g_lines)
    if (!sites.count(l)) ++bad, fprintf(stderr, "launch recorded at a line that is no launch site: %s:%d\n", argv[1], l);
  const std::set<std::string> entries = declared_entries(argv[2]);
  for (const std::string& e : entries)
    if (!g_called.count(e)) ++bad, fprintf(stderr, "entry point never called: %s\n", e.c_str());
  for (const std::string& e : g_called)
    if (!entries.count(e)) ++bad, fprintf(stderr, "called but not declared in %s: %s\n", argv[2], e.c_str());
  fprintf(stderr, "%d calls, %d launches, %zu launch sites, %zu entry points%s\n", g_calls, g_launches, sites.size(), entries.size(),
          bad ? ": COVERAGE INCOMPLETE" : "");
  return bad ? 1 : 0;
}
