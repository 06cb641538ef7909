// ops.inc -- part of curl_kernels.hip (one translation unit; included in this order, not compiled alone).
// ------------------------------------------------------------------------------------------------
// ops
// ------------------------------------------------------------------------------------------------
struct NoK {};
struct OpDefaults {
  static constexpr bool kSingleTileShape = false;
  static constexpr int kLdsFloats = 0;  // per-image table the block stages in LDS before the tile (0 = none)
  static constexpr int kMinWavesPerSimd = 1;  // __launch_bounds__ second argument (register budget)
  // true: a block never crosses an image row (grid.x = blocks per row x rows, blockDim.x <= 256 follows the row
  // width) and the LDS table is built per row by Op::stage_value(table, i, row, args)
  static constexpr bool kRowTiles = false;
  // true: the LDS table is built element by element by Op::stage_value(table, i, row, args) (row = 0 here)
  static constexpr bool kStageValue = false;
  // > 0: the first kRawFloats floats of the image's table are copied to LDS first (coalesced, independent loads) and
  // stage_value reads THAT copy (an even number; the table must be 8-byte aligned)
  static constexpr int kRawFloats = 0;
  // Resident 256-thread workgroups per CU (= waves per SIMD) a LARGE launch of the float4 kernel is held to, with ONE
  // float4 group per lane (0: no cap, kUnroll groups per lane).  The memory system moves the path's six planes fastest
  // with just enough waves in flight to cover the op's own arithmetic: the bare 3-plane copy takes 200.5 us at 8
  // waves per SIMD, 186.7 with two groups per lane -- and 174.9 (6.58 TB/s) at 2-3 waves per SIMD
  // (tools/ubench/occ.hip, profiles/r03/exp27i_residency.log).  Per op from tools/occ_sweep.py
  // (exp27j_occ_sweep_true_residency.log); realised by reserving LDS nobody touches (host_api.inc lds_for_resident).
  static constexpr int kResident = 0;
  // bool / uint8 masks: run the mask-first kernel variant even without CURL_F_MASK_FIRST (no op does: on an all-ones mask it
  // costs the layer 0.5-0.8 %, the Lab stage 1 %, the HSV stage -1.7 ... +0.4 %; profiles/r03/exp29, exp32)
  static constexpr bool kMaskFirst = false;
  // the op's per-image table is the head of the knot workspace row (collapsed curves, masked-out colour): small launches
  // may then collapse the curves inside the streaming kernel (stream_selfprep_kernel) instead of in a launch of their own
  static constexpr bool kSelfPrep = false;
};
#define CONVERTER_OP(NAME, FN, RES)                                                      \
  struct NAME : OpDefaults {                                                             \
    typedef NoK K;                                                                       \
    static constexpr bool kMask = false;                                                 \
    static constexpr int kUnroll = 2;                                                    \
    static constexpr int kResident = RES;                                                \
    static __device__ __forceinline__ K load(const float*, const StreamArgs&) { return K{}; } \
    template <bool, int N>                                                               \
    static __device__ __forceinline__ void apply_n(PxN<N>& p, const float (&)[N], const K&, unsigned) { FN(p); } \
    static constexpr bool kBlendMaskedOut = false;                                       \
    static __device__ __forceinline__ Px masked_out(const K&) { return Px{0.0f, 0.0f, 0.0f}; } \
  };
CONVERTER_OP(OpRgb2Lab, rgb2lab_n<N>, 4)  // 187.6 us uncapped (186.5 at two groups per lane) -> 178.4
CONVERTER_OP(OpLab2Rgb, lab2rgb_n<N>, 4)  // 185.8 -> 179.0
CONVERTER_OP(OpRgb2Hsv, rgb2hsv_n<N>, 3)  // 186.6 -> 177.2
CONVERTER_OP(OpHsv2Rgb, hsv2rgb_n<N>, 2)  // 186.2 -> 173.5

__device__ __forceinline__ Affine load_affine(const float* ws, int c) {
  return Affine{ws[WS_COEF + 2 * c], ws[WS_COEF + 2 * c + 1]};
}

struct OpAdjust3 : OpDefaults {
  static constexpr bool kSelfPrep = true;  // adjust_rgb / adjust_lab, affine form
  struct K {
    Affine k[3];
  };
  static constexpr bool kMask = false;
  static constexpr int kUnroll = 2;
  static constexpr int kResident = 2;  // 190.2 -> 177.5 us (3: 183.9, 4: 195.1)
  static __device__ __forceinline__ K load(const float* ws, const StreamArgs&) {
    K k;
#pragma unroll
    for (int c = 0; c < 3; ++c) k.k[c] = load_affine(ws, c);
    return k;
  }
  template <bool, int N>
  static __device__ __forceinline__ void apply_n(PxN<N>& p, const float (&)[N], const K& k, unsigned) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      Px o = adjust3(Px{p.c0[i], p.c1[i], p.c2[i]}, k.k[0], k.k[1], k.k[2]);
      p.c0[i] = o.c0, p.c1[i] = o.c1, p.c2[i] = o.c2;
    }
  }
  static constexpr bool kBlendMaskedOut = false;
  static __device__ __forceinline__ Px masked_out(const K&) { return Px{0.0f, 0.0f, 0.0f}; }
};
struct OpAdjustHsv : OpDefaults {
  static constexpr bool kSelfPrep = true;
  struct K {
    Affine k[4];
  };
  static constexpr bool kMask = false;
  static constexpr int kUnroll = 2;
  static constexpr int kResident = 2;  // 189.8 -> 177.0 us
  static __device__ __forceinline__ K load(const float* ws, const StreamArgs&) {
    K k;
#pragma unroll
    for (int c = 0; c < 4; ++c) k.k[c] = load_affine(ws, c);
    return k;
  }
  template <bool, int N>
  static __device__ __forceinline__ void apply_n(PxN<N>& p, const float (&)[N], const K& k, unsigned) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      Px o = adjust_hsv4(Px{p.c0[i], p.c1[i], p.c2[i]}, k.k[0], k.k[1], k.k[2], k.k[3]);
      p.c0[i] = o.c0, p.c1[i] = o.c1, p.c2[i] = o.c2;
    }
  }
  static constexpr bool kBlendMaskedOut = false;
  static __device__ __forceinline__ Px masked_out(const K&) { return Px{0.0f, 0.0f, 0.0f}; }
};
struct OpLabStage : OpDefaults {
  static constexpr bool kSelfPrep = true;
  struct K {
    Affine k[3];
    Px masked;
  };
  static constexpr bool kMask = true;
  static constexpr int kUnroll = 1;  // arithmetic-heavy: occupancy beats per-lane ILP (profiles/sweep_r01.md)
  static constexpr int kResident = 6;  // 196.1 -> 191.1 us (7: 193.9, 5: 195.9, 4: 202.1; the layer: 7 = 8)
  static __device__ __forceinline__ K load(const float* ws, const StreamArgs&) {
    K k;
#pragma unroll
    for (int c = 0; c < 3; ++c) k.k[c] = load_affine(ws, c);
    k.masked = Px{ws[WS_MASKED], ws[WS_MASKED + 1], ws[WS_MASKED + 2]};
    return k;
  }
  template <bool BINARY, int N>
  static __device__ __forceinline__ void apply_n(PxN<N>& p, const float (&m)[N], const K& k, unsigned) {
    lab_stage_n<BINARY, N>(p, m, k.k);
  }
  static constexpr bool kBlendMaskedOut = true;  // lab_stage<true> computes m == 0 pixels as if m == 1
  static __device__ __forceinline__ Px masked_out(const K& k) { return k.masked; }
};
// model.py:163-169: RGB -> HSV -> adjust_hsv -> *mask -> RGB, the third "one fused kernel per colour space" of the
// north star (RGB: OpAdjust3, Lab: OpLabStage).  Memory-bound like the Lab stage: 24 / 25 / 28 B/px, ~75 VALU per pixel.
struct OpHsvStage : OpDefaults {
  static constexpr bool kSelfPrep = true;
  struct K {
    Affine k[4];
  };
  static constexpr bool kMask = true;
  static constexpr int kUnroll = 2;  // 63 instructions per pixel: on the copy-like side (one group per lane: +2.0 %, four: +4.6 %; exp12)
  static constexpr int kResident = 4;  // ... and at 3-4 waves per SIMD one group per lane wins: 201.8 -> 190.7 us
  static __device__ __forceinline__ K load(const float* ws, const StreamArgs&) {
    K k;
#pragma unroll
    for (int c = 0; c < 4; ++c) k.k[c] = load_affine(ws, c);
    return k;
  }
  template <bool BINARY, int N>
  static __device__ __forceinline__ void apply_n(PxN<N>& p, const float (&m)[N], const K& k, unsigned) {
    hsv_stage_n<BINARY, N>(p, m, k.k);
  }
  static constexpr bool kBlendMaskedOut = false;  // hsv_stage_n ends in `* m` for a binary mask: m == 0 pixels are 0
  static __device__ __forceinline__ Px masked_out(const K&) { return Px{0.0f, 0.0f, 0.0f}; }  // hsv2rgb(0,0,0)
};
// The same stage with the PAPER's curve (CURL_F_PWL): each of the three Lab curves is the clamped piecewise-linear
// interpolation of its K knots.  Knots and slopes of the image live in LDS; knots are uniformly spaced, so the
// interval is the direct index floor((K-1) x) (no search) and a pixel costs two per-lane LDS gathers and one fma
// per curve.  Not the reference's arithmetic (its apply_curve never clamps S x - j, DESIGN.md 1): an explicit option.
template <int MODE>  // 0: CURL_F_PWL, 1: CURL_F_EXACT_ORDER (the reference's in-order sum per curve: the validation mode)
struct OpLabStageTab : OpDefaults {
  struct K {
    const float* tab;  // {knot, slope} pairs of the 3 curves, back to back; then the masked-out colour
    int n;             // knots per curve
    Px masked;
  };
  static constexpr bool kMask = true;
  static constexpr int kUnroll = 1;
  static constexpr bool kSingleTileShape = true;
  static constexpr bool kStageValue = true;
  static constexpr int kLdsFloats = 6 * CURL_MAX_KNOTS + 4;
  static __device__ __forceinline__ unsigned lds_count(const StreamArgs& a) { return 6u * (unsigned)a.op_flag + 3u; }
  static __device__ __forceinline__ float stage_value(const float* ws, unsigned i, unsigned, const StreamArgs& a) {
    const unsigned Kn = (unsigned)a.op_flag, n6 = 6u * Kn;
    if (i >= n6) return ws[WS_MASKED + (i - n6)];
    unsigned j = i >> 1, jj = j % Kn;  // knot j (curve j / Kn), pair element i & 1
    float c = ws[WS_KNOTS + j];
    if ((i & 1u) == 0u) return c;
    return (jj + 1u < Kn) ? ws[WS_KNOTS + j + 1u] - c : 0.0f;  // curves.py:19
  }
  static __device__ __forceinline__ K load(const float* lds, const StreamArgs& a) {
    const int n6 = 6 * a.op_flag;
    return K{lds, a.op_flag, Px{lds[n6], lds[n6 + 1], lds[n6 + 2]}};
  }
  template <bool BINARY, int N>
  static __device__ __forceinline__ void apply_n(PxN<N>& p, const float (&m)[N], const K& k, unsigned) {
    rgb2lab_n<N>(p);
    const float* T = k.tab;
#pragma unroll
    for (int i = 0; i < N; ++i) {
      // adjust_lab's structure (curves.py:136-180): channel 0 meets its curve unclamped, 1 and 2 clamped first
      float c0 = clamp01(p.c0[i] * scale_tab<MODE>(p.c0[i], T, k.n));
      float c1 = clamp01(p.c1[i]), c2 = clamp01(p.c2[i]);
      c1 = clamp01(c1 * scale_tab<MODE>(c1, T + 2 * k.n, k.n));
      c2 = clamp01(c2 * scale_tab<MODE>(c2, T + 4 * k.n, k.n));
      if (!BINARY) c0 *= m[i], c1 *= m[i], c2 *= m[i];
      p.c0[i] = c0, p.c1[i] = c1, p.c2[i] = c2;
    }
    lab2rgb_n<N>(p);
  }
  static constexpr bool kBlendMaskedOut = true;
  static __device__ __forceinline__ Px masked_out(const K& k) { return k.masked; }
};
struct OpLayer : OpDefaults {
  static constexpr bool kSelfPrep = true;
  typedef LayerCoef K;
  static constexpr bool kMask = true;
  static constexpr int kUnroll = 1;
  static __device__ __forceinline__ K load(const float* ws, const StreamArgs&) {
    K k;
#pragma unroll
    for (int c = 0; c < 3; ++c) k.lab[c] = load_affine(ws, c);
#pragma unroll
    for (int c = 0; c < 3; ++c) k.rgb[c] = load_affine(ws, 3 + c);
#pragma unroll
    for (int c = 0; c < 4; ++c) k.hsv[c] = load_affine(ws, 6 + c);
    return k;
  }
  template <bool BINARY, int N>
  static __device__ __forceinline__ void apply_n(PxN<N>& p, const float (&m)[N], const K& k, unsigned) {
    curl_layer_n<BINARY, N>(p, m, k);
  }
  static constexpr bool kBlendMaskedOut = false;  // curl_layer ends in `* m` for every mask kind
  static __device__ __forceinline__ Px masked_out(const K&) { return Px{0.0f, 0.0f, 0.0f}; }
};

// CURLLayer.forward with the paper's clamped piecewise-linear curves (CURL_F_PWL): all ten curves' knots and slopes of
// the image in LDS.  op_flag packs the knots per curve: Kl | Kr << 10 | Kh << 20.
template <int MODE>  // 0: CURL_F_PWL, 1: CURL_F_EXACT_ORDER
struct OpLayerTab : OpDefaults {
  struct K {
    const float* tab;  // {knot, slope} pairs of the 10 curves, back to back (3 x Kl, 3 x Kr, 4 x Kh)
    int kl, kr, kh;
  };
  static constexpr bool kMask = true;
  static constexpr int kUnroll = 1;
  static constexpr bool kSingleTileShape = true;
  static constexpr bool kStageValue = true;
  static constexpr int kLdsFloats = 2 * MAX_CURVES * CURL_MAX_KNOTS;
  static __device__ __forceinline__ int n_knots(int f) { return 3 * (f & 1023) + 3 * ((f >> 10) & 1023) + 4 * (f >> 20); }
  static __device__ __forceinline__ unsigned lds_count(const StreamArgs& a) { return 2u * (unsigned)n_knots(a.op_flag); }
  static __device__ __forceinline__ float stage_value(const float* ws, unsigned i, unsigned, const StreamArgs& a) {
    const int f = a.op_flag;
    const unsigned kl = f & 1023, kr = (f >> 10) & 1023, kh = f >> 20, j = i >> 1;
    float c = ws[WS_KNOTS + j];
    if ((i & 1u) == 0u) return c;
    // slope j = C[j+1] - C[j] inside its curve, 0 for the curve's last knot (curves.py:19)
    unsigned in_curve = j < 3u * kl ? j % kl : j < 3u * kl + 3u * kr ? (j - 3u * kl) % kr : (j - 3u * kl - 3u * kr) % kh;
    unsigned Kc = j < 3u * kl ? kl : j < 3u * kl + 3u * kr ? kr : kh;
    return (in_curve + 1u < Kc) ? ws[WS_KNOTS + j + 1u] - c : 0.0f;
  }
  static __device__ __forceinline__ K load(const float* lds, const StreamArgs& a) {
    const int f = a.op_flag;
    return K{lds, f & 1023, (f >> 10) & 1023, f >> 20};
  }
  // adjust_rgb / adjust_lab with PWL curves: channel 0 unclamped into its curve, 1 and 2 clamped first (curves.py:36)
  static __device__ __forceinline__ Px adjust3_pwl(Px p, const float* T, int Kc) {
    Px o;
    o.c0 = clamp01(p.c0 * scale_tab<MODE>(p.c0, T, Kc));
    float c1 = clamp01(p.c1), c2 = clamp01(p.c2);
    o.c1 = clamp01(c1 * scale_tab<MODE>(c1, T + 2 * Kc, Kc));
    o.c2 = clamp01(c2 * scale_tab<MODE>(c2, T + 4 * Kc, Kc));
    return o;
  }
  template <bool BINARY, int N>
  static __device__ __forceinline__ void apply_n(PxN<N>& p, const float (&m)[N], const K& k, unsigned) {
    const PxN<N> in = p;
    const float *Tl = k.tab, *Tr = k.tab + 6 * k.kl, *Th = Tr + 6 * k.kr;
    rgb2lab_n<N>(p);
#pragma unroll
    for (int i = 0; i < N; ++i) {
      Px o = adjust3_pwl(Px{p.c0[i], p.c1[i], p.c2[i]}, Tl, k.kl);
      p.c0[i] = o.c0 * m[i], p.c1[i] = o.c1 * m[i], p.c2[i] = o.c2 * m[i];  // model.py:154
    }
    lab2rgb_n<N>(p);
#pragma unroll
    for (int i = 0; i < N; ++i) {
      Px o = adjust3_pwl(Px{p.c0[i], p.c1[i], p.c2[i]}, Tr, k.kr);
      p.c0[i] = o.c0 * m[i], p.c1[i] = o.c1 * m[i], p.c2[i] = o.c2 * m[i];  // model.py:160
    }
    rgb2hsv_n<N>(p);
#pragma unroll
    for (int i = 0; i < N; ++i) {
      // adjust_hsv (curves.py:41-87): H->H, H->S on the adjusted hue, S->S, V->V
      float h = clamp01(p.c0[i] * scale_tab<MODE>(p.c0[i], Th, k.kh));
      float sc = clamp01(p.c1[i]), vc = clamp01(p.c2[i]);
      sc = clamp01(sc * scale_tab<MODE>(h, Th + 2 * k.kh, k.kh));
      sc = clamp01(sc * scale_tab<MODE>(sc, Th + 4 * k.kh, k.kh));
      vc = clamp01(vc * scale_tab<MODE>(vc, Th + 6 * k.kh, k.kh));
      Px res = hsv2rgb(Px{h * m[i], sc * m[i], vc * m[i]});  // model.py:166,169
      p.c0[i] = clamp01(in.c0[i] + res.c0) * m[i];            // model.py:170
      p.c1[i] = clamp01(in.c1[i] + res.c1) * m[i];
      p.c2[i] = clamp01(in.c2[i] + res.c2) * m[i];
    }
  }
  static constexpr bool kBlendMaskedOut = false;
  static __device__ __forceinline__ Px masked_out(const K&) { return Px{0.0f, 0.0f, 0.0f}; }
};

// TriSpaceRegNet.generate_residual (+ generate_image), model.py:499-520: three degree-4 polynomial layers in
// RGB / Lab / HSV + converters, one pass.  The 9 x NC coefficients of the image are staged in LDS by the block
// (kLdsFloats) and reach the packed FMAs as broadcast ds_read_b128 -> VGPR halves (op_sel).  Reading them
// through a uniform global pointer instead made hipcc hoist all 1134 scalar loads and spill SGPRs into VGPR
// lanes (3000 v_readlane/v_writelane per thread, 4.4 ms per batch).
// D = the polynomial order: OpTriSpace<V> is order 4, OpTriSpaceOrder<V, D> the orders below it.  Instantiated for V = 3 (the
// non-spatial model) at every order and for V = 5 at orders 1-3; the spatial order-4 form runs as OpTriSpaceRows below
// (OpTriSpace<5> is the earlier, 125-FMAs-per-output version of the same computation).  Orders 1-3 cost 55 / 20 / 5 FMAs per output with both coordinates
// kept as variables: already fewer than the 69 the order-4 row fold leaves, on tiles that may cross rows and from a table
// that needs a float's own alignment only (the row fold copies the raw table as 8-byte pairs: 9 x 21 floats is odd).
template <int V, int D>
struct OpTriSpaceOrder : OpDefaults {
  struct K {
    const float* coef;
    unsigned W, row0;  // row0: the slab's first row (the coordinates are the full image's)
    float fW, fH;
    bool residual_only;
  };
  static constexpr bool kMask = false;
  static constexpr int kUnroll = 1;
  static constexpr bool kSingleTileShape = true;
  static constexpr int kLdsFloats = 9 * PolyEval<V, D>::kSeqStride;
  static constexpr int kMinWavesPerSimd = kTriSpaceWaves;
  static __device__ __forceinline__ int stage_index(int i) { return poly_seq_index<V, D>(i); }
  static constexpr bool kBlendMaskedOut = false;
  static __device__ __forceinline__ K load(const float* coef_img, const StreamArgs& a) {
    return K{coef_img, a.W, a.row0, (float)a.W, (float)a.H, a.op_flag != 0};
  }
  template <bool, int N>
  static __device__ __forceinline__ void apply_n(PxN<N>& p, const float (&)[N], const K& k, unsigned pix0) {
    float xw[N], yh[N];
    if (V == 5) {  // cat_coords (model.py:487-497): column / width, row / height, true division
      unsigned row = pix0 / k.W, col = pix0 - row * k.W;
#pragma unroll
      for (int i = 0; i < N; ++i) {
        xw[i] = (float)col / k.fW;
        yh[i] = (float)(row + k.row0) / k.fH;
        if (++col == k.W) col = 0, ++row;
      }
    }
    trispace_n<V, N, true, D>(p, xw, yh, k.coef, k.residual_only);
  }
  static __device__ __forceinline__ Px masked_out(const K&) { return Px{0.0f, 0.0f, 0.0f}; }
};

template <int V>
struct OpTriSpace : OpTriSpaceOrder<V, 4> {};

// The spatial polynomial path, one image row per block.  cat_coords' y = row/height is the same for every pixel
// of a row, so the block folds y into the coefficients first (9 polynomials x 70 collapsed coefficients, <= 4
// FMAs each, a handful per thread; collapse_coef) and leaves them in LDS in the consumption order of the
// 4-variable Horner scheme: a pixel then costs 9 x 69 FMAs instead of 9 x 125.
struct OpTriSpaceRows : OpDefaults {
  struct K {
    const float* coef;
    unsigned W;
    float fW, rW;
    bool residual_only;
  };
  static constexpr bool kMask = false;
  static constexpr int kUnroll = 1;
  static constexpr bool kSingleTileShape = true;
  static constexpr bool kRowTiles = true;
  static constexpr int kLdsFloats = 9 * PolyEval<4>::kSeqStride;
  static __device__ __forceinline__ unsigned lds_count(const StreamArgs&) { return kLdsFloats; }
  static constexpr int kMinWavesPerSimd = kTriSpaceWaves;
  // Folding a coefficient reads up to 5 of the image's 1134 raw coefficients through an index table.  Straight from
  // global memory that is a chain of ~12 dependent loads per folded coefficient, ~40 per thread: as long as the
  // row's arithmetic.  The raw block therefore goes to LDS first (three independent 8-byte loads per thread), and
  // a fold is one 16-byte table row + up to 5 LDS reads.
  static constexpr int kRawFloats = 9 * PolyEval<5>::kCoeffs;
  static __device__ __forceinline__ float stage_value(const float* raw, unsigned i, unsigned row, const StreamArgs& a) {
    constexpr unsigned NC4 = PolyEval<4>::kCoeffs, NS4 = PolyEval<4>::kSeqStride, NC5 = PolyEval<5>::kCoeffs;
    unsigned q = i / NS4, pos = i - q * NS4;
    if (pos >= NC4) return 0.0f;  // padding to a 16-byte multiple per polynomial
    return collapse_coef_fold(raw + q * NC5, (int)pos, (float)row / (float)a.H);  // row / height: true division
  }
  static constexpr bool kBlendMaskedOut = false;
  static __device__ __forceinline__ K load(const float* coef_row, const StreamArgs& a) {
    return K{coef_row, a.W, (float)a.W, 1.0f / (float)a.W, a.op_flag != 0};
  }
  template <bool, int N>
  static __device__ __forceinline__ void apply_n(PxN<N>& p, const float (&)[N], const K& k, unsigned pix0) {
    float xw[N], yh[N];
    unsigned col = pix0 % k.W;  // a row tile never wraps
#pragma unroll
    for (int i = 0; i < N; ++i) xw[i] = div_small((float)(col + i), k.fW, k.rW), yh[i] = 0.0f;  // column / width
    trispace_n<4, N, true>(p, xw, yh, k.coef, k.residual_only);
  }
  static __device__ __forceinline__ Px masked_out(const K&) { return Px{0.0f, 0.0f, 0.0f}; }
};

// ChannelPolyLayer / Deg4MobilePolyLayer forward (model.py:295-333, 399-415): img [B,V,H,W] -> [B,3,H,W].
// The image's 3 x NC coefficients go to LDS in the order the Horner scheme consumes them (as OpTriSpace stages its nine
// polynomials); a lane owns VEC pixels = VEC / 2 packed chains per coefficient read (VEC = 4: float4 loads per plane; 1: any
// size or alignment, scalar chains).  n = HW / VEC.
template <int V, int VEC, int D>
__device__ __forceinline__ void poly_layer_block(const float* in, const float* coeffs, float* out, unsigned n) {
  typedef typename Pack<VEC>::T T;
  constexpr int NC = PolyEval<V, D>::kCoeffs, NS = PolyEval<V, D>::kSeqStride;
  __shared__ __attribute__((aligned(16))) float s_coef[3 * NS];
  const unsigned img = blockIdx.y;
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  const size_t plane = (size_t)n;
  const T* p = reinterpret_cast<const T*>(in) + (size_t)img * V * plane + min(i, n - 1u);
  T x[V];
#pragma unroll
  for (int k = 0; k < V; ++k) x[k] = ld<true>(p + (size_t)k * plane);  // before the staging barrier
  const float* table = coeffs + (size_t)img * 3 * NC;
  // (unsigned: the index is never negative, and said so it is not sign-extended into the address)
  for (int j = threadIdx.x; j < 3 * NS; j += 256) s_coef[j] = table[(unsigned)poly_seq_index<V, D>(j)];
  __syncthreads();
  if (i >= n) return;
  // VEC SCALAR Horner chains per lane in lock step (the generated scheme's pixel loop with F = float): they share every
  // coefficient read and are each other's ILP, and scalar FMAs of different waves issue two per quad-cycle (DESIGN.md 3c).
  // (The packed 5-variable scheme as a stand-alone kernel spilled 370 registers at 128 and 290 at 256; inside the fused
  // polynomial path the row fold leaves 4 variables.)
  float o[3][VEC], vs[VEC][V], rs[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e)
#pragma unroll
    for (int k = 0; k < V; ++k) vs[e][k] = lane(x[k], e);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    CURL_FENCE();
    PolyEval<V, D>::template eval<float, true, VEC>(rs, vs, s_coef + c * NS);
#pragma unroll
    for (int e = 0; e < VEC; ++e) o[c][e] = rs[e];
  }
  T* q = reinterpret_cast<T*>(out) + (size_t)img * 3 * plane + i;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    T y;
#pragma unroll
    for (int e = 0; e < VEC; ++e) set_lane(y, e, o[c][e]);
    st<true>(q + (size_t)c * plane, y);
  }
}
// degree 4, and the degrees below it (ChannelPolyLayer(degree): model.py:206-216)
template <int V, int VEC>
__global__ __launch_bounds__(256, 4) void poly_layer_kernel(const float* in, const float* coeffs, float* out, unsigned n) {
  poly_layer_block<V, VEC, 4>(in, coeffs, out, n);
}
template <int V, int VEC, int D>
__global__ __launch_bounds__(256, 4) void poly_layer_order_kernel(const float* in, const float* coeffs, float* out, unsigned n) {
  poly_layer_block<V, VEC, D>(in, coeffs, out, n);
}
