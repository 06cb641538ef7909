// stream.inc -- part of curl_kernels.hip (one translation unit; included in this order, not compiled alone).
// ------------------------------------------------------------------------------------------------
// streaming skeleton
// ------------------------------------------------------------------------------------------------
typedef float v4f __attribute__((ext_vector_type(4)));
// four mask bytes of a lane travel as ONE dword (as a 4 x uint8 vector hipcc unpacked them into four registers after the
// load and re-packed them for the wave's all-set / all-clear tests: 17 VALU instructions per wave for nothing)
typedef unsigned v4b;

struct StreamArgs {
  const float* in;
  float* out;
  const void* mask;   // [B,1,H,W] u8 or f32, or NULL
  const float* coef;  // workspace base (per-image stride below) or NULL
  unsigned coef_stride;
  unsigned n;                 // elements per plane in units of VEC floats
  unsigned blocks_per_image;  // chunks per image
  unsigned n_blocks;          // total
  int no_mem;  // diagnostics: synthesise inputs, suppress stores (VALU-only timing; results undefined)
  unsigned W, H;  // image size in pixels (ops that need pixel coordinates)
  int op_flag;    // op-specific (trispace: residual only)
  int mask_first;  // host side only: launch the MASK_FIRST variant of the kernel (bool / uint8 masks, float4, one group per lane)
  const uint8_t* white;  // FMT_U8HWC only: [B,H,W] 'L' mask of infer.py:39,46 (out*m + (1-m), m = L/255) or NULL
  unsigned units, segs;  // Op::kRowTiles only: VEC-pixel groups per image row, blocks per row
  // Row slabs (curl_*_slab_f32: the split-pixels layout, one slab of every image per GPU): `n` VEC-groups are
  // processed per plane, starting `off` groups into planes that are `plane` groups apart; `row0` is the slab's first
  // image row and H stays the FULL height (pixel coordinates of the polynomial model).  Whole images: plane = n,
  // off = 0, row0 = 0.
  unsigned plane, off, row0;
  // XCD-contiguous tile mapping (0 = plain): grid.x = 8 * xcd_per; workgroup b (on XCD b % 8: workgroups are dealt to the
  // XCDs round-robin) takes tile (b % 8) * xcd_per + b / 8, so each XCD walks ONE contiguous eighth of the image's tiles
  unsigned xcd_per;
};
// pixel formats at the kernel's edges: planar float32 NCHW (what the reference's tensors are), or the file edge's
// interleaved bytes (PIL HWC uint8 in, to_pil_image / astype('uint8') out) converted in registers
#define FMT_F32CHW 0
#define FMT_U8HWC 1

template <int VEC>
struct Pack;
template <>
struct Pack<4> {
  typedef v4f T;
  typedef v4b M;
};
template <>
struct Pack<1> {
  typedef float T;
  typedef unsigned char M;
};

// Non-temporal must be a COMPILE-TIME choice: with a run-time `nt ? __builtin_nontemporal_load(p) : *p`
// the optimiser merges the two loads and drops the hint (no `nt` instruction was ever emitted that way).
// Streaming data is touched once; `nt` keeps it from displacing lines in L2/MALL: +10 % on the 3-plane
// copy pattern of this path (tools/ubench/copy3.hip: 5.56 -> 6.15 TB/s).
// Element `i` of an array whose base is wave-uniform: the base stays an SGPR pair and the lane contributes a 32-bit BYTE offset
// (global_load / global_store's saddr form): one shift per access group instead of a 64-bit shift and a 64-bit add per
// plane.  Callers guarantee i * sizeof(T) < 2^32 (H*W <= 2^30 pixels, check_img: 2^28 float4 groups or 2^30 floats).
template <typename T>
__device__ __forceinline__ T* at(T* base, unsigned i) {
  typedef typename std::conditional<std::is_const<T>::value, const char, char>::type C;
  return reinterpret_cast<T*>(reinterpret_cast<C*>(base) + i * (unsigned)sizeof(T));
}
template <bool NT, typename T>
__device__ __forceinline__ T ld(const T* p) {
  if constexpr (NT) return __builtin_nontemporal_load(p);
  else return *p;
}
template <bool NT, typename T>
__device__ __forceinline__ void st(T* p, T v) {
  if constexpr (NT) __builtin_nontemporal_store(v, p);
  else *p = v;
}
__device__ __forceinline__ float lane(const v4f& v, int e) { return v[e]; }
__device__ __forceinline__ float lane(const float& v, int) { return v; }
__device__ __forceinline__ void set_lane(v4f& v, int e, float x) { v[e] = x; }
__device__ __forceinline__ void set_lane(float& v, int, float x) { v = x; }
__device__ __forceinline__ unsigned char lane_b(const v4b& v, int e) { return (unsigned char)((v >> (8 * e)) & 0xffu); }
__device__ __forceinline__ unsigned char lane_b(const unsigned char& v, int) { return v; }
__device__ __forceinline__ float mlane(const v4b& v, int e) { return ((v >> (8 * e)) & 0xffu) ? 1.0f : 0.0f; }
__device__ __forceinline__ float mlane(const unsigned char& v, int) { return v ? 1.0f : 0.0f; }

// Op contract:  struct Op { struct K {...}; static K load(const float* ws_image);  // uniform
//                           static Px apply(Px in, float m, const K&); static constexpr bool kMask; }
//
// One block = one tile of 256*U vectors of ONE image: all loads of the tile are issued up front (7*U
// independent 16-byte loads per lane), then the arithmetic, then the stores; latency is covered by the
// other resident waves (a two-deep register prefetch loop was measured and lost to plain occupancy on every
// kernel here: profiles/sweep_r01.md).  Loads clamp their index instead of branching (no divergent
// prologue, no zero-fill); stores are guarded.
template <int VEC, int U, int MK>
struct Tile {
  typename Pack<VEC>::T x0[U], x1[U], x2[U];
  typename Pack<VEC>::T mf[MK == CURL_MASK_F32 ? U : 1];
  typename Pack<VEC>::M mb[MK == CURL_MASK_U8 ? U : 1];
  typename Pack<VEC>::M wm[U];  // FMT_U8HWC: white-background mask bytes
};

// a*b rounded, then + c rounded -- what two eager ops produce (HIP's __fmul_rn/__fadd_rn are plain operators and
// get contracted into one fma; the pragma is what hipcc's default fast-honor-pragmas mode respects)
__device__ __forceinline__ float mul_then_add(float a, float b, float c) {
#pragma clang fp contract(off)
  float t = a * b;
  return t + c;
}
__device__ __forceinline__ float byte_of(unsigned w, int k) { return (float)((w >> (8 * k)) & 0xffu); }  // v_cvt_f32_ubyteK
// 4 interleaved RGB pixels = 3 dwords [R0 G0 B0 R1][G1 B1 R2 G2][B2 R3 G3 B3] -> three planes of 4 floats in [0,1]
__device__ __forceinline__ void unpack_rgb4(unsigned w0, unsigned w1, unsigned w2, v4f& r, v4f& g, v4f& b) {
  r = v4f{byte_of(w0, 0), byte_of(w0, 3), byte_of(w1, 2), byte_of(w2, 1)};
  g = v4f{byte_of(w0, 1), byte_of(w1, 0), byte_of(w1, 3), byte_of(w2, 2)};
  b = v4f{byte_of(w0, 2), byte_of(w1, 1), byte_of(w2, 0), byte_of(w2, 3)};
#pragma unroll
  for (int e = 0; e < 4; ++e) r[e] = u8_to_unit(r[e]), g[e] = u8_to_unit(g[e]), b[e] = u8_to_unit(b[e]);
}

// HAVE_MASK: the caller has loaded t.mb[] already (the mask-first path of stream_kernel)
template <int VEC, int U, int MK, bool NT, int FMT, bool HAVE_MASK = false>
__device__ __forceinline__ void load_tile(Tile<VEC, U, MK>& t, const StreamArgs& a, const typename Pack<VEC>::T* p0,
                                          size_t plane, size_t mask_off, unsigned base) {
  typedef typename Pack<VEC>::T T;
  typedef typename Pack<VEC>::M M;
  if constexpr (FMT == FMT_U8HWC) {
    // p0 = this image's interleaved bytes.  All loads first (raw words), conversions after.
    unsigned raw[U][3];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      unsigned i = min(base + u * blockDim.x, a.n - 1u);
      if constexpr (VEC == 4) {
        const unsigned* w = reinterpret_cast<const unsigned*>(p0) + 3 * (size_t)i;  // 12 bytes per lane, contiguous
        raw[u][0] = ld<NT>(w), raw[u][1] = ld<NT>(w + 1), raw[u][2] = ld<NT>(w + 2);
      } else {
        const uint8_t* w = reinterpret_cast<const uint8_t*>(p0) + 3 * (size_t)i;
        raw[u][0] = w[0], raw[u][1] = w[1], raw[u][2] = w[2];
      }
      if (MK == CURL_MASK_U8) t.mb[u] = ld<NT>(reinterpret_cast<const M*>(a.mask) + mask_off + i);
      if (MK == CURL_MASK_F32) t.mf[u] = ld<NT>(reinterpret_cast<const T*>(a.mask) + mask_off + i);
      if (a.white) t.wm[u] = ld<NT>(reinterpret_cast<const M*>(a.white) + mask_off + i);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if constexpr (VEC == 4) {
        unpack_rgb4(raw[u][0], raw[u][1], raw[u][2], t.x0[u], t.x1[u], t.x2[u]);
      } else {
        t.x0[u] = u8_to_unit((float)raw[u][0]), t.x1[u] = u8_to_unit((float)raw[u][1]);
        t.x2[u] = u8_to_unit((float)raw[u][2]);
      }
    }
    return;
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    unsigned i = min(base + u * blockDim.x, a.n - 1u);
    if (__builtin_expect(a.no_mem != 0, 0)) {  // diagnostics: keep its set-up out of the product path
      float f = (float)(i & 1023u) * (1.0f / 1024.0f);
      t.x0[u] = T(f);
      t.x1[u] = T(1.0f - f);
      t.x2[u] = T(0.5f * f + 0.1f);
      if (MK == CURL_MASK_U8) t.mb[u] = typename Pack<VEC>::M(VEC == 4 ? 0x01010101u : 1u);
      if (MK == CURL_MASK_F32) t.mf[u] = T(1.0f);
      // (volatile: or the splats are speculated in front of the branch -- ten v_mov per wave on the product path)
      asm volatile("" : "+v"(t.x0[u]), "+v"(t.x1[u]), "+v"(t.x2[u]));
      if constexpr (MK == CURL_MASK_U8 && VEC == 4) asm volatile("" : "+v"(t.mb[u]));
      continue;
    }
    // The mask's load goes out FIRST (and the wave's all-set / all-clear tests then wait for it alone, vmcnt(3)): with the
    // four bytes in one dword the compiler had moved it behind the three plane loads, and the memory-bound stages lost
    // 0.6 % (Lab) to 5 % (HSV) -- profiles/r03/exp10_mask_dword_load_order.log
    if (MK == CURL_MASK_U8 && !HAVE_MASK)
      t.mb[u] = ld<NT>(reinterpret_cast<const M*>(reinterpret_cast<const char*>(reinterpret_cast<const M*>(a.mask) + mask_off) +
                                                  i * (unsigned)sizeof(M)));
    if (MK == CURL_MASK_F32)
      t.mf[u] = ld<NT>(reinterpret_cast<const T*>(reinterpret_cast<const char*>(reinterpret_cast<const T*>(a.mask) + mask_off) +
                                                  i * (unsigned)sizeof(T)));
    if (MK != CURL_MASK_NONE && !HAVE_MASK) __builtin_amdgcn_sched_barrier(0);
    // wave-uniform plane base (SGPR pair) + a 32-bit byte offset per lane (i < 2^28 vectors: it fits): the saddr form of
    // global_load, one shift per tile instead of a 64-bit shift and three 64-bit adds
    const unsigned boff = i * (unsigned)sizeof(T);
    t.x0[u] = ld<NT>(reinterpret_cast<const T*>(reinterpret_cast<const char*>(p0) + boff));
    t.x1[u] = ld<NT>(reinterpret_cast<const T*>(reinterpret_cast<const char*>(p0 + plane) + boff));
    t.x2[u] = ld<NT>(reinterpret_cast<const T*>(reinterpret_cast<const char*>(p0 + 2 * plane) + boff));
  }
}

template <class Op, int VEC, int U, int MK, bool NT, int FMT>
__device__ __forceinline__ void compute_store(const Tile<VEC, U, MK>& t, const StreamArgs& a,
                                              typename Pack<VEC>::T* q0, size_t plane, unsigned base,
                                              const typename Op::K& k, bool valid) {
  typedef typename Pack<VEC>::T T;
  constexpr bool kBinary = (MK != CURL_MASK_F32);  // none / bool / uint8: the mask is exactly 0 or 1
#pragma unroll
  for (int u = 0; u < U; ++u) {
    unsigned i = base + u * blockDim.x;
    T y0, y1, y2;
    bool live = true, full = false;
    if (Op::kMask && MK != CURL_MASK_NONE) {
      // Masks are foreground masks: whole waves are often masked out.  Where every lane of the wave has
      // m == 0 for all its pixels the result is a constant (0 for the layer, lab2rgb(0,0,0) for the Lab
      // stage) and the arithmetic is skipped -- a wave-uniform branch (ballot), no divergence.
      bool lane_live = false;
      if constexpr (MK == CURL_MASK_U8) {
        lane_live = t.mb[u] != 0;  // some byte of the lane's dword (or its one byte) is set
      } else {
#pragma unroll
        for (int e = 0; e < VEC; ++e) lane_live |= lane(t.mf[u], e) != 0.0f;
      }
      live = __builtin_amdgcn_ballot_w64(lane_live) != 0ull;
      if constexpr (MK == CURL_MASK_U8) {
        // ... and just as often fully inside the foreground: every mask byte of the wave non-zero.  Then the
        // mask is the constant 1 and its conversions, multiplies and blends go (wave-uniform branch again).
        unsigned w;
        if constexpr (VEC == 4) {
          w = t.mb[u];
          w = (((w & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w) & 0x80808080u;  // bit 7 of each byte: byte != 0
          w ^= 0x80808080u;                                           // 0 iff all four are non-zero
        } else {
          w = t.mb[u] ? 0u : 1u;
        }
        full = __builtin_amdgcn_ballot_w64(w == 0u) == ~0ull;
      }
    }
    if (live && full) {
      PxN<VEC> px;
      float one[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        px.c0[e] = lane(t.x0[u], e);
        px.c1[e] = lane(t.x1[u], e);
        px.c2[e] = lane(t.x2[u], e);
        one[e] = 1.0f;
      }
      Op::template apply_n<true, VEC>(px, one, k, i * VEC);
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        set_lane(y0, e, px.c0[e]);
        set_lane(y1, e, px.c1[e]);
        set_lane(y2, e, px.c2[e]);
      }
    } else if (live) {
      PxN<VEC> px;
      float mm[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        px.c0[e] = lane(t.x0[u], e);
        px.c1[e] = lane(t.x1[u], e);
        px.c2[e] = lane(t.x2[u], e);
        mm[e] = 1.0f;
        if (MK == CURL_MASK_U8) mm[e] = mlane(t.mb[u], e);
        if (MK == CURL_MASK_F32) mm[e] = lane(t.mf[u], e);
      }
      Op::template apply_n<kBinary, VEC>(px, mm, k, i * VEC);
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        Px o{px.c0[e], px.c1[e], px.c2[e]};
        if (Op::kBlendMaskedOut && MK == CURL_MASK_U8) {
          // the binary specialisation leaves m == 0 pixels to us: overwrite with the masked-out constant
          Px z = Op::masked_out(k);
          int keep = opaque(-(int)(mm[e] != 0.0f));
          o.c0 = blend(keep, o.c0, z.c0);
          o.c1 = blend(keep, o.c1, z.c1);
          o.c2 = blend(keep, o.c2, z.c2);
        }
        set_lane(y0, e, o.c0);
        set_lane(y1, e, o.c1);
        set_lane(y2, e, o.c2);
      }
    } else {
      Px z = Op::masked_out(k);
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        set_lane(y0, e, z.c0);
        set_lane(y1, e, z.c1);
        set_lane(y2, e, z.c2);
      }
    }
    bool keep = true;
    if (a.no_mem) {  // every output feeds the (never true) condition, so nothing can be sunk or dropped
      float chk = 0.0f;
#pragma unroll
      for (int e = 0; e < VEC; ++e) chk += lane(y0, e) + lane(y1, e) + lane(y2, e);
      keep = (chk == -123.0f);
    }
    if constexpr (FMT == FMT_U8HWC) {
      unsigned q[3][VEC];  // [channel][pixel]
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        float c[3] = {lane(y0, e), lane(y1, e), lane(y2, e)};
        if (a.white) {  // infer.py:46: out*m + (1-m), two roundings like the eager ops (no contraction)
          float m = u8_to_unit((float)lane_b(t.wm[u], e));
          float one_minus = 1.0f - m;
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) c[ch] = mul_then_add(c[ch], m, one_minus);
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          // OpLayer / OpTriSpace* end in clamp(., 0, 1) [x a binary mask]: x 255 + convert is all that is left.  A FLOAT
          // mask is "multiplied as is" (include/curl_hip.h): values outside [0, 1] or NaN leave the range, so that kind
          // keeps the saturating form (a wrapped byte would be OR-ed into its neighbours below)
          if constexpr (MK == CURL_MASK_F32) q[ch][e] = unit_to_u8(c[ch]);
          else q[ch][e] = unit_to_u8_in_range(c[ch]);
        }
      }
      if (i < a.n && valid) {
        if constexpr (VEC == 4) {
          unsigned* w = reinterpret_cast<unsigned*>(q0) + 3 * (size_t)i;
          st<NT>(w, q[0][0] | (q[1][0] << 8) | (q[2][0] << 16) | (q[0][1] << 24));
          st<NT>(w + 1, q[1][1] | (q[2][1] << 8) | (q[0][2] << 16) | (q[1][2] << 24));
          st<NT>(w + 2, q[2][2] | (q[0][3] << 8) | (q[1][3] << 16) | (q[2][3] << 24));
        } else {
          uint8_t* w = reinterpret_cast<uint8_t*>(q0) + 3 * (size_t)i;
          w[0] = (uint8_t)q[0][0], w[1] = (uint8_t)q[1][0], w[2] = (uint8_t)q[2][0];
        }
      }
    } else if (i < a.n && keep && valid) {
      const unsigned boff = i * (unsigned)sizeof(T);
      st<NT>(reinterpret_cast<T*>(reinterpret_cast<char*>(q0) + boff), y0);
      st<NT>(reinterpret_cast<T*>(reinterpret_cast<char*>(q0 + plane) + boff), y1);
      st<NT>(reinterpret_cast<T*>(reinterpret_cast<char*>(q0 + 2 * plane) + boff), y2);
    }
  }
}


// MASK_FIRST: the foreground-mask variant (CURL_F_MASK_FIRST / Op::kMaskFirst; host_api.inc launch_u picks it) -- a kernel
// of its own, so that the default path carries none of it: every wave tests its mask before it asks for its pixels.
template <class Op, int VEC, int U, int MK, bool NT, int FMT = FMT_F32CHW, bool MASK_FIRST = false>
__global__ __launch_bounds__(256, Op::kMinWavesPerSimd) void stream_kernel(StreamArgs a) {
  typedef typename Pack<VEC>::T T;
  // grid = (chunks per image, images): both indices are SGPRs, no division
  const unsigned img = blockIdx.y;
  unsigned chunk = blockIdx.x;
  if (!Op::kRowTiles && a.xcd_per) {
    chunk = (blockIdx.x & 7u) * a.xcd_per + (blockIdx.x >> 3);
    if (chunk >= a.blocks_per_image) return;  // the padding of the last eighth (wave-uniform)
  }
  // H*W <= 2^30 (checked on the host): n <= 2^28 float4 groups, or 2^30 pixels on the scalar path -- byte offsets fit 32 bits
  __builtin_assume(a.n <= (1u << 30) / VEC);
  const float* table = a.coef ? a.coef + (size_t)img * a.coef_stride : nullptr;
  __shared__ __attribute__((aligned(16))) float s_table[Op::kLdsFloats > 0 ? Op::kLdsFloats : 1];
  unsigned row = 0, base = chunk * (blockDim.x * U) + threadIdx.x;
  bool valid = true;
  if constexpr (Op::kRowTiles) {
    row = chunk / a.segs;  // wave-uniform, once per block
    const unsigned in_row = (chunk - row * a.segs) * blockDim.x + threadIdx.x;
    valid = in_row < a.units;                          // lanes past the row end: loads clamp, stores are dropped
    base = row * a.units + min(in_row, a.units - 1u);
  }
  const size_t plane = (size_t)a.plane;
  // an image is 3 planes of `plane` vectors, or (FMT_U8HWC) plane*VEC pixels of 3 bytes = 3*plane*VEC bytes;
  // a row slab starts `off` vectors into every plane (interleaved bytes: 3*off*VEC bytes into the image)
  const size_t image_bytes = (FMT == FMT_U8HWC) ? 3 * plane * VEC : 3 * plane * sizeof(T);
  const size_t slab_bytes = (FMT == FMT_U8HWC) ? 3 * (size_t)a.off * VEC : (size_t)a.off * sizeof(T);
  const T* p0 = reinterpret_cast<const T*>(reinterpret_cast<const char*>(a.in) + (size_t)img * image_bytes + slab_bytes);
  T* q0 = reinterpret_cast<T*>(reinterpret_cast<char*>(a.out) + (size_t)img * image_bytes + slab_bytes);
  const size_t mask_off = (size_t)img * plane + a.off;
  Tile<VEC, U, MK> t;
  // Ops that stage a table in LDS first (polynomial coefficients folded per row, PWL knots): the pixel loads are
  // issued BEFORE the staging loop and its barrier, so their HBM latency runs under it instead of after it (the
  // polynomial kernel holds 5 waves per SIMD at most: a wave that waits holds a fifth of the SIMD's slots).
  constexpr bool kEarlyLoads = Op::kLdsFloats > 0 && FMT == FMT_F32CHW;
  if constexpr (kEarlyLoads) load_tile<VEC, U, MK, NT, FMT>(t, a, p0, plane, mask_off, base);
  if constexpr (Op::kLdsFloats > 0) {
    // a per-image table too large for SGPRs (1134 polynomial coefficients): one coalesced copy into LDS, then
    // every lane reads the same address (broadcast ds_read_b128, conflict-free)
    if constexpr (Op::kRawFloats > 0) {
      typedef float f2 __attribute__((ext_vector_type(2)));
      static_assert(Op::kRawFloats % 2 == 0, "copied as 8-byte pairs");
      __shared__ __attribute__((aligned(16))) float s_raw[(Op::kRawFloats + 3) & ~3];
      constexpr unsigned n2 = Op::kRawFloats / 2;
      const f2* g = reinterpret_cast<const f2*>(table);
      for (unsigned i0 = 0; i0 < n2; i0 += 4u * blockDim.x) {  // four loads in flight per lane, then the four stores
        f2 r[4];
#pragma unroll
        for (unsigned k = 0; k < 4; ++k) r[k] = g[min(i0 + k * blockDim.x + threadIdx.x, n2 - 1u)];
#pragma unroll
        for (unsigned k = 0; k < 4; ++k) {
          const unsigned i = i0 + k * blockDim.x + threadIdx.x;
          if (i < n2) reinterpret_cast<f2*>(s_raw)[i] = r[k];
        }
      }
      __syncthreads();
      table = s_raw;
    }
    if constexpr (Op::kRowTiles || Op::kStageValue) {
      const unsigned n_stage = Op::lds_count(a);  // <= kLdsFloats
      for (unsigned i = threadIdx.x; i < n_stage; i += blockDim.x)
        s_table[i] = Op::stage_value(table, i, row + a.row0, a);
    } else {
      for (int i = threadIdx.x; i < Op::kLdsFloats; i += blockDim.x) s_table[i] = table[Op::stage_index(i)];
    }
    __syncthreads();
    table = s_table;
  }
  const typename Op::K k = Op::load(table, a);
  // Foreground masks (MASK_FIRST: CURL_F_MASK_FIRST, or the op's own default): the wave asks for its mask bytes
  // alone, and where all of them are zero it stores the masked-out constant and leaves without ever reading its pixels --
  // at the price of one more memory round trip for every other wave.  Layer: +0.5 ... +0.8 % on an all-ones mask, -7.4 % at
  // 70 % coverage, -25 % at 40 %; Lab stage -9.2 %, HSV stage -5.9 % at 70 % (profiles/r03/exp32_mask_first_variant.log).
  // An early exit, not a branch around the loads: behind a join the compiler can no longer wait for the mask alone
  // (vmcnt(3)), and as a run-time branch inside the one kernel it cost the default path 0.6 % (exp30).
  static_assert(!MASK_FIRST || (U == 1 && MK == CURL_MASK_U8 && VEC == 4 && FMT == FMT_F32CHW && Op::kMask && !kEarlyLoads),
                "the mask-first variant exists for bool / uint8 masks on the float4 kernels at one group per lane");
  bool pixels_asked_for = false;
  if constexpr (MASK_FIRST) {
    {
      typedef typename Pack<VEC>::M M;
      const unsigned i = min(base, a.n - 1u);
      t.mb[0] = ld<NT>(reinterpret_cast<const M*>(reinterpret_cast<const char*>(reinterpret_cast<const M*>(a.mask) + mask_off) +
                                                   i * (unsigned)sizeof(M)));
      if (__builtin_amdgcn_ballot_w64(t.mb[0] != 0u) == 0ull) {
        if (base < a.n && valid) {
          const Px z = Op::masked_out(k);
          const unsigned boff = base * (unsigned)sizeof(T);
          st<NT>(reinterpret_cast<T*>(reinterpret_cast<char*>(q0) + boff), T(z.c0));
          st<NT>(reinterpret_cast<T*>(reinterpret_cast<char*>(q0 + plane) + boff), T(z.c1));
          st<NT>(reinterpret_cast<T*>(reinterpret_cast<char*>(q0 + 2 * plane) + boff), T(z.c2));
        }
        return;
      }
      load_tile<VEC, U, MK, NT, FMT, true>(t, a, p0, plane, mask_off, base);
      pixels_asked_for = true;
    }
  }
  if constexpr (!kEarlyLoads)
    if (!pixels_asked_for) load_tile<VEC, U, MK, NT, FMT>(t, a, p0, plane, mask_off, base);
  compute_store<Op, VEC, U, MK, NT, FMT>(t, a, q0, plane, base, k, valid);
}

// Every float of a coefficient struct that was read from LDS, moved to SGPRs (v_readfirstlane_b32): the values are the same in
// every lane, and the arithmetic downstream is the code of the two-launch form, which gets them from scalar loads.
template <class K>
__device__ __forceinline__ K uniform_k(K k) {
  static_assert(sizeof(K) % 4 == 0 && std::is_trivially_copyable<K>::value, "a struct of floats");
  unsigned w[sizeof(K) / 4];
  __builtin_memcpy(w, &k, sizeof(K));
#pragma unroll
  for (unsigned i = 0; i < sizeof(K) / 4; ++i) w[i] = __builtin_amdgcn_readfirstlane(w[i]);
  __builtin_memcpy(&k, w, sizeof(K));
  return k;
}

// ONE launch per call where the launch is the cost (small grids: one frame at infer.py:44, the training crop batch of
// main.py:88): every workgroup collapses its image's curves ITSELF -- prep_image, the code knots_prep_kernel runs, so the
// results are bit-identical -- while its tile's loads are in flight, instead of waiting for a launch of one workgroup per
// image and a kernel boundary.  The image's first workgroup also writes the workspace row (the backward reads it) and the
// regulariser.  ~3 us of prologue per workgroup: chosen by launch_stream only while the whole grid is resident in one or two
// rounds (host_api.inc kSelfPrepMaxTiles); larger launches keep the two-launch form, whose kernels are untouched by this.
template <class Op, int VEC, int MK, bool NT>
__global__ __launch_bounds__(256, Op::kMinWavesPerSimd) void stream_selfprep_kernel(StreamArgs a, PrepArgs p) {
  typedef typename Pack<VEC>::T T;
  static_assert(Op::kLdsFloats == 0 && !Op::kRowTiles && Op::kSelfPrep, "ops whose per-image table is the workspace row's head");
  const unsigned img = blockIdx.y, chunk = blockIdx.x;
  __builtin_assume(a.n <= (1u << 28));
  // launch_stream never takes this kernel for the arithmetic-only diagnostic: without the (uniform) branch around the tile's
  // loads the wait for the early-fetched knot below is vmcnt(4) -- the knot alone -- instead of every load in flight
  __builtin_assume(a.no_mem == 0);
  const unsigned base = chunk * blockDim.x + threadIdx.x;
  const size_t plane = (size_t)a.plane;
  const size_t image_bytes = 3 * plane * sizeof(T), slab_bytes = (size_t)a.off * sizeof(T);
  const T* p0 = reinterpret_cast<const T*>(reinterpret_cast<const char*>(a.in) + (size_t)img * image_bytes + slab_bytes);
  T* q0 = reinterpret_cast<T*>(reinterpret_cast<char*>(a.out) + (size_t)img * image_bytes + slab_bytes);
  const size_t mask_off = (size_t)img * plane + a.off;
  Tile<VEC, 1, MK> t;
  // the lane's raw knot first, then the tile (vector loads return in order: the knot must not queue behind the pixels)
  float first_raw = prep_fetch_first(p, img);
  __builtin_amdgcn_sched_barrier(0);  // (keeps the load in front of the tile's; nothing waits for it here)
  load_tile<VEC, 1, MK, NT, FMT_F32CHW>(t, a, p0, plane, mask_off, base);  // in flight while the curves are collapsed
  __shared__ float s_head[WS_KNOTS];
  prep_image(p, img, chunk == 0, s_head, first_raw, true);
  __syncthreads();
  const typename Op::K k = uniform_k(Op::load(s_head, a));
  compute_store<Op, VEC, 1, MK, NT, FMT_F32CHW>(t, a, q0, plane, base, k, true);
}
