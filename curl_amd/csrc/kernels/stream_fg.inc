// stream_fg.inc -- part of curl_kernels.hip (one translation unit; included after stream.inc and ops.inc, not compiled alone).
// ------------------------------------------------------------------------------------------------
// the foreground-aware byte edge (include/curl_hip_fg.h)
// ------------------------------------------------------------------------------------------------
// infer.py:46 whites out every pixel whose mask byte is 0: u8_to_unit(0) = 0, mul_then_add(c, 0, 1) = 1 for every finite c,
// unit_to_u8_in_range(1) = 255.  The byte kernels of stream.inc are bound by VALU issue (DESIGN.md 0), so a wave whose mask
// bytes are all zero has nothing to compute: it stores white and never asks for its pixels.  A kernel of its own (a
// template parameter on stream_kernel would rename the kernels tests/test_build_resources.py pins); a live wave runs
// compute_store, the code of the existing byte kernels, on the tile it loaded -- that is what makes the bytes equal.
//
// Order of a workgroup:
//   1. every lane asks for its mask bytes (one dword = 4 pixels, or one byte), the wave votes (ballot): live or dead;
//   2. ops with an LDS table: the workgroup votes (one LDS word per wave, one barrier).  No wave live: every thread stores
//      white and returns -- no raw-table copy, no row fold;
//   3. live waves ask for their pixels (in flight under the staging);
//   4. the staging of stream_kernel, barriers included, by EVERY wave of the workgroup, dead ones too: no wave returns or
//      branches around a barrier the others wait at;
//   5. dead waves store white and leave; live waves convert, compute and store.
// channels: 3, or 4 (RGBA: the fourth byte of a pixel is loaded with the others and dropped).
template <int VEC>
__device__ __forceinline__ void store_white(uint8_t* q0, unsigned i) {
  if constexpr (VEC == 4) {
    unsigned* w = reinterpret_cast<unsigned*>(q0) + 3 * (size_t)i;
    st<true>(w, ~0u), st<true>(w + 1, ~0u), st<true>(w + 2, ~0u);
  } else {
    uint8_t* w = q0 + 3 * (size_t)i;
    w[0] = 255, w[1] = 255, w[2] = 255;
  }
}

template <class Op, int VEC, bool NT>
__global__ __launch_bounds__(256, Op::kMinWavesPerSimd) void stream_fg_kernel(StreamArgs a, unsigned channels) {
  typedef typename Pack<VEC>::T T;
  typedef typename Pack<VEC>::M M;
  static_assert(Op::kUnroll == 1 || Op::kSingleTileShape, "one group per lane");
  static_assert(!NT || VEC == 4, "the byte path takes plain accesses");
  const unsigned img = blockIdx.y, chunk = blockIdx.x;
  __builtin_assume(a.n <= (1u << 30) / VEC);  // (groups of VEC pixels: the byte class counts pixels, up to 2^30)
  const float* table = a.coef ? a.coef + (size_t)img * a.coef_stride : nullptr;
  unsigned row = 0, base = chunk * blockDim.x + threadIdx.x;
  bool valid = true;
  if constexpr (Op::kRowTiles) {
    row = chunk / a.segs;
    const unsigned in_row = (chunk - row * a.segs) * blockDim.x + threadIdx.x;
    valid = in_row < a.units;  // lanes past the row end: loads clamp (to the row's last group), stores are dropped
    base = row * a.units + min(in_row, a.units - 1u);
  }
  const size_t plane = (size_t)a.plane;  // groups per image
  const uint8_t* p0 = reinterpret_cast<const uint8_t*>(a.in) + (size_t)img * channels * plane * VEC;
  uint8_t* q0 = reinterpret_cast<uint8_t*>(a.out) + (size_t)img * 3 * plane * VEC;
  const unsigned i = min(base, a.n - 1u);
  const bool stores = base < a.n && valid;

  // 1. the mask alone
  Tile<VEC, 1, CURL_MASK_NONE> t;
  t.wm[0] = ld<NT>(reinterpret_cast<const M*>(a.white) + (size_t)img * plane + i);
  const bool wave_live = __builtin_amdgcn_ballot_w64(t.wm[0] != 0) != 0ull;

  // 2. the workgroup's vote
  if constexpr (Op::kLdsFloats > 0) {
    __shared__ unsigned s_vote[4];
    if ((threadIdx.x & 63u) == 0u) s_vote[threadIdx.x >> 6] = wave_live;
    __syncthreads();
    unsigned any = 0;
    for (unsigned w = 0; w < (blockDim.x >> 6); ++w) any |= s_vote[w];
    if (__builtin_amdgcn_readfirstlane(any) == 0u) {  // the same for every thread of the workgroup
      if (stores) store_white<VEC>(q0, base);
      return;
    }
  }

  // 3. the pixels of a live wave, raw
  unsigned raw[4] = {0u, 0u, 0u, 0u};
  if (wave_live) {
    if constexpr (VEC == 4) {
      if (channels == 4) {  // [R G B A] per dword
        const unsigned* w = reinterpret_cast<const unsigned*>(p0) + 4 * (size_t)i;
        raw[0] = ld<NT>(w), raw[1] = ld<NT>(w + 1), raw[2] = ld<NT>(w + 2), raw[3] = ld<NT>(w + 3);
      } else {              // [R0 G0 B0 R1][G1 B1 R2 G2][B2 R3 G3 B3]
        const unsigned* w = reinterpret_cast<const unsigned*>(p0) + 3 * (size_t)i;
        raw[0] = ld<NT>(w), raw[1] = ld<NT>(w + 1), raw[2] = ld<NT>(w + 2);
      }
    } else {
      const uint8_t* w = p0 + (size_t)channels * i;
      raw[0] = w[0], raw[1] = w[1], raw[2] = w[2];
    }
  }

  // 4. stream_kernel's staging, every wave of the workgroup
  __shared__ __attribute__((aligned(16))) float s_table[Op::kLdsFloats > 0 ? Op::kLdsFloats : 1];
  if constexpr (Op::kLdsFloats > 0) {
    if constexpr (Op::kRawFloats > 0) {
      typedef float f2 __attribute__((ext_vector_type(2)));
      static_assert(Op::kRawFloats % 2 == 0, "copied as 8-byte pairs");
      __shared__ __attribute__((aligned(16))) float s_raw[(Op::kRawFloats + 3) & ~3];
      constexpr unsigned n2 = Op::kRawFloats / 2;
      const f2* g = reinterpret_cast<const f2*>(table);
      for (unsigned i0 = 0; i0 < n2; i0 += 4u * blockDim.x) {
        f2 r[4];
#pragma unroll
        for (unsigned k = 0; k < 4; ++k) r[k] = g[min(i0 + k * blockDim.x + threadIdx.x, n2 - 1u)];
#pragma unroll
        for (unsigned k = 0; k < 4; ++k) {
          const unsigned j = i0 + k * blockDim.x + threadIdx.x;
          if (j < n2) reinterpret_cast<f2*>(s_raw)[j] = r[k];
        }
      }
      __syncthreads();
      table = s_raw;
    }
    if constexpr (Op::kRowTiles || Op::kStageValue) {
      const unsigned n_stage = Op::lds_count(a);
      for (unsigned j = threadIdx.x; j < n_stage; j += blockDim.x) s_table[j] = Op::stage_value(table, j, row + a.row0, a);
    } else {
      for (int j = threadIdx.x; j < Op::kLdsFloats; j += blockDim.x) s_table[j] = table[Op::stage_index(j)];
    }
    __syncthreads();
    table = s_table;
  }

  // 5. behind the last barrier
  if (!wave_live) {
    if (stores) store_white<VEC>(q0, base);
    return;
  }
  const typename Op::K k = Op::load(table, a);
  if constexpr (VEC == 4) {
    if (channels == 4) {
      t.x0[0] = v4f{byte_of(raw[0], 0), byte_of(raw[1], 0), byte_of(raw[2], 0), byte_of(raw[3], 0)};
      t.x1[0] = v4f{byte_of(raw[0], 1), byte_of(raw[1], 1), byte_of(raw[2], 1), byte_of(raw[3], 1)};
      t.x2[0] = v4f{byte_of(raw[0], 2), byte_of(raw[1], 2), byte_of(raw[2], 2), byte_of(raw[3], 2)};
#pragma unroll
      for (int e = 0; e < 4; ++e) t.x0[0][e] = u8_to_unit(t.x0[0][e]), t.x1[0][e] = u8_to_unit(t.x1[0][e]), t.x2[0][e] = u8_to_unit(t.x2[0][e]);
    } else {
      unpack_rgb4(raw[0], raw[1], raw[2], t.x0[0], t.x1[0], t.x2[0]);
    }
  } else {
    t.x0[0] = u8_to_unit((float)raw[0]), t.x1[0] = u8_to_unit((float)raw[1]), t.x2[0] = u8_to_unit((float)raw[2]);
  }
  compute_store<Op, VEC, 1, CURL_MASK_NONE, NT, FMT_U8HWC>(t, a, reinterpret_cast<T*>(q0), plane, base, k, valid);
}
