// stream_ragged.inc -- part of curl_kernels.hip (one translation unit; included after stream.inc and ops.inc, not compiled alone).
// ------------------------------------------------------------------------------------------------
// the byte edge for a batch of images of different sizes (include/curl_hip_ragged.h)
// ------------------------------------------------------------------------------------------------
// A 512 x 341 photograph is 171 tiles of 1 024 pixels: fewer workgroups than the part has CUs, a launch bound by its own
// latency.  Here the grid of ONE launch is the sum of many images' tiles.  A workgroup finds its image in the plan's
// descriptor table (a binary search of the running sums of workgroups: blockIdx.x and the table are wave-uniform, the loads
// are scalar), fills a StreamArgs of its own from the descriptor and runs the staging of stream_kernel and compute_store, the
// code of the existing byte kernels, on the tile it loaded -- that is what makes the bytes equal.  A kernel of its own (a
// template parameter on stream_kernel would rename the kernels tests/test_build_resources.py pins); StreamArgs is unchanged.
//
// The plan's layout is the header's (the names there; csrc holds the numbers).
constexpr unsigned kRaggedStamp = 0x52474731u;
constexpr unsigned kRaggedHeaderWords = 32, kRaggedDescWords = 16;
enum {  // header words
  RH_STAMP = 0, RH_B, RH_OP, RH_HAS_MASK, RH_LAUNCHES, RH_N_DWORD, RH_N_BYTE, RH_THREADS_DWORD, RH_GRID_DWORD, RH_THREADS_BYTE,
  RH_GRID_BYTE, RH_IMG_BYTES = 12, RH_MASK_BYTES = 14, RH_OUT_BYTES = 16, RH_HASH = 18
};
enum {  // descriptor words
  RD_FIRST = 0, RD_INDEX, RD_H, RD_W, RD_CHANNELS, RD_N, RD_UNITS, RD_SEGS, RD_TILES, RD_IMG_OFF = 10, RD_MASK_OFF = 12, RD_OUT_OFF = 14
};

// (the kernel takes the fields one by one, as encoder_view_kernel does: scalars and pointers only beside StreamArgs)
struct RaggedArgs {
  const int* plan;       // the device copy of the plan
  const uint8_t* img;    // the three arenas (mask: NULL = no compositing)
  const uint8_t* mask;
  uint8_t* out;
  unsigned long long img_bytes, mask_bytes, out_bytes;
  unsigned long long hash;  // the HOST plan's
  unsigned stamp;
  unsigned table;  // first word of this launch's descriptor table
  unsigned count;  // its descriptors (>= 1)
};

// a wave-uniform word of the plan, in an SGPR whatever kind of load fetched it
__device__ __forceinline__ unsigned ragged_word(const int* p, unsigned i) { return __builtin_amdgcn_readfirstlane((unsigned)p[i]); }
__device__ __forceinline__ unsigned long long ragged_word64(const int* p, unsigned i) {
  return (unsigned long long)ragged_word(p, i) | ((unsigned long long)ragged_word(p, i + 1) << 32);
}

template <class Op, int VEC, bool NT>
__global__ __launch_bounds__(256, Op::kMinWavesPerSimd) void stream_ragged_kernel(
    StreamArgs a0, const int* plan, const uint8_t* img_arena, const uint8_t* mask_arena, uint8_t* out_arena, unsigned long long img_bytes,
    unsigned long long mask_bytes, unsigned long long out_bytes, unsigned long long hash, unsigned stamp, unsigned table_word, unsigned count) {
  const RaggedArgs r{plan, img_arena, mask_arena, out_arena, img_bytes, mask_bytes, out_bytes, hash, stamp, table_word, count};
  typedef typename Pack<VEC>::T T;
  typedef typename Pack<VEC>::M M;
  static_assert(Op::kUnroll == 1 || Op::kSingleTileShape, "one group per lane");
  static_assert(!NT || VEC == 4, "the byte path takes plain accesses");
  // 1. whose plan is this?  A stale or foreign one: no output at all
  if (ragged_word(r.plan, RH_STAMP) != r.stamp || ragged_word64(r.plan, RH_HASH) != r.hash) return;

  // 2. the workgroup's image: the last descriptor whose first workgroup is <= blockIdx.x (scalar throughout)
  const int* tab = r.plan + r.table;
  const unsigned wg = blockIdx.x;
  unsigned lo = 0, hi = r.count;
  while (hi - lo > 1u) {
    const unsigned mid = (lo + hi) >> 1;
    if (ragged_word(tab, mid * kRaggedDescWords + RD_FIRST) <= wg) lo = mid;
    else hi = mid;
  }
  const int* d = tab + lo * kRaggedDescWords;
  const unsigned chunk = wg - ragged_word(d, RD_FIRST);
  const unsigned img = ragged_word(d, RD_INDEX), channels = ragged_word(d, RD_CHANNELS), n = ragged_word(d, RD_N);
  const unsigned long long img_off = ragged_word64(d, RD_IMG_OFF), mask_off = ragged_word64(d, RD_MASK_OFF),
                           out_off = ragged_word64(d, RD_OUT_OFF);

  // 3. the descriptor's extents against the arenas, before any address is formed (every access below is to group
  //    min(., n - 1) of the image: inside [off, off + bytes) of its arena)
  const unsigned long long px = (unsigned long long)n * VEC;
  if (n == 0u || px > (1ull << 30) || (channels != 3u && channels != 4u) || chunk >= ragged_word(d, RD_TILES)) return;
  if (img >= ragged_word(r.plan, RH_B)) return;  // (the image's row of the coefficient table / workspace)
  if (img_off > r.img_bytes || px * channels > r.img_bytes - img_off) return;
  if (out_off > r.out_bytes || px * 3u > r.out_bytes - out_off) return;
  if (r.mask && (mask_off > r.mask_bytes || px > r.mask_bytes - mask_off)) return;
  if ((img_off | mask_off | out_off) % (VEC == 4 ? 4u : 1u)) return;

  StreamArgs a = a0;
  a.n = n, a.plane = n, a.off = 0, a.row0 = 0;
  a.W = ragged_word(d, RD_W), a.H = ragged_word(d, RD_H);
  a.units = ragged_word(d, RD_UNITS), a.segs = ragged_word(d, RD_SEGS);
  a.white = r.mask ? r.mask + mask_off : nullptr;
  const float* table = a.coef ? a.coef + (size_t)img * a.coef_stride : nullptr;
  unsigned row = 0, base = chunk * blockDim.x + threadIdx.x;
  bool valid = true;
  if constexpr (Op::kRowTiles) {
    if (a.segs == 0u || a.units == 0u) return;
    row = chunk / a.segs;
    const unsigned in_row = (chunk - row * a.segs) * blockDim.x + threadIdx.x;
    valid = in_row < a.units;  // lanes past the row end: loads clamp (to the row's last group), stores are dropped
    base = row * a.units + min(in_row, a.units - 1u);
  }
  const size_t plane = (size_t)n;
  const uint8_t* p0 = r.img + img_off;
  uint8_t* q0 = r.out + out_off;
  const unsigned i = min(base, n - 1u);

  // 4. the tile, raw: the mask first, then 3 dwords (RGBA: 4) per four pixels, or the bytes of one pixel
  Tile<VEC, 1, CURL_MASK_NONE> t;
  if (a.white) t.wm[0] = ld<NT>(reinterpret_cast<const M*>(a.white) + i);
  unsigned raw[4] = {0u, 0u, 0u, 0u};
  if constexpr (VEC == 4) {
    if (channels == 4u) {  // [R G B A] per dword
      const unsigned* w = reinterpret_cast<const unsigned*>(p0) + 4 * (size_t)i;
      raw[0] = ld<NT>(w), raw[1] = ld<NT>(w + 1), raw[2] = ld<NT>(w + 2), raw[3] = ld<NT>(w + 3);
    } else {               // [R0 G0 B0 R1][G1 B1 R2 G2][B2 R3 G3 B3]
      const unsigned* w = reinterpret_cast<const unsigned*>(p0) + 3 * (size_t)i;
      raw[0] = ld<NT>(w), raw[1] = ld<NT>(w + 1), raw[2] = ld<NT>(w + 2);
    }
  } else {
    const uint8_t* w = p0 + (size_t)channels * i;
    raw[0] = w[0], raw[1] = w[1], raw[2] = w[2];
  }

  // 5. stream_kernel's staging (every thread of the workgroup is still here: the returns above are workgroup-uniform)
  __shared__ __attribute__((aligned(16))) float s_table[Op::kLdsFloats > 0 ? Op::kLdsFloats : 1];
  if constexpr (Op::kLdsFloats > 0) {
    if constexpr (Op::kRawFloats > 0) {
      typedef float f2 __attribute__((ext_vector_type(2)));
      static_assert(Op::kRawFloats % 2 == 0, "copied as 8-byte pairs");
      __shared__ __attribute__((aligned(16))) float s_raw[(Op::kRawFloats + 3) & ~3];
      constexpr unsigned n2 = Op::kRawFloats / 2;
      const f2* g = reinterpret_cast<const f2*>(table);
      for (unsigned i0 = 0; i0 < n2; i0 += 4u * blockDim.x) {
        f2 v[4];
#pragma unroll
        for (unsigned k = 0; k < 4; ++k) v[k] = g[min(i0 + k * blockDim.x + threadIdx.x, n2 - 1u)];
#pragma unroll
        for (unsigned k = 0; k < 4; ++k) {
          const unsigned j = i0 + k * blockDim.x + threadIdx.x;
          if (j < n2) reinterpret_cast<f2*>(s_raw)[j] = v[k];
        }
      }
      __syncthreads();
      table = s_raw;
    }
    if constexpr (Op::kRowTiles || Op::kStageValue) {
      const unsigned n_stage = Op::lds_count(a);
      for (unsigned j = threadIdx.x; j < n_stage; j += blockDim.x) s_table[j] = Op::stage_value(table, j, row, a);
    } else {
      for (int j = threadIdx.x; j < Op::kLdsFloats; j += blockDim.x) s_table[j] = table[Op::stage_index(j)];
    }
    __syncthreads();
    table = s_table;
  }

  // 6. behind the last barrier: a wave with no lane that stores (past its row's end, past its image's last group) has helped
  //    to stage and leaves -- idle lanes cost arithmetic only inside a row's or an image's LAST wave, whatever the block size
  if (__builtin_amdgcn_ballot_w64(base < n && valid) == 0ull) return;

  // 7. convert, compute, store
  const typename Op::K k = Op::load(table, a);
  if constexpr (VEC == 4) {
    if (channels == 4u) {
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
