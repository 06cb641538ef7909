// stream_ragged_fg.inc -- part of curl_kernels.hip (one translation unit; included after stream_fg.inc and stream_ragged.inc,
// whose store_white, plan layout, RaggedArgs and ragged_word it uses; not compiled alone).
// ------------------------------------------------------------------------------------------------
// the foreground-aware byte edge for a batch of images of different sizes (include/curl_hip_ragged_fg.h)
// ------------------------------------------------------------------------------------------------
// stream_ragged_kernel's workgroup -> (image, tile) lookup in front of stream_fg_kernel's order: a wavefront whose mask bytes
// are all 0 stores white and never asks for its pixels, a workgroup of such wavefronts stages no coefficient table and folds
// no row.  A kernel of its own (a template parameter on either would rename the kernels tests/test_build_resources.py pins);
// StreamArgs, the plan and RaggedArgs are unchanged, and a live wave runs compute_store, the code of the existing byte
// kernels, on the tile it loaded -- that is what makes the bytes equal.
//
// Order of a workgroup:
//   1. the plan's stamp and hash against the arguments; 2. the descriptor (scalar binary search) and its extents against the
//      arenas, the mask arena's unconditionally -- every return up to here is workgroup-uniform;
//   3. every lane asks for its mask bytes (one dword = 4 pixels, or one byte) at its clamped index; the wave votes, and only
//      lanes that STORE vote: the last wave of every short row and of every small image is mostly clamped lanes, which repeat
//      the mask of the row's or the image's last group -- one live pixel there would keep a wave with nothing to store alive;
//   4. ops with an LDS table: the workgroup votes (one LDS word per wave, one barrier).  No wave live: every storing lane
//      stores white and the workgroup returns -- no raw-table copy, no row fold;
//   5. live waves ask for their pixels (in flight under the staging);
//   6. the staging of stream_kernel, barriers included, by EVERY wave still in the workgroup, dead ones too: no wave returns or
//      branches around a barrier the others wait at;
//   7. behind the last barrier a dead wave stores white for its storing lanes (a wave without any has none to store for) and
//      leaves; a live wave converts, computes and stores.
// Ops without an LDS table (the curve layer) have no barrier: a dead wave stores white right after 3.
template <class Op, int VEC, bool NT>
__global__ __launch_bounds__(256, Op::kMinWavesPerSimd) void stream_ragged_fg_kernel(
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

  //    the descriptor's extents against the arenas, before any address is formed (every access below is to group
  //    min(., n - 1) of the image: inside [off, off + bytes) of its arena); the mask is required here
  const unsigned long long px = (unsigned long long)n * VEC;
  if (n == 0u || px > (1ull << 30) || (channels != 3u && channels != 4u) || chunk >= ragged_word(d, RD_TILES)) return;
  if (img >= ragged_word(r.plan, RH_B)) return;  // (the image's row of the coefficient table / workspace)
  if (img_off > r.img_bytes || px * channels > r.img_bytes - img_off) return;
  if (out_off > r.out_bytes || px * 3u > r.out_bytes - out_off) return;
  if (!r.mask || mask_off > r.mask_bytes || px > r.mask_bytes - mask_off) return;
  if ((img_off | mask_off | out_off) % (VEC == 4 ? 4u : 1u)) return;

  StreamArgs a = a0;
  a.n = n, a.plane = n, a.off = 0, a.row0 = 0;
  a.W = ragged_word(d, RD_W), a.H = ragged_word(d, RD_H);
  a.units = ragged_word(d, RD_UNITS), a.segs = ragged_word(d, RD_SEGS);
  a.white = r.mask + mask_off;
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
  const bool stores = base < n && valid;

  // 3. the mask alone; the lanes that store vote
  Tile<VEC, 1, CURL_MASK_NONE> t;
  t.wm[0] = ld<NT>(reinterpret_cast<const M*>(a.white) + i);
  const bool wave_live = __builtin_amdgcn_ballot_w64(stores && t.wm[0] != 0) != 0ull;

  // 4. the workgroup's vote (blockDim.x is the plan's: one to four waves)
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
  } else {
    if (!wave_live) {  // no barrier ahead: nothing to wait for
      if (stores) store_white<VEC>(q0, base);
      return;
    }
  }

  // 5. the pixels of a live wave, raw: 3 dwords (RGBA: 4) per four pixels, or the bytes of one pixel
  unsigned raw[4] = {0u, 0u, 0u, 0u};
  if (wave_live) {
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
  }

  // 6. stream_kernel's staging, every wave still in the workgroup
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

  // 7. behind the last barrier: a dead wave has helped to stage; its storing lanes (if any) store white, and it leaves
  if (!wave_live) {
    if (stores) store_white<VEC>(q0, base);
    return;
  }
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
