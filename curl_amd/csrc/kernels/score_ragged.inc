// score_ragged.inc -- part of curl_kernels.hip (one translation unit; included after stream_ragged.inc, whose plan layout and
// ragged_word it uses; not compiled alone).
// ------------------------------------------------------------------------------------------------
// the exact score of a batch of byte images of different sizes (include/curl_hip_ragged_score.h)
// ------------------------------------------------------------------------------------------------
// Per image the masked sum of squared byte differences and the number of pixels the mask keeps, as integers.  Two passes over
// the plan of operator 0 (flat tiles: 256 lanes, one group per lane):
//   pass 1  one launch per class with the plan's grid.  A workgroup finds its image as stream_ragged_kernel does (stamp and
//           hash, the scalar binary search, the descriptor's extents against all three arenas, all before an address is
//           formed) and writes ITS pair (sse, count) -- zeros when the descriptor fails a check, so pass 2 never sums a word
//           nobody wrote; a stale or foreign plan writes nothing at all.
//   pass 2  one launch of B workgroups: each sums its descriptor's pairs in uint64 and writes sums[2 * index], [2 * index + 1].
// No atomics, no memset; integer sums do not depend on their order.
//
// The partials are uint32: a channel's squared difference is <= 255^2 = 65 025, a pixel's <= 195 075, a lane's (four pixels)
// <= 780 300 and a workgroup's (256 lanes) <= 1 024 * 195 075 = 199 756 800.
typedef unsigned ScorePartial;
static_assert(1024ull * 3ull * 255ull * 255ull <= 0xffffffffull, "a workgroup's sum of squared differences fits its uint32 partial");

// four mask bytes -> 0x80 in every byte that is not 0
__device__ __forceinline__ unsigned score_nonzero_bytes(unsigned m) { return (((m & 0x7f7f7f7fu) + 0x7f7f7f7fu) | m) & 0x80808080u; }

// sum over the four bytes of (a - b)^2 = a.a + b.b - 2 a.b; every term and the result below 2^32 (v_dot4_u32_u8)
__device__ __forceinline__ unsigned score_sq_diff4(unsigned a, unsigned b) {
  const unsigned ab = __builtin_amdgcn_udot4(a, b, 0u, false);
  return __builtin_amdgcn_udot4(a, a, __builtin_amdgcn_udot4(b, b, 0u, false), false) - 2u * ab;
}

// the sum of (x, y) over a workgroup of 256 lanes: the wave's by xor shuffles, the four waves' through LDS; valid in thread 0
__device__ __forceinline__ void score_block_sum(unsigned& x, unsigned& y) {
  __shared__ unsigned s_part[4][2];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64), y += __shfl_xor(y, off, 64);
  const unsigned wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0u) s_part[wave][0] = x, s_part[wave][1] = y;
  __syncthreads();
  if (threadIdx.x == 0u) {
    x = (s_part[0][0] + s_part[1][0]) + (s_part[2][0] + s_part[3][0]);
    y = (s_part[0][1] + s_part[1][1]) + (s_part[2][1] + s_part[3][1]);
  }
}

// pass 1.  partial: the class's first pair (the dword class's at 0, the byte class's behind the dword grid); a / b: laid out
// as the plan's out arena.  Launched with 256 lanes, the flat tiles' block size.
template <int VEC>
__global__ __launch_bounds__(256) void sse_ragged_partial_kernel(const int* plan, const uint8_t* a_arena, const uint8_t* b_arena,
                                                                 const uint8_t* mask_arena, ScorePartial* partial,
                                                                 unsigned long long a_bytes, unsigned long long b_bytes,
                                                                 unsigned long long mask_bytes, unsigned long long hash, unsigned stamp,
                                                                 unsigned table_word, unsigned count) {
  // 1. whose plan is this?  A stale or foreign one: no output at all
  if (ragged_word(plan, RH_STAMP) != stamp || ragged_word64(plan, RH_HASH) != hash) return;

  // 2. the workgroup's image: the last descriptor whose first workgroup is <= blockIdx.x (scalar throughout)
  const int* tab = plan + table_word;
  const unsigned wg = blockIdx.x;
  unsigned lo = 0, hi = count;
  while (hi - lo > 1u) {
    const unsigned mid = (lo + hi) >> 1;
    if (ragged_word(tab, mid * kRaggedDescWords + RD_FIRST) <= wg) lo = mid;
    else hi = mid;
  }
  const int* d = tab + lo * kRaggedDescWords;
  const unsigned chunk = wg - ragged_word(d, RD_FIRST), n = ragged_word(d, RD_N);
  const unsigned long long mask_off = ragged_word64(d, RD_MASK_OFF), rgb_off = ragged_word64(d, RD_OUT_OFF);

  // 3. the descriptor's extents against the arenas, before any address is formed (every access below is to group
  //    min(., n - 1) of the image: inside [off, off + bytes) of its arena).  Workgroup-uniform.
  const unsigned long long px = (unsigned long long)n * VEC;
  bool ok = n != 0u && px <= (1ull << 30) && chunk < ragged_word(d, RD_TILES);
  ok = ok && rgb_off <= a_bytes && px * 3u <= a_bytes - rgb_off && rgb_off <= b_bytes && px * 3u <= b_bytes - rgb_off;
  ok = ok && (!mask_arena || (mask_off <= mask_bytes && px <= mask_bytes - mask_off));
  ok = ok && (rgb_off | mask_off) % (VEC == 4 ? 4u : 1u) == 0u;

  unsigned sse = 0u, kept = 0u;
  if (ok) {
    const unsigned base = chunk * 256u + threadIdx.x;
    const unsigned i = min(base, n - 1u);  // lanes past n: the load clamps, the contribution is dropped
    unsigned s = 0u, c = 0u;
    if constexpr (VEC == 4) {  // [R0 G0 B0 R1][G1 B1 R2 G2][B2 R3 G3 B3] of a and of b, one mask dword
      const unsigned* pa = reinterpret_cast<const unsigned*>(a_arena + rgb_off) + 3 * (size_t)i;
      const unsigned* pb = reinterpret_cast<const unsigned*>(b_arena + rgb_off) + 3 * (size_t)i;
      const unsigned a0 = ld<true>(pa), a1 = ld<true>(pa + 1), a2 = ld<true>(pa + 2);
      const unsigned b0 = ld<true>(pb), b1 = ld<true>(pb + 1), b2 = ld<true>(pb + 2);
      unsigned nz = 0x80808080u;
      if (mask_arena) nz = score_nonzero_bytes(ld<true>(reinterpret_cast<const unsigned*>(mask_arena + mask_off) + i));
      const unsigned k = (nz >> 7) * 0xffu;  // 0xff in the byte of every kept pixel
      // the pixels' bytes of the three dwords: masked-out pixels are 0 in both operands
      const unsigned k0 = __builtin_amdgcn_perm(k, k, 0x01000000u), k1 = __builtin_amdgcn_perm(k, k, 0x02020101u),
                     k2 = __builtin_amdgcn_perm(k, k, 0x03030302u);
      s = score_sq_diff4(a0 & k0, b0 & k0) + score_sq_diff4(a1 & k1, b1 & k1) + score_sq_diff4(a2 & k2, b2 & k2);
      c = (unsigned)__builtin_popcount(nz);
    } else {
      const uint8_t* pa = a_arena + rgb_off + 3 * (size_t)i;
      const uint8_t* pb = b_arena + rgb_off + 3 * (size_t)i;
      const int dr = (int)pa[0] - (int)pb[0], dg = (int)pa[1] - (int)pb[1], db = (int)pa[2] - (int)pb[2];
      c = mask_arena ? (mask_arena[mask_off + i] != 0) : 1u;
      s = c ? (unsigned)(dr * dr + dg * dg + db * db) : 0u;
    }
    if (base < n) sse = s, kept = c;
  }
  score_block_sum(sse, kept);  // (every thread of the workgroup is here: `ok` is workgroup-uniform)
  if (threadIdx.x == 0u) partial[2 * (size_t)wg] = sse, partial[2 * (size_t)wg + 1] = kept;
}

// pass 2.  Workgroup j takes descriptor j (the dword class's, then the byte class's); n_dword / grid_dword are the HOST plan's,
// the pairs of the byte class start behind the dword grid.  The descriptor's pairs [first, first + tiles) lie inside its
// class's grid or nothing is read.  Launched with 256 lanes.
__global__ __launch_bounds__(256) void sse_ragged_final_kernel(const int* plan, const ScorePartial* partial, unsigned long long* sums,
                                                               unsigned long long hash, unsigned stamp, unsigned B, unsigned n_dword,
                                                               unsigned grid_dword, unsigned grid_byte) {
  if (ragged_word(plan, RH_STAMP) != stamp || ragged_word64(plan, RH_HASH) != hash) return;
  const unsigned j = blockIdx.x;
  const int* d = plan + kRaggedHeaderWords + j * kRaggedDescWords;
  const unsigned first = ragged_word(d, RD_FIRST), tiles = ragged_word(d, RD_TILES), index = ragged_word(d, RD_INDEX);
  const bool dword = j < n_dword;
  const unsigned grid = dword ? grid_dword : grid_byte;
  if (index >= B || first > grid || tiles > grid - first) return;
  const ScorePartial* p = partial + 2 * ((size_t)(dword ? 0u : grid_dword) + first);
  unsigned long long s = 0ull, c = 0ull;
  for (unsigned t = threadIdx.x; t < tiles; t += 256u) s += p[2 * (size_t)t], c += p[2 * (size_t)t + 1];
  __shared__ unsigned long long s_sum[4][2];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64), c += __shfl_xor(c, off, 64);
  const unsigned wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0u) s_sum[wave][0] = s, s_sum[wave][1] = c;
  __syncthreads();
  if (threadIdx.x == 0u) {
    s = (s_sum[0][0] + s_sum[1][0]) + (s_sum[2][0] + s_sum[3][0]), c = (s_sum[0][1] + s_sum[1][1]) + (s_sum[2][1] + s_sum[3][1]);
    sums[2 * (size_t)index] = s, sums[2 * (size_t)index + 1] = c;
  }
}
