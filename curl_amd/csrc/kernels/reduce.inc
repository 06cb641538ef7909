// reduce.inc -- part of curl_kernels.hip (one translation unit; included in this order, not compiled alone).
// ------------------------------------------------------------------------------------------------
// wave-wide and strided sums shared by the backward, loss and metric kernels
// ------------------------------------------------------------------------------------------------
// wave-wide sum in 6 DPP adds (VALU rate; __shfl_xor compiles to ds_bpermute + a full wait each): the row's 16
// lanes by quad_perm / half-mirror / mirror, then row_bcast15 and row_bcast31.  The total is in lane 63.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_add(float x) {
  return x + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, ROW_MASK, 0xF, false));
}
// stage-major over a lane's M accumulators: consecutive DPP adds are independent (no wait states between them)
template <int CTRL, int ROW_MASK, int R, int M>
__device__ __forceinline__ void dpp_add_all(float (&x)[R][M]) {
#pragma unroll
  for (int o = 0; o < R; ++o)
#pragma unroll
    for (int j = 0; j < M; ++j) x[o][j] = dpp_add<CTRL, ROW_MASK>(x[o][j]);
  CURL_FENCE();
}
template <int R, int M>
__device__ __forceinline__ void wave_sum_lane63(float (&x)[R][M]) {
  dpp_add_all<0xB1, 0xF>(x);   // quad_perm [1,0,3,2]
  dpp_add_all<0x4E, 0xF>(x);   // quad_perm [2,3,0,1]
  dpp_add_all<0x141, 0xF>(x);  // row_half_mirror
  dpp_add_all<0x140, 0xF>(x);  // row_mirror: every lane of a row holds the row's sum
  dpp_add_all<0x142, 0xA>(x);  // row_bcast15 into rows 1 and 3
  dpp_add_all<0x143, 0xC>(x);  // row_bcast31 into rows 2 and 3
}
// Wave-wide sums of MANY per-lane values (the polynomial backward reduces 3 x 126 per block): the first two stages trade
// lanes between two registers instead of adding a shuffled copy to each -- v_permlane32_swap puts the two 32-lane halves
// of value A into one register's lower half and those of value B into its upper half (one add then serves both),
// v_permlane16_swap does the same with 16-lane rows -- so four values share one register for the four in-row DPP steps:
// 2 swaps + 3 adds + 4 DPP adds per FOUR values instead of 6 DPP adds per value.  dst[i] = sum over the wave of x[i].
__device__ __forceinline__ void lane_swap32(float& a, float& b) {  // a.hi32 <-> b.lo32
  typedef unsigned u2 __attribute__((ext_vector_type(2)));
  u2 r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
  a = __uint_as_float(r.x), b = __uint_as_float(r.y);
}
__device__ __forceinline__ void lane_swap16(float& a, float& b) {  // rows of 16 lanes: a.row1 <-> b.row0, a.row3 <-> b.row2
  typedef unsigned u2 __attribute__((ext_vector_type(2)));
  u2 r = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
  a = __uint_as_float(r.x), b = __uint_as_float(r.y);
}
template <int N>
__device__ __forceinline__ void wave_sum_many(const float (&x)[N], float* dst, int lane_id) {
  constexpr int NQ = (N + 3) / 4;
  float z[1][NQ];
#pragma unroll
  for (int j = 0; j < NQ; ++j) {
    float v0 = x[4 * j], v1 = 4 * j + 1 < N ? x[4 * j + 1] : 0.0f, v2 = 4 * j + 2 < N ? x[4 * j + 2] : 0.0f,
          v3 = 4 * j + 3 < N ? x[4 * j + 3] : 0.0f;
    lane_swap32(v0, v1);
    lane_swap32(v2, v3);
    float y0 = v0 + v1, y1 = v2 + v3;  // lanes 0-31 / 32-63: half sums of values 4j / 4j+1, and of 4j+2 / 4j+3
    lane_swap16(y0, y1);
    z[0][j] = y0 + y1;  // rows 0..3: values 4j, 4j+2, 4j+1, 4j+3, each summed over four lanes
  }
  CURL_FENCE();
  dpp_add_all<0xB1, 0xF>(z);   // quad_perm [1,0,3,2]
  dpp_add_all<0x4E, 0xF>(z);   // quad_perm [2,3,0,1]
  dpp_add_all<0x141, 0xF>(z);  // row_half_mirror
  dpp_add_all<0x140, 0xF>(z);  // row_mirror: every lane of a row holds the row's sum
  if ((lane_id & 15) == 0) {
    const int row = lane_id >> 4, off = ((row & 1) << 1) | (row >> 1);
#pragma unroll
    for (int j = 0; j < NQ; ++j)
      if (4 * j + off < N) dst[4 * j + off] = z[0][j];
  }
}
// A thread's walk over a strided series of float32 block partials, summed in float64: p[j], p[j + step], ... below n.
// Eight loads in flight and eight partial sums per thread (element u of every group of eight goes to sum u; the tail one element
// per sum, in order), added in a fixed tree: the order depends on (j, step, n) only -- bit-reproducible.  Written as
// `for (...) v += p[j]` the walk is one dependent load + add per step, a memory latency each: knots_bwd_kernel's was 16 us of a
// 120 us backward (round 3); the loss terms' and the polynomial coefficients' second passes got the same form in round 5
// (5.6 / 7.5 us each for a few thousand floats per image; the PSNR's two short series are faster as a plain loop).
__device__ __forceinline__ double walk_sum8(const float* p, size_t j, size_t step, size_t n) {
  double v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (; j + 7 * step < n; j += 8 * step) {
    float f[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) f[u] = p[j + u * step];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] += (double)f[u];
  }
  {
    float f[7];
#pragma unroll
    for (int u = 0; u < 7; ++u) f[u] = (j + u * step < n) ? p[j + u * step] : 0.0f;  // the tail's loads go out together too
#pragma unroll
    for (int u = 0; u < 7; ++u) v[u] += (double)f[u];
  }
  return ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
}
