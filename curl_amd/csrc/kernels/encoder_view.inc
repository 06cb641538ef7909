// encoder_view.inc -- part of curl_kernels.hip.  The encoder's view from image bytes (curl_math_view.h), one launch:
// grid (column tiles x row tiles, image); a 256-thread workgroup owns `tr` output rows x 2^tc_log2 output columns and
//   1. copies the rows of the two coefficient tables that its tile uses into LDS (the plan: built on the host, uploaded by
//      the caller), and reads from them the window of input rows and columns the tile needs;
//   2. walks that window in chunks of `chunk_rows` input rows: stages the chunk's bytes -- the interleaved image row segment
//      and, beside it, the mask's, as a one-channel image of pitch W -- with dword loads wherever a dword lies wholly inside
//      the segment (bytes at its two ends: neither the row pitch 3 W nor the image base is 4-byte aligned in general), then
//      runs the HORIZONTAL pass from those bytes into one packed dword {r, g, b, mask} per (input row, output column);
//   3. runs the VERTICAL pass over those rounded bytes, converts and stores: consecutive lanes, consecutive floats of a row.
// Every index that comes out of the plan is clamped to the window, and the window to the image by the call's own H and W:
// a foreign plan gives wrong values, never an access outside the tensors or the workgroup's LDS.
// Steps 1 - 3 are view_tile, which encoder_view_ragged_kernel (encoder_view_ragged.inc) runs too.
// (the kernel takes these one by one -- pointers and ints -- and derives the last four itself: view_layout)
struct ViewArgs {
  const uint8_t* img;
  const uint8_t* mask;  // nullable (then mask_view is too)
  const int* plan;
  float* view;
  float* mask_view;
  int H, W, size, C;
  int ksx, ksy;              // taps per row of the two tables, as the HOST derives them from H, W, size
  int tc_log2, tr;           // the tile: 2^tc_log2 output columns x tr output rows
  int ncols_cap, nrows_cap;  // no tile's window is larger (the tables of a matching plan never ask for more)
  int chunk_rows;
  int pitch_img, pitch_mask;             // LDS bytes per staged row
  int tiles_x;
  unsigned off_ky, off_h, off_stage;     // LDS byte offsets (the X rows lie at 0)
};

// LDS ints per table row: {first, count, k[ksize]}, padded to an odd stride (lanes read different rows at the same tap)
__host__ __device__ static inline int view_lds_row(int ksize) { return view_row_ints(ksize) | 1; }
// the LDS of a workgroup: X rows | Y rows | horizontal results, a dword per (window row, tile column) | staged rows
__host__ __device__ static inline void view_layout(ViewArgs& a) {
  a.tiles_x = (a.size + (1 << a.tc_log2) - 1) >> a.tc_log2;
  a.off_ky = 4u * (unsigned)(view_lds_row(a.ksx) << a.tc_log2);
  a.off_h = a.off_ky + 4u * (unsigned)(a.tr * view_lds_row(a.ksy));
  a.off_stage = a.off_h + 4u * (unsigned)(a.nrows_cap << a.tc_log2);
}
__host__ __device__ static inline unsigned view_lds_bytes(const ViewArgs& a) {
  return a.off_stage + (unsigned)a.chunk_rows * (unsigned)(a.pitch_img + a.pitch_mask);
}

// len bytes from g to the LDS dwords at dst, laid out from g's 4-byte boundary below: byte i of the segment lands at LDS byte
// ((uintptr_t)g & 3) + i.  One wavefront per call; a dword that the segment does not cover whole is put together from its bytes.
__device__ __forceinline__ void view_stage_row(const uint8_t* g, int len, unsigned* dst, int lane) {
  const uintptr_t lo = (uintptr_t)g, hi = lo + (uintptr_t)len, a0 = lo & ~(uintptr_t)3;
  const int ndw = (int)((hi - a0 + 3) >> 2);
  for (int j = lane; j < ndw; j += 64) {
    const uintptr_t a = a0 + 4u * (uintptr_t)j;
    unsigned v = 0;
    if (a >= lo && a + 4 <= hi) {
      v = *reinterpret_cast<const unsigned*>(a);
    } else {
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (a + t >= lo && a + t < hi) v |= (unsigned)*reinterpret_cast<const uint8_t*>(a + t) << (8 * t);
    }
    dst[j] = v;
  }
}

__device__ __forceinline__ int view_clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }
// first + count - origin of table entries that may hold anything: wrapping, never overflowing
__device__ __forceinline__ int view_span(int first, int count, int origin) { return (int)((unsigned)first + (unsigned)count - (unsigned)origin); }

// A workgroup's tile of a view: its first output column and row, and how many of each lie inside the view
struct ViewTile {
  int c0, r0, nc, nr;
};
__device__ __forceinline__ ViewTile view_tile_of(const ViewArgs& a, int tile) {
  const int tx = tile % a.tiles_x, ty = tile / a.tiles_x;
  const int c0 = tx << a.tc_log2, r0 = ty * a.tr;
  return ViewTile{c0, r0, min(1 << a.tc_log2, a.size - c0), min(a.tr, a.size - r0)};
}

// Steps 1 - 3 for ONE tile of ONE image: the code of both kernels (one copy: the shared arithmetic is what makes their bits
// equal).  a: the image's numbers, laid out (view_layout); view_lds: the workgroup's LDS, view_lds_bytes(a) of it; plan_x: the
// image's two tables (`size` X rows, then `size` Y rows); img_b / mask_b: the image's first byte (mask_b nullable); vout / mout:
// the image's [3,size,size] / [1,size,size] (mout nullable).  Every thread of the workgroup calls it (barriers inside).
__device__ __forceinline__ void view_tile(const ViewArgs& a, unsigned char* view_lds, const int* plan_x, const uint8_t* img_b, const uint8_t* mask_b,
                                          float* vout, float* mout, const ViewTile& tile) {
  int* const kx = reinterpret_cast<int*>(view_lds);
  int* const ky = reinterpret_cast<int*>(view_lds + a.off_ky);
  unsigned* const hbuf = reinterpret_cast<unsigned*>(view_lds + a.off_h);
  unsigned char* const stage = view_lds + a.off_stage;
  const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
  const int S = a.size, TC = 1 << a.tc_log2, C = a.C;
  const int c0 = tile.c0, r0 = tile.r0, nc = tile.nc, nr = tile.nr;
  const size_t plane = (size_t)S * (size_t)S;

  // 1. the tile's table rows: a wavefront per row
  const int rix = view_row_ints(a.ksx), riy = view_row_ints(a.ksy), lsx = view_lds_row(a.ksx), lsy = view_lds_row(a.ksy);
  const int* const plan_y = plan_x + (size_t)S * (size_t)rix;
  for (int c = wave; c < nc; c += 4)
    for (int j = lane; j < rix; j += 64) kx[c * lsx + j] = plan_x[(size_t)(c0 + c) * (size_t)rix + j];
  for (int r = wave; r < nr; r += 4)
    for (int j = lane; j < riy; j += 64) ky[r * lsy + j] = plan_y[(size_t)(r0 + r) * (size_t)riy + j];
  __syncthreads();
  // the window: from the first row's first sample to the last row's last, inside the image and inside the LDS set aside
  const int wx0 = view_clampi(kx[0], 0, a.W - 1);
  const int ncols = view_clampi(view_span(kx[(nc - 1) * lsx], kx[(nc - 1) * lsx + 1], wx0), 1, min(a.ncols_cap, a.W - wx0));
  const int wy0 = view_clampi(ky[0], 0, a.H - 1);
  const int nrows = view_clampi(view_span(ky[(nr - 1) * lsy], ky[(nr - 1) * lsy + 1], wy0), 1, min(a.nrows_cap, a.H - wy0));

  unsigned char* const mstage = stage + (size_t)a.chunk_rows * (size_t)a.pitch_img;

  // 2. chunks of input rows: stage, then the horizontal pass
  for (int cy = 0; cy < nrows; cy += a.chunk_rows) {
    const int rows = min(a.chunk_rows, nrows - cy);
    for (int r = wave; r < rows; r += 4) {
      const size_t px = (size_t)(wy0 + cy + r) * (size_t)a.W + (size_t)wx0;
      view_stage_row(img_b + px * (size_t)C, ncols * C, reinterpret_cast<unsigned*>(stage + (size_t)r * a.pitch_img), lane);
      if (mask_b) view_stage_row(mask_b + px, ncols, reinterpret_cast<unsigned*>(mstage + (size_t)r * a.pitch_mask), lane);
    }
    __syncthreads();
    for (int i = t; i < (rows << a.tc_log2); i += 256) {
      const int c = i & (TC - 1), r = i >> a.tc_log2;
      if (c >= nc) continue;
      const int* const kr = kx + c * lsx;
      const int off = view_clampi(view_span(kr[0], 0, wx0), 0, ncols - 1), cnt = view_clampi(kr[1], 0, a.ksx);
      const size_t px = (size_t)(wy0 + cy + r) * (size_t)a.W + (size_t)wx0;
      const unsigned char* const srow = stage + (size_t)r * a.pitch_img + ((uintptr_t)(img_b + px * (size_t)C) & 3);
      const unsigned char* const mrow = mstage + (size_t)r * a.pitch_mask + ((uintptr_t)(mask_b + px) & 3);
      unsigned s0 = view_tap_start(), s1 = s0, s2 = s0, sm = s0;
      for (int x = 0; x < cnt; ++x) {
        const int p = min(off + x, ncols - 1), k = kr[2 + x];
        const unsigned char* const q = srow + p * C;
        s0 = view_tap(s0, k, q[0]), s1 = view_tap(s1, k, q[1]), s2 = view_tap(s2, k, q[2]);
        if (mask_b) sm = view_tap(sm, k, mrow[p]);
      }
      hbuf[((cy + r) << a.tc_log2) + c] = view_clip(s0) | view_clip(s1) << 8 | view_clip(s2) << 16 | (mask_b ? view_clip(sm) << 24 : 0u);
    }
    __syncthreads();
  }

  // 3. the vertical pass on the rounded bytes, to_tensor, and the mask's `> 0`
  for (int i = t; i < (nr << a.tc_log2); i += 256) {
    const int c = i & (TC - 1), r = i >> a.tc_log2;
    if (c >= nc) continue;
    const int* const kr = ky + r * lsy;
    const int off = view_clampi(view_span(kr[0], 0, wy0), 0, nrows - 1), cnt = view_clampi(kr[1], 0, a.ksy);
    unsigned s0 = view_tap_start(), s1 = s0, s2 = s0, sm = s0;
    for (int y = 0; y < cnt; ++y) {
      const int p = min(off + y, nrows - 1), k = kr[2 + y];
      const unsigned v = hbuf[(p << a.tc_log2) + c];
      s0 = view_tap(s0, k, v), s1 = view_tap(s1, k, v >> 8), s2 = view_tap(s2, k, v >> 16), sm = view_tap(sm, k, v >> 24);
    }
    const size_t o = (size_t)(r0 + r) * (size_t)S + (size_t)(c0 + c);
    vout[o] = view_unit(view_clip(s0)), vout[plane + o] = view_unit(view_clip(s1)), vout[2 * plane + o] = view_unit(view_clip(s2));
    if (mout) mout[o] = view_mask(view_clip(sm));
  }
}

__global__ __launch_bounds__(256) void encoder_view_kernel(const uint8_t* img, const uint8_t* mask, const int* plan, float* view, float* mask_view,
                                                           int H, int W, int size, int C, int ksx, int ksy, int tc_log2, int tr, int ncols_cap,
                                                           int nrows_cap, int chunk_rows, int pitch_img, int pitch_mask) {
  ViewArgs a = {img, mask, plan, view, mask_view, H, W, size, C, ksx, ksy, tc_log2, tr, ncols_cap, nrows_cap, chunk_rows, pitch_img, pitch_mask, 0, 0u, 0u, 0u};
  view_layout(a);
  extern __shared__ __align__(16) unsigned char view_lds[];

  const int t = (int)threadIdx.x;
  const int S = a.size, TC = 1 << a.tc_log2, b = (int)blockIdx.y;
  const ViewTile tile = view_tile_of(a, (int)blockIdx.x);
  float* const vout = a.view + (size_t)b * 3u * (size_t)S * (size_t)S;
  float* const mout = a.mask_view ? a.mask_view + (size_t)b * (size_t)S * (size_t)S : nullptr;
  const size_t plane = (size_t)S * (size_t)S;

  // a plan made for another shape: say so in every value (as the layer backward answers an unprepared workspace row)
  const ViewHeader* const hdr = reinterpret_cast<const ViewHeader*>(a.plan);
  if (hdr->stamp != kViewStamp || hdr->H != a.H || hdr->W != a.W || hdr->size != S) {
    const float nan = __builtin_nanf("");
    for (int i = t; i < (tile.nr << a.tc_log2); i += 256) {
      const int c = i & (TC - 1), r = i >> a.tc_log2;
      if (c >= tile.nc) continue;
      const size_t o = (size_t)(tile.r0 + r) * (size_t)S + (size_t)(tile.c0 + c);
      vout[o] = nan, vout[plane + o] = nan, vout[2 * plane + o] = nan;
      if (mout) mout[o] = nan;
    }
    return;
  }

  const uint8_t* const img_b = a.img + (size_t)b * (size_t)a.H * (size_t)a.W * (size_t)C;
  const uint8_t* const mask_b = a.mask ? a.mask + (size_t)b * (size_t)a.H * (size_t)a.W : nullptr;
  view_tile(a, view_lds, a.plan + kViewHeaderInts, img_b, mask_b, vout, mout, tile);
}
