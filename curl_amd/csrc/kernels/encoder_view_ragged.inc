// encoder_view_ragged.inc -- part of curl_kernels.hip (one translation unit; included after encoder_view.inc, whose tile code it
// runs, and after stream_ragged.inc, whose scalar plan reads it uses).
// ------------------------------------------------------------------------------------------------
// the encoder's views of a batch of images of different sizes, one launch (include/curl_hip_view_ragged.h)
// ------------------------------------------------------------------------------------------------
// One frame's view is launch-bound (400 workgroups at 1500 x 1000, 100 at 512 x 341).  Here the grid of ONE launch is the sum
// of all images' tiles, the step stream_ragged_kernel took for the per-pixel pass: a workgroup finds its image in the plan's
// descriptor table (a binary search of the running sums of workgroups; blockIdx.x and the table are wave-uniform, the loads
// scalar), fills a ViewArgs of its own from the descriptor -- every image keeps the tiling it has alone, and lays the
// workgroup's LDS out by its own numbers inside the launch's reservation, the largest image's -- and runs view_tile, the code
// of encoder_view_kernel, on its tile: that is what makes the bits equal.
//
// The plan's layout is the header's (the names there; csrc holds the numbers).
constexpr unsigned kViewRaggedStamp = 0x52565031u;
constexpr unsigned kViewRaggedHeaderWords = 32, kViewRaggedDescWords = 32;
enum {  // header words
  VH_STAMP = 0, VH_B, VH_SIZE, VH_HAS_MASK, VH_GRID, VH_LDS, VH_TABLES, VH_IMG_BYTES = 8, VH_MASK_BYTES = 10, VH_HASH = 12, VH_PLAN_BYTES = 14
};
enum {  // descriptor words
  VD_FIRST = 0, VD_INDEX, VD_H, VD_W, VD_CHANNELS, VD_TILES, VD_KSX, VD_KSY, VD_TC_LOG2, VD_TR, VD_NCOLS_CAP, VD_NROWS_CAP, VD_CHUNK_ROWS,
  VD_PITCH_IMG, VD_PITCH_MASK, VD_LDS, VD_TABLE = 16, VD_TABLE_WORDS = 18, VD_IMG_OFF = 20, VD_MASK_OFF = 22
};
constexpr unsigned kViewRaggedLdsBudget = 48u * 1024u;  // (host_api_view.inc's kViewLdsBudget: no launch reserves more)

// What the HOST plan says travels as arguments (B, size, the arena and plan sizes, the LDS reserved, stamp and hash); what the
// device plan says is held to it before any address is formed.
__global__ __launch_bounds__(256) void encoder_view_ragged_kernel(const int* plan, const uint8_t* img_arena, const uint8_t* mask_arena, float* view,
                                                                  float* mask_view, unsigned long long img_bytes, unsigned long long mask_bytes,
                                                                  unsigned long long plan_words, unsigned long long hash, unsigned stamp, unsigned B,
                                                                  int size, unsigned lds_bytes) {
  extern __shared__ __align__(16) unsigned char view_lds[];
  // 1. whose plan is this?  A stale or foreign one: no output at all
  if (ragged_word(plan, VH_STAMP) != stamp || ragged_word64(plan, VH_HASH) != hash) return;

  // 2. the workgroup's image: the last descriptor whose first workgroup is <= blockIdx.x (scalar throughout)
  const int* tab = plan + kViewRaggedHeaderWords;
  const unsigned wg = blockIdx.x;
  unsigned lo = 0, hi = B;
  while (hi - lo > 1u) {
    const unsigned mid = (lo + hi) >> 1;
    if (ragged_word(tab, mid * kViewRaggedDescWords + VD_FIRST) <= wg) lo = mid;
    else hi = mid;
  }
  const int* d = tab + (size_t)lo * kViewRaggedDescWords;
  const unsigned tile = wg - ragged_word(d, VD_FIRST);
  const unsigned img = ragged_word(d, VD_INDEX), H = ragged_word(d, VD_H), W = ragged_word(d, VD_W), channels = ragged_word(d, VD_CHANNELS);
  const unsigned long long img_off = ragged_word64(d, VD_IMG_OFF), mask_off = ragged_word64(d, VD_MASK_OFF), table = ragged_word64(d, VD_TABLE);

  // 3. the descriptor against the arenas, the plan and the LDS, before any address is formed.  Every return is
  //    workgroup-uniform (all of it is scalar), so the barriers of view_tile see the whole workgroup or none of it.
  const unsigned long long px = (unsigned long long)H * W;
  if (img >= B || (channels != 3u && channels != 4u) || H == 0u || W == 0u || px > (1ull << 30)) return;
  if (img_off > img_bytes || px * channels > img_bytes - img_off) return;
  if (mask_arena && (mask_off > mask_bytes || px > mask_bytes - mask_off)) return;
  const unsigned ksx = ragged_word(d, VD_KSX), ksy = ragged_word(d, VD_KSY), tc_log2 = ragged_word(d, VD_TC_LOG2), tr = ragged_word(d, VD_TR);
  const unsigned ncols_cap = ragged_word(d, VD_NCOLS_CAP), nrows_cap = ragged_word(d, VD_NROWS_CAP), chunk_rows = ragged_word(d, VD_CHUNK_ROWS);
  const unsigned pitch_img = ragged_word(d, VD_PITCH_IMG), pitch_mask = ragged_word(d, VD_PITCH_MASK);
  if (ksx == 0u || ksx > (unsigned)kViewMaxTaps || ksy == 0u || ksy > (unsigned)kViewMaxTaps || tc_log2 > 5u || tr == 0u || tr > 16u) return;
  if (ncols_cap == 0u || ncols_cap > kViewRaggedLdsBudget || nrows_cap == 0u || nrows_cap > kViewRaggedLdsBudget || chunk_rows == 0u ||
      chunk_rows > kViewRaggedLdsBudget)
    return;
  // a staged row: its bytes from the 4-byte boundary below its first, in whole dwords (view_stage_row)
  if (pitch_img > kViewRaggedLdsBudget || pitch_img % 4u || pitch_img < ((ncols_cap * channels + 3u + 3u) & ~3u)) return;
  if (pitch_mask > kViewRaggedLdsBudget || pitch_mask % 4u || (mask_arena && pitch_mask < ((ncols_cap + 3u + 3u) & ~3u))) return;
  const unsigned long long table_words = (unsigned long long)size * (unsigned long long)(view_row_ints((int)ksx) + view_row_ints((int)ksy));
  if (table > plan_words || table_words > plan_words - table) return;

  ViewArgs a = {nullptr, nullptr, plan, view, mask_view, (int)H, (int)W, size, (int)channels, (int)ksx, (int)ksy, (int)tc_log2, (int)tr, (int)ncols_cap,
                (int)nrows_cap, (int)chunk_rows, (int)pitch_img, (int)pitch_mask, 0, 0u, 0u, 0u};
  view_layout(a);
  if ((unsigned long long)a.off_stage + (unsigned long long)chunk_rows * (pitch_img + pitch_mask) > lds_bytes) return;
  const unsigned tiles = (unsigned)a.tiles_x * (((unsigned)size + tr - 1u) / tr);
  if (tile >= tiles || tile >= ragged_word(d, VD_TILES)) return;

  // 4. the tile, by the code of encoder_view_kernel
  const size_t plane = (size_t)size * (size_t)size;
  view_tile(a, view_lds, plan + table, img_arena + img_off, mask_arena ? mask_arena + mask_off : nullptr, view + (size_t)img * 3u * plane,
            mask_view ? mask_view + (size_t)img * plane : nullptr, view_tile_of(a, (int)tile));
}
