// bwd_tile.inc -- part of curl_kernels.hip (one translation unit; included in this order, not compiled alone).
// ------------------------------------------------------------------------------------------------
// the tile of the per-pixel backward kernels (layer_bwd_kernel, layer_pwl_bwd_kernel, stage_bwd_kernel)
// ------------------------------------------------------------------------------------------------
// One 256-thread workgroup per tile of 256 VEC-groups of one image, like the forward.  What the three kernels share lives
// here, once: the arguments of a tile, its addressing and loads with the mask protocol (BwdTile::load), a pixel's inputs
// (BwdTile::m, pin, gin), the guarded store of grad_img (BwdTile::store) and the block's row of partial sums (block_row_sum).  What is
// a kernel's own stays there: its coefficients or LDS table, its pullback, what it sums.
struct BwdArgs {
  const float* in;
  const float* gout;
  float* gin;         // nullable
  const void* mask;
  const float* coef;  // workspace (prep output)
  float* partial;     // [n_blocks][row] block partial sums (row: BWD_NACC, 2 * curves of a stage, n_knots of the PWL layer)
  unsigned coef_stride, n, blocks_per_image;
  unsigned n_blocks;  // (no kernel reads it: the offsets of the two fields below are part of layer_bwd_kernel's machine code)
  int mask_first;  // CURL_F_MASK_FIRST: test the mask before the six plane loads go out
  unsigned stamp;  // ws_stamp of the knot count / row stride this call's workspace rows must have been prepared for
};

// GIN: the kernel stores d loss / d img (store() is there for it).
template <int VEC, int MK, bool GIN>
struct BwdTile {
  typedef typename Pack<VEC>::T T;
  typedef typename Pack<VEC>::M M;
  static constexpr bool kNT = VEC == 4;  // streaming data, touched once (stream.inc)
  unsigned n;    // VEC-groups per plane
  size_t base;   // GIN: the image's first VEC-group in `in`, `gout` and `gin`
  unsigned i;    // this lane's VEC-group of the image
  __device__ __forceinline__ bool valid() const { return i < n; }  // ... which lies inside it
  // A wavefront whose pixels are all masked out (bool / uint8 masks: data.py:190's segmentation masks) has nothing to
  // compute: every gradient it would produce is an exact zero (curl_math_bwd.h, the binary specialisation).  It skips the
  // arithmetic -- and, with CURL_F_MASK_FIRST, asks for its mask bytes first and never reads its six planes.
  bool dead;
  T w2, w1, w0, x2, x1, x0;  // the six planes' groups (left undefined for a dead wave: nothing reads them)
  T mf;
  M mb;

  // How this is written decides whether layer_bwd_kernel's machine code stays what was benchmarked (tools/isa_fingerprint.py:
  // the float4 and the unmasked kernels are instruction for instruction what they were with the tile written out in the kernel).
  // The compiler simplifies load() on its own before it inlines it, so: plane, i, valid, dead and the mask bytes of the ballot
  // are locals, published at the end (a member is re-read from memory around every ld / st call, and the address arithmetic
  // comes out in another shape); `n`, not `plane`, is what the tile keeps, and `base` only with GIN (a value used again at the
  // end is not sunk into the `!dead` branch); the members are declared in the order that gives the merged values' order.
  __device__ __forceinline__ void load(const float* in, const float* gout, const void* mask, unsigned img, unsigned chunk,
                                       unsigned n, int mask_first) {
    const size_t plane = (size_t)n;
    const size_t base = (size_t)img * 3 * plane;
    const T* p0 = reinterpret_cast<const T*>(in) + base;
    const T* g0 = reinterpret_cast<const T*>(gout) + base;
    const unsigned i = chunk * 256u + threadIdx.x;
    const unsigned ic = min(i, n - 1u);
    const bool valid = i < n;
    bool dead = false;
    if constexpr (MK == CURL_MASK_U8) {
      if (mask_first) {
        const M mb = this->mb = ld<kNT>(at(reinterpret_cast<const M*>(mask) + (size_t)img * plane, ic));
        dead = __builtin_amdgcn_ballot_w64(valid && mb != 0) == 0ull;
      }
    }
    if (!dead) {
      x0 = ld<kNT>(at(p0, ic)), x1 = ld<kNT>(at(p0 + plane, ic)), x2 = ld<kNT>(at(p0 + 2 * plane, ic));
      w0 = ld<kNT>(at(g0, ic)), w1 = ld<kNT>(at(g0 + plane, ic)), w2 = ld<kNT>(at(g0 + 2 * plane, ic));
    } else {
      // "defined" without an instruction (left plainly undefined, the compiler zero-fills all 24 registers in front of the branch)
      asm volatile("" : "=v"(x0), "=v"(x1), "=v"(x2), "=v"(w0), "=v"(w1), "=v"(w2));
    }
    if constexpr (MK == CURL_MASK_U8) {
      if (!mask_first) {
        const M mb = this->mb = ld<kNT>(at(reinterpret_cast<const M*>(mask) + (size_t)img * plane, ic));
        dead = __builtin_amdgcn_ballot_w64(valid && mb != 0) == 0ull;
      }
    }
    if (MK == CURL_MASK_F32) mf = ld<kNT>(at(reinterpret_cast<const T*>(mask) + (size_t)img * plane, ic));
    this->n = n, this->i = i, this->dead = dead;
    if constexpr (GIN) this->base = base;
  }

  // Pixel e of the lane: its mask value (bool / uint8 / no mask: exactly 0 or 1), its input and its incoming gradient.  What a
  // lane past the end of the image gets instead (valid() is false: its loads were clamped to the last group) is the kernel's.
  // The kernels run a lane's pixels one after the other: left free, the compiler interleaves the reverse-mode chains of a lane's
  // four pixels and their tapes multiply the VGPR count (layer_bwd_kernel, round 2: 225, two waves per SIMD).  An empty asm in
  // each kernel's pixel loop makes this pixel's inputs depend on `dep`, the previous pixel's result (a scheduling fence alone
  // does not shorten the live ranges).  It stands in the kernels, behind their own treatment of the lanes past the end: moved in
  // here, in front of it, the stage kernels' code came out 30-50 instructions and up to 9 VGPRs away from what was measured.
  __device__ __forceinline__ float m(int e) const {
    float v = 1.0f;
    if (MK == CURL_MASK_U8) v = mlane(mb, e);
    if (MK == CURL_MASK_F32) v = lane(mf, e);
    return v;
  }
  __device__ __forceinline__ Px pin(int e) const { return Px{lane(x0, e), lane(x1, e), lane(x2, e)}; }
  __device__ __forceinline__ Px gin(int e) const { return Px{lane(w0, e), lane(w1, e), lane(w2, e)}; }

  // grad_img of the tile.  The coefficients came from the image's workspace row.  With CURL_F_WS_READY the caller vouches for
  // it; a row nobody prepared for this call's knot counts (a zeroed buffer, another K) must not turn into a plausible-looking
  // gradient image: the workgroup stores NaN instead of what it computed (the second-pass kernels do the same for the knot
  // gradients).  One scalar load per wave, here at the end: held from the start it would be one more live SGPR in a kernel that
  // has none to spare.  A BRANCH around two store sequences (the asm keeps it one): as `y = bad ? NaN : y` it was twelve selects
  // per lane on the product path, +1.3 % per 8 frames (profiles/r05/ab_r05_vs_r04_library.log).
  __device__ __forceinline__ void store(float* gin, const float* row, unsigned stamp, T y0, T y1, T y2) const {
    static_assert(GIN, "a tile without grad_img keeps no base");
    if (valid()) {
      const size_t plane = (size_t)n;
      const unsigned i = this->i;
      T* q0 = reinterpret_cast<T*>(gin) + base;
      if (__builtin_expect(reinterpret_cast<const unsigned*>(row)[WS_STAMP] != stamp, 0)) {
        T nan_t = T(__builtin_nanf(""));
        asm volatile("" : "+v"(nan_t));
        st<kNT>(at(q0, i), nan_t);
        st<kNT>(at(q0 + plane, i), nan_t);
        st<kNT>(at(q0 + 2 * plane, i), nan_t);
      } else {
        st<kNT>(at(q0, i), y0);
        st<kNT>(at(q0 + plane, i), y1);
        st<kNT>(at(q0 + 2 * plane, i), y2);
      }
    }
  }
};

// Row `bid` of `partial`, the block's own: wave sums by lane swaps + in-row DPP (wave_sum_many), then the 4 waves through
// LDS, added in a fixed order (no float atomics: the second pass sums the rows in a fixed order in float64, so results are
// reproducible).  (`bid` by reference: the kernel's own local, worked out where the kernel does -- by value it is sunk to here.)
template <int NACC>
__device__ __forceinline__ void block_row_sum(const float (&acc)[NACC], float (&sPart)[4][NACC], float* partial,
                                              const unsigned& bid) {
  const int wave = threadIdx.x >> 6, lane_id = threadIdx.x & 63;
  wave_sum_many(acc, sPart[wave], lane_id);
  __syncthreads();
  if (threadIdx.x < NACC) {
    int c = threadIdx.x;
    partial[(size_t)bid * NACC + c] = (sPart[0][c] + sPart[1][c]) + (sPart[2][c] + sPart[3][c]);
  }
}
