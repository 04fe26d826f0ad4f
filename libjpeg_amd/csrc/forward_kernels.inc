// forward_kernels.inc -- the text of the three forward kernels (forward.hip includes it; see there for what they compute and for
// the helpers they call).  It is included three times: in namespace mij, where the uniform flavours of both precisions and the ragged
// 8-bit flavours are instantiated, in namespace mij::ragged12 for the ragged 12-bit flavours (the reason is in forward.hip), and in
// namespace mij::planar_in, where PLANAR_IN is true and the pixel's three samples come from three planes (ragged 8-bit flavours only).
// No include guard on purpose.
template <bool RAGGED, int P>
__global__ __launch_bounds__(256) void fdct_blocks_kernel(const typename KernelArgs<RAGGED>::type k)
{
  RaggedItem it{};
  if constexpr (RAGGED) it = find_item(k);
  auto &a = args_of(k, it);
  const unsigned per_frame = a.first_block[a.ncomp];
  const unsigned gid = (RAGGED ? it.wg : blockIdx.x) * blockDim.x + threadIdx.x;
  const unsigned frame = RAGGED ? 0u : blockIdx.y;
  if (gid >= per_frame) return;
  int c = 0;
  while (c + 1 < a.ncomp && gid >= a.first_block[c + 1]) c++;
  const unsigned bi = gid - a.first_block[c];
  const int by = (int)(bi / (unsigned)a.bw[c]), bx = (int)(bi - (unsigned)by * (unsigned)a.bw[c]);
  int16_t *dst = a.coef + (int64_t)frame * a.coef_frame_stride + a.coef_off[c] + (int64_t)bi * 64;
  if (bx >= a.nbx[c] || by >= a.nby[c]) { // MCU padding: no samples; left zero for the entropy coder to fill
    u32x4 *d4 = reinterpret_cast<u32x4 *>(dst);
#pragma unroll
    for (int i = 0; i < 8; i++) d4[i] = u32x4{0, 0, 0, 0};
    return;
  }
  const int W = a.width, H = a.height, nc = a.ncomp, sx = a.subx[c], sy = a.suby[c];
  const uint8_t *img = a.pixels + (int64_t)frame * a.pixel_frame_stride;
  const bool ycc = nc == 3 && a.ycbcr;
  auto sample = [&](int x, int y) -> int { // component c of pixel (x, y), x < W, y < H, with COLOR_BITS fractional bits
    if constexpr (PLANAR_IN) { // three planes of bytes (img is plane 0), read byte by byte: any address, any pitch
      const InputPlanes pl = input_planes<PLANAR_IN>(k, it); // (uniform and read-only: loaded once, outside the loops)
      const int64_t at = (int64_t)y * a.pixel_row_stride + x;
      if (ycc) return ycc_component<P>(c, img[at], pl.p1[at], pl.p2[at]);
      return (int)(c == 0 ? img : c == 1 ? pl.p1 : pl.p2)[at] << 4;
    } else if constexpr (P == 8) {
      const uint8_t *p = img + (int64_t)y * a.pixel_row_stride + (int64_t)x * nc;
      if (ycc) return ycc_component<P>(c, p[0], p[1], p[2]);
      return (int)p[c] << 4;
    } else {
      const uint16_t *p = reinterpret_cast<const uint16_t *>(img + (int64_t)y * a.pixel_row_stride) + (int64_t)x * nc;
      if (ycc) return ycc_component<P>(c, p[0], p[1], p[2]);
      return (int)p[c] << 4;
    }
  };
  int blk[64];
  // interior blocks of frames the fast kernels cover are theirs
  if (a.fast[c] && bx < a.fast_nbx[c] && by < a.fast_nby[c]) return;
  if (sx == 1 && sy == 1) {
    // partial blocks are pre-filled with the level shift (ycbcrtrafo.cpp:100-113)
#pragma unroll
    for (int r = 0; r < 8; r++) {
      const int y = by * 8 + r;
#pragma unroll
      for (int i = 0; i < 8; i++) {
        const int x = bx * 8 + i;
        blk[r * 8 + i] = (x < W && y < H) ? sample(x, y) : ((1 << (P - 1)) << 4);
      }
    }
  } else {
    // box filter over the lines that exist; beyond the right edge the line is the mirror image of its end
    // (downsamplerbase.cpp:141-145), a row of the block without any line stays zero (downsampler.cpp:92-95)
    const int ofs = (bx * sx) << 3;
    int y = (by * sy) << 3;
#pragma unroll
    for (int r = 0; r < 8; r++) { // unrolled: blk stays in registers
      int acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      int lines = 0;
      while (lines < sy && y < H) {
        for (int i = 0; i < 8; i++)
          for (int k = 0; k < sx; k++) {
            int x = ofs + i * sx + k;
            if (x >= W) { const int m = x - W; x = W > m ? W - 1 - m : 0; }
            acc[i] += sample(x, y);
          }
        lines++;
        y++;
      }
      const int norm = lines * sx;
#pragma unroll
      for (int i = 0; i < 8; i++) blk[r * 8 + i] = norm > 1 ? acc[i] / norm : acc[i];
    }
  }
  transform_and_store<P>(blk, a.invq[c], dst);
}

// 4:2:0, tiles of 128 x 128 pixels that lie wholly inside the picture: one workgroup of 256 lanes per tile.  Every lane reads
// the 8 x 8 pixels of ONE luma block once (48 dwords, one memory round trip), computes Y, Cb and Cr of each, transforms the
// luma block, and leaves the 4 x 4 box-filtered chroma samples of its pixels (sums of 2 x 2, >> 2) in LDS; after a
// barrier 128 lanes pick up the 64 + 64 chroma blocks of the tile and transform them.  Compared with the per-component
// kernels no pixel is fetched or unpacked twice.  grid (tiles_x * tiles_y, frames)
// Precision 12: a lane's 8 x 8 pixels are 8 rows of 48 bytes, three 16-byte loads each, taken in two batches of four rows (48
// dwords in flight, as at 8 bits); the box-filtered chroma with its 4 fractional bits reaches 65535, so the LDS samples are
// unsigned there.
template <bool RAGGED, int P>
__global__ __launch_bounds__(256, 2) void fdct420_tile_kernel(const typename KernelArgs<RAGGED>::type k)
{
  typedef typename ChromaSample<P>::type chroma_t;
  constexpr int SB = P == 8 ? 1 : 2; // bytes per sample
  constexpr int RB = 8 / SB;         // rows per batch of loads
  __shared__ chroma_t chroma[2][64 * 64]; // [Cb, Cr][64 lines of 64 samples]
  RaggedItem it{};
  if constexpr (RAGGED) it = find_item(k);
  auto &a = args_of(k, it);
  const int tiles_x = a.width >> 7;
  const int tile = RAGGED ? (int)it.wg : (int)blockIdx.x;
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const unsigned frame = RAGGED ? 0u : blockIdx.y;
  const uint8_t *img = a.pixels + (int64_t)frame * a.pixel_frame_stride;
  int16_t *coef = a.coef + (int64_t)frame * a.coef_frame_stride;
  const int lane = threadIdx.x;
  const int lbx = lane & 15, lby = lane >> 4; // luma block inside the tile
  const int x0 = tx * 128 + lbx * 8, y0 = ty * 128 + lby * 8;
  const InputPlanes pl = input_planes<PLANAR_IN>(k, it);
  {
    int blk[64];
    chroma_t *cb = chroma[0] + (lby * 4) * 64 + lbx * 4, *cr = chroma[1] + (lby * 4) * 64 + lbx * 4;
#pragma unroll
    for (int r0 = 0; r0 < 8; r0 += RB) {
      unsigned dw[RB][6 * SB];
#pragma unroll
      for (int r = 0; r < RB; r++) {
        if constexpr (PLANAR_IN) { // 8 bytes of each plane: two dwords x 3 planes where the interleaved line is 6 dwords
          const int64_t at = (int64_t)(y0 + r0 + r) * a.pixel_row_stride + x0;
          load_line_planar(img + at, pl.p1 + at, pl.p2 + at, dw[r]);
        } else
          load_line<P>(img + (int64_t)(y0 + r0 + r) * a.pixel_row_stride + (int64_t)x0 * (3 * SB), dw[r]);
      }
      if constexpr (RB < 8) __builtin_amdgcn_sched_barrier(0); // the loads of one batch together, as in gather_block_fast
#pragma unroll
      for (int r = r0; r < r0 + RB; r += 2) {
        int sb[4] = {0, 0, 0, 0}, sr[4] = {0, 0, 0, 0};
#pragma unroll
        for (int rr = 0; rr < 2; rr++)
#pragma unroll
          for (int i = 0; i < 8; i++) {
            const int j = 3 * i;
            const auto &d = dw[r - r0 + rr];
            const int r8 = PLANAR_IN ? line_sample_planar(d, 0, i) : line_sample<P>(d, j);
            const int g8 = PLANAR_IN ? line_sample_planar(d, 1, i) : line_sample<P>(d, j + 1);
            const int b8 = PLANAR_IN ? line_sample_planar(d, 2, i) : line_sample<P>(d, j + 2);
            blk[(r + rr) * 8 + i] = ycc_component<P>(0, r8, g8, b8);
            sb[i >> 1] += ycc_component<P>(1, r8, g8, b8);
            sr[i >> 1] += ycc_component<P>(2, r8, g8, b8);
          }
#pragma unroll
        for (int i = 0; i < 4; i++) {
          cb[(r >> 1) * 64 + i] = (chroma_t)(sb[i] >> 2);
          cr[(r >> 1) * 64 + i] = (chroma_t)(sr[i] >> 2);
        }
      }
      if constexpr (RB < 8) __builtin_amdgcn_sched_barrier(0);
    }
    transform_and_store<P>(blk, a.invq[0], coef + a.coef_off[0] + ((int64_t)(y0 >> 3) * a.bw[0] + (x0 >> 3)) * 64);
  }
  __syncthreads();
  if (lane < 128) {
    const int c = 1 + (lane >> 6), n = lane & 63, cbx = n & 7, cby = n >> 3;
    const chroma_t *src = chroma[c - 1] + (cby * 8) * 64 + cbx * 8;
    int blk[64];
#pragma unroll
    for (int r = 0; r < 8; r++)
#pragma unroll
      for (int i = 0; i < 8; i++) blk[r * 8 + i] = src[r * 64 + i];
    transform_and_store<P>(blk, a.invq[c], coef + a.coef_off[c] + ((int64_t)(ty * 8 + cby) * a.bw[c] + (tx * 8 + cbx)) * 64);
  }
}

// the interior blocks of component c: grid (blocks of 256 lanes over fast_nbx * fast_nby, frames)
// (The uniform 2 x 2 flavour fills its 256 registers and spills 32 bytes a lane; the ragged one needs a few more and gets one
// workgroup per CU instead -- 512 registers, the surplus in AGPRs -- so that it touches no scratch memory.  It only sees what
// the tile kernel leaves of a 4:2:0 picture: the strips right of and below the whole tiles, and pictures below 128 x 128.
// The precision-12 2 x 2 flavour would spill 22 registers at two workgroups per CU and gets one as well.)
template <int SX, int SY, bool RAGGED, int P>
__global__ __launch_bounds__(256, SX * SY == 4 ? (RAGGED || P == 12 ? 1 : 2) : 3) void fdct_interior_kernel(const typename KernelArgs<RAGGED>::type k, int c)
{
  RaggedItem it{};
  if constexpr (RAGGED) {
    it = find_item(k);
    c = (int)it.comp;
  }
  auto &a = args_of(k, it);
  const unsigned gid = (RAGGED ? it.wg : blockIdx.x) * blockDim.x + threadIdx.x, frame = RAGGED ? 0u : blockIdx.y;
  const unsigned n = (unsigned)a.fast_nbx[c] * (unsigned)a.fast_nby[c];
  if (gid >= n) return;
  const int by = (int)(gid / (unsigned)a.fast_nbx[c]), bx = (int)(gid - (unsigned)by * (unsigned)a.fast_nbx[c]);
  if (a.tiled420 && bx < a.tile_nbx[c] && by < a.tile_nby[c]) return; // the tile kernel's
  int16_t *dst = a.coef + (int64_t)frame * a.coef_frame_stride + a.coef_off[c] + ((int64_t)by * a.bw[c] + bx) * 64;
  const uint8_t *img = a.pixels + (int64_t)frame * a.pixel_frame_stride;
  int blk[64];
  if constexpr (PLANAR_IN) {
    const InputPlanes pl = input_planes<PLANAR_IN>(k, it);
    gather_block_fast_planar<SX, SY>(img, pl.p1, pl.p2, a.pixel_row_stride, (bx * SX) << 3, (by * SY) << 3, c, blk);
  } else
    gather_block_fast<SX, SY, P>(img, a.pixel_row_stride, (bx * SX) << 3, (by * SY) << 3, c, blk);
  transform_and_store<P>(blk, a.invq[c], dst);
}
