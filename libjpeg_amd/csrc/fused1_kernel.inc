// fused1_kernel.inc -- the text of fused1_kernel, included by kernels.hip (see there: once in mij, once in mij::ragged12, once in
// mij::window, where WINDOW_OUT is true: the crop windows of a list)
template <bool QDEV, int P = 8, bool RAGGED = false>
__global__ __launch_bounds__(F420_THREADS, 4) void fused1_kernel(Fused420Args a)
{
  static_assert(!RAGGED || QDEV, "ragged launches: per-frame tables");
  static_assert(!WINDOW_OUT || (RAGGED && P == 8), "crop windows: the 8-bit ragged flavour");
  PlanarBases pb{}; // (a single component is its own plane)
  WindowBox wb{};
  __shared__ __attribute__((aligned(16))) u32x4 stage_all[4][128];
  const TileCtx t = WINDOW_OUT ? tile_enter_window<false>(a, stage_all, pb, wb) : RAGGED ? tile_enter_ragged(a, stage_all) : tile_enter<1>(a, stage_all);
  if (t.padding) return;

  u32x4 rows[8];
  fetch_tile_blocks(rows, t, t.coef + a.off_y, a.bw_y, a.bh_y);
  WindowClip wc{};
  const BlockOut o = WINDOW_OUT ? block_out_window<P == 12 ? 2 : 1>(a, t, wb, wc) : block_out<P == 12 ? 2 : 1>(a, t);
  if (o.outside) return;
  int v[64];
  dequant_idct_sparse<!QDEV && P == 8>(rows, frame_deltas<QDEV>(a, t.frame, 0), v);
  uint8_t *__restrict__ out_frame = o.out_frame;
  const unsigned out_off = o.out_off;
  const int npx = o.npx, nln = o.nln;
  const bool fast_store = o.fast_store;
  if (P == 12) {
    // COLOR_TO_INT with the level shift 2^11 << 4 the transform left out: (x + 32768 + 8) >> 4, clamped to [0, 4095]
#pragma unroll
    for (int l = 0; l < 8; l++) {
      if (l < nln) {
        unsigned w[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const unsigned lo = (unsigned)min(max((v[l * 8 + 2 * i] + (32768 + 8)) >> 4, 0), 4095);
          const unsigned hi = (unsigned)min(max((v[l * 8 + 2 * i + 1] + (32768 + 8)) >> 4, 0), 4095);
          w[i] = lo | (hi << 16);
        }
        uint8_t *dst = out_frame + (out_off + (unsigned)l * (unsigned)a.row_stride);
        if (fast_store) {
          __builtin_nontemporal_store(u32x4{w[0], w[1], w[2], w[3]}, reinterpret_cast<u32x4_any *>(dst));
        } else {
          uint16_t *d16 = reinterpret_cast<uint16_t *>(dst);
#pragma unroll
          for (int x = 0; x < 8; x++)
            if (x < npx) d16[x] = (uint16_t)(w[x >> 1] >> (16 * (x & 1)));
        }
      }
    }
    return;
  }
#pragma unroll
  for (int l = 0; l < 8; l++) {
    if (WINDOW_OUT ? l >= wc.ln0 && l < nln : l < nln) {
      unsigned b4[2]; // four clamped samples each: level shift, COLOR_TO_INT's rounding, shift, clamp
#pragma unroll
      for (int h = 0; h < 2; h++)
        b4[h] = ashr_sat_pack4<4>(v[l * 8 + 4 * h] + (2048 + 8), v[l * 8 + 4 * h + 1] + (2048 + 8), v[l * 8 + 4 * h + 2] + (2048 + 8), v[l * 8 + 4 * h + 3] + (2048 + 8));
      uint8_t *dst = out_frame + (out_off + (unsigned)l * (unsigned)a.row_stride);
      if (fast_store) {
        __builtin_nontemporal_store(u32x2{b4[0], b4[1]}, reinterpret_cast<u32x2_any *>(dst));
      } else {
#pragma unroll
        for (int x = 0; x < 8; x++)
          if (WINDOW_OUT ? x >= wc.px0 && x < npx : x < npx) dst[x] = (uint8_t)(b4[x >> 2] >> (8 * (x & 3)));
      }
    }
  }
}
