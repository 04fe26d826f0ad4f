// fused420_kernel.inc -- the text of fused420_kernel, included by kernels.hip (see there: once in mij, once in mij::ragged12, once
// in mij::planar, where PLANAR_OUT is true: component planes out; in mij::window and mij::window::planar, where WINDOW_OUT is true:
// the crop windows of a list)
template <bool FAST, int MINW, bool QDEV, int P = 8, bool N12 = false, bool RAGGED = false>
__global__ __launch_bounds__(F420_THREADS, MINW) void fused420_kernel(Fused420Args a)
{
  static_assert(P == 8 || (P == 12 && FAST), "12-bit frames: FAST flavour only (the host checks the ranges)");
  static_assert(!RAGGED || QDEV, "ragged launches: per-frame tables");
  static_assert(!PLANAR_OUT || (RAGGED && P == 8), "planar output: the 8-bit ragged flavours");
  static_assert(!WINDOW_OUT || (RAGGED && P == 8), "crop windows: the 8-bit ragged flavours");
  __shared__ __attribute__((aligned(16))) int cplane[2][F420_CROWS * F420_CPITCH];
  __shared__ __attribute__((aligned(16))) u32x4 stage_all[4][128];

  PlanarBases pb{};
  WindowBox wb{};
  const TileCtx t = WINDOW_OUT ? tile_enter_window<PLANAR_OUT>(a, stage_all, pb, wb) : PLANAR_OUT ? tile_enter_planar(a, stage_all, pb) : RAGGED ? tile_enter_ragged(a, stage_all) : tile_enter<P == 8 ? MIJ_TILE_ORDER : 1>(a, stage_all);
  if (t.padding) return;

  // the luma blocks of phase B are requested in front of phase A's transform (see F420P_MINW; two workgroups per CU leave the 32
  // registers) -- 8-bit frames only: the 12-bit flavour fetches them at the start of phase B
  u32x4 yraw[8];
  auto luma_loads = [&]() { load_tile_blocks(yraw, t, t.coef + a.off_y, a.bw_y, a.bh_y); };
  constexpr bool PREFETCH = P == 8;
  if (PREFETCH) f420_chroma_to_lds<FAST, QDEV, !QDEV && P == 8>(a, t, cplane, luma_loads);
  else f420_chroma_to_lds<FAST, QDEV, !QDEV && P == 8>(a, t, cplane);
  __syncthreads();
  f420_chroma_edges(a, cplane, t.tid, t.tx, t.ty);

  // ------------------------------------------------------------------ phase B: luma + colour
  u32x4 rows[8];
  if (!PREFETCH) luma_loads();
  transpose_blocks(rows, t.stage, t.lane, yraw);
  WindowClip wc{};
  const BlockOut o = WINDOW_OUT ? block_out_window<PLANAR_OUT ? 1 : P == 12 ? 6 : 3>(a, t, wb, wc) : block_out<PLANAR_OUT ? 1 : P == 12 ? 6 : 3>(a, t);
  if (o.outside) return; // no barrier below this point
  int yv[64];
  if (FAST) dequant_idct_sparse<!QDEV && P == 8, P == 8>(rows, frame_deltas<QDEV>(a, t.frame, 0), yv, 0, P == 8 ? LUMA_FOLD_R2 : 2048); // (8 bit: doubled sums, luma13)
  else dequant_idct<false>(rows, frame_deltas<QDEV>(a, t.frame, 0), yv, 128 << 7);

  // chroma window of this block: lines pr = 4 by + m (+0 top, +1 cur, +2 bot), columns pc = 4 bx + 3 + j
  const int *cb_base = cplane[0] + (4 * o.by) * F420_CPITCH + 4 * o.bx;
  const int *cr_base = cplane[1] + (4 * o.by) * F420_CPITCH + 4 * o.bx;

  int cbT[6], cbC[6], cbB[6], crT[6], crC[6], crB[6];
  load6(cb_base, cbT); load6(cb_base + F420_CPITCH, cbC);
  load6(cr_base, crT); load6(cr_base + F420_CPITCH, crC);

#pragma unroll
  for (int m = 0; m < 4; m++) {
    load6(cb_base + (m + 2) * F420_CPITCH, cbB);
    load6(cr_base + (m + 2) * F420_CPITCH, crB);
#pragma unroll
    for (int half = 0; half < 2; half++) {
      const int l = 2 * m + half;
      // vertical filter (upsampler.cpp:149-165): even output lines look up, odd ones down; the
      // rounding constant alternates with the buffer column parity
      int vb[6], vr[6];
#pragma unroll
      for (int j = 0; j < 6; j++) {
        const int rnd = ((j & 1) ^ half) ? 1 : 2;
        vb[j] = tap13(half ? cbB[j] : cbT[j], cbC[j], rnd);
        vr[j] = tap13(half ? crB[j] : crT[j], crC[j], rnd);
      }
      int ub[8], ur[8];
      hfilter8(vb, ub);
      hfilter8(vr, ur);
      if (WINDOW_OUT ? l >= wc.ln0 && l < o.nln : l < o.nln) {
        if (FAST && P == 12) {
          // (y * 8192 + (cb - 32768) * Lb + (cr - 32768) * Lr + 65536) >> 17, clamped to [0, 4095] (ycbcrtrafo.cpp:842-856,
          // :921-936; the reference accumulates in 64 bits).  With y = y' + 32768, cb - 32768 = cb' (no level shift in the
          // transforms) and c L = q 2^13 + r, 0 <= r < 2^13:  ((y' + 32776 + q) 2^13 + r) >> 17 = (y' + 32776 + q) >> 4
          // exactly.  The products must fit 32 bits: |c| <= 4.02 * 45056 + 2 < 181 200 by the host's range check (an IDCT
          // output times 16 is at most 4 sum |c_k| q_k; the 9-bit constants and the two roundings add < 0.5 %), times 11485
          // < 2^31; Lb = 14516 = 4 * 3629 is applied as (c * 3629) >> 11, which is the same number.
          int rr[8], gg[8], bb[8];
#pragma unroll
          for (int x = 0; x < 8; x++) colour12<N12>(yv[l * 8 + x], ub[x], ur[x], rr[x], gg[x], bb[x]);
          store_rgb12_line<F420_12_TEMPORAL>(o.out_frame + o.line_off(l, a), rr, gg, bb, o.fast_store, o.npx);
        } else if (FAST) {
          // y, cb, cr arrive WITHOUT the level shift (DCOFF = false): with y = y' + 2048 and cb - 2048 = cb' the
          // reference's (y * 8192 + (cb - 2048) * Lb + (cr - 2048) * Lr + 65536) >> 17 becomes
          // (y' * 8192 + K + cb' * Lb + cr' * Lr) >> 17 with one constant K for all three channels
          int rr[8], gg[8], bb[8];
#pragma unroll
          for (int x = 0; x < 8; x++) {
            const int yk = luma13(yv[l * 8 + x]); // (level shift and rounding are inside: LUMA_FOLD_R2)
            rr[x] = mad24(ur[x], L_CR_R, yk); // still scaled by 2^17
            gg[x] = mad24(ur[x], -L_CR_G, mad24(ub[x], -L_CB_G, yk));
            bb[x] = mad24(ub[x], L_CB_B, yk);
          }
          if (WINDOW_OUT && PLANAR_OUT) store_planar8_line(o.out_frame, pb, o.line_off(l, a), rr, gg, bb, o.fast_store, o.npx, wc.px0);
          else if (WINDOW_OUT) store_rgb8_line<STORE24_3X8>(o.out_frame, o.line_off(l, a), rr, gg, bb, o.fast_store, o.npx, wc.px0);
          else if (PLANAR_OUT) store_planar8_line(o.out_frame, pb, o.line_off(l, a), rr, gg, bb, o.fast_store, o.npx);
          else store_rgb8_line<STORE24_3X8>(o.out_frame, o.line_off(l, a), rr, gg, bb, o.fast_store, o.npx);
        } else {
          uint8_t *dst = o.out_frame + o.line_off(l, a);
          unsigned px[24];
#pragma unroll
          for (int x = 0; x < 8; x++) {
            int r, g, b;
            ycc_to_rgb<false>(yv[l * 8 + x], ub[x], ur[x], r, g, b);
            px[3 * x] = r; px[3 * x + 1] = g; px[3 * x + 2] = b;
          }
          if (WINDOW_OUT && PLANAR_OUT) {
            store_planar8_bytes(o.out_frame, pb, o.line_off(l, a), px, o.fast_store, o.npx, wc.px0);
          } else if (PLANAR_OUT) {
            store_planar8_bytes(o.out_frame, pb, o.line_off(l, a), px, o.fast_store, o.npx);
          } else if (o.fast_store) {
            unsigned w[6];
#pragma unroll
            for (int i = 0; i < 6; i++) w[i] = px[4 * i] | (px[4 * i + 1] << 8) | (px[4 * i + 2] << 16) | (px[4 * i + 3] << 24);
            store24_3x8(dst, w);
          } else {
#pragma unroll
            for (int x = 0; x < 8; x++)
              if (WINDOW_OUT ? x >= wc.px0 && x < o.npx : x < o.npx) {
                dst[3 * x] = (uint8_t)px[3 * x]; dst[3 * x + 1] = (uint8_t)px[3 * x + 1]; dst[3 * x + 2] = (uint8_t)px[3 * x + 2];
              }
          }
        }
      }
    }
    // slide the three-line window
#pragma unroll
    for (int j = 0; j < 6; j++) { cbT[j] = cbC[j]; cbC[j] = cbB[j]; crT[j] = crC[j]; crC[j] = crB[j]; }
  }
}
