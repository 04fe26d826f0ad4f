// fused420p_kernel.inc -- the text of fused420p_kernel, included by kernels.hip (see there: once in mij, once in mij::planar, and in
// mij::window and mij::window::planar, where WINDOW_OUT is true: the crop windows of a list)
// D2: the second pass of every transform on v_dot2 (idct_columns_dot2; admitted by the host where sum |c| q <= 1476 in all three
// components: plan_reconstruct in capi.cpp)
// The uniform flavours (one table set for the launch, !QDEV && !RAGGED) run the lean transforms: three-operand dot products and,
// with D2, no shifts behind the first pass (dequant_idct16 in kernels.hip).  The per-frame-table and list flavours keep the
// helpers every other kernel has.
template <int MINW, bool QDEV, bool D2 = false, bool RAGGED = false>
__global__ __launch_bounds__(F420_THREADS, MINW) void fused420p_kernel(Fused420Args a)
{
  static_assert(!RAGGED || QDEV, "ragged launches: per-frame tables");
  static_assert(!PLANAR_OUT || RAGGED, "planar output: the ragged flavours");
  static_assert(!WINDOW_OUT || RAGGED, "crop windows: the ragged flavours");
  constexpr bool LEAN = !QDEV && !RAGGED;
  __shared__ __attribute__((aligned(16))) unsigned cpair[F420_CROWS * F420_CPITCH];
  __shared__ __attribute__((aligned(16))) u32x4 stage_all[4][128];

  PlanarBases pb{};
  WindowBox wb{};
  const TileCtx t = WINDOW_OUT ? tile_enter_window<PLANAR_OUT>(a, stage_all, pb, wb) : PLANAR_OUT ? tile_enter_planar(a, stage_all, pb) : RAGGED ? tile_enter_ragged(a, stage_all) : tile_enter(a, stage_all);
  if (t.padding) return;
  const int tid = t.tid, lane = t.lane, wave = t.wave, frame = t.frame, tx = t.tx, ty = t.ty;
  u32x4 *stage = t.stage;
  const int16_t *__restrict__ coef = t.coef;
  // the luma blocks of phase B are requested early: their latency hides behind phase A's transform (see F420P_MINW)
  u32x4 yraw[8];

  // ------------------------------------------------------------------ phase A: chroma -> LDS halves
  // Of the tile's 10 x 10 chroma blocks per component the filters read the 8 x 8 interior in full, but of the ring around it only
  // the column, the line or the single sample that touches the interior.  The four waves take four roles (wave-uniform: no
  // divergence between the transforms): the interior of Cb, the interior of Cr, the ring of Cb, the ring of Cr.  The roles rotate
  // with the workgroup so that every SIMD of a CU sees the heavier interior waves and the lighter ring waves alike.
  // LDS line pr <-> chroma line ty * 64 + pr - 1, column pc <-> chroma column tx * 64 + pc - 4.
  {
    const int role = (wave + (int)((blockIdx.x >> 3) + (blockIdx.x >> 8))) & 3; // (>> 3: workgroups of one XCD; >> 8: of one CU, roughly)
    const int comp = role & 1; // 0 = Cb (low halves), 1 = Cr (high halves); wave-uniform
    const int16_t *__restrict__ plane = coef + (comp ? a.off_cr : a.off_cb);
    const char *pbase = reinterpret_cast<const char *>(plane) + (lane & 7) * 16;
    const int *q = frame_deltas<QDEV>(a, frame, 1 + comp);
    short *cp = reinterpret_cast<short *>(cpair) + comp; // this component's half of every dword
    const int gx0 = tx * 8, gy0 = ty * 8;                // the interior's first block
    const int nb = lane >> 3;
    if (role < 2) {
      // interior: local block n = (lane >> 3) + 8 m is column lane >> 3 of row m -- one load covers a row's 1 KB
      u32x4 rows[8];
      const unsigned xoff = (unsigned)min(gx0 + nb, a.bw_c - 1) * 128u;
      fetch_blocks(rows, stage, lane, [&](int m) -> const u32x4 * {
        const int yy = min(gy0 + m, a.bh_c - 1);
        return reinterpret_cast<const u32x4 *>(pbase + ((unsigned)(yy * a.bw_c) * 128u + xoff));
      });
      load_tile_blocks(yraw, t, coef + a.off_y, a.bw_y, a.bh_y);
      const int cbx = lane & 7, cby = lane >> 3;
      if (gx0 + cbx < a.bw_c && gy0 + cby < a.bh_c) {
        int at = (8 * cby + 1) * F420_CPITCH + 8 * cbx + 4; // the lane's first sample
        // (per-frame tables: the index is formed here and held across the transform.  The build then allocates the 133 registers
        // this instantiation had before the ring was split off, the count tests/test_ragged_batch.py holds it to; 132 otherwise.
        // Three workgroups per CU either way.)
        // (the lean flavours: without the accumulator copies both come out at 126 registers, and
        // tests/test_ragged_batch.py::test_ragged_flavours_cost_the_existing_kernels_nothing holds them to the 127 and -- D2 -- 128 of
        // the build it was written against.  The index held across the transform is the 127th, its column part held apart the
        // 128th.  Four waves per SIMD from 103 to 128 registers: nothing is lost.)
        int at_col = 0;
        if (LEAN && D2) { at_col = 8 * cbx + 4; at -= at_col; asm volatile("" : "+v"(at_col)); }
        if (QDEV || LEAN) asm volatile("" : "+v"(at));
        int v[64];
        dequant_idct_sparse<!QDEV, false, D2, LEAN>(rows, q, v);
        short *dst = cp + 2 * (at + at_col); // one base per lane: the 64 stores take immediate offsets
#pragma unroll
        for (int r = 0; r < 8; r++)
#pragma unroll
          for (int x = 0; x < 8; x++) dst[2 * (r * F420_CPITCH + x)] = (short)v[r * 8 + x];
      }
    } else {
      // ring.  Columns and corners, lane-owns-block: block n = 0..15 is the left (n even) or right (n odd) neighbour of interior
      // row n >> 1; n = 16..19 are the corners (bit 0: right, bit 1: below).  Lines, on the fetching lanes: the blocks above and
      // below interior column lane >> 3 (dequant_idct_line8).  All five requests leave before the luma request.
      auto chunk = [&](int gx, int gy) -> u32x4 {
        const int xx = min(max(gx, 0), a.bw_c - 1), yy = min(max(gy, 0), a.bh_c - 1);
        return *reinterpret_cast<const u32x4 *>(pbase + (unsigned)((yy * a.bw_c + xx) * 128));
      };
      const int gxs = (nb & 1) ? gx0 + 8 : gx0 - 1;
      const u32x4 side0 = chunk(gxs, gy0 + (nb >> 1)), side1 = chunk(gxs, gy0 + 4 + (nb >> 1));
      const u32x4 corner = chunk(gxs, (nb & 2) ? gy0 + 8 : gy0 - 1);
      const u32x4 above = chunk(gx0 + nb, gy0 - 1), below = chunk(gx0 + nb, gy0 + 8);
      load_tile_blocks(yraw, t, coef + a.off_y, a.bw_y, a.bh_y);
      {
        u32x4 rows[8];
        const int k = lane & 7;
        stage[nb * 8 + (k ^ nb)] = side0;
        stage[(nb + 8) * 8 + (k ^ nb)] = side1;
        __builtin_amdgcn_wave_barrier();
        if (lane < 16) {
#pragma unroll
          for (int r = 0; r < 8; r++) rows[r] = stage[lane * 8 + (r ^ (lane & 7))];
        }
        __builtin_amdgcn_wave_barrier();
        stage[nb * 8 + (k ^ nb)] = corner; // (blocks 4..7 repeat 0..3 and are not read)
        __builtin_amdgcn_wave_barrier();
        if (lane >= 16 && lane < 20) {
#pragma unroll
          for (int r = 0; r < 8; r++) rows[r] = stage[(lane - 16) * 8 + (r ^ (lane - 16))];
        }
        __builtin_amdgcn_wave_barrier();
        const bool right = lane & 1, is_corner = lane >= 16, low = lane & 2;
        const int gx = right ? gx0 + 8 : gx0 - 1, gy = is_corner ? (low ? gy0 + 8 : gy0 - 1) : gy0 + (lane >> 1);
        if (lane < 20 && gx >= 0 && gx < a.bw_c && gy >= 0 && gy < a.bh_c) {
          int col[8];
          dequant_idct_column(rows, q, !right, col); // left neighbour: its last column, right one: its first
          const int pc = right ? 68 : 3;
          if (is_corner) {
            cp[2 * ((low ? F420_CROWS - 1 : 0) * F420_CPITCH + pc)] = (short)(low ? col[0] : col[7]);
          } else {
            short *dst = cp + 2 * ((8 * (lane >> 1) + 1) * F420_CPITCH + pc);
#pragma unroll
            for (int r = 0; r < 8; r++) dst[2 * r * F420_CPITCH] = (short)col[r];
          }
        }
      }
      {
        constexpr int W[8] = {512, FIX9(1.501321110) - FIX9(0.899976223) - FIX9(0.390180644) + FIX9(1.175875602), FIX9(0.541196100) + FIX9(0.765366865),
                              FIX9(1.175875602), 512, FIX9(1.175875602) - FIX9(0.390180644), FIX9(0.541196100), FIX9(1.175875602) - FIX9(0.899976223)};
        const int k = lane & 7;
        // the deltas of row k, per lane: read from the kernel argument segment itself (see fused440_kernel)
        typedef const __attribute__((address_space(4))) int kernarg_int;
        int qrow[8];
        if (QDEV) {
          const int *qk = q + k * 8;
#pragma unroll
          for (int i = 0; i < 8; i++) qrow[i] = qk[i];
        } else {
          kernarg_int *qk = (kernarg_int *)__builtin_amdgcn_kernarg_segment_ptr() + (offsetof(Fused420Args, q) / sizeof(int) + (1 + comp) * QROW + k * 8);
#pragma unroll
          for (int i = 0; i < 8; i++) qrow[i] = qk[i];
        }
        const int weight = W[k];
        int line[8];
        short *dst = cp + 2 * (8 * nb + 4 + k);
        const bool col_ok = gx0 + nb < a.bw_c;
        auto mine = [&](const int (&l)[8]) { // line[k] without a register-indexed access
          const int a01 = (k & 1) ? l[1] : l[0], a23 = (k & 1) ? l[3] : l[2], a45 = (k & 1) ? l[5] : l[4], a67 = (k & 1) ? l[7] : l[6];
          const int lo = (k & 2) ? a23 : a01, hi = (k & 2) ? a67 : a45;
          return (short)((k & 4) ? hi : lo);
        };
        dequant_idct_line8(above, qrow, (k & 1) ? -weight : weight, line); // the block above: its last line (even - odd)
        if (col_ok && gy0 > 0) dst[0] = mine(line);
        dequant_idct_line8(below, qrow, weight, line); // the block below: its first line (even + odd)
        if (col_ok && gy0 + 8 < a.bh_c) dst[2 * (F420_CROWS - 1) * F420_CPITCH] = mine(line);
      }
    }
  }
  __syncthreads();

  // ------------------------------------------------------------------ edge fix-up (uniform branch)
  {
    const int last_col = a.cw - 1 - tx * 64; // last valid chroma column, tile-relative
    const int last_row = a.ch - 1 - ty * 64;
    const bool edge = (tx == 0) | (ty == 0) | (last_col < 64) | (last_row < 64);
    if (edge) {
      if (tid < F420_CROWS) { // one thread per stored line: replicate columns
        unsigned *p = cpair + tid * F420_CPITCH;
        if (tx == 0) p[3] = p[4];
        if (last_col < 64) {
          const unsigned v = p[last_col + 4];
          for (int pc = last_col + 5; pc <= 68; pc++) p[pc] = v;
        }
      }
      __syncthreads();
      if (tid < F420_CROWS) { // one thread per stored column: replicate lines
        auto at = [&](int pr) -> unsigned & { return cpair[pr * F420_CPITCH + 3 + tid]; };
        if (ty == 0) at(0) = at(1);
        if (last_row < 64) {
          const unsigned v = at(last_row + 1);
          for (int pr = last_row + 2; pr < F420_CROWS; pr++) at(pr) = v;
        }
      }
      __syncthreads();
    }
  }

  // ------------------------------------------------------------------ phase B: luma, upsampling, colour
  u32x4 rows[8];
  transpose_blocks(rows, stage, lane, yraw);
  WindowClip wc{};
  const BlockOut o = WINDOW_OUT ? block_out_window<PLANAR_OUT ? 1 : 3>(a, t, wb, wc) : block_out<PLANAR_OUT ? 1 : 3>(a, t);
  if (o.outside) return; // no barrier below this point
  int yv[64];
  dequant_idct_sparse<!QDEV, true, D2, LEAN>(rows, frame_deltas<QDEV>(a, frame, 0), yv, 0, LUMA_FOLD_R2);

  const int bx = o.bx, by = o.by, npx = o.npx, nln = o.nln;
  uint8_t *__restrict__ out_frame = o.out_frame;
  const unsigned out_off = o.out_off;
  const bool fast_store = o.fast_store;
  // chroma window of this block: lines pr = 4 by + m (+0 top, +1 cur, +2 bot), columns pc = 4 bx + 3 + j
  const unsigned *c_base = cpair + (4 * by) * F420_CPITCH + 4 * bx;

  // Blocks that lie wholly inside the picture -- all of them, for every wave but those on the right and bottom edges -- take a
  // copy of the loop without the per-line exec masks (wave-uniform choice: one ballot)
  // (a third copy, FULL with every lane active, for frames whose lines do not all start on a dword: store24_nt_shifted)
  const unsigned base_lo = (unsigned)(uintptr_t)out_frame;
  auto lines = [&](auto full_tag, auto shift_tag, auto staged_tag) {
    constexpr bool FULL = decltype(full_tag)::value, SHIFTED = decltype(shift_tag)::value, STAGED = decltype(staged_tag)::value;
    // STAGED: whole waves of whole blocks send a line's pixels through the wave's (idle) fetch staging buffer -- sixteen 24-byte
    // pieces per block row in, 96 chunks of 16 contiguous bytes out -- so that every store instruction writes whole aligned runs of
    // the four 384-byte line segments instead of 16 and then 8 bytes of every lane's 24: tools/microbench/stream_ceiling --staged puts
    // the kernel's access pattern at 0.74-0.755 of 8 TB/s with such stores, 0.71-0.72 with the pieces (profiles/r06/staged_stores.txt).
    // Chunk c of the wave's 96 per line is bytes 16 (c % 24) .. of block row c / 24's segment; lanes 0..31 own a second one
    unsigned so0 = 0, so1 = 0;
    if (STAGED) {
      const unsigned wave_off = (unsigned)((ty * F420_TILE_BLOCKS + wave * 4) * 8) * (unsigned)a.row_stride + (unsigned)(tx * F420_TILE_BLOCKS * 8) * 3u;
      const unsigned c1 = 64u + (unsigned)lane;
      so0 = wave_off + ((unsigned)lane / 24u) * 8u * (unsigned)a.row_stride + ((unsigned)lane % 24u) * 16u;
      so1 = wave_off + (c1 / 24u) * 8u * (unsigned)a.row_stride + (c1 % 24u) * 16u;
    }
    unsigned cT[6], cC[6], cB[6];
    load6(c_base, cT);
    load6(c_base + F420_CPITCH, cC);
#pragma unroll
    for (int m = 0; m < 4; m++) {
      load6(c_base + (m + 2) * F420_CPITCH, cB);
      // 3 * centre + rounding, both roundings, for the two lines that share the centre line
      unsigned w1[6], w2[6];
#pragma unroll
      for (int j = 0; j < 6; j++) { w1[j] = centre3_pk(cC[j], 1); w2[j] = centre3_pk(cC[j], 2); }
#pragma unroll
      for (int half = 0; half < 2; half++) {
        const int l = 2 * m + half;
        // vertical filter (upsampler.cpp:149-165), both components at once
        unsigned v[6];
#pragma unroll
        for (int j = 0; j < 6; j++) v[j] = tap_sum_pk(half ? cB[j] : cT[j], ((j & 1) ^ half) ? w1[j] : w2[j]);
        // horizontal filter in place (upsampler.cpp:291-303); src[k] = v[k + 1]
        unsigned u[8];
        u[7] = tap13_pk(v[5], v[4], 1);
        u[6] = tap13_pk(v[3], v[4], 2);
        u[5] = tap13_pk(v[4], v[3], 1);
        u[4] = tap13_pk(v[2], v[3], 2);
        u[3] = tap13_pk(v[3], v[2], 1);
        u[2] = tap13_pk(v[1], v[2], 2);
        u[1] = tap13_pk(u[2], v[1], 1); // src[1] has already been overwritten by out[2]
        u[0] = tap13_pk(v[0], v[1], 2);
        if (FULL || (WINDOW_OUT ? l >= wc.ln0 && l < nln : l < nln)) {
          int rr[8], gg[8], bb[8];
#pragma unroll
          for (int x = 0; x < 8; x++) {
            const int yk = luma13(yv[l * 8 + x]); // (level shift and rounding are inside: LUMA_FOLD_R2)
            rr[x] = mad16_hi(u[x], L_CR_R, yk); // still scaled by 2^17
            bb[x] = mad16_lo(u[x], L_CB_B, yk);
            gg[x] = dot2_16(u[x], -L_CB_G, -L_CR_G, yk);
          }
          if (PLANAR_OUT) {
            // (planar: three 8-byte stores per line whatever the planes' alignment -- FULL only drops the per-line masks)
            if (WINDOW_OUT) store_planar8_line(out_frame, pb, out_off + (unsigned)l * (unsigned)a.row_stride, rr, gg, bb, FULL || fast_store, npx, wc.px0);
            else store_planar8_line(out_frame, pb, out_off + (unsigned)l * (unsigned)a.row_stride, rr, gg, bb, FULL || fast_store, npx);
          } else if (FULL || fast_store) {
            unsigned w[6];
            rgb_shift17_sat_pack(rr, gg, bb, w);
            const unsigned off = out_off + (unsigned)l * (unsigned)a.row_stride;
            const int m = SHIFTED ? (int)__builtin_amdgcn_readfirstlane((base_lo + (unsigned)l * (unsigned)a.row_stride) & 3u) : 0;
            if (STAGED) {
              unsigned *sw = reinterpret_cast<unsigned *>(stage);
              u32x2 *pw = reinterpret_cast<u32x2 *>(sw + lane * 6);
              pw[0] = u32x2{w[0], w[1]}; pw[1] = u32x2{w[2], w[3]}; pw[2] = u32x2{w[4], w[5]};
              __builtin_amdgcn_wave_barrier();
              const u32x4 v0 = *reinterpret_cast<const u32x4 *>(sw + lane * 4);
              const u32x4 v1 = *reinterpret_cast<const u32x4 *>(sw + ((lane & 31) + 64) * 4);
              __builtin_amdgcn_wave_barrier();
              store16_nt(out_frame, so0 + (unsigned)l * (unsigned)a.row_stride, v0);
              if (lane < 32) store16_nt(out_frame, so1 + (unsigned)l * (unsigned)a.row_stride, v1);
            }
            else if (SHIFTED && m) store24_nt_shifted(out_frame, off, w, bx, m);
            else if (SHIFTED) store24_nt<false>(out_frame, off, w);
            else store24_nt(out_frame, off, w);
          } else {
            if (WINDOW_OUT) store_rgb8_partial(out_frame + (out_off + (unsigned)l * (unsigned)a.row_stride), rr, gg, bb, npx, wc.px0);
            else store_rgb8_partial(out_frame + (out_off + (unsigned)l * (unsigned)a.row_stride), rr, gg, bb, npx);
          }
        }
      }
      // slide the three-line window
#pragma unroll
      for (int j = 0; j < 6; j++) { cT[j] = cC[j]; cC[j] = cB[j]; }
    }
  };
  // (the window flavours: wholly inside the WINDOW -- the interior of a crop runs the code the interior of a picture runs)
  const bool whole = WINDOW_OUT ? __builtin_amdgcn_ballot_w64(npx != 8 || nln != 8 || (wc.px0 | wc.ln0) != 0) == 0 : __builtin_amdgcn_ballot_w64(npx != 8 || nln != 8) == 0;
  if (PLANAR_OUT) {
    if (whole) lines(std::true_type{}, std::false_type{}, std::false_type{});
    else lines(std::false_type{}, std::false_type{}, std::false_type{});
  }
  else if (whole && ((base_lo | (unsigned)a.row_stride) & 3u) && __builtin_amdgcn_ballot_w64(true) == ~0ull) lines(std::true_type{}, std::true_type{}, std::false_type{});
  else if (whole && __builtin_amdgcn_ballot_w64(true) == ~0ull) lines(std::true_type{}, std::false_type{}, std::true_type{});
  else if (whole) lines(std::true_type{}, std::false_type{}, std::false_type{});
  else lines(std::false_type{}, std::false_type{}, std::false_type{});
}
