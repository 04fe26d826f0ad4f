// block_decode.hpp -- the bit reader and the per-symbol and per-block Huffman decoders of the host decoder, header-only and
// `static inline` so that every block loop inlines them.  Included by host_decoder.cpp and speculative_decode.cpp only.
#ifndef MIJ_BLOCK_DECODE_HPP
#define MIJ_BLOCK_DECODE_HPP

#include "host_decoder.hpp"

#include <stdlib.h>
#include <string.h>

#include <algorithm>
#if defined(__x86_64__)
#include <immintrin.h>
#endif

namespace mij {

// ------------------------------------------------------------------------------------------------
// bit reader (io/bitstream.cpp:56-118, byte-stuffing flavour): 64-bit left-aligned window; FF00 -> FF;
// at any other FFxx (or the end of the interval) the reader parks and supplies zero bits.
// ------------------------------------------------------------------------------------------------
struct BitReader {
  const uint8_t *p, *end;
  uint64_t acc = 0;
  int n = 0;
  bool parked = false;
  uint32_t stuffed = 0; // FF 00 pairs taken so far (the speculative decoder needs positions in the unstuffed stream)
  int phantom = 0;      // zero bits supplied after parking that are still in the buffer (upper bound: never drained first)

  BitReader(const uint8_t *b, const uint8_t *e) : p(b), end(e) {}

  inline void refill()
  {
    if (!parked && end - p >= 8) {
      uint64_t v;
      memcpy(&v, p, 8);
      // any 0xFF byte among the eight?  haszero(~v)
      const uint64_t x = ~v;
      if (!((x - 0x0101010101010101ull) & ~x & 0x8080808080808080ull)) {
        const int k = (64 - n) >> 3; // whole bytes that fit
        v = __builtin_bswap64(v);
        if (k < 8) v &= ~0ull << (64 - 8 * k);
        acc |= n < 64 ? (v >> n) : 0;
        p += k;
        n += 8 * k;
        return;
      }
    }
    while (n <= 56) {
      uint64_t c = 0;
      if (!parked) {
        if (p >= end) parked = true;
        else if (*p == 0xff) {
          if (p + 1 < end && p[1] == 0x00) { c = 0xff; p += 2; stuffed++; }
          else parked = true;
        } else c = *p++;
      }
      acc |= c << (56 - n);
      n += 8;
      if (parked) phantom += 8;
    }
  }
  inline int real_bits() const { return n - phantom; } // unread bits that came from the stream
  inline uint32_t peek(int k) const { return (uint32_t)(acc >> (64 - k)); }
  inline void skip(int k) { acc <<= k; n -= k; }
};

static inline int decode_symbol(BitReader &b, const HuffTable &h)
{
  const uint16_t e = h.fast[b.peek(HuffTable::LOOKAHEAD)];
  if (e) {
    b.skip(e >> 8);
    return e & 0xff;
  }
  const int32_t code16 = (int32_t)b.peek(16);
  for (int l = HuffTable::LOOKAHEAD + 1; l <= 16; l++) {
    const int32_t code = code16 >> (16 - l);
    if (code <= h.maxcode[l]) {
      b.skip(l);
      return h.values[(code + h.valoff[l]) & 0xff];
    }
  }
  return -1;
}

static inline int receive_extend(BitReader &b, int s)
{
  int v = (int)b.peek(s);
  b.skip(s);
  if (v < (1 << (s - 1))) v += (int)((~0u) << s) + 1; // sequentialscan.cpp:690-692
  return v;
}

// sequentialscan.cpp:678-773 (ScanStart 0, ScanStop 63, no point transform).  Returns 0 or an error.
// `qsum` accumulates sum |c| * q for the range check that admits the fast kernel arithmetic.
static inline int decode_block(BitReader &b, const HuffTable &dc, const HuffTable &ac, int &pred, int16_t *blk,
                               const uint16_t *q, const uint8_t *zz, uint32_t &qmax)
{
  memset(blk, 0, 128);
  if (b.n < 32) b.refill();
  int s = decode_symbol(b, dc);
  if (s < 0 || s > 15) return MIJPEG_ERR_MALFORMED_STREAM; // ":686 DC coefficient decoding out of sync"
  if (s) pred += receive_extend(b, s);
  if (pred != (int16_t)pred) return MIJPEG_ERR_OVERFLOW_PARAMETER; // beyond the int16 coefficient store
  blk[0] = (int16_t)pred;
  uint32_t qsum = (uint32_t)(pred < 0 ? -pred : pred) * q[0];
  int k = 1;
  do {
    if (b.n < 32) b.refill();
    const int rs = decode_symbol(b, ac);
    if (rs < 0) return MIJPEG_ERR_MALFORMED_STREAM;
    const int r = rs >> 4;
    s = rs & 15;
    if (s == 0) {
      if (r == 15) { k += 16; continue; } // ZRL
      if (r == 0) break;                  // EOB
      return MIJPEG_ERR_MALFORMED_STREAM; // EOB runs only exist in progressive scans (:747-750)
    }
    k += r;
    const int v = receive_extend(b, s);
    if (k >= 64) return MIJPEG_ERR_MALFORMED_STREAM; // ":763 AC coefficient decoding out of sync"
    const int pos = zz[k];
    blk[pos] = (int16_t)v;
    qsum = std::min<uint32_t>(qsum + (uint32_t)(v < 0 ? -v : v) * q[pos], 0x7fffffffu); // saturating: both terms < 2^31
    k++;
  } while (k <= 63);
  if (qsum > qmax) qmax = qsum;
  return 0;
}

// Progressive first passes (sequentialscan.cpp:678-773 with spectral selection, point transform and EOB runs).
// T = int16_t (the store the kernels read) or int32_t (JPEG XT residual frames with hidden bits: 12 + up to 4 bits).
template <class T>
static inline int decode_block_first(BitReader &b, const HuffTable &dc, const HuffTable &ac, int &pred, T *blk,
                                     const uint8_t *zz, int ss, int se, int al, int &skip)
{
  if (ss == 0) {
    if (b.n < 32) b.refill();
    const int s = decode_symbol(b, dc);
    if (s < 0 || s > 15) return MIJPEG_ERR_MALFORMED_STREAM;
    if (s) pred += receive_extend(b, s);
    const int v = (int)((unsigned)pred << al);
    if (v != (T)v) return MIJPEG_ERR_OVERFLOW_PARAMETER;
    blk[0] = (T)v;
  }
  if (se) {
    if (skip > 0) { skip--; return 0; }
    int k = ss ? ss : 1;
    do {
      if (b.n < 32) b.refill();
      const int rs = decode_symbol(b, ac);
      if (rs < 0) return MIJPEG_ERR_MALFORMED_STREAM;
      const int r = rs >> 4, s = rs & 15;
      if (s == 0) {
        if (r == 15) { k += 16; continue; }
        skip = 1 << r;
        if (r) { skip |= (int)b.peek(r); b.skip(r); }
        skip--;
        break;
      }
      k += r;
      const int v = (int)((unsigned)receive_extend(b, s) << al);
      if (k >= 64) return MIJPEG_ERR_MALFORMED_STREAM;
      if (v != (T)v) return MIJPEG_ERR_OVERFLOW_PARAMETER;
      blk[zz[k]] = (T)v;
      k++;
    } while (k <= se);
  }
  return 0;
}

// Successive approximation refinement scans: codestream/refinementscan.cpp:584-700 (T.81 G.1.2.3).
template <class T>
static inline int decode_block_refine(BitReader &b, const HuffTable &ac, T *blk, const uint8_t *zz, int ss, int se, int al,
                                      int &skip)
{
  if (b.n < 32) b.refill();
  if (ss == 0) {
    blk[0] = (T)(blk[0] | (int)(b.peek(1) << al));
    b.skip(1);
  }
  if (se) {
    int k = ss, run = 0, s = 0;
    bool at_start = false, overflow = false;
    if (skip > 0) { run = se - ss + 1; skip--; }
    else { k--; at_start = true; }
    do {
      if (!at_start) {
        const int data = blk[zz[k]];
        if (data) {
          // a correction bit (G.1.2.3): one step away from zero or nothing.  No branch on the bit -- it is a coin toss, and in
          // the hidden refinement scans of a JPEG XT residual most coefficients of a block take this path
          if (b.n < 8) b.refill();
          const int bit = (int)b.peek(1);
          b.skip(1);
          const int nv = data + ((((data >> 31) | 1) * (1 << al)) & -bit);
          overflow |= nv != (T)nv; // beyond the coefficient store
          blk[zz[k]] = (T)nv;
          continue;
        }
        if (run) { run--; continue; }
        blk[zz[k]] = (T)(s * (1 << al));
        if (k == se) break;
      }
      at_start = false;
      if (b.n < 32) b.refill();
      const int rs = decode_symbol(b, ac);
      if (rs < 0) return MIJPEG_ERR_MALFORMED_STREAM;
      const int r = rs >> 4;
      s = rs & 15;
      if (s == 0) {
        if (r == 15) run = r;
        else {
          skip = 1 << r;
          if (r) { skip |= (int)b.peek(r); b.skip(r); }
          skip--;
          run = se - k + 1;
        }
      } else {
        if (s != 1) return MIJPEG_ERR_MALFORMED_STREAM; // the reference warns and decodes on; reported here
        const int sign = (int)b.peek(1);
        b.skip(1);
        if (!sign) s = -s;
        run = r;
      }
    } while (++k <= se);
    if (overflow) return MIJPEG_ERR_OVERFLOW_PARAMETER;
  }
  return 0;
}

// The same AC refinement pass with the block's history as bit masks (x86-64 with BMI2 + AVX2; picked at run time).
// A refinement scan spends its time walking all 63 positions of every block: one correction bit for every coefficient that
// is already non-zero, a Huffman symbol only where a new coefficient appears -- in the hidden refinement scans of a JPEG XT
// residual (the low bits of noise-like coefficients) eight million position visits per scan of a 4K frame, one unpredictable
// branch each.  Here the block's non-zero pattern is one 64-bit mask in reversed zigzag order (bit 63 - k = position k):
//   * the target of a symbol (run r, then place) is the (r + 1)-th zero position from the cursor: popcount + PDEP select;
//   * the correction bits of all non-zero positions passed on the way are read in ONE piece -- they are contiguous in the
//     stream, between this symbol's sign bit and the next symbol -- and PDEP spreads them over those positions (the first bit
//     read belongs to the lowest position = the highest mask bit, which is where PDEP puts the top source bit);
//   * the corrections of the whole block are applied at the end, eight coefficients per instruction.
// Same bits, same reads in the same order as decode_block_refine above (tests/test_host_decoder.py runs both on the same scans).
#if defined(__x86_64__)
struct RefineMasks {
  uint64_t to_rev[8][256]; // natural-order byte i (bit j = coefficient 8 i + j) -> reversed zigzag mask
  uint64_t to_nat[8][256]; // reversed zigzag byte i (bit j = position 63 - (8 i + j)) -> natural-order mask
  uint64_t to_zz[8][256];  // natural-order byte i -> zigzag mask (bit k = position k): what parse_block_refine_ac works on
  uint64_t to_ras[8][256]; // zigzag byte i (bit j = position 8 i + j) -> natural-order mask
};
static const RefineMasks &refine_masks()
{
  static const RefineMasks t = [] {
    RefineMasks m;
    const uint8_t *zz = scan_order();
    int pos_of[64];
    for (int k = 0; k < 64; k++) pos_of[zz[k]] = k;
    for (int i = 0; i < 8; i++)
      for (int v = 0; v < 256; v++) {
        uint64_t a = 0, c = 0, z = 0, r = 0;
        for (int j = 0; j < 8; j++)
          if (v & (1 << j)) {
            a |= 1ull << (63 - pos_of[8 * i + j]);
            c |= 1ull << zz[63 - (8 * i + j)];
            z |= 1ull << pos_of[8 * i + j];
            r |= 1ull << zz[8 * i + j];
          }
        m.to_rev[i][v] = a;
        m.to_nat[i][v] = c;
        m.to_zz[i][v] = z;
        m.to_ras[i][v] = r;
      }
    return m;
  }();
  return t;
}

// (these read the WHOLE block, the lanes of other bands included, which their own scans may be writing at this moment; what is
// read there is masked away by the caller -- hence no_sanitize for the thread sanitizer build, tools/tsan_host.sh)
__attribute__((target("avx2,bmi2,popcnt,lzcnt"), no_sanitize("thread"))) static inline uint64_t nonzero_mask(const int32_t *blk)
{
  const __m256i zero = _mm256_setzero_si256();
  uint64_t m = 0;
  for (int i = 0; i < 8; i++)
    m |= (uint64_t)(uint8_t)~_mm256_movemask_ps(_mm256_castsi256_ps(_mm256_cmpeq_epi32(_mm256_loadu_si256((const __m256i *)(blk + 8 * i)), zero))) << (8 * i);
  return m;
}
__attribute__((target("avx2,bmi2,popcnt,lzcnt"), no_sanitize("thread"))) static inline uint64_t nonzero_mask(const int16_t *blk)
{
  const __m128i zero = _mm_setzero_si128();
  uint64_t m = 0;
  for (int i = 0; i < 8; i++) {
    const __m128i e = _mm_cmpeq_epi16(_mm_loadu_si128((const __m128i *)(blk + 8 * i)), zero);
    m |= (uint64_t)(uint8_t)~_mm_movemask_epi8(_mm_packs_epi16(e, e)) << (8 * i);
  }
  return m;
}
// coefficient += (sign of coefficient) << al where the mask says so; false: a 16-bit store overflowed.
// Only the coefficients the mask names are WRITTEN: scans over other spectral bands of the same component (and the DC scans)
// run side by side with this one and own the rest of the block.
__attribute__((target("avx2,bmi2,popcnt,lzcnt"))) static inline bool apply_corrections(int32_t *blk, uint64_t nat, int al)
{
  const __m256i bitsel = _mm256_setr_epi32(1, 2, 4, 8, 16, 32, 64, 128), one = _mm256_set1_epi32(1);
  for (int i = 0; i < 8; i++) {
    const int byte = (int)((nat >> (8 * i)) & 255);
    if (!byte) continue;
    const __m256i lanes = _mm256_cmpeq_epi32(_mm256_and_si256(_mm256_set1_epi32(byte), bitsel), bitsel);
    __m256i v = _mm256_maskload_epi32((const int *)(blk + 8 * i), lanes);
    const __m256i step = _mm256_sll_epi32(_mm256_or_si256(_mm256_srai_epi32(v, 31), one), _mm_cvtsi32_si128(al));
    v = _mm256_add_epi32(v, step);
    _mm256_maskstore_epi32((int *)(blk + 8 * i), lanes, v);
  }
  return true;
}
static inline bool apply_corrections(int16_t *blk, uint64_t nat, int al)
{
  // (16-bit stores: ordinary progressive pictures and legacy frames with hidden bits, few non-zero coefficients per block)
  bool ok = true;
  while (nat) {
    const int i = __builtin_ctzll(nat);
    nat &= nat - 1;
    const int v = blk[i], nv = v + ((v >> 31) | 1) * (1 << al);
    ok = ok && nv == (int16_t)nv;
    blk[i] = (int16_t)nv;
  }
  return ok;
}

// the correction bits of the non-zero positions in seg, read in stream order and spread over those positions
__attribute__((target("avx2,bmi2,popcnt,lzcnt"))) static inline uint64_t refine_correction_bits(BitReader &b, uint64_t seg)
{
  int left = (int)_mm_popcnt_u64(seg);
  if (!left) return 0;
  uint64_t v = 0;
  while (left > 0) {
    const int c = left < 32 ? left : 32;
    if (b.n < c) b.refill();
    v = (v << c) | b.peek(c);
    b.skip(c);
    left -= c;
  }
  return _pdep_u64(v, seg);
}

template <class T>
__attribute__((target("avx2,bmi2,popcnt,lzcnt"))) static int decode_block_refine_ac_masks(BitReader &b, const HuffTable &ac, T *blk, const uint8_t *zz, int ss,
                                                                                      int se, int al, int &skip)
{
  const RefineMasks &tab = refine_masks();
  const uint64_t mnat = nonzero_mask(blk);
  uint64_t hist = 0;
  for (int i = 0; i < 8; i++) hist |= tab.to_rev[i][(mnat >> (8 * i)) & 255];
  const uint64_t band = (~0ull >> ss) & (~0ull << (63 - se)); // positions ss..se
  const uint64_t M = hist & band, Z = ~hist & band;
  uint64_t corr = 0;
  bool overflow = false;
#define corrections(seg) corr |= refine_correction_bits(b, (seg))
  if (skip > 0) { // inside an EOB run: corrections only
    corrections(M);
    skip--;
  } else {
    int k0 = ss; // next position to look at
    for (;;) {
      if (b.n < 32) b.refill();
      const int rs = decode_symbol(b, ac);
      if (rs < 0) return MIJPEG_ERR_MALFORMED_STREAM;
      const int r = rs >> 4, s = rs & 15;
      const uint64_t ahead = ~0ull >> k0; // positions k0..63
      int val = 0;
      if (s == 0) {
        if (r != 15) { // EOB run: this block's remaining positions take corrections only
          skip = 1 << r;
          if (r) { skip |= (int)b.peek(r); b.skip(r); }
          skip--;
          corrections(M & ahead);
          break;
        }
      } else {
        if (s != 1) return MIJPEG_ERR_MALFORMED_STREAM; // the reference warns and decodes on; reported here
        val = b.peek(1) ? 1 : -1;
        b.skip(1);
      }
      const uint64_t zr = Z & ahead;
      const int c = (int)_mm_popcnt_u64(zr);
      if (c <= r) { // fewer than r + 1 zero positions left: the band ends first
        corrections(M & ahead);
        break;
      }
      const int bit = __builtin_ctzll(_pdep_u64(1ull << (c - r - 1), zr)); // the (r + 1)-th zero position from the cursor
      const int t = 63 - bit;
      corrections(M & ahead & ~((bit == 63 ? 0ull : (2ull << bit)) - 1)); // non-zero positions in front of it
      if (val) {
        const int nv = val * (1 << al);
        overflow |= nv != (T)nv;
        blk[zz[t]] = (T)nv;
      }
      if (t == se) break;
      k0 = t + 1;
    }
  }
  if (corr) {
    uint64_t nat = 0;
    for (int i = 0; i < 8; i++) nat |= tab.to_nat[i][(corr >> (8 * i)) & 255];
    if (!apply_corrections(blk, nat, al)) overflow = true;
  }
  return overflow ? MIJPEG_ERR_OVERFLOW_PARAMETER : 0;
#undef corrections
}

// ... and the same pass WITHOUT the block: what the scan finds (the block's non-zero pattern, reversed zigzag) comes in as a
// mask, what it does goes out as three -- corrections, new coefficients, which of those are positive.  The hidden refinement
// scans of a JPEG XT residual form chains of four over the same component, pipelined row behind row on four threads: with the
// blocks themselves as the medium every one of the 256-byte int32 blocks travels from core to core three times, dirty, on the
// serial path of each scan.  With masks, 8 bytes per block travel, the parsers never touch the coefficient planes, and the
// planes are updated once, by all threads, when the chain is through (apply_deferred_refinement).
// (`unused`: not a template and not inline, and speculative_decode.cpp includes this header without calling it)
__attribute__((target("avx2,bmi2,popcnt,lzcnt"), unused)) static int parse_block_refine_ac(BitReader &b, const HuffTable &ac, uint64_t hist, int ss, int se, int &skip,
                                                                                uint64_t &corr_out, uint64_t &fresh_out, uint64_t &plus_out)
{
  // Masks in zigzag order here, bit k = position k, which makes the target of a symbol -- the (r + 1)-th zero position from the
  // cursor -- one PDEP of 1 << r into the zero positions ahead, no count first; the positions in front of it are the bits below.
  // What the parse depends on is only HOW MANY correction bits a symbol passes (one POPCNT): the bits themselves are collected
  // as they come, first bit on top, and spread over their positions once per block.  Symbol -> PDEP -> POPCNT -> shift is the
  // whole chain from one symbol to the next.
  const uint64_t band = ((2ull << se) - 1) & ~((1ull << ss) - 1); // positions ss..se
  const uint64_t M = hist & band, Z = ~hist & band;
  uint64_t passed = 0, raw = 0, fresh = 0, plus = 0; // passed: the non-zero positions whose correction bits are in raw, in stream order
#define corrections(SEG)                                                                  \
  do {                                                                                     \
    const uint64_t seg_ = (SEG);                                                           \
    int left = (int)_mm_popcnt_u64(seg_);                                                  \
    passed |= seg_;                                                                        \
    if (__builtin_expect(left > 32 || b.n < left, 0)) {                                    \
      while (left > 0) {                                                                   \
        const int c = left < 32 ? left : 32;                                               \
        if (b.n < c) b.refill();                                                           \
        raw = (raw << c) | b.peek(c);                                                      \
        b.skip(c);                                                                         \
        left -= c;                                                                         \
      }                                                                                    \
    } else {                                                                               \
      raw = (raw << left) | ((b.acc >> 1) >> (63 - left)); /* (no bits: nothing moves) */  \
      b.skip(left);                                                                        \
    }                                                                                      \
  } while (0)
  if (skip > 0) { // inside an EOB run: corrections only
    corrections(M);
    skip--;
  } else {
    uint64_t ahead = ~0ull << ss; // positions from the cursor on
    for (;;) {
      if (b.n < 32) b.refill();
      const int rs = decode_symbol(b, ac);
      if (rs < 0) return MIJPEG_ERR_MALFORMED_STREAM;
      const int r = rs >> 4, s = rs & 15;
      uint64_t val = 0, positive = 0;
      if (s == 0) {
        if (r != 15) { // EOB run: this block's remaining positions take corrections only
          skip = 1 << r;
          if (r) { skip |= (int)b.peek(r); b.skip(r); }
          skip--;
          corrections(M & ahead);
          break;
        }
      } else {
        if (s != 1) return MIJPEG_ERR_MALFORMED_STREAM; // the reference warns and decodes on; reported here
        val = ~0ull;
        positive = 0ull - (uint64_t)b.peek(1);
        b.skip(1);
      }
      const uint64_t sel = _pdep_u64(1ull << r, Z & ahead); // the (r + 1)-th zero position from the cursor, as a bit
      if (!sel) { // fewer than r + 1 zero positions left: the band ends first
        corrections(M & ahead);
        break;
      }
      corrections(M & ahead & (sel - 1)); // the non-zero positions in front of it
      fresh |= sel & val;
      plus |= sel & positive;
      if (sel >> se) break; // (the band's last position)
      ahead = ~(sel | (sel - 1));
    }
  }
  // raw holds popcount(passed) bits, the first one read on top; it belongs to the lowest position
  uint64_t corr = 0;
  if (passed) {
    const int n = (int)_mm_popcnt_u64(passed);
    uint64_t x = raw << (64 - n); // first bit read = bit 63
    x = __builtin_bswap64(x);
    x = ((x & 0xf0f0f0f0f0f0f0f0ull) >> 4) | ((x & 0x0f0f0f0f0f0f0f0full) << 4);
    x = ((x & 0xccccccccccccccccull) >> 2) | ((x & 0x3333333333333333ull) << 2);
    x = ((x & 0xaaaaaaaaaaaaaaaaull) >> 1) | ((x & 0x5555555555555555ull) << 1); // ... = bit 0
    corr = _pdep_u64(x, passed);
  }
#undef corrections
  corr_out = corr;
  fresh_out = fresh;
  plus_out = plus;
  return 0;
}
// the block's pattern as the parsers want it
template <class T>
__attribute__((target("avx2,bmi2,popcnt,lzcnt"))) static uint64_t block_history_mask(const T *blk)
{
  const RefineMasks &tab = refine_masks();
  const uint64_t mnat = nonzero_mask(blk);
  uint64_t hist = 0;
  for (int i = 0; i < 8; i++) hist |= tab.to_zz[i][(mnat >> (8 * i)) & 255];
  return hist;
}
// one scan's doing on one block; false: a 16-bit store overflowed
template <class T>
__attribute__((target("avx2,bmi2,popcnt,lzcnt"))) static bool apply_deferred_block(T *blk, const uint8_t *zz, uint64_t corr, uint64_t fresh, uint64_t plus, int al)
{
  while (fresh) {
    const int bit = __builtin_ctzll(fresh);
    fresh &= fresh - 1;
    blk[zz[bit]] = (T)(((plus >> bit) & 1) ? (1 << al) : -(1 << al)); // (al <= 13: fits either store)
  }
  if (!corr) return true;
  const RefineMasks &tab = refine_masks();
  uint64_t nat = 0;
  for (int i = 0; i < 8; i++) nat |= tab.to_ras[i][(corr >> (8 * i)) & 255];
  return apply_corrections(blk, nat, al);
}
#else
__attribute__((unused)) static int parse_block_refine_ac(BitReader &, const HuffTable &, uint64_t, int, int, int &, uint64_t &, uint64_t &, uint64_t &) { return MIJPEG_ERR_MALFORMED_STREAM; }
template <class T> static uint64_t block_history_mask(const T *) { return 0; }
template <class T> static bool apply_deferred_block(T *, const uint8_t *, uint64_t, uint64_t, uint64_t, int) { return false; }
template <class T>
static int decode_block_refine_ac_masks(BitReader &b, const HuffTable &ac, T *blk, const uint8_t *zz, int ss, int se, int al, int &skip)
{
  return decode_block_refine(b, ac, blk, zz, ss, se, al, skip);
}
#endif

// Sequential block into either store (the 32-bit store only ever sees frames with hidden bits, i.e. the progressive
// functions; this overload keeps decode_t<int32_t> complete).
static inline int decode_block_seq(BitReader &b, const HuffTable &dc, const HuffTable &ac, int &pred, int16_t *blk,
                                   const uint16_t *q, const uint8_t *zz, uint32_t &qmax)
{
  return decode_block(b, dc, ac, pred, blk, q, zz, qmax);
}
static inline int decode_block_seq(BitReader &b, const HuffTable &dc, const HuffTable &ac, int &pred, int32_t *blk,
                                   const uint16_t *, const uint8_t *zz, uint32_t &)
{
  int skip = 0;
  memset(blk, 0, 256);
  return decode_block_first<int32_t>(b, dc, ac, pred, blk, zz, 0, 63, 0, skip);
}

// Bytes of entropy coded data per speculative range (speculative_decode.cpp; the scan loop asks whether a scan is worth it)
size_t spec_segment_bytes();

} // namespace mij
#endif
