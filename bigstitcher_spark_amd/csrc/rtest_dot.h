/* r-test chunk sums from 8-bit dot products — the arithmetic of
 * k_rtest_dot (bigstitch.hip, BS_CORR_MODE=dot) and of the host sanitizer
 * program tests/rtest_dot_host.cpp. Loads, masks and the realign are those
 * of rtest_walk.h (whose bounds argument carries over unchanged: only
 * chunks that hold a live element are loaded); what differs is how the 8
 * masked element pairs of a chunk are summed.
 *
 * Each masked u16 is split into its bytes, a = al + 256 ah. For the four
 * elements of two dwords a byte permute gathers the four low bytes into
 * one dword and the four high bytes into another, and the five sums come
 * out of 4 x u8 dot products D(x, y) = sum_i x_i y_i, S(x) = D(x, 1):
 *
 *   sum a  = S(al) + 256 S(ah)                        (likewise b)
 *   sum aa = D(al,al) + 512 D(al,ah) + 65536 D(ah,ah) (likewise b)
 *   sum ab = D(al,bl) + 256 [D(al,bh) + D(ah,bl)] + 65536 D(ah,bh)
 *
 * Thirteen u32 accumulators per lane and no 64-bit operation per chunk;
 * bs_rd_widen recombines them into the five u64 sums. The integers are the
 * ones bs_rw_consume adds, in another order -> bit-identical [PIN-R].
 *
 * Overflow bound. The cross term ab_x takes D(al,bh) + D(ah,bl), at most
 * 2 * 255^2 = 130050 per element; every other accumulator grows slower
 * (255^2 or 255 per element). 8 * 4128 * 130050 = 4294771200 <= 2^32 - 1
 * and one more chunk passes it, so a set of accumulators is exact for
 * BS_RD_MAX_CHUNKS = 4128 chunks between two bs_rd_widen calls, whatever
 * the data. */
#ifndef BS_RTEST_DOT_H
#define BS_RTEST_DOT_H

#include "rtest_walk.h"

#define BS_RD_MAX_CHUNKS 4128

struct bs_rd_acc { /* u32 partial dot products since the last widen */
  uint32_t sa_l, sa_h, sb_l, sb_h;
  uint32_t aa_ll, aa_lh, aa_hh;
  uint32_t bb_ll, bb_lh, bb_hh;
  uint32_t ab_ll, ab_x, ab_hh;
};

BS_RW_FN void bs_rd_zero(bs_rd_acc &c) {
  c.sa_l = c.sa_h = c.sb_l = c.sb_h = 0;
  c.aa_ll = c.aa_lh = c.aa_hh = 0;
  c.bb_ll = c.bb_lh = c.bb_hh = 0;
  c.ab_ll = c.ab_x = c.ab_hh = 0;
}

/* v_perm_b32: result byte i is byte sel[i] of the 8-byte value hi:lo
 * (0..3 from lo, 4..7 from hi). Only selector bytes 0..7 are used here. */
BS_RW_FN uint32_t bs_rd_perm(uint32_t hi, uint32_t lo, uint32_t sel) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_perm(hi, lo, sel);
#else
  const uint64_t v = ((uint64_t)hi << 32) | lo;
  uint32_t o = 0;
  for (int i = 0; i < 4; ++i) {
    const uint32_t s = (sel >> (8 * i)) & 7u;
    o |= (uint32_t)((v >> (8 * s)) & 0xFFu) << (8 * i);
  }
  return o;
#endif
}

#define BS_RD_SEL_LO 0x06040200u /* low bytes of the four u16 of hi:lo */
#define BS_RD_SEL_HI 0x07050301u /* their high bytes */

/* acc + sum of the four u8*u8 products (v_dot4_u32_u8, no clamp) */
BS_RW_FN uint32_t bs_rd_dot4(uint32_t x, uint32_t y, uint32_t acc) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_udot4(x, y, acc, false);
#else
  for (int i = 0; i < 4; ++i)
    acc += ((x >> (8 * i)) & 0xFFu) * ((y >> (8 * i)) & 0xFFu);
  return acc;
#endif
}

/* four element pairs: a0:a1 and b0:b1 are two dwords of u16 each, already
 * masked */
BS_RW_FN void bs_rd_add4(uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1,
                         bs_rd_acc &c) {
  const uint32_t one = 0x01010101u;
  const uint32_t al = bs_rd_perm(a1, a0, BS_RD_SEL_LO);
  const uint32_t ah = bs_rd_perm(a1, a0, BS_RD_SEL_HI);
  const uint32_t bl = bs_rd_perm(b1, b0, BS_RD_SEL_LO);
  const uint32_t bh = bs_rd_perm(b1, b0, BS_RD_SEL_HI);
  c.sa_l = bs_rd_dot4(al, one, c.sa_l);
  c.sa_h = bs_rd_dot4(ah, one, c.sa_h);
  c.sb_l = bs_rd_dot4(bl, one, c.sb_l);
  c.sb_h = bs_rd_dot4(bh, one, c.sb_h);
  c.aa_ll = bs_rd_dot4(al, al, c.aa_ll);
  c.aa_lh = bs_rd_dot4(al, ah, c.aa_lh);
  c.aa_hh = bs_rd_dot4(ah, ah, c.aa_hh);
  c.bb_ll = bs_rd_dot4(bl, bl, c.bb_ll);
  c.bb_lh = bs_rd_dot4(bl, bh, c.bb_lh);
  c.bb_hh = bs_rd_dot4(bh, bh, c.bb_hh);
  c.ab_ll = bs_rd_dot4(al, bl, c.ab_ll);
  c.ab_x = bs_rd_dot4(al, bh, c.ab_x);
  c.ab_x = bs_rd_dot4(ah, bl, c.ab_x);
  c.ab_hh = bs_rd_dot4(ah, bh, c.ab_hh);
}

/* one chunk: realign B, mask both operands with the four dword masks m
 * (bs_rw_dword_mask of the chunk's element mask), add the 8 pairs */
BS_RW_FN void bs_rd_consume_m(const bs_rw_v4 &a, const bs_rw_v4 &lo,
                              const bs_rw_v4 &hi, int de, uint32_t m0,
                              uint32_t m1, uint32_t m2, uint32_t m3,
                              bs_rd_acc &c) {
  const bs_rw_v4 bsh = bs_rw_realign(lo, hi, de);
  bs_rd_add4(a.d[0] & m0, a.d[1] & m1, bsh.d[0] & m0, bsh.d[1] & m1, c);
  bs_rd_add4(a.d[2] & m2, a.d[3] & m3, bsh.d[2] & m2, bsh.d[3] & m3, c);
}

/* drop-in for bs_rw_consume on a bs_rw_fetch step (masks derived here:
 * the path for row strides that move the 16-byte phase from row to row) */
BS_RW_FN void bs_rd_consume(const bs_rw_step &st, int de, bs_rd_acc &c) {
  bs_rd_consume_m(st.a, st.lo, st.hi, de, bs_rw_dword_mask(st.mask, 0),
                  bs_rw_dword_mask(st.mask, 1), bs_rw_dword_mask(st.mask, 2),
                  bs_rw_dword_mask(st.mask, 3), c);
}

/* s = {sum a, sum b, sum aa, sum bb, sum ab} += the accumulators, which are
 * cleared. Each weighted term is below 2^32 * 2^16 and there are at most
 * four of them: no u64 wrap. */
BS_RW_FN void bs_rd_widen(bs_rd_acc &c, uint64_t s[5]) {
  s[0] += (uint64_t)c.sa_l + ((uint64_t)c.sa_h << 8);
  s[1] += (uint64_t)c.sb_l + ((uint64_t)c.sb_h << 8);
  s[2] += (uint64_t)c.aa_ll + ((uint64_t)c.aa_lh << 9) +
          ((uint64_t)c.aa_hh << 16);
  s[3] += (uint64_t)c.bb_ll + ((uint64_t)c.bb_lh << 9) +
          ((uint64_t)c.bb_hh << 16);
  s[4] += (uint64_t)c.ab_ll + ((uint64_t)c.ab_x << 8) +
          ((uint64_t)c.ab_hh << 16);
  bs_rd_zero(c);
}

/* Hoisting. When both views' row strides are multiples of 8 elements, every
 * row of a candidate that one block walks has the same ha, de and nch (row
 * bases differ by multiples of 16 bytes), so for chunk index k the element
 * mask, its dword masks and the lo/hi B chunk choice depend on the
 * candidate alone. bs_rd_hoist derives them once from the first row; a row
 * `row` further on is read at element offsets aoff + row*astep etc. k must
 * be in [0, nch): the mask is then non-zero in EVERY row, so each load
 * holds a live element (the bounds argument of rtest_walk.h). */
struct bs_rd_lane {
  long aoff, lo_off, hi_off; /* element offsets of the three chunks, row 0 */
  uint32_t m0, m1, m2, m3;   /* dword keep-masks */
  int de;
};

BS_RW_FN bool bs_rd_can_hoist(long a_sx, long b_sx) {
  return ((a_sx | b_sx) & 7) == 0;
}

BS_RW_FN bs_rd_lane bs_rd_hoist(const bs_rw_row &r, int k) {
  bs_rd_lane h;
  const unsigned mask = bs_rw_mask(r, k);
  const long bc = r.bc0 + k;
  h.aoff = (r.ac0 + k) * 8;
  h.lo_off = (bs_rw_need_lo(r.de, mask) ? bc : bc + 1) * 8;
  h.hi_off = (bs_rw_need_hi(r.de, mask) ? bc + 1 : bc) * 8;
  h.m0 = bs_rw_dword_mask(mask, 0);
  h.m1 = bs_rw_dword_mask(mask, 1);
  h.m2 = bs_rw_dword_mask(mask, 2);
  h.m3 = bs_rw_dword_mask(mask, 3);
  h.de = r.de;
  return h;
}

struct bs_rd_step {
  bs_rw_v4 a, lo, hi;
};

/* aro / bro: element offsets of the row against row 0 (multiples of 8) */
BS_RW_FN bs_rd_step bs_rd_fetch(const unsigned short *abase,
                                const unsigned short *bbase,
                                const bs_rd_lane &h, long aro, long bro) {
  bs_rd_step s;
  s.a = bs_rw_load16(abase + h.aoff + aro, 0);
  s.lo = bs_rw_load16(bbase + h.lo_off + bro, 0);
  s.hi = bs_rw_load16(bbase + h.hi_off + bro, 0);
  return s;
}

BS_RW_FN void bs_rd_consume_h(const bs_rd_step &s, const bs_rd_lane &h,
                              bs_rd_acc &c) {
  bs_rd_consume_m(s.a, s.lo, s.hi, h.de, h.m0, h.m1, h.m2, h.m3, c);
}

#endif /* BS_RTEST_DOT_H */
