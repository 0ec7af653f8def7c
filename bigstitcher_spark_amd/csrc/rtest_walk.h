/* r-test row walk in 16-byte chunks — the chunk arithmetic shared by
 * k_rtest_wide (bigstitch.hip) and the host sanitizer program
 * (tests/rtest_walk_host.cpp). Everything here works on ELEMENT indices
 * (uint16 units) relative to a view's base pointer, which must be 16-byte
 * aligned (hipMalloc gives 256).
 *
 * One row pair: A elements [ea, ea+nx), B elements [eb, eb+nx); element
 * ea+i pairs with eb+i. The A row is cut on the view's 16-byte grid: chunk
 * k (k = 0..nch-1) holds A elements 8*(ac0+k) + j, j = 0..7; element j is
 * live iff ha <= 8k+j < ha+nx, everything else is masked to zero in BOTH
 * operands (a zero adds nothing to any of the five sums, so heads and
 * tails need no path of their own). The 8 B elements that pair with
 * chunk k start `de` elements (delta = 2*de bytes, constant along the
 * row) into B chunk bc0+k and run into chunk bc0+k+1; they are cut out of
 * the two aligned chunks by a dword select (de>>1) and a 2-byte funnel
 * shift (de&1).
 *
 * Bounds: a chunk is only ever loaded when it holds at least one live
 * element. A live element lies inside its view, so the chunk holding it
 * starts at a non-negative multiple of 16 bytes below that element and
 * ends at most 14 bytes past it — inside the allocation once that is
 * rounded up to a multiple of 16 bytes. Where the lo (or hi) B chunk holds
 * no live element, the other one — which then must — is fetched in its
 * place; its lanes land in masked positions only. */
#ifndef BS_RTEST_WALK_H
#define BS_RTEST_WALK_H

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define BS_RW_FN __host__ __device__ __forceinline__
#else
#define BS_RW_FN static inline
#endif

struct bs_rw_row {
  long ac0; /* A chunk index of the row's first chunk */
  long bc0; /* B chunk index holding the partner of A chunk ac0's element 0
               (can be negative or past the view; then it is never live) */
  int ha;   /* first live element inside chunk 0, 0..7 */
  int de;   /* element phase of B against A's chunk grid, 0..7 */
  int nx;
  int nch;  /* chunks covering the row */
};

struct bs_rw_v4 { /* one 16-byte chunk as four dwords, x lowest */
  uint32_t d[4];
};

BS_RW_FN bs_rw_row bs_rw_setup(long ea, long eb, int nx) {
  bs_rw_row r;
  r.ac0 = ea >> 3;
  r.ha = (int)(ea & 7);
  const long ebs = eb - r.ha; /* B partner of A chunk 0's element 0 */
  r.bc0 = ebs >> 3;           /* arithmetic shift: floor also below zero */
  r.de = (int)(ebs & 7);
  r.nx = nx;
  r.nch = (r.ha + nx + 7) >> 3;
  return r;
}

/* upper bound of bs_rw_setup().nch over all row phases */
BS_RW_FN int bs_rw_max_chunks(int nx) { return (nx + 14) >> 3; }

/* 8-bit live-element mask of chunk k (bit j = element j); 0 for k outside
 * [0, nch) */
BS_RW_FN unsigned bs_rw_mask(const bs_rw_row &r, int k) {
  if (k < 0 || k >= r.nch) return 0u;
  int jlo = r.ha - 8 * k;
  int jhi = r.ha + r.nx - 8 * k;
  jlo = jlo < 0 ? 0 : jlo;
  jhi = jhi > 8 ? 8 : jhi;
  return (0xFFu >> (8 - jhi)) & (0xFFu << jlo) & 0xFFu;
}

/* does the lo / hi B chunk of a step hold a live element? Partner of
 * element j sits at position de+j of the 16-element lo:hi window. */
BS_RW_FN bool bs_rw_need_lo(int de, unsigned mask) {
  return (mask & (0xFFu >> de)) != 0;
}
BS_RW_FN bool bs_rw_need_hi(int de, unsigned mask) {
  return (mask & ~(0xFFu >> de) & 0xFFu) != 0;
}

/* dword i of the 128-bit keep-mask of an element mask */
BS_RW_FN uint32_t bs_rw_dword_mask(unsigned mask, int i) {
  const uint32_t lo = 0u - ((mask >> (2 * i)) & 1u);
  const uint32_t hi = 0u - ((mask >> (2 * i + 1)) & 1u);
  return (lo & 0xFFFFu) | (hi << 16);
}

BS_RW_FN bs_rw_v4 bs_rw_load16(const unsigned short *base, long chunk) {
  bs_rw_v4 v;
#if defined(__HIP_DEVICE_COMPILE__)
  typedef uint32_t v4u __attribute__((ext_vector_type(4)));
  const v4u t = *(const v4u *)(base + chunk * 8); /* global_load_dwordx4 */
  v.d[0] = t.x; v.d[1] = t.y; v.d[2] = t.z; v.d[3] = t.w;
#else
  memcpy(v.d, base + chunk * 8, 16);
#endif
  return v;
}

/* low dword of (hi:lo) >> (16 * odd) */
BS_RW_FN uint32_t bs_rw_funnel(uint32_t hi, uint32_t lo, int odd) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_alignbyte(hi, lo, (uint32_t)(odd << 1));
#else
  return odd ? (lo >> 16) | (hi << 16) : lo;
#endif
}

/* elements de..de+7 of the 16-element window lo:hi */
BS_RW_FN bs_rw_v4 bs_rw_realign(const bs_rw_v4 &lo, const bs_rw_v4 &hi,
                                int de) {
  /* scalars and value selects only: an indexed local array here ends up
   * in scratch memory on the GPU */
  const bool s2 = (de & 4) != 0, s1 = (de & 2) != 0;
  const int odd = de & 1;
  const uint32_t x0 = s2 ? lo.d[2] : lo.d[0], x1 = s2 ? lo.d[3] : lo.d[1],
                 x2 = s2 ? hi.d[0] : lo.d[2], x3 = s2 ? hi.d[1] : lo.d[3],
                 x4 = s2 ? hi.d[2] : hi.d[0], x5 = s2 ? hi.d[3] : hi.d[1];
  const uint32_t y0 = s1 ? x1 : x0, y1 = s1 ? x2 : x1, y2 = s1 ? x3 : x2,
                 y3 = s1 ? x4 : x3, y4 = s1 ? x5 : x4;
  bs_rw_v4 o;
  o.d[0] = bs_rw_funnel(y1, y0, odd);
  o.d[1] = bs_rw_funnel(y2, y1, odd);
  o.d[2] = bs_rw_funnel(y3, y2, odd);
  o.d[3] = bs_rw_funnel(y4, y3, odd);
  return o;
}

struct bs_rw_step { /* what one lane holds between fetch and consume */
  bs_rw_v4 a, lo, hi;
  unsigned mask;
};

/* loads of chunk k of a row pair. k outside [0, nch) is allowed (lanes of
 * a wider group): it re-reads the row's last chunk and masks everything. */
BS_RW_FN bs_rw_step bs_rw_fetch(const unsigned short *abase,
                                const unsigned short *bbase,
                                const bs_rw_row &r, int k) {
  bs_rw_step s;
  s.mask = bs_rw_mask(r, k);
  const int kk = k < r.nch ? k : r.nch - 1;
  const unsigned live = bs_rw_mask(r, kk); /* never 0 */
  const bool nlo = bs_rw_need_lo(r.de, live);
  const bool nhi = bs_rw_need_hi(r.de, live);
  const long bc = r.bc0 + kk;
  s.a = bs_rw_load16(abase, r.ac0 + kk);
  s.lo = bs_rw_load16(bbase, nlo ? bc : bc + 1);
  s.hi = bs_rw_load16(bbase, nhi ? bc + 1 : bc);
  return s;
}

/* mask, realign, and add the chunk's 8 element pairs into
 * s = {sum a, sum b, sum aa, sum bb, sum ab}. Exact: a u16*u16 product
 * fits u32 ((2^16-1)^2 < 2^32) and is widened to u64 before it meets
 * another; the chunk's plain sums stay in u32 (8 * 65535 < 2^20). */
BS_RW_FN void bs_rw_consume(const bs_rw_step &st, int de, uint64_t s[5]) {
  const bs_rw_v4 bsh = bs_rw_realign(st.lo, st.hi, de);
  uint32_t ca = 0, cb = 0;
  uint64_t aa = 0, bb = 0, ab = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int i = 0; i < 4; ++i) {
    const uint32_t m = bs_rw_dword_mask(st.mask, i);
    const uint32_t av = st.a.d[i] & m, bv = bsh.d[i] & m;
    const uint32_t al = av & 0xFFFFu, ah = av >> 16;
    const uint32_t bl = bv & 0xFFFFu, bh = bv >> 16;
    ca += al + ah;
    cb += bl + bh;
    aa += (uint64_t)(al * al) + (uint64_t)(ah * ah);
    bb += (uint64_t)(bl * bl) + (uint64_t)(bh * bh);
    ab += (uint64_t)(al * bl) + (uint64_t)(ah * bh);
  }
  s[0] += ca;
  s[1] += cb;
  s[2] += aa;
  s[3] += bb;
  s[4] += ab;
}

#endif /* BS_RTEST_WALK_H */
