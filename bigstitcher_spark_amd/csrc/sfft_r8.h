/* Strided-pass FFT schedule at n = 512: the radix-8 Stockham stages of
 * xfft_r4.h (E = 8, three constant-geometry stages) run on a workgroup
 * tile of 8 adjacent columns = 4 column PAIRS x 512 elements, every value a
 * quad (x, y, z, w) = two complex numbers, one of each line of the pair.
 * Shared by k_fft_pass_r8 / k_fft_z_fused_r8x (bigstitch.hip) and the host
 * sanitizer program (tests/sfft_r8_host.cpp), which runs the 256 threads as
 * loops and the exchange tile as a heap array of the kernel's size.
 *
 * Two thread mappings of the 256 threads (4 waves):
 *   I/O    pair = tid & 3, lane = tid >> 2: a wave instruction moves 16 rows
 *          x 64 contiguous bytes of global memory. The thread holds rows
 *          lane + 64 r of its pair — exactly v[r] = z[lane + 64 r], the
 *          input of stage 0 (L = 1) and the output of stage 2 (L = 64) of
 *          butterfly `lane`. So the first stage runs on the loaded registers
 *          and the last stage's results go straight to global memory:
 *          natural order in and out, no bit reversal, no LDS staging.
 *   owner  pair = tid >> 6 (the wave), lane = tid & 63: one wave owns one
 *          pair's 8 KB slice of the tile, so an exchange whose two sides are
 *          both in the owner mapping needs no block barrier (same-wave LDS
 *          operations execute in order).
 *
 * Exchange tile: SF_TILE quads (32 KB). Element m of pair p lives at
 * sf_idx(p, m) = 512 p + (xf_swz<8>(m) ^ sf_twist(p)): the x-pass swizzle
 * inside the slice, plus a per-pair XOR so that the I/O mapping, whose
 * neighbouring lanes hold the SAME m of the four pairs, spreads over the
 * banks too (the table tests/sfft_r8_host.cpp prints).
 *
 * Twiddles are the forward set of xf_load_tw<8> (half-circle table of
 * length 2 n = 1024); the inverse multiplies by the conjugate. */
#ifndef BS_SFFT_R8_H
#define BS_SFFT_R8_H

#include <math.h>

#include "xfft_r4.h"

#define SF_N 512       /* FFT length */
#define SF_PAIRS 4     /* column pairs per tile (8 columns) */
#define SF_THREADS 256 /* 4 waves */
#define SF_TILE (SF_PAIRS * SF_N) /* quads in the exchange tile */

BS_XF_FN int sf_io_pair(int tid) { return tid & (SF_PAIRS - 1); }
BS_XF_FN int sf_io_lane(int tid) { return tid >> 2; }
BS_XF_FN int sf_own_pair(int tid) { return tid >> 6; }
BS_XF_FN int sf_own_lane(int tid) { return tid & 63; }

/* per-pair XOR of the slot index inside the slice: 0, 2, 13, 15 */
BS_XF_FN int sf_twist(int p) { return (2 * p) ^ (9 * (p >> 1)); }

/* slot of element m of pair p; a bijection of [0, SF_TILE) that keeps
 * pair p inside [512 p, 512 p + 512) */
BS_XF_FN int sf_idx(int p, int m) {
  return SF_N * p + (xf_swz<8>(m) ^ sf_twist(p));
}

/* the two lines of a thread's pair: a[r], b[r] = element lane + 64 r */
template <class C>
struct sf_lines {
  C a[8], b[8];
};

template <class C, class Q>
BS_XF_FN void sf_split(const Q &q, C &a, C &b) {
  a = {q.x, q.y};
  b = {q.z, q.w};
}

template <class Q, class C>
BS_XF_FN Q sf_join(C a, C b) {
  return {a.x, a.y, b.x, b.y};
}

/* a * b (DIR > 0) or a * conj(b) (DIR < 0) */
template <int DIR, class C>
BS_XF_FN C sf_twmul(C a, C b) {
  return DIR > 0 ? C{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}
                 : C{a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y};
}

/* stage 0 of both lines: no twiddles */
template <int DIR, class C>
BS_XF_FN void sf_stage0(sf_lines<C> &v) {
  xf_bfly<DIR>(v.a);
  xf_bfly<DIR>(v.b);
}

/* stage si >= 1 of both lines; w = the forward twiddles tws.w[si - 1] of
 * the butterfly (lane) the thread runs */
template <int DIR, class C>
BS_XF_FN void sf_stage(sf_lines<C> &v, const C (&w)[7]) {
  BS_XF_UNROLL
  for (int r = 1; r < 8; ++r) v.a[r] = sf_twmul<DIR>(v.a[r], w[r - 1]);
  xf_bfly<DIR>(v.a);
  BS_XF_UNROLL
  for (int r = 1; r < 8; ++r) v.b[r] = sf_twmul<DIR>(v.b[r], w[r - 1]);
  xf_bfly<DIR>(v.b);
}

/* Every slot a thread touches in one exchange is ONE per-thread base XOR a
 * compile-time constant, because the bits an output or input number moves
 * are disjoint from the bits the lane sets:
 *   write after stage L = 1:  sf_idx(p, 8 lane + s)         = base ^ s
 *   write after stage L = 8:  sf_idx(p, 64 (lane / 8) + lane % 8 + 8 s)
 *                                                            = base ^ 9 s
 *   read:                     sf_idx(p, lane + 64 r) = base ^ (64 r | 8 (r & 1))
 * with base = the slot of s = 0 or r = 0. A kernel keeps one base register
 * per exchange side instead of eight addresses; the host program checks
 * the identities against sf_idx for every pair, lane and number. */
BS_XF_FN int sf_put_base(int p, int lane, int L) {
  return sf_idx(p, xf_dst<8>(L, lane, 0));
}
BS_XF_FN int sf_put_xor(int L, int s) { return L == 1 ? s : 9 * s; }
BS_XF_FN int sf_get_base(int p, int lane) { return sf_idx(p, lane); }
BS_XF_FN int sf_get_xor(int r) { return (64 * r) | (8 * (r & 1)); }

/* write side of the exchange after the stage of sub-size L (1 or 8): the
 * outputs of the butterfly whose base slot is `base`. T is anything
 * indexable that yields quads Q (a pointer into LDS on the GPU, a checking
 * wrapper on the host). */
template <class Q, int L, class T, class C>
BS_XF_FN void sf_put(T tile, int base, const sf_lines<C> &v) {
  static_assert(L == 1 || L == 8, "the two exchanges of three stages");
  BS_XF_UNROLL
  for (int s = 0; s < 8; ++s)
    tile[base ^ sf_put_xor(L, s)] = sf_join<Q>(v.a[s], v.b[s]);
}

/* read side: the inputs lane + 64 r of the butterfly */
template <class Q, class T, class C>
BS_XF_FN void sf_get(T tile, int base, sf_lines<C> &v) {
  BS_XF_UNROLL
  for (int r = 0; r < 8; ++r) {
    const Q q = tile[base ^ sf_get_xor(r)];
    sf_split(q, v.a[r], v.b[r]);
  }
}

/* Per-workgroup twiddle table (LDS on the GPU), for a kernel that cannot
 * keep a stage's seven twiddles in registers across its tile loop: the
 * forward twiddles of xf_load_tw<8>, laid out so that a wave's read of
 * w^r is contiguous. Stage 1 (L = 8) depends on lane % 8 only: 7 x 8
 * entries; stage 2 (L = 64): 7 x 64. */
#define SF_TW1 (7 * 8)
#define SF_TWN (SF_TW1 + 7 * 64) /* 504 entries, 4032 bytes */

BS_XF_FN int sf_tw_slot(int si, int r, int lane) {
  return si == 1 ? (r - 1) * 8 + (lane & 7) : SF_TW1 + (r - 1) * 64 + lane;
}

/* entry i of the table, from the half-circle table of length 1024 */
template <class C>
BS_XF_FN C sf_tw_entry(const C *twn, int i) {
  const int si = i < SF_TW1 ? 1 : 2;
  const int k = i < SF_TW1 ? i : i - SF_TW1;
  const int r = (si == 1 ? k >> 3 : k >> 6) + 1;
  const int lane = si == 1 ? k & 7 : k & 63;
  return xf_tw<8>(twn, xf_tw_q<8>(xf_L<8>(si), lane, r), +1);
}

/* the seven twiddles of stage si (1 or 2) of butterfly `lane` */
template <class C, class T>
BS_XF_FN void sf_get_tw(T tab, int si, int lane, C (&w)[7]) {
  BS_XF_UNROLL
  for (int r = 1; r < 8; ++r) w[r - 1] = tab[sf_tw_slot(si, r, lane)];
}

/* cross-power bin conj(a) * b normalised to length `scale`; a magnitude
 * (squared) at or below 1e-40 gives exactly 0 [PIN-EPS] */
template <class C>
BS_XF_FN C sf_crosspower(C a, C b, float scale) {
  const C q = {a.x * b.x + a.y * b.y, a.x * b.y - a.y * b.x};
  const float m = q.x * q.x + q.y * q.y;
  C v = {0.0f, 0.0f};
  if (m > 1e-40f) {
    const float s = scale / sqrtf(m);
    v.x = q.x * s;
    v.y = q.y * s;
  }
  return v;
}

#endif /* BS_SFFT_R8_H */
