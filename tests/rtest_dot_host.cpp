/* Host run of the r-test's 8-bit dot-product sums (csrc/rtest_dot.h), meant
 * to be built with -fsanitize=address,undefined: the views live in heap
 * blocks of exactly n*2 bytes rounded up to 16, so any chunk load outside
 * an allocation is reported. Every case walks the candidate box the way
 * k_rtest_dot does — the hoisted walk (chunk index outer, rows inner) when
 * both row strides are multiples of 8, the per-row walk always — and
 * compares the five sums with a naive u64 triple loop. Also checked: the
 * byte-permute selectors on a known pattern, and the overflow bound
 * BS_RD_MAX_CHUNKS with the kernel's widening guard. Exit 0 = all equal. */
#include "../bigstitcher_spark_amd/csrc/rtest_dot.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

struct view {
  unsigned short *p;
  int w, h, d;
};

static uint32_t rng_state = 24680u;
static uint32_t rnd() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}

static view make_view(int w, int h, int d, bool all_max) {
  const size_t n = (size_t)w * h * d;
  const size_t bytes = (n * 2 + 15) & ~(size_t)15;
  view v = {(unsigned short *)aligned_alloc(16, bytes), w, h, d};
  if (!v.p) abort();
  for (size_t i = 0; i < bytes / 2; ++i) {
    const uint32_t r = rnd();
    /* a good share of 65535; the pad past n is 0xFFFF too, so a masking
     * slip shows in the sums */
    v.p[i] = all_max || i >= n || (r & 3) == 0 ? 65535
                                                : (unsigned short)(r >> 2);
  }
  return v;
}

struct region { /* sub-box of a view, as bs_region */
  const view *v;
  int ox, oy, oz, mx, my, mz;
};

static long cases = 0, hoisted_cases = 0, failures = 0;

static void fail(const char *what) {
  if (failures < 20) fprintf(stderr, "FAIL: %s\n", what);
  ++failures;
}

/* the kernel's guard: widen before a batch of `batch` chunks would pass
 * the bound */
static void guard(bs_rd_acc &acc, uint64_t s[5], int &n, int batch) {
  if (n > BS_RD_MAX_CHUNKS - batch) {
    bs_rd_widen(acc, s);
    n = 0;
  }
  n += batch;
}

static void run_case(const region &a, const region &b, int sx, int sy,
                     int sz) {
  const int s[3] = {sx, sy, sz};
  const int ma[3] = {a.mx, a.my, a.mz}, mb[3] = {b.mx, b.my, b.mz};
  int lo[3], n[3];
  for (int d = 0; d < 3; ++d) { /* the candidate box, A coordinates */
    lo[d] = std::max(0, -s[d]);
    n[d] = std::min(ma[d], mb[d] - s[d]) - lo[d];
    if (n[d] <= 0) return;
  }
  ++cases;
  const long asx = a.v->w, asxy = (long)a.v->w * a.v->h;
  const long bsx = b.v->w, bsxy = (long)b.v->w * b.v->h;
  const bool hoist = bs_rd_can_hoist(asx, bsx);
  if (hoist) ++hoisted_cases;
  uint64_t ref[5] = {0, 0, 0, 0, 0}, row[5] = {0, 0, 0, 0, 0},
           hst[5] = {0, 0, 0, 0, 0};
  int rw = 1; /* lanes per row: also walk the idle lanes' k >= nch */
  while (rw < bs_rw_max_chunks(n[0]) && rw < 64) rw <<= 1;
  for (int z = lo[2]; z < lo[2] + n[2]; ++z) {
    /* row bases exactly as k_rtest_dot forms them */
    const long ea0 =
        (a.oz + z) * asxy + (a.oy + lo[1]) * asx + a.ox + lo[0];
    const long eb0 = (b.oz + z + sz) * bsxy + (b.oy + lo[1] + sy) * bsx +
                     b.ox + lo[0] + sx;
    bs_rd_acc acc;
    int cnt = 0;
    /* naive, and the per-row walk (any stride) */
    bs_rd_zero(acc);
    for (int y = 0; y < n[1]; ++y) {
      const long ea = ea0 + y * asx, eb = eb0 + y * bsx;
      for (int x = 0; x < n[0]; ++x) {
        const uint64_t av = a.v->p[ea + x], bv = b.v->p[eb + x];
        ref[0] += av;
        ref[1] += bv;
        ref[2] += av * av;
        ref[3] += bv * bv;
        ref[4] += av * bv;
      }
      const bs_rw_row r = bs_rw_setup(ea, eb, n[0]);
      for (int k = 0; k < std::max(rw, r.nch); ++k) {
        guard(acc, row, cnt, 1);
        bs_rd_consume(bs_rw_fetch(a.v->p, b.v->p, r, k), r.de, acc);
      }
    }
    bs_rd_widen(acc, row);
    /* the hoisted walk: masks and chunk choice from the first row only */
    if (hoist) {
      const bs_rw_row r0 = bs_rw_setup(ea0, eb0, n[0]);
      for (int y = 0; y < n[1]; ++y) { /* the invariance it rests on */
        const bs_rw_row r = bs_rw_setup(ea0 + y * asx, eb0 + y * bsx, n[0]);
        if (r.ha != r0.ha || r.de != r0.de || r.nch != r0.nch ||
            r.ac0 * 8 != r0.ac0 * 8 + y * asx ||
            r.bc0 * 8 != r0.bc0 * 8 + y * bsx)
          fail("row phase not invariant under a stride multiple of 8");
      }
      cnt = 0;
      for (int k = 0; k < r0.nch; ++k) {
        const bs_rd_lane h = bs_rd_hoist(r0, k);
        if (!(h.m0 | h.m1 | h.m2 | h.m3)) fail("hoisted chunk without mask");
        for (int y = 0; y < n[1]; ++y) {
          guard(acc, hst, cnt, 1);
          bs_rd_consume_h(
              bs_rd_fetch(a.v->p, b.v->p, h, y * asx, y * bsx), h, acc);
        }
      }
      bs_rd_widen(acc, hst);
    }
  }
  for (int q = 0; q < 5; ++q)
    if (ref[q] != row[q] || (hoist && ref[q] != hst[q])) {
      if (failures < 20)
        fprintf(stderr,
                "mismatch sum %d: wa=%d wb=%d oxa=%d oxb=%d s=(%d,%d,%d) "
                "n=(%d,%d,%d) ref=%llu per-row=%llu hoisted=%llu\n",
                q, a.v->w, b.v->w, a.ox, b.ox, sx, sy, sz, n[0], n[1], n[2],
                (unsigned long long)ref[q], (unsigned long long)row[q],
                (unsigned long long)hst[q]);
      ++failures;
    }
}

static void sweep(int wa, int wb, bool all_max) {
  const int oxs[3] = {0, 1, 3};
  view va = make_view(wa, 5, 3, all_max), vb = make_view(wb, 5, 3, all_max);
  /* whole views: boxes that touch the first and the last voxel of either
   * buffer */
  const region fa = {&va, 0, 0, 0, wa, 5, 3};
  const region fb = {&vb, 0, 0, 0, wb, 5, 3};
  for (int sx = -9; sx <= 9; ++sx)
    for (int sy = -1; sy <= 1; ++sy)
      for (int sz = -1; sz <= 1; ++sz) run_case(fa, fb, sx, sy, sz);
  /* sub-boxes: every ox, every sx residue mod 8 in both signs, nx from 1
   * to 20; the last rows and planes of the views included */
  for (int oxa : oxs)
    for (int oxb : oxs)
      for (int sx = -9; sx <= 9; ++sx)
        for (int nx = 1; nx <= 20; ++nx) {
          const int ax = sx >= 0 ? nx : nx - sx;
          const int bx = sx >= 0 ? nx + sx : nx;
          const region ra = {&va, oxa, 1, 1, ax, 4, 2};
          const region rb = {&vb, oxb, 1, 1, bx, 4, 2};
          run_case(ra, rb, sx, 0, 0);
          run_case(ra, rb, sx, 1, -1);
          run_case(ra, rb, sx, -2, 1);
        }
  /* widest boxes an offset leaves, up to the view's right edge */
  for (int oxa : oxs)
    for (int oxb : oxs)
      for (int sx = -9; sx <= 9; ++sx) {
        const region ra = {&va, oxa, 0, 0, wa - oxa, 5, 3};
        const region rb = {&vb, oxb, 0, 0, wb - oxb, 5, 3};
        run_case(ra, rb, sx, 0, 0);
        run_case(ra, rb, sx, -1, 1);
      }
  free(va.p);
  free(vb.p);
}

static void check_perm() {
  /* result byte i = byte sel[i] of hi:lo */
  const uint32_t lo = 0x33221100u, hi = 0x77665544u;
  if (bs_rd_perm(hi, lo, BS_RD_SEL_LO) != 0x66442200u) fail("perm SEL_LO");
  if (bs_rd_perm(hi, lo, BS_RD_SEL_HI) != 0x77553311u) fail("perm SEL_HI");
  if (bs_rd_perm(hi, lo, 0x03020100u) != lo) fail("perm identity lo");
  if (bs_rd_perm(hi, lo, 0x07060504u) != hi) fail("perm identity hi");
  /* on four u16 e0..e3 packed as the chunk's dwords */
  const uint32_t e[4] = {0x1234u, 0xABCDu, 0xFF01u, 0x80FEu};
  const uint32_t d0 = e[0] | (e[1] << 16), d1 = e[2] | (e[3] << 16);
  const uint32_t l = bs_rd_perm(d1, d0, BS_RD_SEL_LO);
  const uint32_t h = bs_rd_perm(d1, d0, BS_RD_SEL_HI);
  for (int i = 0; i < 4; ++i) {
    if (((l >> (8 * i)) & 0xFFu) != (e[i] & 0xFFu)) fail("low byte gather");
    if (((h >> (8 * i)) & 0xFFu) != (e[i] >> 8)) fail("high byte gather");
  }
  if (bs_rd_dot4(0x04030201u, 0x08070605u, 10u) != 10u + 5 + 12 + 21 + 32)
    fail("dot4");
  if (bs_rd_dot4(0xFFFFFFFFu, 0xFFFFFFFFu, 0u) != 4u * 255u * 255u)
    fail("dot4 max");
}

/* `chunks` all-65535 chunks into one accumulator set; guarded = with the
 * kernel's early widening in batches of `batch` */
static void max_chunks(long chunks, bool guarded, int batch, uint64_t s[5],
                       uint32_t *ab_x_before_widen) {
  bs_rw_v4 f;
  for (int i = 0; i < 4; ++i) f.d[i] = 0xFFFFFFFFu;
  bs_rd_acc acc;
  bs_rd_zero(acc);
  int n = 0;
  for (int q = 0; q < 5; ++q) s[q] = 0;
  for (long c = 0; c < chunks; c += batch) {
    const int nb = (int)std::min<long>(batch, chunks - c);
    if (guarded) guard(acc, s, n, batch);
    for (int i = 0; i < nb; ++i)
      bs_rd_consume_m(f, f, f, 0, ~0u, ~0u, ~0u, ~0u, acc);
  }
  if (ab_x_before_widen) *ab_x_before_widen = acc.ab_x;
  bs_rd_widen(acc, s);
}

static bool sums_exact(const uint64_t s[5], long chunks) {
  const uint64_t n = 8ull * (uint64_t)chunks, m = 65535ull;
  return s[0] == n * m && s[1] == n * m && s[2] == n * m * m &&
         s[3] == n * m * m && s[4] == n * m * m;
}

static void check_bound() {
  uint64_t s[5];
  uint32_t x = 0;
  /* the bound itself: exact with no widening in between */
  max_chunks(BS_RD_MAX_CHUNKS, false, 1, s, &x);
  if (!sums_exact(s, BS_RD_MAX_CHUNKS)) fail("4128 max chunks not exact");
  if (x != 4294771200u) fail("cross accumulator at the bound");
  /* ... and it is tight: the next chunk does not fit the fastest
   * accumulator, and unguarded it is indeed lost */
  if ((uint64_t)x + 8ull * 130050ull <= 0xFFFFFFFFull)
    fail("bound not tight");
  max_chunks(BS_RD_MAX_CHUNKS + 1, false, 1, s, nullptr);
  if (sums_exact(s, BS_RD_MAX_CHUNKS + 1)) fail("4129 chunks did not wrap");
  /* the guard covers it, for every batch size the kernel uses */
  for (int batch = 1; batch <= 3; ++batch)
    for (long chunks : {(long)BS_RD_MAX_CHUNKS + 1, 3L * BS_RD_MAX_CHUNKS + 5,
                        20000L}) {
      max_chunks(chunks, true, batch, s, &x);
      if (!sums_exact(s, chunks)) fail("guarded walk past the bound");
    }
}

int main() {
  check_perm();
  check_bound();
  const int widths[2] = {37, 40};
  for (int wa : widths)
    for (int wb : widths) {
      sweep(wa, wb, false);
      sweep(wa, wb, true); /* all-65535 data */
    }
  if (!hoisted_cases) fail("no case took the hoisted walk");
  printf("rtest_dot_host: %ld cases (%ld hoisted), %ld failures\n", cases,
         hoisted_cases, failures);
  return failures ? 1 : 0;
}
