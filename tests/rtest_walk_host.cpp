/* Host run of the r-test's 16-byte row walk (csrc/rtest_walk.h), meant to
 * be built with -fsanitize=address,undefined: the views live in heap
 * blocks of exactly n*2 bytes rounded up to 16, so any chunk load outside
 * an allocation is reported. The five sums of every case are compared
 * with a naive triple loop. Exit 0 = all cases equal. */
#include "../bigstitcher_spark_amd/csrc/rtest_walk.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

struct view {
  unsigned short *p;
  int w, h, d;
};

static uint32_t rng_state = 12345u;
static uint32_t rnd() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}

static view make_view(int w, int h, int d) {
  const size_t n = (size_t)w * h * d;
  const size_t bytes = (n * 2 + 15) & ~(size_t)15;
  view v = {(unsigned short *)aligned_alloc(16, bytes), w, h, d};
  if (!v.p) abort();
  for (size_t i = 0; i < bytes / 2; ++i) {
    const uint32_t r = rnd();
    /* a good share of 65535 (the overflow bound); the pad past n is
     * 0xFFFF too, so a masking slip shows in the sums */
    v.p[i] = i >= n || (r & 3) == 0 ? 65535 : (unsigned short)(r >> 2);
  }
  return v;
}

struct region { /* sub-box of a view, as bs_region */
  const view *v;
  int ox, oy, oz, mx, my, mz;
};

static long cases = 0, failures = 0;

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
  uint64_t ref[5] = {0, 0, 0, 0, 0}, got[5] = {0, 0, 0, 0, 0};
  for (int z = lo[2]; z < lo[2] + n[2]; ++z)
    for (int y = 0; y < n[1]; ++y) {
      /* row bases exactly as k_rtest_wide forms them */
      const long ea = (a.oz + z) * asxy + (a.oy + lo[1] + y) * asx + a.ox +
                      lo[0];
      const long eb = (b.oz + z + sz) * bsxy +
                      (b.oy + lo[1] + sy + y) * bsx + b.ox + lo[0] + sx;
      for (int x = 0; x < n[0]; ++x) {
        const uint64_t av = a.v->p[ea + x], bv = b.v->p[eb + x];
        ref[0] += av;
        ref[1] += bv;
        ref[2] += av * av;
        ref[3] += bv * bv;
        ref[4] += av * bv;
      }
      const bs_rw_row r = bs_rw_setup(ea, eb, n[0]);
      int rw = 1; /* lanes per row: also walk the idle lanes' k >= nch */
      while (rw < bs_rw_max_chunks(n[0]) && rw < 64) rw <<= 1;
      if (r.nch > bs_rw_max_chunks(n[0])) ++failures;
      /* which B chunks a step may load, against plain enumeration: B
       * chunk c is wanted iff a live pair's B element lies in it */
      for (int k = 0; k < r.nch; ++k) {
        bool want_lo = false, want_hi = false;
        for (int x = 0; x < n[0]; ++x)
          if (((ea + x) >> 3) == r.ac0 + k) {
            want_lo |= ((eb + x) >> 3) == r.bc0 + k;
            want_hi |= ((eb + x) >> 3) == r.bc0 + k + 1;
            if (((eb + x) >> 3) < r.bc0 + k || ((eb + x) >> 3) > r.bc0 + k + 1)
              ++failures;
          }
        const unsigned m = bs_rw_mask(r, k);
        if (want_lo != bs_rw_need_lo(r.de, m) ||
            want_hi != bs_rw_need_hi(r.de, m) || !(want_lo || want_hi))
          ++failures;
      }
      for (int k = 0; k < std::max(rw, r.nch); ++k)
        bs_rw_consume(bs_rw_fetch(a.v->p, b.v->p, r, k), r.de, got);
    }
  for (int q = 0; q < 5; ++q)
    if (ref[q] != got[q]) {
      if (failures < 20)
        fprintf(stderr,
                "mismatch sum %d: wa=%d wb=%d oxa=%d oxb=%d s=(%d,%d,%d) "
                "n=(%d,%d,%d) ref=%llu got=%llu\n",
                q, a.v->w, b.v->w, a.ox, b.ox, sx, sy, sz, n[0], n[1], n[2],
                (unsigned long long)ref[q], (unsigned long long)got[q]);
      ++failures;
    }
}

int main() {
  const int widths[2] = {37, 40};
  const int oxs[3] = {0, 1, 3};
  for (int wa : widths)
    for (int wb : widths) {
      view va = make_view(wa, 5, 3), vb = make_view(wb, 5, 3);
      /* whole views: boxes that touch the first and the last voxel of
       * either buffer */
      const region fa = {&va, 0, 0, 0, wa, 5, 3};
      const region fb = {&vb, 0, 0, 0, wb, 5, 3};
      for (int sx = -9; sx <= 9; ++sx)
        for (int sy = -1; sy <= 1; ++sy)
          for (int sz = -1; sz <= 1; ++sz) run_case(fa, fb, sx, sy, sz);
      /* sub-boxes: every ox, every sx residue mod 8 in both signs, nx
       * from 1 to 20; the last rows and planes of the views included */
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
  printf("rtest_walk_host: %ld cases, %ld failures\n", cases, failures);
  return failures ? 1 : 0;
}
