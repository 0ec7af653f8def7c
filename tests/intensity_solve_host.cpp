/* Host run of bs_intensity_solve and bsint::line_fit
 * (csrc/bs_intensity_solve.h), meant to be built by plain g++ with
 * -fsanitize=address,undefined: every array is a heap block of exactly its
 * size. Builds the moments of planted linear relations between three views
 * with 2x2x1 cells, and checks the line fit, the solved relation, the
 * unmatched view, the error answers and call-to-call identity.
 * Exit 0 = all passed. */
#include "../bigstitcher_spark_amd/csrc/bs_intensity_solve.h"

#include <cstdio>
#include <cstdlib>

static uint32_t rs = 2463534242u;
static uint32_t rnd() { /* xorshift32 */
  rs ^= rs << 13;
  rs ^= rs >> 17;
  rs ^= rs << 5;
  return rs;
}

static int failures = 0;
#define EXPECT(c)                                              \
  do {                                                         \
    if (!(c)) {                                                \
      ++failures;                                              \
      fprintf(stderr, "line %d: %s failed\n", __LINE__, #c);   \
    }                                                          \
  } while (0)

/* n samples P in 1/8 grey level, Q = round(gain * P + 8 * offset) */
static bs_intensity_match bucket(uint64_t ca, uint64_t cb, int n, double gain,
                                 double offset) {
  bs_intensity_match m;
  memset(&m, 0, sizeof m);
  m.cell_a = ca;
  m.cell_b = cb;
  m.n_cand = m.n_inl = m.n_inl_first = (uint64_t)n;
  for (int i = 0; i < n; ++i) {
    const uint64_t p = 8 * (400 + rnd() % 1600);
    const uint64_t q = (uint64_t)llround(gain * (double)p + 8.0 * offset);
    m.sp += p;
    m.sq += q;
    m.spp += p * p;
    m.sqq += q * q;
    m.spq += p * q;
  }
  return m;
}

int main() {
  /* line fit: exact on an exact line, refused without spread */
  {
    uint64_t n = 0, sp = 0, sq = 0, spp = 0, spq = 0;
    for (uint64_t p = 100; p < 200; p += 7) {
      const uint64_t q = 3 * p + 40;
      ++n; sp += p; sq += q; spp += p * p; spq += p * q;
    }
    double a = 0, b = 0;
    EXPECT(bsint::line_fit(n, sp, sq, spp, spq, &a, &b));
    EXPECT(a == 3.0 && b == 40.0);
    EXPECT(!bsint::line_fit(4, 400, 100, 40000, 10000, &a, &b));
    EXPECT(!bsint::line_fit(0, 0, 0, 0, 0, &a, &b));
    /* moments near the u64 bound do not overflow the exact products */
    const uint64_t big = 1ull << 24, pv = 524280;
    EXPECT(!bsint::line_fit(big, big * pv, big * pv, big * pv * pv,
                            big * pv * pv, &a, &b));
  }
  const int32_t cg[3] = {2, 2, 1};
  const size_t ncell = 4;
  const int nviews = 4; /* view 3 stays unmatched */
  const size_t npairs = 2, nm = 6;
  int32_t *pv = (int32_t *)malloc(npairs * 2 * sizeof(int32_t));
  size_t *po = (size_t *)malloc((npairs + 1) * sizeof(size_t));
  bs_intensity_match *mm =
      (bs_intensity_match *)malloc(nm * sizeof(bs_intensity_match));
  double *out = (double *)malloc(nviews * 2 * ncell * sizeof(double));
  double *out2 = (double *)malloc(nviews * 2 * ncell * sizeof(double));
  pv[0] = 0; pv[1] = 1; pv[2] = 1; pv[3] = 2;
  po[0] = 0; po[1] = 4; po[2] = 6;
  /* view 1 = 1.25 * view 0 + 150; view 2 = 0.8 * view 1 - 60 */
  mm[0] = bucket(1, 0, 900, 1.25, 150.0);
  mm[1] = bucket(1, 2, 300, 1.25, 150.0);
  mm[2] = bucket(3, 0, 500, 1.25, 150.0);
  mm[3] = bucket(3, 2, 1200, 1.25, 150.0);
  mm[4] = bucket(1, 0, 700, 0.8, -60.0);
  mm[5] = bucket(3, 2, 800, 0.8, -60.0);
  bs_intensity_solve_params prm = {0.01, 0.1, 1000, 0};
  int32_t iters = -1;
  double relres = -1.0;
  EXPECT(bs_intensity_solve(nviews, cg, pv, po, npairs, mm, &prm, out, &iters,
                            &relres) == BS_OK);
  EXPECT(iters > 0 && iters < 1000 && relres <= 1e-10);
  /* a matched bucket's two corrections agree on the data: with
   * q = g p + o, (a_i p + b_i) and (a_j q + b_j) are the same line up to
   * the regularisers' pull (they weigh 1 % of the data) */
  const double *v0 = out, *v1 = out + 2 * ncell, *v2 = out + 4 * ncell,
               *v3 = out + 6 * ncell;
  for (double p = 500; p <= 1900; p += 700) {
    const double q = 1.25 * p + 150.0;
    const double l = v0[1] * p + v0[ncell + 1], r = v1[0] * q + v1[ncell + 0];
    EXPECT(std::fabs(l - r) < 0.02 * p);
    const double t = 0.8 * q - 60.0;
    const double l2 = v1[1] * q + v1[ncell + 1], r2 = v2[0] * t + v2[ncell];
    EXPECT(std::fabs(l2 - r2) < 0.02 * q);
  }
  EXPECT(std::fabs(v0[1] - 1.0) > 0.02); /* something was corrected */
  for (size_t c = 0; c < ncell; ++c)
    EXPECT(v3[c] == 1.0 && v3[ncell + c] == 0.0);
  EXPECT(bs_intensity_solve(nviews, cg, pv, po, npairs, mm, &prm, out2,
                            nullptr, nullptr) == BS_OK);
  EXPECT(memcmp(out, out2, nviews * 2 * ncell * sizeof(double)) == 0);
  /* no pairs: identity, zero iterations */
  EXPECT(bs_intensity_solve(nviews, cg, nullptr, nullptr, 0, nullptr, &prm,
                            out2, &iters, nullptr) == BS_OK);
  EXPECT(iters == 0 && out2[0] == 1.0 && out2[ncell] == 0.0);
  /* errors */
  const int32_t bad_cg[3] = {2, 0, 1};
  EXPECT(bs_intensity_solve(nviews, bad_cg, pv, po, npairs, mm, &prm, out2,
                            nullptr, nullptr) == BS_EINVAL);
  EXPECT(bs_intensity_solve(2, cg, pv, po, npairs, mm, &prm, out2, nullptr,
                            nullptr) == BS_EINVAL); /* view 2 out of range */
  mm[5].cell_b = 4;
  EXPECT(bs_intensity_solve(nviews, cg, pv, po, npairs, mm, &prm, out2,
                            nullptr, nullptr) == BS_EINVAL);
  prm.max_iterations = 0;
  EXPECT(bs_intensity_solve(nviews, cg, pv, po, 1, mm, &prm, out2, nullptr,
                            nullptr) == BS_EINVAL);
  free(pv);
  free(po);
  free(mm);
  free(out);
  free(out2);
  if (failures) {
    fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  printf("intensity_solve_host: all checks passed\n");
  return 0;
}
