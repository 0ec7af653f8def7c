/* Host run of bs_ransac (csrc/bs_ransac.h), meant to be built by plain g++
 * with -fsanitize=address,undefined: every array is a heap block of exactly
 * its size. Plants a translation, a rigid and an affine transform with
 * 40 % gross outliers, and checks the inlier mask, the model, the
 * no-consensus answer and call-to-call identity. Exit 0 = all passed. */
#include "../bigstitcher_spark_amd/csrc/bs_ransac.h"

#include <cstdio>
#include <cstdlib>

static uint32_t rs = 2463534242u;
static double rnd() { /* xorshift32 -> [0, 1) */
  rs ^= rs << 13;
  rs ^= rs >> 17;
  rs ^= rs << 5;
  return rs / 4294967296.0;
}

static int failures = 0;
#define EXPECT(c)                                              \
  do {                                                         \
    if (!(c)) {                                                \
      ++failures;                                              \
      fprintf(stderr, "line %d: %s failed\n", __LINE__, #c);   \
    }                                                          \
  } while (0)

static void run(int model, int reg, const double T[12], size_t n,
                size_t n_out) {
  double *pa = (double *)malloc(n * 3 * sizeof(double));
  double *pb = (double *)malloc(n * 3 * sizeof(double));
  uint8_t *m1 = (uint8_t *)malloc(n), *m2 = (uint8_t *)malloc(n);
  for (size_t i = 0; i < n; ++i) {
    double *a = pa + 3 * i, *b = pb + 3 * i;
    for (int d = 0; d < 3; ++d) a[d] = rnd() * 200.0;
    for (int r = 0; r < 3; ++r)
      b[r] = T[4 * r] * a[0] + T[4 * r + 1] * a[1] + T[4 * r + 2] * a[2] +
             T[4 * r + 3];
    if (i % 5 < 2 && i / 5 * 2 + i % 5 < n_out) /* gross outlier */
      for (int d = 0; d < 3; ++d) b[d] += 40.0 + rnd() * 100.0;
  }
  bs_ransac_params p = {model, reg, 0.1, 0.5, 0.1, 12, 2000};
  double M1[12], M2[12];
  size_t k1 = 0, k2 = 0;
  EXPECT(bs_ransac(pa, pb, n, &p, m1, M1, &k1) == BS_OK);
  EXPECT(bs_ransac(pa, pb, n, &p, m2, M2, &k2) == BS_OK);
  EXPECT(k1 == k2 && memcmp(m1, m2, n) == 0 && memcmp(M1, M2, sizeof(M1)) == 0);
  size_t want = 0;
  for (size_t i = 0; i < n; ++i) {
    const bool out = i % 5 < 2 && i / 5 * 2 + i % 5 < n_out;
    want += !out;
    EXPECT(m1[i] == (out ? 0 : 1));
  }
  EXPECT(k1 == want);
  for (int i = 0; i < 12; ++i) {
    if (!(std::fabs(M1[i] - T[i]) < 1e-6))
      fprintf(stderr, "model %d reg %d entry %d: %.9g want %.9g\n", model, reg,
              i, M1[i], T[i]);
    EXPECT(std::fabs(M1[i] - T[i]) < 1e-6);
  }
  /* optional outputs may be NULL; n == 0 and n below the minimal set */
  EXPECT(bs_ransac(pa, pb, n, &p, nullptr, nullptr, &k2) == BS_OK && k2 == k1);
  EXPECT(bs_ransac(pa, pb, 0, &p, m2, M2, &k2) == BS_OK && k2 == 0);
  EXPECT(bs_ransac(pa, pb, 1, &p, m2, M2, &k2) == BS_OK && k2 == 0);
  free(pa);
  free(pb);
  free(m1);
  free(m2);
}

int main() {
  const double Tt[12] = {1, 0, 0, 7.3, 0, 1, 0, -4.6, 0, 0, 1, 2.2};
  const double c = std::cos(0.3), s = std::sin(0.3);
  const double Tr[12] = {c, -s, 0, 5, s, c, 0, -3, 0, 0, 1, 2};
  const double Ta[12] = {1.02, 0.01, 0, 5, -0.02, 0.97, 0.03, -3,
                         0.01, 0, 1.05, 2};
  run(BS_MODEL_TRANSLATION, BS_MODEL_NONE, Tt, 100, 40);
  run(BS_MODEL_RIGID, BS_MODEL_NONE, Tr, 100, 40);
  run(BS_MODEL_AFFINE, BS_MODEL_NONE, Ta, 100, 40);
  run(BS_MODEL_AFFINE, BS_MODEL_RIGID, Tr, 60, 0); /* [PIN-INTERP] */
  /* pure noise: nothing accepted */
  {
    const size_t n = 80;
    double *pa = (double *)malloc(n * 3 * sizeof(double));
    double *pb = (double *)malloc(n * 3 * sizeof(double));
    uint8_t *m = (uint8_t *)malloc(n);
    for (size_t i = 0; i < 3 * n; ++i) {
      pa[i] = rnd() * 200.0;
      pb[i] = rnd() * 200.0;
    }
    bs_ransac_params p = {BS_MODEL_AFFINE, BS_MODEL_RIGID, 0.1, 0.5, 0.1, 12,
                          500};
    double M[12];
    size_t k = 99;
    EXPECT(bs_ransac(pa, pb, n, &p, m, M, &k) == BS_OK && k == 0);
    for (size_t i = 0; i < n; ++i) EXPECT(m[i] == 0);
    p.model = 7;
    EXPECT(bs_ransac(pa, pb, n, &p, m, M, &k) == BS_EINVAL);
    free(pa);
    free(pb);
    free(m);
  }
  printf("ransac_host: %d failures\n", failures);
  return failures ? 1 : 0;
}
