/* Host emulation of the radix-4 / radix-8 x-pass FFT schedule
 * (bigstitcher_spark_amd/csrc/xfft_r4.h, the functions k_fft_x_fwd_r4 and
 * k_fft_x_inv_r4 call): one wave = a loop over 64 lanes per stage, the
 * wave-private LDS buffer = an array. Built with -fsanitize=address,
 * undefined by tests/test_xfft_r4_cpu.py; no GPU, no library.
 *
 * Checked at h = 256 (E = 4) and h = 512 (E = 8), both directions, against
 * a double-precision naive DFT:
 *   forward  uint16 rows (random, all 0, all 65535, 0/65535 mix, a partial
 *            row with zero fill) -> the n/2+1 half spectrum,
 *   inverse  random Hermitian half spectra -> the real row.
 * Error bound: a plain radix-2 f32 FFT (the arithmetic of ffth_wave) runs
 * on the same inputs with the same unpack / pre-process; the new core's
 * error must stay within 2x of it, case by case. Both are printed.
 * Schedule properties asserted on the way: every LDS index is inside the
 * wave's buffer, every exchange writes each slot exactly once before any
 * read, every read slot was written, the last stage's destination is the
 * register order, and the bank-conflict degree of every LDS access
 * pattern under the two bank rules is <= 2 (1 for the exchanges). */
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../bigstitcher_spark_amd/csrc/xfft_r4.h"

struct c2 { float x, y; };
struct d2 { double x, y; };

static int g_fail = 0;
#define CHECK(cond, ...)                                                    \
  do {                                                                      \
    if (!(cond)) {                                                          \
      if (++g_fail <= 20) {                                                 \
        printf("FAIL %s:%d: ", __FILE__, __LINE__);                         \
        printf(__VA_ARGS__);                                                \
        printf("\n");                                                       \
      }                                                                     \
    }                                                                       \
  } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
  g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
  return (uint32_t)(g_rng >> 16);
}
static float rndf() { return (float)((rnd() & 0xFFFFFF) / 8388608.0 - 1.0); }

/* twn[k] = e^{-2 pi i k / n}, k < n/2 (the device's half-circle table) */
static std::vector<c2> make_twn(int n) {
  std::vector<c2> t(n / 2);
  for (int k = 0; k < n / 2; ++k) {
    double a = -2.0 * M_PI * k / n;
    t[k] = {(float)cos(a), (float)sin(a)};
  }
  return t;
}

/* ---- the emulated wave ---- */
template <int E, int DIR>
static void wave_fft(std::vector<c2> &z, const std::vector<c2> &twn) {
  constexpr int h = xf_geom<E>::H, NS = xf_geom<E>::NS;
  std::vector<c2> lds(h); /* exactly the wave's buffer: ASan guards it */
  std::vector<int> stamp(h);
  c2 v[64][E];
  xf_twset<E, c2> tw[64];
  for (int l = 0; l < 64; ++l) {
    xf_load_tw<E>(tw[l], twn.data(), l, DIR);
    for (int r = 0; r < E; ++r) v[l][r] = z[l + 64 * r];
  }
  for (int si = 0; si < NS; ++si) {
    const int L = xf_L<E>(si);
    for (int l = 0; l < 64; ++l) xf_stage<E, DIR>(v[l], tw[l], si);
    if (si == NS - 1) {
      CHECK(L == 64, "last stage L=%d", L);
      for (int l = 0; l < 64; ++l)
        for (int s = 0; s < E; ++s)
          CHECK(xf_dst<E>(L, l, s) == l + 64 * s,
                "last stage dst(%d,%d)=%d", l, s, xf_dst<E>(L, l, s));
      break;
    }
    for (int i = 0; i < h; ++i) stamp[i] = 0;
    for (int l = 0; l < 64; ++l)
      for (int s = 0; s < E; ++s) {
        const int m = xf_swz<E>(xf_dst<E>(L, l, s));
        CHECK(m >= 0 && m < h, "write index %d outside [0,%d)", m, h);
        if (m < 0 || m >= h) continue;
        CHECK(stamp[m] == 0, "stage L=%d slot %d written twice", L, m);
        stamp[m]++;
        lds[m] = v[l][s];
      }
    for (int i = 0; i < h; ++i)
      CHECK(stamp[i] == 1, "stage L=%d slot %d written %d times", L, i,
            stamp[i]);
    for (int l = 0; l < 64; ++l)
      for (int r = 0; r < E; ++r) {
        const int m = xf_swz<E>(l + 64 * r);
        CHECK(m >= 0 && m < h, "read index %d outside [0,%d)", m, h);
        if (m < 0 || m >= h) continue;
        CHECK(stamp[m] == 1, "read of unwritten slot %d", m);
        v[l][r] = lds[m];
      }
  }
  for (int l = 0; l < 64; ++l)
    for (int r = 0; r < E; ++r) z[l + 64 * r] = v[l][r];
}

/* the kernels' mirror exchange: plain layout, write l + 64 e, read
 * xf_mirror(l + 64 e) */
template <int E>
static void wave_mirror(const std::vector<c2> &z, std::vector<c2> &zm) {
  constexpr int h = xf_geom<E>::H;
  std::vector<c2> lds(h);
  std::vector<int> stamp(h, 0);
  for (int l = 0; l < 64; ++l)
    for (int e = 0; e < E; ++e) {
      const int m = l + 64 * e;
      CHECK(stamp[m] == 0, "mirror slot %d written twice", m);
      stamp[m]++;
      lds[m] = z[m];
    }
  for (int l = 0; l < 64; ++l)
    for (int e = 0; e < E; ++e) {
      const int m = xf_mirror<E>(l + 64 * e);
      CHECK(m >= 0 && m < h, "mirror index %d outside [0,%d)", m, h);
      if (m < 0 || m >= h) continue;
      CHECK(stamp[m] == 1, "mirror read of unwritten slot %d", m);
      zm[l + 64 * e] = lds[m];
    }
}

/* ---- plain radix-2 f32 DIT FFT: the arithmetic of ffth_wave ---- */
static void r2_fft(std::vector<c2> &z, const std::vector<c2> &twn, int dir) {
  const int h = (int)z.size();
  int lg = 0;
  while ((1 << lg) < h) ++lg;
  std::vector<c2> a(h);
  for (int i = 0; i < h; ++i) {
    int r = 0;
    for (int b = 0; b < lg; ++b) r |= ((i >> b) & 1) << (lg - 1 - b);
    a[i] = z[r];
  }
  for (int s = 1; s < h; s <<= 1)
    for (int i = 0; i < h; ++i) {
      if (i & s) continue;
      c2 w = twn[2 * ((i & (s - 1)) * ((h / 2) / s))]; /* tw_h[k]=twn[2k] */
      if (dir < 0) w.y = -w.y;
      const c2 wb = xf_cmul(a[i + s], w), p = a[i];
      a[i] = {p.x + wb.x, p.y + wb.y};
      a[i + s] = {p.x - wb.x, p.y - wb.y};
    }
  z = a;
}

/* ---- forward: uint16 row (mx valid, zero fill) -> X[0..h] ---- */
template <int E, bool NEW>
static std::vector<c2> fwd_row(const std::vector<uint16_t> &row, int mx,
                               const std::vector<c2> &twn) {
  constexpr int h = xf_geom<E>::H;
  std::vector<c2> z(h), zm(h), X(h + 1);
  for (int j = 0; j < h; ++j)
    z[j] = {2 * j < mx ? (float)row[2 * j] : 0.0f,
            2 * j + 1 < mx ? (float)row[2 * j + 1] : 0.0f};
  if (NEW) {
    wave_fft<E, +1>(z, twn);
    wave_mirror<E>(z, zm);
  } else {
    r2_fft(z, twn, +1);
    for (int k = 0; k < h; ++k) zm[k] = z[(h - k) & (h - 1)];
  }
  xf_unpack0(z[0], X[0], X[h]);
  for (int k = 1; k < h; ++k) X[k] = xf_unpack(z[k], zm[k], twn[k]);
  return X;
}

/* ---- inverse: X[0..h] Hermitian half spectrum -> real row of n ---- */
template <int E, bool NEW>
static std::vector<float> inv_row(const std::vector<c2> &X,
                                  const std::vector<c2> &twn) {
  constexpr int h = xf_geom<E>::H;
  std::vector<c2> z(h);
  for (int k = 0; k < h; ++k) z[k] = xf_prep(X[k], X[h - k], twn[k]);
  if (NEW)
    wave_fft<E, -1>(z, twn);
  else
    r2_fft(z, twn, -1);
  std::vector<float> x(2 * h);
  for (int j = 0; j < h; ++j) { x[2 * j] = z[j].x; x[2 * j + 1] = z[j].y; }
  return x;
}

/* ---- bank conflicts ---- */
static int conflict_degree(const int *m, int group, int nbank8) {
  /* m: 64 element indices (8-byte elements); bank pair = m % nbank8 */
  int worst = 1;
  for (int g = 0; g < 64; g += group)
    for (int b = 0; b < nbank8; ++b) {
      int distinct = 0, seen[64];
      for (int l = g; l < g + group; ++l) {
        if (m[l] % nbank8 != b) continue;
        bool dup = false;
        for (int i = 0; i < distinct; ++i) dup |= seen[i] == m[l];
        if (!dup) seen[distinct++] = m[l];
      }
      if (distinct > worst) worst = distinct;
    }
  return worst;
}
/* ds_write_b64: 4 x 16 contiguous lanes, bank (a/4) mod 32 -> m mod 16;
 * ds_read_b64: 2 x 32 lanes, bank (a/4) mod 64 -> m mod 32 */
static int wr_degree(const int *m) { return conflict_degree(m, 16, 16); }
static int rd_degree(const int *m) { return conflict_degree(m, 32, 32); }

template <int E>
static void bank_table() {
  constexpr int h = xf_geom<E>::H, NS = xf_geom<E>::NS;
  int m[64];
  printf("bank conflicts h=%d (degree; 1 = conflict-free)\n", h);
  for (int si = 0; si + 1 < NS; ++si) {
    const int L = xf_L<E>(si);
    printf("  write L=%-3d s=0..%d:", L, E - 1);
    for (int s = 0; s < E; ++s) {
      for (int l = 0; l < 64; ++l) m[l] = xf_swz<E>(xf_dst<E>(L, l, s));
      const int d = wr_degree(m);
      printf(" %d", d);
      CHECK(d == 1, "h=%d write L=%d s=%d degree %d", h, L, s, d);
    }
    printf("\n");
  }
  printf("  read  l+64r r=0..%d:", E - 1);
  for (int r = 0; r < E; ++r) {
    for (int l = 0; l < 64; ++l) m[l] = xf_swz<E>(l + 64 * r);
    const int d = rd_degree(m);
    printf(" %d", d);
    CHECK(d == 1, "h=%d read r=%d degree %d", h, r, d);
  }
  printf("\n  mirror write / read e=0..%d:", E - 1);
  for (int e = 0; e < E; ++e) {
    for (int l = 0; l < 64; ++l) m[l] = l + 64 * e;
    const int dw = wr_degree(m);
    for (int l = 0; l < 64; ++l) m[l] = xf_mirror<E>(l + 64 * e);
    const int dr = rd_degree(m);
    printf(" %d/%d", dw, dr);
    CHECK(dw <= 2 && dr <= 2, "h=%d mirror e=%d degree %d/%d", h, e, dw, dr);
  }
  printf("\n");
  /* the swizzle is a bijection of [0, h) */
  std::vector<int> hit(h, 0);
  for (int i = 0; i < h; ++i) {
    const int s = xf_swz<E>(i);
    CHECK(s >= 0 && s < h, "swz(%d)=%d", i, s);
    if (s >= 0 && s < h) hit[s]++;
  }
  for (int i = 0; i < h; ++i) CHECK(hit[i] == 1, "swz not bijective at %d", i);
}

/* ---- cases ---- */
template <int E>
static void run_size() {
  constexpr int h = xf_geom<E>::H, n = 2 * h;
  const std::vector<c2> twn = make_twn(n);
  bank_table<E>();

  const char *names[5] = {"random", "zeros", "all 65535", "0/65535 mix",
                          "partial+zero fill"};
  for (int c = 0; c < 5; ++c) {
    std::vector<uint16_t> row(n);
    int mx = n;
    for (int i = 0; i < n; ++i)
      row[i] = c == 0 || c == 4 ? (uint16_t)rnd()
               : c == 1         ? 0
               : c == 2         ? 65535
                                : ((rnd() & 1) ? 65535 : 0);
    if (c == 4) mx = n / 2 + 44 + 1; /* odd: the last pair is half filled */
    std::vector<d2> ref(h + 1);
    double scale = 0.0;
    for (int k = 0; k <= h; ++k) {
      double sr = 0.0, sim = 0.0;
      for (int i = 0; i < mx; ++i) {
        const double a = -2.0 * M_PI * (double)((long)k * i % n) / n;
        sr += row[i] * cos(a);
        sim += row[i] * sin(a);
      }
      ref[k] = {sr, sim};
      scale = fmax(scale, hypot(sr, sim));
    }
    const std::vector<c2> Xn = fwd_row<E, true>(row, mx, twn);
    const std::vector<c2> Xr = fwd_row<E, false>(row, mx, twn);
    double en = 0.0, er = 0.0;
    for (int k = 0; k <= h; ++k) {
      en = fmax(en, hypot(Xn[k].x - ref[k].x, Xn[k].y - ref[k].y));
      er = fmax(er, hypot(Xr[k].x - ref[k].x, Xr[k].y - ref[k].y));
    }
    if (scale > 0.0) { en /= scale; er /= scale; }
    printf("h=%d fwd %-18s err new %.3e  radix-2 %.3e\n", h, names[c], en,
           er);
    CHECK(en <= 2.0 * er, "h=%d fwd %s: %.3e > 2 * %.3e", h, names[c], en,
          er);
  }

  for (int c = 0; c < 3; ++c) {
    std::vector<c2> X(h + 1);
    for (int k = 0; k <= h; ++k) X[k] = {rndf(), rndf()};
    X[0].y = 0.0f;
    X[h].y = 0.0f;
    std::vector<double> ref(n);
    double scale = 0.0;
    for (int i = 0; i < n; ++i) {
      double s = X[0].x + ((i & 1) ? -1.0 : 1.0) * X[h].x;
      for (int k = 1; k < h; ++k) {
        const double a = 2.0 * M_PI * (double)((long)k * i % n) / n;
        s += 2.0 * (X[k].x * cos(a) - X[k].y * sin(a));
      }
      ref[i] = s;
      scale = fmax(scale, fabs(s));
    }
    const std::vector<float> xn = inv_row<E, true>(X, twn);
    const std::vector<float> xr = inv_row<E, false>(X, twn);
    double en = 0.0, er = 0.0;
    for (int i = 0; i < n; ++i) {
      en = fmax(en, fabs(xn[i] - ref[i]));
      er = fmax(er, fabs(xr[i] - ref[i]));
    }
    en /= scale;
    er /= scale;
    printf("h=%d inv random %d          err new %.3e  radix-2 %.3e\n", h, c,
           en, er);
    CHECK(en <= 2.0 * er, "h=%d inv %d: %.3e > 2 * %.3e", h, c, en, er);
  }
}

int main() {
  run_size<4>();
  run_size<8>();
  printf("xfft_r4_host: %d failures\n", g_fail);
  return g_fail ? 1 : 0;
}
