/* Host emulation of the strided-pass radix-8 FFT schedule at n = 512
 * (bigstitcher_spark_amd/csrc/sfft_r8.h, the functions k_fft_pass_r8 and
 * k_fft_z_fused_r8x call): one workgroup = loops over 256 threads between
 * the kernel's barriers, the exchange tile = a heap array of exactly
 * SF_TILE quads. Built with -fsanitize=address,undefined by
 * tests/test_sfft_r8_cpu.py; no GPU, no library.
 *
 * A block barrier is the end of a loop over all 256 threads; a wave-level
 * sync is the end of a loop over one wave's 64 threads, and the wave-private
 * exchanges run wave after wave, each one's write AND read before the next
 * wave starts, so they pass only if they really stay inside the owner's
 * slice.
 *
 * Asserted on the way: every exchange index is inside the tile (inside the
 * owner's slice for the wave-private exchanges), every slot is written
 * exactly once before it is read, the I/O mapping covers every (pair, row)
 * once, the last stage's destination is the I/O order, the slot map is a
 * bijection, and every LDS access pattern is conflict-free under the
 * 16-byte lane-group rules. Accuracy: against a double-precision DFT, with
 * the error of a plain radix-2 f32 FFT on the same input as the bar (2x). */
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../bigstitcher_spark_amd/csrc/sfft_r8.h"

struct c2 { float x, y; };
struct q4 { float x, y, z, w; };
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

constexpr int N = SF_N, NT = SF_THREADS, NCOL = 2 * SF_PAIRS;

/* twn[k] = e^{-2 pi i k / 1024}, k < 512 (the device's half-circle table
 * of length 2 n) */
static std::vector<c2> make_twn() {
  std::vector<c2> t(N);
  for (int k = 0; k < N; ++k) {
    double a = -2.0 * M_PI * k / (2 * N);
    t[k] = {(float)cos(a), (float)sin(a)};
  }
  return t;
}

/* ---- the exchange tile, with the checks a race would break ---- */
struct Tile {
  std::vector<q4> data;   /* exactly the kernel's tile: ASan guards it */
  std::vector<int> stamp; /* writes since begin() */
  int lo = 0, hi = SF_TILE; /* the slots the running threads may touch */
  const char *what = "";
  Tile() : data(SF_TILE), stamp(SF_TILE, 0) {}
  void begin(const char *w) {
    what = w;
    for (int &s : stamp) s = 0;
    lo = 0;
    hi = SF_TILE;
  }
  void restrict_to_pair(int p) { lo = SF_N * p; hi = SF_N * p + SF_N; }
  void unrestrict() { lo = 0; hi = SF_TILE; }
  void all_written_once(int from, int to) const {
    for (int i = from; i < to; ++i)
      CHECK(stamp[i] == 1, "%s: slot %d written %d times", what, i, stamp[i]);
  }
  struct Ref {
    Tile *t;
    int i;
    bool ok() const {
      CHECK(i >= 0 && i < SF_TILE, "%s: index %d outside the tile", t->what, i);
      if (i < 0 || i >= SF_TILE) return false;
      CHECK(i >= t->lo && i < t->hi, "%s: index %d outside slice [%d,%d)",
            t->what, i, t->lo, t->hi);
      return true;
    }
    void operator=(const q4 &q) {
      if (!ok()) return;
      CHECK(t->stamp[i] == 0, "%s: slot %d written twice", t->what, i);
      t->stamp[i]++;
      t->data[i] = q;
    }
    operator q4() const {
      if (!ok()) return q4{0, 0, 0, 0};
      CHECK(t->stamp[i] == 1, "%s: read of slot %d written %d times", t->what,
            i, t->stamp[i]);
      return t->data[i];
    }
  };
  struct Handle {
    Tile *t;
    Ref operator[](int i) const { return Ref{t, i}; }
  };
  Handle h() { return Handle{this}; }
};

typedef sf_lines<c2> lines;

struct Block {
  Tile tile;
  std::vector<c2> twt; /* the workgroup's twiddle table, exactly SF_TWN */
  explicit Block(const std::vector<c2> &twn) : twt(SF_TWN) {
    for (int i = 0; i < SF_TWN; ++i) twt[i] = sf_tw_entry(twn.data(), i);
    /* every (stage, lane) reads the forward twiddles of xf_load_tw<8> */
    for (int l = 0; l < 64; ++l) {
      xf_twset<8, c2> ref;
      xf_load_tw<8>(ref, twn.data(), l, +1);
      for (int si = 1; si <= 2; ++si) {
        c2 w[7];
        sf_get_tw(twt.data(), si, l, w);
        for (int r = 0; r < 7; ++r)
          CHECK(w[r].x == ref.w[si - 1][r].x && w[r].y == ref.w[si - 1][r].y,
                "twiddle table stage %d lane %d r %d", si, l, r + 1);
      }
    }
  }
  void tw(int si, int lane, c2 (&w)[7]) const {
    sf_get_tw(twt.data(), si, lane, w);
  }
};

/* column-major tile: col[c][e], c < 8, e < 512 */
typedef std::vector<std::vector<c2>> cols_t;

/* the kernels' load: rows lane + 64 r of the thread's pair; rows at or
 * past `valid` and columns at or past `live` are zero registers */
static void io_load(std::vector<lines> &v, const cols_t &in, int valid,
                    int live) {
  std::vector<int> hit(SF_PAIRS * N, 0);
  for (int tid = 0; tid < NT; ++tid) {
    const int pl = sf_io_pair(tid), l = sf_io_lane(tid);
    for (int r = 0; r < 8; ++r) {
      const int e = l + 64 * r;
      hit[pl * N + e]++;
      const c2 z = {0.0f, 0.0f};
      v[tid].a[r] = (e < valid && 2 * pl < live) ? in[2 * pl][e] : z;
      v[tid].b[r] = (e < valid && 2 * pl + 1 < live) ? in[2 * pl + 1][e] : z;
    }
  }
  for (int i = 0; i < SF_PAIRS * N; ++i)
    CHECK(hit[i] == 1, "I/O mapping covers (pair,row) %d %d times", i, hit[i]);
}

static void io_store(const std::vector<lines> &v, cols_t &out, int live) {
  for (int tid = 0; tid < NT; ++tid) {
    const int pl = sf_io_pair(tid), l = sf_io_lane(tid);
    for (int s = 0; s < 8; ++s) {
      /* the last stage (L = 64) leaves output s of butterfly l at l + 64 s */
      const int e = xf_dst<8>(64, l, s);
      CHECK(e == l + 64 * s, "last stage dst(%d,%d)=%d", l, s, e);
      if (2 * pl < live) out[2 * pl][e] = v[tid].a[s];
      if (2 * pl + 1 < live) out[2 * pl + 1][e] = v[tid].b[s];
    }
  }
}

/* exchange with the I/O threads writing and the owners reading (block
 * barrier between) */
template <int L>
static void xchg_io_to_own(Block &B, std::vector<lines> &v, const char *what) {
  B.tile.begin(what);
  for (int tid = 0; tid < NT; ++tid)
    sf_put<q4, L>(B.tile.h(),
                  sf_put_base(sf_io_pair(tid), sf_io_lane(tid), L), v[tid]);
  B.tile.all_written_once(0, SF_TILE);
  for (int tid = 0; tid < NT; ++tid) {
    B.tile.restrict_to_pair(sf_own_pair(tid));
    sf_get<q4>(B.tile.h(), sf_get_base(sf_own_pair(tid), sf_own_lane(tid)),
               v[tid]);
  }
  B.tile.unrestrict();
}

/* owners write their own slice (wave sync), block barrier, I/O reads */
template <int L>
static void xchg_own_to_io(Block &B, std::vector<lines> &v, const char *what) {
  B.tile.begin(what);
  for (int tid = 0; tid < NT; ++tid) {
    B.tile.restrict_to_pair(sf_own_pair(tid));
    sf_put<q4, L>(B.tile.h(),
                  sf_put_base(sf_own_pair(tid), sf_own_lane(tid), L), v[tid]);
  }
  B.tile.unrestrict();
  B.tile.all_written_once(0, SF_TILE);
  for (int tid = 0; tid < NT; ++tid)
    sf_get<q4>(B.tile.h(), sf_get_base(sf_io_pair(tid), sf_io_lane(tid)),
               v[tid]);
}

/* wave-private: each wave writes and reads its own slice with no block
 * barrier, so one wave runs to the end before the next starts */
template <int L>
static void xchg_own_private(Block &B, std::vector<lines> &v,
                             const char *what) {
  B.tile.begin(what);
  for (int w = 0; w < NT / 64; ++w) {
    B.tile.restrict_to_pair(w);
    for (int tid = 64 * w; tid < 64 * w + 64; ++tid) {
      CHECK(sf_own_pair(tid) == w, "owner of thread %d", tid);
      sf_put<q4, L>(B.tile.h(), sf_put_base(w, sf_own_lane(tid), L), v[tid]);
    }
    B.tile.all_written_once(SF_N * w, SF_N * w + SF_N);
    for (int tid = 64 * w; tid < 64 * w + 64; ++tid)
      sf_get<q4>(B.tile.h(), sf_get_base(w, sf_own_lane(tid)), v[tid]);
  }
  B.tile.unrestrict();
}

template <int DIR>
static void stage_io(Block &B, std::vector<lines> &v, int si) {
  for (int tid = 0; tid < NT; ++tid) {
    if (si == 0) {
      sf_stage0<DIR>(v[tid]);
    } else {
      c2 w[7];
      B.tw(si, sf_io_lane(tid), w);
      sf_stage<DIR>(v[tid], w);
    }
  }
}
template <int DIR>
static void stage_own(Block &B, std::vector<lines> &v, int si) {
  for (int tid = 0; tid < NT; ++tid) {
    if (si == 0) {
      sf_stage0<DIR>(v[tid]);
    } else {
      c2 w[7];
      B.tw(si, sf_own_lane(tid), w);
      sf_stage<DIR>(v[tid], w);
    }
  }
}

/* ---- k_fft_pass_r8: one tile ---- */
template <int DIR>
static void pass_r8(Block &B, const cols_t &in, cols_t &out, int valid,
                    int live) {
  std::vector<lines> v(NT);
  io_load(v, in, valid, live);
  stage_io<DIR>(B, v, 0);
  xchg_io_to_own<1>(B, v, "pass exchange 1");
  stage_own<DIR>(B, v, 1);
  xchg_own_to_io<8>(B, v, "pass exchange 2");
  stage_io<DIR>(B, v, 2);
  io_store(v, out, live);
}

/* ---- k_fft_z_fused_r8x: one tile, result in place of a ---- */
static void fwd_to_owner(Block &B, std::vector<lines> &v) {
  stage_io<+1>(B, v, 0);
  xchg_io_to_own<1>(B, v, "z fwd exchange 1");
  stage_own<+1>(B, v, 1);
  xchg_own_private<8>(B, v, "z fwd exchange 2");
  stage_own<+1>(B, v, 2);
}

static void zfused_r8x(Block &B, cols_t &a, const cols_t &b, int valid_a,
                       int valid_b, int live, float scale) {
  std::vector<lines> va(NT), vb(NT);
  io_load(va, a, valid_a, live);
  io_load(vb, b, valid_b, live);
  fwd_to_owner(B, va);
  fwd_to_owner(B, vb);
  for (int tid = 0; tid < NT; ++tid)
    for (int r = 0; r < 8; ++r) {
      va[tid].a[r] = sf_crosspower(va[tid].a[r], vb[tid].a[r], scale);
      va[tid].b[r] = sf_crosspower(va[tid].b[r], vb[tid].b[r], scale);
    }
  stage_own<-1>(B, va, 0);
  xchg_own_private<1>(B, va, "z inv exchange 1");
  stage_own<-1>(B, va, 1);
  xchg_own_to_io<8>(B, va, "z inv exchange 2");
  stage_io<-1>(B, va, 2);
  io_store(va, a, live);
}

/* ---- references ---- */
static std::vector<double> g_cos, g_sin;
static std::vector<d2> dft(const std::vector<d2> &z, int dir) {
  std::vector<d2> X(N);
  for (int k = 0; k < N; ++k) {
    double sr = 0.0, si = 0.0;
    for (int i = 0; i < N; ++i) {
      const int q = (int)((long)k * i % N);
      const double c = g_cos[q], s = dir * g_sin[q]; /* e^{-dir 2 pi i q/N} */
      sr += z[i].x * c - z[i].y * s;
      si += z[i].x * s + z[i].y * c;
    }
    X[k] = {sr, si};
  }
  return X;
}

/* plain radix-2 f32 DIT FFT with the device's table (tw_512[k] = twn[2k]) */
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
      c2 w = twn[2 * ((i & (s - 1)) * ((h / 2) / s))];
      if (dir < 0) w.y = -w.y;
      const c2 wb = xf_cmul(a[i + s], w), p = a[i];
      a[i] = {p.x + wb.x, p.y + wb.y};
      a[i + s] = {p.x - wb.x, p.y - wb.y};
    }
  z = a;
}

static cols_t random_cols() {
  cols_t c(NCOL, std::vector<c2>(N));
  for (auto &col : c)
    for (auto &z : col) z = {rndf(), rndf()};
  return c;
}

static std::vector<d2> col_d(const std::vector<c2> &col, int valid) {
  std::vector<d2> z(N);
  for (int e = 0; e < N; ++e)
    z[e] = e < valid ? d2{col[e].x, col[e].y} : d2{0.0, 0.0};
  return z;
}
static std::vector<c2> col_f(const std::vector<c2> &col, int valid) {
  std::vector<c2> z(N);
  for (int e = 0; e < N; ++e) z[e] = e < valid ? col[e] : c2{0.0f, 0.0f};
  return z;
}

template <int DIR>
static void pass_case(Block &B, const std::vector<c2> &twn, int valid,
                      int live) {
  const cols_t in = random_cols();
  const c2 mark = {12345.0f, -54321.0f}; /* columns past `live`: no store */
  cols_t out(NCOL, std::vector<c2>(N, mark));
  pass_r8<DIR>(B, in, out, valid, live);
  double en = 0.0, er = 0.0, scale = 0.0;
  for (int c = 0; c < NCOL; ++c) {
    if (c >= live) {
      for (int e = 0; e < N; ++e)
        CHECK(out[c][e].x == mark.x && out[c][e].y == mark.y,
              "column %d past live=%d was stored", c, live);
      continue;
    }
    const std::vector<d2> ref = dft(col_d(in[c], valid), DIR);
    std::vector<c2> r2 = col_f(in[c], valid);
    r2_fft(r2, twn, DIR);
    for (int k = 0; k < N; ++k) {
      scale = fmax(scale, hypot(ref[k].x, ref[k].y));
      en = fmax(en, hypot(out[c][k].x - ref[k].x, out[c][k].y - ref[k].y));
      er = fmax(er, hypot(r2[k].x - ref[k].x, r2[k].y - ref[k].y));
    }
  }
  en /= scale;
  er /= scale;
  printf("pass %s valid=%-3d live=%d  err new %.3e  radix-2 %.3e\n",
         DIR > 0 ? "fwd" : "inv", valid, live, en, er);
  CHECK(en <= 2.0 * er, "pass dir=%d valid=%d live=%d: %.3e > 2 * %.3e", DIR,
        valid, live, en, er);
}

/* the fused chain per column in double, and with the radix-2 f32 FFT */
static std::vector<d2> chain_d(const std::vector<c2> &a,
                               const std::vector<c2> &b, int va, int vb,
                               double scale) {
  const std::vector<d2> A = dft(col_d(a, va), +1), Bs = dft(col_d(b, vb), +1);
  std::vector<d2> Q(N);
  for (int k = 0; k < N; ++k) {
    const d2 q = {A[k].x * Bs[k].x + A[k].y * Bs[k].y,
                  A[k].x * Bs[k].y - A[k].y * Bs[k].x};
    const double m = q.x * q.x + q.y * q.y;
    Q[k] = m > 1e-40 ? d2{q.x * scale / sqrt(m), q.y * scale / sqrt(m)}
                     : d2{0.0, 0.0};
  }
  return dft(Q, -1);
}
static std::vector<c2> chain_r2(const std::vector<c2> &a,
                                const std::vector<c2> &b, int va, int vb,
                                float scale, const std::vector<c2> &twn) {
  std::vector<c2> A = col_f(a, va), Bs = col_f(b, vb), Q(N);
  r2_fft(A, twn, +1);
  r2_fft(Bs, twn, +1);
  for (int k = 0; k < N; ++k) Q[k] = sf_crosspower(A[k], Bs[k], scale);
  r2_fft(Q, twn, -1);
  return Q;
}

static void chain_case(Block &B, const std::vector<c2> &twn, int valid_a,
                       int valid_b, int live, int zero_col) {
  cols_t a = random_cols();
  cols_t b = random_cols();
  /* every bin of this column of b is below the guard: exactly 0 out */
  if (zero_col >= 0)
    for (auto &z : b[zero_col]) z = {0.0f, 0.0f};
  const cols_t a0 = a;
  const float scale = 1.0f / N;
  zfused_r8x(B, a, b, valid_a, valid_b, live, scale);
  double en = 0.0, er = 0.0, sc = 0.0;
  for (int c = 0; c < NCOL; ++c) {
    if (c >= live) {
      for (int e = 0; e < N; ++e)
        CHECK(a[c][e].x == a0[c][e].x && a[c][e].y == a0[c][e].y,
              "chain column %d past live=%d was stored", c, live);
      continue;
    }
    if (c == zero_col) {
      for (int e = 0; e < N; ++e)
        CHECK(a[c][e].x == 0.0f && a[c][e].y == 0.0f,
              "guarded column %d element %d = (%g,%g), not 0", c, e,
              a[c][e].x, a[c][e].y);
      continue;
    }
    const std::vector<d2> ref = chain_d(a0[c], b[c], valid_a, valid_b, scale);
    const std::vector<c2> r2 =
        chain_r2(a0[c], b[c], valid_a, valid_b, scale, twn);
    for (int k = 0; k < N; ++k) {
      sc = fmax(sc, hypot(ref[k].x, ref[k].y));
      en = fmax(en, hypot(a[c][k].x - ref[k].x, a[c][k].y - ref[k].y));
      er = fmax(er, hypot(r2[k].x - ref[k].x, r2[k].y - ref[k].y));
    }
  }
  en /= sc;
  er /= sc;
  printf("chain valid_a=%-3d valid_b=%-3d live=%d  err new %.3e  radix-2 "
         "%.3e\n", valid_a, valid_b, live, en, er);
  CHECK(en <= 2.0 * er, "chain %d/%d live=%d: %.3e > 2 * %.3e", valid_a,
        valid_b, live, en, er);
}

/* ---- bank conflicts of the 16-byte accesses ----
 * ds_write_b128: 8 groups of 8 contiguous lanes, bank (a/4) mod 32, so a
 * 16-byte slot conflicts with slots equal mod 8; ds_read_b128: the four
 * 16-lane groups below, bank (a/4) mod 64, slots equal mod 16. Degree =
 * the most distinct slots one bank set serves in one group. */
static int degree(const int *slot, const int (*groups)[16], int ngroups,
                  int glen, int mod) {
  int worst = 1;
  for (int g = 0; g < ngroups; ++g)
    for (int b = 0; b < mod; ++b) {
      int distinct = 0, seen[16];
      for (int i = 0; i < glen; ++i) {
        const int s = slot[groups[g][i]];
        if (s % mod != b) continue;
        bool dup = false;
        for (int k = 0; k < distinct; ++k) dup |= seen[k] == s;
        if (!dup) seen[distinct++] = s;
      }
      if (distinct > worst) worst = distinct;
    }
  return worst;
}
static int wr_degree(const int *slot) {
  int g[8][16];
  for (int i = 0; i < 8; ++i)
    for (int k = 0; k < 8; ++k) g[i][k] = 8 * i + k;
  return degree(slot, g, 8, 8, 8);
}
static int rd_degree(const int *slot) {
  static const int g[4][16] = {
      {0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
      {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
      {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59},
      {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};
  return degree(slot, g, 4, 16, 16);
}

/* kind: 0 = I/O mapping, 1 = owner mapping; L > 0: the write after the
 * stage of sub-size L, L == 0: the read lane + 64 r. Worst wave. */
static void bank_row(const char *name, int kind, int L) {
  printf("  %-28s", name);
  for (int k = 0; k < 8; ++k) {
    int worst = 1;
    for (int w = 0; w < NT / 64; ++w) {
      int slot[64];
      for (int i = 0; i < 64; ++i) {
        const int tid = 64 * w + i;
        const int p = kind ? sf_own_pair(tid) : sf_io_pair(tid);
        const int l = kind ? sf_own_lane(tid) : sf_io_lane(tid);
        slot[i] = sf_idx(p, L ? xf_dst<8>(L, l, k) : l + 64 * k);
      }
      const int d = L ? wr_degree(slot) : rd_degree(slot);
      if (d > worst) worst = d;
    }
    printf(" %d", worst);
    CHECK(worst == 1, "%s k=%d: degree %d", name, k, worst);
  }
  printf("\n");
}

static void bank_table() {
  printf("bank conflicts, 16-byte slots (degree; 1 = conflict-free), "
         "s or r = 0..7\n");
  bank_row("write L=1  I/O   (fwd x1)", 0, 1);
  bank_row("read       owner (x1, x2)", 1, 0);
  bank_row("write L=8  owner (x2)", 1, 8);
  bank_row("read       I/O   (x2)", 0, 0);
  bank_row("write L=1  owner (z inv x1)", 1, 1);
  std::vector<int> hit(SF_TILE, 0);
  for (int p = 0; p < SF_PAIRS; ++p)
    for (int m = 0; m < SF_N; ++m) {
      const int s = sf_idx(p, m);
      CHECK(s >= SF_N * p && s < SF_N * p + SF_N, "idx(%d,%d)=%d", p, m, s);
      if (s >= 0 && s < SF_TILE) hit[s]++;
    }
  for (int i = 0; i < SF_TILE; ++i)
    CHECK(hit[i] == 1, "slot map not bijective at %d", i);
  /* the base ^ constant form the kernels address with is sf_idx itself */
  for (int p = 0; p < SF_PAIRS; ++p)
    for (int l = 0; l < 64; ++l)
      for (int k = 0; k < 8; ++k) {
        for (int L = 1; L <= 8; L *= 8)
          CHECK((sf_put_base(p, l, L) ^ sf_put_xor(L, k)) ==
                    sf_idx(p, xf_dst<8>(L, l, k)),
                "put identity p=%d lane=%d L=%d s=%d", p, l, L, k);
        CHECK((sf_get_base(p, l) ^ sf_get_xor(k)) == sf_idx(p, l + 64 * k),
              "get identity p=%d lane=%d r=%d", p, l, k);
      }
}

int main() {
  g_cos.resize(N);
  g_sin.resize(N);
  for (int q = 0; q < N; ++q) {
    g_cos[q] = cos(-2.0 * M_PI * q / N);
    g_sin[q] = sin(-2.0 * M_PI * q / N);
  }
  const std::vector<c2> twn = make_twn();
  Block B(twn);
  bank_table();

  const int valids[3] = {512, 300, 1}, lives[3] = {8, 3, 1};
  for (int valid : valids)
    for (int live : lives) {
      pass_case<+1>(B, twn, valid, live);
      pass_case<-1>(B, twn, valid, live);
    }

  chain_case(B, twn, 512, 512, 8, -1);
  chain_case(B, twn, 300, 280, 8, 5); /* unequal extents, a guarded column */
  chain_case(B, twn, 512, 300, 3, 1);
  chain_case(B, twn, 1, 512, 1, -1);

  /* the guard itself: a nonzero bin whose squared magnitude is below 1e-40 */
  {
    const c2 a = {3e-11f, -2e-11f}, b = {1e-11f, 4e-11f};
    const c2 q = sf_crosspower(a, b, 1.0f);
    CHECK(q.x == 0.0f && q.y == 0.0f, "guard: (%g,%g)", q.x, q.y);
    const c2 a1 = {3e-9f, -2e-9f}, b1 = {1e-9f, 4e-9f};
    const c2 q1 = sf_crosspower(a1, b1, 1.0f);
    CHECK(fabs(hypot(q1.x, q1.y) - 1.0) < 1e-6, "above the guard: |q|=%g",
          hypot(q1.x, q1.y));
  }

  printf("sfft_r8_host: %d failures\n", g_fail);
  return g_fail ? 1 : 0;
}
