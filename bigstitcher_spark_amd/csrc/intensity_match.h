/* intensity_match.h — pairwise intensity matching (bs_intensity_match_pair),
 * included at the end of bigstitch.hip. Contract: tests/intensity_ref.py; the
 * [PIN-INT-*] tags used below are spelled out there and in DESIGN.md
 * "Intensity matching".
 *
 * Four kernels, no atomics: every bucket (cellA, cellB) is owned by one
 * 256-thread workgroup and written with ordinary stores.
 *   k_int_render       thread = grid sample; both views sampled, quantised
 *   k_int_moments<M>   block = bucket; six integer sums, either over the
 *                      bucket's search box of the render grid (M = false,
 *                      gives n_cand) or over its compacted members gated by
 *                      a line (M = true, one refit round)
 *   k_int_compact      block = bucket; order-preserving compaction of the
 *                      members' (P, Q) into the bucket's segment
 *   k_int_ransac<HPT>  block = bucket; thread t owns hypotheses t, t+256, ..;
 *                      members stream through LDS, read as broadcasts
 */
#ifndef BS_INTENSITY_MATCH_H
#define BS_INTENSITY_MATCH_H

#include "bs_intensity_solve.h" /* bsint::line_fit, shared with the solver */

#define INT_WG 256          /* threads per block = samples per LDS tile */
#define INT_MAX_ITER 4096   /* INT_WG * largest HPT */
#define INT_MAX_MEMBERS (1u << 24)

struct bs_int_view {
  const unsigned short *ptr;
  int nx, ny, nz;
  int cgx, cgy, cgz;
  float inv[12]; /* world -> view-local, row-major 3x4 (fp32) */
};

struct bs_int_bucket {
  int lo[3], ext[3];      /* search box in render-grid samples */
  unsigned short ca, cb;  /* cell ids */
  unsigned int off;       /* first member in the compacted array */
  int n;                  /* n_cand */
  float a, b;             /* gate line of a refit round */
  int active;             /* refit round: 0 = skip */
};

struct bs_int_winner {
  int count, it;
  float a, b;
};

/* One float32 operation, rounded on its own. The compiler's default lets a
 * multiply and a following add fuse into one FMA (and __fmul_rn / __fadd_rn
 * are plain operators to it, so they fuse as well); the pragma takes the
 * permission away from the operation it encloses, wherever it is inlined. */
__device__ __forceinline__ float int_add(float x, float y) {
#pragma clang fp contract(off)
  return x + y;
}
__device__ __forceinline__ float int_sub(float x, float y) {
#pragma clang fp contract(off)
  return x - y;
}
__device__ __forceinline__ float int_mul(float x, float y) {
#pragma clang fp contract(off)
  return x * y;
}
__device__ __forceinline__ float int_div(float x, float y) {
  return x / y; /* IEEE-rounded: the build keeps correctly rounded division */
}

__device__ __forceinline__ float int_lerp(float c0, float c1, float f) {
  return int_add(c0, int_mul(int_sub(c1, c0), f));
}

/* [PIN-INT-RENDER] + [PIN-INT-CELL]: quantised sample of one view at world
 * point w, -1 when w maps outside ([PIN-BOUNDS]). Every operation is rounded
 * on its own so that the numpy contract forms the same numbers. */
__device__ __forceinline__ int int_sample(const bs_int_view &v, float wx,
                                          float wy, float wz, int *cell) {
  float p[3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
    p[r] = int_add(
        int_add(int_add(int_mul(v.inv[r * 4 + 0], wx),
                            int_mul(v.inv[r * 4 + 1], wy)),
                  int_mul(v.inv[r * 4 + 2], wz)),
        v.inv[r * 4 + 3]);
  const float px = p[0], py = p[1], pz = p[2];
  *cell = 0;
  if (!(px >= 0.0f && px <= (float)(v.nx - 1) && py >= 0.0f &&
        py <= (float)(v.ny - 1) && pz >= 0.0f && pz <= (float)(v.nz - 1)))
    return -1;
  const int x0 = (int)floorf(px), y0 = (int)floorf(py), z0 = (int)floorf(pz);
  const int x1 = min(x0 + 1, v.nx - 1), y1 = min(y0 + 1, v.ny - 1),
            z1 = min(z0 + 1, v.nz - 1);
  const float fx = int_sub(px, (float)x0), fy = int_sub(py, (float)y0),
              fz = int_sub(pz, (float)z0);
  const unsigned short *q = v.ptr;
  const long s0 = (long)z0 * v.ny, s1 = (long)z1 * v.ny;
  const float c000 = q[(s0 + y0) * v.nx + x0], c100 = q[(s0 + y0) * v.nx + x1];
  const float c010 = q[(s0 + y1) * v.nx + x0], c110 = q[(s0 + y1) * v.nx + x1];
  const float c001 = q[(s1 + y0) * v.nx + x0], c101 = q[(s1 + y0) * v.nx + x1];
  const float c011 = q[(s1 + y1) * v.nx + x0], c111 = q[(s1 + y1) * v.nx + x1];
  const float c00 = int_lerp(c000, c100, fx), c10 = int_lerp(c010, c110, fx);
  const float c01 = int_lerp(c001, c101, fx), c11 = int_lerp(c011, c111, fx);
  const float c0 = int_lerp(c00, c10, fy), c1 = int_lerp(c01, c11, fy);
  const float val = int_lerp(c0, c1, fz);
  const int cx = min(v.cgx - 1, (int)int_div(int_mul(px, (float)v.cgx),
                                               (float)v.nx));
  const int cy = min(v.cgy - 1, (int)int_div(int_mul(py, (float)v.cgy),
                                               (float)v.ny));
  const int cz = min(v.cgz - 1, (int)int_div(int_mul(pz, (float)v.cgz),
                                               (float)v.nz));
  *cell = cx + v.cgx * (cy + v.cgy * cz);
  return (int)rintf(int_mul(val, 8.0f));
}

/* Thread = grid sample, x fastest. A sample that is not valid in both views
 * (outside one, or a quantised value outside [lo8, hi8]) is stored as
 * P = Q = -1 with both cell ids 0. */
__global__ __launch_bounds__(INT_WG) void k_int_render(
    bs_int_view va, bs_int_view vb, long g0x, long g0y, long g0z, int dx,
    int dy, long nsamp, double s, int lo8, int hi8, int *__restrict__ P,
    int *__restrict__ Q, unsigned short *__restrict__ cA,
    unsigned short *__restrict__ cB) {
  const long i = (long)blockIdx.x * INT_WG + threadIdx.x;
  if (i >= nsamp) return;
  const int gx = (int)(i % dx), gy = (int)((i / dx) % dy);
  const long gz = i / ((long)dx * dy);
  /* [PIN-INT-GRID]: formed in double, rounded once */
  const float wx = (float)((double)(gx + g0x) * s);
  const float wy = (float)((double)(gy + g0y) * s);
  const float wz = (float)((double)(gz + g0z) * s);
  int ca, cb;
  int p = int_sample(va, wx, wy, wz, &ca);
  int q = int_sample(vb, wx, wy, wz, &cb);
  if (!(p >= lo8 && q >= lo8 && p <= hi8 && q <= hi8)) {
    p = q = -1;
    ca = cb = 0;
  }
  P[i] = p;
  Q[i] = q;
  cA[i] = (unsigned short)ca;
  cB[i] = (unsigned short)cb;
}

/* [PIN-INT-RANSAC] inlier test, each step rounded on its own. NaN in any
 * operand fails the compare. */
__device__ __forceinline__ bool int_inlier(float a, float b, float p, float q,
                                           float eps) {
  return fabsf(int_sub(int_add(int_mul(a, p), b), q)) <= eps;
}

/* Six sums n, Sp, Sq, Spp, Sqq, Spq of one bucket -> out[bucket * 6 ..].
 * MEMBERS = false: walk the search box, a sample counts when it is valid and
 * carries the bucket's two cell ids. MEMBERS = true: walk the compacted
 * members, a sample counts when it passes the bucket's gate line. */
template <bool MEMBERS>
__global__ __launch_bounds__(INT_WG) void k_int_moments(
    const bs_int_bucket *__restrict__ bk, const int *__restrict__ P,
    const int *__restrict__ Q, const unsigned short *__restrict__ cA,
    const unsigned short *__restrict__ cB, int dx, int dy,
    const float2 *__restrict__ members, float eps, u64 *__restrict__ out) {
  __shared__ u64 ws[INT_WG / 64][6];
  const bs_int_bucket b = bk[blockIdx.x];
  const int tid = threadIdx.x;
  u64 s[6] = {0, 0, 0, 0, 0, 0};
  if (MEMBERS) {
    if (!b.active) return; /* uniform over the block */
    const float2 *seg = members + b.off;
    for (int m = tid; m < b.n; m += INT_WG) {
      const float2 v = seg[m];
      if (int_inlier(b.a, b.b, v.x, v.y, eps)) {
        const u64 p = (u64)v.x, q = (u64)v.y;
        s[0] += 1; s[1] += p; s[2] += q;
        s[3] += p * p; s[4] += q * q; s[5] += p * q;
      }
    }
  } else {
    const long vol = (long)b.ext[0] * b.ext[1] * b.ext[2];
    for (long i = tid; i < vol; i += INT_WG) {
      const int x = (int)(i % b.ext[0]), y = (int)((i / b.ext[0]) % b.ext[1]);
      const long z = i / ((long)b.ext[0] * b.ext[1]);
      const long g = ((z + b.lo[2]) * dy + (y + b.lo[1])) * dx + (x + b.lo[0]);
      const int pi = P[g];
      if (pi >= 0 && cA[g] == b.ca && cB[g] == b.cb) {
        const u64 p = (u64)pi, q = (u64)Q[g];
        s[0] += 1; s[1] += p; s[2] += q;
        s[3] += p * p; s[4] += q * q; s[5] += p * q;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) s[k] = wave_sum_u64(s[k]);
  if ((tid & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 6; ++k) ws[tid >> 6][k] = s[k];
  }
  __syncthreads();
  if (tid < 6)
    out[(size_t)blockIdx.x * 6 + tid] =
        ws[0][tid] + ws[1][tid] + ws[2][tid] + ws[3][tid];
}

/* Members of one bucket, in ascending grid order, as float2 (P, Q) into
 * members[off .. off + n). The box is walked in chunks of 256; inside a chunk
 * a wave ranks its members by ballot + popcount, wave bases go through LDS,
 * and a running base carries over to the next chunk. */
__global__ __launch_bounds__(INT_WG) void k_int_compact(
    const bs_int_bucket *__restrict__ bk, const int *__restrict__ P,
    const int *__restrict__ Q, const unsigned short *__restrict__ cA,
    const unsigned short *__restrict__ cB, int dx, int dy,
    float2 *__restrict__ members) {
  __shared__ int wcnt[INT_WG / 64];
  const bs_int_bucket b = bk[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long vol = (long)b.ext[0] * b.ext[1] * b.ext[2];
  int base = 0;
  for (long c0 = 0; c0 < vol; c0 += INT_WG) {
    const long i = c0 + tid;
    bool m = false;
    int p = 0, q = 0;
    if (i < vol) {
      const int x = (int)(i % b.ext[0]), y = (int)((i / b.ext[0]) % b.ext[1]);
      const long z = i / ((long)b.ext[0] * b.ext[1]);
      const long g = ((z + b.lo[2]) * dy + (y + b.lo[1])) * dx + (x + b.lo[0]);
      p = P[g];
      m = p >= 0 && cA[g] == b.ca && cB[g] == b.cb;
      if (m) q = Q[g];
    }
    const unsigned long long bal = __ballot(m);
    const int pre = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wcnt[wave] = __popcll(bal);
    __syncthreads();
    int wb = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < INT_WG / 64; ++w) {
      if (w < wave) wb += wcnt[w];
      tot += wcnt[w];
    }
    const int slot = base + wb + pre;
    if (m && slot < b.n) members[(size_t)b.off + slot] = make_float2(p, q);
    base += tot;
    __syncthreads(); /* wcnt is rewritten by the next chunk */
  }
}

__device__ __forceinline__ u64 int_splitmix64(u64 x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

/* [PIN-INT-RANSAC]. Hypothesis `it` of thread t sits in slot it / 256. A
 * void hypothesis and a slot past `iterations` carry a NaN line, which no
 * sample passes; the tail of the last tile is NaN for the same reason. Each
 * LDS read is one 16-byte broadcast of two samples. */
template <int HPT>
__global__ __launch_bounds__(INT_WG) void k_int_ransac(
    const bs_int_bucket *__restrict__ bk, const float2 *__restrict__ members,
    int iterations, float eps, bs_int_winner *__restrict__ out) {
  __shared__ float4 tile[INT_WG / 2];
  __shared__ bs_int_winner wbest[INT_WG / 64];
  const bs_int_bucket b = bk[blockIdx.x];
  const float2 *seg = members + b.off;
  const int tid = threadIdx.x;
  float ha[HPT], hb[HPT];
  int cnt[HPT];
#pragma unroll
  for (int j = 0; j < HPT; ++j) {
    const int it = tid + INT_WG * j;
    ha[j] = NAN;
    hb[j] = NAN;
    cnt[j] = 0;
    if (it < iterations) {
      const u64 key = ((u64)b.ca << 48) | ((u64)b.cb << 32) | ((u64)it << 8);
      const float2 m1 =
          seg[int_splitmix64(BS_RANSAC_SEED ^ key) % (u64)b.n];
      const float2 m2 =
          seg[int_splitmix64(BS_RANSAC_SEED ^ (key | 1ull)) % (u64)b.n];
      if (m1.x != m2.x) {
        const float a = int_div(int_sub(m2.y, m1.y), int_sub(m2.x, m1.x));
        if (a > 0.0f) {
          ha[j] = a;
          hb[j] = int_sub(m1.y, int_mul(a, m1.x));
        }
      }
    }
  }
  for (int t0 = 0; t0 < b.n; t0 += INT_WG) {
    __syncthreads();
    const int m = t0 + tid;
    ((float2 *)tile)[tid] = m < b.n ? seg[m] : make_float2(NAN, NAN);
    __syncthreads();
#pragma unroll 4
    for (int c = 0; c < INT_WG / 2; ++c) {
      const float4 s = tile[c];
#pragma unroll
      for (int j = 0; j < HPT; ++j)
        cnt[j] += (int)int_inlier(ha[j], hb[j], s.x, s.y, eps) +
                  (int)int_inlier(ha[j], hb[j], s.z, s.w, eps);
    }
  }
  /* arg-max on (count, lowest it): thread, wave, block */
  bs_int_winner w = {-1, 0x7FFFFFFF, NAN, NAN};
#pragma unroll
  for (int j = 0; j < HPT; ++j) {
    const int it = tid + INT_WG * j;
    if (it < iterations && cnt[j] > w.count) {
      w.count = cnt[j];
      w.it = it;
      w.a = ha[j];
      w.b = hb[j];
    }
  }
  for (int off = 32; off >= 1; off >>= 1) {
    bs_int_winner o;
    o.count = __shfl_down(w.count, off);
    o.it = __shfl_down(w.it, off);
    o.a = __shfl_down(w.a, off);
    o.b = __shfl_down(w.b, off);
    if (o.count > w.count || (o.count == w.count && o.it < w.it)) w = o;
  }
  if ((tid & 63) == 0) wbest[tid >> 6] = w;
  __syncthreads();
  if (tid == 0) {
    for (int k = 1; k < INT_WG / 64; ++k) {
      const bs_int_winner o = wbest[k];
      if (o.count > w.count || (o.count == w.count && o.it < w.it)) w = o;
    }
    out[blockIdx.x] = w;
  }
}

/* ------------------------------------------------------------------ host */

enum { INTB_P, INTB_Q, INTB_CA, INTB_CB, INTB_BUCKETS, INTB_SUMS,
       INTB_MEMBERS, INTB_WINNERS, INTB_COUNT };

static int int_buf(bs_ctx *c, int which, size_t bytes, void **out) {
  int rc = ensure_dev(c, &c->int_buf[which], &c->int_cap[which],
                      std::max(bytes, (size_t)16));
  *out = c->int_buf[which];
  return rc;
}

/* bbox of the box [plo, phi] under a row-major 3x4 affine (the corner walk
 * of view_overlaps_block / bscli::tbbox) */
static void int_tbbox(const double *m, const double plo[3],
                      const double phi[3], double lo[3], double hi[3]) {
  for (int d = 0; d < 3; ++d) {
    lo[d] = 1e300;
    hi[d] = -1e300;
  }
  for (int cz = 0; cz < 2; ++cz)
    for (int cy = 0; cy < 2; ++cy)
      for (int cx = 0; cx < 2; ++cx) {
        const double p[3] = {cx ? phi[0] : plo[0], cy ? phi[1] : plo[1],
                             cz ? phi[2] : plo[2]};
        for (int r = 0; r < 3; ++r) {
          const double w = m[r * 4 + 0] * p[0] + m[r * 4 + 1] * p[1] +
                           m[r * 4 + 2] * p[2] + m[r * 4 + 3];
          if (w < lo[r]) lo[r] = w;
          if (w > hi[r]) hi[r] = w;
        }
      }
}

struct int_setup {
  bs_int_view va, vb;
  long g0[3], dims[3]; /* [PIN-INT-GRID]; dims all zero = disjoint */
  long nsamp;
  double s;
  int lo8, hi8;
  int *dP, *dQ;
  unsigned short *dcA, *dcB;
};

/* Validates, forms the grid and renders it. Caller holds c->mu and has set
 * the device. */
static int int_render(bs_ctx *c, int32_t view_a, const double *affine_a,
                      int32_t view_b, const double *affine_b,
                      const bs_intensity_params *p, int_setup *g) {
  if (!(p->render_scale > 0.0 && p->render_scale <= 1.0)) {
    c->err = "intensity: renderScale must be in (0, 1]";
    return BS_EINVAL;
  }
  for (int d = 0; d < 3; ++d)
    if (p->coefficients[d] < 1) {
      c->err = "intensity: numCoefficients must be >= 1 per axis";
      return BS_EINVAL;
    }
  if (p->iterations < 1) {
    c->err = "intensity: iterations must be >= 1";
    return BS_EINVAL;
  }
  if (p->iterations > INT_MAX_ITER) {
    c->err = "intensity: more than 4096 iterations";
    return BS_EUNSUP;
  }
  if ((long long)p->coefficients[0] * p->coefficients[1] * p->coefficients[2] >
      65535) {
    c->err = "intensity: more than 65535 coefficient cells per view";
    return BS_EUNSUP;
  }
  auto ita = c->views.find(view_a), itb = c->views.find(view_b);
  if (ita == c->views.end() || itb == c->views.end()) {
    c->err = "intensity: view not uploaded";
    return BS_ENOVIEW;
  }
  const bs_view_rec *rec[2] = {&ita->second, &itb->second};
  const double *aff[2] = {affine_a, affine_b};
  bs_int_view *dv[2] = {&g->va, &g->vb};
  double lo[3] = {-1e300, -1e300, -1e300}, hi[3] = {1e300, 1e300, 1e300};
  for (int k = 0; k < 2; ++k) {
    bs_int_view &v = *dv[k];
    v.ptr = rec[k]->dptr;
    v.nx = (int)rec[k]->dims[0];
    v.ny = (int)rec[k]->dims[1];
    v.nz = (int)rec[k]->dims[2];
    v.cgx = p->coefficients[0];
    v.cgy = p->coefficients[1];
    v.cgz = p->coefficients[2];
    if (invert34(aff[k], v.inv) != BS_OK) {
      c->err = "intensity: singular view affine";
      return BS_EINVAL;
    }
    const double z3[3] = {0, 0, 0};
    const double d3[3] = {(double)(v.nx - 1), (double)(v.ny - 1),
                          (double)(v.nz - 1)};
    double vlo[3], vhi[3];
    int_tbbox(aff[k], z3, d3, vlo, vhi);
    for (int d = 0; d < 3; ++d) {
      lo[d] = std::max(lo[d], vlo[d]);
      hi[d] = std::min(hi[d], vhi[d]);
    }
  }
  g->s = 1.0 / p->render_scale;
  g->nsamp = 1;
  for (int d = 0; d < 3; ++d) {
    const double a = std::ceil(lo[d] / g->s), b = std::floor(hi[d] / g->s);
    if (!(b >= a)) { /* disjoint (or not a number) on this axis */
      g->nsamp = 0;
      break;
    }
    if (std::fabs(a) > 1e15 || std::fabs(b) > 1e15) {
      c->err = "intensity: more than 2^31 grid samples";
      return BS_EUNSUP;
    }
    g->g0[d] = (long)a;
    g->dims[d] = (long)b - (long)a + 1;
    if (g->dims[d] > (1l << 31) || g->nsamp * g->dims[d] > (1l << 31)) {
      c->err = "intensity: more than 2^31 grid samples";
      return BS_EUNSUP;
    }
    g->nsamp *= g->dims[d];
  }
  if (g->nsamp == 0) {
    for (int d = 0; d < 3; ++d) g->g0[d] = g->dims[d] = 0;
    return BS_OK;
  }
  /* thresholds as integers in 1/8 grey level: P >= 8 min, P <= 8 max */
  const double t0 = std::ceil(8.0 * p->min_threshold);
  g->lo8 = !(t0 > 0.0) ? 0 : t0 >= 2e9 ? 2000000000 : (int)t0;
  g->hi8 = 0x7FFFFFFF;
  if (!std::isnan(p->max_threshold)) {
    const double t1 = std::floor(8.0 * p->max_threshold);
    g->hi8 = t1 < -1.0 ? -2 : t1 >= 2e9 ? 0x7FFFFFFF : (int)t1;
  }
  int rc;
  const size_t n = (size_t)g->nsamp;
  if ((rc = int_buf(c, INTB_P, n * 4, (void **)&g->dP)) ||
      (rc = int_buf(c, INTB_Q, n * 4, (void **)&g->dQ)) ||
      (rc = int_buf(c, INTB_CA, n * 2, (void **)&g->dcA)) ||
      (rc = int_buf(c, INTB_CB, n * 2, (void **)&g->dcB)))
    return rc;
  {
    bs_tim t(c, BS_K_INT_RENDER);
    hipLaunchKernelGGL(k_int_render, dim3((unsigned)((n + INT_WG - 1) / INT_WG)),
                       dim3(INT_WG), 0, c->stream, g->va, g->vb, g->g0[0],
                       g->g0[1], g->g0[2], (int)g->dims[0], (int)g->dims[1],
                       g->nsamp, g->s, g->lo8, g->hi8, g->dP, g->dQ, g->dcA,
                       g->dcB);
  }
  CHK(c, hipGetLastError());
  return BS_OK;
}

extern "C" int bs_debug_intensity_render(
    bs_ctx *c, int32_t view_a, const double affine_a[12], int32_t view_b,
    const double affine_b[12], const bs_intensity_params *p,
    int64_t grid_origin[3], int64_t grid_dims[3], int32_t *p_out,
    int32_t *q_out, uint16_t *cell_a_out, uint16_t *cell_b_out) {
  if (!c || !affine_a || !affine_b || !p || !grid_origin || !grid_dims)
    return BS_EINVAL;
  if (p_out && (!q_out || !cell_a_out || !cell_b_out)) return BS_EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  CHK(c, hipSetDevice(c->dev));
  int_setup st;
  int rc = int_render(c, view_a, affine_a, view_b, affine_b, p, &st);
  if (rc) return rc;
  for (int d = 0; d < 3; ++d) {
    grid_origin[d] = st.g0[d];
    grid_dims[d] = st.dims[d];
  }
  if (st.nsamp && p_out) {
    const size_t n = (size_t)st.nsamp;
    CHK(c, hipMemcpyAsync(p_out, st.dP, n * 4, hipMemcpyDeviceToHost,
                          c->stream));
    CHK(c, hipMemcpyAsync(q_out, st.dQ, n * 4, hipMemcpyDeviceToHost,
                          c->stream));
    CHK(c, hipMemcpyAsync(cell_a_out, st.dcA, n * 2, hipMemcpyDeviceToHost,
                          c->stream));
    CHK(c, hipMemcpyAsync(cell_b_out, st.dcB, n * 2, hipMemcpyDeviceToHost,
                          c->stream));
  }
  CHK(c, hipStreamSynchronize(c->stream));
  flush_stats(c);
  return BS_OK;
}

/* World boxes of a view's coefficient cells: cell i of an axis holds the
 * pixels with (int)(px * cg / n) == i, i.e. [i n / cg, (i + 1) n / cg),
 * widened by half a pixel against the float32 rounding of that test and
 * clipped to the view. */
static void int_cell_boxes(const bs_int_view &v, const double *aff,
                           std::vector<double> &boxes) {
  const int cg[3] = {v.cgx, v.cgy, v.cgz}, nn[3] = {v.nx, v.ny, v.nz};
  boxes.resize((size_t)cg[0] * cg[1] * cg[2] * 6);
  for (int z = 0; z < cg[2]; ++z)
    for (int y = 0; y < cg[1]; ++y)
      for (int x = 0; x < cg[0]; ++x) {
        const int ci[3] = {x, y, z};
        double plo[3], phi[3];
        for (int d = 0; d < 3; ++d) {
          plo[d] = std::max(0.0, (double)ci[d] * nn[d] / cg[d] - 0.5);
          phi[d] = std::min((double)(nn[d] - 1),
                            (double)(ci[d] + 1) * nn[d] / cg[d] + 0.5);
          if (phi[d] < plo[d]) phi[d] = plo[d]; /* cell past the last pixel */
        }
        double *b = &boxes[((size_t)(z * cg[1] + y) * cg[0] + x) * 6];
        int_tbbox(aff, plo, phi, b, b + 3);
      }
}

template <int HPT>
static void int_ransac_launch(bs_ctx *c, int nb, const bs_int_bucket *dbk,
                              const float2 *dmem, int iterations, float eps,
                              bs_int_winner *dwin) {
  hipLaunchKernelGGL(k_int_ransac<HPT>, dim3(nb), dim3(INT_WG), 0, c->stream,
                     dbk, dmem, iterations, eps, dwin);
}

extern "C" int bs_intensity_match_pair(
    bs_ctx *c, int32_t view_a, const double affine_a[12], int32_t view_b,
    const double affine_b[12], const bs_intensity_params *p,
    bs_intensity_match *out, size_t capacity, size_t *n_found) {
  if (!c || !affine_a || !affine_b || !p || !n_found || (capacity > 0 && !out))
    return BS_EINVAL;
  std::lock_guard<std::mutex> lk(c->mu);
  CHK(c, hipSetDevice(c->dev));
  int_setup st;
  int rc = int_render(c, view_a, affine_a, view_b, affine_b, p, &st);
  if (rc) return rc;
  *n_found = 0;
  if (st.nsamp == 0) {
    CHK(c, hipStreamSynchronize(c->stream));
    flush_stats(c);
    return BS_OK;
  }
  const int dx = (int)st.dims[0], dy = (int)st.dims[1];

  /* candidate buckets: every (cellA, cellB) whose world boxes meet inside
   * the grid; the search box is their common part, +-1 sample */
  std::vector<double> boxa, boxb;
  int_cell_boxes(st.va, affine_a, boxa);
  int_cell_boxes(st.vb, affine_b, boxb);
  const size_t nca = boxa.size() / 6, ncb = boxb.size() / 6;
  std::vector<bs_int_bucket> cand;
  for (size_t ia = 0; ia < nca; ++ia) {
    const double *A = &boxa[ia * 6];
    for (size_t ib = 0; ib < ncb; ++ib) {
      const double *B = &boxb[ib * 6];
      bs_int_bucket k{};
      bool ok = true;
      for (int d = 0; d < 3 && ok; ++d) {
        const double l = std::max(A[d], B[d]), h = std::min(A[3 + d], B[3 + d]);
        if (h < l) {
          ok = false;
          break;
        }
        const long gl = std::max(0l, (long)std::floor(l / st.s) - 1 - st.g0[d]);
        const long gh = std::min(st.dims[d] - 1,
                                 (long)std::ceil(h / st.s) + 1 - st.g0[d]);
        if (gh < gl) ok = false;
        k.lo[d] = (int)gl;
        k.ext[d] = (int)(gh - gl + 1);
      }
      if (!ok) continue;
      k.ca = (unsigned short)ia;
      k.cb = (unsigned short)ib;
      cand.push_back(k);
    }
  }
  if (cand.empty()) {
    CHK(c, hipStreamSynchronize(c->stream));
    flush_stats(c);
    return BS_OK;
  }
  bs_int_bucket *dbk;
  u64 *dsums;
  if ((rc = int_buf(c, INTB_BUCKETS, cand.size() * sizeof(bs_int_bucket),
                    (void **)&dbk)) ||
      (rc = int_buf(c, INTB_SUMS, cand.size() * 6 * sizeof(u64),
                    (void **)&dsums)))
    return rc;
  CHK(c, hipMemcpyAsync(dbk, cand.data(), cand.size() * sizeof(bs_int_bucket),
                        hipMemcpyHostToDevice, c->stream));
  {
    bs_tim t(c, BS_K_INT_MOMENTS);
    hipLaunchKernelGGL(k_int_moments<false>, dim3((unsigned)cand.size()),
                       dim3(INT_WG), 0, c->stream, dbk, st.dP, st.dQ, st.dcA,
                       st.dcB, dx, dy, (const float2 *)nullptr, 0.0f, dsums);
  }
  CHK(c, hipGetLastError());
  std::vector<u64> sums(cand.size() * 6);
  CHK(c, hipMemcpyAsync(sums.data(), dsums, sums.size() * sizeof(u64),
                        hipMemcpyDeviceToHost, c->stream));
  CHK(c, hipStreamSynchronize(c->stream));

  /* survivors, in (cellA, cellB) order, with their member segments */
  std::vector<bs_int_bucket> bk;
  const u64 need = (u64)std::max(1, p->min_num_candidates);
  u64 total = 0;
  for (size_t i = 0; i < cand.size(); ++i) {
    const u64 n = sums[i * 6];
    if (n > INT_MAX_MEMBERS) {
      flush_stats(c);
      c->err = "intensity: a bucket has more than 2^24 members";
      return BS_EUNSUP;
    }
    if (n < need) continue;
    bs_int_bucket k = cand[i];
    k.off = (unsigned int)total;
    k.n = (int)n;
    total += n;
    bk.push_back(k);
  }
  if (bk.empty()) {
    flush_stats(c);
    return BS_OK;
  }
  const int nb = (int)bk.size();
  float2 *dmem;
  bs_int_winner *dwin;
  if ((rc = int_buf(c, INTB_BUCKETS, bk.size() * sizeof(bs_int_bucket),
                    (void **)&dbk)) ||
      (rc = int_buf(c, INTB_SUMS, bk.size() * 6 * sizeof(u64),
                    (void **)&dsums)) ||
      (rc = int_buf(c, INTB_MEMBERS, (size_t)total * sizeof(float2),
                    (void **)&dmem)) ||
      (rc = int_buf(c, INTB_WINNERS, bk.size() * sizeof(bs_int_winner),
                    (void **)&dwin)))
    return rc;
  const float eps = (float)(8.0 * p->max_epsilon);
  CHK(c, hipMemcpyAsync(dbk, bk.data(), bk.size() * sizeof(bs_int_bucket),
                        hipMemcpyHostToDevice, c->stream));
  {
    bs_tim t(c, BS_K_INT_MOMENTS);
    hipLaunchKernelGGL(k_int_compact, dim3(nb), dim3(INT_WG), 0, c->stream,
                       dbk, st.dP, st.dQ, st.dcA, st.dcB, dx, dy, dmem);
  }
  {
    bs_tim t(c, BS_K_INT_RANSAC);
    if (p->iterations <= 4 * INT_WG)
      int_ransac_launch<4>(c, nb, dbk, dmem, p->iterations, eps, dwin);
    else if (p->iterations <= 8 * INT_WG)
      int_ransac_launch<8>(c, nb, dbk, dmem, p->iterations, eps, dwin);
    else
      int_ransac_launch<16>(c, nb, dbk, dmem, p->iterations, eps, dwin);
  }
  CHK(c, hipGetLastError());
  std::vector<bs_int_winner> win(bk.size());
  CHK(c, hipMemcpyAsync(win.data(), dwin, win.size() * sizeof(bs_int_winner),
                        hipMemcpyDeviceToHost, c->stream));
  CHK(c, hipStreamSynchronize(c->stream));

  /* refit: round 0 gates with the winner's line, every later round with the
   * line fitted to the current set; a bucket leaves when its count stops
   * growing, after 10 fits, or when a fit is degenerate */
  struct fit_state {
    u64 m[6] = {0, 0, 0, 0, 0, 0}; /* current set */
    bool have = false, rejected = false, done = false;
    int fits = 0;
  };
  std::vector<fit_state> fs(bk.size());
  for (int i = 0; i < nb; ++i) {
    bk[i].a = win[i].a;
    bk[i].b = win[i].b;
    bk[i].active = win[i].count > 0;
    if (!bk[i].active) fs[i].rejected = fs[i].done = true;
  }
  for (int round = 0; round <= 10; ++round) {
    bool any = false;
    for (int i = 0; i < nb; ++i) any = any || bk[i].active;
    if (!any) break;
    CHK(c, hipMemcpyAsync(dbk, bk.data(), bk.size() * sizeof(bs_int_bucket),
                          hipMemcpyHostToDevice, c->stream));
    {
      bs_tim t(c, BS_K_INT_MOMENTS);
      hipLaunchKernelGGL(k_int_moments<true>, dim3(nb), dim3(INT_WG), 0,
                         c->stream, dbk, st.dP, st.dQ, st.dcA, st.dcB, dx, dy,
                         dmem, eps, dsums);
    }
    CHK(c, hipGetLastError());
    sums.resize(bk.size() * 6);
    CHK(c, hipMemcpyAsync(sums.data(), dsums, sums.size() * sizeof(u64),
                          hipMemcpyDeviceToHost, c->stream));
    CHK(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < nb; ++i) {
      if (!bk[i].active) continue;
      fit_state &f = fs[i];
      const u64 *m = &sums[(size_t)i * 6];
      if (f.have && m[0] <= f.m[0]) { /* did not grow: keep the last set */
        f.done = true;
        bk[i].active = 0;
        continue;
      }
      std::memcpy(f.m, m, sizeof(f.m));
      f.have = true;
      double a, b;
      if (!bsint::line_fit(f.m[0], f.m[1], f.m[2], f.m[3], f.m[5], &a, &b)) {
        f.rejected = f.done = true;
        bk[i].active = 0;
        continue;
      }
      if (f.fits == 10) { /* ten refit rounds done: this set is final */
        f.done = true;
        bk[i].active = 0;
        continue;
      }
      ++f.fits;
      bk[i].a = (float)a;
      bk[i].b = (float)b;
    }
  }
  flush_stats(c);

  std::vector<bs_intensity_match> kept;
  for (int i = 0; i < nb; ++i) {
    const fit_state &f = fs[i];
    if (f.rejected || !f.have) continue;
    double a, b;
    if (!bsint::line_fit(f.m[0], f.m[1], f.m[2], f.m[3], f.m[5], &a, &b))
      continue;
    if ((long long)f.m[0] < (long long)p->min_num_inliers ||
        (double)f.m[0] < p->min_inlier_ratio * (double)bk[i].n)
      continue;
    bs_intensity_match r;
    r.cell_a = bk[i].ca;
    r.cell_b = bk[i].cb;
    r.n_cand = (u64)bk[i].n;
    r.n_inl = f.m[0];
    r.best_it = (u64)win[i].it;
    r.n_inl_first = (u64)win[i].count;
    r.sp = f.m[1];
    r.sq = f.m[2];
    r.spp = f.m[3];
    r.sqq = f.m[4];
    r.spq = f.m[5];
    r.a = a;
    r.b = b / 8.0;
    kept.push_back(r);
  }
  *n_found = kept.size();
  const size_t nw = std::min(kept.size(), capacity);
  if (nw) std::memcpy(out, kept.data(), nw * sizeof(bs_intensity_match));
  return BS_OK;
}

#endif /* BS_INTENSITY_MATCH_H */
