/* ip_match.h — interest-point descriptor matching (bs_match_descriptors),
 * included at the end of bigstitch.hip. Contract: tests/match_ref.py; the
 * [PIN-*] tags used below are spelled out there and in DESIGN.md §4.
 *
 * Three kernels, all built on the same idea: the thread owns one query in
 * registers, the searched set streams through LDS in tiles of IP_TILE
 * entries, and every lane of a wave reads the SAME entry at a time — a
 * broadcast read, which has no bank conflicts whatever the stride.
 *   k_ip_knn<K>       thread = point; K-entry sorted list in registers
 *   k_ip_descriptors  thread = descriptor; gathers the relative vectors
 *   k_ip_match<NV,R>  thread = A descriptor (NV float4 in registers); tracks
 *                     best / best index / second over a slice of B; slices
 *                     (gridDim.y) are merged in index order by k_ip_merge
 */
#ifndef BS_IP_MATCH_H
#define BS_IP_MATCH_H

#define IP_TILE 256 /* set entries per LDS tile = threads per block */
#define IP_KMAX 8
#define IP_NMAX 6
#define IP_CMAX 70  /* C(8, 4) */

struct bs_ip_comb { /* [PIN-RGLDM] subsets, lexicographic, as neighbour ranks */
  unsigned char m[IP_CMAX][IP_NMAX];
};

/* [PIN-KNN]. pts.w is unused. A candidate enters the list only when it is
 * strictly closer than the current worst, and inside the list it settles
 * behind every entry that is not farther: on an ascending scan that is the
 * lower-index-first rule. */
template <int K>
__global__ __launch_bounds__(IP_TILE) void k_ip_knn(
    const float4 *__restrict__ pts, int n, int *__restrict__ idx,
    float *__restrict__ d2) {
  __shared__ float4 tile[IP_TILE];
  const int q = blockIdx.x * IP_TILE + threadIdx.x;
  const float4 p = q < n ? pts[q] : make_float4(0.f, 0.f, 0.f, 0.f);
  float bd[K];
  int bi[K];
#pragma unroll
  for (int s = 0; s < K; ++s) {
    bd[s] = INFINITY;
    bi[s] = -1;
  }
  for (int t0 = 0; t0 < n; t0 += IP_TILE) {
    __syncthreads();
    if (t0 + (int)threadIdx.x < n) tile[threadIdx.x] = pts[t0 + threadIdx.x];
    __syncthreads();
    const int cnt = min(IP_TILE, n - t0);
    for (int c = 0; c < cnt; ++c) {
      const float4 b = tile[c];
      const float dx = b.x - p.x, dy = b.y - p.y, dz = b.z - p.z;
      float cd = dx * dx + dy * dy + dz * dz;
      int ci = t0 + c;
      if (ci != q && cd < bd[K - 1]) {
        bool ins = false;
#pragma unroll
        for (int s = 0; s < K; ++s) {
          ins = ins || cd < bd[s];
          if (ins) { /* from its slot on, every entry moves down by one */
            const float td = bd[s];
            const int ti = bi[s];
            bd[s] = cd;
            bi[s] = ci;
            cd = td;
            ci = ti;
          }
        }
      }
    }
  }
  if (q < n) {
#pragma unroll
    for (int s = 0; s < K; ++s) {
      idx[(size_t)q * K + s] = bi[s];
      d2[(size_t)q * K + s] = bd[s];
    }
  }
}

/* [PIN-RGLDM]: descriptor g = point * C + subset; its 3n floats q_j - p are
 * followed by zeros up to s4 float4 (zeros add nothing to a distance).
 * base[g] = the point itself, for the search-radius test. */
__global__ __launch_bounds__(256) void k_ip_descriptors(
    const float4 *__restrict__ pts, const int *__restrict__ knn, int npts,
    int K, int n, int C, int s4, bs_ip_comb comb, float *__restrict__ desc,
    float4 *__restrict__ base) {
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  if (g >= (long)npts * C) return;
  const int pi = (int)(g / C), s = (int)(g % C);
  const float4 p = pts[pi];
  float *o = desc + (size_t)g * s4 * 4;
  for (int j = 0; j < n; ++j) {
    const float4 qv = pts[knn[(size_t)pi * K + comb.m[s][j]]];
    o[3 * j + 0] = qv.x - p.x;
    o[3 * j + 1] = qv.y - p.y;
    o[3 * j + 2] = qv.z - p.z;
  }
  for (int i = 3 * n; i < 4 * s4; ++i) o[i] = 0.f;
  base[g] = p;
}

/* [PIN-DESCDIST] + [PIN-RATIO] scan. Block (x, y) = 256 A descriptors x
 * slice y of B (tiles_per_slice tiles). Strict < on an ascending scan keeps
 * the lower B index on equal distance; `second` is the second smallest
 * value, equal to best when the minimum occurs twice. The eligibility
 * distance is formed with explicitly rounded steps so that it is the same
 * number the reference forms in float32 (no fused multiply-add). */
template <int NV, bool RAD>
__global__ __launch_bounds__(IP_TILE) void k_ip_match(
    const float4 *__restrict__ da, const float4 *__restrict__ basea, int nda,
    const float4 *__restrict__ db, const float4 *__restrict__ baseb, int ndb,
    int tiles_per_slice, float inv_n, float r2, float *__restrict__ pbest,
    float *__restrict__ psecond, int *__restrict__ pbi) {
  __shared__ float4 tb[IP_TILE * NV];
  __shared__ float4 bb[RAD ? IP_TILE : 1];
  const int i = blockIdx.x * IP_TILE + threadIdx.x;
  float4 a[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v)
    a[v] = i < nda ? da[(size_t)i * NV + v] : make_float4(0.f, 0.f, 0.f, 0.f);
  float4 pa = make_float4(0.f, 0.f, 0.f, 0.f);
  if (RAD && i < nda) pa = basea[i];
  float best = INFINITY, second = INFINITY;
  int bi = -1;
  const long lo = (long)blockIdx.y * tiles_per_slice * IP_TILE;
  const int t_end = (int)min((long)ndb, lo + (long)tiles_per_slice * IP_TILE);
  for (int t0 = (int)min(lo, (long)ndb); t0 < t_end; t0 += IP_TILE) {
    const int cnt = min(IP_TILE, t_end - t0);
    __syncthreads();
    for (int e = threadIdx.x; e < cnt * NV; e += IP_TILE)
      tb[e] = db[(size_t)t0 * NV + e];
    if (RAD && (int)threadIdx.x < cnt) bb[threadIdx.x] = baseb[t0 + threadIdx.x];
    __syncthreads();
#pragma unroll 2
    for (int c = 0; c < cnt; ++c) {
      float s = 0.f;
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        const float4 b = tb[c * NV + v];
        const float ex = a[v].x - b.x, ey = a[v].y - b.y, ez = a[v].z - b.z,
                    ew = a[v].w - b.w;
        s = fmaf(ex, ex, s);
        s = fmaf(ey, ey, s);
        s = fmaf(ez, ez, s);
        s = fmaf(ew, ew, s);
      }
      const float d = s * inv_n;
      bool ok = true;
      if (RAD) {
        const float4 pb = bb[c];
        const float dx = pa.x - pb.x, dy = pa.y - pb.y, dz = pa.z - pb.z;
        const float bd2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx),
                                              __fmul_rn(dy, dy)),
                                    __fmul_rn(dz, dz));
        ok = bd2 <= r2;
      }
      if (ok) {
        if (d < best) {
          second = best;
          best = d;
          bi = t0 + c;
        } else if (d < second) {
          second = d;
        }
      }
    }
  }
  if (i < nda) {
    const size_t o = (size_t)blockIdx.y * nda + i;
    pbest[o] = best;
    psecond[o] = second;
    pbi[o] = bi;
  }
}

/* Merge the slices in ascending B order. Earlier slice = lower indices, so
 * it wins an equal distance; the union's second smallest is the smaller of
 * the losing best and the winning side's own second. */
__global__ __launch_bounds__(256) void k_ip_merge(
    const float *__restrict__ pbest, const float *__restrict__ psecond,
    const int *__restrict__ pbi, int nda, int slices, float *__restrict__ best,
    float *__restrict__ second, int *__restrict__ bi) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nda) return;
  float b = pbest[i], s = psecond[i];
  int k = pbi[i];
  for (int y = 1; y < slices; ++y) {
    const size_t o = (size_t)y * nda + i;
    const float b2 = pbest[o], s2 = psecond[o];
    if (b2 < b) {
      s = fminf(b, s2);
      b = b2;
      k = pbi[o];
    } else {
      s = fminf(s, b2);
    }
  }
  best[i] = b;
  second[i] = s;
  bi[i] = k;
}

/* ------------------------------------------------------------------ host */

enum { IPB_PTS_A, IPB_PTS_B, IPB_KNN_A, IPB_KNN_B, IPB_KD2, IPB_DESC_A,
       IPB_DESC_B, IPB_BASE_A, IPB_BASE_B, IPB_PART, IPB_FINAL, IPB_COUNT };

static int ip_buf(bs_ctx *c, int which, size_t bytes, void **out) {
  int rc = ensure_dev(c, &c->ip_buf[which], &c->ip_cap[which],
                      std::max(bytes, (size_t)16));
  *out = c->ip_buf[which];
  return rc;
}

static int ip_check_params(bs_ctx *c, const bs_match_params *p) {
  const int n = p->num_neighbors, r = p->redundancy;
  if (n < 1 || r < 0 || n + r > IP_KMAX || n > IP_NMAX) {
    c->err = "match: needs n >= 1, r >= 0, n + r <= 8, n <= 6";
    return BS_EUNSUP;
  }
  if (p->limit_search_radius && !(p->search_radius >= 0.0)) {
    c->err = "match: negative search radius";
    return BS_EINVAL;
  }
  return BS_OK;
}

static int ip_subsets(int n, int k, bs_ip_comb *cb) {
  int C = 0, pick[IP_NMAX];
  for (int j = 0; j < n; ++j) pick[j] = j;
  for (;;) {
    for (int j = 0; j < n; ++j) cb->m[C][j] = (unsigned char)pick[j];
    ++C;
    int j = n - 1;
    while (j >= 0 && pick[j] == k - n + j) --j;
    if (j < 0) break;
    ++pick[j];
    for (int q = j + 1; q < n; ++q) pick[q] = pick[q - 1] + 1;
  }
  return C;
}

/* [PIN-F32PTS] with a caller-chosen origin */
static int ip_to_f32(bs_ctx *c, const double *pts, size_t n,
                     const double mn[3], std::vector<float4> &out) {
  out.resize(n);
  for (size_t i = 0; i < n; ++i) {
    float v[3];
    for (int d = 0; d < 3; ++d) {
      const double x = pts[3 * i + d];
      if (!std::isfinite(x)) {
        c->err = "match: non-finite coordinate";
        return BS_EINVAL;
      }
      v[d] = (float)(x - mn[d]);
    }
    out[i] = make_float4(v[0], v[1], v[2], 0.f);
  }
  return BS_OK;
}

template <int K>
static void ip_knn_launch_k(bs_ctx *c, const float4 *dp, int n, int *didx,
                            float *dd2) {
  hipLaunchKernelGGL(k_ip_knn<K>, dim3((n + IP_TILE - 1) / IP_TILE),
                     dim3(IP_TILE), 0, c->stream, dp, n, didx, dd2);
}

static void ip_knn_launch(bs_ctx *c, const float4 *dp, int n, int K, int *didx,
                          float *dd2) {
  bs_tim t(c, BS_K_IP_KNN);
  switch (K) {
    case 1: ip_knn_launch_k<1>(c, dp, n, didx, dd2); break;
    case 2: ip_knn_launch_k<2>(c, dp, n, didx, dd2); break;
    case 3: ip_knn_launch_k<3>(c, dp, n, didx, dd2); break;
    case 4: ip_knn_launch_k<4>(c, dp, n, didx, dd2); break;
    case 5: ip_knn_launch_k<5>(c, dp, n, didx, dd2); break;
    case 6: ip_knn_launch_k<6>(c, dp, n, didx, dd2); break;
    case 7: ip_knn_launch_k<7>(c, dp, n, didx, dd2); break;
    default: ip_knn_launch_k<8>(c, dp, n, didx, dd2); break;
  }
}

template <int NV>
static void ip_match_launch_nv(bs_ctx *c, dim3 grid, bool rad,
                               const float4 *da, const float4 *ba, int nda,
                               const float4 *db, const float4 *bb, int ndb,
                               int tps, float inv_n, float r2, float *pb,
                               float *ps, int *pi) {
  if (rad)
    hipLaunchKernelGGL((k_ip_match<NV, true>), grid, dim3(IP_TILE), 0,
                       c->stream, da, ba, nda, db, bb, ndb, tps, inv_n, r2, pb,
                       ps, pi);
  else
    hipLaunchKernelGGL((k_ip_match<NV, false>), grid, dim3(IP_TILE), 0,
                       c->stream, da, ba, nda, db, bb, ndb, tps, inv_n, r2, pb,
                       ps, pi);
}

/* Everything up to the merged per-A-descriptor arrays, downloaded. Returns
 * with *C_out = descriptors per point and empty vectors when either set is
 * too small for a descriptor. Caller holds c->mu and has set the device. */
static int ip_match_raw(bs_ctx *c, const double *pts_a, size_t na,
                        const double *pts_b, size_t nb,
                        const bs_match_params *p, std::vector<float> &best,
                        std::vector<float> &second, std::vector<int> &bidx,
                        int *C_out) {
  int rc = ip_check_params(c, p);
  if (rc) return rc;
  const int n = p->num_neighbors, K = n + p->redundancy;
  bs_ip_comb comb;
  std::memset(&comb, 0, sizeof(comb));
  const int C = ip_subsets(n, K, &comb);
  *C_out = C;
  best.clear();
  second.clear();
  bidx.clear();
  if ((na > 0 && !pts_a) || (nb > 0 && !pts_b)) return BS_EINVAL;
  if (na * (size_t)C >= 0x7FFFFFFFull || nb * (size_t)C >= 0x7FFFFFFFull) {
    c->err = "match: 2^31 descriptors or more in one set";
    return BS_EUNSUP;
  }
  double mn[3] = {0, 0, 0};
  for (int d = 0; d < 3; ++d) { /* [PIN-F32PTS]: minimum over the union */
    double m = INFINITY;
    for (size_t i = 0; i < na; ++i) m = std::min(m, pts_a[3 * i + d]);
    for (size_t i = 0; i < nb; ++i) m = std::min(m, pts_b[3 * i + d]);
    if (na + nb) mn[d] = m;
  }
  std::vector<float4> ha, hb;
  if ((rc = ip_to_f32(c, pts_a, na, mn, ha)) ||
      (rc = ip_to_f32(c, pts_b, nb, mn, hb)))
    return rc;
  if (na <= (size_t)K || nb <= (size_t)K) return BS_OK; /* [PIN-KNN] */

  const int s4 = (3 * n + 3) / 4; /* float4 per descriptor */
  const int nda = (int)(na * C), ndb = (int)(nb * C);
  float4 *dpa, *dpb, *dda, *ddb, *dba, *dbb;
  int *dka, *dkb;
  float *dkd;
  if ((rc = ip_buf(c, IPB_PTS_A, na * 16, (void **)&dpa)) ||
      (rc = ip_buf(c, IPB_PTS_B, nb * 16, (void **)&dpb)) ||
      (rc = ip_buf(c, IPB_KNN_A, na * K * 4, (void **)&dka)) ||
      (rc = ip_buf(c, IPB_KNN_B, nb * K * 4, (void **)&dkb)) ||
      (rc = ip_buf(c, IPB_KD2, std::max(na, nb) * K * 4, (void **)&dkd)) ||
      (rc = ip_buf(c, IPB_DESC_A, (size_t)nda * s4 * 16, (void **)&dda)) ||
      (rc = ip_buf(c, IPB_DESC_B, (size_t)ndb * s4 * 16, (void **)&ddb)) ||
      (rc = ip_buf(c, IPB_BASE_A, (size_t)nda * 16, (void **)&dba)) ||
      (rc = ip_buf(c, IPB_BASE_B, (size_t)ndb * 16, (void **)&dbb)))
    return rc;
  CHK(c, hipMemcpyAsync(dpa, ha.data(), na * 16, hipMemcpyHostToDevice,
                        c->stream));
  CHK(c, hipMemcpyAsync(dpb, hb.data(), nb * 16, hipMemcpyHostToDevice,
                        c->stream));
  ip_knn_launch(c, dpa, (int)na, K, dka, dkd);
  {
    bs_tim t(c, BS_K_IP_DESC);
    hipLaunchKernelGGL(k_ip_descriptors, dim3((nda + 255) / 256), dim3(256), 0,
                       c->stream, dpa, dka, (int)na, K, n, C, s4, comb,
                       (float *)dda, dba);
  }
  ip_knn_launch(c, dpb, (int)nb, K, dkb, dkd);
  {
    bs_tim t(c, BS_K_IP_DESC);
    hipLaunchKernelGGL(k_ip_descriptors, dim3((ndb + 255) / 256), dim3(256), 0,
                       c->stream, dpb, dkb, (int)nb, K, n, C, s4, comb,
                       (float *)ddb, dbb);
  }
  /* Split B over gridDim.y until the grid has ~8 blocks per CU (256 CUs);
   * a slice is a whole number of tiles and no slice is empty. */
  const int gx = (nda + IP_TILE - 1) / IP_TILE;
  const int ntile = (ndb + IP_TILE - 1) / IP_TILE;
  int want = c->ip_split > 0 ? c->ip_split : (2048 + gx - 1) / gx;
  want = std::max(1, std::min(std::min(want, ntile), 65535));
  const int tps = (ntile + want - 1) / want;
  const int gy = (ntile + tps - 1) / tps;
  float *dpart, *dfin;
  if ((rc = ip_buf(c, IPB_PART, (size_t)gy * nda * 12, (void **)&dpart)) ||
      (rc = ip_buf(c, IPB_FINAL, (size_t)nda * 12, (void **)&dfin)))
    return rc;
  float *pb_ = dpart, *ps_ = dpart + (size_t)gy * nda;
  int *pi_ = (int *)(dpart + (size_t)2 * gy * nda);
  float *fb = dfin, *fs = dfin + nda;
  int *fi = (int *)(dfin + (size_t)2 * nda);
  const bool rad = p->limit_search_radius != 0;
  const float r2 = (float)(p->search_radius * p->search_radius);
  const float inv_n = 1.0f / (float)n;
  {
    bs_tim t(c, BS_K_IP_MATCH);
    const dim3 grid(gx, gy);
    switch (s4) {
      case 1: ip_match_launch_nv<1>(c, grid, rad, dda, dba, nda, ddb, dbb, ndb,
                                    tps, inv_n, r2, pb_, ps_, pi_); break;
      case 2: ip_match_launch_nv<2>(c, grid, rad, dda, dba, nda, ddb, dbb, ndb,
                                    tps, inv_n, r2, pb_, ps_, pi_); break;
      case 3: ip_match_launch_nv<3>(c, grid, rad, dda, dba, nda, ddb, dbb, ndb,
                                    tps, inv_n, r2, pb_, ps_, pi_); break;
      case 4: ip_match_launch_nv<4>(c, grid, rad, dda, dba, nda, ddb, dbb, ndb,
                                    tps, inv_n, r2, pb_, ps_, pi_); break;
      default: ip_match_launch_nv<5>(c, grid, rad, dda, dba, nda, ddb, dbb,
                                     ndb, tps, inv_n, r2, pb_, ps_, pi_); break;
    }
    hipLaunchKernelGGL(k_ip_merge, dim3((nda + 255) / 256), dim3(256), 0,
                       c->stream, pb_, ps_, pi_, nda, gy, fb, fs, fi);
  }
  CHK(c, hipGetLastError());
  best.resize(nda);
  second.resize(nda);
  bidx.resize(nda);
  CHK(c, hipMemcpyAsync(best.data(), fb, (size_t)nda * 4,
                        hipMemcpyDeviceToHost, c->stream));
  CHK(c, hipMemcpyAsync(second.data(), fs, (size_t)nda * 4,
                        hipMemcpyDeviceToHost, c->stream));
  CHK(c, hipMemcpyAsync(bidx.data(), fi, (size_t)nda * 4,
                        hipMemcpyDeviceToHost, c->stream));
  CHK(c, hipStreamSynchronize(c->stream));
  flush_stats(c);
  return BS_OK;
}

extern "C" int bs_debug_ip_knn(bs_ctx *c, const double *pts, size_t n,
                               int32_t k, int32_t *idx_out, float *d2_out) {
  if (!c || (n > 0 && (!pts || !idx_out || !d2_out))) return BS_EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  CHK(c, hipSetDevice(c->dev));
  if (k < 1 || k > IP_KMAX || n >= 0x7FFFFFFFull / IP_KMAX) {
    c->err = "debug_ip_knn: needs 1 <= k <= 8";
    return BS_EUNSUP;
  }
  if (n <= (size_t)k) { /* [PIN-KNN]: too few points for a full list */
    for (size_t i = 0; i < n * k; ++i) {
      idx_out[i] = -1;
      d2_out[i] = INFINITY;
    }
    return BS_OK;
  }
  const double zero[3] = {0, 0, 0};
  std::vector<float4> h;
  int rc = ip_to_f32(c, pts, n, zero, h);
  if (rc) return rc;
  float4 *dp;
  int *dk;
  float *dd;
  if ((rc = ip_buf(c, IPB_PTS_A, n * 16, (void **)&dp)) ||
      (rc = ip_buf(c, IPB_KNN_A, n * k * 4, (void **)&dk)) ||
      (rc = ip_buf(c, IPB_KD2, n * k * 4, (void **)&dd)))
    return rc;
  CHK(c, hipMemcpyAsync(dp, h.data(), n * 16, hipMemcpyHostToDevice,
                        c->stream));
  ip_knn_launch(c, dp, (int)n, k, dk, dd);
  CHK(c, hipGetLastError());
  CHK(c, hipMemcpyAsync(idx_out, dk, n * k * 4, hipMemcpyDeviceToHost,
                        c->stream));
  CHK(c, hipMemcpyAsync(d2_out, dd, n * k * 4, hipMemcpyDeviceToHost,
                        c->stream));
  CHK(c, hipStreamSynchronize(c->stream));
  flush_stats(c);
  return BS_OK;
}

extern "C" int bs_debug_ip_match(bs_ctx *c, const double *pts_a, size_t na,
                                 const double *pts_b, size_t nb,
                                 const bs_match_params *p, float *best_out,
                                 float *second_out, int32_t *best_b_out) {
  if (!c || !p) return BS_EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  CHK(c, hipSetDevice(c->dev));
  std::vector<float> best, second;
  std::vector<int> bi;
  int C = 0;
  int rc = ip_match_raw(c, pts_a, na, pts_b, nb, p, best, second, bi, &C);
  if (rc) return rc;
  if (!best.empty() && (!best_out || !second_out || !best_b_out))
    return BS_EINVAL;
  if (!best.empty()) {
    std::memcpy(best_out, best.data(), best.size() * 4);
    std::memcpy(second_out, second.data(), second.size() * 4);
    std::memcpy(best_b_out, bi.data(), bi.size() * 4);
  }
  return BS_OK;
}

extern "C" int bs_match_descriptors(bs_ctx *c, const double *pts_a, size_t na,
                                    const double *pts_b, size_t nb,
                                    const bs_match_params *p,
                                    bs_match_candidate *out, size_t capacity,
                                    size_t *n_found) {
  if (!c || !p || !n_found || (capacity > 0 && !out)) return BS_EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  CHK(c, hipSetDevice(c->dev));
  std::vector<float> best, second;
  std::vector<int> bi;
  int C = 0;
  int rc = ip_match_raw(c, pts_a, na, pts_b, nb, p, best, second, bi, &C);
  if (rc) return rc;
  /* [PIN-RATIO] on the float32 values */
  std::vector<bs_match_candidate> kept;
  const float ratio = p->ratio_of_distance, thr = p->difference_threshold;
  for (size_t i = 0; i < best.size(); ++i) {
    if (bi[i] < 0 || !(second[i] < INFINITY)) continue;
    if (best[i] * ratio <= second[i] && best[i] < thr)
      kept.push_back({(int32_t)(i / C), (int32_t)(bi[i] / C), best[i],
                      second[i]});
  }
  /* [PIN-AMBIG]: unique pairs (the descriptor match with the smallest best
   * represents the pair; stable sort keeps the lower descriptor on a tie) */
  std::stable_sort(kept.begin(), kept.end(),
                   [](const bs_match_candidate &x, const bs_match_candidate &y) {
                     if (x.a != y.a) return x.a < y.a;
                     if (x.b != y.b) return x.b < y.b;
                     return x.best < y.best;
                   });
  kept.erase(std::unique(kept.begin(), kept.end(),
                         [](const bs_match_candidate &x,
                            const bs_match_candidate &y) {
                           return x.a == y.a && x.b == y.b;
                         }),
             kept.end());
  std::vector<int> cnt_a(na, 0), cnt_b(nb, 0);
  for (const auto &k : kept) {
    ++cnt_a[k.a];
    ++cnt_b[k.b];
  }
  kept.erase(std::remove_if(kept.begin(), kept.end(),
                            [&](const bs_match_candidate &k) {
                              return cnt_a[k.a] != 1 || cnt_b[k.b] != 1;
                            }),
             kept.end());
  *n_found = kept.size();
  const size_t nw = std::min(kept.size(), capacity);
  if (nw) std::memcpy(out, kept.data(), nw * sizeof(bs_match_candidate));
  return BS_OK;
}

#endif /* BS_IP_MATCH_H */
