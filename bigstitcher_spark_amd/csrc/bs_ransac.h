/* bs_ransac.h — host-only RANSAC over interest-point correspondences
 * ([PIN-RANSAC], bs_ransac in include/bigstitch.h). Plain C++17 with no HIP
 * in it: bigstitch.hip includes it for the library, and
 * tests/ransac_host.cpp includes it for a stand-alone program that can be
 * built with a host sanitizer.
 *
 * Restated from the published method (Fischler & Bolles 1981; the refit
 * loop follows mpicbg's RANSAC as called through the reference's
 * SparkGeometricDescriptorMatching.java:564-621 with the models of
 * AbstractRegistration.java:110-140); mpicbg is not part of the reference
 * tree. Every model maps A onto B: pb ~ M * (pa, 1), M row-major 3x4.
 *   generator   xorshift64* (Vigna 2016), state seeded with BS_RANSAC_SEED
 *               at every call, so the same input gives the same output
 *   draw        `minimal` distinct indices by rejection, index = r % n
 *   models      TRANSLATION mean difference; RIGID Horn 1987 (unit
 *               quaternion = dominant eigenvector of the 4x4 N matrix, by
 *               cyclic Jacobi); AFFINE least squares about the centroids,
 *               refused when the A scatter matrix is singular (coplanar)
 *   [PIN-INTERP] regularised model = (1 - lambda) * M_model + lambda * M_reg
 *               entry by entry; minimal set = the larger of the two minima
 */
#ifndef BS_RANSAC_H
#define BS_RANSAC_H

#include "../../include/bigstitch.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#define BS_RANSAC_SEED 0x9E3779B97F4A7C15ull

namespace bs_ransac_impl {

struct rng {
  uint64_t s;
  uint64_t next() {
    s ^= s >> 12;
    s ^= s << 25;
    s ^= s >> 27;
    return s * 0x2545F4914F6CDD1Dull;
  }
};

static inline int min_points(int model) {
  switch (model) {
    case BS_MODEL_TRANSLATION: return 1;
    case BS_MODEL_RIGID: return 3;
    case BS_MODEL_AFFINE: return 4;
    default: return 0; /* IDENTITY / NONE */
  }
}

static inline void identity(double M[12]) {
  std::memset(M, 0, 12 * sizeof(double));
  M[0] = M[5] = M[10] = 1.0;
}

static void centroids(const double *pa, const double *pb, const int *ix, int m,
                      double ca[3], double cb[3]) {
  for (int d = 0; d < 3; ++d) ca[d] = cb[d] = 0.0;
  for (int i = 0; i < m; ++i)
    for (int d = 0; d < 3; ++d) {
      ca[d] += pa[3 * (size_t)ix[i] + d];
      cb[d] += pb[3 * (size_t)ix[i] + d];
    }
  for (int d = 0; d < 3; ++d) {
    ca[d] /= m;
    cb[d] /= m;
  }
}

/* dominant eigenvector of a symmetric 4x4 by cyclic Jacobi */
static void eig4_max(double A[4][4], double q[4]) {
  double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
  for (int sweep = 0; sweep < 64; ++sweep) {
    double off = 0.0;
    for (int i = 0; i < 4; ++i)
      for (int j = i + 1; j < 4; ++j) off += A[i][j] * A[i][j];
    if (off < 1e-300) break;
    for (int p = 0; p < 4; ++p)
      for (int r = p + 1; r < 4; ++r) {
        if (A[p][r] == 0.0) continue;
        const double th = (A[r][r] - A[p][p]) / (2.0 * A[p][r]);
        const double t = (th >= 0 ? 1.0 : -1.0) /
                         (std::fabs(th) + std::sqrt(th * th + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < 4; ++k) { /* A <- A J */
          const double akp = A[k][p], akr = A[k][r];
          A[k][p] = c * akp - s * akr;
          A[k][r] = s * akp + c * akr;
        }
        for (int k = 0; k < 4; ++k) { /* A <- J^T A */
          const double apk = A[p][k], ark = A[r][k];
          A[p][k] = c * apk - s * ark;
          A[r][k] = s * apk + c * ark;
        }
        for (int k = 0; k < 4; ++k) {
          const double vkp = V[k][p], vkr = V[k][r];
          V[k][p] = c * vkp - s * vkr;
          V[k][r] = s * vkp + c * vkr;
        }
      }
  }
  int best = 0;
  for (int i = 1; i < 4; ++i)
    if (A[i][i] > A[best][best]) best = i;
  for (int k = 0; k < 4; ++k) q[k] = V[k][best];
}

static bool fit_one(int model, const double *pa, const double *pb,
                    const int *ix, int m, double M[12]) {
  if (model == BS_MODEL_IDENTITY) {
    identity(M);
    return true;
  }
  if (m < min_points(model)) return false;
  double ca[3], cb[3];
  centroids(pa, pb, ix, m, ca, cb);
  if (model == BS_MODEL_TRANSLATION) {
    identity(M);
    for (int d = 0; d < 3; ++d) M[4 * d + 3] = cb[d] - ca[d];
    return true;
  }
  /* S[i][j] = sum (a - ca)_i (b - cb)_j ; Q[i][j] = sum (a-ca)_i (a-ca)_j */
  double S[3][3] = {}, Q[3][3] = {};
  for (int i = 0; i < m; ++i) {
    double a[3], b[3];
    for (int d = 0; d < 3; ++d) {
      a[d] = pa[3 * (size_t)ix[i] + d] - ca[d];
      b[d] = pb[3 * (size_t)ix[i] + d] - cb[d];
    }
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) {
        S[r][c] += a[r] * b[c];
        Q[r][c] += a[r] * a[c];
      }
  }
  double R[3][3];
  if (model == BS_MODEL_RIGID) {
    double N[4][4] = {
        {S[0][0] + S[1][1] + S[2][2], S[1][2] - S[2][1], S[2][0] - S[0][2],
         S[0][1] - S[1][0]},
        {S[1][2] - S[2][1], S[0][0] - S[1][1] - S[2][2], S[0][1] + S[1][0],
         S[2][0] + S[0][2]},
        {S[2][0] - S[0][2], S[0][1] + S[1][0], -S[0][0] + S[1][1] - S[2][2],
         S[1][2] + S[2][1]},
        {S[0][1] - S[1][0], S[2][0] + S[0][2], S[1][2] + S[2][1],
         -S[0][0] - S[1][1] + S[2][2]}};
    double q[4];
    eig4_max(N, q);
    const double nq = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] +
                                q[3] * q[3]);
    if (!(nq > 0.0)) return false;
    const double w = q[0] / nq, x = q[1] / nq, y = q[2] / nq, z = q[3] / nq;
    R[0][0] = w * w + x * x - y * y - z * z;
    R[0][1] = 2 * (x * y - w * z);
    R[0][2] = 2 * (x * z + w * y);
    R[1][0] = 2 * (x * y + w * z);
    R[1][1] = w * w - x * x + y * y - z * z;
    R[1][2] = 2 * (y * z - w * x);
    R[2][0] = 2 * (x * z - w * y);
    R[2][1] = 2 * (y * z + w * x);
    R[2][2] = w * w - x * x - y * y + z * z;
  } else if (model == BS_MODEL_AFFINE) {
    /* R = S^T Q^-1 ; Q symmetric 3x3, inverse by cofactors */
    double K[3][3];
    K[0][0] = Q[1][1] * Q[2][2] - Q[1][2] * Q[2][1];
    K[0][1] = Q[0][2] * Q[2][1] - Q[0][1] * Q[2][2];
    K[0][2] = Q[0][1] * Q[1][2] - Q[0][2] * Q[1][1];
    K[1][0] = Q[1][2] * Q[2][0] - Q[1][0] * Q[2][2];
    K[1][1] = Q[0][0] * Q[2][2] - Q[0][2] * Q[2][0];
    K[1][2] = Q[0][2] * Q[1][0] - Q[0][0] * Q[1][2];
    K[2][0] = Q[1][0] * Q[2][1] - Q[1][1] * Q[2][0];
    K[2][1] = Q[0][1] * Q[2][0] - Q[0][0] * Q[2][1];
    K[2][2] = Q[0][0] * Q[1][1] - Q[0][1] * Q[1][0];
    const double det = Q[0][0] * K[0][0] + Q[0][1] * K[1][0] + Q[0][2] * K[2][0];
    const double scale = Q[0][0] + Q[1][1] + Q[2][2];
    /* coplanar (or fewer than four distinct) points: det is a rounding
     * residue of scale^3 */
    if (!(std::fabs(det) > 1e-12 * scale * scale * scale)) return false;
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) {
        double v = 0.0;
        for (int k = 0; k < 3; ++k) v += S[k][r] * K[k][c];
        R[r][c] = v / det;
      }
  } else {
    return false;
  }
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) M[4 * r + c] = R[r][c];
    M[4 * r + 3] = cb[r] - (R[r][0] * ca[0] + R[r][1] * ca[1] + R[r][2] * ca[2]);
  }
  return true;
}

static bool fit(const bs_ransac_params *p, const double *pa, const double *pb,
                const int *ix, int m, double M[12]) {
  if (!fit_one(p->model, pa, pb, ix, m, M)) return false;
  if (p->regularizer == BS_MODEL_NONE || p->lambda == 0.0) return true;
  double G[12];
  if (!fit_one(p->regularizer, pa, pb, ix, m, G)) return false;
  for (int i = 0; i < 12; ++i) /* [PIN-INTERP] */
    M[i] = (1.0 - p->lambda) * M[i] + p->lambda * G[i];
  return true;
}

static int inliers(const double M[12], const double *pa, const double *pb,
                   size_t n, double eps, std::vector<int> &out) {
  out.clear();
  const double e2 = eps * eps;
  for (size_t i = 0; i < n; ++i) {
    const double *a = pa + 3 * i, *b = pb + 3 * i;
    double d2 = 0.0;
    for (int r = 0; r < 3; ++r) {
      const double v = M[4 * r] * a[0] + M[4 * r + 1] * a[1] +
                       M[4 * r + 2] * a[2] + M[4 * r + 3] - b[r];
      d2 += v * v;
    }
    if (d2 <= e2) out.push_back((int)i);
  }
  return (int)out.size();
}

} /* namespace bs_ransac_impl */

extern "C" int bs_ransac(const double *pa, const double *pb, size_t n,
                         const bs_ransac_params *p, uint8_t *inlier_out,
                         double model_out[12], size_t *n_inliers) {
  using namespace bs_ransac_impl;
  if (!p || !n_inliers || (n > 0 && (!pa || !pb)) || n > 0x7FFFFFFFu)
    return BS_EINVAL;
  const bool model_ok = p->model == BS_MODEL_TRANSLATION ||
                        p->model == BS_MODEL_RIGID ||
                        p->model == BS_MODEL_AFFINE;
  const bool reg_ok = p->regularizer == BS_MODEL_NONE ||
                      p->regularizer == BS_MODEL_IDENTITY ||
                      p->regularizer == BS_MODEL_TRANSLATION ||
                      p->regularizer == BS_MODEL_RIGID ||
                      p->regularizer == BS_MODEL_AFFINE;
  if (!model_ok || !reg_ok || !(p->max_epsilon >= 0.0) || p->iterations < 0 ||
      !(p->lambda >= 0.0 && p->lambda <= 1.0))
    return BS_EINVAL;
  *n_inliers = 0;
  if (inlier_out && n) std::memset(inlier_out, 0, n);
  if (model_out) identity(model_out);
  int minimal = min_points(p->model);
  if (p->regularizer != BS_MODEL_NONE && p->lambda != 0.0)
    minimal = std::max(minimal, min_points(p->regularizer));
  if ((size_t)minimal > n || n == 0) return BS_OK;

  rng g = {BS_RANSAC_SEED};
  std::vector<int> best, cur, nxt;
  std::vector<int> pick((size_t)minimal);
  double bestM[12], M[12];
  identity(bestM);
  for (int it = 0; it < p->iterations; ++it) {
    for (int k = 0; k < minimal;) {
      const int c = (int)(g.next() % (uint64_t)n);
      bool dup = false;
      for (int j = 0; j < k; ++j) dup |= pick[(size_t)j] == c;
      if (!dup) pick[(size_t)k++] = c;
    }
    if (!fit(p, pa, pb, pick.data(), minimal, M)) continue;
    int cnt = inliers(M, pa, pb, n, p->max_epsilon, cur);
    if (cnt < minimal) continue;
    /* refit on the inliers until the set stops growing */
    for (;;) {
      double M2[12];
      if (!fit(p, pa, pb, cur.data(), cnt, M2)) break;
      const int c2 = inliers(M2, pa, pb, n, p->max_epsilon, nxt);
      if (c2 <= cnt) {
        /* keep the model that was fitted on the final set when that set
         * is still its own consensus */
        if (c2 == cnt && nxt == cur) std::memcpy(M, M2, sizeof(M));
        break;
      }
      cur.swap(nxt);
      cnt = c2;
      std::memcpy(M, M2, sizeof(M));
    }
    if (cnt > (int)best.size()) { /* ties: the earlier iteration stays */
      best = cur;
      std::memcpy(bestM, M, sizeof(M));
    }
  }
  const size_t nb = best.size();
  if (nb < (size_t)std::max(p->min_num_inliers, minimal) ||
      (double)nb / (double)n < p->min_inlier_ratio)
    return BS_OK;
  /* final model: refit on the inliers */
  double F[12];
  if (fit(p, pa, pb, best.data(), (int)nb, F)) std::memcpy(bestM, F, sizeof(F));
  if (inlier_out)
    for (int i : best) inlier_out[i] = 1;
  if (model_out) std::memcpy(model_out, bestM, sizeof(bestM));
  *n_inliers = nb;
  return BS_OK;
}

#endif /* BS_RANSAC_H */
