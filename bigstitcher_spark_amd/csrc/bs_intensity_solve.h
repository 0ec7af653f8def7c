/* bs_intensity_solve.h — host-only global intensity solve
 * (bs_intensity_solve) and the moment line fit shared with
 * bs_intensity_match_pair. Plain C++17, no HIP: included by bigstitch.hip
 * for the library, and directly by bin/solve-intensities and
 * tests/intensity_solve_host.cpp. Contract: tests/intensity_ref.py.
 *
 * [PIN-INT-SOLVE] unknowns (a_c, b_c) per (view, cell); minimise in double
 *   E = sum_buckets sum_inliers (a_i p + b_i - a_j q - b_j)^2
 *     + l_id sum_c (W_c + Wm) [s2 (a_c - 1)^2 + b_c^2]
 *     + l_sm Wm sum_{6-neighbour cells c, c' of one view}
 *                   [s2 (a_c - a_c')^2 + (b_c - b_c')^2]
 * with intensities in grey levels, W_c the inlier count touching cell c, Wm
 * the mean inlier count per bucket and s2 = (sum Spp + sum Sqq) / (2 sum n).
 * The first term is expanded exactly from the buckets' moments. The normal
 * equations are solved by Jacobi-preconditioned conjugate gradient from
 * a = 1, b = 0 until the residual, measured in the preconditioner's norm
 * relative to the right-hand side, is <= 1e-10, or max_iterations. */
#ifndef BS_INTENSITY_SOLVE_H
#define BS_INTENSITY_SOLVE_H

#include "../../include/bigstitch.h"

#include <cmath>
#include <cstring>
#include <vector>

namespace bsint {

/* Least-squares line q = a p + b from integer moments, exact numerator and
 * denominator. false when den <= 0 (no spread in p, or n == 0). */
inline bool line_fit(uint64_t n, uint64_t sp, uint64_t sq, uint64_t spp,
                     uint64_t spq, double *a, double *b) {
  const __int128 num = (__int128)n * spq - (__int128)sp * sq;
  const __int128 den = (__int128)n * spp - (__int128)sp * sp;
  if (den <= 0) return false;
  *a = (double)num / (double)den;
  const double t = *a * (double)sp;
  *b = ((double)sq - t) / (double)n;
  return true;
}

struct term { /* one bucket: unknown offsets and moments in grey levels */
  size_t ia, ib;
  double n, sp, sq, spp, sqq, spq;
};

struct system {
  int nviews = 0, cg[3] = {1, 1, 1};
  size_t ncell = 1;
  std::vector<term> terms;
  std::vector<double> wid; /* l_id (W_c + Wm) per (view, cell) */
  double s2 = 1.0, ksm = 0.0;

  size_t size() const { return (size_t)nviews * ncell * 2; }

  /* y = H x; with diag_only, y = diag(H) */
  void apply(const double *x, double *y, bool diag_only) const {
    const size_t N = size();
    for (size_t i = 0; i < N; ++i) y[i] = 0.0;
    for (const term &t : terms) {
      if (diag_only) {
        y[t.ia] += t.spp;
        y[t.ia + 1] += t.n;
        y[t.ib] += t.sqq;
        y[t.ib + 1] += t.n;
        continue;
      }
      const double ai = x[t.ia], bi = x[t.ia + 1], aj = x[t.ib],
                   bj = x[t.ib + 1];
      const double e1 = t.sp * ai + t.n * bi - t.sq * aj - t.n * bj;
      y[t.ia] += t.spp * ai + t.sp * bi - t.spq * aj - t.sp * bj;
      y[t.ia + 1] += e1;
      y[t.ib] += -t.spq * ai - t.sq * bi + t.sqq * aj + t.sq * bj;
      y[t.ib + 1] -= e1;
    }
    for (size_t u = 0; u < (size_t)nviews * ncell; ++u) {
      y[2 * u] += wid[u] * s2 * (diag_only ? 1.0 : x[2 * u]);
      y[2 * u + 1] += wid[u] * (diag_only ? 1.0 : x[2 * u + 1]);
    }
    const size_t stride[3] = {1, (size_t)cg[0], (size_t)cg[0] * cg[1]};
    for (int v = 0; v < nviews; ++v)
      for (int z = 0; z < cg[2]; ++z)
        for (int yy = 0; yy < cg[1]; ++yy)
          for (int xx = 0; xx < cg[0]; ++xx) {
            const int ci[3] = {xx, yy, z};
            const size_t u =
                (size_t)v * ncell + ((size_t)z * cg[1] + yy) * cg[0] + xx;
            for (int d = 0; d < 3; ++d) {
              if (ci[d] + 1 >= cg[d]) continue;
              const size_t w = u + stride[d];
              if (diag_only) {
                y[2 * u] += ksm * s2;
                y[2 * w] += ksm * s2;
                y[2 * u + 1] += ksm;
                y[2 * w + 1] += ksm;
                continue;
              }
              const double da = ksm * s2 * (x[2 * u] - x[2 * w]);
              const double db = ksm * (x[2 * u + 1] - x[2 * w + 1]);
              y[2 * u] += da;
              y[2 * w] -= da;
              y[2 * u + 1] += db;
              y[2 * w + 1] -= db;
            }
          }
  }
};

}  // namespace bsint

extern "C" int bs_intensity_solve(int32_t nviews, const int32_t cg[3],
                                  const int32_t *pair_views,
                                  const size_t *pair_offsets, size_t npairs,
                                  const bs_intensity_match *matches,
                                  const bs_intensity_solve_params *prm,
                                  double *coeff_out, int32_t *iterations_out,
                                  double *rel_residual_out) {
  if (nviews < 1 || !cg || !prm || !coeff_out || prm->max_iterations < 1 ||
      (npairs > 0 && (!pair_views || !pair_offsets)))
    return BS_EINVAL;
  for (int d = 0; d < 3; ++d)
    if (cg[d] < 1) return BS_EINVAL;
  bsint::system S;
  S.nviews = nviews;
  for (int d = 0; d < 3; ++d) S.cg[d] = cg[d];
  S.ncell = (size_t)cg[0] * cg[1] * cg[2];
  const size_t nu = (size_t)nviews * S.ncell, N = 2 * nu;
  std::vector<double> W(nu, 0.0);
  double sum_n = 0.0, sum_sq = 0.0;
  for (size_t k = 0; k < npairs; ++k) {
    const int32_t va = pair_views[2 * k], vb = pair_views[2 * k + 1];
    if (va < 0 || va >= nviews || vb < 0 || vb >= nviews || va == vb ||
        pair_offsets[k + 1] < pair_offsets[k])
      return BS_EINVAL;
    if (pair_offsets[k + 1] > pair_offsets[k] && !matches) return BS_EINVAL;
    for (size_t i = pair_offsets[k]; i < pair_offsets[k + 1]; ++i) {
      const bs_intensity_match &m = matches[i];
      if (m.cell_a >= S.ncell || m.cell_b >= S.ncell) return BS_EINVAL;
      if (m.n_inl == 0) continue;
      bsint::term t;
      const size_t ua = (size_t)va * S.ncell + (size_t)m.cell_a,
                   ub = (size_t)vb * S.ncell + (size_t)m.cell_b;
      t.ia = 2 * ua;
      t.ib = 2 * ub;
      t.n = (double)m.n_inl;
      t.sp = (double)m.sp / 8.0;
      t.sq = (double)m.sq / 8.0;
      t.spp = (double)m.spp / 64.0;
      t.sqq = (double)m.sqq / 64.0;
      t.spq = (double)m.spq / 64.0;
      S.terms.push_back(t);
      W[ua] += t.n;
      W[ub] += t.n;
      sum_n += t.n;
      sum_sq += t.spp + t.sqq;
    }
  }
  std::vector<double> x(N);
  for (size_t u = 0; u < nu; ++u) {
    x[2 * u] = 1.0;
    x[2 * u + 1] = 0.0;
  }
  int iters = 0;
  double relres = 0.0;
  if (!S.terms.empty()) {
    const double wm = sum_n / (double)S.terms.size();
    S.s2 = sum_sq / (2.0 * sum_n);
    if (!(S.s2 > 0.0)) S.s2 = 1.0;
    S.ksm = prm->lambda_smooth * wm;
    S.wid.resize(nu);
    for (size_t u = 0; u < nu; ++u)
      S.wid[u] = prm->lambda_identity * (W[u] + wm);
    std::vector<double> rhs(N, 0.0), diag(N), r(N), z(N), p(N), hp(N);
    for (size_t u = 0; u < nu; ++u) rhs[2 * u] = S.wid[u] * S.s2;
    S.apply(nullptr, diag.data(), true);
    for (size_t i = 0; i < N; ++i)
      if (!(diag[i] > 0.0)) diag[i] = 1.0; /* both lambdas zero, no data */
    S.apply(x.data(), hp.data(), false);
    double rz = 0.0, bnorm = 0.0;
    for (size_t i = 0; i < N; ++i) {
      r[i] = rhs[i] - hp[i];
      z[i] = r[i] / diag[i];
      p[i] = z[i];
      rz += r[i] * z[i];
      bnorm += rhs[i] * rhs[i] / diag[i];
    }
    if (!(bnorm > 0.0)) bnorm = 1.0;
    relres = std::sqrt(rz / bnorm);
    while (relres > 1e-10 && iters < prm->max_iterations) {
      S.apply(p.data(), hp.data(), false);
      double php = 0.0;
      for (size_t i = 0; i < N; ++i) php += p[i] * hp[i];
      if (!(php > 0.0)) break;
      const double alpha = rz / php;
      double rz2 = 0.0;
      for (size_t i = 0; i < N; ++i) {
        x[i] += alpha * p[i];
        r[i] -= alpha * hp[i];
        z[i] = r[i] / diag[i];
        rz2 += r[i] * z[i];
      }
      const double beta = rz2 / rz;
      for (size_t i = 0; i < N; ++i) p[i] = z[i] + beta * p[i];
      rz = rz2;
      relres = std::sqrt(rz / bnorm);
      ++iters;
    }
  }
  /* per view: a-plane, then b-plane */
  for (int v = 0; v < nviews; ++v)
    for (size_t cidx = 0; cidx < S.ncell; ++cidx) {
      const size_t u = (size_t)v * S.ncell + cidx;
      coeff_out[(size_t)v * 2 * S.ncell + cidx] = x[2 * u];
      coeff_out[(size_t)v * 2 * S.ncell + S.ncell + cidx] = x[2 * u + 1];
    }
  if (iterations_out) *iterations_out = iters;
  if (rel_residual_out) *rel_residual_out = relres;
  return BS_OK;
}

#endif /* BS_INTENSITY_SOLVE_H */
