/* x-pass FFT schedule: radix-4 (h = 256) and radix-8 (h = 512) Stockham
 * over one wave's registers and a wave-private LDS buffer — the index,
 * twiddle and butterfly arithmetic shared by k_fft_x_fwd_r4 /
 * k_fft_x_inv_r4 (bigstitch.hip) and the host sanitizer program
 * (tests/xfft_r4_host.cpp), which emulates a wave with a loop over 64
 * lanes and an array for the LDS buffer.
 *
 * h = 64*E complex points, E = 4 or 8, radix R = E. Lane l holds
 * v[r] = z[l + 64 r]. Constant-geometry DIT Stockham (the schedule of
 * fft_stockham, fixed to one radix): for sub-size L = 1, R, R^2, ... < h,
 * with j = l % L and b = l / L,
 *   t_r   = v[r] * w_{LR}^{j r}            (L = 1: no twiddles)
 *   out_s = DFT_R(t)_s
 *   out_s belongs at index R L b + j + L s.
 * After every stage but the last the wave writes its R outputs to the
 * buffer at xf_swz(index) and reads xf_swz(l + 64 r) back. In the last
 * stage L = 64, so b = 0, j = l and the destination l + 64 s is the
 * register order: natural order in, natural order out, no bit reversal.
 *
 * Twiddles come from the half-circle table of the REAL length n = 2h:
 * twn[k] = e^{-2 pi i k / n}, k < h. w_{LR}^{j r} = e^{-2 pi i q / n} with
 * q = j r n / (L R) < n; q >= h is the sign flip of twn[q - h]. They depend
 * on the lane and the stage only, so a kernel reads them once per wave.
 *
 * The complex type C is any struct with float members x, y. */
#ifndef BS_XFFT_R4_H
#define BS_XFFT_R4_H

#if defined(__HIPCC__)
#define BS_XF_FN __host__ __device__ __forceinline__
#define BS_XF_UNROLL _Pragma("unroll")
#else
#define BS_XF_FN static inline
#define BS_XF_UNROLL
#endif

/* E -> number of stages: 4^4 = 256, 8^3 = 512 */
template <int E>
struct xf_geom {
  static_assert(E == 4 || E == 8, "radix-4 at h=256, radix-8 at h=512");
  static constexpr int R = E;
  static constexpr int H = 64 * E;
  static constexpr int LOG2R = E == 4 ? 2 : 3;
  static constexpr int NS = E == 4 ? 4 : 3;
};

/* sub-size of stage si: R^si */
template <int E>
BS_XF_FN int xf_L(int si) { return 1 << (xf_geom<E>::LOG2R * si); }

/* XOR swizzle of an exchange-buffer element index (a bijection of
 * [0, h)): with it every write of every stage hits 16 distinct 8-byte
 * bank pairs per 16-lane group and the strided read 32 distinct ones per
 * 32-lane half (the table tests/xfft_r4_host.cpp prints). */
template <int E>
BS_XF_FN int xf_swz(int m) { return m ^ ((m >> xf_geom<E>::LOG2R) & 15); }

/* where output s of lane l goes after the stage of sub-size L */
template <int E>
BS_XF_FN int xf_dst(int L, int lane, int s) {
  return xf_geom<E>::R * L * (lane / L) + (lane % L) + L * s;
}

/* w_{LR}^{(lane % L) r} as an index q into the full circle of n = 2h */
template <int E>
BS_XF_FN int xf_tw_q(int L, int lane, int r) {
  return (lane % L) * r * ((2 * xf_geom<E>::H) / (L * xf_geom<E>::R));
}

/* e^{-dir 2 pi i q / n} from the half-circle table, q < n = 2h */
template <int E, class C>
BS_XF_FN C xf_tw(const C *twn, int q, int dir) {
  constexpr int h = xf_geom<E>::H;
  C w = twn[q >= h ? q - h : q];
  if (q >= h) { w.x = -w.x; w.y = -w.y; }
  if (dir < 0) w.y = -w.y;
  return w;
}

template <class C>
BS_XF_FN C xf_cmul(C a, C b) {
  return {a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x};
}

/* in-place 4-point DFT, kernel e^{-dir 2 pi i r s / 4} */
template <int DIR, class C>
BS_XF_FN void xf_dft4(C &t0, C &t1, C &t2, C &t3) {
  const C a0 = {t0.x + t2.x, t0.y + t2.y}, a1 = {t0.x - t2.x, t0.y - t2.y};
  const C a2 = {t1.x + t3.x, t1.y + t3.y}, a3 = {t1.x - t3.x, t1.y - t3.y};
  t0 = {a0.x + a2.x, a0.y + a2.y};
  t2 = {a0.x - a2.x, a0.y - a2.y};
  /* -i*a3 forward, +i*a3 inverse */
  const C ia = DIR > 0 ? C{a3.y, -a3.x} : C{-a3.y, a3.x};
  t1 = {a1.x + ia.x, a1.y + ia.y};
  t3 = {a1.x - ia.x, a1.y - ia.y};
}

/* in-place R-point DFT of a lane's registers */
template <int DIR, class C>
BS_XF_FN void xf_bfly(C (&t)[4]) {
  xf_dft4<DIR>(t[0], t[1], t[2], t[3]);
}

template <int DIR, class C>
BS_XF_FN void xf_bfly(C (&t)[8]) {
  /* evens and odds, then out_k = E_k + w8^k O_k, out_{k+4} = E_k - .. */
  xf_dft4<DIR>(t[0], t[2], t[4], t[6]);
  xf_dft4<DIR>(t[1], t[3], t[5], t[7]);
  constexpr float c = 0.70710678118654752440f;
  const C o0 = t[1];
  /* w8 = (1 - dir*i)/sqrt2, w8^2 = -dir*i, w8^3 = (-1 - dir*i)/sqrt2 */
  const C o1 = DIR > 0 ? C{c * (t[3].x + t[3].y), c * (t[3].y - t[3].x)}
                       : C{c * (t[3].x - t[3].y), c * (t[3].y + t[3].x)};
  const C o2 = DIR > 0 ? C{t[5].y, -t[5].x} : C{-t[5].y, t[5].x};
  const C o3 = DIR > 0 ? C{c * (t[7].y - t[7].x), -c * (t[7].x + t[7].y)}
                       : C{-c * (t[7].x + t[7].y), c * (t[7].x - t[7].y)};
  const C e0 = t[0], e1 = t[2], e2 = t[4], e3 = t[6];
  t[0] = {e0.x + o0.x, e0.y + o0.y};
  t[4] = {e0.x - o0.x, e0.y - o0.y};
  t[1] = {e1.x + o1.x, e1.y + o1.y};
  t[5] = {e1.x - o1.x, e1.y - o1.y};
  t[2] = {e2.x + o2.x, e2.y + o2.y};
  t[6] = {e2.x - o2.x, e2.y - o2.y};
  t[3] = {e3.x + o3.x, e3.y + o3.y};
  t[7] = {e3.x - o3.x, e3.y - o3.y};
}

/* the twiddles of one lane: tw[si - 1][r - 1] for stages si >= 1, r >= 1 */
template <int E, class C>
struct xf_twset {
  C w[xf_geom<E>::NS - 1][E - 1];
};

template <int E, class C>
BS_XF_FN void xf_load_tw(xf_twset<E, C> &t, const C *twn, int lane,
                         int dir) {
  BS_XF_UNROLL
  for (int si = 1; si < xf_geom<E>::NS; ++si)
    BS_XF_UNROLL
    for (int r = 1; r < E; ++r)
      t.w[si - 1][r - 1] =
          xf_tw<E>(twn, xf_tw_q<E>(xf_L<E>(si), lane, r), dir);
}

/* one lane's work in stage si: twiddle, butterfly. The exchange between
 * stages is the caller's (LDS on the GPU, an array on the host). */
template <int E, int DIR, class C>
BS_XF_FN void xf_stage(C (&v)[E], const xf_twset<E, C> &t, int si) {
  if (si > 0)
    BS_XF_UNROLL
    for (int r = 1; r < E; ++r) v[r] = xf_cmul(v[r], t.w[si - 1][r - 1]);
  xf_bfly<DIR>(v);
}

/* ---- packed-real ends (the formulas of k_fft_x_fwd / k_fft_x_inv) ---- */

/* forward unpack: Z = FFT_h(x[2j] + i x[2j+1]); for 0 < k < h
 *   X[k] = (Z[k] + conj(Z[h-k]))/2 + w^k * (-i/2) (Z[k] - conj(Z[h-k])),
 * w = twn[k]. k = 0 gives X[0] and X[h] (xf_unpack0). */
template <class C>
BS_XF_FN C xf_unpack(C zk, C zm, C w) {
  const C ze = {0.5f * (zk.x + zm.x), 0.5f * (zk.y - zm.y)};
  const C dd = {zk.x - zm.x, zk.y + zm.y};
  const C zo = {0.5f * dd.y, -0.5f * dd.x};
  const C wzo = xf_cmul(w, zo);
  return {ze.x + wzo.x, ze.y + wzo.y};
}

template <class C>
BS_XF_FN void xf_unpack0(C z0, C &x0, C &xh) {
  x0 = {z0.x + z0.y, 0.0f};
  xh = {z0.x - z0.y, 0.0f};
}

/* inverse pre-process: Z2[k] = A + i conj(w^k) B, A = X[k] + conj(X[h-k]),
 * B = X[k] - conj(X[h-k]); the inverse h-point FFT of Z2 is
 * (x[2j], x[2j+1]) of the UNNORMALISED length-n inverse. */
template <class C>
BS_XF_FN C xf_prep(C xk, C xm, C w) {
  const C A = {xk.x + xm.x, xk.y - xm.y};
  const C B = {xk.x - xm.x, xk.y + xm.y};
  const C wc = {w.x, -w.y};
  const C wb = xf_cmul(wc, B);
  return {A.x - wb.y, A.y + wb.x};
}

/* index of the mirror partner Z[h - k] (k = 0 pairs with itself) */
template <int E>
BS_XF_FN int xf_mirror(int k) { return (xf_geom<E>::H - k) & (xf_geom<E>::H - 1); }

#endif /* BS_XFFT_R4_H */
