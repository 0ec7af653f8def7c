"""numpy restatement of intensity matching and the intensity solve: the
contract of bs_intensity_match_pair / bs_intensity_solve (DESIGN.md
"Intensity matching").
float32 steps are spelled one operation at a time (numpy rounds each float32
operation on its own), integer steps use Python ints, so the device result
can be compared bit for bit.

[PIN-INT-GRID]   spacing s = 1 / renderScale; sample g sits at world point
                 (g + g0) * s, formed in double and rounded once to float32;
                 g0 .. g0 + dims - 1 are the grid points inside the
                 intersection of the two views' transformed bounding boxes
[PIN-INT-RENDER] inverse affine in double, rounded to 12 float32;
                 px = ((i0 wx + i1 wy) + i2 wz) + i3; inside test and
                 trilinear lerp chain of the fusion kernel; quantised sample
                 P = rint(val * 8), units of 1/8 grey level
[PIN-INT-CELL]   cell per axis = min(cg - 1, int(px * float(cg) / float(n)))
                 linear id x fastest; a sample that is not valid in both
                 views carries P = Q = -1 and both cell ids 0
[PIN-INT-RANSAC] draw k of iteration it takes member
                 splitmix64(SEED ^ (cellA<<48 | cellB<<32 | it<<8 | k)) % n;
                 a = (Q2 - Q1) / (P2 - P1) must be > 0, b = Q1 - a P1; inlier
                 iff |(a P + b) - Q| <= float32(8 maxEpsilon); most inliers
                 wins, lowest it on a tie; then least-squares refits from
                 exact integer moments while the inlier count grows, at most
                 10 of them
[PIN-INT-TRUST]  no median-cost trim (maxTrust is not applied)
[PIN-INT-SOLVE]  see solve_dense()
"""

import numpy as np

F = np.float32
SEED = 0x9E3779B97F4A7C15
_M = (1 << 64) - 1

DEFAULTS = dict(render_scale=0.25, coefficients=(8, 8, 8),
                min_num_candidates=1000, min_threshold=1.0,
                max_threshold=None, iterations=1000, max_epsilon=5.1,
                min_inlier_ratio=0.1, min_num_inliers=10)

FIELDS = ("cell_a", "cell_b", "n_cand", "n_inl", "best_it", "n_inl_first",
          "sp", "sq", "spp", "sqq", "spq")


def invert34(m):
    """world -> local, the library's invert34: double, then 12 float32."""
    m = [float(v) for v in np.asarray(m, np.float64).reshape(12)]
    a = [m[0], m[1], m[2], m[4], m[5], m[6], m[8], m[9], m[10]]
    det = (a[0] * (a[4] * a[8] - a[5] * a[7])
           - a[1] * (a[3] * a[8] - a[5] * a[6])
           + a[2] * (a[3] * a[7] - a[4] * a[6]))
    i = 1.0 / det
    ai = [(a[4] * a[8] - a[5] * a[7]) * i, (a[2] * a[7] - a[1] * a[8]) * i,
          (a[1] * a[5] - a[2] * a[4]) * i, (a[5] * a[6] - a[3] * a[8]) * i,
          (a[0] * a[8] - a[2] * a[6]) * i, (a[2] * a[3] - a[0] * a[5]) * i,
          (a[3] * a[7] - a[4] * a[6]) * i, (a[1] * a[6] - a[0] * a[7]) * i,
          (a[0] * a[4] - a[1] * a[3]) * i]
    t = [m[3], m[7], m[11]]
    inv = np.zeros(12, F)
    for r in range(3):
        for k in range(3):
            inv[r * 4 + k] = F(ai[r * 3 + k])
        inv[r * 4 + 3] = F(-(ai[r * 3] * t[0] + ai[r * 3 + 1] * t[1]
                             + ai[r * 3 + 2] * t[2]))
    return inv


def tbbox(m, dims_xyz):
    """Bounding box of [0, dims - 1]^3 under the row-major 3x4 affine m."""
    m = [float(v) for v in np.asarray(m, np.float64).reshape(12)]
    lo, hi = [1e300] * 3, [-1e300] * 3
    for cz in (0, 1):
        for cy in (0, 1):
            for cx in (0, 1):
                p = [float(dims_xyz[0] - 1) if cx else 0.0,
                     float(dims_xyz[1] - 1) if cy else 0.0,
                     float(dims_xyz[2] - 1) if cz else 0.0]
                for r in range(3):
                    w = (m[r * 4] * p[0] + m[r * 4 + 1] * p[1]
                         + m[r * 4 + 2] * p[2] + m[r * 4 + 3])
                    lo[r] = min(lo[r], w)
                    hi[r] = max(hi[r], w)
    return lo, hi


def grid(aff_a, dims_a, aff_b, dims_b, render_scale):
    """[PIN-INT-GRID]: (g0, dims) as xyz int tuples; dims all zero when the
    boxes do not intersect."""
    s = 1.0 / float(render_scale)
    la, ha = tbbox(aff_a, dims_a)
    lb, hb = tbbox(aff_b, dims_b)
    g0, dims = [], []
    for d in range(3):
        lo, hi = max(la[d], lb[d]), min(ha[d], hb[d])
        a, b = int(np.ceil(lo / s)), int(np.floor(hi / s))
        if b < a:
            return (0, 0, 0), (0, 0, 0)
        g0.append(a)
        dims.append(b - a + 1)
    return tuple(g0), tuple(dims)


def _sample(vol, inv, cg, wx, wy, wz):
    """[PIN-INT-RENDER] + [PIN-INT-CELL] for one view. vol (nz, ny, nx)
    uint16; wx, wy, wz float32 arrays of one shape. Returns inside mask,
    quantised int32 sample, cell id, local float32 coordinates."""
    nz, ny, nx = vol.shape
    p = []
    for r in range(3):
        t = inv[r * 4] * wx
        t = t + inv[r * 4 + 1] * wy
        t = t + inv[r * 4 + 2] * wz
        t = t + inv[r * 4 + 3]
        assert t.dtype == F
        p.append(t)
    px, py, pz = p
    inside = ((px >= 0) & (px <= F(nx - 1)) & (py >= 0) & (py <= F(ny - 1))
              & (pz >= 0) & (pz <= F(nz - 1)))
    cx_ = np.where(inside, px, F(0))
    cy_ = np.where(inside, py, F(0))
    cz_ = np.where(inside, pz, F(0))
    x0 = np.floor(cx_).astype(np.int64)
    y0 = np.floor(cy_).astype(np.int64)
    z0 = np.floor(cz_).astype(np.int64)
    x1 = np.minimum(x0 + 1, nx - 1)
    y1 = np.minimum(y0 + 1, ny - 1)
    z1 = np.minimum(z0 + 1, nz - 1)
    fx = cx_ - x0.astype(F)
    fy = cy_ - y0.astype(F)
    fz = cz_ - z0.astype(F)
    v = vol.astype(F)

    def lerp(c0, c1, f):
        d = c1 - c0
        d = d * f
        return c0 + d

    c00 = lerp(v[z0, y0, x0], v[z0, y0, x1], fx)
    c10 = lerp(v[z0, y1, x0], v[z0, y1, x1], fx)
    c01 = lerp(v[z1, y0, x0], v[z1, y0, x1], fx)
    c11 = lerp(v[z1, y1, x0], v[z1, y1, x1], fx)
    c0 = lerp(c00, c10, fy)
    c1 = lerp(c01, c11, fy)
    val = lerp(c0, c1, fz)
    assert val.dtype == F
    q = np.rint(val * F(8)).astype(np.int32)
    cell = []
    for pc, c, n in ((cx_, cg[0], nx), (cy_, cg[1], ny), (cz_, cg[2], nz)):
        t = pc * F(c)
        t = t / F(n)
        cell.append(np.minimum(c - 1, t.astype(np.int32)))
    cid = cell[0] + cg[0] * (cell[1] + cg[1] * cell[2])
    return inside, q, cid.astype(np.int32), (px, py, pz)


def render(vol_a, aff_a, vol_b, aff_b, render_scale=0.25,
           coefficients=(8, 8, 8), min_threshold=1.0, max_threshold=None,
           **_):
    """dict(origin, dims (xyz), P, Q int32, cell_a, cell_b uint16, arrays of
    shape (gz, gy, gx); local_a / local_b float32 view coordinates)."""
    da = vol_a.shape[::-1]
    db = vol_b.shape[::-1]
    g0, dims = grid(aff_a, da, aff_b, db, render_scale)
    shape = dims[::-1]
    out = dict(origin=g0, dims=dims, P=np.zeros(shape, np.int32),
               Q=np.zeros(shape, np.int32),
               cell_a=np.zeros(shape, np.uint16),
               cell_b=np.zeros(shape, np.uint16), local_a=None, local_b=None,
               inside=np.zeros(shape, bool))
    if 0 in dims:
        return out
    s = 1.0 / float(render_scale)
    w = [((np.arange(dims[d], dtype=np.float64) + float(g0[d])) * s)
         .astype(F) for d in range(3)]
    wz, wy, wx = np.meshgrid(w[2], w[1], w[0], indexing="ij")
    ia, P, ca, la = _sample(vol_a, invert34(aff_a), coefficients, wx, wy, wz)
    ib, Q, cb, lb = _sample(vol_b, invert34(aff_b), coefficients, wx, wy, wz)
    lo = 8.0 * float(min_threshold)
    valid = ia & ib & (P >= lo) & (Q >= lo)
    if max_threshold is not None and not np.isnan(max_threshold):
        hi = 8.0 * float(max_threshold)
        valid &= (P <= hi) & (Q <= hi)
    out["inside"] = ia & ib
    out["P"] = np.where(valid, P, -1).astype(np.int32)
    out["Q"] = np.where(valid, Q, -1).astype(np.int32)
    out["cell_a"] = np.where(valid, ca, 0).astype(np.uint16)
    out["cell_b"] = np.where(valid, cb, 0).astype(np.uint16)
    out["local_a"], out["local_b"] = la, lb
    return out


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & _M
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M
    return x ^ (x >> 31)


def moments(P, Q):
    """(n, Sp, Sq, Spp, Sqq, Spq) as Python ints."""
    p = P.astype(np.int64)
    q = Q.astype(np.int64)
    return (int(len(p)), int(p.sum()), int(q.sum()), int((p * p).sum()),
            int((q * q).sum()), int((p * q).sum()))


def line_fit(m):
    """(a, b) in sample units from exact moments, None when den <= 0."""
    n, sp, sq, spp, _, spq = m
    num = n * spq - sp * sq
    den = n * spp - sp * sp
    if den <= 0:
        return None
    a = float(num) / float(den)
    t = a * float(sp)
    return a, (float(sq) - t) / float(n)


def gate(a, b, Pf, Qf, eps):
    """Inlier mask of the float32 line (a, b), one rounded step at a time."""
    with np.errstate(invalid="ignore"):
        t = F(a) * Pf
        t = t + F(b)
        t = t - Qf
        return np.abs(t) <= eps


def ransac(cell_a, cell_b, Pm, Qm, iterations, eps):
    """(best_it, count, a, b) of [PIN-INT-RANSAC] over one bucket."""
    n = len(Pm)
    Pf, Qf = Pm.astype(F), Qm.astype(F)
    a = np.full(iterations, np.nan, F)
    b = np.full(iterations, np.nan, F)
    for it in range(iterations):
        key = (cell_a << 48) | (cell_b << 32) | (it << 8)
        i1 = splitmix64(SEED ^ key) % n
        i2 = splitmix64(SEED ^ (key | 1)) % n
        if Pf[i1] == Pf[i2]:
            continue
        sl = (Qf[i2] - Qf[i1]) / (Pf[i2] - Pf[i1])
        if not sl > 0:
            continue
        a[it] = sl
        t = sl * Pf[i1]
        b[it] = Qf[i1] - t
    counts = np.zeros(iterations, np.int64)
    step = max(1, (1 << 22) // max(n, 1))
    with np.errstate(invalid="ignore"):
        for i0 in range(0, iterations, step):
            t = a[i0:i0 + step, None] * Pf[None, :]
            t = t + b[i0:i0 + step, None]
            t = t - Qf[None, :]
            counts[i0:i0 + step] = (np.abs(t) <= eps).sum(axis=1)
    it = int(np.argmax(counts))  # first maximum = lowest it
    return it, int(counts[it]), a[it], b[it]


def _bucket(a_id, b_id, Pm, Qm, prm, eps):
    """One bucket of match_pair: (kind, record or None)."""
    n_cand = len(Pm)
    if n_cand < max(1, prm["min_num_candidates"]):
        return "dropped_small", None
    it, first, la, lb = ransac(a_id, b_id, Pm, Qm, prm["iterations"], eps)
    Pf, Qf = Pm.astype(F), Qm.astype(F)
    if first == 0:
        return "rejected_fit", None
    mask = gate(la, lb, Pf, Qf, eps)
    cur = moments(Pm[mask], Qm[mask])
    assert cur[0] == first
    for _ in range(10):
        fit = line_fit(cur)
        if fit is None:
            return "rejected_fit", None
        mask = gate(fit[0], fit[1], Pf, Qf, eps)
        new = moments(Pm[mask], Qm[mask])
        if new[0] > cur[0]:
            cur = new
        else:
            break
    fit = line_fit(cur)
    if fit is None:
        return "rejected_fit", None
    if (cur[0] < prm["min_num_inliers"]
            or float(cur[0]) < prm["min_inlier_ratio"] * float(n_cand)):
        return "rejected_ratio", None
    return "records", dict(
        cell_a=a_id, cell_b=b_id, n_cand=n_cand, n_inl=cur[0], best_it=it,
        n_inl_first=first, sp=cur[1], sq=cur[2], spp=cur[3], sqq=cur[4],
        spq=cur[5], a=fit[0], b=fit[1] / 8.0)


def match_pair(vol_a, aff_a, vol_b, aff_b, workers=1, **kw):
    """The contract of bs_intensity_match_pair. Returns dict(render=...,
    buckets={(ca, cb): n_cand} of every non-empty bucket, records=[dict] of
    the accepted ones sorted by (ca, cb), dropped_small, rejected_fit,
    rejected_ratio = lists of (ca, cb)). workers > 1 spreads the buckets over
    that many threads (same result)."""
    prm = dict(DEFAULTS)
    prm.update(kw)
    r = render(vol_a, aff_a, vol_b, aff_b, **prm)
    out = dict(render=r, buckets={}, records=[], dropped_small=[],
               rejected_fit=[], rejected_ratio=[])
    P, Q = r["P"].ravel(), r["Q"].ravel()
    ca, cb = r["cell_a"].ravel().astype(np.int64), r["cell_b"].ravel()
    valid = np.flatnonzero(P >= 0)
    if len(valid) == 0:
        return out
    key = ca[valid] * 65536 + cb[valid]
    order = np.argsort(key, kind="stable")  # members stay in grid order
    skey = key[order]
    starts = np.flatnonzero(np.r_[True, skey[1:] != skey[:-1]])
    ends = np.r_[starts[1:], len(skey)]
    eps = F(8.0 * float(prm["max_epsilon"]))
    jobs = []
    for s0, s1 in zip(starts, ends):
        idx = valid[order[s0:s1]]
        a_id, b_id = int(skey[s0] // 65536), int(skey[s0] % 65536)
        out["buckets"][(a_id, b_id)] = len(idx)
        jobs.append((a_id, b_id, P[idx], Q[idx], prm, eps))
    if workers > 1:
        from concurrent.futures import ThreadPoolExecutor

        with ThreadPoolExecutor(workers) as ex:
            res = list(ex.map(lambda j: _bucket(*j), jobs))
    else:
        res = [_bucket(*j) for j in jobs]
    for j, (kind, rec) in zip(jobs, res):
        out[kind].append(rec if kind == "records" else (j[0], j[1]))
    return out


def records_array(records, dtype):
    """Reference records as the binding's structured array."""
    arr = np.zeros(len(records), dtype)
    for i, r in enumerate(records):
        for k in dtype.names:
            arr[i][k] = r[k]
    return arr


# ------------------------------------------------------------------ solve

def normal_equations(nviews, cg, pairs, lambda_identity=0.01,
                     lambda_smooth=0.1):
    """Dense H, rhs of [PIN-INT-SOLVE] and sigma^2. pairs: list of (view_a,
    view_b, records). Unknown (view v, cell c): a at 2 (v ncell + c), b right
    after it.

    E = sum_buckets sum_inliers (a_i p + b_i - a_j q - b_j)^2
      + l_id sum_c (W_c + Wm) [s2 (a_c - 1)^2 + b_c^2]
      + l_sm Wm sum_{neighbour pairs c, c' of one view}
                    [s2 (a_c - a_c')^2 + (b_c - b_c')^2]
    p, q in grey levels; every unordered 6-neighbour pair counts once."""
    ncell = cg[0] * cg[1] * cg[2]
    N = 2 * nviews * ncell
    H = np.zeros((N, N))
    rhs = np.zeros(N)
    W = np.zeros(nviews * ncell)
    sum_n = sum_sq = 0.0
    nb = 0
    for va, vb, recs in pairs:
        for r in recs:
            n = float(r["n_inl"])
            if n == 0:
                continue
            sp, sq = float(r["sp"]) / 8.0, float(r["sq"]) / 8.0
            spp, sqq, spq = (float(r["spp"]) / 64.0, float(r["sqq"]) / 64.0,
                             float(r["spq"]) / 64.0)
            ua = va * ncell + int(r["cell_a"])
            ub = vb * ncell + int(r["cell_b"])
            ix = [2 * ua, 2 * ua + 1, 2 * ub, 2 * ub + 1]
            # sum over inliers of u u^T, u = (p, 1, -q, -1)
            M = np.array([[spp, sp, -spq, -sp], [sp, n, -sq, -n],
                          [-spq, -sq, sqq, sq], [-sp, -n, sq, n]])
            H[np.ix_(ix, ix)] += M
            W[ua] += n
            W[ub] += n
            sum_n += n
            sum_sq += spp + sqq
            nb += 1
    if nb == 0:
        return None
    wm = sum_n / nb
    s2 = sum_sq / (2.0 * sum_n)
    for u in range(nviews * ncell):
        k = lambda_identity * (W[u] + wm)
        H[2 * u, 2 * u] += k * s2
        rhs[2 * u] += k * s2
        H[2 * u + 1, 2 * u + 1] += k
    ks = lambda_smooth * wm
    stride = (1, cg[0], cg[0] * cg[1])
    for v in range(nviews):
        for z in range(cg[2]):
            for y in range(cg[1]):
                for x in range(cg[0]):
                    u = v * ncell + (z * cg[1] + y) * cg[0] + x
                    for d, c in enumerate((x, y, z)):
                        if c + 1 >= cg[d]:
                            continue
                        w = u + stride[d]
                        for o, k in ((0, ks * s2), (1, ks)):
                            i, j = 2 * u + o, 2 * w + o
                            H[i, i] += k
                            H[j, j] += k
                            H[i, j] -= k
                            H[j, i] -= k
    return H, rhs, s2


def solve_dense(nviews, cg, pairs, **kw):
    """(coeff (nviews, 2, gz, gy, gx), sigma, condition number of the
    Jacobi-scaled normal matrix) by dense least squares."""
    ncell = cg[0] * cg[1] * cg[2]
    ne = normal_equations(nviews, cg, pairs, **kw)
    if ne is None:
        c = np.zeros((nviews, 2, cg[2], cg[1], cg[0]))
        c[:, 0] = 1.0
        return c, 1.0, 1.0
    H, rhs, s2 = ne
    d = 1.0 / np.sqrt(np.diag(H))
    Hs = H * d[:, None] * d[None, :]
    xs = np.linalg.lstsq(Hs, rhs * d, rcond=None)[0]
    x = (xs * d).reshape(nviews, ncell, 2)
    c = np.stack([x[:, :, 0], x[:, :, 1]], axis=1)
    return (c.reshape(nviews, 2, cg[2], cg[1], cg[0]), float(np.sqrt(s2)),
            float(np.linalg.cond(Hs)))


def sample_coefficients(coeff, local, dims_xyz):
    """[PIN-COEFF] of the fusion kernel in float64: (a, b) of one view's
    (2, gz, gy, gx) grid at local coordinates, trilinear over cell centres."""
    cg = coeff.shape[1:][::-1]
    t, i0, i1, f = [], [], [], []
    for d in range(3):
        v = np.asarray(local[d], np.float64) * cg[d] / dims_xyz[d] - 0.5
        v = np.clip(v, 0.0, cg[d] - 1)
        a = v.astype(np.int64)
        i0.append(a)
        i1.append(np.minimum(a + 1, cg[d] - 1))
        f.append(v - a)
    out = []
    for pl in range(2):
        g = coeff[pl]

        def lerp(c0, c1, w):
            return c0 + (c1 - c0) * w

        e00 = lerp(g[i0[2], i0[1], i0[0]], g[i0[2], i0[1], i1[0]], f[0])
        e10 = lerp(g[i0[2], i1[1], i0[0]], g[i0[2], i1[1], i1[0]], f[0])
        e01 = lerp(g[i1[2], i0[1], i0[0]], g[i1[2], i0[1], i1[0]], f[0])
        e11 = lerp(g[i1[2], i1[1], i0[0]], g[i1[2], i1[1], i1[0]], f[0])
        out.append(lerp(lerp(e00, e10, f[1]), lerp(e01, e11, f[1]), f[2]))
    return out[0], out[1]
