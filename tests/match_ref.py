"""float64 numpy restatement of interest-point descriptor matching
(bs_match_descriptors; the reference's PRECISE_TRANSLATION matcher,
SparkGeometricDescriptorMatching.java:594-604 -> mvrecon RGLDMPairwise).
Not a test. mvrecon's matcher is not part of the reference tree, so this
file IS the contract; every restated constant carries a [PIN-*] tag.

  [PIN-F32PTS]  both sets arrive as float64 world coordinates; the per-axis
                minimum over the union is subtracted in double and the result
                rounded to float32. Reference and device start from those
                float32 values; the reference then computes in float64.
  [PIN-KNN]     k = n + r nearest neighbours within the point's own set,
                itself excluded, ascending squared distance, ties to the
                lower index. Fewer than k + 1 points: no descriptors.
  [PIN-RGLDM]   one descriptor per n-subset of the k neighbours, subsets in
                lexicographic order of neighbour rank; the descriptor is the
                3n relative vectors q_j - p; index = point * C + subset.
  [PIN-DESCDIST] mean over the n members of the squared Euclidean distance
                between corresponding relative vectors.
  [PIN-RATIO]   best / second = two smallest distances over all (eligible) B
                descriptors, ties to the lower B index; with a search radius
                a B descriptor is eligible when the float32 squared distance
                of the base points, fl(fl(fl(dx*dx) + fl(dy*dy)) + fl(dz*dz)),
                is <= (float32)(radius * radius). Kept when
                best * ratio <= second and best < difference_threshold; fewer
                than two eligible descriptors: not kept.
  [PIN-AMBIG]   kept (a, b) base pairs made unique, then every pair whose a
                occurs with more than one b or whose b with more than one a
                is dropped; sorted by (a, b).
  [PIN-RANSAC]  host side (csrc/bs_ransac.h), tested against planted
                transforms in tests/test_match_ref_cpu.py: xorshift64* seeded
                with 0x9E3779B97F4A7C15, `iterations` minimal sets, inliers
                error <= max_epsilon, refit until the set stops growing,
                largest consensus wins (ties: earlier iteration), accepted
                when inliers >= min_num_inliers and inliers / candidates >=
                min_inlier_ratio. [PIN-INTERP]: (1 - lambda) M_t + lambda M_r.
"""

from __future__ import annotations

import itertools

import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)


def to_f32(pa, pb):
    """[PIN-F32PTS] -> (A float32 (na,3), B float32 (nb,3))."""
    pa = np.asarray(pa, np.float64).reshape(-1, 3)
    pb = np.asarray(pb, np.float64).reshape(-1, 3)
    both = np.concatenate([pa, pb])
    mn = both.min(axis=0) if len(both) else np.zeros(3)
    return (pa - mn).astype(np.float32), (pb - mn).astype(np.float32)


def knn(p32, k):
    """[PIN-KNN] on float32 points, computed in float64.
    Returns idx int32 (N, k), d2 float64 (N, k) and gap float64 (N,): the
    smallest relative gap between consecutive distances among ranks 0..k
    (rank k is the first neighbour left out). N <= k: idx -1, d2 inf."""
    p = np.asarray(p32, np.float64)
    n = len(p)
    if n <= k:
        return (np.full((n, k), -1, np.int32), np.full((n, k), np.inf),
                np.full(n, np.inf))
    idx = np.empty((n, k), np.int32)
    d2 = np.empty((n, k))
    gap = np.full(n, np.inf)
    for s in range(0, n, 512):
        q = p[s:s + 512]
        d = ((q[:, None, :] - p[None, :, :]) ** 2).sum(-1)
        d[np.arange(len(q)), np.arange(s, s + len(q))] = np.inf
        order = np.argsort(d, axis=1, kind="stable")[:, :k + 1]
        ds = np.take_along_axis(d, order, axis=1)
        idx[s:s + 512] = order[:, :k]
        d2[s:s + 512] = ds[:, :k]
        hi = ds[:, 1:]
        ok = np.isfinite(hi) & (hi > 0)
        g = np.where(ok, (hi - ds[:, :-1]) / np.where(ok, hi, 1.0), np.inf)
        # equal distances (hi == lo, both finite) are a zero gap
        g = np.where(np.isfinite(hi) & (hi == ds[:, :-1]), 0.0, g)
        gap[s:s + 512] = g.min(axis=1)
    return idx, d2, gap


def subsets(n, r):
    """[PIN-RGLDM] n-subsets of ranks 0..n+r-1, lexicographic."""
    return np.array(list(itertools.combinations(range(n + r), n)), np.int64)


def descriptors(p32, n, r):
    """(N*C, n, 3) float64 relative vectors; empty when N <= n + r."""
    p = np.asarray(p32, np.float64)
    idx, _, _ = knn(p32, n + r)
    comb = subsets(n, r)
    if len(p) <= n + r:
        return np.zeros((0, n, 3))
    nb = idx[:, comb]                       # (N, C, n)
    rel = p[nb] - p[:, None, None, :]       # (N, C, n, 3)
    return rel.reshape(-1, n, 3)


def _f32_base_d2(a32, b32):
    """[PIN-RATIO] eligibility distance, float32 with every step rounded."""
    a = np.asarray(a32, np.float32)
    b = np.asarray(b32, np.float32)
    dx = a[:, None, 0] - b[None, :, 0]
    dy = a[:, None, 1] - b[None, :, 1]
    dz = a[:, None, 2] - b[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz    # float32 throughout


def match_raw_multi(a32, b32, n=3, r=1, radii=(None,)):
    """match_raw for several search radii on one distance matrix."""
    da = descriptors(a32, n, r)
    db = descriptors(b32, n, r)
    C = len(subsets(n, r))
    na, nb = len(da), len(db)
    out = [dict(best=np.full(na, np.inf), second=np.full(na, np.inf),
                best_b=np.full(na, -1, np.int32),
                second_b=np.full(na, -1, np.int32), C=C) for _ in radii]
    if na == 0 or nb == 0:
        return out
    fa = da.reshape(na, -1)
    fb = db.reshape(nb, -1)
    nb2 = (fb * fb).sum(1)
    rows = max(1, (1 << 23) // nb)
    rows = max(C, rows // C * C)            # whole base points per chunk
    for s in range(0, na, rows):
        q = fa[s:s + rows]
        ar = np.arange(len(q))
        d0 = (q * q).sum(1)[:, None] + nb2[None, :] - 2.0 * (q @ fb.T)
        for res, radius in zip(out, radii):
            d = d0
            if radius is not None:
                r2 = np.float32(float(radius) * float(radius))
                pa = np.asarray(a32)[s // C:(s + len(q)) // C]
                far = _f32_base_d2(pa, b32) > r2          # (pts A, pts B)
                d = d0.reshape(len(pa), C, len(far[0]), C).copy()
                d[np.broadcast_to(far[:, None, :, None], d.shape)] = np.inf
                d = d.reshape(len(q), nb)
            i1 = np.argmin(d, axis=1)       # first occurrence = lower index
            v1 = d[ar, i1].copy()
            d[ar, i1] = np.inf
            i2 = np.argmin(d, axis=1)
            v2 = d[ar, i2]
            d[ar, i1] = v1                  # d0 is reused by the next radius
            h1 = np.isfinite(v1)
            h2 = np.isfinite(v2)
            qq = q.reshape(len(q), n, 3)
            e1 = ((qq - db[i1]) ** 2).sum(-1).mean(-1)
            e2 = ((qq - db[i2]) ** 2).sum(-1).mean(-1)
            res["best"][s:s + rows] = np.where(h1, e1, np.inf)
            res["second"][s:s + rows] = np.where(h2, e2, np.inf)
            res["best_b"][s:s + rows] = np.where(h1, i1, -1)
            res["second_b"][s:s + rows] = np.where(h2, i2, -1)
    return out


def match_raw(a32, b32, n=3, r=1, search_radius=None):
    """Per A descriptor: best, second (float64, inf where missing), best_b
    and second_b (int32 B descriptor index, -1 where missing).

    The two smallest are selected on |a|^2 + |b|^2 - 2ab (exact for the
    integer lattice, 1e-11 absolute otherwise) and their distances are then
    recomputed directly as [PIN-DESCDIST] states them."""
    return match_raw_multi(a32, b32, n, r, (search_radius,))[0]


def candidates(raw, ratio=3.0, difference_threshold=FLT_MAX):
    """[PIN-RATIO] test + [PIN-AMBIG] on match_raw's result -> (M, 2) int32
    array of (a, b) base-point pairs sorted by (a, b)."""
    C = raw["C"]
    best, second = raw["best"], raw["second"]
    with np.errstate(invalid="ignore"):
        keep = (np.isfinite(second) & (raw["best_b"] >= 0)
                & (best * ratio <= second) & (best < difference_threshold))
    a = np.nonzero(keep)[0] // C
    b = raw["best_b"][keep] // C
    pairs = np.unique(np.stack([a, b], 1).astype(np.int64), axis=0)
    if len(pairs) == 0:
        return np.zeros((0, 2), np.int32)
    _, ia, ca = np.unique(pairs[:, 0], return_inverse=True, return_counts=True)
    _, ib, cb = np.unique(pairs[:, 1], return_inverse=True, return_counts=True)
    ok = (ca[ia] == 1) & (cb[ib] == 1)
    return pairs[ok].astype(np.int32)


def ratio_margin(raw, ratio=3.0):
    """|best * ratio / second - 1| per A descriptor (inf where the test is
    not near its boundary by construction: missing second, or both zero)."""
    best, second = raw["best"], raw["second"]
    m = np.full(len(best), np.inf)
    ok = np.isfinite(second) & (second > 0)
    m[ok] = np.abs(best[ok] * ratio / second[ok] - 1.0)
    return m
