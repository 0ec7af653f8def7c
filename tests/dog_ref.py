"""float64 numpy restatement of Difference-of-Gaussian interest point
detection — the arithmetic contract of bs_detect_dog (include/bigstitch.h).

Not a test. mvrecon's DoGImgLib2 is not part of the reference tree, so
this file restates the published method (Lowe 2004; Preibisch 2010) and
the call site SparkInterestPointDetection.java:552-601; every restated
constant carries the same [PIN-*] tag as the HIP code.

Volumes are (nz, ny, nx) arrays; locations are returned in xyz order.
"""

from __future__ import annotations

import numpy as np

K = 2.0 ** 0.25  # [PIN-SIGMA]
IMAGE_SIGMA = 0.5


def box_mean(vol, ds):
    """[PIN-DS2X] float box mean over ds=(dx,dy,dz) cells, dims floor(n/f)."""
    dx, dy, dz = ds
    nz, ny, nx = (vol.shape[0] // dz, vol.shape[1] // dy, vol.shape[2] // dx)
    v = vol[:nz * dz, :ny * dy, :nx * dx].astype(np.float64)
    return v.reshape(nz, dz, ny, dy, nx, dx).mean(axis=(1, 3, 5))


def sigmas(sigma):
    """[PIN-SIGMA] -> (s1, s2, weight)."""
    s1 = np.sqrt(sigma * sigma - IMAGE_SIGMA ** 2)
    s2 = np.sqrt((sigma * K) ** 2 - IMAGE_SIGMA ** 2)
    return s1, s2, 1.0 / (K - 1.0)


def taps(s):
    """[PIN-GAUSS] unit-sum taps over |x| <= h-1."""
    h = max(2, int(3.0 * s + 0.5) + 1)
    x = np.arange(-(h - 1), h, dtype=np.float64)
    w = np.exp(-x * x / (2.0 * s * s))
    return w / w.sum()


def _blur_axis(a, w, axis):
    r = len(w) // 2
    pad = [(0, 0)] * a.ndim
    pad[axis] = (r, r)
    p = np.pad(a, pad, mode="symmetric")  # mirror, edge sample repeated
    out = np.zeros_like(a)
    n = a.shape[axis]
    for k, wk in enumerate(w):
        sl = [slice(None)] * a.ndim
        sl[axis] = slice(k, k + n)
        out += wk * p[tuple(sl)]
    return out


def blur(a, s):
    w = taps(s)
    for axis in (2, 1, 0):  # x, y, z
        a = _blur_axis(a, w, axis)
    return a


def detection_input(vol, ds):
    """Raw (un-normalised) detection-scale input as float64."""
    if tuple(ds) == (1, 1, 1):
        return vol.astype(np.float64)
    return box_mean(vol, ds)


def dog_volume(vol, sigma, lo, hi, ds=(1, 1, 1)):
    """[PIN-DOG-SIGN] D = (G_s1(f) - G_s2(f)) * w, float64 (nz,ny,nx)."""
    f = (detection_input(vol, ds) - lo) / (hi - lo)
    s1, s2, w = sigmas(sigma)
    return (blur(f, s1) - blur(f, s2)) * w


def _neighbour_extremes(D):
    """(max, min) over the 26 neighbours for every interior voxel."""
    c = D[1:-1, 1:-1, 1:-1]
    nmax = np.full(c.shape, -np.inf)
    nmin = np.full(c.shape, np.inf)
    nz, ny, nx = D.shape
    for dz in (0, 1, 2):
        for dy in (0, 1, 2):
            for dx in (0, 1, 2):
                if dz == dy == dx == 1:
                    continue
                v = D[dz:dz + nz - 2, dy:dy + ny - 2, dx:dx + nx - 2]
                np.maximum(nmax, v, out=nmax)
                np.minimum(nmin, v, out=nmin)
    return nmax, nmin


def classify(D, thr, eps):
    """[PIN-EXTREMA] with a tolerance band. Returns
    {+1: (sure, possible), -1: (sure, possible)} of boolean (nz,ny,nx)
    arrays: sure beats every neighbour and the gate |D| >= thr by more than
    eps, possible comes within eps of doing so."""
    nmax, nmin = _neighbour_extremes(D)
    c = D[1:-1, 1:-1, 1:-1]
    gate = np.abs(c) - thr
    out = {}
    for kind, margin in ((1, c - nmax), (-1, nmin - c)):
        sure = np.zeros(D.shape, bool)
        poss = np.zeros(D.shape, bool)
        sure[1:-1, 1:-1, 1:-1] = (margin > eps) & (gate > eps)
        poss[1:-1, 1:-1, 1:-1] = (margin > -eps) & (gate > -eps)
        out[kind] = (sure, poss)
    return out


def _fit(D, p0):
    """[PIN-SUBPIX] at integer xyz p0 -> (p, offset, value, converged)."""
    nz, ny, nx = D.shape
    dims = (nx, ny, nz)
    p = list(p0)

    def at(q, d=None, s=0, e=None, t=0):
        q = list(q)
        if d is not None:
            q[d] += s
        if e is not None:
            q[e] += t
        return D[q[2], q[1], q[0]]

    for m in range(11):
        if any(p[d] < 1 or p[d] > dims[d] - 2 for d in range(3)):
            break
        v = at(p)
        g = np.zeros(3)
        H = np.zeros((3, 3))
        for d in range(3):
            a, b = at(p, d, 1), at(p, d, -1)
            g[d] = 0.5 * (a - b)
            H[d, d] = a - 2.0 * v + b
        for d in range(3):
            for e in range(d + 1, 3):
                H[d, e] = H[e, d] = 0.25 * (
                    at(p, d, 1, e, 1) - at(p, d, 1, e, -1)
                    - at(p, d, -1, e, 1) + at(p, d, -1, e, -1))
        det = np.linalg.det(H)
        if abs(det) < 1e-30:
            break
        o = -np.linalg.solve(H, g)
        lim = 0.5 + 0.01 * m
        if np.all(np.abs(o) <= lim):
            return p, o, v + 0.5 * float(g @ o), 1
        if m == 10:
            break
        for d in range(3):
            if abs(o[d]) > lim:
                p[d] += 1 if o[d] > 0 else -1
    return list(p0), np.zeros(3), at(p0), 0


def _trilinear_clamped(raw, loc):
    nz, ny, nx = raw.shape
    dims = (nx, ny, nz)
    i0, i1, f = [], [], []
    for d in range(3):
        fl = int(np.floor(loc[d]))
        f.append(loc[d] - fl)
        i0.append(min(max(fl, 0), dims[d] - 1))
        i1.append(min(max(fl + 1, 0), dims[d] - 1))
    acc = 0.0
    for c in range(8):
        ix = i1[0] if c & 1 else i0[0]
        iy = i1[1] if c & 2 else i0[1]
        iz = i1[2] if c & 4 else i0[2]
        wx = f[0] if c & 1 else 1.0 - f[0]
        wy = f[1] if c & 2 else 1.0 - f[1]
        wz = f[2] if c & 4 else 1.0 - f[2]
        acc += wx * wy * wz * raw[iz, iy, ix]
    return acc


def detect(vol, sigma, threshold, lo, hi, find_min=False, find_max=True,
           localization="quadratic", ds=(1, 1, 1), D=None):
    """Same fields and order as bs_detect_dog: dict of loc (N,3) xyz in
    view pixels, value, intensity, kind, converged (+ 'voxel', the final
    integer detection-scale voxel, for diagnostics)."""
    quad = localization.lower() == "quadratic"
    raw = detection_input(vol, ds)
    if D is None:
        D = dog_volume(vol, sigma, lo, hi, ds)
    nz, ny, nx = D.shape
    gate = threshold / 3.0 if quad else threshold  # [PIN-THRESH]
    nmax, nmin = _neighbour_extremes(D)
    c = D[1:-1, 1:-1, 1:-1]
    rows = []
    for kind, sel in ((1, c > nmax), (-1, c < nmin)):
        if (kind == 1 and not find_max) or (kind == -1 and not find_min):
            continue
        zz, yy, xx = np.nonzero(sel & (np.abs(c) >= gate))
        for z, y, x in zip(zz + 1, yy + 1, xx + 1):
            p0 = [int(x), int(y), int(z)]
            if quad:
                p, o, val, conv = _fit(D, p0)
            else:
                p, o, val, conv = p0, np.zeros(3), D[z, y, x], 1
            if abs(val) < threshold:
                continue
            loc = np.array(p, np.float64) + o
            fin = p[0] + nx * (p[1] + ny * p[2])
            start = p0[0] + nx * (p0[1] + ny * p0[2])
            rows.append((fin, -kind, start, loc, val,
                         _trilinear_clamped(raw, loc), kind, conv, p))
    rows.sort(key=lambda r: r[:3])
    n = len(rows)
    f = np.array(ds, np.float64)
    loc = np.array([r[3] for r in rows], np.float64).reshape(n, 3)
    return dict(
        loc=loc * f + (f - 1.0) / 2.0,  # [PIN-MIP]
        value=np.array([r[4] for r in rows], np.float64),
        intensity=np.array([r[5] for r in rows], np.float64),
        kind=np.array([r[6] for r in rows], np.int32),
        converged=np.array([r[7] for r in rows], np.int32),
        voxel=np.array([r[8] for r in rows], np.int64).reshape(n, 3),
    )


# ------------------------------------------------------------ generators

def _centres(rng, shape, n, border, min_dist):
    """n sub-pixel centres (z,y,x), >= border from every face and
    >= min_dist apart (rejection sampling; raises if they do not fit)."""
    lo = np.full(3, float(border))
    hi = np.array(shape, np.float64) - 1.0 - border
    pts = []
    for _ in range(20000):
        if len(pts) == n:
            break
        c = lo + rng.random(3) * (hi - lo)
        if all(np.linalg.norm(c - q) >= min_dist for q in pts):
            pts.append(c)
    if len(pts) != n:
        raise ValueError(f"cannot place {n} centres in {shape}")
    return np.array(pts)


def _blobs(shape, centres, sig, amp):
    zz, yy, xx = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape],
                             indexing="ij")
    out = np.zeros(shape)
    for (cz, cy, cx), s, a in zip(centres, sig, amp):
        out += a * np.exp(-((zz - cz) ** 2 + (yy - cy) ** 2 + (xx - cx) ** 2)
                          / (2.0 * s * s))
    return out


def make_bright(shape, n, seed, border=2.0):
    """Background 100 +- 10 uniform integer noise plus n Gaussian blobs of
    sigma 1.5-2.2, amplitude 300-2000, centres >= 7 px apart.
    Returns (uint16 volume, centres (n,3) zyx)."""
    rng = np.random.default_rng(seed)
    cen = _centres(rng, shape, n, border, 7.0)
    sig = rng.uniform(1.5, 2.2, n)
    amp = rng.uniform(300.0, 2000.0, n)
    bg = rng.integers(90, 111, size=shape).astype(np.float64)
    return np.rint(bg + _blobs(shape, cen, sig, amp)).astype(np.uint16), cen


def make_dark(shape, n, seed, border=2.0):
    v, cen = make_bright(shape, n, seed, border)
    return (4000 - v.astype(np.int64)).astype(np.uint16), cen


def make_mixed(shape, n, seed, border=2.0):
    """Background 2000 +- 10, alternating +/- blobs of amplitude 800-1200,
    centres >= 9 px apart. Returns (volume, centres, signs)."""
    rng = np.random.default_rng(seed)
    cen = _centres(rng, shape, n, border, 9.0)
    sig = rng.uniform(1.5, 2.2, n)
    sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    amp = rng.uniform(800.0, 1200.0, n) * sign
    bg = rng.integers(1990, 2011, size=shape).astype(np.float64)
    vol = np.rint(bg + _blobs(shape, cen, sig, amp)).astype(np.uint16)
    return vol, cen, sign.astype(np.int32)
