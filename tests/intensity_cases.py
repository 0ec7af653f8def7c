"""Seeded inputs for the intensity-matching tests, with their reference
results (tests/intensity_ref.py) computed once per process and shared.

A scene of smooth Gaussian blobs on a base level is sampled analytically at
each view's voxel positions. View A is the scene plus noise; view B is
GAIN * scene + OFFSET plus noise, plus a few bright balls planted in B only:
outliers that RANSAC has to reject. What the cases contain between them
(bucket sizes, a dropped bucket, a ratio-rejected bucket) is asserted on the
reference alone in tests/test_intensity_ref_cpu.py."""

import functools

import numpy as np

from tests import intensity_ref as ir

GAIN, OFFSET = 1.25, 150.0
DIMS = (40, 36, 28)  # x, y, z
ALL = ("shift_int", "shift_half", "sheared", "thresholds", "disjoint",
       "lattice")


def _translate(t):
    m = np.hstack([np.eye(3), np.zeros((3, 1))])
    m[:, 3] = t
    return m


def _world(aff, dims):
    z, y, x = np.meshgrid(np.arange(dims[2]), np.arange(dims[1]),
                          np.arange(dims[0]), indexing="ij")
    p = np.stack([x, y, z], axis=-1).astype(np.float64)
    return p @ aff[:, :3].T + aff[:, 3]


def _scene(w, blobs):
    v = np.full(w.shape[:-1], 300.0)
    for cx, cy, cz, sig, amp in blobs:
        d2 = ((w[..., 0] - cx) ** 2 + (w[..., 1] - cy) ** 2
              + (w[..., 2] - cz) ** 2)
        v += amp * np.exp(-d2 / (2.0 * sig * sig))
    return v


def _views(seed, aff_a, aff_b, balls, noise=1.0, dims=DIMS):
    rng = np.random.default_rng(seed)
    nb = 40
    blobs = np.column_stack([
        rng.uniform(-5, 70, nb), rng.uniform(-5, 45, nb),
        rng.uniform(-5, 35, nb), rng.uniform(5.0, 9.0, nb),
        rng.uniform(150.0, 700.0, nb)])
    wa, wb = _world(aff_a, dims), _world(aff_b, dims)
    a = _scene(wa, blobs) + rng.normal(0.0, noise, wa.shape[:-1])
    b = (GAIN * _scene(wb, blobs) + OFFSET
         + rng.normal(0.0, noise, wb.shape[:-1]))
    for cx, cy, cz, rad, add in balls:  # world centre, radius, grey levels
        d2 = ((wb[..., 0] - cx) ** 2 + (wb[..., 1] - cy) ** 2
              + (wb[..., 2] - cz) ** 2)
        b = np.where(d2 <= rad * rad, b + add, b)
    q = lambda v: np.clip(np.rint(v), 0, 65535).astype(np.uint16)  # noqa: E731
    return q(a), q(b)


def _inputs(name):
    eye = _translate((0, 0, 0))
    if name == "shift_int":
        # cells 2x2x2 at scale 1: y splits the overlap into slabs of 14, 4
        # and 14 rows; the ball fills about a third of one 4-row bucket
        aff_b = _translate((22, 4, 0))
        a, b = _views(11, eye, aff_b, [(31.0, 19.5, 6.5, 5.0, 1200.0),
                                       (27.0, 30.0, 22.0, 2.0, 1200.0)])
        return dict(a=a, b=b, aff_a=eye, aff_b=aff_b, prm=dict(
            render_scale=1.0, coefficients=(2, 2, 2), min_num_candidates=500,
            iterations=1000, min_inlier_ratio=0.8))
    if name == "shift_half":
        aff_b = _translate((17.5, -6.5, 3.5))
        a, b = _views(12, eye, aff_b, [(30.0, 10.0, 12.0, 2.5, 1500.0)])
        return dict(a=a, b=b, aff_a=eye, aff_b=aff_b, prm=dict(
            render_scale=0.5, coefficients=(3, 2, 1), min_num_candidates=60,
            iterations=300))
    if name == "sheared":
        c, s = np.cos(0.06), np.sin(0.06)
        aff_b = np.array([[c, -s, 0.05, 14.0], [s, c, 0.0, 5.0],
                          [0.0, 0.03, 1.0, -2.0]])
        a, b = _views(13, eye, aff_b, [(25.0, 20.0, 10.0, 3.0, 2000.0),
                                       (33.0, 12.0, 20.0, 2.0, 2000.0)])
        return dict(a=a, b=b, aff_a=eye, aff_b=aff_b, prm=dict(
            render_scale=1.0, coefficients=(3, 3, 2), min_num_candidates=100,
            iterations=4096))
    if name == "thresholds":
        aff_b = _translate((12, 2, -3))
        a, b = _views(14, eye, aff_b, [(25.0, 20.0, 10.0, 3.0, 2000.0)])
        return dict(a=a, b=b, aff_a=eye, aff_b=aff_b, prm=dict(
            render_scale=1.0, coefficients=(2, 2, 1), min_num_candidates=100,
            iterations=7, min_threshold=500.0, max_threshold=1300.0))
    if name == "disjoint":
        aff_b = _translate((45, 0, 0))
        a, b = _views(15, eye, aff_b, [])
        return dict(a=a, b=b, aff_a=eye, aff_b=aff_b, prm=dict(
            render_scale=0.5, coefficients=(2, 2, 2), min_num_candidates=10,
            iterations=1000))
    if name == "lattice":
        # exact integers on one line Q = 2 P + 40 (sample units): every
        # non-void hypothesis has all 8 * 8 * 4 = 256 members as inliers
        dims = (12, 8, 4)
        z, y, x = np.meshgrid(np.arange(dims[2]), np.arange(dims[1]),
                              np.arange(dims[0]), indexing="ij")
        a = (10 + 3 * x + 5 * y + 7 * z).astype(np.uint16)
        aff_b = _translate((4, 0, 0))
        b = (2 * (10 + 3 * (x + 4) + 5 * y + 7 * z) + 5).astype(np.uint16)
        return dict(a=a, b=b, aff_a=eye, aff_b=aff_b, prm=dict(
            render_scale=1.0, coefficients=(1, 1, 1), min_num_candidates=256,
            iterations=300, max_epsilon=0.05, min_inlier_ratio=1.0,
            min_num_inliers=256))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def case(name):
    """Inputs plus `ref`, the reference's match_pair result. Shared: do not
    modify."""
    c = _inputs(name)
    c["name"] = name
    c["ref"] = ir.match_pair(c["a"], c["aff_a"], c["b"], c["aff_b"],
                             **c["prm"])
    return c


# A 3-view chain for the solver: views 0-1 and 1-2 overlap, 0-2 do not.
@functools.lru_cache(maxsize=None)
def chain():
    affs = [_translate((0, 0, 0)), _translate((22, 3, 0)),
            _translate((44, -2, 1))]
    rng = np.random.default_rng(21)
    nb = 60
    blobs = np.column_stack([
        rng.uniform(-5, 90, nb), rng.uniform(-5, 45, nb),
        rng.uniform(-5, 35, nb), rng.uniform(5.0, 9.0, nb),
        rng.uniform(150.0, 700.0, nb)])
    gains = [(1.0, 0.0), (GAIN, OFFSET), (0.9, -40.0)]
    vols = []
    for aff, (g, o) in zip(affs, gains):
        w = _world(aff, DIMS)
        v = g * _scene(w, blobs) + o + rng.normal(0.0, 1.0, w.shape[:-1])
        vols.append(np.clip(np.rint(v), 0, 65535).astype(np.uint16))
    prm = dict(render_scale=1.0, coefficients=(2, 2, 2),
               min_num_candidates=200, iterations=300)
    pairs = []
    for i, j in ((0, 1), (1, 2)):
        r = ir.match_pair(vols[i], affs[i], vols[j], affs[j], **prm)
        pairs.append((i, j, r["records"]))
    return dict(vols=vols, affs=affs, prm=prm, pairs=pairs, gains=gains)
