"""Inputs shared by tests/test_match_ref_cpu.py and tests/test_gpu_match.py
(not a test), with the reference results of tests/match_ref.py computed once
per case and cached.

Scene recipe: A = seeded uniform points in a box; B = A with 20 % dropped,
translated by SHIFT, Gaussian jitter sigma 0.05 px, plus 20 % unrelated
points, shuffled. Both sets sit at a large world offset so [PIN-F32PTS]'s
min subtraction matters.

The device computes in float32 and the reference in float64, so index
equality can only be asked where the reference's own decisions have margin.
The generator therefore removes points until the reference finds
  - no kNN rank gap below KNN_GAP relative (ranks 0..k, either set), and
  - no A descriptor with best * ratio / second within RATIO_MARGIN of 1,
    without and with the SEARCH_RADIUS used by the tests.
Each round removes every offending point (an offending descriptor removes
its A base point) and refills A from a small reserve, so A keeps exactly its
N points (one past a wave, one past a tile); B's own kNN near-ties cannot be
cured from A, so they are removed from B. tests/test_match_ref_cpu.py asserts the margins and
that only a handful of points went.

The lattice case has no margins at all: every coordinate is a small
integer, so every distance is exact in float32 and float64 alike and the
comparison pins the tie rules. It uses n = 2 so that the mean of
[PIN-DESCDIST] (a division by n) is exact too.
"""

from __future__ import annotations

import functools

import numpy as np

from tests import match_ref as mr

SHIFT = np.array([7.3, -4.6, 2.2])
JITTER = 0.05
WORLD0 = np.array([1000.5, 2000.25, -300.0])
RATIO = 3.0
SEARCH_RADIUS = 12.0
KNN_GAP = 1e-4
RATIO_MARGIN = 1e-3

# points per block of the kNN kernel's LDS tile (IP_TILE in bigstitch.hip):
# 257 is one past it
TILE = 256

SPARE = 16

# name -> (N, box xyz, n, r)
SCENES = {
    "n3": (3, (64, 64, 32), 3, 1),
    "n37": (37, (64, 64, 32), 3, 1),
    "n65": (65, (64, 64, 32), 3, 1),
    "n257": (TILE + 1, (128, 128, 64), 3, 1),
    "n1000": (1000, (256, 256, 64), 3, 1),
    "n1000_n3r0": (1000, (256, 256, 64), 3, 0),
    "n1000_n4r2": (1000, (256, 256, 64), 4, 2),
}
LATTICE = "lattice"
ALL = list(SCENES) + [LATTICE]


def make_scene(n_pts, box, seed):
    """-> A (N,3), B (M,3) float64 world coordinates and src (M,) int: the
    A index each B point came from, -1 for unrelated points."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.0, 1.0, (n_pts, 3)) * np.array(box, np.float64)
    keep = np.sort(rng.permutation(n_pts)[:n_pts - n_pts // 5])
    b = a[keep] + SHIFT + rng.normal(0.0, JITTER, (len(keep), 3))
    extra = rng.uniform(0.0, 1.0, (n_pts // 5, 3)) * np.array(box, np.float64)
    b = np.concatenate([b, extra + SHIFT])
    src = np.concatenate([keep, np.full(len(extra), -1)])
    perm = rng.permutation(len(b))
    return a + WORLD0, b[perm] + WORLD0, src[perm]


def _evaluate(a, b, n, r):
    a32, b32 = mr.to_f32(a, b)
    k = n + r
    res = dict(a32=a32, b32=b32, n=n, r=r,
               knn_a=mr.knn(a32, k), knn_b=mr.knn(b32, k))
    res["raw"], res["raw_sr"] = mr.match_raw_multi(
        a32, b32, n, r, (None, SEARCH_RADIUS))
    res["cand"] = mr.candidates(res["raw"], RATIO)
    res["cand_sr"] = mr.candidates(res["raw_sr"], RATIO)
    return res


def _offenders(res):
    C = res["raw"]["C"]
    bad_a = set(np.nonzero(res["knn_a"][2] < KNN_GAP)[0].tolist())
    bad_b = set(np.nonzero(res["knn_b"][2] < KNN_GAP)[0].tolist())
    for raw in (res["raw"], res["raw_sr"]):
        m = mr.ratio_margin(raw, RATIO)
        bad_a |= set((np.nonzero(m < RATIO_MARGIN)[0] // C).tolist())
    return sorted(bad_a), sorted(bad_b)


@functools.lru_cache(maxsize=None)
def case(name):
    """dict: a, b (float64 world), truth (A index -> B index or -1), n, r,
    removed (points dropped for margin), and the reference results a32,
    b32, knn_a, knn_b (idx, d2, gap), raw, raw_sr, cand, cand_sr."""
    if name == LATTICE:
        g = np.arange(5) * 4.0
        a = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
        b = a[::-1] + np.array([4.0, 0.0, 8.0])   # reversed order, shifted
        res = _evaluate(a + WORLD0, b + WORLD0, 2, 1)
        res.update(a=a + WORLD0, b=b + WORLD0, removed=0,
                   truth=np.arange(len(a))[::-1].copy())
        return _freeze(res)
    n_pts, box, n, r = SCENES[name]
    # A keeps exactly n_pts points: a removed point is replaced by the next
    # of SPARE reserve points generated with the scene (B was derived from
    # all of them, so a reserve point has its B partner like any other)
    a_all, b, src = make_scene(n_pts + SPARE, box, 7000 + n_pts)
    ida = np.arange(n_pts)
    nxt = n_pts
    removed = 0
    for _ in range(20):
        a = a_all[ida]
        res = _evaluate(a, b, n, r)
        bad_a, bad_b = _offenders(res)
        if not bad_a and not bad_b:
            break
        removed += len(bad_a) + len(bad_b)
        fill = np.arange(nxt, nxt + len(bad_a))
        nxt += len(bad_a)
        assert nxt <= len(a_all), f"{name}: reserve used up"
        ida = np.concatenate([np.delete(ida, bad_a), fill])
        b, src = np.delete(b, bad_b, axis=0), np.delete(src, bad_b)
    else:
        raise AssertionError(f"{name}: margins not reached")
    pos = {int(s): j for j, s in enumerate(src) if s >= 0}
    truth = np.array([pos.get(int(i), -1) for i in ida], np.int64)
    res.update(a=a, b=b, truth=truth, removed=removed)
    return _freeze(res)


def _freeze(res):
    for v in res.values():
        for x in (v if isinstance(v, tuple) else
                  v.values() if isinstance(v, dict) else (v,)):
            if isinstance(x, np.ndarray):
                x.setflags(write=False)
    return res
