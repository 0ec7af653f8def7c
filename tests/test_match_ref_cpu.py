"""CPU tests of the interest-point matching contract: the numpy reference
(tests/match_ref.py) on the shared inputs (tests/match_cases.py) has the
margins the GPU comparisons in tests/test_gpu_match.py rely on, and the
host-side bs_ransac (no GPU) recovers planted transforms."""

import os
import subprocess

import numpy as np
import pytest

from tests import match_cases as mc
from tests import match_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = [s for s in mc.SCENES if s != "n3"]


# -- reference margins ------------------------------------------------------
@pytest.mark.parametrize("name", list(mc.SCENES))
def test_margins(name):
    c = mc.case(name)
    N = mc.SCENES[name][0]
    assert len(c["a"]) == N
    print(f"{name}: na={len(c['a'])} nb={len(c['b'])} removed={c['removed']}")
    assert c["removed"] <= max(4, N // 50)     # a handful
    for key in ("knn_a", "knn_b"):
        assert c[key][2].min(initial=np.inf) >= mc.KNN_GAP
    for key in ("raw", "raw_sr"):
        m = mr.ratio_margin(c[key], mc.RATIO)
        assert m.min(initial=np.inf) >= mc.RATIO_MARGIN
        raw = c[key]
        ok = np.isfinite(raw["second"])
        if ok.any():
            close = np.mean(raw["second"][ok] < 1.001 * raw["best"][ok])
            print(f"  {key}: best/second within 1e-3 in {close:.4%}")
            assert close <= 0.02    # the GPU raw test's exclusion cap


def test_empty_case():
    c = mc.case("n3")
    assert len(c["raw"]["best"]) == 0 and len(c["cand"]) == 0
    assert np.all(c["knn_a"][0] == -1)


def test_lattice_is_exact():
    """Every lattice quantity is an integer or a half: exact in float32."""
    c = mc.case(mc.LATTICE)
    assert c["n"] == 2
    for key in ("raw", "raw_sr"):
        for q in ("best", "second"):
            v = c[key][q]
            v = v[np.isfinite(v)]
            assert np.array_equal(v * 2, np.rint(v * 2))
            assert np.array_equal(v.astype(np.float32).astype(np.float64), v)
    d2 = c["knn_a"][1]
    assert np.array_equal(d2, np.rint(d2))
    # ties everywhere: the lower-index rule decides
    assert c["knn_a"][2].max() == 0.0
    assert np.mean(c["raw"]["second"] == c["raw"]["best"]) > 0.5


@pytest.mark.parametrize("name", ["n37", "n257"])
def test_descriptors_translation_invariant(name):
    c = mc.case(name)
    n, r = c["n"], c["r"]
    # float64 throughout, on a 1/16 px grid so that the shift is exact
    a32 = np.rint(np.asarray(c["a32"], np.float64) * 16) / 16
    moved = a32 + np.array([64.0, -128.0, 32.5])
    assert np.array_equal(moved - np.array([64.0, -128.0, 32.5]), a32)
    d0 = mr.descriptors(a32, n, r)
    d1 = mr.descriptors(moved, n, r)
    assert d0.shape == (len(a32) * len(mr.subsets(n, r)), n, 3)
    assert np.array_equal(d0, d1)


@pytest.mark.parametrize("name", SCENES)
def test_candidates_are_mostly_true(name):
    c = mc.case(name)
    for key in ("cand", "cand_sr"):
        cand = c[key]
        true = int(np.sum(c["truth"][cand[:, 0]] == cand[:, 1]))
        false = len(cand) - true
        print(f"{name} {key}: {len(cand)} candidates, {false} false")
        assert true >= 12
        assert false / len(cand) < 0.9          # RANSAC's outlier tolerance
        # [PIN-AMBIG]: unique on both sides, sorted by (a, b)
        assert len(np.unique(cand[:, 0])) == len(cand)
        assert len(np.unique(cand[:, 1])) == len(cand)
        assert np.all(np.diff(cand[:, 0]) > 0)


def test_radius_eligibility():
    """With a search radius every best_b lies within it."""
    c = mc.case("n1000")
    raw = c["raw_sr"]
    C = raw["C"]
    has = raw["best_b"] >= 0
    pa = np.asarray(c["a32"], np.float64)[np.nonzero(has)[0] // C]
    pb = np.asarray(c["b32"], np.float64)[raw["best_b"][has] // C]
    assert np.all(np.linalg.norm(pa - pb, axis=1) <= mc.SEARCH_RADIUS + 1e-3)
    assert not np.array_equal(raw["best_b"], c["raw"]["best_b"])


# -- bs_ransac through ctypes (host only) -----------------------------------
@pytest.fixture(scope="module")
def ransac():
    try:
        from bigstitcher_spark_amd._native import load_lib, ransac as fn
        load_lib()
    except Exception as e:  # library not built / not loadable on this host
        pytest.skip(f"libbigstitch not available: {e}")
    return fn


def _rot(ax, ang):
    ax = np.asarray(ax, float) / np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K


PLANTED = {
    "translation": np.hstack([np.eye(3), [[7.3], [-4.6], [2.2]]]),
    "rigid": np.hstack([_rot((1, 2, 3), 0.4), [[5.0], [-3.0], [2.0]]]),
    "affine": np.array([[1.02, 0.01, 0.0, 5.0], [-0.02, 0.97, 0.03, -3.0],
                        [0.01, 0.0, 1.05, 2.0]]),
}


def _planted(model, n, outliers, seed):
    rng = np.random.default_rng(seed)
    pa = rng.uniform(0, 200, (n, 3))
    T = PLANTED[model]
    pb = pa @ T[:, :3].T + T[:, 3]
    bad = np.zeros(n, bool)
    bad[rng.permutation(n)[:outliers]] = True
    pb[bad] += rng.uniform(40, 140, (outliers, 3))
    return pa, pb, bad


@pytest.mark.parametrize("model", list(PLANTED))
@pytest.mark.parametrize("outliers", [0, 40])
def test_ransac_recovers_planted(ransac, model, outliers):
    pa, pb, bad = _planted(model, 100, outliers, 5)
    mask, M, n = ransac(pa, pb, model=model, regularizer="none",
                        max_epsilon=0.5, iterations=2000)
    assert n == 100 - outliers and np.array_equal(mask, ~bad)
    err = np.abs(M - PLANTED[model]).max()
    print(f"{model} outliers={outliers}: max model error {err:.3g}")
    assert err <= 1e-6
    mask2, M2, n2 = ransac(pa, pb, model=model, regularizer="none",
                           max_epsilon=0.5, iterations=2000)
    assert n2 == n and mask2.tobytes() == mask.tobytes()
    assert M2.tobytes() == M.tobytes()


def test_ransac_regularised_defaults(ransac):
    """AFFINE regularised by RIGID at lambda 0.1 on rigid data is exact."""
    pa, pb, bad = _planted("rigid", 100, 40, 6)
    mask, M, n = ransac(pa, pb, max_epsilon=0.5, iterations=2000)
    assert n == 60 and np.array_equal(mask, ~bad)
    assert np.abs(M - PLANTED["rigid"]).max() <= 1e-6


def test_ransac_pure_noise(ransac):
    rng = np.random.default_rng(9)
    pa, pb = rng.uniform(0, 200, (2, 80, 3))
    for model in PLANTED:
        mask, M, n = ransac(pa, pb, model=model, regularizer="none",
                            max_epsilon=0.5, iterations=500)
        assert n == 0 and not mask.any()
        assert np.array_equal(M, np.hstack([np.eye(3), np.zeros((3, 1))]))


def test_ransac_on_reference_candidates(ransac):
    """The scene's candidates, false ones included, give back SHIFT."""
    c = mc.case("n1000")
    cand = c["cand"]
    pa, pb = c["a"][cand[:, 0]], c["b"][cand[:, 1]]
    mask, M, n = ransac(pa, pb, model="translation", regularizer="none")
    true = c["truth"][cand[:, 0]] == cand[:, 1]
    assert np.array_equal(mask, true)
    assert np.abs(M[:, 3] - mc.SHIFT).max() < 3 * mc.JITTER / np.sqrt(n) + 1e-9


def test_ransac_host_program(tmp_path):
    """The stand-alone program builds with plain g++ and passes."""
    exe = str(tmp_path / "ransac_host")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall",
                        os.path.join(ROOT, "tests", "ransac_host.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
