"""CPU tests of the intensity-matching contract (tests/intensity_ref.py), of
what tests/intensity_cases.py promises to contain, and of the host-only
bs_intensity_solve (through ctypes and as a sanitised stand-alone program).

Bounds:
  gain, offset    accepted buckets recover 1.25 within 2 % and 150 within 10
                  grey levels despite the planted outliers
  solve           |da| <= 1e-6, |db| <= 1e-6 * sigma against dense least
                  squares of the same E: the CG stops at a relative residual
                  of 1e-10 and the scaled normal matrix has a condition number
                  that the test asserts to be <= 1e4
  pipeline        match -> solve -> apply cuts the mean |A - B| over the
                  overlap to at most one fifth (a condition on the inputs)
"""

import os
import subprocess

import numpy as np
import pytest

from tests import intensity_cases as ic
from tests import intensity_ref as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cases_contain_what_they_promise():
    sizes = []
    for name in ic.ALL:
        sizes += list(ic.case(name)["ref"]["buckets"].values())
    assert any(0 < n < 256 for n in sizes)
    assert 256 in sizes
    assert any(n > 256 and n % 256 for n in sizes)
    assert ic.case("sheared")["ref"]["dropped_small"]
    assert ic.case("shift_int")["ref"]["rejected_ratio"]
    assert {ic.case(n)["prm"]["iterations"] for n in ic.ALL} >= {
        7, 300, 1000, 4096}
    for name in ic.ALL:
        if name != "disjoint":
            assert ic.case(name)["ref"]["records"], name


def test_disjoint_is_empty():
    r = ic.case("disjoint")["ref"]
    assert r["render"]["dims"] == (0, 0, 0) and not r["records"]


def test_sheared_search_boxes_hold_non_members():
    """Under rotation + shear a bucket's bounding box holds samples of other
    buckets: the kernels must test ids, not trust the box."""
    r = ic.case("sheared")["ref"]["render"]
    ca, cb, ok = r["cell_a"], r["cell_b"], r["P"] >= 0
    mixed = 0
    for rec in ic.case("sheared")["ref"]["records"]:
        m = ok & (ca == rec["cell_a"]) & (cb == rec["cell_b"])
        z, y, x = np.nonzero(m)
        box = (slice(z.min(), z.max() + 1), slice(y.min(), y.max() + 1),
               slice(x.min(), x.max() + 1))
        mixed += m[box].sum() < ok[box].sum()
    assert mixed >= 5


def test_thresholds_both_bite():
    c = ic.case("thresholds")
    full = ir.render(c["a"], c["aff_a"], c["b"], c["aff_b"],
                     render_scale=c["prm"]["render_scale"],
                     coefficients=c["prm"]["coefficients"])
    P, Q = full["P"], full["Q"]
    inside = P >= 0
    lo, hi = 8 * c["prm"]["min_threshold"], 8 * c["prm"]["max_threshold"]
    assert np.any(inside & ((P < lo) | (Q < lo)))
    assert np.any(inside & ((P > hi) | (Q > hi)))
    kept = c["ref"]["render"]["P"] >= 0
    assert 0 < kept.sum() < inside.sum()


def test_lattice_ties_go_to_the_lowest_iteration():
    c = ic.case("lattice")
    (rec,) = c["ref"]["records"]
    assert rec["n_cand"] == rec["n_inl"] == rec["n_inl_first"] == 256
    assert rec["a"] == 2.0 and rec["b"] == 5.0
    # the winner is the first hypothesis that is not void
    P = c["ref"]["render"]["P"].ravel()
    for it in range(rec["best_it"] + 1):
        i1 = ir.splitmix64(ir.SEED ^ (it << 8)) % 256
        i2 = ir.splitmix64(ir.SEED ^ ((it << 8) | 1)) % 256
        assert (P[i1] != P[i2]) == (it == rec["best_it"])


def test_splitmix64_published_vector():
    # first outputs of splitmix64 seeded with 0 (Vigna's reference code)
    assert ir.splitmix64(0) == 0xE220A8397B1DCDAF
    assert ir.splitmix64(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4


@pytest.mark.parametrize("name", ["shift_int", "shift_half", "sheared",
                                  "thresholds"])
def test_reference_recovers_gain_and_offset(name):
    for r in ic.case(name)["ref"]["records"]:
        assert abs(r["a"] - ic.GAIN) <= 0.02 * ic.GAIN, r
        assert abs(r["b"] - ic.OFFSET) <= 10.0, r
        assert r["n_inl"] >= r["n_inl_first"]


def _solve_native(nviews, cg, pairs, **kw):
    from bigstitcher_spark_amd import _native

    arr = [(i, j, ir.records_array(recs, _native.INTENSITY_MATCH_DTYPE))
           for i, j, recs in pairs]
    return _native.intensity_solve(nviews, cg, arr, **kw)


def test_solve_matches_dense_least_squares():
    ch = ic.chain()
    cg = ch["prm"]["coefficients"]
    assert all(len(recs) >= 2 for _, _, recs in ch["pairs"])
    ref, sigma, cond = ir.solve_dense(3, cg, ch["pairs"])
    assert cond <= 1e4, cond
    got, iters, relres = _solve_native(3, cg, ch["pairs"])
    assert got.shape == ref.shape == (3, 2, 2, 2, 2)
    assert relres <= 1e-10 and 0 < iters < 1000
    da = np.abs(got[:, 0] - ref[:, 0]).max()
    db = np.abs(got[:, 1] - ref[:, 1]).max()
    print("solve: cond %.1f iters %d relres %.2e da %.2e db %.2e sigma %.1f"
          % (cond, iters, relres, da, db, sigma))
    assert da <= 1e-6
    assert db <= 1e-6 * sigma
    # views are not identity any more, and differ from each other
    assert np.abs(got[0, 0] - got[1, 0]).min() > 0.05


def test_solve_unmatched_view_is_identity_and_errors():
    ch = ic.chain()
    cg = ch["prm"]["coefficients"]
    got, _, _ = _solve_native(4, cg, ch["pairs"])  # view 3 has no matches
    assert np.all(got[3, 0] == 1.0) and np.all(got[3, 1] == 0.0)
    got, iters, _ = _solve_native(2, cg, [])
    assert iters == 0 and np.all(got[:, 0] == 1.0) and np.all(got[:, 1] == 0)
    with pytest.raises(RuntimeError):
        _solve_native(1, cg, ch["pairs"])  # view index out of range
    with pytest.raises(RuntimeError):
        _solve_native(3, (1, 1, 1), ch["pairs"])  # cell id out of range


def test_reference_pipeline_cuts_the_seam_difference():
    ch = ic.chain()
    cg = ch["prm"]["coefficients"]
    coeff, _, _ = ir.solve_dense(3, cg, ch["pairs"])
    for i, j in ((0, 1), (1, 2)):
        r = ir.render(ch["vols"][i], ch["affs"][i], ch["vols"][j],
                      ch["affs"][j], **ch["prm"])
        ok = r["P"] >= 0
        p, q = r["P"][ok] / 8.0, r["Q"][ok] / 8.0
        la = [v[ok] for v in r["local_a"]]
        lb = [v[ok] for v in r["local_b"]]
        aa, ba = ir.sample_coefficients(coeff[i], la, ic.DIMS)
        ab, bb = ir.sample_coefficients(coeff[j], lb, ic.DIMS)
        before = np.abs(p - q).mean()
        after = np.abs(aa * p + ba - (ab * q + bb)).mean()
        print("pair %d-%d: mean |A-B| %.2f -> %.2f" % (i, j, before, after))
        assert after <= before / 5.0


def test_intensity_solve_host_program(tmp_path):
    """The stand-alone program builds with g++ under the address and
    undefined-behaviour sanitizers and passes."""
    exe = str(tmp_path / "intensity_solve_host")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall",
                        "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests",
                                     "intensity_solve_host.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_kernel_names_follow_the_header_enum():
    """stats() labels timings by position: the binding's name list has to
    spell the ids of enum bs_kernel_id in order."""
    import re

    from bigstitcher_spark_amd._native import BS_K_NAMES

    with open(os.path.join(ROOT, "include", "bigstitch.h")) as f:
        body = f.read().split("enum bs_kernel_id {")[1].split("};")[0]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ids = re.findall(r"\bBS_K_([A-Z0-9_]+)\b", body)
    assert ids[-1] == "COUNT"
    assert [i.lower() for i in ids[:-1]] == BS_K_NAMES
    assert {"int_render", "int_moments", "int_ransac"} <= set(BS_K_NAMES)
