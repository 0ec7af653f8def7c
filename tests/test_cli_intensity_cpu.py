"""CPU tests of the intensity CLIs: what match-intensities refuses before it
touches a GPU, and solve-intensities (host only) on a match container
written here in the [PIN-INTMATCH-IO] layout, against the dense reference
solve of tests/intensity_ref.py (|da| <= 1e-6, |db| <= 1e-6 sigma, as in
tests/test_intensity_ref_cpu.py)."""

import os

import numpy as np

from tests import intensity_cases as ic
from tests import intensity_ref as ir
from tests import n5util
from tests.intensity_io import read_coefficients, run, write_matches


def test_match_intensities_refuses_what_is_not_built(tmp_path):
    out = str(tmp_path / "m.n5")
    r = run("match-intensities", "-x", "nowhere.xml", "-o", out, "--method",
            "HISTOGRAM")
    assert r.returncode == 2 and "not built" in r.stderr
    r = run("match-intensities", "-x", "nowhere.xml", "-o", out, "--maxTrust",
            "2.5")
    assert r.returncode == 2 and "not built" in r.stderr
    r = run("match-intensities", "-o", out)
    assert r.returncode == 2 and "--xml" in r.stderr
    r = run("match-intensities", "-x", "nowhere.xml", "-o", out,
            "--numIterations", "5000")
    assert r.returncode == 2
    assert not os.path.exists(out)


def test_solve_intensities_cli(tmp_path):
    ch = ic.chain()
    cg = ch["prm"]["coefficients"]
    d = str(tmp_path)
    # the XML only has to list the three views
    xml = os.path.join(d, "dataset.xml")
    n5util.make_dataset_xml(xml, "dataset.n5", [
        dict(id=i, dims=ic.DIMS, pos=tuple(ch["affs"][i][:, 3]))
        for i in range(3)])
    mt, co = os.path.join(d, "matches.n5"), os.path.join(d, "coeff.n5")
    write_matches(mt, cg, [((0, i), (0, j), recs)
                           for i, j, recs in ch["pairs"]])
    r = run("solve-intensities", "-x", xml, "--matchesPath", mt, "-o", co,
            "--numCoefficients", "2,2,2", "--intensityN5Group", "grp",
            "--intensityN5Dataset", "coef")
    assert r.returncode == 0, r.stderr + r.stdout
    assert "Connected pairs: 2" in r.stdout and "different" not in r.stderr
    ref, sigma, cond = ir.solve_dense(3, cg, ch["pairs"])
    assert cond <= 1e4
    for v in range(3):
        got = read_coefficients(co, f"grp/setup{v}/timepoint0/coef")
        assert got.shape == (2, 2, 2, 2)
        assert np.abs(got[0] - ref[v][0]).max() <= 1e-6
        assert np.abs(got[1] - ref[v][1]).max() <= 1e-6 * sigma
    # a different --numCoefficients is warned about, as the reference does;
    # here the stored cell ids then fall outside the grid
    r = run("solve-intensities", "-x", xml, "--matchesPath", mt, "-o",
            os.path.join(d, "c2.n5"), "--numCoefficients", "1,1,1")
    assert "different from specified numCoefficients" in r.stderr
    assert r.returncode == 1
    r = run("solve-intensities", "-x", xml, "--matchesPath", mt, "-o",
            os.path.join(d, "c3.h5"))
    assert r.returncode == 2 and "not built" in r.stderr
