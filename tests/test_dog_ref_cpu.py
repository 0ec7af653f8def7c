"""CPU tests for Difference-of-Gaussian interest point detection: the
numpy restatement (tests/dog_ref.py) on inputs with a known answer, the
margins tests/test_gpu_detect.py relies on (asserted on the reference
alone, so a device comparison there can never be excused by a fragile
input), and the detect-interestpoints refusals that must not touch the GPU.
"""

import os
import subprocess

import numpy as np
import pytest

from tests import dog_cases as dc
from tests import dog_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.environ.get("BS_BIN",
                     os.path.join(ROOT, "bigstitcher_spark_amd", "bin"))


def _one_blob(centre_zyx, amp=0.5, sig=1.8, shape=(24, 26, 28)):
    zz, yy, xx = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape],
                             indexing="ij")
    cz, cy, cx = centre_zyx
    return amp * np.exp(-((zz - cz) ** 2 + (yy - cy) ** 2 + (xx - cx) ** 2)
                        / (2 * sig * sig))


def test_single_blob_subpixel():
    centre = (11.3, 12.6, 14.2)  # z,y,x
    vol = 0.2 + _one_blob(centre)  # noiseless, already in [0,1]
    r = dog_ref.detect(vol, 1.8, 0.008, 0.0, 1.0)
    assert len(r["value"]) == 1
    assert r["kind"][0] == 1 and r["converged"][0] == 1 and r["value"][0] > 0
    want = np.array(centre[::-1])
    assert np.abs(r["loc"][0] - want).max() <= 0.5
    assert np.array_equal(r["voxel"][0], np.rint(want))
    # the inverted volume: same place, a minimum, negated value
    inv = dog_ref.detect(1.0 - vol, 1.8, 0.008, 0.0, 1.0, find_min=True,
                         find_max=False)
    assert len(inv["value"]) == 1 and inv["kind"][0] == -1
    assert np.abs(inv["loc"][0] - r["loc"][0]).max() <= 1e-9
    assert abs(inv["value"][0] + r["value"][0]) <= 1e-12
    # MAX on the inverted volume sees only the faint ring around the
    # minimum (a DoG response has a side lobe of the opposite sign)
    ring = dog_ref.detect(1.0 - vol, 1.8, 0.008, 0.0, 1.0)
    assert np.all(ring["value"] < 0.1 * r["value"][0])


def test_taps_and_mirror():
    s1, s2, w = dog_ref.sigmas(1.8)
    assert len(dog_ref.taps(s1)) == 11 and len(dog_ref.taps(s2)) == 13
    assert abs(w - 1.0 / (2 ** 0.25 - 1)) < 1e-15
    assert abs(dog_ref.taps(s2).sum() - 1.0) < 1e-15
    # a constant volume has zero DoG whatever the mirror does, also when
    # the radius exceeds the axis length
    assert np.abs(dog_ref.dog_volume(np.full((3, 4, 20), 7.0), 1.8, 0.0,
                                     10.0)).max() < 1e-14
    # radius 6 on a 5-long axis: several reflections, checked by hand
    a = np.arange(5, dtype=np.float64).reshape(5, 1, 1)
    got = dog_ref._blur_axis(a, dog_ref.taps(s2), 0)[:, 0, 0]
    idx = lambda i: (i % 10) if (i % 10) < 5 else 9 - (i % 10)  # noqa: E731
    want = [sum(t * idx(z + k - 6) for k, t in enumerate(dog_ref.taps(s2)))
            for z in range(5)]
    assert np.abs(got - want).max() < 1e-14


def test_box_mean_drops_partial_cell():
    v = np.arange(4 * 6 * 7, dtype=np.uint16).reshape(4, 6, 7)
    b = dog_ref.box_mean(v, (2, 2, 1))
    assert b.shape == (4, 3, 3)
    assert b[1, 2, 1] == v[1, 4:6, 2:4].mean()


@pytest.mark.parametrize("which", ["bright", "dark"])
@pytest.mark.parametrize("shape", list(dc.BRIGHT_SHAPES))
def test_gpu_input_margins_quadratic(which, shape):
    """Every reference point converged and clears the final threshold by
    25 %, and there is one point per planted blob: a float32 device cannot
    legitimately gain or lose a point on these inputs."""
    r = dc.ref_detect(which, shape)
    assert len(r["value"]) == dc.BRIGHT_SHAPES[shape]
    assert np.all(r["converged"] == 1)
    assert np.abs(r["value"]).min() >= 1.25 * dc.T_BRIGHT
    assert np.all(r["kind"] == (1 if which == "bright" else -1))
    cen = (dc.bright if which == "bright" else dc.dark)(shape)[1][:, ::-1]
    for c in cen:  # each planted centre has a detection within 0.5 px
        assert np.abs(r["loc"] - c).max(axis=1).min() <= 0.5


@pytest.mark.parametrize("shape", list(dc.DS_SHAPES))
def test_gpu_input_margins_ds(shape):
    r = dc.ref_detect("bright", shape, (2, 2, 1))
    assert len(r["value"]) >= 5
    assert np.all(r["converged"] == 1)
    assert np.abs(r["value"]).min() >= 1.25 * dc.T_BRIGHT


@pytest.mark.parametrize("shape", list(dc.MIXED_SHAPES))
def test_gpu_input_margins_mixed(shape):
    """possible == sure and both equal the planted count per sign, so the
    5 % cap in the GPU test can never hide a failure."""
    _, _, sign = dc.mixed(shape)
    cl = dog_ref.classify(dc.ref_volume("mixed", shape), dc.T_MIXED, dc.EPS)
    for kind in (1, -1):
        sure, poss = cl[kind]
        assert np.array_equal(sure, poss)
        assert sure.sum() == (sign == kind).sum()
    r = dog_ref.detect(dc.mixed(shape)[0], dc.SIGMA, dc.T_MIXED, dc.LO, dc.HI,
                       find_min=True, find_max=True, localization="none",
                       D=dc.ref_volume("mixed", shape))
    assert len(r["value"]) == len(sign)
    assert np.all(r["converged"] == 1)


# ---- detect-interestpoints refusals (no XML read, no GPU call) -----------
_BASE = ["-x", "/nonexistent/dataset.xml", "-l", "beads", "-s", "1.8", "-t",
         "0.008", "-i0", "0", "-i1", "255"]


def _cli(args):
    return subprocess.run([os.path.join(BIN, "detect-interestpoints"), *args],
                          capture_output=True, text=True)


@pytest.mark.parametrize("flag", [
    ["--overlappingOnly"], ["--onlyCompareOverlapTiles"],
    ["--maxSpotsPerOverlap"], ["--medianFilter", "10"], ["--prefetch"],
    ["--keepTemporaryN5"]])
def test_cli_refused_flags(flag):
    r = _cli(_BASE + flag)
    assert r.returncode == 2, (r.stdout, r.stderr)
    lines = r.stderr.strip().splitlines()
    assert len(lines) == 1 and flag[0] in lines[0]


def test_cli_missing_required():
    r = _cli([a for a in _BASE if a not in ("-l", "beads")])
    assert r.returncode == 2 and "--label" in r.stderr
    for drop in ("-s", "-t", "-i0", "-i1", "-x"):
        i = _BASE.index(drop)
        assert _cli(_BASE[:i] + _BASE[i + 2:]).returncode == 2, drop
    assert _cli(_BASE + ["--type", "ALL"]).returncode == 2
    assert _cli(_BASE + ["--localization", "CUBIC"]).returncode == 2
    assert _cli(_BASE + ["-dsxy", "3"]).returncode == 2
    # a complete command line gets past the argument checks (exit 1: the
    # XML does not exist) — the refusals above are not a blanket exit 2
    assert _cli(_BASE).returncode == 1
