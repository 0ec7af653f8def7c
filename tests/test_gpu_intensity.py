"""GPU tests of intensity matching (bs_intensity_match_pair /
Context.intensity_match_pair / bs_debug_intensity_render) against the numpy
contract in tests/intensity_ref.py, on the cases of tests/intensity_cases.py
(what those contain is asserted in tests/test_intensity_ref_cpu.py).

Every device result is an integer or a fixed formula of integers, so the
bounds are exact: grid geometry, the four render arrays, the bucket list and
all integer fields equal the reference's; a and b (doubles formed from exact
integer moments) agree to 1e-12 relative; two calls agree bit for bit."""

import os

import numpy as np
import pytest

from tests import intensity_cases as ic

pytestmark = pytest.mark.gpu

INT_FIELDS = ("cell_a", "cell_b", "n_cand", "n_inl", "best_it",
              "n_inl_first", "sp", "sq", "spp", "sqq", "spq")


@pytest.fixture(scope="module")
def ctx():
    from bigstitcher_spark_amd import Context

    c = Context(0)
    yield c
    c.close()


def _upload(ctx, c):
    ctx.upload(0, c["a"])
    ctx.upload(1, c["b"])


@pytest.mark.parametrize("name", ic.ALL)
def test_render_equals_reference(ctx, name):
    c = ic.case(name)
    _upload(ctx, c)
    prm = c["prm"]
    got = ctx.debug_intensity_render(
        0, c["aff_a"], 1, c["aff_b"], render_scale=prm["render_scale"],
        coefficients=prm["coefficients"],
        min_threshold=prm.get("min_threshold", 1.0),
        max_threshold=prm.get("max_threshold"))
    ref = c["ref"]["render"]
    assert got["origin"] == ref["origin"] and got["dims"] == ref["dims"]
    for k in ("P", "Q", "cell_a", "cell_b"):
        assert got[k].dtype == ref[k].dtype
        assert np.array_equal(got[k], ref[k]), (name, k)


@pytest.mark.parametrize("name", ic.ALL)
def test_matches_equal_reference(ctx, name):
    c = ic.case(name)
    _upload(ctx, c)
    got = ctx.intensity_match_pair(0, c["aff_a"], 1, c["aff_b"], **c["prm"])
    ref = c["ref"]["records"]
    assert len(got) == len(ref), (name, len(got), len(ref))
    for g, r in zip(got, ref):
        for k in INT_FIELDS:
            assert int(g[k]) == r[k], (name, k, g, r)
        assert abs(g["a"] - r["a"]) <= 1e-12 * abs(r["a"])
        assert abs(g["b"] - r["b"]) <= 1e-12 * abs(r["b"])
    again = ctx.intensity_match_pair(0, c["aff_a"], 1, c["aff_b"],
                                     **c["prm"])
    assert got.tobytes() == again.tobytes()


def test_sizing_convention(ctx):
    c = ic.case("shift_half")
    _upload(ctx, c)
    prm = ctx._intensity_params(
        **{**dict(min_threshold=1.0, max_threshold=None, max_epsilon=5.1,
                  min_inlier_ratio=0.1, min_num_inliers=10), **c["prm"]})
    n_ref = len(c["ref"]["records"])
    assert n_ref > 2
    rc, got, n = ctx.intensity_match_pair_raw(0, c["aff_a"], 1, c["aff_b"],
                                              prm, 0)
    assert rc == 0 and n == n_ref and len(got) == 0
    rc, got, n = ctx.intensity_match_pair_raw(0, c["aff_a"], 1, c["aff_b"],
                                              prm, 2)
    assert rc == 0 and n == n_ref and len(got) == 2
    assert [int(g["cell_a"]) for g in got] == [
        r["cell_a"] for r in c["ref"]["records"][:2]]


def test_error_codes(ctx):
    c = ic.case("shift_half")
    _upload(ctx, c)
    base = dict(render_scale=0.5, coefficients=(3, 2, 1),
                min_num_candidates=60, min_threshold=1.0, max_threshold=None,
                iterations=300, max_epsilon=5.1, min_inlier_ratio=0.1,
                min_num_inliers=10)

    def rc(va=0, vb=1, aff_b=c["aff_b"], **kw):
        prm = ctx._intensity_params(**{**base, **kw})
        return ctx.intensity_match_pair_raw(va, c["aff_a"], vb, aff_b, prm,
                                            0)[0]

    EINVAL, ENOVIEW, EUNSUP = -1, -5, -6
    assert rc() == 0
    assert rc(vb=77) == ENOVIEW and rc(va=78) == ENOVIEW
    assert rc(render_scale=0.0) == EINVAL
    assert rc(render_scale=1.5) == EINVAL
    assert rc(render_scale=float("nan")) == EINVAL
    assert rc(coefficients=(3, 0, 1)) == EINVAL
    assert rc(iterations=0) == EINVAL
    assert rc(iterations=4097) == EUNSUP
    assert rc(iterations=4096) == 0
    assert rc(coefficients=(64, 32, 32)) == EUNSUP  # 65536 cells
    assert rc(aff_b=np.zeros((3, 4))) == EINVAL  # singular
    with pytest.raises(RuntimeError, match="not uploaded"):
        ctx.intensity_match_pair(0, c["aff_a"], 99, c["aff_b"])


def test_size_limits_are_refused(ctx):
    """More than 2^31 grid samples is refused before anything is allocated;
    a bucket above 2^24 members (here 257 * 256 * 256 samples in the single
    cell pair) is refused once it has been counted."""
    EUNSUP = -6
    eye = np.hstack([np.eye(3), np.zeros((3, 1))])
    base = dict(render_scale=1.0, coefficients=(1, 1, 1),
                min_num_candidates=1, min_threshold=1.0, max_threshold=None,
                iterations=1, max_epsilon=5.1, min_inlier_ratio=0.1,
                min_num_inliers=10)
    c = ic.case("lattice")
    _upload(ctx, c)
    big = eye.copy()
    big[:, :3] *= 2000.0  # 12 x 8 x 4 voxels spread over 22001 x 14001 x 6001
    prm = ctx._intensity_params(**base)
    assert ctx.intensity_match_pair_raw(0, big, 1, big, prm, 0)[0] == EUNSUP
    flat = np.full((256, 256, 257), 100, np.uint16)
    ctx.upload(0, flat)
    ctx.upload(1, flat)
    rc, _, _ = ctx.intensity_match_pair_raw(0, eye, 1, eye, prm, 0)
    assert rc == EUNSUP
    prm = ctx._intensity_params(**{**base, "coefficients": (2, 1, 1)})
    rc, _, n = ctx.intensity_match_pair_raw(0, eye, 1, eye, prm, 0)
    assert rc == 0 and n == 0  # two buckets below the limit, no spread in P
    ctx.release(0)
    ctx.release(1)


def test_kernel_stats_are_reported(ctx):
    c = ic.case("shift_int")
    _upload(ctx, c)
    ctx.reset_stats()
    ctx.intensity_match_pair(0, c["aff_a"], 1, c["aff_b"], **c["prm"])
    st = ctx.stats()["kernels"]
    for k in ("int_render", "int_moments", "int_ransac"):
        assert st[k]["launches"] >= 1, k
    assert st["int_render"]["launches"] == 1  # one call sized and filled


# CLI end to end ------------------------------------------------------------
def test_cli_match_solve_fuse(tmp_path):
    """Two tiles -> match-intensities -> solve-intensities -> affine-fusion
    --intensityN5Path. Coefficients within 1e-6 / 1e-6 sigma of the reference
    pipeline's (same bounds as the solver test); the two corrected tiles,
    read back from fusions in which the first resp. the last view wins,
    differ over the overlap by at most a fifth of the raw difference."""
    from tests import intensity_ref as ir
    from tests import intensity_io as tci

    c = ic.case("shift_int")
    prm = c["prm"]
    cg = prm["coefficients"]
    d = str(tmp_path)
    xml = tci.write_tiles(d, (c["a"], c["b"]), (c["aff_a"], c["aff_b"]))
    mt, co, fused = (os.path.join(d, n) for n in
                     ("matches.n5", "coeff.n5", "fused.n5"))
    r = tci.run("match-intensities", "-x", xml, "-o", mt,
                "--numCoefficients", "%d,%d,%d" % cg, "--renderScale", "1.0",
                "--minNumCandidates", str(prm["min_num_candidates"]),
                "--numIterations", str(prm["iterations"]),
                "--minInlierRatio", str(prm["min_inlier_ratio"]))
    assert r.returncode == 0, r.stderr + r.stdout
    r = tci.run("solve-intensities", "-x", xml, "--matchesPath", mt, "-o", co,
                "--numCoefficients", "%d,%d,%d" % cg)
    assert r.returncode == 0, r.stderr + r.stdout
    ref, sigma, cond = ir.solve_dense(2, cg, [(0, 1, c["ref"]["records"])])
    assert cond <= 1e4
    for v in range(2):
        got = tci.read_coefficients(co, f"setup{v}/timepoint0/intensity")
        assert got.shape == ref[v].shape
        assert np.abs(got[0] - ref[v][0]).max() <= 1e-6
        assert np.abs(got[1] - ref[v][1]).max() <= 1e-6 * sigma
    r = tci.run("create-fusion-container", "-x", xml, "-s", "N5", "-o", fused,
                "--blockSize", "32,32,32", "--dataType", "FLOAT32")
    assert r.returncode == 0, r.stderr + r.stdout
    from tests import n5util

    tiles = []
    for ftype in ("LOWEST_VIEWID_WINS", "HIGHEST_VIEWID_WINS"):
        r = tci.run("affine-fusion", "-o", fused, "-f", ftype,
                    "--intensityN5Path", co)
        assert r.returncode == 0, r.stderr + r.stdout
        vol, _ = n5util.read_dataset(fused, "ch0tp0/s0")
        assert vol.shape == (28, 40, 62)
        tiles.append(vol[:, 4:36, 22:40].astype(np.float64))
    a = c["a"][:, 4:36, 22:40].astype(np.float64)
    b = c["b"][:, 0:32, 0:18].astype(np.float64)
    before = np.abs(a - b).mean()
    after = np.abs(tiles[0] - tiles[1]).mean()
    print("seam: mean |A-B| %.2f -> %.2f" % (before, after))
    assert after <= before / 5.0


def test_cli_eviction_gives_the_same_matches(tmp_path):
    """Three mutually overlapping tiles: with room for two resident views
    match-intensities evicts and reads one of them again, and writes the
    same container as with all three resident."""
    from tests import intensity_io as tci

    affs = [ic._translate(t) for t in ((0, 0, 0), (12, 2, 0), (24, -2, 1))]
    rng = np.random.default_rng(31)
    blobs = np.column_stack([
        rng.uniform(-5, 70, 30), rng.uniform(-5, 45, 30),
        rng.uniform(-5, 35, 30), rng.uniform(5.0, 9.0, 30),
        rng.uniform(150.0, 700.0, 30)])
    vols = [np.rint(g * ic._scene(ic._world(a, ic.DIMS), blobs) + o)
            .astype(np.uint16)
            for a, (g, o) in zip(affs, ((1.0, 0.0), (1.25, 150.0),
                                        (0.9, 40.0)))]
    d = str(tmp_path)
    xml = tci.write_tiles(d, vols, affs)
    outs = []
    for name, budget in (("all.n5", None), ("two.n5", "0")):
        env = dict(os.environ)
        if budget is not None:
            env["BS_INTENSITY_BUDGET_MB"] = budget
        out = os.path.join(d, name)
        r = tci.run("match-intensities", "-x", xml, "-o", out,
                    "--numCoefficients", "2,2,2", "--renderScale", "1.0",
                    "--minNumCandidates", "200", "--numIterations", "300",
                    env=env)
        assert r.returncode == 0, r.stderr + r.stdout
        assert "3 overlapping pairs" in r.stdout
        assert ("4 view uploads" if budget else "3 view uploads") in r.stdout
        outs.append(out)
    for pair in ("tp0_setup0__tp0_setup1", "tp0_setup0__tp0_setup2",
                 "tp0_setup1__tp0_setup2"):
        blocks = [open(os.path.join(o, "matches", pair, "0", "0"),
                       "rb").read() for o in outs]
        assert len(blocks[0]) > 12 and blocks[0] == blocks[1]
