"""GPU tests of the dot-product r-test (k_rtest_dot, BS_CORR_MODE=dot): its
raw integer sums, through bs_debug_rtest, must EQUAL numpy's exact uint64
sums and those of the wide and legacy kernels — for every 16-byte phase of
the shift on the hoisted path (row strides multiples of 8) and the per-row
path, differing tile sizes and offsets, the narrowest overlaps, all-65535
data on multi-chunk rows, full-wave rows, a 40-candidate list whose z-ranges
make blocks skip different candidates (the per-wave LDS slots and the
barrier-free candidate loop), and threads owning 1, 2, 3 and 4 rows (the
batched tail). A stitched pair must come out identical in all three modes.
The arithmetic, its bounds and its overflow limit are checked on the CPU
(tests/test_rtest_dot_cpu.py). Helpers as in test_gpu_rtest_wide.py."""

import os

import numpy as np
import pytest

from oracle import phasecorr, synth

pytestmark = pytest.mark.gpu


def _make_ctx(mode):
    from bigstitcher_spark_amd import Context

    old = os.environ.get("BS_CORR_MODE")
    os.environ["BS_CORR_MODE"] = mode  # read once, in bs_ctx_create
    try:
        return Context(0)
    finally:
        if old is None:
            del os.environ["BS_CORR_MODE"]
        else:
            os.environ["BS_CORR_MODE"] = old


@pytest.fixture(scope="module")
def ctxs():
    cs = [_make_ctx(m) for m in ("dot", "wide", "legacy")]
    yield cs
    for c in cs:
        c.close()


def _vol(shape_xyz, seed):
    """Random uint16 (nz, ny, nx) over the full range, 65535 included."""
    nx, ny, nz = shape_xyz
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 65536, size=(nz, ny, nx), dtype=np.uint16)
    v[rng.random(v.shape) < 0.05] = 65535
    return v


def _pair(a, b, off_a=None, size_a=None, off_b=None, size_b=None):
    full = lambda v: (v.shape[2], v.shape[1], v.shape[0])  # noqa: E731
    return dict(view_a=0, view_b=1,
                off_a=off_a or (0, 0, 0), size_a=size_a or full(a),
                off_b=off_b or (0, 0, 0), size_b=size_b or full(b))


def _ref_sums(a, b, pair, shifts):
    """Exact sums over each shift's overlap box, in uint64 (the largest
    term, 65535^2 * voxels, stays far below 2^64 at these sizes)."""
    def region(v, off, size):
        return v[off[2]:off[2] + size[2], off[1]:off[1] + size[1],
                 off[0]:off[0] + size[0]].astype(np.uint64)
    ra = region(a, pair["off_a"], pair["size_a"])
    rb = region(b, pair["off_b"], pair["size_b"])
    sums = np.zeros((len(shifts), 5), np.uint64)
    nvox = np.zeros(len(shifts), np.int64)
    for i, s in enumerate(shifts):
        lo = [max(0, -s[d]) for d in range(3)]
        hi = [min(pair["size_a"][d], pair["size_b"][d] - s[d])
              for d in range(3)]
        if any(h <= l for l, h in zip(lo, hi)):
            continue
        A = ra[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]]
        B = rb[lo[2] + s[2]:hi[2] + s[2], lo[1] + s[1]:hi[1] + s[1],
               lo[0] + s[0]:hi[0] + s[0]]
        sums[i] = [A.sum(), B.sum(), (A * A).sum(), (B * B).sum(),
                   (A * B).sum()]
        nvox[i] = A.size
    return sums, nvox


def _check(ctxs, a, b, pair, shifts):
    ref, nref = _ref_sums(a, b, pair, shifts)
    assert nref.max() > 0  # the case must scan something
    got = []
    for c in ctxs:
        c.upload(0, a)
        c.upload(1, b)
        c.reset_stats()
        sums, nvox = c.debug_rtest(pair, shifts)
        assert c.stats()["kernels"]["corr"]["launches"] == 1
        assert np.array_equal(nvox, nref)
        assert np.array_equal(sums, ref)
        got.append(sums)
    assert np.array_equal(got[0], got[1])  # dot == wide
    assert np.array_equal(got[0], got[2])  # dot == legacy


def _phase_shifts():
    """sx = -9..9 (every 16-byte phase, both signs) with mixed sy, sz."""
    sy = (-2, 0, 1, 3)
    sz = (-1, 0, 2)
    return [(sx, sy[i % 4], sz[i % 3]) for i, sx in enumerate(range(-9, 10))]


@pytest.mark.parametrize("shape", [(40, 12, 6), (37, 11, 5)],
                         ids=["40x12x6_hoisted", "37x11x5_per_row"])
def test_all_phases(ctxs, shape):
    a, b = _vol(shape, 1), _vol(shape, 2)
    _check(ctxs, a, b, _pair(a, b), _phase_shifts())


def test_differing_tiles_and_offsets(ctxs):
    a, b = _vol((40, 12, 6), 3), _vol((37, 11, 5), 4)
    pair = _pair(a, b, off_a=(3, 1, 1), size_a=(30, 9, 4),
                 off_b=(1, 2, 0), size_b=(33, 8, 5))
    _check(ctxs, a, b, pair, _phase_shifts())
    # whole views of unequal width: odd and even row strides together
    _check(ctxs, a, b, _pair(a, b), _phase_shifts())
    _check(ctxs, b, a, _pair(b, a), _phase_shifts())
    # both strides multiples of 8 (hoisted), tiles and offsets unequal
    a, b = _vol((40, 12, 6), 5), _vol((48, 11, 5), 6)
    pair = _pair(a, b, off_a=(3, 1, 1), size_a=(30, 9, 4),
                 off_b=(1, 2, 0), size_b=(41, 8, 5))
    _check(ctxs, a, b, pair, _phase_shifts())


@pytest.mark.parametrize("nx", range(1, 10))
def test_narrow_overlaps(ctxs, nx):
    a, b = _vol((40, 12, 6), 5), _vol((40, 12, 6), 6)
    shifts = [(40 - nx, 0, 0), (nx - 40, 1, 0), (40 - nx, -1, 1),
              (nx - 40, 0, -2)]
    _check(ctxs, a, b, _pair(a, b), shifts)
    # the same widths from narrow tiles at odd offsets
    pair = _pair(a, b, off_a=(5, 0, 0), size_a=(nx, 12, 6),
                 off_b=(2, 0, 0), size_b=(nx + 3, 12, 6))
    _check(ctxs, a, b, pair, [(0, 0, 0), (1, 0, 0), (2, 1, 0), (3, 0, 1)])


def test_all_max_values_multi_chunk(ctxs):
    """All-65535 on 1024x40x3. A 1024-wide row that starts on the 16-byte
    grid has 128 chunks, two per lane and row; rows that start one element
    off it (a 1024-wide region at x offset 1 of a 1040-wide view) have 129,
    so lane 0 walks three."""
    shifts = [(0, 0, 0), (1, 0, 0), (-3, 1, -1), (4, -2, 1), (-8, 0, 0)]
    a = np.full((3, 40, 1024), 65535, np.uint16)
    _check(ctxs, a, a.copy(), _pair(a, a), shifts)
    for w in (1040, 1037):  # hoisted, per-row
        a = np.full((3, 40, w), 65535, np.uint16)
        pair = _pair(a, a, off_a=(1, 0, 0), size_a=(1024, 40, 3),
                     off_b=(3, 0, 0), size_b=(1024, 40, 3))
        _check(ctxs, a, a.copy(), pair, shifts)


def test_full_wave_rows(ctxs):
    a, b = _vol((512, 16, 2), 7), _vol((512, 16, 2), 8)
    shifts = [(0, 0, 0), (1, 0, 0), (2, 1, 0), (7, -1, 1), (-3, 0, 0),
              (-8, 2, -1), (-5, 0, 1), (4, 0, 0)]
    _check(ctxs, a, b, _pair(a, b), shifts)


def test_forty_candidates_skipped_by_different_blocks(ctxs):
    """40 shifts whose z-ranges differ: plane z runs candidate i only when
    max(0, -sz_i) <= z < min(20, 20 - sz_i), so every block skips its own
    subset of the list and adds nothing for it."""
    a, b = _vol((40, 12, 20), 11), _vol((40, 12, 20), 12)
    shifts = [((i * 5) % 19 - 9, i % 5 - 2, (i * 7) % 39 - 19)
              for i in range(40)]
    assert len({s[2] for s in shifts}) > 30
    _check(ctxs, a, b, _pair(a, b), shifts)
    _check(ctxs, a, b, _pair(a, b), shifts[::-1])


@pytest.mark.parametrize("width", [64, 61], ids=["hoisted", "per_row"])
def test_rows_per_thread(ctxs, width):
    """nx = 52 is walked 8 lanes per row, 32 rows per block step, 256 rows
    per step of the whole y-split: ny = 400 gives threads 1 and 2 rows (the
    batched tail alone), ny = 650 gives 2 and 3, ny = 900 gives 3 and 4 (a
    batch of three, then a tail of one)."""
    a, b = _vol((width, 900, 2), 13), _vol((width, 900, 2), 14)
    nx = 52
    shifts = [(width - nx, 500, 0), (nx - width, -500, 1),
              (width - nx, 250, -1), (nx - width, 0, 0), (width - nx, 0, 1)]
    _check(ctxs, a, b, _pair(a, b), shifts)


@pytest.mark.parametrize("true_shift", [(5.25, -3.5, 2.0), (6.25, -3.5, 2.0)],
                         ids=["odd_sx", "even_sx"])
def test_stitch_modes_identical(ctxs, true_shift):
    a, b = synth.make_pair((64, 64, 64), true_shift, seed=11)
    ref = phasecorr.phase_correlation_shift(a, b, ds=(1, 1, 1))
    pair = _pair(a, b)
    got = []
    for c in ctxs:
        c.upload(0, a)
        c.upload(1, b)
        got.append(c.stitch_batch([pair], ds=(1, 1, 1))[0])
    d, w, l = got
    assert d["valid"] == w["valid"] == l["valid"] == ref["valid"]
    assert d["shift"].tobytes() == w["shift"].tobytes() == l["shift"].tobytes()
    assert (np.float64(d["r"]).tobytes() == np.float64(w["r"]).tobytes()
            == np.float64(l["r"]).tobytes())
    assert np.all(np.abs(d["shift"] - ref["shift"]) < 1e-3)
    assert d["r"] == pytest.approx(ref["r"], abs=1e-9)
