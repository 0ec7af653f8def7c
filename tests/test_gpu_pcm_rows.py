"""GPU tests of the sparse PCM (BS_PCM_MODE=rows): the
inverse x pass of the normal path keeps only the row maxima, and a second
pass over a device-side row list writes the rows the peak stage reads
(the rows R with rowmax >= d5 and their 8 periodic neighbours). Everything
is compared byte for byte with a BS_PCM_MODE=full context, which writes
the whole PCM as before. Inputs: tests/peak_prefilter_cases.py (their
prefilter margins are asserted on the CPU in test_peak_prefilter_cpu.py)."""

import os

import numpy as np
import pytest

from oracle import synth
from tests import peak_prefilter_cases as pc

pytestmark = pytest.mark.gpu


def _make_ctx(mode):
    from bigstitcher_spark_amd import Context

    old = os.environ.get("BS_PCM_MODE")
    os.environ["BS_PCM_MODE"] = mode  # read once, in bs_ctx_create
    try:
        return Context(0)
    finally:
        if old is None:
            del os.environ["BS_PCM_MODE"]
        else:
            os.environ["BS_PCM_MODE"] = old


@pytest.fixture(scope="module")
def ctxs():
    rows, full = _make_ctx("rows"), _make_ctx("full")
    yield rows, full
    rows.close()
    full.close()


def _pair_desc(a, va=0, vb=1):
    nz, ny, nx = a.shape
    return dict(view_a=va, view_b=vb, off_a=(0, 0, 0), size_a=(nx, ny, nz),
                off_b=(0, 0, 0), size_b=(nx, ny, nz))


def _stitch(c, a, b, ds=(1, 1, 1), pad_mode="pow2"):
    """One pair -> dict(res, v, idx, launches of peak / peak_rows /
    fft_x_inv)."""
    c.upload(0, a)
    c.upload(1, b)
    c.reset_stats()
    res = c.stitch_batch([_pair_desc(a)], ds=ds, pad_mode=pad_mode,
                         min_overlap_ratio=0.05)[0]
    v, idx = c.debug_last_top5()
    k = c.stats()["kernels"]
    return dict(res=res, v=v, idx=idx, peak=k["peak"]["launches"],
                peak_rows=k["peak_rows"]["launches"],
                x_inv=k["fft_x_inv"]["launches"])


def _dirty(c, shape, shift, seed, ds=(1, 1, 1), pad_mode="pow2"):
    """Stitch ANOTHER pair of the same dims first: a single-pair batch
    always runs in slot 0, so the next pair finds that pair's rows in the
    PCM buffer and its stamps in the row-stamp array (the real-use
    condition: the buffer is never cleared between pairs)."""
    a, b = synth.make_pair(shape, shift, seed=seed + 1000)
    _stitch(c, a, b, ds, pad_mode)


def _run_pair(ctxs, a, b, shape, shift, seed, ds=(1, 1, 1), pad="pow2"):
    """The pair through both contexts, with everything the tests compare:
    rows context -> result, row list, raw buffer, then the rebuilt PCM;
    full context -> result and its PCM."""
    rows, full = ctxs
    _dirty(rows, shape, shift, seed, ds, pad)
    gr = _stitch(rows, a, b, ds, pad)
    gr["rowlist"] = rows.debug_rowlist()
    gr["raw"] = rows.debug_pcm(raw=True)  # before the rebuild below
    gr["pcm"] = rows.debug_pcm()
    gf = _stitch(full, a, b, ds, pad)
    gf["rowlist"] = full.debug_rowlist()
    gf["pcm"] = full.debug_pcm()
    return gr, gf


_CACHE = {}


@pytest.fixture
def run(ctxs, request):
    """Each PAIR_CASES entry runs once; the tests share the results."""
    case = request.param
    name, shape, shift, seed, ds, pad = case
    if name not in _CACHE:
        a, b = pc.make_pair_case(case)
        _CACHE[name] = _run_pair(ctxs, a, b, shape, shift, seed, ds, pad)
    return _CACHE[name]


def _assert_equal(gr, gf):
    assert gr["res"]["valid"] == gf["res"]["valid"]
    assert gr["res"]["shift"].tobytes() == gf["res"]["shift"].tobytes()
    assert (np.float64(gr["res"]["r"]).tobytes() ==
            np.float64(gf["res"]["r"]).tobytes())
    assert gr["v"].tobytes() == gf["v"].tobytes()
    assert np.array_equal(gr["idx"], gf["idx"])


def expected_rows(p):
    """R ∪ its 8 periodic (y,z) neighbours from a full (pz, py, px) PCM, as
    sorted row indices z*py + y: row maxima, dominant rows, d5, the rows
    with rowmax >= d5, one step of periodic dilation."""
    rowmax = p.max(axis=2)
    dom = rowmax > pc._wrap_neighbour_max(rowmax, (0, 1))
    assert dom.sum() >= 5
    d5 = np.sort(rowmax[dom])[::-1][4]
    in_r = rowmax >= d5
    mark = np.zeros_like(in_r)
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            mark |= np.roll(in_r, (dz, dy), axis=(0, 1))
    return np.flatnonzero(mark.ravel()), int(in_r.sum())


PAIRS = pytest.mark.parametrize("run", pc.PAIR_CASES, ids=pc.PAIR_IDS,
                                indirect=True)


@PAIRS
def test_mode_equality(run):
    gr, gf = run
    _assert_equal(gr, gf)
    assert gr["res"]["valid"]
    # no fallback, one prefilter interval, one timed inverse x pass each
    assert (gr["peak"], gr["peak_rows"], gr["x_inv"]) == (0, 1, 1)
    assert (gf["peak"], gf["peak_rows"], gf["x_inv"]) == (0, 1, 1)


@PAIRS
def test_row_set(run):
    gr, gf = run
    exp, n_r = expected_rows(gf["pcm"])
    assert 1 <= n_r <= pc.CAP // 4
    got = gr["rowlist"]
    assert len(np.unique(got)) == len(got)  # every row listed once
    assert np.array_equal(np.sort(got), exp)
    pz, py, px = gf["pcm"].shape
    raw = gr["raw"].reshape(pz * py, px)
    whole = gf["pcm"].reshape(pz * py, px)
    assert raw[exp].tobytes() == whole[exp].tobytes()
    assert len(gf["rowlist"]) == 0  # the full context lists nothing


@PAIRS
def test_rematerialise(run):
    gr, gf = run
    assert gr["pcm"].shape == gf["pcm"].shape
    assert gr["pcm"].tobytes() == gf["pcm"].tobytes()


def test_wrap(ctxs):
    a, b = pc.identical_pair()
    gr, gf = _run_pair(ctxs, a, b, (32, 32, 32), (3.0, -2.0, 1.0), 5)
    _assert_equal(gr, gf)
    assert gr["idx"][0] == 0  # the peak sits at linear index 0
    pz, py, _px = gf["pcm"].shape
    got = gr["rowlist"]
    assert np.array_equal(np.sort(got), expected_rows(gf["pcm"])[0])
    assert np.any(got % py == py - 1) and np.any(got // py == pz - 1)
    assert (pz - 1) * py + (py - 1) in got  # the corner neighbour of row 0
    assert gr["pcm"].tobytes() == gf["pcm"].tobytes()


def test_fallback(ctxs):
    rows, full = ctxs
    a = np.full((32, 32, 32), 777, np.uint16)
    _dirty(rows, (32, 32, 32), (3.0, -2.0, 1.0), 5)
    gr = _stitch(rows, a, a.copy())
    gf = _stitch(full, a, a.copy())
    _assert_equal(gr, gf)
    assert not gr["res"]["valid"] and not gf["res"]["valid"]
    # prefilter rejected -> the full inverse x pass, then ONE full scan
    assert (gr["peak"], gr["peak_rows"], gr["x_inv"]) == (1, 1, 2)
    assert (gf["peak"], gf["peak_rows"], gf["x_inv"]) == (1, 1, 1)
    assert rows.debug_pcm(raw=True).tobytes() == full.debug_pcm().tobytes()


def test_slots_and_epochs(ctxs):
    """Four distinct pairs in one batch use both pipeline slots twice; the
    second batch meets the first one's rows and stamps in every slot."""
    rows, full = ctxs
    shifts = [(57.3, 3.3, -2.6), (-55.5, 2.5, 1.5), (3.4, 56.6, -1.5),
              (2.5, -3.5, 57.25)]
    vols = [synth.make_pair((64, 64, 64), s, seed=21 + i)
            for i, s in enumerate(shifts)]
    pairs = [_pair_desc(vols[i][0], 2 * i, 2 * i + 1) for i in range(4)]
    out = {}
    for name, c in (("rows", rows), ("full", full)):
        for i, (a, b) in enumerate(vols):
            c.upload(2 * i, a)
            c.upload(2 * i + 1, b)
        out[name] = [c.stitch_batch(pairs, ds=(1, 1, 1),
                                    min_overlap_ratio=0.05)
                     for _ in range(2)]
    for batch in out["rows"]:
        for got, ref in zip(batch, out["full"][0]):
            assert got["valid"] == ref["valid"]
            assert got["shift"].tobytes() == ref["shift"].tobytes()
            assert (np.float64(got["r"]).tobytes() ==
                    np.float64(ref["r"]).tobytes())
    assert any(r["valid"] for r in out["full"][0])
    assert rows.debug_pcm().tobytes() == full.debug_pcm().tobytes()
