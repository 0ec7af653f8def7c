"""GPU tests of the peak prefilter: the top five PCM
maxima found from the inverse x pass's row maxima must be exactly the
full scan's — end to end against a BS_PEAK_MODE=full context, and on
known volumes through bs_debug_peak_scan against the oracle's
_local_maxima_topk. Inputs and their justification:
tests/peak_prefilter_cases.py and tests/test_peak_prefilter_cpu.py."""

import os

import numpy as np
import pytest

from tests import peak_prefilter_cases as pc

pytestmark = pytest.mark.gpu


def _make_ctx(mode):
    from bigstitcher_spark_amd import Context

    old = os.environ.get("BS_PEAK_MODE")
    os.environ["BS_PEAK_MODE"] = mode  # read once, in bs_ctx_create
    try:
        return Context(0)
    finally:
        if old is None:
            del os.environ["BS_PEAK_MODE"]
        else:
            os.environ["BS_PEAK_MODE"] = old


@pytest.fixture(scope="module")
def ctxs():
    auto, full = _make_ctx("auto"), _make_ctx("full")
    yield auto, full
    auto.close()
    full.close()


def _run_both(ctxs, a, b, ds=(1, 1, 1), pad_mode="pow2"):
    """One pair through both contexts -> [(result, top5 v, top5 idx,
    peak launches, peak_rows launches)] for (auto, full)."""
    nz, ny, nx = a.shape
    pair = dict(view_a=0, view_b=1, off_a=(0, 0, 0), size_a=(nx, ny, nz),
                off_b=(0, 0, 0), size_b=(nx, ny, nz))
    out = []
    for c in ctxs:
        c.upload(0, a)
        c.upload(1, b)
        c.reset_stats()
        res = c.stitch_batch([pair], ds=ds, pad_mode=pad_mode,
                             min_overlap_ratio=0.05)[0]
        v, idx = c.debug_last_top5()
        k = c.stats()["kernels"]
        out.append((res, v, idx, k["peak"]["launches"],
                    k["peak_rows"]["launches"]))
    return out


def _assert_modes_equal(got_auto, got_full):
    ra, va, ia, _, _ = got_auto
    rf, vf, i_f, _, _ = got_full
    assert ra["valid"] == rf["valid"]
    assert ra["shift"].tobytes() == rf["shift"].tobytes()
    assert np.float64(ra["r"]).tobytes() == np.float64(rf["r"]).tobytes()
    assert va.tobytes() == vf.tobytes()
    assert np.array_equal(ia, i_f)


@pytest.mark.parametrize("case", pc.PAIR_CASES, ids=pc.PAIR_IDS)
def test_mode_equality(ctxs, case):
    _name, _shape, _shift, _seed, ds, pad = case
    a, b = pc.make_pair_case(case)
    ga, gf = _run_both(ctxs, a, b, ds, pad)
    _assert_modes_equal(ga, gf)
    assert ga[3] == 0 and ga[4] == 1  # no fallback; prefilter ran
    assert gf[3] == 1 and gf[4] == 0  # the full context never prefilters


def test_mode_equality_identical_tiles(ctxs):
    a, b = pc.identical_pair()
    ga, gf = _run_both(ctxs, a, b)
    _assert_modes_equal(ga, gf)
    assert ga[3] == 0 and ga[4] == 1
    assert ga[2][0] == 0  # the peak sits at linear index 0
    assert ga[0]["valid"] and np.all(np.abs(ga[0]["shift"]) < 1e-3)


def test_constant_tiles_fall_back(ctxs):
    a = np.full((32, 32, 32), 777, np.uint16)
    ga, gf = _run_both(ctxs, a, a.copy())
    _assert_modes_equal(ga, gf)
    assert not ga[0]["valid"] and not gf[0]["valid"]
    assert ga[3] == 1 and ga[4] == 1  # prefilter ran, then ONE full scan


KNOWN = pc.known_volumes()


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_known_answers(ctxs, name):
    vol, falls_back = KNOWN[name]
    ev, ei = pc.padded_top5(pc.oracle_top5(vol))
    for c in ctxs:  # auto path on both contexts: the mode is an argument
        v, idx, fb = c.debug_peak_scan(vol, "auto")
        assert fb == falls_back
        assert v.tobytes() == ev.tobytes()
        assert np.array_equal(idx, ei)
    v, idx, fb = ctxs[0].debug_peak_scan(vol, "full")
    assert not fb
    assert v.tobytes() == ev.tobytes() and np.array_equal(idx, ei)
