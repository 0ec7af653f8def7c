"""CPU checks of the PCM path conformance cases (tests/pcm_cases.py): every
case pads to the dims it is named for (which is what sends it to its
kernel), the oracle's answer is usable for the comparisons the GPU test
makes, and the three metrics have teeth: a single wrong twiddle plane, or a
single stale row past the valid extent, raises at least one of them to 8x
what the float32 yardstick scores on the same case. The GPU test's bound K
is capped at 8 for that reason."""

import numpy as np
import pytest

from tests import pcm_cases as pc
from oracle import phasecorr

TEETH = 8.0

_CACHE = {}


@pytest.fixture
def cs(request):
    case = request.param
    name = case["name"]
    if name not in _CACHE:
        a, b = pc.oracle_inputs(case)
        ref = pc.Reference(a, b, case["pad_mode"])
        _CACHE[name] = dict(case=case, a=a, b=b, ref=ref,
                            m32=ref.metrics(pc.pcm32(a, b, case["pad_mode"])))
    return _CACHE[name]


ALL = pytest.mark.parametrize("cs", pc.CASES, ids=pc.IDS, indirect=True)
RAGGED = pytest.mark.parametrize(
    "cs", [c for c in pc.CASES if c["ragged"]],
    ids=[c["name"] for c in pc.CASES if c["ragged"]], indirect=True)


def test_case_table():
    """The paths the table is meant to reach, by padded dims."""
    pads = {c["name"]: c["pad"] for c in pc.CASES}
    assert {pads["x%d_full" % n][2] for n in (8, 16, 32, 64, 128, 256)} == \
        {8, 16, 32, 64, 128, 256}
    for n in (1, 2, 4, 8, 16, 32, 64, 128, 256, 1024):
        assert pads["y%d_full" % n][1] == n and pads["z%d_full" % n][0] == n
    for n in pc.FAST_SIZES:
        assert pads["fast_x%d" % n][2] == n
        assert pads["fast_y%d" % n][1] == n
        assert pads["fast_z%d" % n][0] == n
    assert max(int(np.prod(c["shape"])) for c in pc.CASES) <= 1024 * 16 * 32


@ALL
def test_padded_dims(cs):
    case, a, b = cs["case"], cs["a"], cs["b"]
    assert phasecorr.pad_shape(a.shape, b.shape, case["pad_mode"]) == \
        case["pad"] == cs["ref"].shape
    if case["ragged"]:  # zero-fill on the case's axis
        assert b.shape[case["axis"]] < case["pad"][case["axis"]]
    if case["nz_b"] is not None:
        assert a.shape[0] != b.shape[0]
    full = pc.make_case(case)[0]
    assert any(n % d for n, d in zip(full.shape[::-1], case["ds"])) or \
        case["ds"] == (1, 1, 1)


@ALL
def test_oracle_usable(cs):
    case = cs["case"]
    a, b, _ = pc.make_case(case)
    res = phasecorr.phase_correlation_shift(
        a, b, ds=case["ds"], pad_mode=case["pad_mode"])
    if pc.is_size1(case):
        assert not res["valid"]
        assert phasecorr._local_maxima_topk(cs["ref"].p64, 6) == []
        return
    assert res["valid"]
    gap = pc.top_gap(cs["ref"].p64)
    print("top-six gap %.3e" % gap)
    assert gap > 1e-4


def _assert_teeth(cs, faulty):
    m32, mf = cs["m32"], cs["ref"].metrics(faulty)
    ratios = [f / y for f, y in zip(mf, m32)]
    print("yardstick %s  fault %s  ratios %s" % (
        " ".join("%.2e" % v for v in m32), " ".join("%.2e" % v for v in mf),
        " ".join("%.1f" % r for r in ratios)))
    assert max(ratios) >= TEETH


@ALL
def test_teeth_plane_fault(cs):
    _assert_teeth(cs, pc.plane_fault_pcm(cs["ref"], pc.fault_axis(cs["case"])))


@RAGGED
def test_teeth_stale_row(cs):
    _assert_teeth(cs, pc.stale_row_pcm(cs["ref"], cs["a"], cs["b"],
                                       cs["case"]["axis"]))


def test_yardstick_is_float32_of_the_oracle():
    """pcm32 is the oracle's computation and nothing else: it agrees with the
    float64 PCM to float32 rounding."""
    case = pc.BY_NAME["x64_ragged"]
    a, b = pc.oracle_inputs(case)
    p64, shape = phasecorr.pcm(a, b)
    p32 = pc.pcm32(a, b)
    assert p32.shape == shape
    assert np.max(np.abs(p32 - p64)) < 1e-5
