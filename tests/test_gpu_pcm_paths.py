"""PCM path conformance: every FFT dispatch path of stitch_phaseA at PCM
level against the float64 oracle (DESIGN.md §4 "PCM path conformance").

One default context (no mode variables), the C ABI only: stitch_batch,
debug_pcm, debug_last_top5, debug_rowlist. The cases (tests/pcm_cases.py)
are the smallest pairs that reach each path: the shuffle and wave-resident x
passes at Px = 8..256, k_fft_pass at Py = 1..1024, the fused z kernels at
Pz = 1..1024, the mixed-radix kernels on each axis at sizes covering every
radix alone and combined, and k_downsample on its dword and scalar paths
away from offset 0. test_pcm_cases_cpu.py proves on the CPU that each case
pads to the dims it is named for.

The error bar is a plain float32 FFT of the same operation (pcm_cases.pcm32),
never another GPU kernel: for each of e_pcm = max |P - P64| and the max and
rms of the weighted spectrum error D (pcm_cases.Reference.metrics),
gpu <= K * yardstick. K is measured (below); it may never exceed 8, the
factor by which a single wrong twiddle plane or a single stale row is shown
to raise these metrics (test_pcm_cases_cpu.py).

K = 7: twice the largest ratio gpu / yardstick measured on MI355X over all
91 cases and the three metrics (3.32, rounded up; the factor 2 is for the
spread between seeds). Measured ratios, smallest to largest per group
(e_pcm / max D / rms D); profiles/pcm_paths_errors.md has every case:
  x pow2, Px 8..256      0.88-1.28 / 0.72-1.34 / 0.97-1.19
  y pow2, Py 1..1024     0.83-2.15 / 0.42-1.99 / 0.95-1.24
  z pow2, Pz 1..1024     0.82-1.31 / 0.58-2.89 / 0.92-1.46
  fast pad, 10..1000     0.94-1.77 / 0.55-3.32 / 0.98-1.51
  downsample             1.03-2.02 / 0.71-1.80 / 1.04-1.25
The largest are max D of fast_y70 (3.32), z2_full (2.89), fast_y210 (2.71)
and fast_x486 (2.48): single bins, the rms of the same cases is 1.0-1.5.
Every dirty run was byte-equal to its clean run. The padded sizes 1 (invalid,
like the oracle) and 2 on y and z sit inside these ranges."""

import numpy as np
import pytest

from oracle import phasecorr
from tests import pcm_cases as pc

pytestmark = pytest.mark.gpu

K_CAP = 8  # tied to the teeth check in test_pcm_cases_cpu.py
K = 7  # measured, see the docstring
assert K <= K_CAP

DIRTY = [c for c in pc.CASES if c["ragged"]]
MIXED = ("x64_ragged", "y128_ragged", "z256_unequal", "y2_full")


@pytest.fixture(scope="module")
def ctx():
    from bigstitcher_spark_amd import Context

    c = Context(0)
    yield c
    c.close()


def _stitch(c, desc):
    c.upload(0, desc["upload_a"])
    c.upload(1, desc["upload_b"])
    res = c.stitch_batch([desc["pair"]], ds=desc["ds"],
                         pad_mode=desc["pad_mode"])[0]
    v, idx = c.debug_last_top5()
    rows = c.debug_rowlist()
    return dict(res=res, v=v, idx=idx, rows=rows, pcm=c.debug_pcm())


_REF = {}
_CLEAN = {}


def _reference(case):
    """Oracle side of a case, computed once and left unchanged."""
    name = case["name"]
    if name not in _REF:
        a, b = pc.oracle_inputs(case)
        fa, fb, desc = pc.make_case(case)
        ref = pc.Reference(a, b, case["pad_mode"])
        ref.p64.setflags(write=False)
        _REF[name] = dict(
            desc=desc, ref=ref,
            m32=ref.metrics(pc.pcm32(a, b, case["pad_mode"])),
            res=phasecorr.phase_correlation_shift(
                fa, fb, ds=case["ds"], pad_mode=case["pad_mode"]),
            top5=[int(np.ravel_multi_index(pk, ref.shape)) for _v, pk in
                  phasecorr._local_maxima_topk(ref.p64, 5)])
    return _REF[name]


def _clean(ctx, case):
    """The first run of a case in the module's context."""
    if case["name"] not in _CLEAN:
        _CLEAN[case["name"]] = _stitch(ctx, _reference(case)["desc"])
    return _CLEAN[case["name"]]


def _check(case, got, tag):
    o = _reference(case)
    ref, m32 = o["ref"], o["m32"]
    assert got["pcm"].shape == ref.shape == case["pad"]
    mg = ref.metrics(got["pcm"])
    print("PCMPATH %s %s  gpu %s  f32 %s  ratio %s" % (
        tag, case["name"], " ".join("%.3e" % v for v in mg),
        " ".join("%.3e" % v for v in m32),
        " ".join("%.2f" % (g / y) for g, y in zip(mg, m32))))
    for name, g, y in zip(pc.METRIC_NAMES, mg, m32):
        assert g <= K * y, (name, g, y, g / y)
    res = got["res"]
    assert res["valid"] == o["res"]["valid"]
    assert len(set(got["rows"].tolist())) == len(got["rows"])
    nrows = ref.shape[0] * ref.shape[1]
    assert all(0 <= r < nrows for r in got["rows"].tolist())
    if not res["valid"]:
        assert pc.is_size1(case)  # the only invalid cases of the table
        return
    assert np.all(np.abs(res["shift"] - o["res"]["shift"]) < 1e-3), (
        res["shift"], o["res"]["shift"])
    assert abs(res["r"] - o["res"]["r"]) < 1e-9
    found = [int(i) for v, i in zip(got["v"], got["idx"]) if v > -2.0e38]
    assert found == o["top5"]


@pytest.mark.parametrize("case", pc.CASES, ids=pc.IDS)
def test_path(ctx, case):
    _check(case, _clean(ctx, case), "clean")


@pytest.mark.parametrize("case", DIRTY, ids=[c["name"] for c in DIRTY])
def test_dirty(ctx, case):
    """The case again, right after a full-extent pair of the same padded
    dims: every row and plane past `valid` now holds that pair's spectrum,
    which the zero-fill guards must mask. Same bounds, and the PCM is
    byte-equal to the first run's."""
    clean = _clean(ctx, case)
    da, db = pc.dirty_pair(case)
    ctx.upload(0, da)
    ctx.upload(1, db)
    full = dict(view_a=0, view_b=1, off_a=(0, 0, 0), size_a=da.shape[::-1],
                off_b=(0, 0, 0), size_b=db.shape[::-1])
    ctx.stitch_batch([full], ds=(1, 1, 1), pad_mode=case["pad_mode"])
    assert ctx.debug_pcm().shape == case["pad"]  # same buffers, same layout
    got = _stitch(ctx, _reference(case)["desc"])
    _check(case, got, "dirty")
    assert got["pcm"].tobytes() == clean["pcm"].tobytes()
    assert got["res"]["shift"].tobytes() == clean["res"]["shift"].tobytes()
    assert np.array_equal(got["idx"], clean["idx"])


def test_mixed_batch(ctx):
    """Four pairs of four different padded dims in one call, twice: the
    slots reuse their buffers across dims, and every result equals the same
    pair stitched alone."""
    cases = [pc.BY_NAME[n] for n in MIXED]
    assert len({c["pad"] for c in cases}) == len(cases)
    alone = [_clean(ctx, c)["res"] for c in cases]
    pairs = []
    for i, c in enumerate(cases):
        desc = _reference(c)["desc"]
        assert desc["ds"] == (1, 1, 1) and desc["pad_mode"] == "pow2"
        ctx.upload(10 + 2 * i, desc["upload_a"])
        ctx.upload(11 + 2 * i, desc["upload_b"])
        pairs.append(dict(desc["pair"], view_a=10 + 2 * i,
                          view_b=11 + 2 * i))
    try:
        for _ in range(2):
            got = ctx.stitch_batch(pairs, ds=(1, 1, 1))
            for g, s, c in zip(got, alone, cases):
                assert g["valid"] == s["valid"], c["name"]
                assert g["shift"].tobytes() == s["shift"].tobytes(), c["name"]
                assert (np.float64(g["r"]).tobytes() ==
                        np.float64(s["r"]).tobytes()), c["name"]
    finally:
        for i in range(2 * len(cases)):
            ctx.release(10 + i)


def test_px_below_8_refused(ctx):
    """The one size limit below 1024 (include/bigstitch.h): a padded x size
    under 8 is a clean BS_EUNSUP for the batch, and the context stays
    usable."""
    case = pc.BY_NAME["x8_ragged"]
    a, b, _ = pc.make_case(case)
    ctx.upload(0, a[:, :, :4])
    ctx.upload(1, b[:, :, :4])
    pair = dict(view_a=0, view_b=1, off_a=(0, 0, 0), size_a=(4, 10, 6),
                off_b=(0, 0, 0), size_b=(4, 10, 6))
    with pytest.raises(RuntimeError, match="rc=-6"):
        ctx.stitch_batch([pair], ds=(1, 1, 1))
    got = _stitch(ctx, _reference(case)["desc"])
    assert got["pcm"].tobytes() == _clean(ctx, case)["pcm"].tobytes()
