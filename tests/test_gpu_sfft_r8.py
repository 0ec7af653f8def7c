"""GPU tests of the radix-8 strided FFT passes at n = 512 (DESIGN.md §4
"y and fused-z passes: radix-8 register stages", BS_SFFT_MODE=r8:
k_fft_pass_r8 and k_fft_z_fused_r8x) against the in-LDS radix-2^2 kernels
(BS_SFFT_MODE=lds, the parent's passes, unchanged in the file) and the CPU
oracle. ds = (1, 1, 1); the x extent is small so that a case costs seconds:
Cx = 17 or 9 still gives full chunks of 8 columns and a last chunk of one.

The error bar is the parent's kernel measured in the same test: with
e_mode = max |debug_pcm(mode) - oracle pcm|, e_r8 <= 2 * e_lds (a different
rounding order and nothing else), after the precondition that the oracle's
smallest gap among the top six PCM maxima exceeds 100 * e_lds, so rounding
cannot reorder the peaks the modes must agree on. Seeds were picked on the
CPU so that this gap is above 1e-4.

Measured on MI355X (e_lds / e_r8): y_only 1.55e-7 / 1.50e-7, z_only
1.09e-7 / 9.5e-8, both_zero_fill 7.2e-8 / 5.6e-8, odd_extents 7.21e-8 /
7.21e-8, unequal_z 8.8e-8 / 8.9e-8; the top-six gaps are 2.5e-4 to 2.3e-3."""

import os

import numpy as np
import pytest

from oracle import phasecorr, synth

pytestmark = pytest.mark.gpu

# name, shape of a (nz, ny, nx), nz of b (None: as a), shift (x, y, z), seed
CASES = [
    ("y_only", (24, 512, 24), None, (2.25, 37.5, -1.5), 23),
    ("z_only", (512, 24, 24), None, (-2.5, 1.75, 41.25), 28),
    ("both_zero_fill", (300, 400, 20), None, (1.5, -21.25, 17.5), 30),
    ("odd_extents", (511, 257, 12), None, (1.25, 9.5, -30.75), 23),
    ("unequal_z", (300, 24, 24), 280, (2.0, -1.5, 12.25), 23),
]
IDS = [c[0] for c in CASES]


def _make_ctx(mode):
    from bigstitcher_spark_amd import Context

    old = os.environ.get("BS_SFFT_MODE")
    os.environ["BS_SFFT_MODE"] = mode  # read once, in bs_ctx_create
    try:
        return Context(0)
    finally:
        if old is None:
            del os.environ["BS_SFFT_MODE"]
        else:
            os.environ["BS_SFFT_MODE"] = old


@pytest.fixture(scope="module")
def ctxs():
    r8, lds = _make_ctx("r8"), _make_ctx("lds")
    yield r8, lds
    r8.close()
    lds.close()


def _stitch(c, a, b, pad_mode="pow2"):
    c.upload(0, a)
    c.upload(1, b)
    pair = dict(view_a=0, view_b=1, off_a=(0, 0, 0), size_a=a.shape[::-1],
                off_b=(0, 0, 0), size_b=b.shape[::-1])
    res = c.stitch_batch([pair], ds=(1, 1, 1), pad_mode=pad_mode)[0]
    v, idx = c.debug_last_top5()
    return dict(res=res, v=v, idx=idx, pcm=c.debug_pcm())


def make_case(case):
    """The pair of a case (CPU only; also used to pick the seeds)."""
    _name, shape, nz_b, shift, seed = case
    a, b = synth.make_pair(shape, shift, seed=seed)
    if nz_b is not None:
        b = np.ascontiguousarray(b[:nz_b])
    return a, b


def top6_gap(p):
    top6 = np.array([v for v, _ in phasecorr._local_maxima_topk(p, 6)])
    return float(np.min(-np.diff(top6)))


_CACHE = {}


@pytest.fixture
def run(ctxs, request):
    """Each case runs once: oracle, r8 context, lds context."""
    name = request.param[0]
    if name not in _CACHE:
        a, b = make_case(request.param)
        p, _ = phasecorr.pcm(a, b)
        _CACHE[name] = dict(
            ref=phasecorr.phase_correlation_shift(a, b, ds=(1, 1, 1)),
            p=p, gap=top6_gap(p),
            r8=_stitch(ctxs[0], a, b), lds=_stitch(ctxs[1], a, b))
    return _CACHE[name]


ALL = pytest.mark.parametrize("run", CASES, ids=IDS, indirect=True)


@ALL
def test_against_oracle(run):
    ref = run["ref"]
    assert ref["valid"]
    for mode in ("r8", "lds"):
        got = run[mode]["res"]
        assert got["valid"] == ref["valid"], mode
        assert np.all(np.abs(got["shift"] - ref["shift"]) < 1e-3), (
            mode, got["shift"], ref["shift"])


@ALL
def test_modes_agree(run):
    r8, lds = run["r8"], run["lds"]
    assert r8["res"]["valid"] == lds["res"]["valid"]
    assert (np.float64(r8["res"]["r"]).tobytes() ==
            np.float64(lds["res"]["r"]).tobytes())
    assert np.array_equal(r8["idx"], lds["idx"])


@ALL
def test_pcm_error(run):
    p = run["p"]
    assert run["r8"]["pcm"].shape == p.shape == run["lds"]["pcm"].shape
    e_lds = float(np.max(np.abs(run["lds"]["pcm"] - p)))
    e_r8 = float(np.max(np.abs(run["r8"]["pcm"] - p)))
    print("e_lds %.3e  e_r8 %.3e  top-six gap %.3e" % (e_lds, e_r8,
                                                        run["gap"]))
    assert run["gap"] > 1e-4  # how the seeds were picked
    assert run["gap"] > 100.0 * e_lds  # precondition: peaks cannot reorder
    assert e_r8 <= 2.0 * e_lds


def test_fast_pad_untouched(ctxs):
    """pad_mode="fast" at Py = Pz = 300 runs the mixed-radix kernels in both
    modes: byte-equal results."""
    shape, shift = (300, 300, 20), (1.5, -12.25, 9.5)
    a, b = synth.make_pair(shape, shift, seed=23)
    r8 = _stitch(ctxs[0], a, b, pad_mode="fast")
    lds = _stitch(ctxs[1], a, b, pad_mode="fast")
    assert r8["pcm"].shape[:2] == (300, 300)
    assert r8["res"]["valid"] and lds["res"]["valid"]
    assert r8["res"]["shift"].tobytes() == lds["res"]["shift"].tobytes()
    assert (np.float64(r8["res"]["r"]).tobytes() ==
            np.float64(lds["res"]["r"]).tobytes())
    assert r8["v"].tobytes() == lds["v"].tobytes()
    assert np.array_equal(r8["idx"], lds["idx"])
    assert r8["pcm"].tobytes() == lds["pcm"].tobytes()
