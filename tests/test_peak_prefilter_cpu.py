"""CPU check of the peak prefilter: a numpy restatement of
its five steps against oracle.phasecorr._local_maxima_topk, on float32
oracle PCMs of exactly the inputs test_gpu_peak_prefilter.py runs.

This is also where those inputs are justified: every pair whose GPU test
asserts "no fallback" must pass the prefilter on the oracle PCM with
margin (|L| >= 5 and |R| <= CAP/4), every fallback case must fail its
condition. A seed that misses the margin gets replaced, not the margin.
"""

import numpy as np
import pytest

from tests import peak_prefilter_cases as pc


def _check_exact(p, res):
    """Proof obligation: whenever |L| >= 5 the prefilter's top five ARE
    the oracle's, values bitwise and indices exactly."""
    ref = pc.oracle_top5(p)
    assert len(ref) == 5
    assert [i for _, i in res["top5"]] == [i for _, i in ref]
    assert [np.float32(v) for v, _ in res["top5"]] == \
        [np.float32(v) for v, _ in ref]


@pytest.mark.parametrize("case", pc.PAIR_CASES, ids=pc.PAIR_IDS)
def test_pair_passes_prefilter_with_margin(case):
    _name, _shape, _shift, _seed, ds, pad = case
    a, b = pc.make_pair_case(case)
    p = pc.oracle_pcm32(a, b, ds, pad)
    res = pc.prefilter(p)
    print(case[0], p.shape, {k: res[k] for k in ("ndom", "nR", "nL")})
    assert res["ndom"] >= 5
    assert res["nL"] >= 5
    assert res["nR"] <= pc.CAP // 4
    _check_exact(p, res)


def test_identical_tiles_peak_at_origin():
    a, b = pc.identical_pair()
    p = pc.oracle_pcm32(a, b)
    res = pc.prefilter(p)
    print("identical", {k: res[k] for k in ("ndom", "nR", "nL")})
    assert res["nL"] >= 5 and res["nR"] <= pc.CAP // 4
    assert res["top5"][0][1] == 0  # delta at linear index 0
    _check_exact(p, res)


KNOWN = pc.known_volumes()


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_known_volume_condition(name):
    vol, falls_back = KNOWN[name]
    res = pc.prefilter(vol)
    print(name, {k: res[k] for k in ("ndom", "nR", "nL")})
    assert res["ok"] == (not falls_back)
    if not falls_back:
        assert res["nR"] <= pc.CAP // 4
        _check_exact(vol, res)


def test_known_volume_stories():
    """The known answers say what their names claim."""
    top = {n: pc.oracle_top5(v) for n, (v, _) in KNOWN.items()}
    sh = KNOWN["equal_spikes"][0].shape
    spikes = np.flatnonzero(KNOWN["equal_spikes"][0])
    assert [i for _, i in top["equal_spikes"]] == list(spikes[:5])
    c0, c1 = 0, int(np.prod(sh)) - 1
    for n in ("corner_unequal", "corner_equal", "corner_equal_checked"):
        assert c0 not in [i for _, i in top[n]]
    assert c1 not in [i for _, i in top["corner_equal_checked"]]
    assert [i for _, i in top["corner_unequal_checked"]][3] == c1
    assert c0 not in [i for _, i in top["corner_unequal_checked"]]
    assert [v for v, _ in top["adjacent_tie"]] == [4.0, 3.0, 2.0, 1.0]
    assert len(top["three_spikes"]) == 3
    assert pc.prefilter(KNOWN["three_spikes"][0])["ndom"] == 3
    lat = pc.prefilter(KNOWN["even_lattice"][0])
    assert lat["nR"] == 1024 > pc.CAP and lat["nL"] == 1024 * 8
    assert [i for _, i in top["even_lattice"]] == [0, 2, 4, 6, 8]
    assert top["constant"] == []
    assert pc.prefilter(KNOWN["constant"][0])["ndom"] == 0
