"""Shared inputs of the peak-prefilter tests (CPU restatement and GPU).

The stitch path finds the PCM's top five strict local maxima from the
row maxima the inverse x pass emits (DESIGN.md §4 "peak prefilter") and
falls back to the full-volume scan when the prefilter cannot prove its
answer. Both test files use exactly the inputs defined here:
test_peak_prefilter_cpu.py justifies them (margins on the oracle PCM),
test_gpu_peak_prefilter.py runs them through the library.
"""

from __future__ import annotations

import numpy as np

from oracle import phasecorr, synth

CAP = 512  # BS_PEAK_ROWS_CAP in csrc/bigstitch.hip (cost guard on |R|)

SENT_V = np.float32(-3.0e38)  # the scan's "no peak" entry
SENT_I = np.int64(0x7FFFFFFFFFFFFFFF)


# ---------------------------------------------------------------- restatement

def _wrap_neighbour_max(a, axes):
    """max over the 3^len(axes) - 1 periodic neighbours along `axes`."""
    m = np.full(a.shape, -np.inf, a.dtype)
    offs = np.array(np.meshgrid(*[[-1, 0, 1]] * len(axes))).reshape(
        len(axes), -1).T
    for off in offs:
        if not off.any():
            continue
        m = np.maximum(m, np.roll(a, tuple(off), axis=axes))
    return m


def prefilter(p: np.ndarray, cap: int = CAP):
    """Steps 1-5 of the prefilter on a float32 (pz, py, px) volume.

    Returns dict(ndom, nR, nL, ok, top5) with top5 = list of
    (value, linear index) under (value desc, index asc), or None when
    fewer than five rows are dominant."""
    p = np.asarray(p, np.float32)
    pz, py, px = p.shape
    rowmax = p.max(axis=2)
    dom = rowmax > _wrap_neighbour_max(rowmax, (0, 1))
    ndom = int(dom.sum())
    if ndom < 5:
        return dict(ndom=ndom, nR=0, nL=0, ok=False, top5=None)
    d5 = np.sort(rowmax[dom])[::-1][4]
    rows = np.argwhere(rowmax >= d5)
    found = []
    for z, y in rows:
        for x in np.flatnonzero(p[z, y] >= d5):
            v = p[z, y, x]
            strict = True
            for dz in (-1, 0, 1):
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        if dz == dy == dx == 0:
                            continue
                        n = p[(z + dz) % pz, (y + dy) % py, (x + dx) % px]
                        strict = strict and bool(v > n)
            if strict:
                found.append((float(v), int((z * py + y) * px + x)))
    found.sort(key=lambda t: (-t[0], t[1]))
    nR, nL = len(rows), len(found)
    return dict(ndom=ndom, nR=nR, nL=nL, ok=nL >= 5 and nR <= cap,
                top5=found[:5])


def oracle_top5(p: np.ndarray):
    """oracle.phasecorr._local_maxima_topk as [(value, linear index)]."""
    p = np.asarray(p, np.float32)
    return [(v, int(np.ravel_multi_index(pos, p.shape)))
            for v, pos in phasecorr._local_maxima_topk(p, 5)]


def padded_top5(top):
    """Top-five list -> (values float32[5], indices int64[5]) padded with
    the scan's sentinels, the layout the library reports."""
    v = np.full(5, SENT_V, np.float32)
    i = np.full(5, SENT_I, np.int64)
    for k, (val, idx) in enumerate(top[:5]):
        v[k], i[k] = val, idx
    return v, i


# ------------------------------------------------------- end-to-end pair cases
# (name, shape (nz,ny,nx), true shift (x,y,z), seed, ds, pad_mode). The
# shift puts ~10% of the x extent in overlap. Seeds were picked so that
# the oracle PCM passes the prefilter with margin (|L| >= 5,
# |R| <= CAP/4): test_peak_prefilter_cpu.py asserts exactly that.

PAIR_CASES = [
    ("lds64", (64, 64, 64), (57.3, 3.3, -2.6), 11, (1, 1, 1), "pow2"),
    ("waveE1", (32, 32, 128), (115.4, -3.5, 2.25), 11, (1, 1, 1), "pow2"),
    ("waveE2", (16, 16, 256), (230.6, 2.5, -1.25), 11, (1, 1, 1), "pow2"),
    ("waveE4", (8, 8, 512), (460.7, 1.5, -1.25), 17, (1, 1, 1), "pow2"),
    ("waveE8", (8, 8, 1024), (921.4, -1.5, 1.25), 13, (1, 1, 1), "pow2"),
    ("ragged", (40, 50, 60), (54.3, -2.5, 1.75), 11, (1, 1, 1), "pow2"),
    ("fast48", (48, 48, 48), (43.4, 2.5, -1.5), 11, (1, 1, 1), "fast"),
    ("fast50", (50, 50, 50), (45.3, -2.5, 1.5), 11, (1, 1, 1), "fast"),
    ("ds221", (64, 64, 64), (57.5, 3.0, -2.0), 11, (2, 2, 1), "pow2"),
]
PAIR_IDS = [c[0] for c in PAIR_CASES]


def make_pair_case(case):
    _name, shape, shift, seed, _ds, _pad = case
    return synth.make_pair(shape, shift, seed=seed)


def identical_pair():
    """Two identical 32^3 tiles: the PCM is a delta at linear index 0, so
    the winning row and its neighbours wrap in all three axes."""
    a, _ = synth.make_pair((32, 32, 32), (0.0, 0.0, 0.0), seed=5)
    return a, a.copy()


def oracle_pcm32(a, b, ds=(1, 1, 1), pad_mode="pow2"):
    p, _ = phasecorr.pcm(phasecorr.downsample(a, ds),
                         phasecorr.downsample(b, ds), pad_mode=pad_mode)
    return p.astype(np.float32)


# --------------------------------------------------------- known-answer volumes
# name -> (volume float32 (pz,py,px), falls_back)

def _spikes(shape, spikes):
    v = np.zeros(shape, np.float32)
    for pos, val in spikes:
        v[pos] = val
    return v


def known_volumes():
    out = {}
    sh = (16, 16, 32)
    out["random"] = (
        np.random.default_rng(7).random(sh, dtype=np.float32), False)
    iso = [(2, 2, 3), (1, 5, 30), (4, 9, 0), (7, 3, 31), (9, 12, 16),
           (12, 6, 7), (14, 14, 20), (4, 2, 11)]
    # eight equal isolated spikes: the five lowest linear indices win
    out["equal_spikes"] = (_spikes(sh, [(p, 1.0) for p in iso]), False)
    big5 = [(iso[k], 5.0 + k) for k in range(5)]
    c0, c1 = (0, 0, 0), (sh[0] - 1, sh[1] - 1, sh[2] - 1)  # wrap neighbours
    # the issue's corner cases: five larger spikes make up the top five
    out["corner_unequal"] = (
        _spikes(sh, [(c0, 2.0), (c1, 3.0)] + big5), False)
    out["corner_equal"] = (
        _spikes(sh, [(c0, 3.0), (c1, 3.0)] + big5), False)
    # sharper variants: d5 lies BELOW the corner values, so the row check
    # itself must reject the non-strict corner(s) through the wrap
    out["corner_unequal_checked"] = (
        _spikes(sh, [(c0, 2.0), (c1, 3.0), (iso[0], 7.0), (iso[1], 6.0),
                     (iso[2], 5.0), (iso[3], 1.0)]), False)
    out["corner_equal_checked"] = (
        _spikes(sh, [(c0, 3.0), (c1, 3.0), (iso[0], 7.0), (iso[1], 6.0),
                     (iso[2], 5.0), (iso[3], 1.0), (iso[4], 0.5)]), False)
    # global top = two equal x-adjacent values (neither strict) + 4 lower
    out["adjacent_tie"] = (
        _spikes(sh, [((4, 4, 10), 9.0), ((4, 4, 11), 9.0)] +
                [(iso[k + 3], 1.0 + k) for k in range(4)]), True)
    out["three_spikes"] = (
        _spikes(sh, [(iso[0], 3.0), (iso[1], 2.0), (iso[2], 1.0)]), True)
    # value 1 at every even (x,y,z) of 16 x 64 x 64 (px,py,pz): every one
    # is a strict maximum, |R| = 32*32 = 1024 rows of 4096 > CAP
    lat = np.zeros((64, 64, 16), np.float32)
    lat[::2, ::2, ::2] = 1.0
    out["even_lattice"] = (lat, True)
    out["constant"] = (np.full(sh, 0.25, np.float32), True)
    return out
