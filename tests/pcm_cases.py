"""Cases, yardstick and metrics of the PCM path conformance tests
(test_pcm_cases_cpu.py, test_gpu_pcm_paths.py). CPU only.

Every case is the smallest pair that still reaches one FFT dispatch path of
stitch_phaseA (DESIGN.md §4 "PCM path conformance"): the padded dims decide
the kernel, so each case records the padded dims it is named for and the CPU
test checks them against oracle.phasecorr.pad_shape.

The yardstick pcm32 is the oracle's computation carried out in float32 with
scipy.fft: a plain float32 FFT of the same operation, not the code under
test. A GPU path is held to K times the yardstick's own error against the
float64 oracle, on three metrics (see `metrics`)."""

import functools

import numpy as np
from scipy import fft as sfft

from oracle import phasecorr, synth

Z, Y, X = 0, 1, 2  # axis numbers of a (nz, ny, nx) volume

FAST_SIZES = (10, 12, 14, 18, 30, 42, 70, 98, 210, 250, 486, 1000)

# Seeds other than DEFAULT_SEED, picked on the CPU (test_pcm_cases_cpu.py
# states the conditions: oracle valid, top-six gap > 1e-4, teeth >= 8x).
DEFAULT_SEED = 23
SEEDS = {"y32_full": 24, "y128_ragged": 25, "z128_full": 24,
         "z1024_unequal": 25, "fast_z486": 24}


def _fast_extent(size):
    """Smallest extent that pad_mode="fast" still pads to `size`: one more
    than the even 7-smooth size below it, so the zero-fill is as long as the
    size allows (and the extent is odd)."""
    n = size - 1
    while n > 8 and phasecorr._next_fast_even(n - 1) == size:
        n -= 1
    return n


def _axis_shift(n):
    """Shift along the axis under test, in px: a sub-pixel part always, and
    an integer part that grows with the size but keeps most of the overlap."""
    if n < 8:
        return 0.25
    return float(min(n // 8, 37)) + 0.25


def _case(name, shape, shift, pad, axis, ragged=False, nz_b=None,
          pad_mode="pow2", ds=(1, 1, 1), upload=None, off=(0, 0, 0)):
    return dict(name=name, shape=tuple(shape), shift=tuple(shift),
                pad=tuple(pad), axis=axis, ragged=ragged, nz_b=nz_b,
                pad_mode=pad_mode, ds=tuple(ds), upload=upload,
                off=tuple(off), seed=SEEDS.get(name, DEFAULT_SEED))


def _build_cases():
    cs = []
    # x, pow2: the other axes (6, 10) pad to (8, 16)
    for px in (8, 16, 32, 64, 128, 256):
        sx = _axis_shift(px)
        cs.append(_case("x%d_full" % px, (6, 10, px), (sx, -1.5, 1.0),
                        (8, 16, px), X))
        nx = 5 if px == 8 else px - 3
        cs.append(_case("x%d_ragged" % px, (6, 10, nx), (sx, -1.5, 1.0),
                        (8, 16, px), X, ragged=True))
    for px in (64, 256):  # rows start 2 bytes past a 4-byte boundary
        cs.append(_case("x%d_crop_unaligned" % px, (6, 10, px - 3),
                        (_axis_shift(px), -1.5, 1.0), (8, 16, px), X,
                        ragged=True, upload=(6, 10, px), off=(1, 0, 0)))
    # y, pow2: nx = 24 -> Cx = 17, two full chunks of 8 columns and one of 1
    for py in (1, 2, 4, 8, 16, 32, 64, 128, 256, 1024):
        sy = 0.0 if py == 1 else _axis_shift(py)
        cs.append(_case("y%d_full" % py, (6, py, 24), (2.25, sy, 1.0),
                        (8, py, 32), Y))
        if py >= 8:
            cs.append(_case("y%d_ragged" % py, (6, py - 3, 24),
                            (2.25, sy, 1.0), (8, py, 32), Y, ragged=True))
    # z, pow2
    for pz in (1, 2, 4, 8, 16, 32, 64, 128, 256, 1024):
        sz = 0.0 if pz == 1 else _axis_shift(pz)
        cs.append(_case("z%d_full" % pz, (pz, 10, 24), (2.25, -1.5, sz),
                        (pz, 16, 32), Z))
        if pz in (8, 128, 256, 1024):
            cs.append(_case("z%d_ragged" % pz, (pz - 3, 10, 24),
                            (2.25, -1.5, sz), (pz, 16, 32), Z, ragged=True))
            cs.append(_case("z%d_unequal" % pz, (pz - 2, 10, 24),
                            (2.25, -1.5, sz), (pz, 16, 32), Z, ragged=True,
                            nz_b=max(pz - 7, pz // 2 + 1)))
    # fast pad: each size on each axis, the other two small and non-pow2
    # ((9, 11, 19) pad to (10, 12, 20)); extents just below the size
    for n in FAST_SIZES:
        e, s = _fast_extent(n), _axis_shift(n)
        cs.append(_case("fast_x%d" % n, (9, 11, e), (s, -1.5, 1.0),
                        (10, 12, n), X, ragged=True, pad_mode="fast"))
        cs.append(_case("fast_y%d" % n, (9, e, 19), (2.25, s, 1.0),
                        (10, n, 20), Y, ragged=True, pad_mode="fast"))
        cs.append(_case("fast_z%d" % n, (e, 11, 19), (2.25, -1.5, s),
                        (n, 12, 20), Z, ragged=True, pad_mode="fast"))
    # pow2 y (k_fft_pass) between two mixed-radix axes
    cs.append(_case("fast_mixed", (45, 64, 50), (4.25, -6.5, 3.0),
                    (48, 64, 50), Y, pad_mode="fast"))
    cs.append(_case("fast_z30_unequal", (29, 11, 19), (2.25, -1.5, 3.25),
                    (30, 12, 20), Z, ragged=True, nz_b=25, pad_mode="fast"))
    # downsample: regions inside larger uploads, no extent a multiple of ds.
    # `pad` is the padded size of the DOWNSAMPLED pair.
    cs.append(_case("ds221_even", (9, 21, 67), (8.5, -3.0, 1.0), (16, 16, 64),
                    Y, ragged=True, ds=(2, 2, 1), upload=(11, 24, 72),
                    off=(2, 1, 1)))  # even x offset: dword loads
    cs.append(_case("ds221_odd", (9, 21, 67), (8.5, -3.0, 1.0), (16, 16, 64),
                    Y, ragged=True, ds=(2, 2, 1), upload=(11, 24, 72),
                    off=(3, 1, 1)))  # odd x offset: scalar loads
    cs.append(_case("ds442", (13, 30, 70), (9.0, -6.0, 2.0), (8, 8, 32),
                    Y, ragged=True, ds=(4, 4, 2), upload=(15, 33, 76),
                    off=(2, 1, 1)))
    cs.append(_case("ds112", (13, 10, 24), (2.25, -1.5, 2.5), (8, 16, 32),
                    Z, ragged=True, ds=(1, 1, 2), upload=(15, 12, 28),
                    off=(3, 1, 1)))
    return cs


CASES = _build_cases()
IDS = [c["name"] for c in CASES]
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def is_size1(case):
    """A padded size of 1 on y or z: the oracle finds no strict maximum
    (a voxel is its own periodic neighbour), so the pair is invalid."""
    return 1 in case["pad"][:2]


@functools.lru_cache(maxsize=None)
def _pair(shape, shift, seed):
    a, b = synth.make_pair(shape, shift, seed=seed)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def make_case(case):
    """(a, b, desc): the two full-resolution regions (nz, ny, nx) uint16 and
    what the C ABI needs to stitch them: desc = dict(upload_a, upload_b, pair
    (the bs_pair_desc fields for views 0 and 1), ds, pad_mode)."""
    a, b = _pair(case["shape"], case["shift"], case["seed"])
    if case["nz_b"] is not None:
        b = np.ascontiguousarray(b[:case["nz_b"]])
    ua, ub = a, b
    if case["upload"] is not None:
        ox, oy, oz = case["off"]
        ua = np.full(case["upload"], 40000, np.uint16)
        ub = np.full(case["upload"], 50000, np.uint16)
        ua[oz:oz + a.shape[0], oy:oy + a.shape[1], ox:ox + a.shape[2]] = a
        ub[oz:oz + b.shape[0], oy:oy + b.shape[1], ox:ox + b.shape[2]] = b
    pair = dict(view_a=0, view_b=1, off_a=case["off"], size_a=a.shape[::-1],
                off_b=case["off"], size_b=b.shape[::-1])
    return a, b, dict(upload_a=ua, upload_b=ub, pair=pair, ds=case["ds"],
                      pad_mode=case["pad_mode"])


def oracle_inputs(case):
    """The pair the FFT sees: the regions after [PIN-DS]."""
    a, b, _ = make_case(case)
    return phasecorr.downsample(a, case["ds"]), \
        phasecorr.downsample(b, case["ds"])


def dirty_pair(case):
    """A full-extent pair of the case's padded dims from another seed, to be
    stitched with ds = (1, 1, 1) just before the case: it leaves its spectrum
    in every row and plane the case does not write."""
    rng = np.random.default_rng(case["seed"] + 1000)
    a = rng.integers(90, 3000, size=case["pad"]).astype(np.uint16)
    b = np.roll(a, (1, 2, 3), axis=(0, 1, 2))
    b = (b + rng.integers(0, 21, size=case["pad"])).astype(np.uint16)
    return a, b


# ---- yardstick and metrics ----

def pcm32(a, b, pad_mode="pow2"):
    """oracle.phasecorr.pcm in float32 (scipy.fft keeps the precision of its
    input): returns the float32 PCM of the padded shape."""
    shape = phasecorr.pad_shape(a.shape, b.shape, pad_mode)
    fa = sfft.rfftn(a.astype(np.float32), s=shape, axes=(0, 1, 2))
    fb = sfft.rfftn(b.astype(np.float32), s=shape, axes=(0, 1, 2))
    assert fa.dtype == np.complex64 and fb.dtype == np.complex64
    q = np.conj(fa) * fb
    mag = np.abs(q)
    assert q.dtype == np.complex64 and mag.dtype == np.float32
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(mag < np.float32(1e-20), np.complex64(0), q / mag)
    assert q.dtype == np.complex64
    p = sfft.irfftn(q, s=shape, axes=(0, 1, 2))
    assert p.dtype == np.float32 and p.shape == shape
    return p


def _cross_power(fa, fb):
    q = np.conj(fa) * fb
    mag = np.abs(q)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(mag < 1e-20, 0.0, q / mag)


class Reference:
    """The float64 quantities every metric is taken against."""

    def __init__(self, a, b, pad_mode="pow2"):
        self.pad_mode = pad_mode
        self.p64, self.shape = phasecorr.pcm(a, b, pad_mode=pad_mode)
        self.fa = np.fft.rfftn(a, s=self.shape, axes=(0, 1, 2))
        self.fb = np.fft.rfftn(b, s=self.shape, axes=(0, 1, 2))
        self.q64 = _cross_power(self.fa, self.fb)
        m = np.minimum(np.abs(self.fa), np.abs(self.fb))
        # down-weights the ill-conditioned bins; no bin is left out
        self.w = np.minimum(1.0, m / np.median(m))

    def metrics(self, p):
        """(e_pcm, max D, rms D) of a PCM of the padded shape:
        e_pcm = max |P - P64|; D = |rfftn(P) - Q64| * w per spectrum bin."""
        assert p.shape == self.shape, (p.shape, self.shape)
        p = np.asarray(p, np.float64)
        e_pcm = float(np.max(np.abs(p - self.p64)))
        d = np.abs(np.fft.rfftn(p, axes=(0, 1, 2)) - self.q64) * self.w
        return e_pcm, float(np.max(d)), float(np.sqrt(np.mean(d * d)))


METRIC_NAMES = ("e_pcm", "max_D", "rms_D")


def top_gap(p64, k=6):
    """Smallest gap among the oracle's top-k maxima (inf with fewer than
    two): rounding cannot reorder peaks that are further apart."""
    top = np.array([v for v, _ in phasecorr._local_maxima_topk(p64, k)])
    return float(np.min(-np.diff(top))) if top.size > 1 else float("inf")


# ---- injected faults (float64, CPU): what the metrics must see ----

def _pcm_from_spectra(fa, fb, shape):
    return np.fft.irfftn(_cross_power(fa, fb), s=shape, axes=(0, 1, 2))


def plane_fault_pcm(ref, axis):
    """One index plane (k = n // 3 and its mirror) of B's spectrum rotated
    by one twiddle step 2 pi / n along `axis`: a wrong twiddle on one
    index."""
    n = ref.shape[axis]
    k = n // 3
    w = np.exp(2j * np.pi / n)
    fb = ref.fb.copy()
    sl = [slice(None)] * 3
    sl[axis] = k
    fb[tuple(sl)] *= w
    mirror = (n - k) % n
    if axis != X and mirror != k:  # x holds the half spectrum: no mirror
        sl[axis] = mirror
        fb[tuple(sl)] *= np.conj(w)
    return _pcm_from_spectra(ref.fa, fb, ref.shape)


def fault_axis(case):
    """The plane fault goes on the case's axis; a one-point axis has no
    twiddle to get wrong, so the size-1 cases take it on x."""
    return X if case["pad"][case["axis"]] == 1 else case["axis"]


def stale_row_pcm(ref, a, b, axis):
    """One stale row (a copy of row 0) just past B's valid extent along
    `axis` before the transform: a zero-fill guard that lets one element
    through."""
    assert b.shape[axis] < ref.shape[axis]
    bp = np.zeros(ref.shape, np.float64)
    bp[:b.shape[0], :b.shape[1], :b.shape[2]] = b
    src = [slice(None)] * 3
    dst = [slice(None)] * 3
    src[axis], dst[axis] = 0, b.shape[axis]
    bp[tuple(dst)] = bp[tuple(src)]
    fb = np.fft.rfftn(bp, axes=(0, 1, 2))
    return _pcm_from_spectra(ref.fa, fb, ref.shape)
