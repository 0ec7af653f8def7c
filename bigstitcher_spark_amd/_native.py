"""ctypes binding of libbigstitch (the C ABI in include/bigstitch.h).

This is the ONLY compute path of the package: there is no CPU fallback.
If the HIP extension is missing or no GPU is present, every entry point
raises NativeUnavailable — by design (the oracle package is test
infrastructure and must never be routed to from here).
"""

from __future__ import annotations

import ctypes as C
import os

import numpy as np

_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                         "libbigstitch.so")


class NativeUnavailable(RuntimeError):
    pass


class _Pair(C.Structure):
    _fields_ = [
        ("view_a", C.c_int32), ("view_b", C.c_int32),
        ("off_a", C.c_int64 * 3), ("size_a", C.c_int64 * 3),
        ("off_b", C.c_int64 * 3), ("size_b", C.c_int64 * 3),
    ]


class _StitchParams(C.Structure):
    _fields_ = [
        ("ds", C.c_int32 * 3), ("peaks_to_check", C.c_int32),
        ("do_subpixel", C.c_int32), ("min_overlap_ratio", C.c_double),
        ("pad_mode", C.c_int32), ("_pad", C.c_int32),
    ]


class _ShiftResult(C.Structure):
    _fields_ = [("shift", C.c_double * 3), ("r", C.c_double),
                ("valid", C.c_int32)]


class _FuseView(C.Structure):
    _fields_ = [
        ("view_id", C.c_int32), ("affine", C.c_double * 12),
        ("blend_border", C.c_float * 3), ("blend_range", C.c_float * 3),
    ]


class _BlockDesc(C.Structure):
    _fields_ = [("min", C.c_int64 * 3), ("size", C.c_int64 * 3)]


class _FuseParams(C.Structure):
    _fields_ = [
        ("fusion_type", C.c_int32), ("out_dtype", C.c_int32),
        ("min_intensity", C.c_double), ("max_intensity", C.c_double),
        ("interp", C.c_int32),
        ("masks", C.c_int32), ("mask_offset", C.c_double * 3),
    ]


class _DogParams(C.Structure):
    _fields_ = [
        ("sigma", C.c_double), ("threshold", C.c_double),
        ("min_intensity", C.c_double), ("max_intensity", C.c_double),
        ("find_min", C.c_int32), ("find_max", C.c_int32),
        ("localization", C.c_int32), ("ds", C.c_int32 * 3),
    ]


class _InterestPoint(C.Structure):
    _fields_ = [
        ("loc", C.c_double * 3), ("value", C.c_float),
        ("intensity", C.c_float), ("kind", C.c_int32),
        ("converged", C.c_int32),
    ]


# numpy view of bs_interest_point[] (same layout as _InterestPoint)
_IP_DTYPE = np.dtype([("loc", np.float64, 3), ("value", np.float32),
                      ("intensity", np.float32), ("kind", np.int32),
                      ("converged", np.int32)])
assert _IP_DTYPE.itemsize == C.sizeof(_InterestPoint)

LOCALIZATION = {"none": 0, "quadratic": 1}


class _MatchParams(C.Structure):
    _fields_ = [
        ("num_neighbors", C.c_int32), ("redundancy", C.c_int32),
        ("ratio_of_distance", C.c_float), ("difference_threshold", C.c_float),
        ("limit_search_radius", C.c_int32), ("search_radius", C.c_double),
    ]


class _RansacParams(C.Structure):
    _fields_ = [
        ("model", C.c_int32), ("regularizer", C.c_int32),
        ("lambda_", C.c_double), ("max_epsilon", C.c_double),
        ("min_inlier_ratio", C.c_double), ("min_num_inliers", C.c_int32),
        ("iterations", C.c_int32),
    ]


class _IntensityParams(C.Structure):
    _fields_ = [
        ("render_scale", C.c_double), ("coefficients", C.c_int32 * 3),
        ("min_num_candidates", C.c_int32), ("min_threshold", C.c_double),
        ("max_threshold", C.c_double), ("iterations", C.c_int32),
        ("min_num_inliers", C.c_int32), ("max_epsilon", C.c_double),
        ("min_inlier_ratio", C.c_double),
    ]


class _IntensitySolveParams(C.Structure):
    _fields_ = [
        ("lambda_identity", C.c_double), ("lambda_smooth", C.c_double),
        ("max_iterations", C.c_int32), ("_pad", C.c_int32),
    ]


# numpy view of bs_intensity_match[]
INTENSITY_MATCH_DTYPE = np.dtype(
    [(k, np.uint64) for k in ("cell_a", "cell_b", "n_cand", "n_inl",
                              "best_it", "n_inl_first", "sp", "sq", "spp",
                              "sqq", "spq")]
    + [("a", np.float64), ("b", np.float64)])
assert INTENSITY_MATCH_DTYPE.itemsize == 104


# numpy view of bs_match_candidate[]
_CAND_DTYPE = np.dtype([("a", np.int32), ("b", np.int32),
                        ("best", np.float32), ("second", np.float32)])
assert _CAND_DTYPE.itemsize == 16

FLT_MAX = float(np.finfo(np.float32).max)
MODELS = {"none": -1, "translation": 0, "rigid": 1, "affine": 2,
          "identity": 3}


BS_K_NAMES = [
    "downsample", "fft_x_fwd", "fft_y_fwd", "fft_z_fwd", "fft_z_inv",
    "fft_y_inv", "fft_x_inv", "peak", "peak_merge", "corr", "subpix",
    "fuse", "synth", "pyramid", "peak_rows",
    "dog_xy", "dog_z", "dog_extrema", "dog_subpix",
    "int_render", "int_moments", "int_ransac",
    "ip_knn", "ip_desc", "ip_match",
]
_NK = len(BS_K_NAMES)


class _Stats(C.Structure):
    _fields_ = [
        ("total_ms", C.c_double * _NK), ("launches", C.c_longlong * _NK),
        ("batch_ms", C.c_double), ("pairs", C.c_longlong),
        ("blocks", C.c_longlong),
    ]


FUSION_AVG = 0
FUSION_AVG_BLEND = 1
FUSION_MAX_INTENSITY = 2
FUSION_LOWEST_VIEWID_WINS = 3
FUSION_HIGHEST_VIEWID_WINS = 4
FUSION_CLOSEST_PIXEL_WINS = 5
OUT_DTYPES = {np.dtype(np.float32): 0, np.dtype(np.uint16): 1,
              np.dtype(np.uint8): 2}

_lib = None


def load_lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise NativeUnavailable(
            f"{_LIB_PATH} not built — run `make` (or __graft_entry__.build())"
        )
    lib = C.CDLL(_LIB_PATH)
    lib.bs_ctx_create.argtypes = [C.POINTER(C.c_void_p), C.c_int]
    lib.bs_ctx_destroy.argtypes = [C.c_void_p]
    lib.bs_last_error.argtypes = [C.c_void_p]
    lib.bs_last_error.restype = C.c_char_p
    lib.bs_view_upload.argtypes = [C.c_void_p, C.c_int32, C.c_void_p,
                                   C.c_int64 * 3]
    lib.bs_view_release.argtypes = [C.c_void_p, C.c_int32]
    lib.bs_view_download.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    lib.bs_view_synth.argtypes = [C.c_void_p, C.c_int32, C.c_int64 * 3,
                                  C.c_void_p, C.c_int32, C.c_uint32,
                                  C.c_uint16, C.c_uint16]
    lib.bs_view_set_coefficients.argtypes = [C.c_void_p, C.c_int32,
                                             C.c_void_p, C.c_int32 * 3]
    lib.bs_view_combine_avg.argtypes = [C.c_void_p, C.c_int32,
                                        C.POINTER(C.c_int32), C.c_int32]
    lib.bs_view_sum.argtypes = [C.c_void_p, C.c_int32,
                                C.POINTER(C.c_uint64)]
    lib.bs_stitch_batch.argtypes = [C.c_void_p, C.POINTER(_Pair), C.c_size_t,
                                    C.POINTER(_StitchParams),
                                    C.POINTER(_ShiftResult)]
    lib.bs_fuse_blocks.argtypes = [C.c_void_p, C.POINTER(_FuseView),
                                   C.c_size_t, C.POINTER(_BlockDesc),
                                   C.c_size_t, C.POINTER(C.c_int32),
                                   C.POINTER(C.c_int64),
                                   C.POINTER(_FuseParams),
                                   C.POINTER(C.c_void_p)]
    lib.bs_fuse_volume.argtypes = [C.c_void_p, C.POINTER(_FuseView),
                                   C.c_size_t, C.c_int64 * 3, C.c_int64 * 3,
                                   C.POINTER(_FuseParams), C.c_int32,
                                   C.POINTER(C.c_int32),
                                   C.POINTER(C.c_int64),
                                   C.POINTER(C.c_void_p)]
    lib.bs_get_stats.argtypes = [C.c_void_p, C.POINTER(_Stats)]
    lib.bs_reset_stats.argtypes = [C.c_void_p]
    lib.bs_debug_last_top5.argtypes = [C.c_void_p, C.c_float * 5,
                                       C.c_int64 * 5]
    lib.bs_debug_pcm.argtypes = [C.c_void_p, C.c_void_p, C.c_int64 * 3]
    lib.bs_debug_pcm_raw.argtypes = [C.c_void_p, C.c_void_p, C.c_int64 * 3]
    lib.bs_debug_rowlist.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t,
                                     C.POINTER(C.c_size_t)]
    lib.bs_debug_peak_scan.argtypes = [C.c_void_p, C.c_void_p, C.c_int64 * 3,
                                       C.c_int, C.c_float * 5, C.c_int64 * 5,
                                       C.POINTER(C.c_int)]
    lib.bs_debug_rtest.argtypes = [C.c_void_p, C.POINTER(_Pair), C.c_void_p,
                                   C.c_int, C.c_void_p, C.c_void_p]
    lib.bs_detect_dog.argtypes = [C.c_void_p, C.c_int32,
                                  C.POINTER(_DogParams), C.c_void_p,
                                  C.c_size_t, C.POINTER(C.c_size_t)]
    lib.bs_debug_dog_volume.argtypes = [C.c_void_p, C.c_int32,
                                        C.POINTER(_DogParams), C.c_void_p,
                                        C.c_int64 * 3]
    lib.bs_match_descriptors.argtypes = [
        C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
        C.POINTER(_MatchParams), C.c_void_p, C.c_size_t,
        C.POINTER(C.c_size_t)]
    lib.bs_debug_ip_knn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t,
                                    C.c_int32, C.c_void_p, C.c_void_p]
    lib.bs_debug_ip_match.argtypes = [
        C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
        C.POINTER(_MatchParams), C.c_void_p, C.c_void_p, C.c_void_p]
    lib.bs_ransac.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t,
                              C.POINTER(_RansacParams), C.c_void_p,
                              C.c_double * 12, C.POINTER(C.c_size_t)]
    lib.bs_intensity_match_pair.argtypes = [
        C.c_void_p, C.c_int32, C.c_double * 12, C.c_int32, C.c_double * 12,
        C.POINTER(_IntensityParams), C.c_void_p, C.c_size_t,
        C.POINTER(C.c_size_t)]
    lib.bs_debug_intensity_render.argtypes = [
        C.c_void_p, C.c_int32, C.c_double * 12, C.c_int32, C.c_double * 12,
        C.POINTER(_IntensityParams), C.c_int64 * 3, C.c_int64 * 3,
        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.bs_intensity_solve.argtypes = [
        C.c_int32, C.c_int32 * 3, C.c_void_p, C.c_void_p, C.c_size_t,
        C.c_void_p, C.POINTER(_IntensitySolveParams), C.c_void_p,
        C.POINTER(C.c_int32), C.POINTER(C.c_double)]
    _lib = lib
    return lib


def intensity_solve(nviews, coefficients, pairs, lambda_identity=0.01,
                    lambda_smooth=0.1, max_iterations=1000):
    """Host-side global intensity solve (bs_intensity_solve; no GPU, no
    Context). pairs: list of (view_a, view_b, matches) with view indices in
    0..nviews-1 and matches an INTENSITY_MATCH_DTYPE array as returned by
    Context.intensity_match_pair(view_a, .., view_b, ..). Returns
    (coeff float64 (nviews, 2, gz, gy, gx), iterations, relative residual);
    coeff[v, 0] multiplies, coeff[v, 1] adds (grey levels)."""
    lib = load_lib()
    cg = [int(v) for v in coefficients]
    ncell = cg[0] * cg[1] * cg[2]
    pv = np.zeros((len(pairs), 2), np.int32)
    offs = np.zeros(len(pairs) + 1, np.uintp)
    chunks = []
    for k, (va, vb, m) in enumerate(pairs):
        pv[k] = (va, vb)
        m = np.ascontiguousarray(m, INTENSITY_MATCH_DTYPE)
        chunks.append(m)
        offs[k + 1] = offs[k] + len(m)
    allm = (np.concatenate(chunks) if chunks
            else np.zeros(0, INTENSITY_MATCH_DTYPE))
    prm = _IntensitySolveParams(float(lambda_identity), float(lambda_smooth),
                                int(max_iterations), 0)
    out = np.zeros((int(nviews), 2 * ncell), np.float64)
    it = C.c_int32(0)
    rr = C.c_double(0.0)
    rc = lib.bs_intensity_solve(
        int(nviews), (C.c_int32 * 3)(*cg), pv.ctypes.data_as(C.c_void_p),
        offs.ctypes.data_as(C.c_void_p), len(pairs),
        allm.ctypes.data_as(C.c_void_p), C.byref(prm),
        out.ctypes.data_as(C.c_void_p), C.byref(it), C.byref(rr))
    if rc != 0:
        raise RuntimeError(f"bs_intensity_solve rc={rc}")
    return (out.reshape(int(nviews), 2, cg[2], cg[1], cg[0]), int(it.value),
            float(rr.value))


def ransac(pa, pb, model="affine", regularizer="rigid", lam=0.1,
           max_epsilon=5.0, min_inlier_ratio=0.1, min_num_inliers=12,
           iterations=10000):
    """Host-side RANSAC (bs_ransac; no GPU, no Context) over correspondences
    pa[i] <-> pb[i], (N,3) xyz. Returns (inlier mask bool (N,), model (3,4)
    mapping A onto B, number of inliers); zero inliers when no consensus
    was accepted."""
    lib = load_lib()
    pa = np.ascontiguousarray(pa, np.float64).reshape(-1, 3)
    pb = np.ascontiguousarray(pb, np.float64).reshape(-1, 3)
    if len(pa) != len(pb):
        raise ValueError("ransac: pa and pb differ in length")
    prm = _RansacParams(MODELS[model.lower()], MODELS[regularizer.lower()],
                        float(lam), float(max_epsilon),
                        float(min_inlier_ratio), int(min_num_inliers),
                        int(iterations))
    mask = np.zeros(len(pa), np.uint8)
    model_out = (C.c_double * 12)()
    n = C.c_size_t(0)
    rc = lib.bs_ransac(pa.ctypes.data_as(C.c_void_p),
                       pb.ctypes.data_as(C.c_void_p), len(pa), C.byref(prm),
                       mask.ctypes.data_as(C.c_void_p), model_out,
                       C.byref(n))
    if rc != 0:
        raise RuntimeError(f"bs_ransac rc={rc}")
    return (mask.astype(bool), np.array(model_out[:]).reshape(3, 4),
            int(n.value))


class Context:
    """One HIP device context (one per GPU; the partition layer hash-shards
    work units across Contexts — SURVEY.md §5, no collectives)."""

    def __init__(self, device: int = 0):
        self._lib = load_lib()
        self._h = C.c_void_p()
        rc = self._lib.bs_ctx_create(C.byref(self._h), device)
        if rc != 0:
            raise NativeUnavailable(
                f"bs_ctx_create failed rc={rc}: "
                f"{self._lib.bs_last_error(None).decode()}"
            )

    def close(self):
        if self._h:
            self._lib.bs_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError(
                f"{what} rc={rc}: {self._lib.bs_last_error(self._h).decode()}"
            )

    # -- views ------------------------------------------------------------
    def upload(self, view_id: int, vol: np.ndarray):
        """vol: (nz, ny, nx) C-contiguous uint16."""
        vol = np.ascontiguousarray(vol, dtype=np.uint16)
        nz, ny, nx = vol.shape
        dims = (C.c_int64 * 3)(nx, ny, nz)
        self._check(
            self._lib.bs_view_upload(
                self._h, view_id, vol.ctypes.data_as(C.c_void_p), dims
            ),
            "bs_view_upload",
        )

    def release(self, view_id: int):
        self._check(self._lib.bs_view_release(self._h, view_id),
                    "bs_view_release")

    def download(self, view_id: int, shape_zyx) -> np.ndarray:
        out = np.empty(shape_zyx, np.uint16)
        self._check(
            self._lib.bs_view_download(
                self._h, view_id, out.ctypes.data_as(C.c_void_p)
            ),
            "bs_view_download",
        )
        return out

    def synth(self, view_id: int, shape_zyx, blobs: np.ndarray,
              noise_seed: int, floor: int = 90, amp: int = 21):
        nz, ny, nx = shape_zyx
        dims = (C.c_int64 * 3)(nx, ny, nz)
        blobs = np.ascontiguousarray(blobs, np.float32)
        self._check(
            self._lib.bs_view_synth(
                self._h, view_id, dims, blobs.ctypes.data_as(C.c_void_p),
                len(blobs), noise_seed & 0xFFFFFFFF, floor, amp
            ),
            "bs_view_synth",
        )

    def set_coefficients(self, view_id: int, ab):
        """ab: (2, gz, gy, gx) float32 (a-plane, b-plane) or None."""
        if ab is None:
            self._check(
                self._lib.bs_view_set_coefficients(
                    self._h, view_id, None, (C.c_int32 * 3)(0, 0, 0)),
                "bs_view_set_coefficients")
            return
        ab = np.ascontiguousarray(ab, np.float32)
        _, gz, gy, gx = ab.shape
        self._check(
            self._lib.bs_view_set_coefficients(
                self._h, view_id, ab.ctypes.data_as(C.c_void_p),
                (C.c_int32 * 3)(gx, gy, gz)),
            "bs_view_set_coefficients")

    # -- stitching --------------------------------------------------------
    def stitch_batch(self, pairs, ds=(2, 2, 1), peaks_to_check=5,
                     do_subpixel=True, min_overlap_ratio=0.25,
                     pad_mode="pow2"):
        """pairs: list of dicts {view_a, view_b, off_a, size_a, off_b,
        size_b} with off/size in (x,y,z). Returns list of dicts(shift
        (sx,sy,sz), r, valid) per oracle.phasecorr [PIN-SIGN]."""
        n = len(pairs)
        cp = (_Pair * n)()
        for i, p in enumerate(pairs):
            cp[i].view_a = p["view_a"]
            cp[i].view_b = p["view_b"]
            for d in range(3):
                cp[i].off_a[d] = p["off_a"][d]
                cp[i].size_a[d] = p["size_a"][d]
                cp[i].off_b[d] = p["off_b"][d]
                cp[i].size_b[d] = p["size_b"][d]
        prm = _StitchParams(
            (C.c_int32 * 3)(*ds), peaks_to_check, int(do_subpixel),
            min_overlap_ratio, {"pow2": 0, "fast": 1}[pad_mode], 0,
        )
        res = (_ShiftResult * n)()
        self._check(
            self._lib.bs_stitch_batch(self._h, cp, n, C.byref(prm), res),
            "bs_stitch_batch",
        )
        return [
            dict(shift=np.array(res[i].shift[:]), r=res[i].r,
                 valid=bool(res[i].valid))
            for i in range(n)
        ]

    # -- fusion -----------------------------------------------------------
    def fuse_blocks(self, views, blocks, view_idx_per_block,
                    fusion_type=FUSION_AVG_BLEND, out_dtype=np.float32,
                    min_intensity=0.0, max_intensity=65535.0,
                    masks=False, mask_offset=(0.0, 0.0, 0.0)):
        """views: list of dicts {view_id, affine (3,4), border, range};
        blocks: list of (min_xyz, size_xyz); view_idx_per_block: list of
        index lists into views. Returns list of (nz,ny,nx) arrays."""
        nv, nb = len(views), len(blocks)
        cv = (_FuseView * nv)()
        for i, v in enumerate(views):
            cv[i].view_id = v["view_id"]
            aff = np.asarray(v["affine"], np.float64).reshape(12)
            for d in range(12):
                cv[i].affine[d] = aff[d]
            for d in range(3):
                cv[i].blend_border[d] = v.get("border", (0, 0, 0))[d]
                cv[i].blend_range[d] = v.get("range", (40, 40, 40))[d]
        cb = (_BlockDesc * nb)()
        outs, outptrs = [], (C.c_void_p * nb)()
        offs = (C.c_int64 * (nb + 1))()
        flat = []
        dt = np.dtype(out_dtype)
        for i, (bmin, bsize) in enumerate(blocks):
            for d in range(3):
                cb[i].min[d] = bmin[d]
                cb[i].size[d] = bsize[d]
            offs[i] = len(flat)
            flat.extend(view_idx_per_block[i])
            a = np.empty((bsize[2], bsize[1], bsize[0]), dt)
            outs.append(a)
            outptrs[i] = a.ctypes.data
        offs[nb] = len(flat)
        cidx = (C.c_int32 * max(1, len(flat)))(*flat) if flat else \
            (C.c_int32 * 1)(0)
        prm = _FuseParams(fusion_type, OUT_DTYPES[dt], min_intensity,
                          max_intensity, 1, 1 if masks else 0,
                          (C.c_double * 3)(*mask_offset))
        self._check(
            self._lib.bs_fuse_blocks(self._h, cv, nv, cb, nb, cidx, offs,
                                     C.byref(prm), outptrs),
            "bs_fuse_blocks",
        )
        return outs

    def fuse_volume(self, views, vol_min, vol_dims, downsamplings=None,
                    fusion_type=FUSION_AVG_BLEND, out_dtype=np.float32,
                    min_intensity=0.0, max_intensity=65535.0,
                    masks=False, mask_offset=(0.0, 0.0, 0.0),
                    out_buffers=None):
        """Whole-volume fusion + pyramid. downsamplings: list of (dx,dy,dz)
        absolute factors per level (level 0 must be (1,1,1)). Returns a
        list of (nz,ny,nx) arrays, one per level. out_buffers: optional
        pre-allocated per-level arrays to write into (avoids the
        first-touch page-fault cost on the D2H path for repeat calls)."""
        if downsamplings is None:
            downsamplings = [(1, 1, 1)]
        nv, nl = len(views), len(downsamplings)
        cv = (_FuseView * nv)()
        for i, v in enumerate(views):
            cv[i].view_id = v["view_id"]
            aff = np.asarray(v["affine"], np.float64).reshape(12)
            for d in range(12):
                cv[i].affine[d] = aff[d]
            for d in range(3):
                cv[i].blend_border[d] = v.get("border", (0, 0, 0))[d]
                cv[i].blend_range[d] = v.get("range", (40, 40, 40))[d]
        dt = np.dtype(out_dtype)
        prm = _FuseParams(fusion_type, OUT_DTYPES[dt], min_intensity,
                          max_intensity, 1, 1 if masks else 0,
                          (C.c_double * 3)(*mask_offset))
        vmin = (C.c_int64 * 3)(*[int(x) for x in vol_min])
        vdim = (C.c_int64 * 3)(*[int(x) for x in vol_dims])
        cds = (C.c_int32 * (3 * nl))(
            *[int(f) for lvl in downsamplings for f in lvl])
        ldims = (C.c_int64 * (3 * nl))()
        outs, outptrs = [], (C.c_void_p * nl)()
        for l, lvl in enumerate(downsamplings):
            d = [(int(vol_dims[k]) + lvl[k] - 1) // lvl[k] for k in range(3)]
            if out_buffers is not None:
                a = out_buffers[l]
                assert a.shape == (d[2], d[1], d[0]) and a.dtype == dt \
                    and a.flags["C_CONTIGUOUS"]
            else:
                a = np.empty((d[2], d[1], d[0]), dt)
            outs.append(a)
            outptrs[l] = a.ctypes.data
        self._check(
            self._lib.bs_fuse_volume(self._h, cv, nv, vmin, vdim,
                                     C.byref(prm), nl, cds, ldims, outptrs),
            "bs_fuse_volume",
        )
        return outs

    # -- interest point detection -----------------------------------------
    @staticmethod
    def _dog_params(sigma, threshold, min_intensity, max_intensity,
                    find_min, find_max, localization, ds):
        return _DogParams(float(sigma), float(threshold),
                          float(min_intensity), float(max_intensity),
                          int(bool(find_min)), int(bool(find_max)),
                          LOCALIZATION[localization.lower()],
                          (C.c_int32 * 3)(*[int(f) for f in ds]))

    def detect_dog_raw(self, view_id, prm, capacity):
        """ABI-level call: (structured array of min(n_found, capacity)
        points, n_found)."""
        out = np.zeros(capacity, _IP_DTYPE)
        n = C.c_size_t(0)
        self._check(
            self._lib.bs_detect_dog(
                self._h, view_id, C.byref(prm),
                out.ctypes.data_as(C.c_void_p) if capacity else None,
                capacity, C.byref(n)),
            "bs_detect_dog",
        )
        return out[:min(capacity, n.value)], int(n.value)

    def detect_dog(self, view_id, sigma, threshold, min_intensity,
                   max_intensity, find_min=False, find_max=True,
                   localization="quadratic", ds=(1, 1, 1)):
        """Difference-of-Gaussian interest points of an uploaded view.
        ds: residual box-mean factors (x,y,z). Returns a dict of arrays:
        loc (N,3) float64 in xyz view pixels, value, intensity (float32),
        kind (+1 max / -1 min), converged (int32); sorted by final voxel."""
        prm = self._dog_params(sigma, threshold, min_intensity,
                               max_intensity, find_min, find_max,
                               localization, ds)
        _, n = self.detect_dog_raw(view_id, prm, 0)
        pts, n2 = self.detect_dog_raw(view_id, prm, n)
        if n2 != n:
            raise RuntimeError(f"bs_detect_dog: count changed {n} -> {n2}")
        return {k: np.ascontiguousarray(pts[k]) for k in _IP_DTYPE.names}

    def debug_dog_volume(self, view_id, sigma, min_intensity, max_intensity,
                         ds=(1, 1, 1)):
        """The DoG volume D at detection scale, (nz, ny, nx) float32."""
        prm = self._dog_params(sigma, 0.0, min_intensity, max_intensity,
                               False, True, "none", ds)
        dims = (C.c_int64 * 3)()
        self._check(self._lib.bs_debug_dog_volume(self._h, view_id,
                                                  C.byref(prm), None, dims),
                    "bs_debug_dog_volume")
        out = np.empty((dims[2], dims[1], dims[0]), np.float32)
        self._check(
            self._lib.bs_debug_dog_volume(
                self._h, view_id, C.byref(prm),
                out.ctypes.data_as(C.c_void_p), dims),
            "bs_debug_dog_volume",
        )
        return out

    # -- interest point matching ------------------------------------------
    @staticmethod
    def _match_params(num_neighbors, redundancy, ratio_of_distance,
                      difference_threshold, search_radius):
        return _MatchParams(int(num_neighbors), int(redundancy),
                            float(ratio_of_distance),
                            float(difference_threshold),
                            0 if search_radius is None else 1,
                            0.0 if search_radius is None
                            else float(search_radius))

    @staticmethod
    def _pts(p):
        return np.ascontiguousarray(p, np.float64).reshape(-1, 3)

    def match_descriptors_raw(self, pts_a, pts_b, prm, capacity):
        """ABI-level call: (structured array of min(n_found, capacity)
        candidates, n_found)."""
        pa, pb = self._pts(pts_a), self._pts(pts_b)
        out = np.zeros(capacity, _CAND_DTYPE)
        n = C.c_size_t(0)
        self._check(
            self._lib.bs_match_descriptors(
                self._h, pa.ctypes.data_as(C.c_void_p), len(pa),
                pb.ctypes.data_as(C.c_void_p), len(pb), C.byref(prm),
                out.ctypes.data_as(C.c_void_p) if capacity else None,
                capacity, C.byref(n)),
            "bs_match_descriptors",
        )
        return out[:min(capacity, n.value)], int(n.value)

    def match_descriptors(self, pts_a, pts_b, num_neighbors=3, redundancy=1,
                          ratio_of_distance=3.0,
                          difference_threshold=FLT_MAX, search_radius=None):
        """Geometric descriptor matching (PRECISE_TRANSLATION) of two (N,3)
        xyz world-coordinate point sets. Returns a dict of arrays a, b
        (int32 indices into the inputs, sorted by (a, b)), best, second
        (float32 descriptor distances)."""
        prm = self._match_params(num_neighbors, redundancy, ratio_of_distance,
                                 difference_threshold, search_radius)
        _, n = self.match_descriptors_raw(pts_a, pts_b, prm, 0)
        out, n2 = self.match_descriptors_raw(pts_a, pts_b, prm, n)
        if n2 != n:
            raise RuntimeError(
                f"bs_match_descriptors: count changed {n} -> {n2}")
        return {k: np.ascontiguousarray(out[k]) for k in _CAND_DTYPE.names}

    def debug_ip_knn(self, pts, k):
        """k nearest neighbours of every point within its set: (idx int32
        (N,k), d2 float32 (N,k)). pts are used as float32 as given."""
        p = self._pts(pts)
        idx = np.full((len(p), k), -1, np.int32)
        d2 = np.full((len(p), k), np.inf, np.float32)
        self._check(
            self._lib.bs_debug_ip_knn(
                self._h, p.ctypes.data_as(C.c_void_p), len(p), k,
                idx.ctypes.data_as(C.c_void_p),
                d2.ctypes.data_as(C.c_void_p)),
            "bs_debug_ip_knn",
        )
        return idx, d2

    def debug_ip_match(self, pts_a, pts_b, num_neighbors=3, redundancy=1,
                       search_radius=None):
        """Raw descriptor scan: (best float32, second float32, best_b int32)
        per A descriptor (point * C + subset); empty when either set has
        fewer than n + r + 1 points."""
        import math
        pa, pb = self._pts(pts_a), self._pts(pts_b)
        prm = self._match_params(num_neighbors, redundancy, 3.0, FLT_MAX,
                                 search_radius)
        k = num_neighbors + redundancy
        nd = 0
        if 1 <= num_neighbors <= k and min(len(pa), len(pb)) > k:
            nd = len(pa) * math.comb(k, num_neighbors)
        best = np.full(nd, np.inf, np.float32)
        second = np.full(nd, np.inf, np.float32)
        bi = np.full(nd, -1, np.int32)
        self._check(
            self._lib.bs_debug_ip_match(
                self._h, pa.ctypes.data_as(C.c_void_p), len(pa),
                pb.ctypes.data_as(C.c_void_p), len(pb), C.byref(prm),
                best.ctypes.data_as(C.c_void_p),
                second.ctypes.data_as(C.c_void_p),
                bi.ctypes.data_as(C.c_void_p)),
            "bs_debug_ip_match",
        )
        return best, second, bi

    # -- debug (not part of the product surface) --------------------------
    @staticmethod
    def _intensity_params(render_scale, coefficients, min_num_candidates,
                          min_threshold, max_threshold, iterations,
                          max_epsilon, min_inlier_ratio, min_num_inliers):
        return _IntensityParams(
            float(render_scale), (C.c_int32 * 3)(*[int(v) for v in
                                                   coefficients]),
            int(min_num_candidates), float(min_threshold),
            float("nan") if max_threshold is None else float(max_threshold),
            int(iterations), int(min_num_inliers), float(max_epsilon),
            float(min_inlier_ratio))

    @staticmethod
    def _affine12(m):
        m = np.ascontiguousarray(m, np.float64).reshape(-1)
        if m.size != 12:
            raise ValueError("affine must be 3x4")
        return (C.c_double * 12)(*m)

    def intensity_match_pair_raw(self, view_a, affine_a, view_b, affine_b,
                                 prm, capacity):
        """One bs_intensity_match_pair call with a buffer of `capacity`
        records: (rc, records written, n_found)."""
        buf = np.zeros(max(int(capacity), 1), INTENSITY_MATCH_DTYPE)
        n = C.c_size_t(0)
        rc = self._lib.bs_intensity_match_pair(
            self._h, view_a, self._affine12(affine_a), view_b,
            self._affine12(affine_b), C.byref(prm),
            buf.ctypes.data_as(C.c_void_p) if capacity else None,
            int(capacity), C.byref(n))
        return rc, buf[:min(int(capacity), n.value)], int(n.value)

    def intensity_match_pair(self, view_a, affine_a, view_b, affine_b,
                             render_scale=0.25, coefficients=(8, 8, 8),
                             min_num_candidates=1000, min_threshold=1.0,
                             max_threshold=None, iterations=1000,
                             max_epsilon=5.1, min_inlier_ratio=0.1,
                             min_num_inliers=10):
        """Intensity matches of two uploaded views (bs_intensity_match_pair):
        an INTENSITY_MATCH_DTYPE array sorted by (cell_a, cell_b)."""
        prm = self._intensity_params(render_scale, coefficients,
                                     min_num_candidates, min_threshold,
                                     max_threshold, iterations, max_epsilon,
                                     min_inlier_ratio, min_num_inliers)
        # one call is enough unless more buckets come back than guessed
        rc, got, n = self.intensity_match_pair_raw(view_a, affine_a, view_b,
                                                   affine_b, prm, 1024)
        self._check(rc, "bs_intensity_match_pair")
        if n > len(got):
            rc, got, n2 = self.intensity_match_pair_raw(
                view_a, affine_a, view_b, affine_b, prm, n)
            self._check(rc, "bs_intensity_match_pair")
            assert n2 == n
        return got.copy()

    def debug_intensity_render(self, view_a, affine_a, view_b, affine_b,
                               render_scale=0.25, coefficients=(8, 8, 8),
                               min_threshold=1.0, max_threshold=None):
        """The render stage alone: dict(origin, dims (x,y,z), P, Q int32 and
        cell_a, cell_b uint16 arrays of shape (gz, gy, gx))."""
        prm = self._intensity_params(render_scale, coefficients, 1,
                                     min_threshold, max_threshold, 1, 1.0,
                                     0.0, 1)
        g0 = (C.c_int64 * 3)()
        gd = (C.c_int64 * 3)()
        fa, fb = self._affine12(affine_a), self._affine12(affine_b)
        self._check(self._lib.bs_debug_intensity_render(
            self._h, view_a, fa, view_b, fb, C.byref(prm), g0, gd, None,
            None, None, None), "bs_debug_intensity_render")
        shape = (gd[2], gd[1], gd[0])
        P = np.zeros(shape, np.int32)
        Q = np.zeros(shape, np.int32)
        ca = np.zeros(shape, np.uint16)
        cb = np.zeros(shape, np.uint16)
        if P.size:
            self._check(self._lib.bs_debug_intensity_render(
                self._h, view_a, fa, view_b, fb, C.byref(prm), g0, gd,
                P.ctypes.data_as(C.c_void_p), Q.ctypes.data_as(C.c_void_p),
                ca.ctypes.data_as(C.c_void_p),
                cb.ctypes.data_as(C.c_void_p)), "bs_debug_intensity_render")
        return dict(origin=tuple(g0), dims=tuple(gd), P=P, Q=Q, cell_a=ca,
                    cell_b=cb)

    def debug_last_top5(self):
        """Top five PCM maxima of the last stitched pair as the candidate
        stage received them: (values float32[5], linear indices int64[5])."""
        v, idx = (C.c_float * 5)(), (C.c_int64 * 5)()
        self._check(self._lib.bs_debug_last_top5(self._h, v, idx),
                    "bs_debug_last_top5")
        return np.array(v[:], np.float32), np.array(idx[:], np.int64)

    def debug_pcm(self, raw=False):
        """PCM of the last stitched pair as float32 (pz, py, px). Under
        BS_PCM_MODE=rows the library first rebuilds the whole volume;
        raw=True returns the buffer as it stands instead (only the rows
        of debug_rowlist() belong to the pair then)."""
        fn = self._lib.bs_debug_pcm_raw if raw else self._lib.bs_debug_pcm
        dims = (C.c_int64 * 3)()
        self._check(fn(self._h, None, dims), "bs_debug_pcm")
        px, py, pz = dims[:]
        out = np.empty((pz, py, px), np.float32)
        self._check(fn(self._h, out.ctypes.data_as(C.c_void_p), dims),
                    "bs_debug_pcm")
        return out

    def debug_rowlist(self):
        """PCM rows (z * py + y, int32, unordered) the inverse x pass
        wrote for the last stitched pair under BS_PCM_MODE=rows."""
        out = np.empty(9 * 512, np.int32)  # 9 * BS_PEAK_ROWS_CAP
        n = C.c_size_t(0)
        self._check(
            self._lib.bs_debug_rowlist(self._h, out.ctypes.data_as(C.c_void_p),
                                       out.size, C.byref(n)),
            "bs_debug_rowlist")
        return out[:n.value].copy()

    def debug_peak_scan(self, vol: np.ndarray, mode: str = "auto"):
        """Run the stitch path's peak stage on a (pz, py, px) float32
        volume. Returns (values float32[5], indices int64[5], fell_back)."""
        vol = np.ascontiguousarray(vol, np.float32)
        pz, py, px = vol.shape
        v, idx = (C.c_float * 5)(), (C.c_int64 * 5)()
        fb = C.c_int(0)
        self._check(
            self._lib.bs_debug_peak_scan(
                self._h, vol.ctypes.data_as(C.c_void_p),
                (C.c_int64 * 3)(px, py, pz), {"auto": 0, "full": 1}[mode],
                v, idx, C.byref(fb)),
            "bs_debug_peak_scan",
        )
        return (np.array(v[:], np.float32), np.array(idx[:], np.int64),
                bool(fb.value))

    def debug_rtest(self, pair, shifts):
        """Run this context's r-test kernel (BS_CORR_MODE) on integer
        shifts (n, 3) = (sx, sy, sz) of one pair dict at ds = 1, without
        the min_overlap filter. Returns (sums uint64 (n, 5) = sum a, b, aa,
        bb, ab over each overlap, voxel counts int64 (n,))."""
        cp = _Pair()
        cp.view_a = pair["view_a"]
        cp.view_b = pair["view_b"]
        for d in range(3):
            cp.off_a[d] = pair["off_a"][d]
            cp.size_a[d] = pair["size_a"][d]
            cp.off_b[d] = pair["off_b"][d]
            cp.size_b[d] = pair["size_b"][d]
        sh = np.ascontiguousarray(shifts, np.int32).reshape(-1, 3)
        n = len(sh)
        sums = np.zeros((n, 5), np.uint64)
        nvox = np.zeros(n, np.int64)
        self._check(
            self._lib.bs_debug_rtest(
                self._h, C.byref(cp), sh.ctypes.data_as(C.c_void_p), n,
                sums.ctypes.data_as(C.c_void_p),
                nvox.ctypes.data_as(C.c_void_p)),
            "bs_debug_rtest",
        )
        return sums, nvox

    # -- stats ------------------------------------------------------------
    def stats(self):
        s = _Stats()
        self._check(self._lib.bs_get_stats(self._h, C.byref(s)),
                    "bs_get_stats")
        return dict(
            kernels={
                BS_K_NAMES[i]: dict(total_ms=s.total_ms[i],
                                    launches=int(s.launches[i]))
                for i in range(_NK)
            },
            batch_ms=s.batch_ms, pairs=int(s.pairs), blocks=int(s.blocks),
        )

    def reset_stats(self):
        self._check(self._lib.bs_reset_stats(self._h), "bs_reset_stats")
