"""Inputs shared by tests/test_dog_ref_cpu.py and tests/test_gpu_detect.py
(not a test). The CPU file asserts on the numpy reference alone that these
inputs have the margins the GPU comparisons rely on; the GPU file compares
the device against the same cached reference results."""

from __future__ import annotations

import functools

import numpy as np

from tests import dog_ref

SIGMA = 1.8
LO, HI = 0.0, 4095.0
T_BRIGHT = 0.008   # MAX / MIN, QUADRATIC
T_MIXED = 0.02     # BOTH, NONE
EPS = 1e-5

# (z,y,x) -> number of planted blobs; border 2.0 puts some two voxels from
# a face. (5,9,70): the sigma2 filter radius 6 exceeds nz-1 and ny-1 is
# barely above it, so the mirror reflects more than once.
BRIGHT_SHAPES = {(40, 48, 56): 14, (19, 70, 33): 8, (12, 37, 150): 9,
                 (5, 9, 70): 4}
MIXED_SHAPES = {(40, 48, 56): 10, (12, 37, 150): 6}
DS_SHAPES = {(20, 48, 56): 10, (20, 48, 59): 10}  # second: odd x dim


def _seed(shape):
    return 1000 + shape[0] * 7 + shape[1] * 3 + shape[2]


@functools.lru_cache(maxsize=None)
def bright(shape):
    vol, cen = dog_ref.make_bright(shape, BRIGHT_SHAPES.get(
        shape, DS_SHAPES.get(shape)), _seed(shape))
    vol.setflags(write=False)
    return vol, cen


@functools.lru_cache(maxsize=None)
def dark(shape):
    vol, cen = dog_ref.make_dark(shape, BRIGHT_SHAPES[shape], _seed(shape))
    vol.setflags(write=False)
    return vol, cen


@functools.lru_cache(maxsize=None)
def mixed(shape):
    vol, cen, sign = dog_ref.make_mixed(shape, MIXED_SHAPES[shape],
                                        _seed(shape) + 1)
    vol.setflags(write=False)
    return vol, cen, sign


@functools.lru_cache(maxsize=None)
def ref_volume(which, shape, ds=(1, 1, 1)):
    vol = {"bright": bright, "dark": dark, "mixed": mixed}[which](shape)[0]
    D = dog_ref.dog_volume(vol, SIGMA, LO, HI, ds)
    D.setflags(write=False)
    return D


@functools.lru_cache(maxsize=None)
def ref_detect(which, shape, ds=(1, 1, 1)):
    """Reference points: bright -> MAX, dark -> MIN, both QUADRATIC."""
    vol = {"bright": bright, "dark": dark}[which](shape)[0]
    return dog_ref.detect(vol, SIGMA, T_BRIGHT, LO, HI,
                          find_min=which == "dark",
                          find_max=which == "bright",
                          localization="quadratic", ds=ds,
                          D=ref_volume(which, shape, ds))
