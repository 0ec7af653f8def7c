#!/usr/bin/env python3
"""Difference-of-Gaussian interest point detection throughput
(bs_detect_dog, DESIGN.md "Interest point detection").

Workload: one device-generated synthetic view (bs_view_synth),
1024x1024x256 uint16, sigma 1.8, threshold 0.008, ds (1,1,1), MAX,
QUADRATIC. Run it alone on the device. Reports the median wall time of
>= 10 whole calls (host clock around the blocking call, which ends in a
stream synchronise and includes the candidate download and host sort),
Mvox/s, per-kernel ms from the library's event timers, achieved bytes/s
of each kernel against the traffic model below, and the wall time of the
numpy restatement (tests/dog_ref.py) for scale. Writes one JSON document
to --out and prints it as one line.

Traffic model (bytes per voxel, halos ignored):
  dog_xy       2 read (uint16) + 8 written (two float volumes)
  dog_z        8 read + 4 written (D)
  dog_extrema  4 read
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bigstitcher_spark_amd import Context  # noqa: E402
from oracle import synth  # noqa: E402
from tests import dog_ref  # noqa: E402

MODEL_BYTES = {"dog_xy": 10, "dog_z": 12, "dog_extrema": 4}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=[256, 1024, 1024],
                    help="z y x")
    ap.add_argument("--sigma", type=float, default=1.8)
    ap.add_argument("--threshold", type=float, default=0.008)
    ap.add_argument("--lo", type=float, default=0.0)
    ap.add_argument("--hi", type=float, default=4095.0)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ref-planes", type=int, default=32,
                    help="z planes of the view the numpy reference is timed "
                         "on (scaled linearly to the whole view; 0 = whole "
                         "view, -1 = skip)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles",
                                                  "detect_dog.json"))
    args = ap.parse_args()
    if args.steps < 10:
        ap.error("--steps must be >= 10 (median of >= 10 timed calls)")
    nz, ny, nx = args.shape
    nvox = nz * ny * nx

    ctx = Context(0)
    rng = np.random.default_rng(7)
    blobs = synth.make_scene((nz, ny, nx), rng, margin=8)
    ctx.synth(0, (nz, ny, nx), blobs, noise_seed=11)
    prm = ctx._dog_params(args.sigma, args.threshold, args.lo, args.hi,
                          False, True, "quadratic", (1, 1, 1))
    _, n = ctx.detect_dog_raw(0, prm, 0)
    for _ in range(args.warmup):
        ctx.detect_dog_raw(0, prm, n)
    ctx.reset_stats()
    wall = []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        pts, n2 = ctx.detect_dog_raw(0, prm, n)
        wall.append(time.perf_counter() - t0)
        assert n2 == n
    k = ctx.stats()["kernels"]
    med = statistics.median(wall)
    kernels = {}
    for name in ("dog_xy", "dog_z", "dog_extrema", "dog_subpix"):
        ms = k[name]["total_ms"] / max(1, k[name]["launches"])
        kernels[name] = dict(ms_per_launch=round(ms, 4),
                             launches=k[name]["launches"])
        if name in MODEL_BYTES and ms > 0:
            kernels[name]["model_bytes_per_voxel"] = MODEL_BYTES[name]
            kernels[name]["achieved_GBps"] = round(
                MODEL_BYTES[name] * nvox / (ms * 1e-3) / 1e9, 1)
    kernel_ms = sum(v["ms_per_launch"] * v["launches"]
                    for v in kernels.values()) / args.steps

    ref = None
    if args.ref_planes >= 0:
        planes = nz if args.ref_planes == 0 else min(nz, args.ref_planes)
        sub = ctx.download(0, (nz, ny, nx))[:planes]
        t0 = time.perf_counter()
        dog_ref.detect(sub, args.sigma, args.threshold, args.lo, args.hi)
        t = time.perf_counter() - t0
        ref = dict(planes_timed=planes, seconds=round(t, 3),
                   seconds_scaled_to_view=round(t * nz / planes, 3))
    ctx.close()

    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short",
                                 "HEAD"], capture_output=True,
                                text=True).stdout.strip() or None
    except OSError:
        commit = None
    res = dict(
        workload=dict(shape_zyx=[nz, ny, nx], sigma=args.sigma,
                      threshold=args.threshold, lo=args.lo, hi=args.hi,
                      ds=[1, 1, 1], type="MAX", localization="QUADRATIC"),
        points=n, steps=args.steps, warmup=args.warmup,
        wall_ms_median=round(med * 1e3, 3),
        wall_ms_min=round(min(wall) * 1e3, 3),
        wall_ms_max=round(max(wall) * 1e3, 3),
        mvox_per_s=round(nvox / med / 1e6, 1),
        kernel_ms_per_call=round(kernel_ms, 3),
        model_bytes_per_voxel=sum(MODEL_BYTES.values()),
        model_GBps_over_kernel_time=round(
            sum(MODEL_BYTES.values()) * nvox / (kernel_ms * 1e-3) / 1e9, 1),
        kernels=kernels, numpy_reference=ref,
        date=time.strftime("%Y-%m-%d"), parent_commit=commit,
    )
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
