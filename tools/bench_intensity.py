#!/usr/bin/env python3
"""Intensity matching throughput (bs_intensity_match_pair, DESIGN.md
"Intensity matching").

Workload: two --size^3 uint16 views of one smooth synthetic scene, view B =
1.25 * scene + 150, both with +-2 grey levels of noise; 8x8x8 coefficient
cells, renderScale 0.25, 1000 RANSAC iterations, every other parameter at the
CLI default. Two placements: B shifted along x so that 10 % of the view
overlaps, and B on top of A (full overlap). Run it alone on the device.
Reports per placement the median wall time of the whole blocking call over
--calls calls after --warmup warm-ups (render, moments, compaction, RANSAC,
refit rounds, downloads and the host geometry in between), per-kernel ms per
call from the library's event timers, and the time of the numpy contract
(tests/intensity_ref.py, buckets spread over --cpu-workers threads) on the
same input, whose records must equal the device's. Writes one JSON document
to --out and prints it as one line.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bigstitcher_spark_amd import Context  # noqa: E402
from tests import intensity_ref as ir  # noqa: E402

INT_FIELDS = ir.FIELDS


def curve(rng, n):
    """Smooth 1-D profile in [0, 1] over n + n world positions."""
    x = np.arange(2 * n, dtype=np.float64)
    v = np.zeros_like(x)
    for _ in range(6):
        v += rng.uniform(0.3, 1.0) * np.sin(
            x * rng.uniform(0.01, 0.06) + rng.uniform(0, 6.28))
    return (v - v.min()) / (v.max() - v.min())


def make_views(size, shift_x, seed=5):
    rng = np.random.default_rng(seed)
    cx, cy, cz = curve(rng, size), curve(rng, size), curve(rng, size)

    def scene(x0):
        return (300.0 + 500.0 * cz[:size, None, None]
                + 500.0 * cy[None, :size, None]
                + 500.0 * cx[None, None, x0:x0 + size])

    def quant(v):
        v += rng.integers(-2, 3, size=v.shape)
        return np.clip(np.rint(v), 0, 65535).astype(np.uint16)

    a = quant(scene(0))
    b = quant(1.25 * scene(shift_x) + 150.0)
    aff_a = np.hstack([np.eye(3), np.zeros((3, 1))])
    aff_b = aff_a.copy()
    aff_b[0, 3] = float(shift_x)
    return a, aff_a, b, aff_b


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cpu-workers", type=int, default=16)
    ap.add_argument("--skip-cpu", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles",
                                                  "match_intensity.json"))
    args = ap.parse_args()
    prm = dict(render_scale=0.25, coefficients=(8, 8, 8), iterations=1000)
    doc = dict(tool="tools/bench_intensity.py", size=args.size, params=dict(
        prm, coefficients=list(prm["coefficients"])), calls=args.calls,
        warmup=args.warmup, cpu_workers=args.cpu_workers, cases=[])
    with Context(0) as ctx:
        for name, shift in (("overlap_10pct", int(round(0.9 * args.size))),
                            ("overlap_full", 0)):
            a, aff_a, b, aff_b = make_views(args.size, shift)
            ctx.upload(0, a)
            ctx.upload(1, b)
            for _ in range(args.warmup):
                got = ctx.intensity_match_pair(0, aff_a, 1, aff_b, **prm)
            ctx.reset_stats()
            wall = []
            for _ in range(args.calls):
                t0 = time.perf_counter()
                got = ctx.intensity_match_pair(0, aff_a, 1, aff_b, **prm)
                wall.append((time.perf_counter() - t0) * 1e3)
            st = ctx.stats()["kernels"]
            row = dict(
                case=name, shift_x=shift, buckets=int(len(got)),
                inliers=int(got["n_inl"].sum()),
                candidates=int(got["n_cand"].sum()),
                wall_ms_median=statistics.median(wall),
                wall_ms_min=min(wall), wall_ms_max=max(wall),
                kernel_ms_per_call={
                    k: st[k]["total_ms"] / args.calls
                    for k in ("int_render", "int_moments", "int_ransac")},
                kernel_launches_per_call={
                    k: st[k]["launches"] / args.calls
                    for k in ("int_render", "int_moments", "int_ransac")})
            if not args.skip_cpu:
                t0 = time.perf_counter()
                ref = ir.match_pair(a, aff_a, b, aff_b,
                                    workers=args.cpu_workers, **prm)
                row["numpy_ref_s"] = time.perf_counter() - t0
                row["numpy_ref_equal"] = bool(
                    len(ref["records"]) == len(got) and all(
                        int(g[k]) == r[k] for g, r in zip(got, ref["records"])
                        for k in INT_FIELDS))
                row["speedup_vs_numpy"] = (row["numpy_ref_s"] * 1e3
                                           / row["wall_ms_median"])
            doc["cases"].append(row)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
