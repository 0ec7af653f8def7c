#!/usr/bin/env python3
"""Solo timing of the production r-test (k_rtest / k_rtest_wide /
k_rtest_dot, chosen by BS_CORR_MODE = legacy | wide | dot) through bs_debug_rtest: the launch phase B makes, alone on
the device, HIP-event timed (stat `corr`).

Geometry is the headline benchmark's: two 512^3 uint16 synthetic views and
the candidate set of ONE peak with its 8 periodic wraps, filtered at
min_overlap_ratio 0.05 as phase B does (the debug entry itself does not
filter). Run once per x-shift parity, boxes otherwise alike:

    BS_CORR_MODE=wide   python tools/bench_rtest.py --sx 460
    BS_CORR_MODE=wide   python tools/bench_rtest.py --sx 459
    BS_CORR_MODE=legacy python tools/bench_rtest.py --sx 459

Prints one JSON line: median / min / max ms of --launches launches, the
scanned bytes (4 per voxel pair, candidates summed; shared planes hit L2
so HBM bytes are lower) and the rate they imply. Records:
profiles/rtest_wide_solo.json, profiles/rtest_dot_solo.json."""

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--sx", type=int, default=460, help="peak x (0..size)")
    ap.add_argument("--sy", type=int, default=5)
    ap.add_argument("--sz", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--min-overlap", type=float, default=0.05)
    args = ap.parse_args()
    if args.launches < 10:
        ap.error("--launches must be >= 10")

    from bigstitcher_spark_amd import Context
    from oracle import synth

    n = args.size
    shape = (n, n, n)
    ctx = Context(0)
    blobs_a, blobs_b = synth.pair_blobs_union(
        shape, (float(args.sx), float(args.sy), float(args.sz)), seed=17)
    ctx.synth(0, shape, blobs_a, noise_seed=0)
    ctx.synth(1, shape, blobs_b, noise_seed=1)
    pair = dict(view_a=0, view_b=1, off_a=(0, 0, 0), size_a=(n, n, n),
                off_b=(0, 0, 0), size_b=(n, n, n))
    peak = (args.sx % n, args.sy % n, args.sz % n)
    wraps = [tuple(peak[d] - (n if ci >> d & 1 else 0) for d in range(3))
             for ci in range(8)]
    _, nvox = ctx.debug_rtest(pair, wraps)
    keep = [w for w, v in zip(wraps, nvox)
            if v >= max(args.min_overlap * n ** 3, 1.0)]
    if not keep:
        sys.exit("no candidate passes the overlap filter")
    for _ in range(args.warmup):
        ctx.debug_rtest(pair, keep)
    ms = []
    for _ in range(args.launches):
        ctx.reset_stats()
        sums, nv = ctx.debug_rtest(pair, keep)
        k = ctx.stats()["kernels"]["corr"]
        assert k["launches"] == 1
        ms.append(k["total_ms"])
    ctx.close()
    scanned = 4.0 * float(nv.sum())
    med = float(np.median(ms))
    print(json.dumps({
        "tool": "bench_rtest",
        "mode": os.environ.get("BS_CORR_MODE", "default"),
        "size": n,
        "peak": list(peak),
        "x_parity": "odd" if args.sx & 1 else "even",
        "candidates": [list(map(int, w)) for w in keep],
        "launches": args.launches,
        "corr_ms": {"median": round(med, 4), "min": round(min(ms), 4),
                    "max": round(max(ms), 4)},
        "scanned_bytes": scanned,
        "scanned_GBps_at_median": round(scanned / (med * 1e-3) / 1e9, 1),
        "checksum": int(sums.sum(dtype=np.uint64) & np.uint64(0xFFFFFFFF)),
    }))


if __name__ == "__main__":
    main()
