#!/usr/bin/env python3
"""Interest-point descriptor matching throughput (bs_match_descriptors,
DESIGN.md "Interest point matching").

Workload: the synthetic recipe of tests/match_cases.py (A uniform in a box
at the density of its N = 1000 scene, B = A with 20 % dropped, translated,
jittered, plus 20 % unrelated points) at --sizes points per side, n = 3,
r = 1, no search radius. Run it alone on the device. Reports per size the
median wall time of the whole blocking call (upload, three kernels,
download, host ratio test), per-kernel ms from the library's event timers,
and the descriptor scan's lane-ops per second against the model below. The
comparison figure is the same job on the host's CPUs, timed in the same
run: scipy.spatial.cKDTree for the kNN and for the 2-NN search in
descriptor space (--cpu-workers threads). Writes one JSON document to --out and prints
it as one line.

Lane-op model of k_ip_match per descriptor pair (n = 3: 9 components
padded to 12): 12 subtract + 12 fused multiply-add + 1 scale + 4
compare/select = 29 lane-ops; the chip's peak is 78.6e12 lane-ops/s
(157.3 TFLOPS FP32 vector counts a fused multiply-add as two).
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
from tests import match_cases as mc  # noqa: E402

LANE_OPS_PER_PAIR = 29
PEAK_LANE_OPS = 78.6e12


def scene(n_pts):
    s = (n_pts / 1000.0) ** (1.0 / 3.0)
    box = (256.0 * s, 256.0 * s, 64.0 * s)
    return mc.make_scene(n_pts, box, 4000 + n_pts)[:2]


def cpu_job(a, b, n, r, ratio, workers):
    """kNN + descriptors + 2-NN in descriptor space on the host."""
    import itertools

    from scipy.spatial import cKDTree

    comb = np.array(list(itertools.combinations(range(n + r), n)))

    def desc(p):
        _, idx = cKDTree(p).query(p, k=n + r + 1, workers=workers)
        rel = p[idx[:, 1:][:, comb]] - p[:, None, None, :]
        return rel.reshape(len(p) * len(comb), 3 * n)

    t0 = time.perf_counter()
    da, db = desc(a), desc(b)
    t1 = time.perf_counter()
    d, _ = cKDTree(db).query(da, k=2, workers=workers)
    keep = int(np.sum(d[:, 0] ** 2 * ratio <= d[:, 1] ** 2))
    t2 = time.perf_counter()
    return dict(knn_desc_s=round(t1 - t0, 3), search_s=round(t2 - t1, 3),
                total_s=round(t2 - t0, 3), kept_descriptors=keep)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[20000, 200000])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cpu-max", type=int, default=200000,
                    help="largest size the host comparison is run at")
    ap.add_argument("--cpu-workers", type=int, default=16,
                    help="threads of the host comparison")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles",
                                                  "match_ip.json"))
    args = ap.parse_args()
    n, r = 3, 1
    C = 4
    ctx = Context(0)
    prm = ctx._match_params(n, r, mc.RATIO, 3.4028234663852886e38, None)
    res = dict(workload=dict(n=n, r=r, ratio=mc.RATIO, search_radius=None,
                             recipe="tests/match_cases.py make_scene"),
               steps=args.steps, warmup=args.warmup,
               lane_ops_per_pair=LANE_OPS_PER_PAIR, sizes={})
    for size in args.sizes:
        a, b = scene(size)
        _, cnt = ctx.match_descriptors_raw(a, b, prm, 0)
        for _ in range(args.warmup):
            ctx.match_descriptors_raw(a, b, prm, cnt)
        ctx.reset_stats()
        wall = []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            _, c2 = ctx.match_descriptors_raw(a, b, prm, cnt)
            wall.append(time.perf_counter() - t0)
            assert c2 == cnt
        k = ctx.stats()["kernels"]
        pairs = float(len(a) * C) * float(len(b) * C)
        per_call = {name: k[name]["total_ms"] / args.steps
                    for name in ("ip_knn", "ip_desc", "ip_match")}
        lane = pairs * LANE_OPS_PER_PAIR / (per_call["ip_match"] * 1e-3)
        entry = dict(
            points_a=len(a), points_b=len(b), descriptor_pairs=pairs,
            candidates=cnt,
            wall_ms_median=round(statistics.median(wall) * 1e3, 3),
            wall_ms_min=round(min(wall) * 1e3, 3),
            wall_ms_max=round(max(wall) * 1e3, 3),
            kernel_ms_per_call={n_: round(v, 4) for n_, v in per_call.items()},
            match_lane_ops_per_s=lane,
            match_share_of_peak=round(lane / PEAK_LANE_OPS, 4))
        if size <= args.cpu_max:
            entry["cpu_ckdtree"] = cpu_job(a, b, n, r, mc.RATIO,
                                           args.cpu_workers)
            entry["speedup_vs_cpu"] = round(
                entry["cpu_ckdtree"]["total_s"] * 1e3
                / entry["wall_ms_median"], 1)
        res["sizes"][str(size)] = entry
        print(f"# {size}: {entry}", file=sys.stderr, flush=True)
    res["cpu_workers"] = args.cpu_workers
    ctx.close()
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
