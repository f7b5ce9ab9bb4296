"""Clustering measurement: device.region_hclust on the distances of synthetic
spectra, beside scipy's linkage on one host thread on the same matrix.

  python tools/hclust_bench.py [--sizes 2000,8192,24611] [--out profiles/spectra/hclust_bench.json]

The driver (no --measure) runs one measuring process per size, each under its
own `timeout`, chained so that nothing starts after a step that failed, and
merges their lines into --out.  The library must be built (__graft_entry__.build()).

A measuring process (--measure --n N) makes synthetic counts from a seeded
generator at ncol = 256, runs device.region_distances on them and then, for
each method, device.region_hclust --warmup + --reps times, each call on a fresh
device copy of the distances made outside the timed part (keep_input=False:
the call consumes its copy and allocates nothing).  Reported per method: the
medians of the hipEvent phases of ks_hclust_stats (check, init, merge), of the
wall clock around the synchronous call, n_rescans, and the merge time per step.

The yardstick is scipy.cluster.hierarchy.linkage of the downloaded matrix, one
call per method on one host thread (--no-scipy skips it; it is skipped with a
note where scipy is not importable).  For complete and single linkage the
heights are also compared with scipy's bit for bit (the synthetic distances
are tie-free, where the two must agree); for average within rtol 1e-9.

n = 24,611 is the reference's region list (test.R:762): 302,838,355 distances,
2.42 GB on the device, and as much again for the copy.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

METHODS = ("complete", "single", "average")


def measure(args) -> dict:
    import torch

    from kmer_spans_amd import _lib, device as D
    assert torch.cuda.is_available(), "hclust_bench needs a HIP device"
    ctx = _lib.context(0)
    D.bind_torch_stream(ctx)
    n, ncol = args.n, args.ncol
    rng = np.random.default_rng(args.seed)
    counts = rng.integers(0, 2000, size=(n, ncol)).astype(np.uint32)
    counts[rng.random((n, ncol)) < 0.4] = 0
    counts[:, 0] |= 1
    dist, dst = D.region_distances(ctx, torch.from_numpy(counts.view(np.int32)).cuda())
    res = {"n": n, "ncol": ncol, "pairs": int(dist.numel()), "matrix_bytes": 8 * int(dist.numel()),
           "build": _lib.build_id(), "device": torch.cuda.get_device_name(0), "reps": args.reps,
           "warmup": args.warmup, "seed": args.seed, "ms_distances": round(dst["ms_total"], 4), "methods": {}}
    trees = {}
    for method in METHODS:
        stats, wall = [], []
        for r in range(args.warmup + args.reps):
            work = dist.clone()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tree, st = D.region_hclust(ctx, work, method=method, keep_input=False)
            if r >= args.warmup:
                wall.append((time.perf_counter() - t0) * 1e3)
                stats.append(st)
            del work
        trees[method] = tree
        med = {key: float(np.median([s[key] for s in stats])) for key in ("ms_total", "ms_check", "ms_init", "ms_merge")}
        res["methods"][method] = {
            "ms_check_median": round(med["ms_check"], 4), "ms_init_median": round(med["ms_init"], 4),
            "ms_merge_median": round(med["ms_merge"], 3),
            "ms_merge_min_max": [round(min(s["ms_merge"] for s in stats), 3), round(max(s["ms_merge"] for s in stats), 3)],
            "ms_total_median": round(med["ms_total"], 3), "ms_wall_median": round(float(np.median(wall)), 3),
            "us_per_step": round(med["ms_merge"] * 1e3 / (n - 1), 3),
            "n_rescans": int(stats[-1]["n_rescans"]), "rescans_per_step": round(stats[-1]["n_rescans"] / (n - 1), 3),
            "work_bytes": int(stats[-1]["work_bytes"]),
            "heights_sorted": bool((np.diff(tree["height"]) >= 0).all())}
    if not args.no_scipy:
        try:
            from scipy.cluster.hierarchy import linkage
        except ImportError:
            res["scipy"] = "not importable here"
        else:
            import scipy
            host = dist.cpu().numpy()
            res["scipy"] = {"version": scipy.__version__, "threads": 1, "where": "the GPU machine's host CPU"}
            for method in METHODS:
                t0 = time.perf_counter()
                z = linkage(host, method)
                ms = (time.perf_counter() - t0) * 1e3
                line = res["methods"][method]
                line["scipy_linkage_ms"] = round(ms, 2)
                line["scipy_over_device_wall"] = round(ms / line["ms_wall_median"], 3)
                h = trees[method]["height"]
                if method == "average":
                    line["heights_vs_scipy"] = {"max_rel_diff": float(np.max(np.abs(h - z[:, 2]) / np.abs(z[:, 2])))}
                else:
                    line["heights_vs_scipy"] = {"bit_mismatches": int((h.view(np.uint64) != z[:, 2].view(np.uint64)).sum())}
    return res


def drive(args) -> int:
    me = os.path.abspath(__file__)
    tmp = os.path.join(os.path.dirname(os.path.abspath(args.out)), ".hclust_bench_")
    os.makedirs(os.path.dirname(tmp), exist_ok=True)
    sizes = [int(x) for x in args.sizes.split(",")]
    steps = []
    for n in sizes:  # every GPU step under its own time limit; nothing starts after a step that failed
        reps = args.reps if n < 20000 else max(1, min(args.reps, 3))
        steps.append(f"timeout -k 10 {args.step_timeout} {sys.executable} {me} --measure --n {n} --ncol {args.ncol} "
                     f"--reps {reps} --warmup {args.warmup} --seed {args.seed} "
                     f"{'--no-scipy ' if args.no_scipy else ''}--out {tmp}{n}.json")
    rc = subprocess.call(["bash", "-c", "set -o pipefail; " + " && ".join(steps)])
    if rc != 0:
        print(f"a measuring step ended with status {rc}", file=sys.stderr)
        return rc
    res = {"tool": "hclust_bench", "same_session": True, "sizes": []}
    for n in sizes:
        with open(f"{tmp}{n}.json") as f:
            res["sizes"].append(json.load(f))
        os.remove(f"{tmp}{n}.json")
    text = json.dumps(res)
    print(text)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2000,8192,24611")
    ap.add_argument("--n", type=int, default=24611)
    ap.add_argument("--ncol", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5, help="timed calls per method (at most 3 from n = 20,000 on)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--no-scipy", action="store_true", help="skip the host yardstick")
    ap.add_argument("--step-timeout", type=int, default=400, help="seconds per measuring process")
    ap.add_argument("--measure", action="store_true", help="one measuring process (the driver starts these)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectra", "hclust_bench.json"))
    args = ap.parse_args()
    if not args.measure:
        return drive(args)
    res = measure(args)
    text = json.dumps(res)
    print(text)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
