"""Silhouette measurement: device.region_silhouette on the distances of
synthetic spectra and the groups of their complete-linkage tree, beside
sklearn's silhouette_samples on the host on the same matrix.

  python tools/silhouette_bench.py [--sizes 2000,8192,24611] [--ks 2,50,2000]
                                   [--out profiles/spectra/silhouette_bench.json]

The driver (no --measure) runs one measuring process per size, each under its
own `timeout`, chained so that nothing starts after a step that failed, and
merges their lines into --out.  The library must be built (__graft_entry__.build()).

A measuring process (--measure --n N) makes synthetic counts from a seeded
generator at ncol = 256, runs device.region_distances and the complete-linkage
device.region_hclust on them (the input is kept) and then, for each k below n,
cuts the tree into k groups and runs device.region_silhouette --warmup + --reps
times.  Reported per k: the medians of the hipEvent phases of
ks_silhouette_stats (check, sums, widths) and of the wall clock around the
synchronous call, n_chunks, work_bytes, the time of the sums per matrix byte,
and ms_sums over ms_check: the finiteness pass is one coalesced read of the
matrix in the same call, the figure the sums are to be compared with.

What the scattered columns cost: the same group sizes with contiguous labels
(group 1 the first n_1 observations, and so on) are timed too.  The kernel
reads D(i, j) for the columns j above a strip of 64 rows as one entry of each
of 64 rows; with contiguous members consecutive j share a row's cache line,
with the tree's scattered members they do not.  `contiguous` holds that run.

The yardstick is sklearn.metrics.silhouette_samples(metric="precomputed") on
the downloaded square matrix, skipped from --sklearn-max-n on (8 n^2 bytes: 4.8
GB at n = 24,611), with --no-sklearn and where sklearn is not importable.  The
largest difference between its widths and the device's is reported.

n = 24,611 is the reference's region list (test.R:762): 302,838,355 distances,
2.42 GB on the device.
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

PHASES = ("ms_total", "ms_check", "ms_sums", "ms_widths")


def timed(D, ctx, dist, group, args):
    """Medians over the timed calls: (line, result of the last call)."""
    import torch
    stats, wall = [], []
    for r in range(args.warmup + args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res, st = D.region_silhouette(ctx, dist, group)
        if r >= args.warmup:
            wall.append((time.perf_counter() - t0) * 1e3)
            stats.append(st)
    med = {key: float(np.median([s[key] for s in stats])) for key in PHASES}
    nbytes = 8 * int(dist.numel())
    line = {"ms_check_median": round(med["ms_check"], 4), "ms_sums_median": round(med["ms_sums"], 4),
            "ms_sums_min_max": [round(min(s["ms_sums"] for s in stats), 4), round(max(s["ms_sums"] for s in stats), 4)],
            "ms_widths_median": round(med["ms_widths"], 4), "ms_total_median": round(med["ms_total"], 4),
            "ms_wall_median": round(float(np.median(wall)), 3),
            "check_GBps": round(nbytes / med["ms_check"] / 1e6, 1),
            "sums_ps_per_matrix_byte": round(med["ms_sums"] * 1e9 / nbytes, 3),
            "sums_over_check": round(med["ms_sums"] / med["ms_check"], 2),
            "n_chunks": int(stats[-1]["n_chunks"]), "work_bytes": int(stats[-1]["work_bytes"])}
    return line, res


def measure(args) -> dict:
    import torch

    import kmer_spans_amd as K
    from kmer_spans_amd import _lib, device as D
    assert torch.cuda.is_available(), "silhouette_bench needs a HIP device"
    ctx = _lib.context(0)
    D.bind_torch_stream(ctx)
    n, ncol = args.n, args.ncol
    rng = np.random.default_rng(args.seed)
    counts = rng.integers(0, 2000, size=(n, ncol)).astype(np.uint32)
    counts[rng.random((n, ncol)) < 0.4] = 0
    counts[:, 0] |= 1
    dist, dst = D.region_distances(ctx, torch.from_numpy(counts.view(np.int32)).cuda())
    tree, hst = D.region_hclust(ctx, dist, method="complete", keep_input=True)
    res = {"n": n, "ncol": ncol, "pairs": int(dist.numel()), "matrix_bytes": 8 * int(dist.numel()),
           "build": _lib.build_id(), "device": torch.cuda.get_device_name(0), "reps": args.reps,
           "warmup": args.warmup, "seed": args.seed, "ms_distances": round(dst["ms_total"], 4),
           "ms_hclust": round(hst["ms_total"], 3), "k": {}}
    host = None
    want_sklearn = not args.no_sklearn and n < args.sklearn_max_n
    if want_sklearn:
        try:
            import sklearn
            from sklearn.metrics import silhouette_samples
        except ImportError:
            res["sklearn"] = "not importable here"
            want_sklearn = False
        else:
            from scipy.spatial.distance import squareform
            res["sklearn"] = {"version": sklearn.__version__, "where": "the GPU machine's host CPU",
                              "square_matrix_bytes": 8 * n * n}
            host = squareform(dist.cpu().numpy())
    elif not args.no_sklearn:
        res["sklearn"] = f"skipped: the square matrix is {8 * n * n} bytes"
    for k in (int(x) for x in args.ks.split(",")):
        if k >= n:
            continue
        group = K.cut_tree(tree, k=k)
        line, out = timed(D, ctx, dist, group, args)
        size = out["size"]
        line.update({"largest_group": int(size.max()), "singletons": int((size == 1).sum()),
                     "avg_width_all": out["avg_width_all"], "max_diameter": float(np.nanmax(out["diameter"])),
                     "cut_height_bound": float(tree["height"][n - k - 1])})
        contiguous = np.repeat(np.arange(1, k + 1), size).astype(np.int32)
        cl, _ = timed(D, ctx, dist, contiguous, args)
        line["contiguous"] = {key: cl[key] for key in ("ms_sums_median", "ms_sums_min_max", "sums_over_check")}
        line["scattered_over_contiguous"] = round(line["ms_sums_median"] / cl["ms_sums_median"], 2)
        if want_sklearn:
            t0 = time.perf_counter()
            w = silhouette_samples(host, group, metric="precomputed")
            ms = (time.perf_counter() - t0) * 1e3
            line["sklearn_ms"] = round(ms, 2)
            line["sklearn_over_device_wall"] = round(ms / line["ms_wall_median"], 2)
            line["max_abs_width_diff_vs_sklearn"] = float(np.abs(w - out["width"]).max())
        res["k"][str(k)] = line
    return res


def drive(args) -> int:
    me = os.path.abspath(__file__)
    tmp = os.path.join(os.path.dirname(os.path.abspath(args.out)), ".silhouette_bench_")
    os.makedirs(os.path.dirname(tmp), exist_ok=True)
    sizes = [int(x) for x in args.sizes.split(",")]
    steps = []
    for n in sizes:  # every GPU step under its own time limit; nothing starts after a step that failed
        reps = args.reps if n < 20000 else max(1, min(args.reps, 3))
        steps.append(f"timeout -k 10 {args.step_timeout} {sys.executable} {me} --measure --n {n} --ncol {args.ncol} "
                     f"--ks {args.ks} --reps {reps} --warmup {args.warmup} --seed {args.seed} "
                     f"--sklearn-max-n {args.sklearn_max_n} {'--no-sklearn ' if args.no_sklearn else ''}"
                     f"--out {tmp}{n}.json")
    rc = subprocess.call(["bash", "-c", "set -o pipefail; " + " && ".join(steps)])
    if rc != 0:
        print(f"a measuring step ended with status {rc}", file=sys.stderr)
        return rc
    res = {"tool": "silhouette_bench", "same_session": True, "sizes": []}
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
    ap.add_argument("--ks", default="2,50,2000", help="group counts, each a cut_tree(k=) of the complete-linkage tree")
    ap.add_argument("--n", type=int, default=24611)
    ap.add_argument("--ncol", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7, help="timed calls per k (at most 3 from n = 20,000 on)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--no-sklearn", action="store_true", help="skip the host yardstick")
    ap.add_argument("--sklearn-max-n", type=int, default=10000, help="no yardstick from this n on (8 n^2 bytes)")
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds per measuring process")
    ap.add_argument("--measure", action="store_true", help="one measuring process (the driver starts these)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectra", "silhouette_bench.json"))
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
