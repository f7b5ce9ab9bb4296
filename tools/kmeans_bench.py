"""k-means measurement: device.region_kmeans on synthetic spectra, beside
ks_spectra_cross_dist_dev on the same m x g x ncol shape (the same inner loop,
with the m x g output the assignment does not write) and a host Lloyd on one
thread.

  python tools/kmeans_bench.py [--sizes 24611,250000,1000000] [--gs 2,50,2000]
                               [--out profiles/spectra/kmeans_bench.json]

The driver (no --measure) runs one measuring process per size, each under its
own `timeout`, chained so that nothing starts after a step that failed, and
merges their lines into --out.  The library must be built (__graft_entry__.build()).

A measuring process (--measure --n N) makes synthetic counts from the seeded
generator of tools/spectra_dist_bench.py at ncol = 256 (in row blocks, the same
stream of draws per block) and, for each g, draws g distinct start rows and
  - runs device.region_kmeans(iter_max = --iter-max) --warmup + --reps times:
    the medians of the wall clock around the synchronous call, of ms_total,
    ms_normalise and ms_wss, the sums ms_assign and ms_update with the passes
    run, panel_bytes and work_bytes;
  - runs --iter-max single-pass calls (iter_max = 1), each started from the
    centres the one before returned: the same passes one by one, which gives
    the per-pass ms_assign and ms_update whose medians are reported (a call's
    stats hold only the sums over its passes);
  - times ks_spectra_cross_dist_dev (device.region_distances, squared, into a
    preallocated m x g output) on the rows against the start rows in the same
    process: `cross_dist_ms_distance_median`, and `assign_over_cross_dist`, the
    per-pass assignment over it.  Skipped where the output would exceed
    --cross-max-bytes;
  - runs the host Lloyd from the same start for the same number of passes where
    m * g <= --host-max-pairs: sklearn's KMeans(init=centres, n_init=1,
    algorithm="lloyd", tol=0) limited to one thread with threadpoolctl where
    both import, otherwise the numpy loop of tests/kmeansref.py.  The share of
    equal labels and the largest centre difference are reported.  (sklearn
    ends with an assignment to its final centres; R and this library return
    the labels the last centres were computed from.)

n = 24,611 is the reference's region list (test.R:762); its condensed matrix is
2.42 GB.  At 250,000 and 1,000,000 rows the matrix would be 250 GB and 4 TB:
there is no tree to compare with.
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


def synthetic_counts(n: int, ncol: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    out = np.empty((n, ncol), dtype=np.uint32)
    for r0 in range(0, n, 65536):
        r1 = min(r0 + 65536, n)
        block = rng.integers(0, 2000, size=(r1 - r0, ncol)).astype(np.uint32)
        block[rng.random((r1 - r0, ncol)) < 0.4] = 0
        out[r0:r1] = block
    out[:, 0] |= 1
    return out


def med(xs):
    return round(float(np.median(xs)), 4)


def host_lloyd(counts, start, passes: int) -> dict:
    """One thread on the host, from the same start."""
    from tests import kmeansref as R
    p = R.profiles(counts)
    init = p[start]
    try:
        import sklearn
        from sklearn.cluster import KMeans
        from threadpoolctl import threadpool_limits
    except ImportError:
        t0 = time.perf_counter()
        r = R.kmeans(counts, start, iter_max=passes)
        return {"what": "the numpy loop of tests/kmeansref.py", "ms": round((time.perf_counter() - t0) * 1e3, 1),
                "labels": r["cluster"], "centers": r["centers"], "passes": r["iter"]}
    with threadpool_limits(limits=1):
        t0 = time.perf_counter()
        km = KMeans(n_clusters=init.shape[0], init=init, n_init=1, algorithm="lloyd", tol=0, max_iter=passes).fit(p)
        ms = (time.perf_counter() - t0) * 1e3
    return {"what": f"sklearn {sklearn.__version__} KMeans(lloyd, tol=0), one thread (profiles made beforehand)",
            "ms": round(ms, 1), "labels": km.labels_ + 1, "centers": km.cluster_centers_, "passes": int(km.n_iter_)}


def measure(args) -> dict:
    import torch

    from kmer_spans_amd import _lib, device as D
    assert torch.cuda.is_available(), "kmeans_bench needs a HIP device"
    ctx = _lib.context(0)
    D.bind_torch_stream(ctx)
    n, ncol = args.n, args.ncol
    counts = synthetic_counts(n, ncol, args.seed)
    dev = torch.from_numpy(counts.view(np.int32)).cuda()
    res = {"n": n, "ncol": ncol, "build": _lib.build_id(), "device": torch.cuda.get_device_name(0),
           "reps": args.reps, "warmup": args.warmup, "seed": args.seed, "iter_max": args.iter_max,
           "condensed_matrix_bytes": 4 * n * (n - 1), "g": {}}
    rng = np.random.default_rng(args.seed + 1)
    for g in (int(x) for x in args.gs.split(",")):
        if g > n:
            continue
        start = np.sort(rng.choice(n, size=g, replace=False)).astype(np.int64)
        start_dev = torch.from_numpy(start).cuda()
        stats, wall, out = [], [], None
        for r in range(args.warmup + args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out, st = D.region_kmeans(ctx, dev, start_dev, iter_max=args.iter_max)
            if r >= args.warmup:
                wall.append((time.perf_counter() - t0) * 1e3)
                stats.append(st)
        last = stats[-1]
        line = {"passes": int(out["iter"]), "converged": bool(out["converged"]),
                "ms_wall_median": med(wall), "ms_total_median": med([s["ms_total"] for s in stats]),
                "ms_normalise_median": med([s["ms_normalise"] for s in stats]),
                "ms_assign_sum_median": med([s["ms_assign"] for s in stats]),
                "ms_update_sum_median": med([s["ms_update"] for s in stats]),
                "ms_wss_median": med([s["ms_wss"] for s in stats]),
                "panel_bytes": int(last["panel_bytes"]), "work_bytes": int(last["work_bytes"]),
                "tot_withinss": out["tot_withinss"], "totss": out["totss"],
                "smallest_group": int(out["size"].min()), "largest_group": int(out["size"].max())}
        # the same passes one by one
        cen, assign, update = start_dev, [], []
        for _ in range(int(out["iter"])):
            one, st = D.region_kmeans(ctx, dev, cen, iter_max=1)
            cen = one["centers"]
            assign.append(st["ms_assign"])
            update.append(st["ms_update"])
        same = bool(torch.equal(one["cluster"], out["cluster"]))
        line.update({"ms_assign_pass_median": med(assign), "ms_assign_pass_min_max": [round(min(assign), 4),
                                                                                        round(max(assign), 4)],
                     "ms_update_pass_median": med(update), "ms_update_pass_min_max": [round(min(update), 4),
                                                                                      round(max(update), 4)],
                     "single_passes_reach_the_same_labels": same,
                     "assign_ps_per_pair_column": round(med(assign) * 1e9 / (n * g * ncol), 4)})
        # yardstick 1: the existing cross-distance kernel on the same shape
        if 8 * n * g <= args.cross_max_bytes:
            buf = torch.empty((n, g), dtype=torch.float64, device="cuda")
            dd = []
            for r in range(args.warmup + args.reps):
                _, dst = D.region_distances(ctx, dev, None, start_dev, squared=True, out=buf)
                if r >= args.warmup:
                    dd.append(dst["ms_distance"])
            first = torch.argmin(buf, dim=1).to(torch.int32) + 1
            one, _ = D.region_kmeans(ctx, dev, start_dev, iter_max=1)
            line.update({"cross_dist_ms_distance_median": med(dd), "cross_dist_output_bytes": 8 * n * g,
                         "assign_over_cross_dist": round(med(assign) / med(dd), 3),
                         "first_pass_labels_equal_cross_dist_argmin": bool(torch.equal(first, one["cluster"]))})
            del buf
        else:
            line["cross_dist"] = f"skipped: the output would be {8 * n * g} bytes"
        # yardstick 2: a host Lloyd on one thread
        if n * g <= args.host_max_pairs and not args.no_host:
            h = host_lloyd(counts, start, int(out["iter"]))
            lab, cen_d = out["cluster"].cpu().numpy(), out["centers"].cpu().numpy()
            line["host"] = {"what": h["what"], "ms": h["ms"], "passes": h["passes"],
                            "host_over_device_wall": round(h["ms"] / line["ms_wall_median"], 1),
                            "labels_equal_share": round(float((h["labels"] == lab).mean()), 6),
                            "max_abs_centre_diff": float(np.abs(h["centers"] - cen_d).max())}
        elif not args.no_host:
            line["host"] = f"skipped: m * g = {n * g} exceeds --host-max-pairs"
        res["g"][str(g)] = line
    return res


def drive(args) -> int:
    me = os.path.abspath(__file__)
    tmp = os.path.join(os.path.dirname(os.path.abspath(args.out)), ".kmeans_bench_")
    os.makedirs(os.path.dirname(tmp), exist_ok=True)
    sizes = [int(x) for x in args.sizes.split(",")]
    steps = []
    for n in sizes:  # every GPU step under its own time limit; nothing starts after a step that failed
        steps.append(f"timeout -k 10 {args.step_timeout} {sys.executable} {me} --measure --n {n} --ncol {args.ncol} "
                     f"--gs {args.gs} --reps {args.reps} --warmup {args.warmup} --seed {args.seed} "
                     f"--iter-max {args.iter_max} --host-max-pairs {args.host_max_pairs} "
                     f"--cross-max-bytes {args.cross_max_bytes} {'--no-host ' if args.no_host else ''}"
                     f"--out {tmp}{n}.json")
    rc = subprocess.call(["bash", "-c", "set -o pipefail; " + " && ".join(steps)])
    if rc != 0:
        print(f"a measuring step ended with status {rc}", file=sys.stderr)
        return rc
    res = {"tool": "kmeans_bench", "same_session": True, "sizes": []}
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
    ap.add_argument("--sizes", default="24611,250000,1000000")
    ap.add_argument("--gs", default="2,50,2000", help="numbers of groups")
    ap.add_argument("--n", type=int, default=24611)
    ap.add_argument("--ncol", type=int, default=256)
    ap.add_argument("--iter-max", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3, help="timed full calls per g")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--no-host", action="store_true", help="skip the host Lloyd")
    ap.add_argument("--host-max-pairs", type=int, default=60_000_000, help="no host Lloyd where m * g exceeds this")
    ap.add_argument("--cross-max-bytes", type=int, default=32 << 30, help="no cross-distance run above this output size")
    ap.add_argument("--step-timeout", type=int, default=420, help="seconds per measuring process")
    ap.add_argument("--measure", action="store_true", help="one measuring process (the driver starts these)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectra", "kmeans_bench.json"))
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
