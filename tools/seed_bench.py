"""Seeding measurement: device.region_kmeans_seed (maximin and k-means++) on
synthetic spectra, beside one read of the profile panel, one assignment pass of
device.region_kmeans on the same (m, g), sklearn's kmeans_plusplus on one host
thread, and the Lloyd runs the seeds lead to.

  python tools/seed_bench.py [--sizes 24611,250000,1000000] [--gs 2,50,2000]
                             [--out profiles/spectra/seed_bench.json]

The driver (no --measure) runs one measuring process per size, each under its
own `timeout`, chained so that nothing starts after a step that failed, and
merges their lines into --out.  The library must be built (__graft_entry__.build()).

A measuring process (--measure --n N) makes the synthetic counts of
tools/kmeans_bench.py at ncol = 256 and, for each g and each method,
  - runs device.region_kmeans_seed --warmup + --reps times (maximin from row 0;
    k-means++ with seed 0 and a drawn first row): the medians of the wall clock
    around the synchronous call, of ms_total, ms_normalise and ms_steps, and
    ms_steps / g, the time of one step (a select and a pass over the panel);
  - `panel_read_ms`: the median time of torch.sum over a float64 [m, ncol]
    tensor, 8 m ncol bytes read once (a torch reduction, not a kernel of this
    library), and `step_over_panel_read`, with the step's bytes per second;
  - `kmeans_assign_pass_ms`: the median ms_assign of device.region_kmeans(
    iter_max = 1) started from the picked rows: the same m x g x ncol
    arithmetic in one launch with tile reuse, and `call_over_assign_pass`;
  - where m * g <= --host-max-pairs, sklearn.cluster.kmeans_plusplus(p, g,
    n_local_trials = 1) on the profiles (made beforehand) limited to one
    thread with threadpoolctl: `host_ms` and `host_over_device_wall`.
For g = --lloyd-g it then runs device.region_kmeans(iter_max = --lloyd-iter)
from the maximin rows, from the k-means++ rows of seeds 0 .. 4 and from the g
distinct random rows tools/kmeans_bench.py starts from, and reports
tot_withinss, iter and converged of each.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from kmeans_bench import med, synthetic_counts  # noqa: E402


def host_kmeanspp(p, g: int):
    try:
        import sklearn
        from sklearn.cluster import kmeans_plusplus
        from threadpoolctl import threadpool_limits
    except ImportError as e:
        return f"skipped: {e}"
    with threadpool_limits(limits=1):
        t0 = time.perf_counter()
        kmeans_plusplus(p, g, n_local_trials=1, random_state=0)
        ms = (time.perf_counter() - t0) * 1e3
    return {"what": f"sklearn {sklearn.__version__} kmeans_plusplus(n_local_trials=1), one thread (profiles made "
                    "beforehand)", "ms": round(ms, 1)}


def measure(args) -> dict:
    import torch

    from kmer_spans_amd import _lib, device as D
    assert torch.cuda.is_available(), "seed_bench needs a HIP device"
    ctx = _lib.context(0)
    D.bind_torch_stream(ctx)
    n, ncol = args.n, args.ncol
    counts = synthetic_counts(n, ncol, args.seed)
    dev = torch.from_numpy(counts.view(np.int32)).cuda()
    res = {"n": n, "ncol": ncol, "build": _lib.build_id(), "device": torch.cuda.get_device_name(0),
           "reps": args.reps, "warmup": args.warmup, "seed": args.seed, "g": {}}
    # one read of 8 m ncol bytes
    x = torch.ones((n, ncol), dtype=torch.float64, device="cuda")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    reads = []
    for r in range(2 + 5):
        ev[0].record()
        x.sum()
        ev[1].record()
        torch.cuda.synchronize()
        if r >= 2:
            reads.append(ev[0].elapsed_time(ev[1]))
    del x
    res["panel_read_ms"] = med(reads)
    res["panel_bytes"] = 8 * n * ncol
    rng = np.random.default_rng(args.seed + 1)  # the start rows of tools/kmeans_bench.py, drawn in its order
    p = None
    for g in (int(v) for v in args.gs.split(",")):
        if g > n:
            continue
        random_start = np.sort(rng.choice(n, size=g, replace=False)).astype(np.int64)
        line = {}
        for method, kw in (("maximin", {"first": 0}), ("kmeans++", {"seed": 0, "first": None})):
            stats, wall, out = [], [], None
            for r in range(args.warmup + args.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out, st = D.region_kmeans_seed(ctx, dev, g, method=method, **kw)
                if r >= args.warmup:
                    wall.append((time.perf_counter() - t0) * 1e3)
                    stats.append(st)
            step = med([s["ms_steps"] for s in stats]) / g
            ml = {"ms_wall_median": med(wall), "ms_total_median": med([s["ms_total"] for s in stats]),
                  "ms_normalise_median": med([s["ms_normalise"] for s in stats]),
                  "ms_steps_median": med([s["ms_steps"] for s in stats]), "ms_per_step": round(step, 5),
                  "step_over_panel_read": round(step / res["panel_read_ms"], 3),
                  "step_bytes_per_second": round(8 * n * ncol / (step * 1e-3)),
                  "n_launches": int(stats[-1]["n_launches"]), "work_bytes": int(stats[-1]["work_bytes"]),
                  "n_distinct": int(out["n_distinct"]), "potential_final": out["potential_final"],
                  "radius": out["radius"]}
            assign = []
            for r in range(args.warmup + args.reps):
                _, kst = D.region_kmeans(ctx, dev, out["rows"], iter_max=1)
                if r >= args.warmup:
                    assign.append(kst["ms_assign"])
            ml["kmeans_assign_pass_ms"] = med(assign)
            ml["call_over_assign_pass"] = round(ml["ms_total_median"] / med(assign), 2)
            line[method] = ml
        if n * g <= args.host_max_pairs and not args.no_host:
            if p is None:
                from tests import kmeansref as R
                p = R.profiles(counts)
            h = host_kmeanspp(p, g)
            if isinstance(h, dict):
                h["host_over_device_wall"] = round(h["ms"] / line["kmeans++"]["ms_wall_median"], 1)
            line["host"] = h
        elif not args.no_host:
            line["host"] = f"skipped: m * g = {n * g} exceeds --host-max-pairs"
        if g == args.lloyd_g:
            starts = [("maximin", D.region_kmeans_seed(ctx, dev, g, method="maximin")[0]["rows"])]
            starts += [(f"kmeans++ seed {s}",
                        D.region_kmeans_seed(ctx, dev, g, method="kmeans++", seed=s, first=None)[0]["rows"])
                       for s in range(5)]
            starts.append(("random distinct rows", torch.from_numpy(random_start).cuda()))
            line["lloyd"] = {"iter_max": args.lloyd_iter, "runs": []}
            for name, start in starts:
                km, kst = D.region_kmeans(ctx, dev, start, iter_max=args.lloyd_iter)
                line["lloyd"]["runs"].append({"start": name, "tot_withinss": km["tot_withinss"], "iter": int(km["iter"]),
                                              "converged": bool(km["converged"]), "totss": km["totss"],
                                              "smallest_group": int(km["size"].min()),
                                              "ms_total": round(kst["ms_total"], 3)})
        res["g"][str(g)] = line
    return res


def drive(args) -> int:
    me = os.path.abspath(__file__)
    tmp = os.path.join(os.path.dirname(os.path.abspath(args.out)), ".seed_bench_")
    os.makedirs(os.path.dirname(tmp), exist_ok=True)
    sizes = [int(v) for v in args.sizes.split(",")]
    steps = []
    for n in sizes:  # every GPU step under its own time limit; nothing starts after a step that failed
        steps.append(f"timeout -k 10 {args.step_timeout} {sys.executable} {me} --measure --n {n} --ncol {args.ncol} "
                     f"--gs {args.gs} --reps {args.reps} --warmup {args.warmup} --seed {args.seed} "
                     f"--lloyd-g {args.lloyd_g} --lloyd-iter {args.lloyd_iter} "
                     f"--host-max-pairs {args.host_max_pairs} {'--no-host ' if args.no_host else ''}"
                     f"--out {tmp}{n}.json")
    rc = subprocess.call(["bash", "-c", "set -o pipefail; " + " && ".join(steps)])
    if rc != 0:
        print(f"a measuring step ended with status {rc}", file=sys.stderr)
        return rc
    res = {"tool": "seed_bench", "same_session": True, "sizes": []}
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
    ap.add_argument("--gs", default="2,50,2000", help="numbers of centres")
    ap.add_argument("--n", type=int, default=24611)
    ap.add_argument("--ncol", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3, help="timed calls per g and method")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--lloyd-g", type=int, default=50, help="the g whose seeds are run through region_kmeans")
    ap.add_argument("--lloyd-iter", type=int, default=50)
    ap.add_argument("--no-host", action="store_true", help="skip sklearn's kmeans_plusplus")
    ap.add_argument("--host-max-pairs", type=int, default=60_000_000, help="no host run where m * g exceeds this")
    ap.add_argument("--step-timeout", type=int, default=420, help="seconds per measuring process")
    ap.add_argument("--measure", action="store_true", help="one measuring process (the driver starts these)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectra", "seed_bench.json"))
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
