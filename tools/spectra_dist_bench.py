"""Pairwise-distance measurement: device.region_distances at the reference's
own list size, the tiled kernel beside the one-thread-per-pair comparison
build, in one GPU session.

  python tools/spectra_dist_bench.py [--no-build] [--out profiles/spectra/dist_bench.json]
  python tools/spectra_dist_bench.py --parent-lib PATH [--rounds 3] [--knn-k 10]
                                     [--out profiles/spectra/dist_metrics_bench.json]

The driver (no --measure) builds the library and the comparison library

  make -C kmer_spans_amd/csrc
  make -C kmer_spans_amd/csrc EXTRA=-DKS_DIST_NAIVE BUILD=build_distnaive \
       OUT=../libkmerspans_distnaive.so

(--no-build: both are already built from this tree), then runs one measuring
process per library, each under its own `timeout`, chained by && so that
nothing starts after a step that failed, and merges their lines into --out.

A measuring process (--measure) times, with synthetic counts from a seeded
generator:
  condensed  m = 24,611 rows (the reference's region list, test.R:762),
             ncol = 256: 302,838,355 distances, 2.42 GB of output;
  cross      65,536 rows against 64 rows at ncol = 256.
Median of --reps (20) calls after --warmup (3); the times are the hipEvent
phases of ks_dist_stats (normalise, distance) and the wall clock around the
synchronous call.  Rates: FP64 operations 3 * ncol * pairs / distance time
(one subtract, one multiply, one add per pair and column, none fused) and
output bytes 8 * pairs / distance time.  Bounds, and where they come from:
  FP64 vector  78.6 TFLOP/s is AMD's published peak for the MI355X, counted as
               fused multiply-adds (2 per lane and clock); this kernel may not
               fuse, so its ceiling is half of that, 39.3 T operations/s.
               Nobody has measured an FP64 vector rate in this repository.
  HBM          8 TB/s, the published peak (the output is written once).
2,000 random pairs of each form are compared with a host loop in the
contract's order (squared distances, bit for bit).  --host-m rows (2,000) are
also timed through scipy's pdist on the host, for orientation only.

Acceptance: the tiled kernel's distance time on the condensed case is below the
comparison build's from the same session ("ok"; exit status 1 otherwise).

--metric NAME (euclidean by default) times that metric of region_distances
instead.  The rate then counts the contract's FP64 operations
per pair and column -- euclidean and hellinger 3, manhattan and maximum 2,
canberra 4 (a sum, a difference, a division, an addition; the division is many
instructions) -- and the spot check uses the host model of tests/metricref.py
on the distances themselves (the squared form where the metric has one).
--knn-k K also times device.region_knn(K) in the self form on the condensed
case's rows and reports the medians of ms_select and ms_merge.

--parent-lib PATH is the driver of the metric measurement: PATH is
libkmerspans.so built from the parent commit, which knows euclidean only.  It
runs --rounds measuring processes of the parent's library and of this tree's
in alternation (euclidean), then one process per other metric with this
tree's, all in one session and chained as above, and writes the spread of each
library's euclidean medians and every metric's time as a multiple of this
tree's euclidean median.
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

FP64_FMA_FLOPS = 78.6e12   # AMD's published MI355X peak FP64 vector rate, FMA counted as two
FP64_UNFUSED_OPS = FP64_FMA_FLOPS / 2
HBM_BYTES_PER_S = 8.0e12
NAIVE_LIB = os.path.join(ROOT, "kmer_spans_amd", "libkmerspans_distnaive.so")
OPS_PER_COLUMN = {"euclidean": 3, "manhattan": 2, "maximum": 2, "canberra": 4, "hellinger": 3}


def host_sq(p: np.ndarray, i: np.ndarray, j: np.ndarray) -> np.ndarray:
    pt = np.ascontiguousarray(p.T)
    acc = np.zeros(i.size)
    for k in range(pt.shape[0]):
        d = pt[k][i] - pt[k][j]
        acc = acc + d * d
    return acc


def measure(args) -> dict:
    import torch

    from kmer_spans_amd import _lib, device as D
    assert torch.cuda.is_available(), "spectra_dist_bench needs a HIP device"
    ctx = _lib.context(0)
    D.bind_torch_stream(ctx)
    rng = np.random.default_rng(args.seed)
    ncol = args.ncol
    metric = args.metric
    squared = metric in ("euclidean", "hellinger")
    how = dict(squared=squared, metric=metric)  # euclidean is flags the parent commit's library knows too
    ops_per_column = OPS_PER_COLUMN[metric]

    def host_model(i, j):
        if metric == "euclidean":
            return host_sq(prof, i, j)
        from tests import metricref
        return metricref.result(metric, metricref.VALUE[metric](prof, i, j), squared=squared)
    n = max(args.m, args.cross_a)
    counts = rng.integers(0, 2000, size=(n, ncol)).astype(np.uint32)
    counts[rng.random((n, ncol)) < 0.4] = 0
    counts[:, 0] |= 1
    dc = torch.from_numpy(counts.view(np.int32)).cuda()
    prof = counts.astype(np.float64) / counts.sum(axis=1, dtype=np.uint64).astype(np.float64)[:, None]
    res = {"variant": args.variant, "build": _lib.build_id(), "lib": os.path.basename(_lib.LIB_PATH),
           "device": torch.cuda.get_device_name(0), "ncol": ncol, "reps": args.reps, "warmup": args.warmup,
           "seed": args.seed, "metric": metric, "squared": squared, "fp64_ops_per_column": ops_per_column}

    def timed(what, pairs, run, sample):
        stats, wall = [], []
        for r in range(args.warmup + args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out, st = run()
            torch.cuda.synchronize()
            if r >= args.warmup:
                wall.append((time.perf_counter() - t0) * 1e3)
                stats.append(st)
        med = {key: float(np.median([s[key] for s in stats])) for key in ("ms_total", "ms_normalise", "ms_distance")}
        t = med["ms_distance"] * 1e-3
        ops, byts = float(ops_per_column) * ncol * pairs / t, 8.0 * pairs / t
        line = {"pairs": pairs, "output_bytes": 8 * pairs, "panel_bytes": int(stats[-1]["panel_bytes"]),
                "ms_distance_median": round(med["ms_distance"], 4),
                "ms_distance_min_max": [round(min(s["ms_distance"] for s in stats), 4),
                                        round(max(s["ms_distance"] for s in stats), 4)],
                "ms_normalise_median": round(med["ms_normalise"], 4), "ms_total_median": round(med["ms_total"], 4),
                "ms_wall_median": round(float(np.median(wall)), 4),
                "fp64_ops_per_s": round(ops, 1), "fraction_of_unfused_fp64_peak": round(ops / FP64_UNFUSED_OPS, 4),
                "output_bytes_per_s": round(byts, 1), "fraction_of_8TBps": round(byts / HBM_BYTES_PER_S, 4)}
        line["nearer_bound"] = ("fp64" if line["fraction_of_unfused_fp64_peak"] >= line["fraction_of_8TBps"]
                                else "hbm_write")
        got, want = sample(out)
        line["spot_check"] = {"pairs": int(want.size),
                              "mismatches": int((got.view(np.uint64) != want.view(np.uint64)).sum())}
        res[what] = line

    # condensed
    m = args.m
    pairs = m * (m - 1) // 2
    out = torch.empty(pairs, dtype=torch.float64, device="cuda")
    si = rng.integers(0, m - 1, 2000)
    sj = np.minimum(si + 1 + (rng.random(2000) * (m - 1 - si)).astype(np.int64), m - 1)
    off = torch.from_numpy(si * m - si * (si + 1) // 2 + (sj - si - 1)).cuda()
    rows = torch.arange(m, device="cuda")
    timed("condensed", pairs, lambda: D.region_distances(ctx, dc, rows=rows, out=out, **how),
          lambda o: (o[off].cpu().numpy(), host_model(si, sj)))
    res["condensed"]["m"] = m
    del out
    # cross
    na, nb = args.cross_a, args.cross_b
    rb_host = rng.integers(0, n, nb)
    ra, rb = torch.arange(na, device="cuda"), torch.from_numpy(rb_host).cuda()
    out = torch.empty(na * nb, dtype=torch.float64, device="cuda")
    ci, cj = rng.integers(0, na, 2000), rng.integers(0, nb, 2000)
    coff = torch.from_numpy(ci * nb + cj).cuda()
    timed("cross", na * nb, lambda: D.region_distances(ctx, dc, rows=ra, rows_b=rb, out=out, **how),
          lambda o: (o.reshape(-1)[coff].cpu().numpy(), host_model(ci, rb_host[cj])))
    res["cross"]["na"], res["cross"]["nb"] = na, nb
    del out
    if args.knn_k > 0:
        stats = []
        for r in range(args.warmup + args.reps):
            _, _, st = D.region_knn(ctx, dc, args.knn_k, rows=rows, **how)
            if r >= args.warmup:
                stats.append(st)
        sel = [s["ms_select"] for s in stats]
        res["knn"] = {"m": m, "k": args.knn_k, "ms_select_median": round(float(np.median(sel)), 4),
                      "ms_select_min_max": [round(min(sel), 4), round(max(sel), 4)],
                      "ms_merge_median": round(float(np.median([s["ms_merge"] for s in stats])), 4),
                      "n_splits": int(stats[-1]["n_splits"])}
    if args.host_m > 0:
        try:
            from scipy.spatial.distance import pdist
            t0 = time.perf_counter()
            pdist(prof[:args.host_m])
            dt = time.perf_counter() - t0
            hp = args.host_m * (args.host_m - 1) // 2
            res["host_scipy_pdist"] = {"m": args.host_m, "pairs": hp, "ms": round(dt * 1e3, 2),
                                       "fp64_ops_per_s": round(3.0 * ncol * hp / dt, 1),
                                       "note": "orientation only, one host thread"}
        except ImportError:
            res["host_scipy_pdist"] = None
    return res


def drive(args) -> int:
    csrc = os.path.join(ROOT, "kmer_spans_amd", "csrc")
    if not args.no_build:
        subprocess.check_call(["make", "-s", "-j", "16", "-C", csrc])
        subprocess.check_call(["make", "-s", "-j", "16", "-C", csrc, "EXTRA=-DKS_DIST_NAIVE", "BUILD=build_distnaive",
                               "OUT=../libkmerspans_distnaive.so"])
    tmp = os.path.join(os.path.dirname(os.path.abspath(args.out)), ".dist_bench_")
    os.makedirs(os.path.dirname(tmp), exist_ok=True)
    common = (f"--measure --m {args.m} --ncol {args.ncol} --cross-a {args.cross_a} --cross-b {args.cross_b} "
              f"--reps {args.reps} --warmup {args.warmup} --seed {args.seed}")
    me = os.path.abspath(__file__)
    # every GPU step under its own time limit; nothing starts after a step that failed
    script = (f"set -o pipefail; "
              f"timeout -k 10 {args.step_timeout} {sys.executable} {me} {common} --variant tiled "
              f"--host-m {args.host_m} --out {tmp}tiled.json && "
              f"timeout -k 10 {args.step_timeout} env KS_LIB_PATH={NAIVE_LIB} {sys.executable} {me} {common} "
              f"--variant one_thread_per_pair --host-m 0 --out {tmp}naive.json")
    rc = subprocess.call(["bash", "-c", script])
    if rc != 0:
        print(f"a measuring step ended with status {rc}", file=sys.stderr)
        return rc
    parts = {}
    for name in ("tiled", "naive"):
        with open(f"{tmp}{name}.json") as f:
            parts[name] = json.load(f)
        os.remove(f"{tmp}{name}.json")
    t, nv = parts["tiled"], parts["naive"]
    res = {"tool": "spectra_dist_bench", "same_session": True, "built_here": not args.no_build,
           "bounds": {"fp64_vector_fma_flops": FP64_FMA_FLOPS, "fp64_unfused_ops": FP64_UNFUSED_OPS,
                      "hbm_bytes_per_s": HBM_BYTES_PER_S,
                      "source": "AMD's published MI355X peaks; no FP64 vector rate has been measured here"},
           "tiled": t, "one_thread_per_pair": nv}
    for form in ("condensed", "cross"):
        res[f"{form}_naive_over_tiled"] = round(nv[form]["ms_distance_median"] / t[form]["ms_distance_median"], 3)
    clean = all(parts[v][form]["spot_check"]["mismatches"] == 0 for v in parts for form in ("condensed", "cross"))
    res["ok"] = bool(t["condensed"]["ms_distance_median"] < nv["condensed"]["ms_distance_median"] and clean)
    text = json.dumps(res)
    print(text)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    return 0 if res["ok"] else 1


def drive_metrics(args) -> int:
    """The parent commit's library beside this tree's, euclidean, in alternation; then the other metrics."""
    tmp = os.path.join(os.path.dirname(os.path.abspath(args.out)), ".dist_metrics_")
    os.makedirs(os.path.dirname(tmp), exist_ok=True)
    me = os.path.abspath(__file__)
    common = (f"--measure --m {args.m} --ncol {args.ncol} --cross-a {args.cross_a} --cross-b {args.cross_b} "
              f"--reps {args.reps} --warmup {args.warmup} --seed {args.seed} --host-m 0 --knn-k {args.knn_k}")
    runs = []  # (label, variant, metric, environment)
    for r in range(args.rounds):
        runs.append((f"parent_{r}", "parent", "euclidean", f"env KS_LIB_PATH={os.path.abspath(args.parent_lib)} "))
        runs.append((f"this_{r}", "this", "euclidean", ""))
    runs += [(metric, "this", metric, "") for metric in ("manhattan", "maximum", "canberra", "hellinger")]
    # every GPU step under its own time limit; nothing starts after a step that failed
    script = "set -o pipefail; " + " && ".join(
        f"timeout -k 10 {args.step_timeout} {env}{sys.executable} {me} {common} --variant {variant} "
        f"--metric {metric} --out {tmp}{label}.json" for label, variant, metric, env in runs)
    rc = subprocess.call(["bash", "-c", script])
    if rc != 0:
        print(f"a measuring step ended with status {rc}", file=sys.stderr)
        return rc
    lines = {}
    for label, _, _, _ in runs:
        with open(f"{tmp}{label}.json") as f:
            lines[label] = json.load(f)
        os.remove(f"{tmp}{label}.json")

    def spread(variant, pick):
        v = [pick(lines[f"{variant}_{r}"]) for r in range(args.rounds)]
        return {"medians": v, "min": min(v), "median": round(float(np.median(v)), 4), "max": max(v)}
    res = {"tool": "spectra_dist_bench", "same_session": True, "alternating_rounds": args.rounds, "m": args.m,
           "ncol": args.ncol, "reps": args.reps, "warmup": args.warmup,
           "builds": {"parent": lines["parent_0"]["build"], "this": lines["this_0"]["build"]},
           "device": lines["this_0"]["device"], "euclidean": {}, "metrics": {}}
    picks = {"condensed_ms_distance": lambda x: x["condensed"]["ms_distance_median"],
             "cross_ms_distance": lambda x: x["cross"]["ms_distance_median"]}
    if args.knn_k > 0:
        picks["knn_ms_select"] = lambda x: x["knn"]["ms_select_median"]
    for name, pick in picks.items():
        res["euclidean"][name] = {v: spread(v, pick) for v in ("parent", "this")}
    base = {name: res["euclidean"][name]["this"]["median"] for name in picks}
    clean = True
    for label, x in lines.items():
        clean = clean and all(x[form]["spot_check"]["mismatches"] == 0 for form in ("condensed", "cross"))
    for metric in ("manhattan", "maximum", "canberra", "hellinger"):
        x = lines[metric]
        res["metrics"][metric] = {
            "fp64_ops_per_column": x["fp64_ops_per_column"], "condensed": x["condensed"], "cross": x["cross"],
            "knn": x.get("knn"),
            "over_euclidean": {name: round(pick(x) / base[name], 3) for name, pick in picks.items()}}
    # the euclidean kernels stay inside the parent's own spread of this session
    res["euclidean_within_parent_spread"] = {
        name: bool(res["euclidean"][name]["this"]["median"] <= res["euclidean"][name]["parent"]["max"])
        for name in picks}
    res["spot_checks_clean"] = clean
    res["ok"] = bool(clean)
    text = json.dumps(res)
    print(text)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    return 0 if res["ok"] else 1


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=24611)
    ap.add_argument("--ncol", type=int, default=256)
    ap.add_argument("--cross-a", type=int, default=65536)
    ap.add_argument("--cross-b", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--host-m", type=int, default=2000, help="rows timed through scipy's pdist on the host (0: none)")
    ap.add_argument("--no-build", action="store_true", help="both libraries are already built from this tree")
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds per measuring process")
    ap.add_argument("--measure", action="store_true", help="one measuring process (the driver starts these)")
    ap.add_argument("--variant", default="tiled", help="label of the library build measured")
    ap.add_argument("--metric", default="euclidean", choices=sorted(OPS_PER_COLUMN),
                    help="the metric a measuring process times")
    ap.add_argument("--knn-k", type=int, default=0, help="also time region_knn at this k (0: not)")
    ap.add_argument("--parent-lib", default=None,
                    help="the parent commit's libkmerspans.so: the driver of the metric measurement")
    ap.add_argument("--rounds", type=int, default=3, help="alternating runs of each library with --parent-lib")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "spectra",
                                "dist_metrics_bench.json" if args.parent_lib else "dist_bench.json")
    if args.parent_lib and not args.measure:
        return drive_metrics(args)
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
