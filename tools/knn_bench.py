"""Nearest-neighbour measurement: device.region_knn (self form) on synthetic
spectra, beside the only other route to the same lists -- region_distances into
query-row blocks followed by torch.topk -- and beside ks_spectra_cross_dist_dev
alone on the same na x nb x ncol shape.

  python tools/knn_bench.py [--shapes 24611:1,24611:10,24611:64,250000:10]
                            [--out profiles/spectra/knn_bench.json]

The driver (no --measure) runs one measuring process per size, each under its
own `timeout`, chained so that nothing starts after a step that failed, and
merges their lines into --out.  The library must be built (__graft_entry__.build()).

A measuring process (--measure --n N --ks K,K,..) makes synthetic counts from
the seeded generator of tools/spectra_dist_bench.py at ncol = 256 and, in one
process:
  - for each k runs device.region_knn(k, squared=True) --warmup + --reps times:
    the medians of the wall clock around the synchronous call and of ms_total,
    ms_normalise, ms_select and ms_merge, with n_splits, panel_bytes, work_bytes;
  - yardstick (b), once per size: ks_spectra_cross_dist_dev (device.
    region_distances, squared, into one preallocated block of at most
    --block-bytes) over all query rows, block by block: the sum of the blocks'
    ms_distance (the kernel alone; the same pairs, with the na x nb output the
    selection does not write).  `select_over_cross_dist` = ms_select over it;
  - yardstick (a), for each k: the same blocks, each followed by masking the
    block's diagonal and torch.topk(k, largest=False, sorted=True): the wall
    clock over all blocks, synchronised at the end.  `knn_over_blocks_topk` =
    the call's wall clock over it.  The distances of the two routes are compared
    bit for bit (torch's tie order is not this library's, so not the indices).
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

from tools.kmeans_bench import med, synthetic_counts  # noqa: E402


def measure(args) -> dict:
    import torch

    from kmer_spans_amd import _lib, device as D
    assert torch.cuda.is_available(), "knn_bench needs a HIP device"
    ctx = _lib.context(0)
    D.bind_torch_stream(ctx)
    n, ncol = args.n, args.ncol
    dev = torch.from_numpy(synthetic_counts(n, ncol, args.seed).view(np.int32)).cuda()
    every = torch.arange(n, dtype=torch.int64, device="cuda")
    brows = max(1, min(n, args.block_bytes // (8 * n)))
    buf = torch.empty(brows * n, dtype=torch.float64, device="cuda")
    blocks = [(r0, min(r0 + brows, n)) for r0 in range(0, n, brows)]
    res = {"n": n, "ncol": ncol, "form": "self", "ordered_pairs": n * (n - 1), "build": _lib.build_id(),
           "device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup, "seed": args.seed,
           "dense_matrix_bytes": 8 * n * n, "block_rows": brows, "blocks": len(blocks), "k": {}}

    def by_blocks(k):
        """(kernel ms summed over the blocks, [n, k] top-k values or None): k None = the distances alone."""
        ms, vals = 0.0, []
        for r0, r1 in blocks:
            out = buf[:(r1 - r0) * n]
            block, st = D.region_distances(ctx, dev, every[r0:r1], every, squared=True, out=out)
            ms += st["ms_distance"]
            if k is not None:
                block[torch.arange(r1 - r0, device="cuda"), every[r0:r1]] = float("inf")  # the query itself
                vals.append(torch.topk(block, k, dim=1, largest=False, sorted=True).values)
        return ms, (torch.cat(vals) if k is not None else None)

    cross = []
    for r in range(args.warmup + args.reps):
        ms, _ = by_blocks(None)
        if r >= args.warmup:
            cross.append(ms)
    res["cross_dist_ms_distance_median"] = med(cross)
    for k in (int(x) for x in args.ks.split(",")):
        stats, wall, dist = [], [], None
        for r in range(args.warmup + args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, dist, st = D.region_knn(ctx, dev, k, squared=True)
            if r >= args.warmup:
                wall.append((time.perf_counter() - t0) * 1e3)
                stats.append(st)
        topk_wall, vals = [], None
        for r in range(args.warmup + args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, vals = by_blocks(k)
            torch.cuda.synchronize()
            if r >= args.warmup:
                topk_wall.append((time.perf_counter() - t0) * 1e3)
        last = stats[-1]
        sel = med([s["ms_select"] for s in stats])
        res["k"][str(k)] = {
            "ms_wall_median": med(wall), "ms_total_median": med([s["ms_total"] for s in stats]),
            "ms_normalise_median": med([s["ms_normalise"] for s in stats]), "ms_select_median": sel,
            "ms_merge_median": med([s["ms_merge"] for s in stats]), "n_splits": int(last["n_splits"]),
            "tiles_per_split": int(last["tiles_per_split"]), "panel_bytes": int(last["panel_bytes"]),
            "work_bytes": int(last["work_bytes"]),
            "select_ps_per_pair_column": round(sel * 1e9 / (n * n * ncol), 4),
            "select_over_cross_dist": round(sel / med(cross), 3),
            "blocks_topk_ms_wall_median": med(topk_wall),
            "knn_over_blocks_topk": round(med(wall) / med(topk_wall), 3),
            "distances_equal_blocks_topk": bool(torch.equal(vals.view(torch.int64), dist.view(torch.int64)))}
        del vals, dist
    return res


def drive(args) -> int:
    me = os.path.abspath(__file__)
    tmp = os.path.join(os.path.dirname(os.path.abspath(args.out)), ".knn_bench_")
    os.makedirs(os.path.dirname(tmp), exist_ok=True)
    sizes: dict[int, list[int]] = {}
    for shape in args.shapes.split(","):
        n, k = (int(x) for x in shape.split(":"))
        sizes.setdefault(n, []).append(k)
    steps = []
    for n, ks in sizes.items():  # every GPU step under its own time limit; nothing starts after a step that failed
        steps.append(f"timeout -k 10 {args.step_timeout} {sys.executable} {me} --measure --n {n} --ncol {args.ncol} "
                     f"--ks {','.join(str(k) for k in ks)} --reps {args.reps} --warmup {args.warmup} "
                     f"--seed {args.seed} --block-bytes {args.block_bytes} --out {tmp}{n}.json")
    rc = subprocess.call(["bash", "-c", "set -o pipefail; " + " && ".join(steps)])
    if rc != 0:
        print(f"a measuring step ended with status {rc}", file=sys.stderr)
        return rc
    res = {"tool": "knn_bench", "same_session": True, "sizes": []}
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
    ap.add_argument("--shapes", default="24611:1,24611:10,24611:64,250000:10", help="n:k, self form")
    ap.add_argument("--n", type=int, default=24611)
    ap.add_argument("--ks", default="10")
    ap.add_argument("--ncol", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3, help="timed calls per shape")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--block-bytes", type=int, default=8 << 30, help="the query-row block of the distance route")
    ap.add_argument("--step-timeout", type=int, default=420, help="seconds per measuring process")
    ap.add_argument("--measure", action="store_true", help="one measuring process (the driver starts these)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectra", "knn_bench.json"))
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
