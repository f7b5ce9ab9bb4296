"""Neighbour-joining measurement: device.region_nj on the distances of
synthetic spectra, with and without compaction, beside the numpy reference of
tests/test_nj.py at the smallest size.

  python tools/nj_bench.py [--sizes 2000,8192,24611] [--out profiles/spectra/nj_bench.json]

The driver (no --measure) runs one measuring process per size, each under its
own `timeout`, chained so that nothing starts after a step that failed, and
merges their lines into --out.  The library must be built (__graft_entry__.build()).

A measuring process (--measure --n N) makes synthetic counts from a seeded
generator at ncol = 256, runs device.region_distances on them and then
device.region_nj --warmup + --reps times with compaction and as often
without, alternating, each call on a fresh device copy of the distances made
outside the timed part (keep_input=False: the call consumes its copy).
Reported per variant: the medians of the hipEvent phases of ks_nj_stats
(check, init, join), of the wall clock around the synchronous call, the join
time per step, and the bytes of the matrix k_nj_min read.

Those bytes are counted here from the returned tree: at every step the kernel
reads the row segment D(i, i+1 .. m-1) of every live row i of the m stored
ones, and the join table says which row dies (the second of the pair; rows
keep their order, so a node's row is the row of its first member).  Divided
by ms_join -- the whole step loop: k_nj_min, k_nj_join, the compactions and
the gaps between launches -- this is a LOWER bound of what k_nj_min achieves,
to set beside the 6.2 TB/s k_hclust_init reached on the same kind of row scan
(DESIGN.md 6h).  The reads of S are not counted.

The numpy reference (ref_nj, one host thread) is timed at n <= --ref-max only,
for scale; there its tree is also compared with the device's bit for bit.

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

MIN_DIM = 8  # ks_nj_dev: no compaction to fewer rows


def min_kernel_bytes(join: np.ndarray, n: int, compact: bool) -> int:
    """Bytes of D that k_nj_min reads over the n - 3 steps."""
    row_of = {}  # node code -> original row
    live = np.ones(n, dtype=bool)
    stored = np.arange(n)  # original rows of the stored matrix, in order
    pos = np.arange(n)     # original row -> stored index
    m = n
    seg = int((m - 1 - pos[live]).sum())  # entries of the live rows' segments
    total = 0
    for s in range(n - 3):
        total += seg
        a, b = (row_of[c] if c > 0 else -c - 1 for c in join[s].tolist())
        row_of[s + 1] = a
        live[b] = False
        seg -= m - 1 - int(pos[b])
        left = n - s - 1
        if compact and 2 * left <= m and left >= MIN_DIM:
            stored = stored[live[stored]]
            m = left
            pos[stored] = np.arange(m)
            seg = int((m - 1 - pos[stored]).sum())
    return 8 * total


def measure(args) -> dict:
    import torch

    from kmer_spans_amd import _lib, device as D
    assert torch.cuda.is_available(), "nj_bench needs a HIP device"
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
           "warmup": args.warmup, "seed": args.seed, "ms_distances": round(dst["ms_total"], 4), "variants": {}}
    variants = {"compact": True, "no_compact": False}
    stats = {v: [] for v in variants}
    wall = {v: [] for v in variants}
    trees = {}
    for r in range(args.warmup + args.reps):
        for name, compact in variants.items():  # alternating: both see the same machine
            work = dist.clone()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tree, st = D.region_nj(ctx, work, keep_input=False, compact=compact)
            if r >= args.warmup:
                wall[name].append((time.perf_counter() - t0) * 1e3)
                stats[name].append(st)
            trees[name] = tree
            del work
    same = all(np.array_equal(trees["compact"][k].view(np.uint8), trees["no_compact"][k].view(np.uint8))
               for k in ("join", "length", "root", "root_length"))
    res["variants_bit_equal"] = bool(same)
    for name, compact in variants.items():
        med = {key: float(np.median([s[key] for s in stats[name]])) for key in ("ms_total", "ms_check", "ms_init", "ms_join")}
        nbytes = min_kernel_bytes(trees[name]["join"], n, compact)
        res["variants"][name] = {
            "ms_check_median": round(med["ms_check"], 4), "ms_init_median": round(med["ms_init"], 4),
            "ms_join_median": round(med["ms_join"], 3),
            "ms_join_min_max": [round(min(s["ms_join"] for s in stats[name]), 3),
                                round(max(s["ms_join"] for s in stats[name]), 3)],
            "ms_total_median": round(med["ms_total"], 3), "ms_wall_median": round(float(np.median(wall[name])), 3),
            "us_per_step": round(med["ms_join"] * 1e3 / (n - 3), 3),
            "n_compactions": int(stats[name][-1]["n_compactions"]), "work_bytes": int(stats[name][-1]["work_bytes"]),
            "min_kernel_matrix_bytes": nbytes,
            "min_kernel_TBps_lower_bound": round(nbytes / (med["ms_join"] * 1e-3) / 1e12, 3),
            "negative_lengths": int((trees[name]["length"] < 0).sum())}
    if n <= args.ref_max:
        from tests.test_nj import ref_nj
        host = dist.cpu().numpy()
        t0 = time.perf_counter()
        want = ref_nj(host, n)
        ms = (time.perf_counter() - t0) * 1e3
        res["numpy_ref"] = {"ms": round(ms, 1), "threads": 1, "where": "the GPU machine's host CPU",
                            "over_device_wall": round(ms / res["variants"]["compact"]["ms_wall_median"], 2),
                            "bit_equal": bool(all(np.array_equal(np.ascontiguousarray(want[k]).view(np.uint8),
                                                                 trees["compact"][k].view(np.uint8))
                                                  for k in ("join", "length", "root", "root_length")))}
    return res


def drive(args) -> int:
    me = os.path.abspath(__file__)
    tmp = os.path.join(os.path.dirname(os.path.abspath(args.out)), ".nj_bench_")
    os.makedirs(os.path.dirname(tmp), exist_ok=True)
    sizes = [int(x) for x in args.sizes.split(",")]
    steps = []
    for n in sizes:  # every GPU step under its own time limit; nothing starts after a step that failed
        reps = args.reps if n < 20000 else max(1, min(args.reps, 2))
        steps.append(f"timeout -k 10 {args.step_timeout} {sys.executable} {me} --measure --n {n} --ncol {args.ncol} "
                     f"--reps {reps} --warmup {args.warmup} --seed {args.seed} --ref-max {args.ref_max} "
                     f"--out {tmp}{n}.json")
    rc = subprocess.call(["bash", "-c", "set -o pipefail; " + " && ".join(steps)])
    if rc != 0:
        print(f"a measuring step ended with status {rc}", file=sys.stderr)
        return rc
    res = {"tool": "nj_bench", "same_session": True, "sizes": []}
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
    ap.add_argument("--reps", type=int, default=3, help="timed calls per variant (at most 2 from n = 20,000 on)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--ref-max", type=int, default=2000, help="largest n at which the numpy reference is timed")
    ap.add_argument("--step-timeout", type=int, default=500, help="seconds per measuring process")
    ap.add_argument("--measure", action="store_true", help="one measuring process (the driver starts these)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectra", "nj_bench.json"))
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
