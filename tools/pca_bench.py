"""Principal-component measurement: device.region_pca at the reference's own
list size, per stage, beside numpy's SVD on one host thread.

  python tools/pca_bench.py [--out profiles/spectra/pca_bench.json]

Synthetic counts from the seeded generator of tools/spectra_dist_bench.py.
Cases: m = 2,000 and m = 24,611 rows (the reference's region list, test.R:762)
at ncol = 256, centred and uncentred (test.R:811 and :735), and m = 8,192 at
ncol = 1024, the cap.  Per case the median of --reps (5) calls after --warmup
(1): the hipEvent stages of ks_pca_stats (normalise + centre, G, eigen,
projection), the sweep and rotation counts, and the wall clock around the
synchronous call, scores included, all ncol components.

For orientation only: np.linalg.svd(xc, full_matrices=False) of the same
(centred) profile matrix in a child process held to one thread, and the
largest difference between its singular values and the device's
sdev * sqrt(m - 1), relative to the largest.  There is no pass/fail threshold
on time; the exit status is 0 unless a step fails.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [(2000, 256, True), (2000, 256, False), (24611, 256, True), (24611, 256, False), (8192, 1024, True)]
ONE_THREAD = {"OMP_NUM_THREADS": "1", "OPENBLAS_NUM_THREADS": "1", "MKL_NUM_THREADS": "1"}


def synth(seed: int, n: int, ncol: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, 2000, size=(n, ncol)).astype(np.uint32)
    counts[rng.random((n, ncol)) < 0.4] = 0
    counts[:, 0] |= 1
    return counts


def host_svd(args) -> int:
    """Child process (one thread, no GPU): time numpy's SVD of the profile matrix."""
    counts = synth(args.seed, args.m, args.ncol)
    p = counts.astype(np.float64) / counts.sum(axis=1, dtype=np.uint64).astype(np.float64)[:, None]
    xc = p - p.mean(axis=0) if args.center else p
    t0 = time.perf_counter()
    sv = np.linalg.svd(xc, full_matrices=False, compute_uv=True)[1]
    ms = (time.perf_counter() - t0) * 1e3
    np.save(args.out, np.concatenate([[ms], sv]))
    return 0


def measure(args) -> dict:
    import torch

    from kmer_spans_amd import _lib, device as D
    assert torch.cuda.is_available(), "pca_bench needs a HIP device"
    ctx = _lib.context(0)
    D.bind_torch_stream(ctx)
    res = {"tool": "pca_bench", "build": _lib.build_id(), "device": torch.cuda.get_device_name(0),
           "reps": args.reps, "warmup": args.warmup, "seed": args.seed, "cases": []}
    stages = ("ms_total", "ms_normalise", "ms_gram", "ms_eigen", "ms_project")
    for m, ncol, center in CASES:
        counts = synth(args.seed, m, ncol)
        dc = torch.from_numpy(counts.view(np.int32)).cuda()
        stats, wall, out = [], [], None
        for r in range(args.warmup + args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out, st = D.region_pca(ctx, dc, center=center)
            torch.cuda.synchronize()
            if r >= args.warmup:
                wall.append((time.perf_counter() - t0) * 1e3)
                stats.append(st)
        line = {"m": m, "ncol": ncol, "center": center, "n_sweeps": int(stats[-1]["n_sweeps"]),
                "n_rotations": int(stats[-1]["n_rotations"]), "work_bytes": int(stats[-1]["panel_bytes"]),
                "ms_wall_median": round(float(np.median(wall)), 3)}
        for key in stages:
            line[key + "_median"] = round(float(np.median([s[key] for s in stats])), 4)
        line["ms_eigen_per_round_us"] = round(1e3 * line["ms_eigen_median"] / (line["n_sweeps"] * (ncol - 1)), 3)
        sdev = out["sdev"].cpu().numpy()
        del out, dc
        if not args.no_host:
            with tempfile.TemporaryDirectory() as tmp:
                path = os.path.join(tmp, "svd.npy")
                cmd = [sys.executable, os.path.abspath(__file__), "--host-svd", "--m", str(m), "--ncol", str(ncol),
                       "--seed", str(args.seed), "--out", path] + (["--center"] if center else [])
                subprocess.check_call(cmd, env={**os.environ, **ONE_THREAD}, timeout=args.host_timeout)
                got = np.load(path)
            sv = got[1:]
            line["host_numpy_svd"] = {"ms": round(float(got[0]), 1), "threads": 1, "note": "orientation only",
                                      "max_singular_value_difference_relative":
                                          float(np.abs(sdev * np.sqrt(m - 1.0) - sv).max() / sv[0])}
        res["cases"].append(line)
        print(json.dumps(line), flush=True)
    return res


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--no-host", action="store_true", help="skip the host SVD")
    ap.add_argument("--host-timeout", type=int, default=240, help="seconds per host SVD")
    ap.add_argument("--host-svd", action="store_true", help="the child process that times numpy's SVD")
    ap.add_argument("--m", type=int, default=0)
    ap.add_argument("--ncol", type=int, default=0)
    ap.add_argument("--center", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectra", "pca_bench.json"))
    args = ap.parse_args()
    if args.host_svd:
        return host_svd(args)
    res = measure(args)
    text = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
