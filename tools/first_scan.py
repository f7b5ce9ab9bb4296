"""First scan of a DeviceSeqs: what a caller who scans a genome once pays.

One genome, one count, one table; then N scans, each through a new DeviceSeqs
object over the same tensors, so each has a new sequence index and is a build
(run segmentation, layout, chunk table, predictor).  Prints one JSON line with
the wall time and the phase times of every scan and their medians.

  python tools/first_scan.py --scans 8 --out first_scan.json
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--scans", type=int, default=8)
    p.add_argument("--k", type=int, default=13)
    p.add_argument("--score", default="log2")
    p.add_argument("--scale", type=float, default=1.0)
    p.add_argument("--ncontigs", type=int, default=24)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import torch
    from kmer_spans_amd import _lib, device as D, genome
    ctx = _lib.context(0)
    D.bind_torch_stream(ctx)
    parts, lens = genome.human_like(scale=a.scale, seed=1, device="cuda", ncontigs=a.ncontigs)
    ds = D.from_parts(parts, lens, "cuda")
    del parts
    counts = torch.zeros(4 ** a.k, dtype=torch.int32, device="cuda")
    words = D.count(ctx, ds, a.k, counts)
    tab = D.DeviceTable.from_counts(ctx, counts, a.k, a.score, total=words, thr=0.75 if a.score == "rank" else 0.0,
                                    expand=True)
    D.scan(ctx, ds, a.k, tab, 100, 20.0)  # workspace growth, code objects
    keys = ("ms_total", "ms_runs", "ms_layout", "ms_scan", "ms_predict", "ms_carry", "ms_stitch", "ms_rescan",
            "ms_finish")
    wall, phases = [], []
    for _ in range(a.scans):
        fresh = D.DeviceSeqs(ds.seq, ds.offsets, ds.offsets_dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pos, sc, st = D.scan(ctx, fresh, a.k, tab, 100, 20.0)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        assert st["ms_runs"] > 0 and fresh.seq_index().info()["builds"] == 1
        phases.append({key: round(st[key], 3) for key in keys})
    out = {"build_id": _lib.build_id(), "genome_bp": int(ds.total),
           "regions": int(pos.shape[1]), "wall_ms": [round(x, 3) for x in wall],
           "median_wall_ms": round(statistics.median(wall), 3),
           "median_phase_ms": {key: round(statistics.median(ph[key] for ph in phases), 3) for key in keys}}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    tab.close()


if __name__ == "__main__":
    main()
