"""Per-region spectra measurement: device.region_spectra on the region lists
the benchmark's genome produces, against the scan step that produced them.

  python tools/spectra_bench.py [--scale 1.0] [--k 13] [--q 4] [--out f.json]

On the human-shaped genome of bench.py, counts k-mers, then for the
weighted-rank table (thr 0.75) and for the log-ratio table: one device.scan
(timed: median of --reps steps after --warmup), then device.region_spectra on
the regions it returned (q-mers, both strands, entropy on; the same reps,
median wall clock around the synchronous call, and the hipEvent phases of
ks_spectra_stats).  --check random rows of each list (200) are compared with
a host count of the same substrings, as far as --check-bases (60 Mbases of
substrings per list) goes: a list of giant regions gets fewer rows checked, and
the output says how many ("spot_check": rows, bases).  The algorithmic bytes of the spectra are the bases
covered plus the rows written once and read once by the entropy pass:
sum(widths) + 2 * n * 4^q * 4 B; the rate is given against 8 TB/s.

A second block times four lists of equal size whose intervals are pure A,
(CA)n, (CAG)n and random sequence: the bins 64 lanes contend for.  To measure
what the count kernel's per-lane run lengths are worth, build the comparison
library that does one LDS add per word and time this block alone with it:

  make -C kmer_spans_amd/csrc EXTRA=-DKS_SPECTRA_NO_RLE BUILD=build_norle \
       OUT=../libkmerspans_norle.so
  KS_LIB_PATH=kmer_spans_amd/libkmerspans_norle.so \
       python tools/spectra_bench.py --contended-only --variant add_per_word

Acceptance: on each list the median spectra time is no longer than the median
scan step ("ok" in the output; the exit status is 1 otherwise).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from kmer_spans_amd import _lib, device as D, genome  # noqa: E402

HBM_BYTES_PER_S = 8.0e12


def rc_perm(q: int) -> np.ndarray:
    c = np.arange(4 ** q)
    r = np.zeros_like(c)
    for _ in range(q):
        r = (r << 2) | ((c & 3) ^ 2)
        c = c >> 2
    return r


def host_row(sub: np.ndarray, q: int, both: bool) -> np.ndarray:
    """The spectrum of one substring (uint8 array) counted on the host."""
    row = np.zeros(4 ** q, dtype=np.int64)
    n = sub.size - q + 1
    if n > 0:
        e = ((sub >> 1) & 3).astype(np.int64)
        isn = np.concatenate(([0], np.cumsum((sub | 0x20) == ord("n"))))
        code = np.zeros(n, dtype=np.int64)
        for j in range(q):
            code = (code << 2) | e[j:j + n]
        ok = (isn[q:q + n] - isn[:n]) == 0
        row += np.bincount(code[ok], minlength=4 ** q)
    return row + row[rc_perm(q)] if both else row


def median_ms(fn, reps: int, warmup: int):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts, last = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        last = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), ts, last


def spectra_line(ctx, ds, pos, q, reps, warmup, check, check_bases, rng):
    n = int(pos.shape[1])
    out = torch.empty((n, 4 ** q), dtype=torch.int32, device="cuda")
    pos_dev = torch.from_numpy(np.ascontiguousarray(pos)).cuda()
    stats = []

    def run_numpy():
        r = D.region_spectra(ctx, ds, pos, q=q, both_strands=True, entropy=True, out=out)
        stats.append(r[2])
        return r

    def run_dev():
        return D.region_spectra(ctx, ds, pos_dev, q=q, both_strands=True, entropy=True, out=out)
    ms, all_ms, (counts, ent, st) = median_ms(run_numpy, reps, warmup)
    ms_dev, _, _ = median_ms(run_dev, reps, 1)
    timed = stats[-reps:]
    phases = {key: round(float(np.median([s[key] for s in timed])), 4)
              for key in ("ms_total", "ms_plan", "ms_count", "ms_entropy")}
    bases = int(st["n_bases"])
    algo_bytes = bases + 2 * n * 4 ** q * 4
    line = {"regions": n, "bases_covered": bases, "words": int(st["n_words"]), "tiles": int(st["n_tiles"]),
            "ms_median": round(ms, 4), "ms_min": round(min(all_ms), 4), "ms_max": round(max(all_ms), 4),
            "ms_median_pos_on_device": round(ms_dev, 4), "phase_ms": phases, "algorithmic_bytes": algo_bytes,
            "bytes_per_s": round(algo_bytes / (ms * 1e-3), 1),
            "fraction_of_8TBps": round(algo_bytes / (ms * 1e-3) / HBM_BYTES_PER_S, 5),
            "device_bytes_per_s": round(algo_bytes / (phases["ms_total"] * 1e-3), 1) if phases["ms_total"] else None}
    # spot check: random rows against a host count of the same substrings
    ids = rng.permutation(n)[:check]
    budget, rows, cb, bad = check_bases, 0, 0, 0
    hc = counts[torch.from_numpy(ids).cuda()].cpu().numpy().view(np.uint32).astype(np.int64)
    he = ent[torch.from_numpy(ids).cuda()].cpu().numpy()
    for j, i in enumerate(ids):
        s, b, e = (int(x) for x in pos[:, i])
        if rows and cb + (e - b + 1) > budget:
            continue
        a0 = int(ds.offsets[s]) + b - 1
        sub = ds.seq[a0:a0 + (e - b + 1)].cpu().numpy()
        want = host_row(sub, q, True)
        t = want.sum()
        p = want[want > 0] / t if t else np.zeros(0)
        h = float(-(p * np.log2(p)).sum()) if t else float("nan")
        same = np.array_equal(hc[j], want) and (np.isnan(he[j]) if t == 0 else abs(he[j] - h) < 1e-9)
        bad += 0 if same else 1
        rows += 1
        cb += e - b + 1
    line["spot_check"] = {"rows": rows, "bases": cb, "mismatches": bad}
    del out, pos_dev
    return line


def contended_block(ctx, q, reps, warmup, tile):
    """Equal lists (131072 intervals of one tile each) on pure A, (CA)n, (CAG)n
    and random sequence."""
    n, w = 131072, tile
    L = n * w
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    pats = {"A": torch.tensor([65], dtype=torch.uint8), "CA": torch.tensor([67, 65], dtype=torch.uint8),
            "CAG": torch.tensor([67, 65, 71], dtype=torch.uint8)}
    idx = torch.arange(L, device="cuda")
    seqs = {name: p.cuda()[idx % p.numel()] for name, p in pats.items()}
    seqs["random"] = torch.tensor([65, 67, 71, 84], dtype=torch.uint8, device="cuda")[
        torch.randint(0, 4, (L,), generator=g, device="cuda")]
    del idx
    beg = np.arange(n, dtype=np.int64) * w + 1
    pos = np.stack([np.zeros(n, dtype=np.int64), beg, beg + w - 1]).astype(np.int32)
    pos_dev = torch.from_numpy(pos).cuda()
    out = torch.empty((n, 4 ** q), dtype=torch.int32, device="cuda")
    res = {}
    for name, s in seqs.items():
        ds = D.from_parts([s], [L], "cuda")
        stats = []

        def run():
            r = D.region_spectra(ctx, ds, pos_dev, q=q, both_strands=True, entropy=True, out=out)
            stats.append(r[2])
        median_ms(run, reps, warmup)
        cms = float(np.median([x["ms_count"] for x in stats[-reps:]]))
        res[name] = {"ms_count": round(cms, 4), "Gbases_per_s_count_kernel": round(L / (cms * 1e-3) / 1e9, 2)}
        del ds
    res["what"] = f"{n} intervals of {w} bases each ({L} bases), q = {q}, both strands; count kernel, hipEvents"
    return res


def genome_lists(args, ctx, k, q, rng, res) -> bool:
    """The two region lists of the benchmark genome: scan step against spectra call."""
    t0 = time.time()
    parts, lens = genome.human_like(scale=args.scale, seed=1, device="cuda", ncontigs=args.ncontigs)
    ds = D.from_parts(parts, lens, "cuda")
    del parts
    torch.cuda.synchronize()
    res["genome_bp"] = int(ds.total)
    res["genome_s"] = round(time.time() - t0, 2)
    counts = torch.zeros(4 ** k, dtype=torch.int32, device="cuda")
    words = D.count(ctx, ds, k, counts)
    ok = True
    for name, score, thr in (("weighted_rank", "rank", 0.75), ("log_ratio", "log2", 0.0)):
        D.DeviceTable.from_counts(ctx, counts, k, score, total=words, thr=thr, expand=True).close()  # grows the pools
        table = D.DeviceTable.from_counts(ctx, counts, k, score, total=words, thr=thr, expand=True)
        scan_ms, scan_all, (pos, _, _) = median_ms(
            lambda: D.scan(ctx, ds, k, table, args.min_width, args.min_score), args.reps, args.warmup)
        table.close()
        line = spectra_line(ctx, ds, pos, q, args.reps, args.warmup, args.check, args.check_bases, rng)
        line["scan_step_ms_median"] = round(scan_ms, 4)
        line["scan_step_ms_min_max"] = [round(min(scan_all), 4), round(max(scan_all), 4)]
        line["spectra_over_scan"] = round(line["ms_median"] / scan_ms, 4)
        line["ok"] = bool(line["ms_median"] <= scan_ms and line["spot_check"]["mismatches"] == 0)
        ok = ok and line["ok"]
        res["lists"][name] = line
        del pos
    del ds, counts
    torch.cuda.empty_cache()
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--k", type=int, default=13)
    ap.add_argument("--q", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--check", type=int, default=200)
    ap.add_argument("--check-bases", type=int, default=60_000_000,
                    help="stop the spot check of a list once its substrings add up to this many bases")
    ap.add_argument("--contended-only", action="store_true", help="only the contended-bins block")
    ap.add_argument("--variant", default="run_lengths",
                    help="label of the library build measured (see the comparison build above)")
    ap.add_argument("--min-width", type=int, default=100)
    ap.add_argument("--min-score", type=float, default=20.0)
    ap.add_argument("--ncontigs", type=int, default=24)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "spectra_bench needs a HIP device"
    k, q = args.k, args.q
    ctx = _lib.context(0)
    D.bind_torch_stream(ctx)
    rng = np.random.default_rng(1)
    res = {"tool": "spectra_bench", "variant": args.variant, "scale": args.scale, "k": k, "q": q,
           "both_strands": True, "entropy": True, "reps": args.reps, "warmup": args.warmup,
           "build": _lib.build_id(), "tile_bases": int(_lib.load().ks_spectra_tile_bases()), "lists": {}}
    ok = True
    if not args.contended_only:
        ok = genome_lists(args, ctx, k, q, rng, res)
    res["contended"] = contended_block(ctx, q, 5, 2, res["tile_bases"])
    res["ok"] = ok
    text = json.dumps(res)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
