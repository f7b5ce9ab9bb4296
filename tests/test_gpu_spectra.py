"""Per-region q-mer spectra and Shannon entropy on the device
(ks_region_spectra / ks_region_spectra_dev) against the brute force of
tests/test_spectra.py: counts by exact integer equality, entropy within
4^q * 2q * 2^-52 of the exactly summed value (NaN exactly where a row is
empty), stats by equality.  Runs on an MI355X (pytest -m gpu)."""
import math
import random

import numpy as np
import pytest

from tests.test_spectra import brute_entropy, brute_spectrum, entropy_bound, rc_code

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from kmer_spans_amd import _lib
    from kmer_spans_amd import device as D
    c = _lib.context(0)
    D.bind_torch_stream(c)
    return c


@pytest.fixture(scope="module")
def TILE():
    from kmer_spans_amd import _lib
    return int(_lib.load().ks_spectra_tile_bases())


def brute_counts(seq: bytes, beg: int, end: int, q: int) -> np.ndarray:
    """brute_spectrum's single-strand row with a rolling code (the same
    windows, one pass): the large cases would take minutes otherwise."""
    row = [0] * 4 ** q
    mask = 4 ** q - 1
    code = run = 0
    for ch in seq[beg - 1:end]:
        run = 0 if ch in (78, 110) else run + 1
        code = ((code << 2) | ((ch >> 1) & 3)) & mask
        if run >= q:
            row[code] += 1
    return np.array(row, dtype=np.int64)


def numpy_counts(seq: bytes, q: int):
    """Per sequence: the code of the word starting at every byte and whether it
    is a word (no N/n); a row is then one bincount over a slice.  The same
    windows as brute_spectrum (checked below), for lists of millions of bases."""
    a = np.frombuffer(seq, dtype=np.uint8)
    n = a.size - q + 1
    e = ((a >> 1) & 3).astype(np.int64)
    code = np.zeros(max(n, 0), dtype=np.int64)
    for j in range(q):
        code = (code << 2) | e[j:j + n]
    isn = np.concatenate(([0], np.cumsum((a | 0x20) == ord("n"))))
    ok = (isn[q:q + n] - isn[:n]) == 0

    def row(beg, end):
        lo, hi = beg - 1, end - q + 1  # word starts [lo, hi)
        if hi <= lo:
            return np.zeros(4 ** q, dtype=np.int64)
        return np.bincount(code[lo:hi][ok[lo:hi]], minlength=4 ** q)
    return row


def wave_budget(q: int) -> int:
    """Waves the counting kernel starts at most (ks_spectra.hip: four per
    block, at most 8 blocks per CU and as many as 160 KiB of LDS hold): a list
    with more tiles gives every wave a block of several."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return cus * max(1, min(8, (160 * 1024) // (4 * 4 ** q * 4))) * 4


_RC = {}


def fold(row, q, both):
    if not both:
        return row
    if q not in _RC:
        _RC[q] = np.array([rc_code(c, q) for c in range(4 ** q)])
    return row + row[_RC[q]]


def test_rolling_brute_force_is_the_brute_force():
    rng = random.Random(3)
    s = "".join(rng.choice("ACGTacgtNnRYK") for _ in range(400)).encode()
    for q in range(1, 7):
        for beg, end in ((1, 400), (7, 6), (5, 5 + q - 1), (100, 333)):
            for both in (False, True):
                assert np.array_equal(fold(brute_counts(s, beg, end, q), q, both), brute_spectrum(s, beg, end, q, both))
                assert np.array_equal(fold(numpy_counts(s, q)(beg, end), q, both), brute_spectrum(s, beg, end, q, both))


def check_device(ctx, seqs, ivs, q, both, ds=None, pos=None, seq_base=0, out=None, what="", rows=None):
    """Run device.region_spectra on intervals ivs = [(seq_id, beg, end)] (0-based
    ids) and compare every row, every entropy and the stats with the brute force."""
    import torch
    from kmer_spans_amd import device as D
    if ds is None:
        ds = D.from_host(seqs, "cuda")
    if pos is None:
        pos = np.array(ivs, dtype=np.int32).reshape(-1, 3).T.copy()
    counts, ent, st = D.region_spectra(ctx, ds, pos, q=q, both_strands=both, seq_base=seq_base, out=out)
    counts_ne, none, _ = D.region_spectra(ctx, ds, pos, q=q, both_strands=both, seq_base=seq_base, entropy=False)
    assert none is None and torch.equal(counts, counts_ne), (what, "entropy=False changes the counts")
    got = counts.cpu().numpy().view(np.uint32).astype(np.int64)
    h = ent.cpu().numpy()
    assert got.shape == (len(ivs), 4 ** q) and h.shape == (len(ivs),)
    words = 0
    worst = 0.0
    for i, (s, b, e) in enumerate(ivs):
        single = rows[s](b, e) if rows is not None else brute_counts(seqs[s], b, e, q)
        words += int(single.sum())
        want = fold(single, q, both)
        assert np.array_equal(got[i], want), (what, "row", i, (s, b, e), q, both,
                                              np.nonzero(got[i] != want)[0][:8].tolist())
        href = brute_entropy(want)
        if math.isnan(href):
            assert math.isnan(h[i]), (what, "entropy of an empty row", i, h[i])
        else:
            err = abs(h[i] - href)
            worst = max(worst, err)
            assert err <= entropy_bound(q), (what, "entropy", i, (s, b, e), q, h[i], href, err)
    assert st["n_regions"] == len(ivs) and st["n_words"] == words, (what, st, words)
    assert st["n_bases"] == sum(e - b + 1 for _, b, e in ivs), (what, st)
    print(f"{what}: {len(ivs)} rows q={q} both={both}, largest entropy error {worst:.3e} "
          f"(bound {entropy_bound(q):.3e})")
    return got, h, st


# ------------------------------------------------------------ known answers

@pytest.mark.parametrize("both", [False, True])
def test_known_answer(ctx, both):
    import kmer_spans_amd as K
    from kmer_spans_amd import device as D
    want = np.zeros(16, dtype=np.int64)
    want[[1, 7, 14]] = 2 if both else 1  # AC, CG, GT; rc(AC) = GT, rc(CG) = CG
    pos = np.array([[0], [1], [4]], dtype=np.int32)
    r = K.region_spectra("ACGT", pos, q=2, both_strands=both)  # api -> host entry
    assert r["counts"].dtype == np.uint32 and r["counts"][0].tolist() == want.tolist()
    assert r["kmers"] == K.kmer_seq(2) and [r["kmers"][c] for c in (1, 7, 14)] == ["AC", "CG", "GT"]
    assert abs(r["entropy"][0] - math.log2(3)) <= entropy_bound(2)
    assert np.allclose(r["freq"][0], want / want.sum(), rtol=0, atol=1e-16)
    r2 = K.region_spectra("ACGT", pos.T.copy(), q=2, both_strands=both)  # [R, 3] layout
    assert np.array_equal(r2["counts"], r["counts"])
    got, h, st = check_device(ctx, [b"ACGT"], [(0, 1, 4)], 2, both, what="known")
    assert got[0].tolist() == want.tolist() and abs(h[0] - math.log2(3)) <= entropy_bound(2)
    # an empty row: NaN entropy, NaN frequencies
    r = K.region_spectra(["ACGT", "NNNN"], np.array([[0, 1, 0], [1, 1, 3], [1, 4, 2]], dtype=np.int32), q=2,
                         both_strands=both)
    assert r["counts"].sum() == 0 and np.isnan(r["entropy"]).all() and np.isnan(r["freq"]).all()


# --------------------------------------------------------------- randomised

def _random_case(rng):
    seqs = []
    for _ in range(rng.randint(1, 4)):
        L = rng.randint(0, 5000)
        s = [rng.choice("ACGTacgtNnRYK") if rng.random() < 0.15 else rng.choice("ACGT") for _ in range(L)]
        for _ in range(rng.randint(0, 3)):  # N runs
            if L:
                a = rng.randrange(L)
                for j in range(a, min(L, a + rng.randint(1, 40))):
                    s[j] = "N"
        seqs.append("".join(s).encode())
    return seqs


def _random_intervals(rng, seqs, q):
    nz = [i for i, s in enumerate(seqs) if len(s) >= 8] or [0]
    ivs = []

    def one(s, wmax=None):
        L = len(seqs[s])
        b = rng.randint(1, L + 1)
        w = rng.randint(0, min(L - b + 1, wmax if wmax is not None else L))
        return (s, b, b + w - 1)
    for _ in range(rng.randint(1, 60)):
        ivs.append(one(rng.randrange(len(seqs)), rng.choice([None, 30, 300])))
    s = rng.choice(nz)
    L = len(seqs[s])
    b = rng.randint(1, max(1, L - q + 1))
    ivs.append((s, b, b - 1))                       # width 0
    if L >= q:
        ivs.append((s, b, b + q - 2))               # width q - 1
        ivs.append((s, b, b + q - 1))               # width q
    ivs.append((s, 1, L))                           # the whole sequence
    ivs.append((s, 1, rng.randint(0, L)))           # starts at 1
    ivs.append((s, rng.randint(1, L + 1), L))       # ends at len
    d = one(s, 200)
    ivs += [d, d]                                   # a duplicate pair
    if L >= 8:
        a = rng.randint(1, L - 6)
        ivs += [(s, a, min(L, a + 50)), (s, a + 3, min(L, a + 90))]  # an overlapping pair
    rng.shuffle(ivs)
    return ivs


@pytest.mark.parametrize("both", [False, True])
def test_random_intervals(ctx, both):
    import kmer_spans_amd as K
    rng = random.Random(100 + both)
    for seed in range(40):
        seqs = _random_case(rng)
        q = 1 + seed % 6
        ivs = _random_intervals(rng, seqs, q)
        got, h, _ = check_device(ctx, seqs, ivs, q, both, what=f"random {seed}")
        if seed % 8 == 0:  # the host entry gives the same rows and the same entropy bits
            r = K.region_spectra(seqs, np.array(ivs, dtype=np.int32).T.copy(), q=q, both_strands=both)
            assert np.array_equal(r["counts"].astype(np.int64), got)
            assert np.array_equal(r["entropy"].view(np.uint64), h.view(np.uint64))


# --------------------------------------------------------------- tile seams

@pytest.mark.parametrize("q", [1, 4, 6])
def test_tile_seams(ctx, TILE, q):
    from kmer_spans_amd import device as D
    rng = random.Random(q)
    L = 3 * TILE + 7
    base = [rng.choice("ACGT") for _ in range(L)]
    ivs = []
    for off in (1, 2, 17):
        for w in (TILE - 1, TILE, TILE + 1, 2 * TILE, 2 * TILE + q - 1):
            ivs.append((0, off, off + w - 1))
    ivs.append((0, 1, L))
    nspots = [None] + sorted({TILE, TILE - 1, TILE + 1, TILE - (q - 1), TILE + (q - 1)})
    for spot in nspots:  # a single N at the seam (1-based position), one base before / after, q - 1 before / after
        s = list(base)
        if spot is not None:
            s[spot - 1] = "N"
        seqs = ["".join(s).encode()]
        for both in (False, True):
            check_device(ctx, seqs, ivs, q, both, what=f"seams N@{spot}")


# ------------------------------------------------ one interval over many waves

def test_one_interval_over_many_waves(ctx, TILE):
    import torch
    rng = random.Random(5)
    L = 70 * TILE + 3
    seq = "".join(rng.choice("ACGTN") if rng.random() < 0.01 else rng.choice("ACGT") for _ in range(L)).encode()
    ivs = [(0, 1, L), (0, 10 * TILE + 5, 10 * TILE + 900)]  # atomic merge; plain stores
    for q, both in ((4, True), (6, False)):
        out = torch.full((2, 4 ** q), 0x7f7f7f7f, dtype=torch.int32, device="cuda")  # overwritten, not added to
        got, _, st = check_device(ctx, [seq], ivs, q, both, out=out, what="many waves")
        assert np.array_equal(out.cpu().numpy().view(np.uint32).astype(np.int64), got)
        assert st["n_tiles"] == 72  # 71 tiles of the long interval, one of the short


# ------------------------------------------------------ many short intervals

def test_many_short_intervals(ctx):
    rng = random.Random(6)
    L = 200_000
    seq = "".join(rng.choice("ACGT") for _ in range(L)).encode()
    ivs = []
    for _ in range(5000):
        w = rng.randint(4, 400)
        b = rng.randint(1, L - w + 1)
        ivs.append((0, b, b + w - 1))
    check_device(ctx, [seq], ivs, 4, True, what="short")


# ------------------------------------- more tiles than waves: blocks of tiles

@pytest.mark.parametrize("q,n", [(6, 5000), (4, 24000)])
def test_short_intervals_beyond_the_wave_budget(ctx, q, n):
    """More one-tile intervals than the kernel starts waves: every wave walks a
    block of them, flushing, zeroing and reusing its LDS histogram at each
    interval change (a count leaking into the next row shows here)."""
    rng = random.Random(60 + q)
    L = 100_000
    seq = "".join(rng.choice("ACGTN") if rng.random() < 0.01 else rng.choice("ACGT") for _ in range(L)).encode()
    ivs = []
    for _ in range(n):
        w = rng.randint(0, 90)
        b = rng.randint(1, L - w + 1)
        ivs.append((0, b, b + w - 1))
    _, _, st = check_device(ctx, [seq], ivs, q, True, what="short, blocks of tiles", rows=[numpy_counts(seq, q)])
    assert st["n_tiles"] == n and n >= 2 * wave_budget(q), (st, wave_budget(q))


def test_multi_tile_intervals_beyond_the_wave_budget(ctx, TILE):
    """Thousands of intervals of 1-3 tiles at q = 6: a wave adds several tiles
    of one row in LDS, starts in the middle of an interval, is cut at its
    block's end inside one, and crosses interval changes, so shared rows get
    partial sums from several waves and single-tile rows lie between them."""
    rng = random.Random(66)
    q = 6
    L = 300_000
    seqs = ["".join(rng.choice("ACGTN") if rng.random() < 0.002 else rng.choice("ACGT") for _ in range(n)).encode()
            for n in (L, 3 * TILE + 11)]
    ivs = []
    for _ in range(3000):
        s = rng.randrange(2)
        w = rng.choice([rng.randint(TILE + 1, 3 * TILE), rng.randint(TILE + 1, 3 * TILE), rng.randint(0, TILE)])
        w = min(w, len(seqs[s]))
        b = rng.randint(1, len(seqs[s]) - w + 1)
        ivs.append((s, b, b + w - 1))
    _, _, st = check_device(ctx, seqs, ivs, q, True, what="multi-tile, blocks of tiles",
                            rows=[numpy_counts(x, q) for x in seqs])
    assert st["n_tiles"] >= 2 * wave_budget(q) and st["n_tiles"] > 1.5 * len(ivs), (st, wave_budget(q))


# ------------------------------------------------------------ contended bins

@pytest.mark.parametrize("q", [2, 4])
def test_contended_bins(ctx, TILE, q):
    rng = random.Random(7)
    W = 5 * TILE
    seqs = [b"A" * W, b"CA" * (W // 2), (b"CAG" * (W // 3 + 1))[:W],
            "".join(rng.choice("ACGT") for _ in range(W)).encode()]
    ivs = []
    for s in range(4):
        ivs += [(s, 1, W), (s, 301, 400), (s, 2, 101)]
    check_device(ctx, seqs, ivs, q, True, what="contended")


# ------------------------------------------------------------------ pipeline

def _planted(ctx, k):
    import torch
    from kmer_spans_amd import device as D, genome
    s = genome.contig(300_000, 17, device="cuda", repeats=True)
    ds = D.from_parts([s, s[:40_000].clone()], [s.numel(), 40_000], "cuda")
    counts = torch.zeros(4 ** k, dtype=torch.int32, device="cuda")
    words = D.count(ctx, ds, k, counts)
    return ds, [ds.host_seq(0), ds.host_seq(1)], counts, words


def test_pipeline_scan_regions(ctx):
    """device.scan's pos goes to device.region_spectra unchanged, as numpy and
    as a CUDA tensor; the reference is the brute force on subseq(seq[id + 1],
    beg, end) of the same numbers."""
    import torch
    from kmer_spans_amd import device as D
    k = 7
    ds, host, counts, words = _planted(ctx, k)
    tab = D.DeviceTable.from_counts(ctx, counts, k, "rank", total=words, thr=0.75, expand=True)
    pos, _, _ = D.scan(ctx, ds, k, tab, 20, 5.0)
    assert pos.shape[1] >= 5
    ivs = [tuple(int(x) for x in c) for c in pos.T]
    got, h, _ = check_device(ctx, host, ivs, 4, True, ds=ds, pos=pos, what="scan regions (numpy)")
    got_t, h_t, _ = check_device(ctx, host, ivs, 4, True, ds=ds, pos=torch.from_numpy(pos.copy()).cuda(),
                                 what="scan regions (tensor)")
    assert np.array_equal(got, got_t) and np.array_equal(h.view(np.uint64), h_t.view(np.uint64))


def test_pipeline_tr_lr_regions(ctx):
    import torch
    from kmer_spans_amd import device as D
    k = 7
    ds, host, counts, words = _planted(ctx, k)
    oc = counts.cpu().numpy().astype(np.float64)
    tr = np.log2(oc + 1.0) - np.log2(np.median(oc) + 1.0) - 0.4  # repeats score positive
    ks = np.random.default_rng(k).normal(size=4 ** k)
    ttr = D.DeviceTable(ctx, tr, k, 0.0, expand=True)
    tks = D.DeviceTable(ctx, ks, k, 0.0, compress=False)
    pos, _, _ = D.tr_lr(ctx, ds, k, ttr, tks, 5)
    assert pos.shape[1] >= 5 and pos[0].min() >= 1
    ivs = [(int(c[0]) - 1, int(c[1]), int(c[2])) for c in pos.T]
    check_device(ctx, host, ivs, 4, True, ds=ds, pos=pos, seq_base=1, what="tr_lr regions (numpy)")
    check_device(ctx, host, ivs, 3, False, ds=ds, pos=torch.from_numpy(pos.copy()).cuda(), seq_base=1,
                 what="tr_lr regions (tensor)")


# ----------------------------------------------------- device-entry validation

@pytest.mark.parametrize("bad", ["end", "seq_id"])
def test_device_entry_rejects_a_bad_interval(ctx, bad):
    """The planning kernel's check: one bad interval among good ones is an
    argument error naming it, no row of the output has been touched (neither
    by the counting kernel nor by the clearing of multi-tile rows), and the
    context is fine afterwards."""
    import torch
    import kmer_spans_amd as K
    from kmer_spans_amd import _lib, device as D
    rng = random.Random(9)
    T = int(_lib.load().ks_spectra_tile_bases())
    seqs = ["".join(rng.choice("ACGT") for _ in range(n)).encode() for n in (2 * T + 50, 300)]
    ds = D.from_host(seqs, "cuda")
    good = [(0, 1, 2 * T + 50), (1, 5, 200), (0, 100, 99), (1, 1, 300), (0, 50, 650)]  # row 0: three tiles
    ivs = list(good)
    ivs[3] = (1, 1, 301) if bad == "end" else (2, 1, 10)
    out = torch.full((len(ivs), 256), 0x7f7f7f7f, dtype=torch.int32, device="cuda")
    with pytest.raises(K.KmerSpansError, match="^interval 3 out of range$"):
        D.region_spectra(ctx, ds, np.array(ivs, dtype=np.int32).T.copy(), q=4, out=out)
    assert bool((out == 0x7f7f7f7f).all())
    check_device(ctx, seqs, good, 4, True, ds=ds, out=out, what="after a rejected call")
