"""The k nearest regions by spectrum on the device (ks_spectra_knn_dev and the
host entry) against the host model of tests/knnref.py: index identical, dist
identical in every bit when squared and within 1 ulp of np.sqrt of the model's
squared value otherwise.  Runs on an MI355X (pytest -m gpu)."""
import ctypes as C

import numpy as np
import pytest

from tests import knnref as R
from tests.kmeansref import profiles, sqdist
from tests.test_gpu_spectra_dist import assert_sqrt_of
from tests.test_kmeans import tie_heavy_case
from tests.test_knn import LINE5, equal_root_case, proportional_family_case
from tests.test_nj import bits
from tests.test_spectra_dist import random_counts

pytestmark = pytest.mark.gpu

TILE = 64  # candidates per tile of k_knn_select


@pytest.fixture(scope="module")
def ctx():
    from kmer_spans_amd import _lib
    from kmer_spans_amd import device as D
    c = _lib.context(0)
    D.bind_torch_stream(c)
    return c


def to_dev(counts):
    import torch
    return torch.from_numpy(np.ascontiguousarray(counts, dtype=np.uint32).view(np.int32)).cuda()


def model_full(counts, rows=None, rows_b=None):
    """The model's list at the largest k the shape allows: every shorter list is a prefix of it."""
    pa = profiles(counts, rows)
    pb = pa if rows_b is None else profiles(counts, rows_b)
    cand = pb.shape[0] - (1 if rows_b is None else 0)
    return R.select(sqdist(pa, pb), min(R.MAX_K, cand), np.arange(pa.shape[0]) if rows_b is None else None)


def check_knn(ctx, counts, k, rows=None, rows_b=None, full=None, what="", dev=None, plain=True):
    """device.region_knn, squared and plain, against the model; the spectra's bits are unchanged."""
    from kmer_spans_amd import device as D
    dev = to_dev(counts) if dev is None else dev
    hrows = rows.cpu().numpy() if hasattr(rows, "cpu") else rows
    hrows_b = rows_b.cpu().numpy() if hasattr(rows_b, "cpu") else rows_b
    windex, wacc = model_full(counts, hrows, hrows_b) if full is None else full
    windex, wacc = windex[:, :k], wacc[:, :k]
    index, acc, st = D.region_knn(ctx, dev, k, rows=rows, rows_b=rows_b, squared=True)
    assert str(index.dtype) == "torch.int64" and tuple(index.shape) == windex.shape == tuple(acc.shape)
    gi, ga = index.cpu().numpy(), acc.cpu().numpy()
    assert np.array_equal(gi, windex), (what, "index", int((gi != windex).sum()), np.argwhere(gi != windex)[:4])
    assert np.array_equal(bits(ga), bits(wacc)), (what, "squared dist", int((bits(ga) != bits(wacc)).sum()))
    if plain:
        index2, d, _ = D.region_knn(ctx, dev, k, rows=rows, rows_b=rows_b)
        assert np.array_equal(index2.cpu().numpy(), windex), (what, "index of the plain call")
        assert_sqrt_of(d.cpu().numpy(), wacc, what)
    assert np.array_equal(dev.cpu().numpy().view(np.uint32), np.asarray(counts, dtype=np.uint32)), (what, "spectra")
    na = windex.shape[0]
    nb = na if rows_b is None else len(hrows_b)
    assert st["panel_bytes"] >= 8 * counts.shape[1] * (na if rows_b is None else na + nb)
    assert st["n_splits"] >= 1 and st["tiles_per_split"] * st["n_splits"] >= (nb + TILE - 1) // TILE
    if st["n_splits"] > 1:
        assert st["work_bytes"] >= 12 * na * k * st["n_splits"]
    return index, acc, st


# ------------------------------------------------------------- known answers

def test_line(ctx):
    import kmer_spans_amd as K
    index, acc, _ = check_knn(ctx, LINE5, 4, what="line")
    assert index.cpu().tolist() == [[1, 2, 3, 4], [0, 2, 3, 4], [3, 1, 0, 4], [2, 1, 0, 4], [3, 2, 1, 0]]
    assert acc.cpu().tolist()[3] == [.03125, .28125, .5, .5]
    index, acc, _ = check_knn(ctx, LINE5, 4, rows=np.array([0, 3]), rows_b=np.array([4, 2, 0, 1]), what="line, cross")
    assert index.cpu().tolist() == [[2, 3, 1, 0], [1, 3, 0, 2]]
    hi, hd = K.region_knn(LINE5, 2, squared=True)  # api -> host entry
    assert hi.tolist() == [[1, 2], [0, 2], [3, 1], [2, 1], [3, 2]] and hd[:, 0].tolist() == [.03125] * 4 + [.5]


# ------------------------------------------------- sizes across the tile edges

@pytest.mark.parametrize("m", [2, 3, 63, 64, 65, 129, 257, 1025])
def test_self_sizes(ctx, m):
    """The tile edge (64 rows, 64 candidates) with one either side, several row
    tiles, and k either side of 16 and at 64."""
    counts = random_counts(np.random.default_rng(m), m, 16)
    dev, full = to_dev(counts), model_full(counts)
    for k in (1, 2, 15, 16, 17, 63, 64):
        if k <= m - 1:
            check_knn(ctx, counts, k, full=full, what=f"self m={m} k={k}", dev=dev, plain=k in (1, 17, 64))


@pytest.mark.parametrize("na", [1, 64, 65])
def test_cross_sizes(ctx, na):
    counts = random_counts(np.random.default_rng(na + 7), 1100, 16)
    dev = to_dev(counts)
    rows = np.arange(na, dtype=np.int64) * 3
    for nb in (1, 63, 64, 65, 1025):
        rows_b = (np.arange(nb, dtype=np.int64) * 7 + 1) % 1100
        full = model_full(counts, rows, rows_b)
        for k in sorted({1, min(nb, 10), min(nb, 64)}):
            check_knn(ctx, counts, k, rows=rows, rows_b=rows_b, full=full, what=f"cross na={na} nb={nb} k={k}",
                      dev=dev, plain=k == 1)


@pytest.mark.parametrize("m,ncol,k", [(65, 1, 3), (130, 15, 10), (130, 17, 10), (200, 256, 10), (65, 4096, 5)])
def test_column_counts(ctx, m, ncol, k):
    """One column (every row is the profile (1): all at 0), one either side of
    the 16-column LDS chunk, the flagship 256, and the largest ncol."""
    counts = random_counts(np.random.default_rng(ncol + m), m, ncol)
    check_knn(ctx, counts, k, what=f"self m={m} ncol={ncol}")
    check_knn(ctx, counts, k, rows=np.arange(0, m, 2), rows_b=np.arange(m - 1, -1, -3), what=f"cross ncol={ncol}")


# ---------------------------------------------------------------- split seams

def planted(base, t):
    """A near copy of the counts row `base`: proportional but for t + 1 counts in column 0."""
    row = base.astype(np.uint64) * 1000
    row[0] += t + 1
    return row.astype(np.uint32)


def test_split_seams(ctx):
    """64 queries against 1064 candidates (17 tiles, the last one of 40): the
    candidate tiles are split over the grid.  Near copies of three queries are
    planted so that the k best of query 0 lie all in the first split, of query
    1 all in the last split and of query 2 one in every split; every query's
    list is the model's."""
    from kmer_spans_amd import device as D
    rng = np.random.default_rng(99)
    na, nb, ncol = 64, 1064, 16
    q = rng.integers(1, 1000, size=(na, ncol)).astype(np.uint32)
    cand = random_counts(rng, nb, ncol)
    rows, rows_b = np.arange(na, dtype=np.int64), np.arange(na, na + nb, dtype=np.int64)
    _, _, st = D.region_knn(ctx, to_dev(np.vstack([q, cand])), 1, rows=rows, rows_b=rows_b)
    ns, per = int(st["n_splits"]), int(st["tiles_per_split"]) * TILE
    print(f"na = {na}, nb = {nb}: {ns} splits of {per} candidates")
    assert 3 <= ns <= R.MAX_K and (ns - 1) * per < nb <= ns * per
    k, last_lo = ns, (ns - 1) * per
    assert per >= k and nb - last_lo >= k + 1
    first = rng.choice(per, size=k, replace=False)
    last = last_lo + rng.choice(nb - last_lo, size=k, replace=False)
    used = set(first.tolist()) | set(last.tolist())
    each = np.array([rng.choice([j for j in range(y * per, min((y + 1) * per, nb)) if j not in used])
                     for y in range(ns)])
    for qi, where in ((0, first), (1, last), (2, each)):
        for t, at in enumerate(where):
            cand[at] = planted(q[qi], t)
    counts = np.vstack([q, cand])
    index, _, st2 = check_knn(ctx, counts, k, rows=rows, rows_b=rows_b, what="split seams")
    assert st2["n_splits"] == ns
    got = index.cpu().numpy()
    assert got[0].tolist() == first.tolist() and (got[0] < per).all()  # planted t is the t-th nearest
    assert got[1].tolist() == last.tolist() and (got[1] >= last_lo).all()
    assert got[2].tolist() == each.tolist() and sorted((got[2] // per).tolist()) == list(range(ns))
    # one split: a single candidate tile
    _, _, st1 = check_knn(ctx, counts, 10, rows=rows, rows_b=rows_b[:64], what="one split")
    assert st1["n_splits"] == 1 and st1["ms_merge"] == 0.0


# ----------------------------------------- insert-heavy and reject-heavy orders

@pytest.mark.parametrize("order", ["descending", "ascending"])
def test_sorted_candidates(ctx, order):
    """nb = 1025, k = 64.  Candidates by descending distance to query 0: every
    tile beats the list's k-th entry and every candidate is inserted.  By
    ascending distance: nothing after the first k is."""
    rng = np.random.default_rng(1025)
    counts = random_counts(rng, 1025 + 3, 16)
    acc0 = sqdist(profiles(counts[:1]), profiles(counts[3:]))[0]
    by = np.argsort(acc0, kind="stable")
    rows_b = 3 + (by[::-1] if order == "descending" else by)
    index, _, _ = check_knn(ctx, counts, 64, rows=np.arange(3), rows_b=rows_b, what=order)
    want = np.arange(1024, 1024 - 64, -1) if order == "descending" else np.arange(64)
    ties = np.unique(acc0).size != acc0.size
    assert ties or index.cpu().numpy()[0].tolist() == want.tolist()


# ---------------------------------------------------------------------- ties

def test_all_rows_equal(ctx):
    m = 130
    scale = (np.arange(m, dtype=np.uint32) % 7 + 1)[:, None]
    counts = np.tile(np.array([[3, 1, 4, 1]], dtype=np.uint32), (m, 1)) * scale
    index, acc, _ = check_knn(ctx, counts, 17, what="all equal")
    assert not acc.cpu().numpy().any()
    got = index.cpu().numpy()
    for s in (0, 5, 16, 17, 18, 63, 64, 129):
        assert got[s].tolist() == [j for j in range(m) if j != s][:17]


@pytest.mark.parametrize("k", [1, 5, 16, 21])
def test_proportional_families_across_a_tile_boundary(ctx, k):
    """3k proportional rows at positions 60 .. 60 + 3k - 1: all at exactly 0, the lowest positions win."""
    counts = proportional_family_case(k, 60)
    index, acc, _ = check_knn(ctx, counts, k, what=f"family k={k}")
    got = index.cpu().numpy()
    for s in range(60, 60 + 3 * k):
        assert got[s].tolist() == [j for j in range(60, 60 + 3 * k) if j != s][:k]
    assert not acc.cpu().numpy()[60:60 + 3 * k].any()


@pytest.mark.parametrize("m", [130, 600])
def test_tie_heavy(ctx, m):
    counts, _ = tie_heavy_case(m)
    full = model_full(counts)
    tied = int((np.diff(full[1], axis=1) == 0).any(axis=1).sum())
    print(f"m = {m}: {tied} rows with equal distances inside their list")
    assert tied > m // 2
    for k in (1, 16, 64):
        check_knn(ctx, counts, k, full=full, what=f"ties m={m} k={k}", plain=False)


def test_equal_roots(ctx):
    counts, rows, rows_b = equal_root_case()
    from kmer_spans_amd import device as D
    index, d, _ = D.region_knn(ctx, to_dev(counts), 3, rows=rows, rows_b=rows_b)
    assert index.cpu().tolist() == [[1, 0, 2]]  # by the squared value, not by (root, position)
    d = d.cpu().numpy()
    assert abs(int(bits(d)[0, 0]) - int(bits(d)[0, 1])) <= 1
    check_knn(ctx, counts, 3, rows=rows, rows_b=rows_b, what="equal roots")


# ---------------------------------------- consistency with the existing entries

@pytest.mark.parametrize("m", [130, 1025])
def test_consistent_with_region_distances_and_kmeans(ctx, m):
    import torch
    from kmer_spans_amd import device as D
    counts = random_counts(np.random.default_rng(m * 3), m, 16)
    dev = to_dev(counts)
    # k = 1, self form: the first-minimum argmin of the dense squared block, the diagonal masked
    rows = torch.from_numpy(np.random.default_rng(m).permutation(m).astype(np.int64)).cuda()
    block, _ = D.region_distances(ctx, dev, rows, rows, squared=True)
    masked = block.cpu().numpy().copy()
    np.fill_diagonal(masked, np.inf)
    index, acc, _ = D.region_knn(ctx, dev, 1, rows=rows, squared=True)
    assert np.array_equal(index.cpu().numpy()[:, 0], np.argmin(masked, axis=1))
    assert np.array_equal(bits(acc.cpu().numpy()[:, 0]), bits(masked.min(axis=1)))
    # cross form: the returned squared distances are region_distances' entries at the returned positions
    rows_b = torch.from_numpy(np.random.default_rng(m + 1).integers(0, m, size=m // 2).astype(np.int64)).cuda()
    block, _ = D.region_distances(ctx, dev, rows, rows_b, squared=True)
    index, acc, _ = D.region_knn(ctx, dev, 10, rows=rows, rows_b=rows_b, squared=True)
    assert torch.equal(torch.gather(block, 1, index).view(torch.int64), acc.view(torch.int64))
    # the first pass of k-means from init_rows is the nearest candidate among those rows
    start = (np.arange(24, dtype=np.int64) * 5) % m
    km, _ = D.region_kmeans(ctx, dev, start, rows=rows, iter_max=1)
    index, _, _ = D.region_knn(ctx, dev, 1, rows=rows, rows_b=rows[torch.from_numpy(start).cuda()])
    assert np.array_equal(km["cluster"].cpu().numpy(), index.cpu().numpy()[:, 0] + 1)


# -------------------------------------------------------------- selections

def test_selections(ctx):
    """A descending selection with repeats, as numpy and as a CUDA tensor; a
    repeated row finds its copy at exactly 0 and never itself."""
    import torch
    m = 300
    counts = random_counts(np.random.default_rng(300), m, 16)
    dev = to_dev(counts)
    rows = np.concatenate([np.arange(m - 1, -1, -2), [5, 5, 17, 299, 0, 5]]).astype(np.int64)
    full = model_full(counts, rows)
    index, acc, _ = check_knn(ctx, counts, 10, rows=rows, full=full, what="numpy selection", dev=dev)
    check_knn(ctx, counts, 10, rows=torch.from_numpy(rows).cuda(), full=full, what="cuda selection", dev=dev)
    got, ga = index.cpu().numpy(), acc.cpu().numpy()
    assert all(s not in got[s] for s in range(rows.size))
    five = np.flatnonzero(rows == 5)  # positions 147, 150, 151, 155
    assert five.size == 4
    for s in five:
        assert got[s, :3].tolist() == [j for j in five if j != s] and not ga[s, :3].any() and ga[s, 3] > 0
    rows_b = np.concatenate([rows[::-1][:40], [5, 5]])
    check_knn(ctx, counts, 7, rows=rows, rows_b=torch.from_numpy(rows_b).cuda(), what="cross, mixed", dev=dev)


# ---------------------------------------------------------------- robustness

def raw_knn(ctx, sp, ncol, k, index, dist, rows=None, rows_b=None, flags=1):
    """ks_spectra_knn_dev through ctypes on caller-owned tensors."""
    import torch
    from kmer_spans_amd import _lib
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    torch.cuda.current_stream().synchronize()
    rc = _lib.load().ks_spectra_knn_dev(ctx.handle, ptr(sp), sp.shape[0], ncol, ptr(rows),
                                        sp.shape[0] if rows is None else rows.numel(), ptr(rows_b),
                                        0 if rows_b is None else rows_b.numel(), k, flags, ptr(index), ptr(dist), None)
    return rc, _lib.load().ks_last_error().decode()


def test_repeat_gives_the_same_bits(ctx):
    from kmer_spans_amd import device as D
    counts = random_counts(np.random.default_rng(513), 513, 16)
    dev = to_dev(counts)
    a = D.region_knn(ctx, dev, 20)
    b = D.region_knn(ctx, dev, 20)
    assert np.array_equal(a[0].cpu().numpy(), b[0].cpu().numpy())
    assert np.array_equal(bits(a[1].cpu().numpy()), bits(b[1].cpu().numpy()))


def test_rejected_calls_leave_the_outputs_untouched(ctx):
    import torch
    m, ncol, k = 90, 16, 5
    counts = random_counts(np.random.default_rng(90), m, ncol)
    empty = counts.copy()
    empty[37] = 0
    rows_ok = torch.arange(m, dtype=torch.int64, device="cuda")
    bad_rows = rows_ok.clone()
    bad_rows[[11, 40]] = torch.tensor([m, -1], device="cuda")
    few = rows_ok[:4].clone()
    cases = [("bad index", to_dev(counts), bad_rows, None, k, "row index 11 out of range"),
             ("bad candidate index", to_dev(counts), rows_ok, bad_rows, k,
              "row index 11 of the second selection out of range"),
             ("empty row", to_dev(empty), rows_ok, None, k, "row 37 has no counts"),
             ("empty candidate row", to_dev(empty), few, rows_ok, k, "row 37 of the second selection has no counts"),
             ("index before empty row", to_dev(empty), rows_ok, bad_rows, k,
              "row index 11 of the second selection out of range"),
             ("k above the candidates, self", to_dev(counts), few, None, 4,
              "k exceeds the number of candidate rows (k = 4, 3 candidates)"),
             ("k above the candidates, cross", to_dev(counts), rows_ok, few, 5,
              "k exceeds the number of candidate rows (k = 5, 4 candidates)"),
             ("empty row before k", to_dev(empty), rows_ok[36:39].clone(), None, 3, "row 1 has no counts")]
    for name, sp, rows, rows_b, kk, text in cases:
        index = torch.full((m, kk), -77, dtype=torch.int64, device="cuda")
        dist = torch.full((m, kk), -7.5, dtype=torch.float64, device="cuda")
        rc, msg = raw_knn(ctx, sp, ncol, kk, index, dist, rows=rows, rows_b=rows_b)
        assert rc != 0 and msg == text, (name, msg)
        assert (index == -77).all() and (dist == -7.5).all(), (name, "an output was written")
        check_knn(ctx, counts, k, what=f"after {name}", plain=False)


def test_host_entry(ctx):
    import kmer_spans_amd as K
    m = 257
    counts = random_counts(np.random.default_rng(2570), m, 17)
    rows = np.arange(m - 1, -1, -1)
    wi, wa = R.knn(counts, 12, rows=rows, squared=True)
    gi, ga = K.region_knn(counts.astype(np.int64), 12, rows=rows, squared=True)
    assert gi.dtype == np.int64 and np.array_equal(gi, wi) and np.array_equal(bits(ga), bits(wa))
    rows_b = np.arange(0, m, 3)
    wi, wa = R.knn(counts, 64, rows_b=rows_b, squared=True)
    gi, gd = K.region_knn(counts, 64, rows_b=rows_b)
    assert np.array_equal(gi, wi)
    assert_sqrt_of(gd, wa, "host entry, cross")


# ------------------------------------------------------------------ pipeline

def test_pipeline_scan_spectra_knn(ctx):
    """The planted-repeat scan of the distance tests: the poly-A copies of 150
    and 420 bases between N runs have proportional spectra, so each is the
    other's nearest neighbour at exactly 0."""
    import torch
    from kmer_spans_amd import device as D
    k = 7
    rng = np.random.default_rng(17)
    s = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=120_000)
    plants = {"a150": (20_000, b"A" * 150), "a420": (50_000, b"A" * 420), "ca": (80_000, b"CA" * 120),
              "ca2": (100_000, b"CA" * 60)}
    for name, (at, unit) in plants.items():
        flank = ord("N") if name.startswith("a") else ord("G")
        s[at - 30:at] = flank
        s[at:at + len(unit)] = np.frombuffer(unit, dtype=np.uint8)
        s[at + len(unit):at + len(unit) + 30] = flank
    ds = D.from_host([s.tobytes()], "cuda")
    kc = torch.zeros(4 ** k, dtype=torch.int32, device="cuda")
    words = D.count(ctx, ds, k, kc)
    tab = D.DeviceTable.from_counts(ctx, kc, k, "rank", total=words, thr=0.75, expand=True)
    pos, _, _ = D.scan(ctx, ds, k, tab, 20, 5.0)
    nreg = pos.shape[1]
    assert nreg >= 4
    sp, _, _ = D.region_spectra(ctx, ds, pos, q=4, both_strands=True, entropy=False)

    def region_in(name):
        at, unit = plants[name]  # the copy covers 1-based at + 1 .. at + len(unit)
        hit = [r for r in range(nreg)
               if min(pos[2, r], at + len(unit)) - max(pos[1, r], at + 1) + 1 > len(unit) // 2]
        assert len(hit) == 1, (name, pos.T.tolist())
        return hit[0]
    ra, rb = region_in("a150"), region_in("a420")
    kk = min(3, nreg - 1)
    index, d, _ = D.region_knn(ctx, sp, kk)
    index, d = index.cpu().numpy(), d.cpu().numpy()
    assert index[ra, 0] == rb and index[rb, 0] == ra and d[ra, 0] == 0.0 and d[rb, 0] == 0.0
    host = sp.cpu().numpy().view(np.uint32)
    wi, wa = R.knn(host, kk, squared=True)
    assert np.array_equal(index, wi)
    assert_sqrt_of(d, wa, "pipeline")


# -------------------------------------------------------- scale: invariants

def test_scale_invariants(ctx):
    """m = 8,192, ncol = 256, k = 10: the full model is slow here, so what must
    hold of any result, and the model's list for 64 sampled rows."""
    import torch
    from kmer_spans_amd import device as D
    m, ncol, k = 8192, 256, 10
    counts = random_counts(np.random.default_rng(8192), m, ncol)
    dev = to_dev(counts)
    index, acc, st = D.region_knn(ctx, dev, k, squared=True)
    print(f"m = {m}: ms_normalise {st['ms_normalise']:.3f} ms_select {st['ms_select']:.3f} ms_merge "
          f"{st['ms_merge']:.3f} splits {st['n_splits']} x {st['tiles_per_split']} tiles, panel {st['panel_bytes']} "
          f"work {st['work_bytes']}")
    assert int(index.min()) >= 0 and int(index.max()) < m
    own = torch.arange(m, device="cuda")[:, None]
    assert not bool((index == own).any())  # no row holds its own position
    later, earlier = acc[:, 1:], acc[:, :-1]
    assert bool(((later > earlier) | ((later == earlier) & (index[:, 1:] > index[:, :-1]))).all())  # (dist, index)
    block, _ = D.region_distances(ctx, dev, torch.arange(m, device="cuda"), torch.arange(m, device="cuda"),
                                  squared=True)
    assert torch.equal(torch.gather(block, 1, index).view(torch.int64), acc.view(torch.int64))
    del block
    sample = np.sort(np.random.default_rng(1).choice(m, size=64, replace=False))
    p = profiles(counts)
    wi, wa = R.select(sqdist(p[sample], p), k, sample)
    assert np.array_equal(index.cpu().numpy()[sample], wi)
    assert np.array_equal(bits(acc.cpu().numpy()[sample]), bits(wa))
    assert st["panel_bytes"] >= 8 * m * ncol
