"""Pairwise distances between region spectra on the device
(ks_spectra_dist_dev / ks_spectra_cross_dist_dev and the host forms) against
the host reference of tests/test_spectra_dist.py: the squared distances bit
for bit, the plain ones within 1 ulp of np.sqrt of those (exactly 0 where the
square is 0, NaN where it is NaN; a NaN equals a NaN whatever its sign bit).  Runs on an MI355X (pytest -m gpu)."""
import numpy as np
import pytest

from tests.test_spectra_dist import (bits, condensed_pairs, pair_offsets, profiles, random_counts, ref_condensed_sq,
                                     ref_cross_sq, ref_sq)

pytestmark = pytest.mark.gpu


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


def same_bits(got, want) -> np.ndarray:
    """Elementwise: the same bits, or NaN on both sides (the contract says NaN
    for an empty row; the sign and payload of a NaN are nobody's result: the
    host's 0 / 0 sets the sign bit, the device's does not)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))


def assert_sqrt_of(got, sq, what=""):
    """got is within 1 ulp of np.sqrt(sq): 0 where sq is 0, NaN where it is NaN."""
    got, sq = np.asarray(got).ravel(), np.asarray(sq).ravel()
    nan = np.isnan(sq)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN pattern")
    assert not got[sq == 0].any(), (what, "sqrt of an exact 0")
    with np.errstate(invalid="ignore"):
        want = np.sqrt(sq)
    diff = np.abs(bits(got[~nan]).astype(np.int64) - bits(want[~nan]).astype(np.int64))
    worst = int(diff.max(initial=0))
    print(f"{what}: device sqrt differs from np.sqrt by at most {worst} ulp over {diff.size} values")
    assert worst <= 1, (what, worst)
    return worst


def check_device(ctx, counts, rows=None, rows_b=None, want_sq=None, what="", dev_counts=None):
    """device.region_distances, squared and plain, against the host reference."""
    from kmer_spans_amd import device as D
    dc = to_dev(counts) if dev_counts is None else dev_counts
    if want_sq is None:
        want_sq = ref_condensed_sq(counts, rows) if rows_b is None else ref_cross_sq(counts, rows, rows_b)
    sq, st = D.region_distances(ctx, dc, rows=rows, rows_b=rows_b, squared=True)
    assert tuple(sq.shape) == want_sq.shape, (what, sq.shape, want_sq.shape)
    got = sq.cpu().numpy()
    same = same_bits(got, want_sq)
    assert same.all(), (what, "squared distances differ at", np.argwhere(~same)[:8].tolist(),
                        got[~same][:4], want_sq[~same][:4])
    assert st["n_pairs"] == want_sq.size and st["bytes_written"] == 8 * want_sq.size, (what, st)
    d, _ = D.region_distances(ctx, dc, rows=rows, rows_b=rows_b)
    assert_sqrt_of(d.cpu().numpy(), want_sq, what)
    return got


# ------------------------------------------------------------ known answers

def test_known_answer(ctx):
    import kmer_spans_amd as K
    c = np.array([[1, 1, 0, 0], [0, 0, 2, 2], [3, 1, 0, 0], [5, 5, 0, 0]], dtype=np.uint32)
    want = np.array([1.0, 0.125, 0.0, 1.125, 1.0, 0.125])  # pairs 01 02 03 12 13 23
    got = check_device(ctx, c, what="known")
    assert got.tolist() == want.tolist()
    assert K.region_distances(c, squared=True).tolist() == want.tolist()  # api -> host entry
    assert_sqrt_of(K.region_distances(c), want, "known, host entry")
    x = K.region_distances(c, rows=[3, 1], rows_b=[0, 2, 1], squared=True)
    assert x.tolist() == [[0.0, 0.125, 1.0], [1.0, 1.125, 0.0]]
    assert K.region_distances(c.astype(np.int64), rows=[2, 0], squared=True).tolist() == [0.125]


# --------------------------------------------- tile edges, chunks, diagonal

@pytest.mark.parametrize("ncol", [4, 16, 256, 4096])
@pytest.mark.parametrize("m", [2, 3, 63, 64, 65, 129, 200])
def test_random_counts(ctx, m, ncol):
    rng = np.random.default_rng(1000 * m + ncol)
    check_device(ctx, random_counts(rng, m, ncol), what=f"m={m} ncol={ncol}")


@pytest.mark.parametrize("ncol", [1, 17, 33])
def test_ncol_off_the_chunk(ctx, ncol):
    """ncol below one k chunk of 16, and one past a whole number of chunks."""
    rng = np.random.default_rng(ncol)
    c = random_counts(rng, 70, ncol)
    check_device(ctx, c, what=f"ncol={ncol}")
    check_device(ctx, c, rows=None, rows_b=np.arange(5, 70, 3), what=f"cross ncol={ncol}")


def test_many_tiles(ctx):
    """m = 2,563 at ncol = 16: 41 tile rows, 861 tiles through the triangular mapping."""
    rng = np.random.default_rng(2563)
    check_device(ctx, random_counts(rng, 2563, 16), what="many tiles")


# ------------------------------------------------------- the contract's edges

def test_large_bins(ctx):
    """Bins up to 2^32 - 1 and a row sum near 2^44."""
    rng = np.random.default_rng(44)
    ncol = 4096
    c = rng.integers(0, 2 ** 32, size=(9, ncol), dtype=np.uint64).astype(np.uint32)
    c[0] = 0xFFFFFFFF                       # T = 4096 * (2^32 - 1) = 2^44 - 4096
    c[1] = 0xFFFFFFFF
    c[1, 7] = 0
    c[2, :] = 0
    c[2, 4095] = 0xFFFFFFFF                 # one huge bin
    c[3, :] = 1                             # proportional to row 0
    assert int(c[0].astype(np.uint64).sum()) == 2 ** 44 - 4096
    got = check_device(ctx, c, what="large bins")
    assert got[0] != 0.0 and got[2] == 0.0  # pairs (0, 1) and (0, 3)
    c16 = c[:, :16].copy()
    check_device(ctx, c16, rows=[0, 1, 2, 3, 8], rows_b=[8, 0, 4], what="large bins, cross")


def test_empty_row_is_nan(ctx):
    rng = np.random.default_rng(5)
    c = random_counts(rng, 67, 16)
    c[0] = 0
    c[65] = 0
    got = check_device(ctx, c, what="empty rows")
    i, j = condensed_pairs(67)
    empty = np.isin(i, (0, 65)) | np.isin(j, (0, 65))
    assert np.isnan(got[empty]).all() and not np.isnan(got[~empty]).any()
    x = check_device(ctx, c, rows=[0, 3], rows_b=[65, 4, 0], what="empty rows, cross")
    assert np.isnan(x[0]).all() and np.isnan(x[1, [0, 2]]).all() and not np.isnan(x[1, 1])


def test_proportional_rows_are_at_zero(ctx):
    """A row and its multiples x2, x3, x1000: repeats of one unit at different
    lengths cluster at distance exactly 0, not at 1e-9."""
    rng = np.random.default_rng(6)
    for ncol in (4, 256):
        c = random_counts(rng, 70, ncol, hi=4000)
        base = c[10].astype(np.uint64)
        c[11], c[40], c[69] = (base * 2).astype(np.uint32), (base * 3).astype(np.uint32), (base * 1000).astype(np.uint32)
        got = check_device(ctx, c, what=f"proportional ncol={ncol}")
        i, j = condensed_pairs(70)
        fam = np.isin(i, (10, 11, 40, 69)) & np.isin(j, (10, 11, 40, 69))
        assert fam.sum() == 6 and not got[fam].any()
        x = check_device(ctx, c, rows=[69, 10, 3], rows_b=[11, 40, 10, 69, 5], what="proportional, cross")
        assert not x[:2, :4].any()


def test_row_selections(ctx):
    import torch
    rng = np.random.default_rng(7)
    c = random_counts(rng, 150, 16)
    dc = to_dev(c)
    full = check_device(ctx, c, dev_counts=dc, what="all rows")
    rev = np.arange(149, -1, -1)
    got = check_device(ctx, c, rows=rev, dev_counts=dc, what="reversed")
    i, j = condensed_pairs(150)
    assert np.array_equal(bits(got), bits(full[pair_offsets(149 - j, 149 - i, 150)]))  # d(i, j) = d(j, i): same bits
    rep = np.array([5, 5, 9, 140, 5, 9, 0, 149, 140] * 9)  # 81 rows: repeats, two tile rows
    got = check_device(ctx, c, rows=rep, dev_counts=dc, what="repeats")
    i, j = condensed_pairs(rep.size)
    assert not got[rep[i] == rep[j]].any()
    sub = np.sort(rng.permutation(150)[:77])
    got = check_device(ctx, c, rows=sub, dev_counts=dc, what="subset")
    i, j = condensed_pairs(77)
    assert np.array_equal(bits(got), bits(full[pair_offsets(sub[i], sub[j], 150)]))
    # selections as CUDA tensors
    check_device(ctx, c, rows=torch.from_numpy(sub).cuda(), dev_counts=dc, want_sq=ref_condensed_sq(c, sub),
                 what="subset (tensor)")


def test_cross_form(ctx):
    import torch
    rng = np.random.default_rng(8)
    c = random_counts(rng, 200, 64)
    dc = to_dev(c)
    full = check_device(ctx, c, dev_counts=dc, what="condensed")
    a, b = np.arange(0, 130), np.arange(130, 200)  # disjoint, a < b: the same pairs as the condensed form
    x = check_device(ctx, c, rows=a, rows_b=b, dev_counts=dc, what="cross")
    ii, jj = np.meshgrid(a, b, indexing="ij")
    assert np.array_equal(bits(x), bits(full[pair_offsets(ii.ravel(), jj.ravel(), 200)].reshape(130, 70)))
    xt = check_device(ctx, c, rows=b, rows_b=a, dev_counts=dc, what="cross, swapped")
    assert np.array_equal(bits(xt.T), bits(x))
    one_a = check_device(ctx, c, rows=[17], rows_b=b, dev_counts=dc, what="na = 1")
    one_b = check_device(ctx, c, rows=a, rows_b=[199], dev_counts=dc, what="nb = 1")
    assert np.array_equal(bits(one_a[0]), bits(x[17])) and np.array_equal(bits(one_b[:, 0]), bits(x[:, 69]))
    # rows=None: all rows against a few centroids; overlapping selections hold exact zeros
    cen = check_device(ctx, c, rows=None, rows_b=torch.tensor([3, 150, 3], device="cuda"), dev_counts=dc,
                       want_sq=ref_cross_sq(c, None, [3, 150, 3]), what="centroids")
    assert cen[3, 0] == 0.0 and cen[150, 1] == 0.0 and cen[3, 2] == 0.0


def test_out_reuse(ctx):
    import torch
    from kmer_spans_amd import device as D
    import kmer_spans_amd as K
    rng = np.random.default_rng(9)
    c = random_counts(rng, 90, 16)
    dc = to_dev(c)
    want = ref_condensed_sq(c)
    out = torch.full((want.size,), -7.0, dtype=torch.float64, device="cuda")
    res, _ = D.region_distances(ctx, dc, squared=True, out=out)
    assert res.data_ptr() == out.data_ptr() and np.array_equal(bits(out.cpu().numpy()), bits(want))
    b = np.array([4, 80, 33])
    out2 = out[:90 * 3]
    res, _ = D.region_distances(ctx, dc, rows_b=b, squared=True, out=out2)
    assert res.shape == (90, 3) and res.data_ptr() == out.data_ptr()
    assert np.array_equal(bits(res.cpu().numpy()), bits(ref_cross_sq(c, None, b)))
    assert np.array_equal(bits(out[270:].cpu().numpy()), bits(want[270:]))  # nothing past the block was written
    for bad in (out[:5], out.to(torch.float32), out.cpu()):
        with pytest.raises(K.KmerSpansError, match="out must be"):
            D.region_distances(ctx, dc, squared=True, out=bad)
    # the host entry gives the same bits
    assert np.array_equal(bits(K.region_distances(c, squared=True)), bits(want))
    assert np.array_equal(bits(K.region_distances(c, rows_b=b, squared=True)), bits(ref_cross_sq(c, None, b)))


# ----------------------------------------------------- device-entry validation

@pytest.mark.parametrize("form", ["condensed", "cross_a", "cross_b"])
def test_device_entry_rejects_a_bad_row_index(ctx, form):
    """The index check runs on the device before anything is written: one bad
    index among good ones is an argument error naming its position, the
    output is untouched, and the context is fine afterwards."""
    import torch
    import kmer_spans_amd as K
    from kmer_spans_amd import device as D
    rng = np.random.default_rng(10)
    c = random_counts(rng, 100, 16)
    dc = to_dev(c)
    good = np.arange(0, 100, 1)[::-1].copy()
    bad = good.copy()
    bad[70] = 100 if form != "cross_b" else -1
    if form == "condensed":
        out = torch.full((100 * 99 // 2,), -7.0, dtype=torch.float64, device="cuda")
        kw, msg = dict(rows=bad), "^row index 70 out of range$"
        ok = dict(rows=good)
    elif form == "cross_a":
        out = torch.full((100 * 5,), -7.0, dtype=torch.float64, device="cuda")
        kw, msg = dict(rows=bad, rows_b=[1, 2, 3, 4, 5]), "^row index 70 out of range$"
        ok = dict(rows=good, rows_b=[1, 2, 3, 4, 5])
    else:
        out = torch.full((5 * 100,), -7.0, dtype=torch.float64, device="cuda")
        kw, msg = dict(rows=[1, 2, 3, 4, 5], rows_b=bad), "^row index 70 of the second selection out of range$"
        ok = dict(rows=[1, 2, 3, 4, 5], rows_b=good)
    with pytest.raises(K.KmerSpansError, match=msg):
        D.region_distances(ctx, dc, out=out, **kw)
    assert bool((out == -7.0).all())
    check_device(ctx, c, dev_counts=dc, what="after a rejected call", **ok)


# ------------------------------------------------------------------ pipeline

def test_pipeline_scan_spectra_distances(ctx):
    """A planted-repeat scan, device.region_spectra on its regions, then
    device.region_distances on the counts left on the device: bit for bit the
    host reference on the downloaded counts.  Two planted copies of one repeat
    at different lengths, poly-A of 150 and of 420 bases, lie between N runs:
    a region cannot cross an N, so theirs hold nothing but A, every tetramer
    window inside is AAAA, and the folded counts are (w, w) on AAAA / TTTT
    whatever the widths -- proportional, which is checked here on the host from
    the downloaded counts; the two regions then sit at exactly 0.  (Copies in
    random flanks, like the two (CA)n here, take in a flank base or two as the
    scan's maximum falls, and are held to the bitwise match only.)"""
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
    counts = torch.zeros(4 ** k, dtype=torch.int32, device="cuda")
    words = D.count(ctx, ds, k, counts)
    tab = D.DeviceTable.from_counts(ctx, counts, k, "rank", total=words, thr=0.75, expand=True)
    pos, _, _ = D.scan(ctx, ds, k, tab, 20, 5.0)
    assert pos.shape[1] >= 4
    sp, _, _ = D.region_spectra(ctx, ds, pos, q=4, both_strands=True, entropy=False)
    host = sp.cpu().numpy().view(np.uint32)
    R = pos.shape[1]

    def region_in(name):
        at, unit = plants[name]  # the copy covers 1-based at + 1 .. at + len(unit)
        hit = [r for r in range(R)
               if min(pos[2, r], at + len(unit)) - max(pos[1, r], at + 1) + 1 > len(unit) // 2]
        assert len(hit) == 1, (name, pos.T.tolist())
        return hit[0]
    ra, rb = region_in("a150"), region_in("a420")
    sel = np.unique(np.concatenate([np.arange(min(R, 200)), [ra, rb]]))  # the reference loop stays short
    got = check_device(ctx, host, rows=sel, dev_counts=sp, what="pipeline")
    full, _ = D.region_distances(ctx, sp, squared=True)  # every region, selection-free
    i, j = condensed_pairs(sel.size)
    assert np.array_equal(bits(full.cpu().numpy()[pair_offsets(sel[i], sel[j], R)]), bits(got))
    ca, cb = [int(x) for x in host[ra]], [int(x) for x in host[rb]]
    proportional = sum(ca) > 0 and sum(cb) > 0 and all(x * sum(cb) == y * sum(ca) for x, y in zip(ca, cb))
    print(f"{R} regions; poly-A regions {pos[:, ra].tolist()} and {pos[:, rb].tolist()}: "
          f"proportional counts: {proportional}")
    x, _ = D.region_distances(ctx, sp, rows=[ra], rows_b=[rb], squared=True)
    ia, ib = int(np.searchsorted(sel, min(ra, rb))), int(np.searchsorted(sel, max(ra, rb)))
    at = pair_offsets([ia], [ib], sel.size)[0]
    assert bits(x.cpu().numpy())[0, 0] == bits(got)[at]
    assert proportional and sum(ca) != sum(cb), (ca, cb)
    assert got[at] == 0.0 and float(x[0, 0]) == 0.0


# ------------------------------------------------------ beyond 2^31 entries

def test_offsets_beyond_int32(ctx):
    """m = 66,000 at ncol = 4: 2,177,967,000 entries (17.4 GB).  100,000 random
    pairs, the first and last 1,000 entries and the entries either side of
    offset 2^31 against the host reference; gathered on the device, only the
    samples come back."""
    import torch
    from kmer_spans_amd import device as D
    m, ncol = 66_000, 4
    free, _ = torch.cuda.mem_get_info()
    if free < 24 * 2 ** 30:
        pytest.skip(f"{free / 2 ** 30:.1f} GiB free, the output alone takes 17.4 GB")
    total = m * (m - 1) // 2
    assert total > 2 ** 31
    rng = np.random.default_rng(66)
    c = random_counts(rng, m, ncol, hi=100_000)
    c[123] = 0
    c[65_999] = c[0] * 7
    p = profiles(c)
    starts = np.array([i * m - i * (i + 1) // 2 for i in range(m)], dtype=np.int64)  # offset of pair (i, i + 1)
    off = np.concatenate([np.arange(1000), np.arange(total - 1000, total), np.arange(2 ** 31 - 8, 2 ** 31 + 8)])
    i = np.searchsorted(starts[:m - 1], off, side="right") - 1
    j = off - starts[i] + i + 1
    ri = rng.integers(0, m - 1, 100_000)
    rj = ri + 1 + (rng.random(100_000) * (m - 1 - ri)).astype(np.int64)
    rj = np.minimum(rj, m - 1)
    i, j = np.concatenate([i, ri, [0, 122]]), np.concatenate([j, rj, [65_999, 123]])
    off = i * m - i * (i + 1) // 2 + (j - i - 1)
    assert (i < j).all() and off.min() == 0 and off.max() == total - 1 and (off >= 2 ** 31).sum() > 1000
    want = ref_sq(p, i, j)
    out = torch.empty(total, dtype=torch.float64, device="cuda")
    dc = to_dev(c)
    idx = torch.from_numpy(off).cuda()
    _, st = D.region_distances(ctx, dc, squared=True, out=out)
    got = out[idx].cpu().numpy()
    assert st["n_pairs"] == total
    same = same_bits(got, want)
    assert same.all(), (np.argwhere(~same)[:8].tolist(), off[~same][:8].tolist())
    assert got[-2] == 0.0 and np.isnan(got[-1])
    D.region_distances(ctx, dc, out=out)
    assert_sqrt_of(out[idx].cpu().numpy(), want, "beyond 2^31")
    del out
    torch.cuda.empty_cache()
