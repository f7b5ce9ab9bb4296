"""The k nearest regions by spectrum (ks_spectra_knn, include/kmer_spans.h):
the host model of tests/knnref.py against lists worked by hand, against a plain
nested Python loop, the tie rules, and the argument checks of both C entries
and both Python wrappers, which happen before any device use -- this file runs
without a GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from kmer_spans_amd import _lib
from tests import knnref as R
from tests.kmeansref import profiles, sqdist
from tests.test_nj import bits

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kmer_spans.h")

# x = 0, .125, .375, .5, 1 on the line (x, 1 - x): the squared distance of two rows is 2 (x - x')^2
LINE5 = np.array([[0, 8], [1, 7], [3, 5], [4, 4], [8, 0]], dtype=np.uint32)


def equal_root_case():
    """Query row 0 = (1, 0, 0) against rows 1 and 2 = (0, 1/2 + j 2^-28, 1/2 -
    j 2^-28) with j = 10 and j = 9: the squared distances 1.5 + 2 j^2 2^-56
    differ (by 2 ulp) and their square roots are the same double.  The farther
    one has the lower position, so ordering by the root and then the position
    would swap them.  Rows 3 and 4 are farther than both.
    Returns (counts, rows, rows_b)."""
    h = 2 ** 27
    counts = np.array([[5, 0, 0], [0, h + 10, h - 10], [0, h + 9, h - 9], [0, h + 4000, h - 4000], [0, 1, 0]],
                      dtype=np.uint32)
    return counts, np.array([0], dtype=np.int64), np.array([1, 2, 3, 4], dtype=np.int64)


def proportional_family_case(k: int, at: int = 60, m: int = None):
    """m rows of 4 columns; positions at .. at + 3k - 1 are proportional to row
    `at` (multiples 1 .. 3k of (1, 2, 3, 5)), so each is at exactly 0 from the
    others; every other row is random.  Returns counts."""
    m = at + 3 * k + 40 if m is None else m
    rng = np.random.default_rng(k * 1000 + at)
    counts = rng.integers(1, 200, size=(m, 4)).astype(np.uint32)
    for t in range(3 * k):
        counts[at + t] = np.array([1, 2, 3, 5], dtype=np.uint32) * (t + 1)
    return counts


# ------------------------------------------------------------- known answers

def test_five_points_on_a_line():
    """Profiles (x, 1 - x) with x = 0, .125, .375, .5, 1; acc = 2 (x - x')^2, every value exact in binary:
             0        1        2        3        4
      0      -     .03125   .28125     .5        2
      1   .03125      -      .125    .28125   1.53125
      2   .28125    .125       -     .03125   .78125
      3     .5     .28125   .03125      -       .5
      4      2    1.53125   .78125     .5        -
    Self form, nearest first: row 0: 1 2 3 4; row 1: 0 2 3 4; row 2: 3 1 0 4; row 3: 2 1 0 4 (rows 0 and 4 tie
    at .5: the lower position first); row 4: 3 2 1 0.
    Cross form, queries rows (0, 3), candidates rows (4, 2, 0, 1) at positions 0 .. 3: query 0 has acc (2, .28125,
    0, .03125): positions 2 3 1 0; query 1 (row 3) has (.5, .03125, .5, .28125): positions 1 3 0 2 (the tie at .5
    again by position)."""
    full = [[1, 2, 3, 4], [0, 2, 3, 4], [3, 1, 0, 4], [2, 1, 0, 4], [3, 2, 1, 0]]
    dfull = [[.03125, .28125, .5, 2], [.03125, .125, .28125, 1.53125], [.03125, .125, .28125, .78125],
             [.03125, .28125, .5, .5], [.5, .78125, 1.53125, 2]]
    for k in (1, 2, 4):
        index, acc = R.knn(LINE5, k, squared=True)
        assert index.dtype == np.int64 and index.tolist() == [row[:k] for row in full]
        assert acc.tolist() == [row[:k] for row in dfull]
        _, d = R.knn(LINE5, k)
        assert np.array_equal(bits(d), bits(np.sqrt(np.array([row[:k] for row in dfull]))))
    cross = [[2, 3, 1, 0], [1, 3, 0, 2]]
    dcross = [[0, .03125, .28125, 2], [.03125, .28125, .5, .5]]
    for k in (1, 2, 4):
        index, acc = R.knn(LINE5, k, rows=[0, 3], rows_b=[4, 2, 0, 1], squared=True)
        assert index.tolist() == [row[:k] for row in cross] and acc.tolist() == [row[:k] for row in dcross]


def test_model_is_the_plain_loop():
    """Nested Python loops over Python floats and sorted() on (acc, position) tuples, bit for bit."""
    rng = np.random.default_rng(11)
    counts = rng.integers(0, 6, size=(70, 5)).astype(np.uint32)  # small counts: proportional rows and ties occur
    counts[:, 0] += 1
    rows = rng.integers(0, 70, size=40)
    rows_b = rng.integers(0, 70, size=55)
    for self_form in (True, False):
        pa = profiles(counts, rows)
        pb = pa if self_form else profiles(counts, rows_b)
        k = 9
        index, acc = R.knn(counts, k, rows=rows, rows_b=None if self_form else rows_b, squared=True)
        ties = 0
        for s in range(pa.shape[0]):
            cand = []
            for j in range(pb.shape[0]):
                if self_form and j == s:
                    continue
                a = 0.0
                for c in range(pa.shape[1]):
                    d = float(pa[s, c]) - float(pb[j, c])
                    a = a + d * d
                cand.append((a, j))
            best = sorted(cand)[:k]
            assert [j for _, j in best] == index[s].tolist()
            assert [a for a, _ in best] == acc[s].tolist()
            ties += len({a for a, _ in best}) < k
        assert ties > 0  # the position decided somewhere


# ---------------------------------------------------------------------- ties

def test_all_rows_equal():
    counts = np.tile(np.array([[3, 1, 4]], dtype=np.uint32), (9, 1)) * np.arange(1, 10, dtype=np.uint32)[:, None]
    index, acc = R.knn(counts, 4, squared=True)
    assert not acc.any()
    for s in range(9):
        assert index[s].tolist() == [j for j in range(9) if j != s][:4]
    index, _ = R.knn(counts, 4, rows=[0, 1], rows_b=np.arange(9))
    assert index.tolist() == [[0, 1, 2, 3], [0, 1, 2, 3]]  # the cross form keeps every candidate


def test_proportional_family_larger_than_k():
    k, at = 5, 60
    counts = proportional_family_case(k, at)
    index, acc = R.knn(counts, k, squared=True)
    for s in range(at, at + 3 * k):
        assert not acc[s].any()
        assert index[s].tolist() == [j for j in range(at, at + 3 * k) if j != s][:k]  # the lowest positions win


def test_equal_roots_are_ordered_by_the_squared_value():
    counts, rows, rows_b = equal_root_case()
    acc = sqdist(profiles(counts, rows), profiles(counts, rows_b))[0]
    assert acc[1] < acc[0] and np.sqrt(acc[1]) == np.sqrt(acc[0])  # such a pair exists
    assert acc[0] < acc[2] < acc[3]
    index, d = R.knn(counts, 3, rows=rows, rows_b=rows_b)
    assert index.tolist() == [[1, 0, 2]] and d[0, 0] == d[0, 1]
    by_root = np.lexsort((np.arange(4), np.sqrt(acc)))[:3]
    assert by_root.tolist() == [0, 1, 2]  # what sorting the roots would give


def test_a_repeated_row_finds_its_copy_and_not_itself():
    rng = np.random.default_rng(2)
    counts = rng.integers(1, 50, size=(30, 6)).astype(np.uint32)
    rows = np.array([4, 9, 4, 20, 9, 1], dtype=np.int64)
    index, acc = R.knn(counts, 2, rows=rows, squared=True)
    assert index[0, 0] == 2 and index[2, 0] == 0 and index[1, 0] == 4 and index[4, 0] == 1
    assert not acc[[0, 1, 2, 4], 0].any() and (acc[[3, 5], 0] > 0).all()
    assert all(s not in index[s] for s in range(rows.size))


def test_k_equal_to_the_number_of_candidates():
    rng = np.random.default_rng(7)
    counts = rng.integers(1, 50, size=(12, 6)).astype(np.uint32)
    index, _ = R.knn(counts, 11)
    for s in range(12):
        assert sorted(index[s].tolist()) == [j for j in range(12) if j != s]
    index, _ = R.knn(counts, 5, rows=[0, 1, 2], rows_b=[3, 3, 4, 0, 11])
    assert all(sorted(row.tolist()) == [0, 1, 2, 3, 4] for row in index)
    with pytest.raises(AssertionError, match="k exceeds"):
        R.knn(counts, 12)
    with pytest.raises(AssertionError, match="k exceeds"):
        R.knn(counts, 6, rows=[0, 1, 2], rows_b=[3, 3, 4, 0, 11])


# ------------------------------------------------------------ argument checks

def _knn(dev, na=5, ncol=4, k=2, flags=0, n=None, rows=None, rows_b=None, nb=None, null=(), sp=None):
    """A ks_spectra_knn(_dev) call that must be refused before any device use."""
    L = _lib.load()
    m = max(na, 1)
    b = {"sp": np.ones((m if n is None else max(n, 1), max(min(ncol, 64), 1)), dtype=np.uint32),
         "index": np.full((m, 64), -7, dtype=np.int64), "dist": np.full((m, 64), -7.5)}
    if sp is not None:
        b["sp"] = np.ascontiguousarray(sp, dtype=np.uint32)
    ptr = {key: (None if key in null else v.ctypes.data) for key, v in b.items()}
    ra = None if rows is None else np.ascontiguousarray(rows, dtype=np.int64)
    rb = None if rows_b is None else np.ascontiguousarray(rows_b, dtype=np.int64)
    args = [None, ptr["sp"], b["sp"].shape[0] if n is None else n, ncol, None if ra is None else ra.ctypes.data, na,
            None if rb is None else rb.ctypes.data, (0 if rb is None else rb.size) if nb is None else nb, k, flags,
            ptr["index"], ptr["dist"]]
    rc = L.ks_spectra_knn_dev(*args, None) if dev else L.ks_spectra_knn(*args)
    assert (b["index"] == -7).all() and (b["dist"] == -7.5).all(), "an output was written"
    return rc, L.ks_last_error().decode()


@pytest.mark.parametrize("dev", [False, True])
def test_entries_validate_before_any_device_call(dev):
    for na in (0, -2):
        rc, msg = _knn(dev, na=na)
        assert rc != 0 and "at least 1 query row" in msg, msg
    for nb in (0, -1):
        rc, msg = _knn(dev, rows_b=[0, 1], nb=nb)
        assert rc != 0 and "at least 1 candidate row" in msg, msg
    for ncol in (0, -1, _lib.KS_DIST_MAX_NCOL + 1):
        rc, msg = _knn(dev, ncol=ncol)
        assert rc != 0 and "ncol must be between 1 and 4096" in msg, msg
    for k in (0, -1, _lib.KS_KNN_MAX_K + 1):
        rc, msg = _knn(dev, k=k)
        assert rc != 0 and "k must be between 1 and 64" in msg, msg
    for flags in (2, 3, -1):
        rc, msg = _knn(dev, flags=flags)
        assert rc != 0 and "unknown flags" in msg, msg
    rc, msg = _knn(dev, n=3)  # rows NULL and na = 5 > n
    assert rc != 0 and "exceeds n = 3" in msg, msg
    rc, msg = _knn(dev, null=("sp",))
    assert rc != 0 and "null spectra" in msg
    for out in ("index", "dist"):
        rc, msg = _knn(dev, null=(out,))
        assert rc != 0 and "null output" in msg, out


def test_host_entry_checks_indices_sums_and_k_in_that_order():
    """The host entry finds a bad index, an empty row and a k above the candidates before any device call:
    indices first (queries, then candidates), then empty rows (queries, then candidates), then k."""
    sp = np.ones((6, 4), dtype=np.uint32)
    sp[3] = 0
    rc, msg = _knn(False, na=6, sp=sp)
    assert rc != 0 and msg == "row 3 has no counts", msg
    rc, msg = _knn(False, na=5, sp=sp, rows=[0, 3, 9, 3, -1])
    assert rc != 0 and msg == "row index 2 out of range", msg
    rc, msg = _knn(False, na=5, sp=sp, rows=[4, 4, 3, 3, 0])
    assert rc != 0 and msg == "row 2 has no counts", msg
    rc, msg = _knn(False, na=2, sp=sp, rows=[0, 1], rows_b=[2, 6, -1])
    assert rc != 0 and msg == "row index 1 of the second selection out of range", msg
    rc, msg = _knn(False, na=2, sp=sp, rows=[0, 1], rows_b=[2, 3, 3])
    assert rc != 0 and msg == "row 1 of the second selection has no counts", msg
    # precedence: a candidate's bad index before a query's empty row; a query's empty row before a candidate's
    rc, msg = _knn(False, na=2, sp=sp, rows=[3, 1], rows_b=[2, 6])
    assert rc != 0 and msg == "row index 1 of the second selection out of range", msg
    rc, msg = _knn(False, na=2, sp=sp, rows=[1, 3], rows_b=[3, 2])
    assert rc != 0 and msg == "row 1 has no counts", msg
    rc, msg = _knn(False, na=2, sp=sp, rows=[9, 1], rows_b=[2, 6])
    assert rc != 0 and msg == "row index 0 out of range", msg
    # k comes last
    rc, msg = _knn(False, na=3, sp=sp, rows=[0, 1, 2], k=3)
    assert rc != 0 and msg == "k exceeds the number of candidate rows (k = 3, 2 candidates)", msg
    rc, msg = _knn(False, na=3, sp=sp, rows=[0, 1, 2], rows_b=[4, 5], k=3)
    assert rc != 0 and msg == "k exceeds the number of candidate rows (k = 3, 2 candidates)", msg
    rc, msg = _knn(False, na=1, sp=sp, rows=[0], k=1)
    assert rc != 0 and msg == "k exceeds the number of candidate rows (k = 1, 0 candidates)", msg
    rc, msg = _knn(False, na=3, sp=sp, rows=[0, 3, 2], k=3)
    assert rc != 0 and msg == "row 1 has no counts", msg
    rc, msg = _knn(False, na=3, sp=sp, rows=[0, 1, 2], rows_b=[7], k=3)
    assert rc != 0 and msg == "row index 0 of the second selection out of range", msg


def test_python_argument_checks():
    import kmer_spans_amd as K
    ok = np.ones((5, 4), dtype=np.uint32)
    for bad in (np.ones(5), np.ones((5, 4)), np.full((5, 4), -1)):
        with pytest.raises(K.KmerSpansError, match="counts"):
            K.region_knn(bad, 2)
    for bad in (1.5, "2", None, True):
        with pytest.raises(K.KmerSpansError, match="k must be an integer"):
            K.region_knn(ok, bad)
    for bad in (0, -3, 65):
        with pytest.raises(K.KmerSpansError, match="^k must be between 1 and 64"):
            K.region_knn(ok, bad)
    with pytest.raises(K.KmerSpansError, match="not an int32"):
        K.region_knn(ok, 2 ** 40)
    for bad in ([[0, 1]], [0.5, 1.0]):
        with pytest.raises(K.KmerSpansError, match="rows must be a 1-d array"):
            K.region_knn(ok, 1, rows=bad)
        with pytest.raises(K.KmerSpansError, match="rows_b must be a 1-d array"):
            K.region_knn(ok, 1, rows_b=bad)
    with pytest.raises(K.KmerSpansError, match="at least 1 candidate row"):
        K.region_knn(ok, 1, rows_b=[])
    with pytest.raises(K.KmerSpansError, match="^row index 1 out of range$"):
        K.region_knn(ok, 1, rows=[0, 5])
    with pytest.raises(K.KmerSpansError, match="^row index 0 of the second selection out of range$"):
        K.region_knn(ok, 1, rows_b=[-1])
    with pytest.raises(K.KmerSpansError, match="^k exceeds the number of candidate rows \\(k = 5, 4 candidates\\)$"):
        K.region_knn(ok, 5)
    empty = ok.copy()
    empty[2] = 0
    with pytest.raises(K.KmerSpansError, match="^row 2 has no counts$"):
        K.region_knn(empty, 9)  # the empty row before the too large k
    # the device wrapper refuses what is no CUDA tensor before it loads the library
    from kmer_spans_amd import device as D
    with pytest.raises(K.KmerSpansError, match="counts must be a contiguous int32"):
        D.region_knn(None, ok, 2)
    assert _lib.knn_k(np.int64(7)) == (7, 7) and _lib.knn_k(0) == (0, 1) and _lib.knn_k(900) == (900, 64)
    assert _lib.KnnStats().as_dict().keys() >= {"ms_total", "ms_normalise", "ms_select", "ms_merge", "n_splits",
                                                "tiles_per_split", "panel_bytes", "work_bytes"}
    hdr = open(HEADER).read()
    assert _lib.KS_KNN_MAX_K == R.MAX_K == 64 and "#define KS_KNN_MAX_K 64\n" in hdr
    assert C.sizeof(_lib.KnnStats) == 64
    assert "region_knn" in K.__all__ and {"ks_spectra_knn", "ks_spectra_knn_dev"} <= set(_lib.EXPORTS)
