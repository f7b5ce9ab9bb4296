"""Pairwise distances between region spectra (ks_spectra_dist /
ks_spectra_cross_dist, include/kmer_spans.h): the host reference the GPU tests
compare against bit for bit, the argument checks of the host entries, which
all happen before any device use, and the kernels' 64-bit index arithmetic
(csrc/ks_dist_index.h) walked on the host -- this file runs without a GPU."""
import ctypes as C

import numpy as np
import pytest

from kmer_spans_amd._lib import KS_DIST_MAX_NCOL, KS_DIST_SQUARED


# ------------------------------------------------------------ host reference

def profiles(counts) -> np.ndarray:
    """p[k] = (double)c[k] / (double)T, T the row sum in 64-bit integers; one
    IEEE division per element; NaN rows where T = 0."""
    c = np.asarray(counts).astype(np.uint64)
    t = c.sum(axis=1, dtype=np.uint64)
    assert int(t.max(initial=0)) < 2 ** 44
    with np.errstate(invalid="ignore", divide="ignore"):
        return c.astype(np.float64) / t.astype(np.float64)[:, None]


def ref_sq(p: np.ndarray, i, j) -> np.ndarray:
    """The contract's order of operations for the pairs (i[x], j[x]) of the
    profile matrix p: acc = 0; for k ascending: d = p_i[k] - p_j[k];
    acc = acc + d * d -- a Python loop over k, vectorised over the pairs (numpy
    rounds the subtraction, the product and the sum separately: no FMA)."""
    i, j = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)
    pt = np.ascontiguousarray(p.T)
    acc = np.zeros(i.size, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        for k in range(pt.shape[0]):
            d = pt[k][i] - pt[k][j]
            acc = acc + d * d
    return acc


def condensed_pairs(m: int):
    """(i, j) of every pair in the order of R's dist object / scipy's pdist."""
    i, j = np.triu_indices(m, 1)
    return i.astype(np.int64), j.astype(np.int64)


def ref_condensed_sq(counts, rows=None) -> np.ndarray:
    p = profiles(counts)
    if rows is not None:
        p = p[np.asarray(rows, dtype=np.int64)]
    return ref_sq(p, *condensed_pairs(p.shape[0]))


def ref_cross_sq(counts, rows_a, rows_b) -> np.ndarray:
    p = profiles(counts)
    a = np.arange(p.shape[0]) if rows_a is None else np.asarray(rows_a, dtype=np.int64)
    b = np.asarray(rows_b, dtype=np.int64)
    ii, jj = np.meshgrid(a, b, indexing="ij")
    return ref_sq(p, ii.ravel(), jj.ravel()).reshape(a.size, b.size)


def bits(x) -> np.ndarray:
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def random_counts(rng, m: int, ncol: int, hi: int = 1000) -> np.ndarray:
    c = rng.integers(0, hi, size=(m, ncol)).astype(np.uint32)
    c[rng.random((m, ncol)) < 0.3] = 0  # spectra of low-complexity regions are sparse
    c[:, 0] |= 1  # no empty row
    return c


def test_reference_known_answer():
    c = np.array([[1, 1, 0, 0], [0, 0, 2, 2], [3, 1, 0, 0], [5, 5, 0, 0]], dtype=np.uint32)
    want = {(0, 1): 1.0, (0, 2): 0.125, (0, 3): 0.0, (1, 2): 0.5625 + 0.0625 + 0.5, (1, 3): 1.0, (2, 3): 0.125}
    i, j = condensed_pairs(4)
    assert list(zip(i.tolist(), j.tolist())) == sorted(want)
    assert ref_condensed_sq(c).tolist() == [want[k] for k in sorted(want)]


@pytest.mark.parametrize("ncol", [4, 256, 4096])
def test_reference_properties(ncol):
    """The reference is scipy's pdist bit for bit, symmetric, 0 on the diagonal
    and exactly 0 between proportional rows; an empty row is NaN against all."""
    rng = np.random.default_rng(ncol)
    c = random_counts(rng, 24, ncol)
    c[5] = c[4] * 3
    c[6] = c[4] * 1000
    c[7] = 0
    p = profiles(c)
    i, j = condensed_pairs(24)
    sq = ref_sq(p, i, j)
    assert np.array_equal(bits(sq), bits(ref_sq(p, j, i)))
    assert not ref_sq(p, np.arange(7), np.arange(7)).any()
    at = {(a, b): x for a, b, x in zip(i.tolist(), j.tolist(), sq.tolist())}
    assert at[(4, 5)] == 0.0 and at[(4, 6)] == 0.0 and at[(5, 6)] == 0.0
    with_7 = np.array([x for (a, b), x in at.items() if 7 in (a, b)])
    assert with_7.size == 23 and np.isnan(with_7).all()
    assert not np.isnan(np.array([x for (a, b), x in at.items() if 7 not in (a, b)])).any()
    dist = pytest.importorskip("scipy.spatial.distance")
    keep = np.array([r for r in range(24) if r != 7])
    pk = p[keep]
    ii, jj = condensed_pairs(keep.size)
    assert np.array_equal(bits(np.sqrt(ref_sq(pk, ii, jj))), bits(dist.pdist(pk)))


# ------------------------------------------------- host entries: validation

def _dist(c, rows, m, ncol=None, n=None, flags=0, out=True, spectra=True):
    from kmer_spans_amd import _lib
    L = _lib.load()
    c = np.ascontiguousarray(c, dtype=np.uint32)
    n = c.shape[0] if n is None else n
    ncol = c.shape[1] if ncol is None else ncol
    r = np.ascontiguousarray(rows, dtype=np.int64) if rows is not None else None
    o = np.full(max(1, abs(m) * abs(m)), -7.0)
    rc = L.ks_spectra_dist(None, c.ctypes.data if spectra else None, n, ncol, r.ctypes.data if r is not None else None,
                           m, flags, o.ctypes.data if out else None)
    return rc, L.ks_last_error().decode(), o


def _cross(c, ra, na, rb, nb, ncol=None, n=None, flags=0, out=True, spectra=True):
    from kmer_spans_amd import _lib
    L = _lib.load()
    c = np.ascontiguousarray(c, dtype=np.uint32)
    n = c.shape[0] if n is None else n
    ncol = c.shape[1] if ncol is None else ncol
    a = np.ascontiguousarray(ra, dtype=np.int64) if ra is not None else None
    b = np.ascontiguousarray(rb, dtype=np.int64) if rb is not None else None
    o = np.full(max(1, abs(na) * abs(nb)), -7.0)
    rc = L.ks_spectra_cross_dist(None, c.ctypes.data if spectra else None, n, ncol,
                                 a.ctypes.data if a is not None else None, na,
                                 b.ctypes.data if b is not None else None, nb, flags, o.ctypes.data if out else None)
    return rc, L.ks_last_error().decode(), o


C8 = np.arange(1, 33, dtype=np.uint32).reshape(8, 4)


@pytest.mark.parametrize("kw,msg", [
    (dict(ncol=0), "ncol must be between 1 and 4096"),
    (dict(ncol=-4), "ncol must be between 1 and 4096"),
    (dict(ncol=KS_DIST_MAX_NCOL + 1), "ncol must be between 1 and 4096"),
    (dict(n=-1), "must not be negative"),
    (dict(m=-1), "must not be negative"),
    (dict(flags=KS_DIST_SQUARED << 1), "unknown distance flags"),
    (dict(spectra=False), "null spectra"),
    (dict(out=False), "null output"),
    (dict(rows=None, m=9), "exceeds n"),
    (dict(rows=[0, 1, 8, 2]), "row index 2 out of range"),
    (dict(rows=[-1, 1, 7, 2]), "row index 0 out of range"),
    (dict(rows=[0, 1, 7, 2 ** 40]), "row index 3 out of range"),
])
def test_condensed_host_entry_rejects_arguments_before_device(kw, msg):
    kw = dict(kw)
    rows = kw.pop("rows", [0, 1, 2, 3])
    m = kw.pop("m", 4)
    rc, err, o = _dist(C8, rows, m, **kw)
    assert rc == 1 and msg in err, (rc, err)
    assert (o == -7.0).all()


@pytest.mark.parametrize("kw,msg", [
    (dict(ncol=0), "ncol must be between 1 and 4096"),
    (dict(ncol=KS_DIST_MAX_NCOL + 1), "ncol must be between 1 and 4096"),
    (dict(n=-1), "must not be negative"),
    (dict(na=-1), "must not be negative"),
    (dict(nb=-2), "must not be negative"),
    (dict(flags=6), "unknown distance flags"),
    (dict(spectra=False), "null spectra"),
    (dict(out=False), "null output"),
    (dict(ra=None, na=9), "exceeds n"),
    (dict(rb=None, nb=9), "exceeds n"),
    (dict(ra=[0, 8]), "row index 1 out of range"),
    (dict(ra=[-5, 3]), "row index 0 out of range"),
    (dict(rb=[0, 1, 8]), "row index 2 of the second selection out of range"),
    (dict(rb=[0, -1, 7]), "row index 1 of the second selection out of range"),
])
def test_cross_host_entry_rejects_arguments_before_device(kw, msg):
    kw = dict(kw)
    ra, rb = kw.pop("ra", [0, 1]), kw.pop("rb", [2, 3, 4])
    na, nb = kw.pop("na", 2), kw.pop("nb", 3)
    rc, err, o = _cross(C8, ra, na, rb, nb, **kw)
    assert rc == 1 and msg in err, (rc, err)
    assert (o == -7.0).all()


def test_no_pair_is_ok():
    """m = 0 and m = 1 (na = 0 or nb = 0) write nothing and need no device; the
    other checks still come first."""
    from kmer_spans_amd import _lib
    L = _lib.load()
    for m, rows in ((0, None), (0, []), (1, None), (1, [7])):
        rc, err, o = _dist(C8, rows, m)
        assert rc == 0 and (o == -7.0).all(), (m, rows, err)
    assert _dist(C8, [8], 1)[0] == 1          # the index of a single row is still checked
    assert _dist(C8, None, 0, ncol=0)[0] == 1
    for na, nb in ((0, 0), (0, 3), (2, 0)):
        rc, err, o = _cross(C8, [0, 1][:na], na, [2, 3, 4][:nb], nb)
        assert rc == 0 and (o == -7.0).all(), (na, nb, err)
    assert _cross(C8, [9, 1], 2, [], 0)[0] == 1
    assert L.ks_spectra_dist(None, None, 0, 4, None, 0, 0, None) == 0
    assert L.ks_spectra_cross_dist(None, None, 0, 4, None, 0, None, 0, 0, None) == 0
    st = _lib.DistStats()
    st.n_pairs = 7
    assert L.ks_spectra_dist_dev(None, None, 0, 16, None, 0, 0, None, C.byref(st)) == 0
    assert st.n_pairs == 0
    st.n_pairs = 7
    assert L.ks_spectra_cross_dist_dev(None, None, 0, 16, None, 0, None, 0, 0, None, C.byref(st)) == 0
    assert st.n_pairs == 0
    assert L.ks_spectra_dist_dev(None, None, 0, 4097, None, 0, 0, None, None) == 1


def test_api_validates_before_device():
    import kmer_spans_amd as K
    assert "region_distances" in K.__all__
    assert K.region_distances(C8[:1]).shape == (0,)
    assert K.region_distances(C8, rows=[3]).shape == (0,)
    assert K.region_distances(C8, rows=[], rows_b=[1, 2]).shape == (0, 2)
    assert K.region_distances(C8, rows_b=[]).shape == (8, 0)
    with pytest.raises(K.KmerSpansError, match="^row index 1 out of range$"):
        K.region_distances(C8, rows=[0, 8])
    with pytest.raises(K.KmerSpansError, match="^row index 0 of the second selection out of range$"):
        K.region_distances(C8, rows_b=[-1])
    with pytest.raises(K.KmerSpansError, match="counts must be"):
        K.region_distances(np.zeros(4))
    with pytest.raises(K.KmerSpansError, match="counts must be"):
        K.region_distances(np.zeros((2, 4)))  # float64
    with pytest.raises(K.KmerSpansError, match="uint32 range"):
        K.region_distances(np.array([[1, -1], [2, 2]]), rows=[0, 1])
    with pytest.raises(K.KmerSpansError, match="integer row indices"):
        K.region_distances(C8, rows=[0.5, 1.0])
    with pytest.raises(K.KmerSpansError, match="ncol must be between 1 and 4096"):
        K.region_distances(np.zeros((3, 4097), dtype=np.uint32))


# ------------------------------------------------------- index arithmetic

def pair_offsets(i, j, m):
    from kmer_spans_amd import _lib
    i, j = np.ascontiguousarray(i, dtype=np.int64), np.ascontiguousarray(j, dtype=np.int64)
    off = np.full(i.size, -1, dtype=np.int64)
    _lib.load().ks_dist_pair_offsets(i.ctypes.data, j.ctypes.data, i.size, m, off.ctypes.data)
    return off


def tiles_of(t, tiles):
    from kmer_spans_amd import _lib
    t = np.ascontiguousarray(t, dtype=np.int64)
    row = np.full(t.size, -1, dtype=np.int64)
    col = np.full(t.size, -1, dtype=np.int64)
    _lib.load().ks_dist_tiles_of(t.ctypes.data, t.size, tiles, row.ctypes.data, col.ctypes.data)
    return row, col


def test_pair_offset_is_the_condensed_order():
    for m in range(1, 71):
        i, j = condensed_pairs(m)
        assert np.array_equal(pair_offsets(i, j, m), np.arange(m * (m - 1) // 2)), m


@pytest.mark.parametrize("m", [65_537, 3_000_000])
def test_pair_offset_beyond_int32(m):
    """First, last and seam pairs (the last pair of a row and the first of the
    next) against Python integers."""
    pairs = [(0, 1), (0, m - 1), (1, 2), (m - 2, m - 1), (m - 3, m - 2), (m - 3, m - 1)]
    for i in (1, 2, 255, 32_768, 32_769, m // 2, m // 2 + 1, m - 4):
        pairs += [(i - 1, m - 1), (i, i + 1), (i, m - 1)]
    want = [i * m - i * (i + 1) // 2 + (j - i - 1) for i, j in pairs]
    got = pair_offsets([p[0] for p in pairs], [p[1] for p in pairs], m)
    assert got.tolist() == want
    total = m * (m - 1) // 2
    assert want[3] == total - 1 and total > 2 ** 31
    for x in range(len(pairs)):  # a seam: the next row starts right after the last pair of a row
        if pairs[x][1] == m - 1 and pairs[x][0] + 2 < m:
            i = pairs[x][0]
            assert pair_offsets([i + 1], [i + 2], m)[0] == want[x] + 1


def test_tile_inverse_every_id():
    for T in range(1, 301):
        r, c = np.triu_indices(T)  # tiles on or above the diagonal, row-major: the linear order
        row, col = tiles_of(np.arange(r.size), T)
        assert np.array_equal(row, r) and np.array_equal(col, c), T


def test_tile_inverse_large_grid():
    """T = 2^20 (a 67-million-row list): the first and last id of every tile
    row and their neighbours, against integer arithmetic."""
    T = 1 << 20
    r = np.arange(T, dtype=np.int64)
    start = r * T - r * (r - 1) // 2  # < 2^40: exact in int64
    total = T * (T + 1) // 2
    assert int(start[-1]) == total - 1 and int(start[12345]) == 12345 * T - 12345 * 12344 // 2
    for delta in (0, 1, -1, 2, -2):
        t = start + delta
        ok = (t >= 0) & (t < total)
        t = t[ok]
        want_row = np.searchsorted(start, t, side="right") - 1
        row, col = tiles_of(t, T)
        assert np.array_equal(row, want_row), delta
        assert np.array_equal(col, want_row + (t - start[want_row])), delta
        assert (col < T).all() and (col >= row).all()


def test_tile_rows():
    from kmer_spans_amd import _lib
    assert _lib.load().ks_dist_tile_rows() == 64
