"""The metric field of the distance flags (KS_DIST_METRIC_MASK: manhattan,
maximum, canberra, hellinger beside euclidean; include/kmer_spans.h): the host
model of tests/metricref.py against scipy and against answers worked by hand,
the model's properties, and the flag checks of the C entries and the Python
wrappers, which all happen before any device use -- this file runs without a
GPU."""
import ctypes as C

import numpy as np
import pytest

from kmer_spans_amd import _lib
from tests import metricref as M
from tests.test_knn import _knn
from tests.test_spectra_dist import C8, _cross, _dist, bits, condensed_pairs, profiles, random_counts

FLAG = {"euclidean": 0x000, "manhattan": 0x100, "maximum": 0x200, "canberra": 0x300, "hellinger": 0x400}
NO_SQUARED = ("manhattan", "maximum", "canberra")
FLAG_MESSAGES = ("unknown distance flags", "unknown flags", "unknown distance metric", "needs euclidean or hellinger")


def ulps(got, want) -> np.ndarray:
    """The distance in units of the last place between non-negative doubles."""
    return np.abs(bits(got).astype(np.int64) - bits(want).astype(np.int64))


# ------------------------------------------------------------- known answers

KNOWN = np.array([[1, 1, 0, 0], [0, 0, 2, 2], [3, 1, 0, 0], [5, 5, 0, 0]], dtype=np.uint32)
# profiles (.5 .5 0 0), (0 0 .5 .5), (.75 .25 0 0), (.5 .5 0 0); pairs 01 02 03 12 13 23


def value(metric, counts):
    return M.condensed_value(metric, counts)


def test_known_answers_euclidean_manhattan_maximum():
    assert value("euclidean", KNOWN).tolist() == [1.0, 0.125, 0.0, 1.125, 1.0, 0.125]
    assert value("manhattan", KNOWN).tolist() == [2.0, 0.5, 0.0, 2.0, 2.0, 0.5]
    assert value("maximum", KNOWN).tolist() == [0.5, 0.25, 0.0, 0.75, 0.5, 0.25]
    # the maximum is not in the last column, and a later smaller t does not replace it
    c = np.array([[1, 6, 1, 0], [4, 1, 2, 1]], dtype=np.uint32)  # p = (1 6 1 0) / 8, (4 1 2 1) / 8
    assert value("maximum", c).tolist() == [0.625] and value("manhattan", c).tolist() == [0.375 + 0.625 + 0.125 + 0.125]


def test_known_answers_canberra():
    c = np.array([[2, 0, 0, 0], [7, 0, 0, 0], [1, 1, 1, 1], [1, 3, 0, 0]], dtype=np.uint32)
    # profiles (1 0 0 0), (1 0 0 0), (.25 .25 .25 .25), (.25 .75 0 0)
    p = profiles(c)
    i, j = condensed_pairs(4)
    assert M.canberra_count(p, i, j).tolist() == [1, 4, 2, 4, 2, 4]
    one_all = 0.75 / 1.25 + 1.0 + 1.0 + 1.0   # (1 0 0 0) against (.25 x 4): cnt == ncol, no scaling
    one_two = (0.75 / 1.25 + 0.75 / 0.75) / (2.0 / 4.0)  # against (.25 .75 0 0): columns 2, 3 omitted, cnt = 2
    all_two = 0.0 / 0.5 + 0.5 / 1.0 + 1.0 + 1.0  # (.25 x 4) against (.25 .75 0 0): cnt == ncol
    # pair (0, 1): the single common non-zero column, |1 - 1| / 2 = 0, scaled by 4 / 1
    assert value("canberra", c).tolist() == [0.0, one_all, one_two, one_all, one_two, all_two]
    assert one_two == 3.2 and all_two == 2.5
    # the first matrix: disjoint supports keep every column at 1; rows 0 and 2 share two columns
    two = (0.25 / 1.25 + 0.25 / 0.75) / (2.0 / 4.0)
    assert value("canberra", KNOWN).tolist() == [4.0, two, 0.0, 4.0, 4.0, two]
    assert M.canberra_count(profiles(KNOWN), i, j).tolist() == [4, 2, 2, 4, 4, 2]


def test_known_answers_hellinger():
    c = np.array([[1, 1, 1, 1], [4, 0, 0, 0], [0, 0, 9, 0], [3, 3, 3, 3]], dtype=np.uint32)
    # roots (.5 .5 .5 .5), (1 0 0 0), (0 0 1 0), (.5 .5 .5 .5): every root is exact
    v = value("hellinger", c)
    assert v.tolist() == [1.0, 1.0, 0.0, 2.0, 1.0, 1.0]
    assert M.result("hellinger", v, squared=True).tolist() == [0.5, 0.5, 0.0, 1.0, 0.5, 0.5]
    assert M.result("hellinger", v).tolist() == [np.sqrt(0.5), np.sqrt(0.5), 0.0, 1.0, np.sqrt(0.5), np.sqrt(0.5)]
    assert M.result("euclidean", value("euclidean", KNOWN)).tolist() == [1.0, np.sqrt(0.125), 0.0, np.sqrt(1.125),
                                                                           1.0, np.sqrt(0.125)]
    assert M.result("manhattan", value("manhattan", KNOWN)).tolist() == [2.0, 0.5, 0.0, 2.0, 2.0, 0.5]


# ---------------------------------------------------------- model properties

def property_case(ncol):
    c = random_counts(np.random.default_rng(ncol), 24, ncol)
    c[5] = c[4] * 3
    c[6] = c[4] * 1000
    c[7] = 0
    return c


@pytest.mark.parametrize("ncol", [1, 4, 17, 256])
@pytest.mark.parametrize("metric", M.METRICS)
def test_model_properties(metric, ncol):
    """Symmetric in the bits, 0 on the diagonal and between proportional rows,
    NaN against an empty row and nowhere else, never negative."""
    p = profiles(property_case(ncol))
    i, j = condensed_pairs(24)
    v = M.VALUE[metric](p, i, j)
    back = M.VALUE[metric](p, j, i)
    nan = (i == 7) | (j == 7)
    assert np.array_equal(np.isnan(v), nan) and np.array_equal(np.isnan(back), nan)
    assert np.array_equal(bits(v[~nan]), bits(back[~nan]))
    rows = np.array([r for r in range(24) if r != 7])
    assert not bits(M.VALUE[metric](p, rows, rows)).any()  # +0.0, not -0.0
    assert np.isnan(M.VALUE[metric](p, [7], [7])).all()
    at = {(a, b): x for a, b, x in zip(i.tolist(), j.tolist(), v.tolist())}
    assert at[(4, 5)] == 0.0 and at[(4, 6)] == 0.0 and at[(5, 6)] == 0.0
    assert (v[~nan] >= 0).all() and not np.signbit(v[~nan]).any()


def test_hellinger_is_bounded_and_exact_at_its_ends():
    c = np.array([[1, 0, 0, 0], [0, 0, 7, 0], [4, 4, 4, 4], [0, 0, 0, 5], [1, 0, 0, 0]], dtype=np.uint32)
    c = np.vstack([c, c[2:3] * 3, c[2:3] * 1000])
    p = profiles(c)
    one = M.result("hellinger", M.hellinger(p, [0, 0, 1, 3], [1, 3, 3, 4]))
    assert one.tolist() == [1.0, 1.0, 1.0, 1.0]  # disjoint support
    zero = M.hellinger(p, [2, 2, 5, 0], [5, 6, 6, 4])
    assert not bits(zero).any()  # proportional rows: x 3, x 1000, and a copy
    r = profiles(random_counts(np.random.default_rng(3), 40, 33))
    d = M.result("hellinger", M.hellinger(r, *condensed_pairs(40)))
    assert (d >= 0).all() and (d <= 1.0).all()


# ------------------------------------------------------ model against scipy

@pytest.mark.parametrize("ncol", [1, 4, 17, 256])
def test_model_against_scipy(ncol):
    """cityblock and chebyshev run the header's order of operations (one
    accumulator, k ascending): bit for bit.  canberra: scipy omits the columns
    where both are 0 but does not rescale, so it is multiplied by ncol / cnt;
    that and the Hellinger form through pdist round differently: within 2 ulp
    per column."""
    dist = pytest.importorskip("scipy.spatial.distance")
    p = profiles(random_counts(np.random.default_rng(100 + ncol), 30, ncol))
    i, j = condensed_pairs(30)
    assert np.array_equal(bits(M.manhattan(p, i, j)), bits(dist.pdist(p, "cityblock")))
    assert np.array_equal(bits(M.maximum(p, i, j)), bits(dist.pdist(p, "chebyshev")))
    assert np.array_equal(bits(np.sqrt(M.euclidean(p, i, j))), bits(dist.pdist(p)))
    cnt = M.canberra_count(p, i, j)
    assert cnt.min() >= 1
    assert ulps(M.canberra(p, i, j), dist.pdist(p, "canberra") * (ncol / cnt)).max() <= 2 * ncol
    h = M.result("hellinger", M.hellinger(p, i, j))
    assert ulps(h, dist.pdist(np.sqrt(p)) * np.sqrt(0.5)).max() <= 2 * ncol


# -------------------------------------------- C entries: the checks of flags

def _dist_dev(cross, flags, m=4, ncol=4, out=None):
    """ks_spectra_dist_dev / ks_spectra_cross_dist_dev with pointers that are
    never followed: the call ends at an argument check or has no pair."""
    L = _lib.load()
    sp = np.ones((8, 4), dtype=np.uint32)
    out = np.full(64, -7.0) if out is None else out
    st = _lib.DistStats()
    if cross:
        rc = L.ks_spectra_cross_dist_dev(None, sp.ctypes.data, 8, ncol, None, m, None, m, flags, out.ctypes.data,
                                         C.byref(st))
    else:
        rc = L.ks_spectra_dist_dev(None, sp.ctypes.data, 8, ncol, None, m, flags, out.ctypes.data, C.byref(st))
    assert (out == -7.0).all(), "an output was written"
    return rc, L.ks_last_error().decode()


def dist_calls(flags):
    """(name, rc, message) of the four distance entries refusing `flags`; the
    helpers assert that the sentinels of the output are untouched."""
    def host(r):
        rc, msg, o = r
        assert (o == -7.0).all(), "an output was written"
        return rc, msg
    return [("dist", *host(_dist(C8, [0, 1, 2, 3], 4, flags=flags))),
            ("cross", *host(_cross(C8, [0, 1], 2, [2, 3, 4], 3, flags=flags))),
            ("dist_dev", *_dist_dev(False, flags)), ("cross_dev", *_dist_dev(True, flags))]


@pytest.mark.parametrize("metric", M.METRICS)
def test_every_metric_passes_the_flag_checks(metric):
    """A call that is valid up to its flags ends without a pair (rc 0) or at
    the next check in the order, "null spectra": neither needs a device."""
    for sq in (0, 1):
        if sq and metric in NO_SQUARED:
            continue
        flags = FLAG[metric] | sq
        assert _lib.DIST_METRICS[metric] == FLAG[metric]
        rc, msg, o = _dist(C8, None, 1, flags=flags)  # a single row: no pair
        assert rc == 0 and (o == -7.0).all(), msg
        rc, msg, o = _cross(C8, [0, 1], 2, [], 0, flags=flags)
        assert rc == 0 and (o == -7.0).all(), msg
        assert _dist_dev(False, flags, m=0)[0] == 0 and _dist_dev(True, flags, m=0)[0] == 0
        for rc, msg in (_dist(C8, [0, 1, 2, 3], 4, flags=flags, spectra=False)[:2],
                        _cross(C8, [0, 1], 2, [2, 3, 4], 3, flags=flags, spectra=False)[:2],
                        _knn(False, flags=flags, null=("sp",)), _knn(True, flags=flags, null=("sp",))):
            assert rc != 0 and msg == "null spectra" and not any(t in msg for t in FLAG_MESSAGES), msg


@pytest.mark.parametrize("field", [5, 15])
def test_unknown_metric_field(field):
    for sq in (0, 1):
        flags = (field << 8) | sq
        for name, rc, msg in dist_calls(flags):
            assert rc == 1 and msg == f"unknown distance metric {field}", (name, msg)
        for dev in (False, True):
            rc, msg = _knn(dev, flags=flags)
            assert rc != 0 and msg == f"unknown distance metric {field}", msg


@pytest.mark.parametrize("metric", NO_SQUARED)
def test_squared_needs_euclidean_or_hellinger(metric):
    flags = FLAG[metric] | _lib.KS_DIST_SQUARED
    calls = dist_calls(flags) + [("knn", *_knn(False, flags=flags)), ("knn_dev", *_knn(True, flags=flags))]
    for name, rc, msg in calls:
        assert rc != 0 and metric in msg and "needs euclidean or hellinger" in msg, (name, msg)


def test_unknown_bits_keep_their_messages():
    for flags in (2, 6, -1, 0x1000, 0x100 | 2, 0x500 | 0x80):
        for name, rc, msg in dist_calls(flags):
            assert rc == 1 and msg == f"unknown distance flags 0x{flags & 0xffffffff:x}", (name, msg)
        for dev in (False, True):
            rc, msg = _knn(dev, flags=flags)
            assert rc != 0 and msg == f"unknown flags 0x{flags & 0xffffffff:x} for a nearest-neighbour call", msg


def test_the_flag_checks_keep_their_place_in_the_order():
    """ncol first, then unknown bits, the metric field, the squared form; then
    the rest (n, the selections)."""
    assert "ncol must be" in _dist(C8, [0, 1], 2, ncol=0, flags=0x500)[1]
    assert "unknown distance flags" in _dist(C8, [0, 1], 2, n=-1, flags=0x502)[1]
    assert "unknown distance metric 5" in _dist(C8, [0, 1], 2, n=-1, flags=0x501)[1]
    assert "needs euclidean or hellinger" in _dist(C8, [0, 1], 2, n=-1, flags=0x101)[1]
    assert "must not be negative" in _dist(C8, [0, 1], 2, n=-1, flags=0x100)[1]
    assert "k must be between" in _knn(False, k=0, flags=0x500)[1]
    assert "unknown distance metric 5" in _knn(False, n=3, flags=0x500)[1]
    assert "needs euclidean or hellinger" in _knn(True, n=3, flags=0x301)[1]
    assert "exceeds n = 3" in _knn(True, n=3, flags=0x300)[1]


# ------------------------------------------------------------ Python wrappers

def test_dist_flags_helper():
    assert set(_lib.DIST_METRICS) == set(M.METRICS) == set(FLAG)
    for metric in M.METRICS:
        assert _lib.dist_flags(metric, False) == FLAG[metric]
        if metric in M.HAS_SQUARED:
            assert _lib.dist_flags(metric, True) == FLAG[metric] | 1
    with pytest.raises(_lib.KmerSpansError, match="metric must be one of .*'canberra', 'euclidean', 'hellinger', "
                                                  "'manhattan', 'maximum'.*not 'minkowski'"):
        _lib.dist_flags("minkowski", False)
    with pytest.raises(_lib.KmerSpansError, match="metric must be one of"):
        _lib.dist_flags(None, False)
    for metric in NO_SQUARED:
        with pytest.raises(_lib.KmerSpansError, match=f"squared=True has no meaning for metric='{metric}'"):
            _lib.dist_flags(metric, True)


def test_wrappers_refuse_before_the_library_is_called(monkeypatch):
    import kmer_spans_amd as K
    from kmer_spans_amd import api

    def no_library():
        raise AssertionError("the library was called")
    monkeypatch.setattr(api, "load", no_library)
    for call in (lambda **kw: K.region_distances(C8, **kw), lambda **kw: K.region_distances(C8, rows_b=[1, 2], **kw),
                 lambda **kw: K.region_knn(C8, 2, **kw)):
        with pytest.raises(K.KmerSpansError, match="metric must be one of"):
            call(metric="cityblock")
        with pytest.raises(K.KmerSpansError, match="squared=True has no meaning for metric='manhattan'"):
            call(metric="manhattan", squared=True)
    # the wrappers' own checks still come first
    with pytest.raises(K.KmerSpansError, match="counts must be"):
        K.region_distances(np.zeros(4), metric="cityblock")
    with pytest.raises(K.KmerSpansError, match="integer row indices"):
        K.region_distances(C8, rows=[0.5], metric="cityblock")
    with pytest.raises(K.KmerSpansError, match="k must be an integer"):
        K.region_knn(C8, 2.5, metric="cityblock")


def test_wrappers_without_a_pair_take_every_metric():
    import kmer_spans_amd as K
    for metric in M.METRICS:
        assert K.region_distances(C8, rows=[3], metric=metric).shape == (0,)
        assert K.region_distances(C8, rows_b=[], metric=metric).shape == (8, 0)
