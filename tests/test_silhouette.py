"""Silhouette widths, medoids and diameters of a grouping (ks_silhouette /
ks_silhouette_dev, include/kmer_spans.h): the host reference the GPU tests
compare against bit for bit (a numpy transcription of the header's contract),
known answers worked by hand, an independent check against sklearn, the pin of
the chunked summation order, and the argument checks of both entries, which
all happen before any device use -- this file runs without a GPU."""
import os

import numpy as np
import pytest

from kmer_spans_amd import _lib
from tests.test_nj import bits, square0

CHUNK = _lib.KS_SIL_CHUNK  # the binding's copy of include/kmer_spans.h: the reference chunks as the library does
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kmer_spans.h")


# ------------------------------------------------------------ host reference

def _sum_in_order(x) -> np.ndarray:
    """Row sums of x [n, m], left to right in one accumulator started at +0.0
    (np.cumsum adds in order, np.sum does not; the zero column makes the start
    +0.0, which matters only for a row of -0.0)."""
    x = np.asarray(x, dtype=np.float64)
    return np.cumsum(np.concatenate([np.zeros((x.shape[0], 1)), x], axis=1), axis=1)[:, -1]


def chunked_sums(M, group, ngroups: int, chunk: int = CHUNK) -> np.ndarray:
    """S [n, ngroups] of the header: per group the members ascending, a partial
    per `chunk` consecutive members, the partials added in order.  chunk=None
    is the plain left-to-right sum over all members (the order the contract
    does NOT use)."""
    n = M.shape[0]
    S = np.zeros((n, ngroups))
    for c in range(1, ngroups + 1):
        mem = np.flatnonzero(group == c)
        if chunk is None:
            S[:, c - 1] = _sum_in_order(M[:, mem])
        else:
            parts = [_sum_in_order(M[:, mem[t:t + chunk]]) for t in range(0, mem.size, chunk)]
            S[:, c - 1] = _sum_in_order(np.stack(parts, axis=1)) if parts else 0.0
    return S


def ref_silhouette(d, n: int, group, ngroups=None):
    """The header's definitions, operation for operation."""
    d = np.asarray(d, dtype=np.float64)
    group = np.asarray(group, dtype=np.int64)
    g = int(group.max()) if ngroups is None else int(ngroups)
    assert d.shape == (n * (n - 1) // 2,) and n >= 2 and np.isfinite(d).all()
    assert group.shape == (n,) and group.min() >= 1 and group.max() <= g
    M = square0(d, n)
    S = chunked_sums(M, group, g)
    size = np.bincount(group, minlength=g + 1)[1:].astype(np.int32)
    assert (size > 0).sum() >= 2
    a, b, width = np.zeros(n), np.zeros(n), np.zeros(n)
    far = np.zeros(n)
    neighbor = np.zeros(n, dtype=np.int32)
    with np.errstate(all="ignore"):
        for i in range(n):
            o = int(group[i])
            for c in range(1, g + 1):
                if c == o or size[c - 1] == 0:
                    continue
                mean = S[i, c - 1] / np.float64(size[c - 1])
                if neighbor[i] == 0 or mean < b[i]:
                    b[i], neighbor[i] = mean, c
            if size[o - 1] > 1:
                a[i] = S[i, o - 1] / np.float64(size[o - 1] - 1)
                if a[i] < b[i]:
                    width[i] = (b[i] - a[i]) / b[i]
                elif a[i] > b[i]:
                    width[i] = (b[i] - a[i]) / a[i]
            for j in np.flatnonzero(group == o):
                if M[i, j] > far[i]:
                    far[i] = M[i, j]
    medoid = np.full(g, -1, dtype=np.int32)
    diameter = np.full(g, np.nan)
    avg_width = np.full(g, np.nan)
    for c in range(1, g + 1):
        mem = np.flatnonzero(group == c)
        if mem.size == 0:
            continue
        best, diam = mem[0], 0.0
        for i in mem:
            if S[i, c - 1] < S[best, c - 1]:
                best = i
            if far[i] > diam:
                diam = far[i]
        medoid[c - 1], diameter[c - 1] = best, diam
        avg_width[c - 1] = _sum_in_order(width[mem][None, :])[0] / np.float64(mem.size)
    return {"width": width, "a": a, "b": b, "neighbor": neighbor, "size": size, "medoid": medoid,
            "diameter": diameter, "avg_width": avg_width,
            "avg_width_all": float(_sum_in_order(width[None, :])[0] / np.float64(n)), "sums": S, "far": far}


FLOAT_KEYS = ("width", "a", "b", "diameter", "avg_width")
INT_KEYS = ("neighbor", "size", "medoid")


def assert_same_silhouette(got, want, what="", sums=True):
    """Every output bit for bit (NaN included: the bits are compared)."""
    for k in INT_KEYS:
        assert np.array_equal(np.asarray(got[k]), want[k]), (what, k, np.asarray(got[k])[:8], want[k][:8])
    for k in FLOAT_KEYS:
        x, y = bits(got[k]), bits(want[k])
        if k in ("diameter", "avg_width"):  # any NaN for an empty group
            empty = want["size"] == 0
            assert np.isnan(np.asarray(got[k])[empty]).all(), (what, k)
            x, y = x[~empty], y[~empty]
        assert np.array_equal(x, y), (what, k, int((x != y).sum()))
    assert bits([got["avg_width_all"]])[0] == bits([want["avg_width_all"]])[0], (what, "avg_width_all")
    if sums:
        assert np.array_equal(bits(got["sums"]), bits(want["sums"])), (what, "sums")


def ties_in(ref, group):
    """(rows whose b is reached by two or more groups, groups whose smallest
    S(i, c) is reached by two or more members) of a reference result."""
    group = np.asarray(group)
    S, size = ref["sums"], ref["size"]
    g = size.size
    with np.errstate(all="ignore"):
        mean = S / np.where(size > 0, size, 1).astype(np.float64)[None, :]
    other = (np.arange(1, g + 1)[None, :] != group[:, None]) & (size > 0)[None, :]
    b_ties = int(((np.where(other, mean, np.inf) == ref["b"][:, None]).sum(axis=1) >= 2).sum())
    med_ties = 0
    for c in range(1, g + 1):
        mem = np.flatnonzero(group == c)
        if mem.size:
            med_ties += int((S[mem, c - 1] == S[mem, c - 1].min()).sum() >= 2)
    return b_ties, med_ties


def line_dist(x) -> np.ndarray:
    x = np.asarray(x, dtype=np.float64)
    i, j = np.triu_indices(x.size, 1)
    return np.abs(x[i] - x[j])


def order_pin_case():
    """n = 700 with a group of 600 members (three chunks) and one of 100;
    distances a random mantissa times 2^k, k in -30 .. 30, so that where a sum
    is rounded depends on where it is cut."""
    n = 700
    rng = np.random.default_rng(20240)
    m = n * (n - 1) // 2
    d = np.ldexp(1.0 + rng.random(m), rng.integers(-30, 31, size=m))
    group = np.ones(n, dtype=np.int32)
    group[rng.permutation(n)[:100]] = 2
    return d, n, group, 2


# ------------------------------------------------------------- known answers

def test_line_two_groups():
    """Points 0 1 3 | 10 12 on a line, groups 1 1 1 2 2.
    S(i, 1) = 4 3 5 26 32, S(i, 2) = 22 20 16 2 2.
    a = 4/2 3/2 5/2 | 2/1 2/1;  b = 22/2 20/2 16/2 | 26/3 32/3.
    width = (b - a) / b everywhere: 9/11, 8.5/10, 5.5/8, (26/3 - 2)/(26/3),
    (32/3 - 2)/(32/3).  Medoids: the smallest own sum, 3 at point 1; 2 = 2 at
    points 3 and 4, the lower index wins.  Diameters 3 and 2."""
    r = ref_silhouette(line_dist([0, 1, 3, 10, 12]), 5, [1, 1, 1, 2, 2])
    assert r["sums"].tolist() == [[4, 22], [3, 20], [5, 16], [26, 2], [32, 2]]
    assert r["a"].tolist() == [2.0, 1.5, 2.5, 2.0, 2.0]
    assert r["b"].tolist() == [11.0, 10.0, 8.0, 26.0 / 3.0, 32.0 / 3.0]
    assert r["width"].tolist() == [9.0 / 11.0, 8.5 / 10.0, 5.5 / 8.0, (26.0 / 3.0 - 2.0) / (26.0 / 3.0),
                                   (32.0 / 3.0 - 2.0) / (32.0 / 3.0)]
    assert r["neighbor"].tolist() == [2, 2, 2, 1, 1]
    assert r["size"].tolist() == [3, 2] and r["medoid"].tolist() == [1, 3] and r["diameter"].tolist() == [3.0, 2.0]
    w = r["width"]
    assert r["avg_width"].tolist() == [((w[0] + w[1]) + w[2]) / 3.0, (w[3] + w[4]) / 2.0]
    assert r["avg_width_all"] == ((((w[0] + w[1]) + w[2]) + w[3]) + w[4]) / 5.0


def test_line_three_groups():
    """Points 0 1 | 5 6 | 20, groups 1 1 2 2 3.  a = 1 1 1 1 and 0 for the
    singleton.  Means to the other groups: point 0: 5.5 (2), 20 (3); point 1:
    4.5, 19; point 5: 4.5 (1), 15 (3); point 6: 5.5 (1), 14 (3); point 20: 19.5
    (1), 14.5 (2).  width = 4.5/5.5 3.5/4.5 3.5/4.5 4.5/5.5 and 0 for the
    singleton.  Medoids 0, 2 (ties, the lower index) and 4; diameters 1 1 0."""
    r = ref_silhouette(line_dist([0, 1, 5, 6, 20]), 5, [1, 1, 2, 2, 3])
    assert r["a"].tolist() == [1.0, 1.0, 1.0, 1.0, 0.0]
    assert r["b"].tolist() == [5.5, 4.5, 4.5, 5.5, 14.5]
    assert r["neighbor"].tolist() == [2, 2, 1, 1, 2]
    assert r["width"].tolist() == [4.5 / 5.5, 3.5 / 4.5, 3.5 / 4.5, 4.5 / 5.5, 0.0]
    assert r["size"].tolist() == [2, 2, 1] and r["medoid"].tolist() == [0, 2, 4]
    assert r["diameter"].tolist() == [1.0, 1.0, 0.0] and r["avg_width"][2] == 0.0
    assert ties_in(r, [1, 1, 2, 2, 3]) == (0, 2)


def test_all_singletons():
    """Every observation its own group: every width is 0, S(i, c) is D(i, c - 1),
    b is the row's smallest entry and neighbor the lowest index that has it."""
    n = 40
    rng = np.random.default_rng(40)
    d = rng.integers(1, 6, size=n * (n - 1) // 2).astype(np.float64)
    r = ref_silhouette(d, n, np.arange(1, n + 1))
    M = square0(d, n)
    assert np.array_equal(bits(r["sums"]), bits(M))
    assert not r["width"].any() and not r["a"].any() and not r["diameter"].any() and not r["avg_width"].any()
    assert r["avg_width_all"] == 0.0 and r["medoid"].tolist() == list(range(n)) and (r["size"] == 1).all()
    off = M + np.diag(np.full(n, np.inf))
    assert np.array_equal(r["b"], off.min(axis=1)) and np.array_equal(r["neighbor"], off.argmin(axis=1) + 1)


def test_equal_a_and_b_is_zero():
    """Four points at equal distances in two groups: a == b, width 0 by definition."""
    r = ref_silhouette(np.full(6, 0.75), 4, [1, 2, 1, 2])
    assert not r["width"].any() and r["a"].tolist() == r["b"].tolist() == [0.75] * 4
    assert r["neighbor"].tolist() == [2, 1, 2, 1] and r["medoid"].tolist() == [0, 1]


# -------------------------------------------------------- empty groups, ngroups

def test_ngroups_above_the_largest_label_and_empty_groups_in_the_middle():
    n = 90
    rng = np.random.default_rng(9)
    d = rng.random(n * (n - 1) // 2)
    dense = rng.integers(1, 4, size=n)             # labels 1 2 3
    sparse = np.array([0, 2, 5, 6])[dense]          # the same groups as 2 5 6 of 9
    r3, r9 = ref_silhouette(d, n, dense), ref_silhouette(d, n, sparse, ngroups=9)
    keep = [1, 4, 5]
    for k in ("width", "a", "b"):
        assert np.array_equal(bits(r3[k]), bits(r9[k])), k
    assert np.array_equal(np.array([0, 2, 5, 6])[r3["neighbor"]], r9["neighbor"])
    for k in ("size", "medoid", "diameter", "avg_width"):
        assert np.array_equal(r3[k], r9[k][keep]), k
    empty = np.setdiff1d(np.arange(9), keep)
    assert not r9["size"][empty].any() and (r9["medoid"][empty] == -1).all()
    assert np.isnan(r9["diameter"][empty]).all() and np.isnan(r9["avg_width"][empty]).all()
    assert not r9["sums"][:, empty].any() and not np.signbit(r9["sums"][:, empty]).any()
    assert np.array_equal(bits(r3["sums"]), bits(r9["sums"][:, keep]))


# ---------------------------------------------------------- against sklearn

@pytest.mark.parametrize("n,g", [(50, 2), (300, 7), (700, 2)])
def test_against_sklearn(n, g):
    """sklearn sums in another order: each mean carries at most n 2^-53
    relative error either way, and a width (at most 1 in magnitude) moves by at
    most twice the sum of the two: 8 n 2^-53 absolute covers it."""
    metrics = pytest.importorskip("sklearn.metrics")
    rng = np.random.default_rng(n)
    d = rng.random(n * (n - 1) // 2) + 0.01  # non-negative, tie-free
    assert np.unique(d).size == d.size
    group = rng.integers(1, g + 1, size=n)
    group[:g] = np.arange(1, g + 1)
    r = ref_silhouette(d, n, group)
    want = metrics.silhouette_samples(square0(d, n), group, metric="precomputed")
    err = np.abs(r["width"] - want).max()
    print(f"n = {n} g = {g}: max |width - sklearn| = {err:.3e}, bound {8 * n * 2.0 ** -53:.3e}")
    assert err <= 8 * n * 2.0 ** -53


# ----------------------------------------------------------------- order pin

def test_order_pin_chunked_sums_differ_from_left_to_right():
    """The contract's sums are chunked; on this input that is visible in the
    bits, so a kernel that adds in another order fails the GPU test on it."""
    d, n, group, g = order_pin_case()
    assert np.bincount(group)[1] > 2 * CHUNK
    M = square0(d, n)
    chunked, plain = chunked_sums(M, group, g), chunked_sums(M, group, g, chunk=None)
    differ = bits(chunked) != bits(plain)
    print(f"{int(differ[:, 0].sum())} of {n} sums over the large group differ in bits")
    assert differ[:, 0].any()
    assert not differ[:, 1].any()  # 100 members: one chunk, the same order
    assert np.array_equal(bits(ref_silhouette(d, n, group)["sums"]), bits(chunked))
    rel = np.abs(chunked - plain) / plain
    assert rel.max() < n * 2.0 ** -53


def test_tie_heavy_inputs_have_ties():
    """What the GPU test relies on: both kinds of tie occur in its inputs."""
    for n in (130, 600):
        d, group, g = tie_heavy_case(n)
        b_ties, med_ties = ties_in(ref_silhouette(d, n, group, g), group)
        print(f"n = {n}: {b_ties} rows with a tie in b, {med_ties} groups with a tie in the medoid")
        assert b_ties > 0 and med_ties > 0


def tie_heavy_case(n: int):
    """Distances from {0, 1, 2, 3}, groups of five members interleaved: equal
    sizes, small integer sums, so equal means and equal medoid sums abound."""
    rng = np.random.default_rng(n)
    d = rng.integers(0, 4, size=n * (n - 1) // 2).astype(np.float64)
    g = n // 5
    return d, (np.arange(n) % g + 1).astype(np.int32), g


# ------------------------------------------------------------ argument checks

def _sil(n, group=None, ngroups=2, flags=0, dev=False, d=None, diss=True, has_group=True, outs=(True,) * 9):
    """A call that must be refused before any device use: this machine has no GPU."""
    from kmer_spans_amd import _lib
    L = _lib.load()
    m = max(abs(n), 2)
    d = np.ones(m * (m - 1) // 2) if d is None else np.ascontiguousarray(d, dtype=np.float64)
    group = np.arange(m) % 2 + 1 if group is None else group
    group = np.ascontiguousarray(group, dtype=np.int32)
    res = _lib.silhouette_outputs(m, max(ngroups, 1))
    ptr = [p if keep else None for p, keep in zip(_lib.silhouette_out_args(res), outs)]
    dp = d.ctypes.data if diss else None
    gp = group.ctypes.data if has_group else None
    if dev:  # the pointer is never followed: the arguments fail first
        rc = L.ks_silhouette_dev(None, dp, n, gp, ngroups, flags, *ptr, None, None)
    else:
        rc = L.ks_silhouette(None, dp, n, gp, ngroups, flags, *ptr, None)
    return rc, L.ks_last_error().decode()


@pytest.mark.parametrize("dev", [False, True])
def test_entries_validate_before_any_device_call(dev):
    for n in (1, 0, -3):
        rc, msg = _sil(n, dev=dev)
        assert rc != 0 and "at least 2 observations" in msg
    rc, msg = _sil(5, dev=dev, diss=False)
    assert rc != 0 and "null dissimilarities" in msg
    rc, msg = _sil(5, dev=dev, has_group=False)
    assert rc != 0 and "null group" in msg
    for k in range(9):
        rc, msg = _sil(5, dev=dev, outs=tuple(x != k for x in range(9)))
        assert rc != 0 and "null output" in msg, k
    for flags in (1, 2, 8, -1):
        rc, msg = _sil(5, flags=flags, dev=dev)
        assert rc != 0 and "unknown silhouette flags" in msg
    rc, msg = _sil(5, ngroups=0, dev=dev)
    assert rc != 0 and "ngroups = 0" in msg


@pytest.mark.parametrize("dev", [False, True])
def test_bad_label_names_the_first_index(dev):
    for group, g, i, v in (([1, 2, 3, 1, 4], 3, 4, 4), ([1, 0, 2, 0, 1], 2, 1, 0), ([2, 1, -7, 9, 1], 2, 2, -7),
                           ([3, 1, 2, 1, 1], 2, 0, 3)):
        rc, msg = _sil(5, group=group, ngroups=g, dev=dev)
        assert rc != 0 and msg == f"group[{i}] = {v} is not in 1 .. {g}", msg


@pytest.mark.parametrize("dev", [False, True])
def test_one_non_empty_group(dev):
    for group, g in (([1] * 5, 1), ([1] * 5, 4), ([3] * 5, 4)):
        rc, msg = _sil(5, group=group, ngroups=g, dev=dev)
        assert rc != 0 and "at least 2 non-empty groups" in msg, msg


@pytest.mark.parametrize("badval", [np.nan, np.inf, -np.inf])
def test_host_entry_rejects_non_finite(badval):
    """ks_silhouette checks every entry on the host before any device call."""
    import kmer_spans_amd as K
    d = np.ones(10)
    d[[4, 7]] = badval
    rc, msg = _sil(5, d=d)
    assert rc != 0 and msg == "dissimilarity at offset 4 is not finite"
    with pytest.raises(K.KmerSpansError, match="^dissimilarity at offset 4 is not finite$"):
        K.region_silhouette(d, [1, 2, 1, 2, 1])


def test_python_argument_checks():
    import kmer_spans_amd as K
    from kmer_spans_amd import _lib
    for size in (0, 2, 4, 5, 7):
        with pytest.raises(K.KmerSpansError, match="n\\(n-1\\)/2"):
            K.region_silhouette(np.ones(size), [1, 2])
    with pytest.raises(K.KmerSpansError, match="1-d"):
        K.region_silhouette(np.ones((3, 1)), [1, 2, 1])
    for bad in ([1, 2], [1, 2, 1, 2], [[1, 2, 1]], [1.0, 2.0, 1.0], [1, 2, 2 ** 40]):
        with pytest.raises(K.KmerSpansError, match="group"):
            K.region_silhouette(np.ones(3), bad)
    for bad in (0, -1, 2.5, 2 ** 31):
        with pytest.raises(K.KmerSpansError, match="ngroups"):
            K.region_silhouette(np.ones(3), [1, 2, 1], ngroups=bad)
    with pytest.raises(K.KmerSpansError, match="^group\\[1\\] = 2 is not in 1 .. 1$"):
        K.region_silhouette(np.ones(3), [1, 2, 1], ngroups=1)
    with pytest.raises(K.KmerSpansError, match="at least 2 non-empty groups"):
        K.region_silhouette(np.ones(3), [2, 2, 2])
    g, ng = _lib.silhouette_group(np.array([1, 5, 2], dtype=np.int64), 3)
    assert g.dtype == np.int32 and ng == 5
    assert _lib.silhouette_group([1, 5, 2], 3, ngroups=8)[1] == 8
    assert _lib.SilhouetteStats().as_dict().keys() >= {"ms_check", "ms_sums", "ms_widths", "n_chunks", "work_bytes"}
    assert _lib.KS_SIL_CHUNK == 256 and "#define KS_SIL_CHUNK 256\n" in open(HEADER).read()
    assert "region_silhouette" in K.__all__
