"""Lloyd k-means and group means of region spectra (ks_spectra_kmeans /
ks_spectra_group_means, include/kmer_spans.h): the host model of
tests/kmeansref.py against known answers worked by hand, against the plain
nested loops of the header, against an independent Lloyd in numpy, the pin of
the chunked summation order, the tie and edge cases, and the argument checks of
all four entries, which happen before any device use -- this file runs without
a GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from kmer_spans_amd import _lib
from tests import kmeansref as R
from tests.test_nj import bits

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kmer_spans.h")


# ------------------------------------------------------------------- inputs

def planted_counts(rng, m: int, ncol: int, g: int, depth: int = 4000):
    """m rows drawn from g well separated column distributions (each group has
    its own heavy columns); returns (counts uint32 [m, ncol], planted labels 1 .. g)."""
    base = rng.random((g, ncol)) * 0.2
    for j in range(g):
        base[j, (j * 3) % ncol] += 3.0
        base[j, (j * 7 + 1) % ncol] += 2.0
    base /= base.sum(axis=1, keepdims=True)
    truth = (np.arange(m) % g).astype(np.int64)
    rng.shuffle(truth)
    counts = np.stack([rng.multinomial(depth, base[j]) for j in truth]).astype(np.uint32)
    return counts, (truth + 1).astype(np.int32)


def order_pin_case():
    """700 rows x 512 columns, a group of 600 members (three chunks) and one of
    100.  'Heavy' rows carry counts near 2^32 in most columns (T about 2^40, so a
    count of 1 is a profile entry of 2^-40), 'light' rows small counts (entries
    up to 1): the columns' sums round differently depending on where they are cut."""
    rng = np.random.default_rng(20250)
    m, ncol = 700, 512
    k = rng.integers(0, 32, size=(m, ncol))
    counts = np.floor(np.ldexp(1.0 + rng.random((m, ncol)), k)).astype(np.uint64)
    heavy = rng.random(m) < 0.5
    big = rng.random((m, ncol)) < 0.97
    counts[heavy[:, None] & big] = 0xFFFFFFFF
    light = ~heavy
    counts[light] = np.where(rng.random((int(light.sum()), ncol)) < 0.97, 0, counts[light] & 0xFF)
    counts[:, 0] |= 1  # no empty row
    counts[int(np.flatnonzero(light)[0]), 1:] = 0  # a profile entry of 1
    group = np.ones(m, dtype=np.int32)
    group[rng.permutation(m)[:100]] = 2
    return counts.astype(np.uint32), group


def tie_heavy_case(m: int):
    """Counts from {0, 1, 2, 3} in 4 columns: many rows are proportional, so
    initial centres taken from rows repeat each other and rows sit at equal
    distances from several centres.  Returns (counts, init_rows)."""
    rng = np.random.default_rng(m)
    counts = rng.integers(0, 4, size=(m, 4)).astype(np.uint32)
    counts[counts.sum(axis=1) == 0, 0] = 1
    return counts, np.arange(0, m, 5, dtype=np.int64)[:24]


def centre_ties(counts, init_rows) -> int:
    """Rows of the first pass whose smallest distance is reached by two or more centres."""
    p = R.profiles(counts)
    acc = R.sqdist(p, p[init_rows])
    return int(((acc == acc.min(axis=1, keepdims=True)).sum(axis=1) >= 2).sum())


LINE = np.array([[0, 8], [1, 7], [6, 2], [8, 0]], dtype=np.uint32)


# ------------------------------------------------------------- known answers

def test_four_points_on_a_line():
    """Counts (0 8) (1 7) (6 2) (8 0): profiles (0, 1) (.125, .875) (.75, .25)
    (1, 0), every value below exact in binary.  Centres start at rows 0 and 1.
    Pass 1: squared distances to (c1, c2) = (0, .03125) (.03125, 0) (1.125,
    .78125) (2, 1.53125): labels 1 2 2 2; c2 = ((.125 + .75 + 1) / 3, (.875 +
    .25 + 0) / 3) = (.625, .375), c1 stays (0, 1).
    Pass 2: row 1 is at .03125 from c1 and .5 from c2: labels 1 1 2 2; c1 =
    (.0625, .9375), c2 = (.875, .125).
    Pass 3: nothing changes: converged, iter = 3.
    withinss: rows 0 and 1 are at 2 * .0625^2 = .0078125 from c1, rows 2 and 3
    at 2 * .125^2 = .03125 from c2: .015625 and .0625, tot .078125.  totss: the centre of all rows is (.46875, .53125),
    the rows are at .439453125, .236328125, .158203125, .564453125: 1.3984375."""
    r = R.kmeans(LINE, [0, 1])
    assert r["cluster"].tolist() == [1, 1, 2, 2] and r["iter"] == 3 and r["converged"] is True
    assert r["centers"].tolist() == [[0.0625, 0.9375], [0.875, 0.125]]
    assert r["withinss"].tolist() == [0.015625, 0.0625] and r["size"].tolist() == [2, 2]
    assert r["tot_withinss"] == 0.078125 and r["totss"] == 1.3984375 and r["betweenss"] == 1.3984375 - 0.078125
    one = R.kmeans(LINE, [0, 1], iter_max=1)
    assert one["cluster"].tolist() == [1, 2, 2, 2] and one["iter"] == 1 and one["converged"] is False
    assert one["centers"].tolist() == [[0.0, 1.0], [0.625, 0.375]]
    # withinss of the returned labels against the returned centres: row 0 at 0; rows 1 2 3 at .5, .03125, .28125
    assert one["withinss"].tolist() == [0.0, 0.5 + 0.03125 + 0.28125]
    two = R.kmeans(LINE, [0, 1], iter_max=2)
    assert two["cluster"].tolist() == [1, 1, 2, 2] and two["iter"] == 2 and two["converged"] is False
    assert np.array_equal(bits(two["centers"]), bits(r["centers"]))
    gm = R.group_means(LINE, [1, 1, 2, 2])
    assert gm["centers"].tolist() == [[0.0625, 0.9375], [0.875, 0.125]] and gm["size"].tolist() == [2, 2]
    assert gm["withinss"].tolist() == [0.015625, 0.0625]


def test_pieces_are_the_plain_loops():
    """The squared distance, the centre and the wss as nested Python loops over
    Python floats (IEEE doubles, one rounding per operation), bit for bit."""
    rng = np.random.default_rng(5)
    m, ncol, g = 300, 7, 3
    counts = rng.integers(0, 50, size=(m, ncol)).astype(np.uint32)
    counts[:, 0] += 1
    p = R.profiles(counts)
    for s in range(m):
        T = int(counts[s].sum())
        assert [float(x) for x in p[s]] == [float(int(counts[s, c])) / float(T) for c in range(ncol)]
    cen = p[[3, 50, 200]] * 0.5 + 0.01
    acc = R.sqdist(p, cen)
    for s in range(0, m, 17):
        for j in range(g):
            a = 0.0
            for c in range(ncol):
                d = float(p[s, c]) - float(cen[j, c])
                a = a + d * d
            assert a == acc[s, j]
    label = R.assign(acc)
    for s in range(m):
        best, at = float("inf"), 0
        for j in range(g):
            if acc[s, j] < best:
                best, at = float(acc[s, j]), j + 1
        assert at == label[s]
    label[:280] = 1  # a group of more than one chunk
    new = R.update(p, label, cen)
    wss = R.withinss(p, label, new)
    for j in range(g):
        mem = [s for s in range(m) if label[s] == j + 1]
        for c in range(ncol):
            S = 0.0
            for t in range(0, len(mem), R.CHUNK):
                P = 0.0
                for s in mem[t:t + R.CHUNK]:
                    P = P + float(p[s, c])
                S = S + P
            assert S / float(len(mem)) == new[j, c]
        S = 0.0
        for t in range(0, len(mem), R.CHUNK):
            P = 0.0
            for s in mem[t:t + R.CHUNK]:
                a = 0.0
                for c in range(ncol):
                    d = float(p[s, c]) - float(new[j, c])
                    a = a + d * d
                P = P + a
            S = S + P
        assert S == wss[j]


# -------------------------------------------------- against an independent Lloyd

def plain_lloyd(p, cen, iter_max):
    """Broadcast distances, argmin, np.add.at means: no order is shared with the model."""
    cen = cen.copy()
    label = np.zeros(p.shape[0], dtype=np.int64)
    for _ in range(iter_max):
        new = ((p[:, None, :] - cen[None, :, :]) ** 2).sum(axis=2).argmin(axis=1) + 1
        if (new == label).all():
            break
        label = new
        s = np.zeros_like(cen)
        np.add.at(s, label - 1, p)
        n = np.bincount(label, minlength=cen.shape[0] + 1)[1:]
        cen[n > 0] = s[n > 0] / n[n > 0, None]
    return label, cen


@pytest.mark.parametrize("m,ncol,g", [(400, 16, 4), (1025, 16, 5), (700, 33, 7), (1500, 16, 3)])
def test_against_an_independent_lloyd(m, ncol, g):
    """Planted, well separated groups.  Either order of at most m additions of
    values in [0, 1] errs by at most m 2^-53 relative, and a mean is <= 1: the
    centres agree within m 2^-52 absolute; the labels are equal."""
    rng = np.random.default_rng(m + g)
    counts, truth = planted_counts(rng, m, ncol, g)
    start = np.array([int(np.flatnonzero(truth == j + 1)[0]) for j in range(g)])
    r = R.kmeans(counts, start, iter_max=20)
    p = R.profiles(counts)
    label, cen = plain_lloyd(p, p[start], 20)
    assert r["converged"] and np.array_equal(r["cluster"], label)
    assert np.array_equal(r["cluster"], truth)  # the plant is recovered
    err = np.abs(r["centers"] - cen).max()
    print(f"m = {m}: max |centre - plain| = {err:.3e}, bound {m * 2.0 ** -52:.3e}")
    assert err <= m * 2.0 ** -52


# ----------------------------------------------------------------- order pin

def test_order_pin_chunked_centres_differ_from_left_to_right():
    """The contract's sums are chunked; on this input that is visible in the
    bits of most entries of the large group's centre, so a kernel that adds in
    another order fails the GPU test on it."""
    counts, group = order_pin_case()
    p = R.profiles(counts)
    pos = p[p > 0]
    span = np.log2(pos.max()) - np.log2(pos.min())
    assert span >= 40, span
    assert np.bincount(group)[1] == 600 and np.bincount(group)[2] == 100
    zero = np.zeros((2, p.shape[1]))
    chunked, plain = R.update(p, group, zero), R.update(p, group, zero, chunk=None)
    differ = bits(chunked) != bits(plain)
    print(f"{int(differ[0].sum())} of {p.shape[1]} entries of the large group's centre differ in bits; "
          f"profile entries span {span:.1f} binades")
    assert differ[0].sum() >= p.shape[1] // 4
    assert not differ[1].any()  # 100 members: one chunk, the same order
    assert np.array_equal(bits(R.group_means(counts, group)["centers"]), bits(chunked))
    assert np.abs(chunked - plain).max() <= 700 * 2.0 ** -53


# ------------------------------------------------------------ ties and edges

def test_equidistant_row_takes_the_lower_label():
    counts = np.array([[4, 0], [0, 4], [2, 2]], dtype=np.uint32)  # row 2 is midway between rows 0 and 1
    r = R.kmeans(counts, [0, 1], iter_max=1)
    assert r["cluster"].tolist() == [1, 2, 1]
    r = R.kmeans(counts, [1, 0], iter_max=1)
    assert r["cluster"].tolist() == [2, 1, 1]


def test_duplicate_initial_centres():
    """Two equal centres: in the first pass the lower label takes every row of
    theirs; the higher one stays empty and keeps its bits, size 0 and withinss
    +0.0.  Later passes may hand it rows: its centre is still the row's profile
    while the lower label's centre has moved to its members' mean."""
    rng = np.random.default_rng(3)
    counts = rng.integers(1, 30, size=(50, 5)).astype(np.uint32)
    r = R.kmeans(counts, [7, 7, 20], iter_max=1)
    p = R.profiles(counts)
    assert 2 not in r["cluster"] and r["size"][1] == 0 and r["cluster"][7] == 1
    assert np.array_equal(bits(r["centers"][1]), bits(p[7]))
    assert not np.array_equal(bits(r["centers"][0]), bits(p[7]))
    assert r["withinss"][1] == 0.0 and not np.signbit(r["withinss"][1])
    full = R.kmeans(counts, [7, 7, 20], iter_max=50)
    assert full["converged"] and full["size"].sum() == 50


def test_a_centre_nobody_is_nearest_to_stays_empty():
    counts = np.array([[9, 1], [8, 2], [1, 9], [2, 8]], dtype=np.uint32)
    far = np.array([[0.9, 0.1], [0.1, 0.9], [5.0, -4.0]])
    r = R.kmeans(counts, far)
    assert r["cluster"].tolist() == [1, 1, 2, 2] and r["size"].tolist() == [2, 2, 0]
    assert np.array_equal(bits(r["centers"][2]), bits(far[2])) and bits(r["withinss"])[2] == 0
    assert r["converged"] and r["iter"] == 2  # the second pass changes nothing and is counted


def test_iter_max_one_labels_are_those_of_the_initial_centres():
    rng = np.random.default_rng(8)
    counts, _ = planted_counts(rng, 200, 8, 3)
    p = R.profiles(counts)
    r = R.kmeans(counts, [0, 1, 2], iter_max=1)
    assert r["converged"] is False and r["iter"] == 1
    assert np.array_equal(r["cluster"], R.assign(R.sqdist(p, p[[0, 1, 2]])))
    assert not np.array_equal(bits(r["centers"]), bits(p[[0, 1, 2]]))  # updated after the last pass


def test_one_group_is_totss_and_more_groups_than_rows():
    rng = np.random.default_rng(13)
    counts = rng.integers(1, 90, size=(600, 6)).astype(np.uint32)
    r = R.kmeans(counts, [5])
    assert r["iter"] == 2 and r["converged"] and r["size"].tolist() == [600]
    assert bits([r["tot_withinss"]])[0] == bits([r["totss"]])[0] == bits(r["withinss"])[0]
    few = counts[:3]
    r = R.kmeans(few, [0, 1, 2, 0, 1], iter_max=5)  # g = 5 > m = 3
    assert r["cluster"].tolist() == [1, 2, 3] and r["size"].tolist() == [1, 1, 1, 0, 0]
    assert not r["withinss"].any() and r["tot_withinss"] == 0.0 and r["converged"] and r["iter"] == 2


def test_tie_heavy_inputs_have_ties():
    """What the GPU test relies on: ties between centres do occur in its inputs."""
    for m in (130, 600):
        counts, init_rows = tie_heavy_case(m)
        n = centre_ties(counts, init_rows)
        print(f"m = {m}: {n} rows at equal distance from two or more centres")
        assert n > 0


def test_proportional_rows_share_a_group_at_distance_zero():
    counts = np.array([[1, 2, 3], [2, 4, 6], [50, 100, 150], [9, 1, 1], [18, 2, 2]], dtype=np.uint32)
    r = R.kmeans(counts, [0, 3])
    assert r["cluster"].tolist() == [1, 1, 1, 2, 2] and not r["withinss"].any()
    assert np.array_equal(bits(r["centers"]), bits(R.profiles(counts)[[0, 3]]))


# -------------------------------------------------------------- monotonicity

def test_tot_withinss_never_rises():
    """For one start, tot_withinss from iter_max = t to t + 1 never rises beyond
    64 ncol 2^-53 totss, the rounding of the sums."""
    rng = np.random.default_rng(1025)
    m, ncol, g = 1025, 16, 5
    counts = rng.integers(0, 40, size=(m, ncol)).astype(np.uint32)
    counts[:, 0] += 1
    start = np.arange(g) * 200
    prev, passes = None, 0
    for t in range(1, 80):
        r = R.kmeans(counts, start, iter_max=t)
        if prev is not None:
            assert r["tot_withinss"] <= prev + 64 * ncol * 2.0 ** -53 * r["totss"], t
        prev, passes = r["tot_withinss"], t
        if r["converged"]:
            break
    print(f"{passes} passes, converged {r['converged']}")
    assert r["tot_withinss"] <= r["totss"]


# ------------------------------------------------------------ argument checks

def _buffers(m, ncol, g):
    m, ncol, g = max(m, 1), max(min(ncol, 64), 1), max(min(g, 64), 1)
    return {"sp": np.ones((m, ncol), dtype=np.uint32), "init": np.full((g, ncol), 1.0 / ncol),
            "init_rows": np.zeros(g, dtype=np.int64), "cluster": np.zeros(m, dtype=np.int32),
            "centers": np.zeros((g, ncol)), "size": np.zeros(g, dtype=np.int32), "withinss": np.zeros(g),
            "group": np.ones(m, dtype=np.int32)}


def _kmeans(dev, m=5, ncol=4, g=2, iter_max=3, flags=0, n=None, rows=None, form="init", null=(), sp=None, init=None,
            init_rows=None):
    """A ks_spectra_kmeans(_dev) call that must be refused before any device use."""
    L = _lib.load()
    b = _buffers(m, ncol, g)
    if sp is not None:
        b["sp"] = np.ascontiguousarray(sp, dtype=np.uint32)
    if init is not None:
        b["init"] = np.ascontiguousarray(init, dtype=np.float64)
    if init_rows is not None:
        b["init_rows"] = np.ascontiguousarray(init_rows, dtype=np.int64)
    ptr = {k: (None if k in null else v.ctypes.data) for k, v in b.items()}
    rp = None if rows is None else np.ascontiguousarray(rows, dtype=np.int64).ctypes.data
    res = _lib.KmeansResult()
    args = [None, ptr["sp"], m if n is None else n, ncol, rp, m,
            ptr["init"] if form in ("init", "both") else None,
            ptr["init_rows"] if form in ("rows", "both") else None, g, iter_max, flags, ptr["cluster"],
            ptr["centers"], ptr["size"], ptr["withinss"], None if "res" in null else C.byref(res)]
    rc = L.ks_spectra_kmeans_dev(*args, None) if dev else L.ks_spectra_kmeans(*args)
    return rc, L.ks_last_error().decode()


def _means(dev, m=5, ncol=4, ngroups=2, flags=0, n=None, rows=None, group=None, null=(), sp=None):
    L = _lib.load()
    b = _buffers(m, ncol, ngroups)
    if sp is not None:
        b["sp"] = np.ascontiguousarray(sp, dtype=np.uint32)
    if group is not None:
        b["group"] = np.ascontiguousarray(group, dtype=np.int32)
    ptr = {k: (None if k in null else v.ctypes.data) for k, v in b.items()}
    rp = None if rows is None else np.ascontiguousarray(rows, dtype=np.int64).ctypes.data
    args = [None, ptr["sp"], m if n is None else n, ncol, rp, m, ptr["group"], ngroups, flags, ptr["centers"],
            ptr["size"], ptr["withinss"]]
    rc = L.ks_spectra_group_means_dev(*args, None) if dev else L.ks_spectra_group_means(*args)
    return rc, L.ks_last_error().decode()


@pytest.mark.parametrize("dev", [False, True])
def test_kmeans_entries_validate_before_any_device_call(dev):
    for m in (0, -2):
        rc, msg = _kmeans(dev, m=m)
        assert rc != 0 and "at least 1 row" in msg, msg
    for ncol in (0, -1, _lib.KS_DIST_MAX_NCOL + 1):
        rc, msg = _kmeans(dev, ncol=ncol)
        assert rc != 0 and "ncol must be between 1 and 4096" in msg, msg
    for g in (0, -1, _lib.KS_KM_MAX_GROUPS + 1):
        rc, msg = _kmeans(dev, g=g)
        assert rc != 0 and "groups must be between 1 and 65536" in msg, msg
    for it in (0, -5):
        rc, msg = _kmeans(dev, iter_max=it)
        assert rc != 0 and f"iter_max = {it} is not positive" in msg, msg
    for flags in (1, 2, -1):
        rc, msg = _kmeans(dev, flags=flags)
        assert rc != 0 and "unknown flags" in msg, msg
    rc, msg = _kmeans(dev, n=3)  # rows NULL and m = 5 > n
    assert rc != 0 and "exceeds n = 3" in msg, msg
    rc, msg = _kmeans(dev, null=("sp",))
    assert rc != 0 and "null spectra" in msg
    rc, msg = _kmeans(dev, form="both")
    assert rc != 0 and "exactly one of" in msg and "both are set" in msg
    rc, msg = _kmeans(dev, form="neither")
    assert rc != 0 and "exactly one of" in msg and "both are NULL" in msg
    for out in ("cluster", "centers", "size", "withinss", "res"):
        rc, msg = _kmeans(dev, null=(out,))
        assert rc != 0 and "null output" in msg, out


@pytest.mark.parametrize("dev", [False, True])
def test_group_means_entries_validate_before_any_device_call(dev):
    rc, msg = _means(dev, m=0)
    assert rc != 0 and "at least 1 row" in msg
    rc, msg = _means(dev, ncol=0)
    assert rc != 0 and "ncol must be between" in msg
    for ng in (0, -3, _lib.KS_KM_MAX_GROUPS + 1):
        rc, msg = _means(dev, ngroups=ng)
        assert rc != 0 and f"ngroups = {ng} is not in 1 .. 65536" in msg, msg
    rc, msg = _means(dev, flags=4)
    assert rc != 0 and "unknown flags" in msg
    rc, msg = _means(dev, n=2)
    assert rc != 0 and "exceeds n = 2" in msg
    rc, msg = _means(dev, null=("sp",))
    assert rc != 0 and "null spectra" in msg
    rc, msg = _means(dev, null=("group",))
    assert rc != 0 and "null group" in msg
    for out in ("centers", "size", "withinss"):
        rc, msg = _means(dev, null=(out,))
        assert rc != 0 and "null output" in msg, out
    for group, g, i, v in (([1, 2, 3, 1, 4], 3, 4, 4), ([1, 0, 2, 0, 1], 2, 1, 0), ([2, 1, -7, 9, 1], 2, 2, -7)):
        rc, msg = _means(dev, group=group, ngroups=g)
        assert rc != 0 and msg == f"group[{i}] = {v} is not in 1 .. {g}", msg


def test_host_entries_check_indices_sums_and_centres():
    """The host entries find a bad index, an empty row, a non-finite centre and
    a bad initial row before any device call; the index comes first."""
    sp = np.ones((5, 4), dtype=np.uint32)
    sp[3] = 0
    for call in (_kmeans, _means):
        rc, msg = call(False, sp=sp)
        assert rc != 0 and msg == "row 3 has no counts", msg
        rc, msg = call(False, sp=sp, rows=[0, 3, 9, 3, -1])
        assert rc != 0 and msg == "row index 2 out of range", msg
        rc, msg = call(False, sp=sp, rows=[4, 4, 3, 3, 0])
        assert rc != 0 and msg == "row 2 has no counts", msg
    for bad in (np.nan, np.inf, -np.inf):
        init = np.full((2, 4), 0.25)
        init[1, 2] = bad
        init[1, 3] = np.nan
        rc, msg = _kmeans(False, init=init)
        assert rc != 0 and msg == "center[1][2] is not finite", msg
    rc, msg = _kmeans(False, form="rows", init_rows=[0, 5])
    assert rc != 0 and msg == "initial row index 1 out of range", msg
    rc, msg = _kmeans(False, form="rows", init_rows=[-1, 2])
    assert rc != 0 and msg == "initial row index 0 out of range", msg
    rc, msg = _kmeans(False, sp=sp, form="rows", init_rows=[0, 7])  # the rows are checked first
    assert rc != 0 and msg == "row 3 has no counts", msg


def test_python_argument_checks():
    import kmer_spans_amd as K
    ok = np.ones((5, 4), dtype=np.uint32)
    for bad in (np.ones(5), np.ones((5, 4)), np.full((5, 4), -1)):
        with pytest.raises(K.KmerSpansError, match="counts"):
            K.region_kmeans(bad, [0, 1])
        with pytest.raises(K.KmerSpansError, match="counts"):
            K.region_group_means(bad, [1, 1, 1, 1, 1])
    for bad in ([], np.ones((2, 3)), [[0.5, 0.5]], [0.0, 1.0], np.ones((0, 4)), "ab"):
        with pytest.raises(K.KmerSpansError, match="centers"):
            K.region_kmeans(ok, bad)
    with pytest.raises(K.KmerSpansError, match="^initial row index 1 out of range$"):
        K.region_kmeans(ok, [0, 5])
    with pytest.raises(K.KmerSpansError, match="^center\\[0\\]\\[3\\] is not finite$"):
        K.region_kmeans(ok, np.array([[0.25, 0.25, 0.25, np.nan]]))
    with pytest.raises(K.KmerSpansError, match="iter_max = 0"):
        K.region_kmeans(ok, [0, 1], iter_max=0)
    with pytest.raises(K.KmerSpansError, match="group must hold"):
        K.region_group_means(ok, [1, 2])
    with pytest.raises(K.KmerSpansError, match="^group\\[1\\] = 2 is not in 1 .. 1$"):
        K.region_group_means(ok, [1, 2, 1, 1, 1], ngroups=1)
    with pytest.raises(K.KmerSpansError, match="^row index 1 out of range$"):
        K.region_group_means(ok, [1, 1], rows=[0, 5])
    init, rows, g = _lib.kmeans_centers([3, 1], 4)
    assert init is None and rows.dtype == np.int64 and g == 2
    init, rows, g = _lib.kmeans_centers(np.full((3, 4), 0.25, dtype=np.float32), 4)
    assert rows is None and init.dtype == np.float64 and g == 3
    assert _lib.KmeansStats().as_dict().keys() >= {"ms_normalise", "ms_assign", "ms_update", "ms_wss", "n_iter",
                                                   "panel_bytes", "work_bytes"}
    hdr = open(HEADER).read()
    assert _lib.KS_KM_CHUNK == R.CHUNK == 256 and "#define KS_KM_CHUNK 256\n" in hdr
    assert _lib.KS_KM_MAX_GROUPS == 65536 and "#define KS_KM_MAX_GROUPS 65536\n" in hdr
    assert C.sizeof(_lib.KmeansResult) == 24 and C.sizeof(_lib.KmeansStats) == 64
    assert {"region_kmeans", "region_group_means"} <= set(K.__all__)
