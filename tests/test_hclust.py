"""Hierarchical clustering of a condensed dissimilarity vector (ks_hclust /
ks_hclust_dev / ks_hclust_cut, include/kmer_spans.h): the host reference the
GPU tests compare against bit for bit (a numpy transcription of the header's
contract), known answers worked by hand, scipy as the independent check where
it is installed, the host-only tree cut through ctypes, and the argument
checks of the device entries, which all happen before any device use -- this
file runs without a GPU."""
import ctypes as C

import numpy as np
import pytest

METHODS = ("complete", "single", "average")


# ------------------------------------------------------------ host reference

def square(d, n: int) -> np.ndarray:
    """The condensed vector as a full symmetric matrix, +inf on the diagonal."""
    m = np.full((n, n), np.inf)
    i, j = np.triu_indices(n, 1)
    m[i, j] = d
    m[j, i] = d
    return m


def ref_hclust(d, n: int, method: str = "complete"):
    """The header's algorithm, step for step: (ia, ib, height, n_rescans).
    np.argmin returns the first minimum, which is the tie rule (and compares
    -0.0 equal to +0.0)."""
    assert method in METHODS
    d = np.asarray(d, dtype=np.float64)
    assert d.shape == (n * (n - 1) // 2,) and n >= 2 and np.isfinite(d).all()
    m = square(d, n)
    live = np.ones(n, dtype=bool)
    size = np.ones(n)
    nn = np.full(n, -1, dtype=np.int64)
    dnn = np.full(n, np.inf)

    def rescan(i):
        row = np.where(live[i + 1:], m[i, i + 1:], np.inf)
        j = int(np.argmin(row))
        if row[j] < np.inf:
            nn[i], dnn[i] = i + 1 + j, row[j]
        else:
            nn[i], dnn[i] = -1, np.inf

    for i in range(n - 1):
        rescan(i)
    ia, ib, height = np.zeros(n - 1, np.int32), np.zeros(n - 1, np.int32), np.zeros(n - 1)
    rescans = 0
    for s in range(n - 1):
        im = int(np.argmin(np.where(live[:n - 1], dnn[:n - 1], np.inf)))
        jm = int(nn[im])
        a, b = min(im, jm), max(im, jm)
        ia[s], ib[s], height[s] = a, b, dnn[im]
        live[b] = False
        k = live.copy()
        k[a] = False
        x, y = m[a, k], m[b, k]
        if method == "complete":
            r = np.where(y > x, y, x)
        elif method == "single":
            r = np.where(y < x, y, x)
        else:
            p, q = size[a] * x, size[b] * y  # each operation rounded on its own
            r = (p + q) / (size[a] + size[b])
        m[a, k] = r
        m[k, a] = r
        size[a] += size[b]
        marked = np.flatnonzero(live[:n - 1] & ((nn[:n - 1] == a) | (nn[:n - 1] == b)))
        marked = np.union1d(marked, [a])
        rescans += marked.size
        for i in marked:
            rescan(int(i))
    return ia, ib, height, rescans


def ref_merge_order(ia, ib, n: int):
    """R's merge table and leaf order from the steps' (a, b)."""
    lab = [-(i + 1) for i in range(n)]
    merge = np.zeros((n - 1, 2), dtype=np.int32)
    for s in range(n - 1):
        x, y = lab[ia[s]], lab[ib[s]]
        if x < 0 and y < 0:
            row = (x, y) if -x < -y else (y, x)
        elif x < 0 or y < 0:
            row = (min(x, y), max(x, y))  # the singleton, then the cluster
        else:
            row = (min(x, y), max(x, y))  # the earlier step first
        merge[s] = row
        lab[ia[s]] = s + 1
    order, stack = [], [n - 1]
    while stack:
        x = stack.pop()
        if x < 0:
            order.append(-x)
        else:
            stack.append(int(merge[x - 1, 1]))
            stack.append(int(merge[x - 1, 0]))
    return merge, np.array(order, dtype=np.int32)


def ref_tree(d, n, method="complete"):
    ia, ib, height, rescans = ref_hclust(d, n, method)
    merge, order = ref_merge_order(ia, ib, n)
    return {"merge": merge, "height": height, "order": order, "method": method, "n_rescans": rescans}


def ref_cut(merge, height, n: int, k=None, h=None) -> np.ndarray:
    """Apply the first n - k merges; groups numbered by first appearance."""
    if k is None:
        k = n - int((np.asarray(height) <= h).sum())
    members = {}
    for t in range(n - k):
        got = []
        for x in merge[t]:
            got += [int(-x - 1)] if x < 0 else members.pop(int(x))
        members[t + 1] = got
    group = np.zeros(n, dtype=np.int32)
    owner = np.arange(n) + n  # singletons: distinct ids
    for t, got in members.items():
        owner[got] = t
    seen = {}
    for i in range(n):
        group[i] = seen.setdefault(int(owner[i]), len(seen) + 1)
    return group


def bits(x) -> np.ndarray:
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def assert_same_tree(got, want, what=""):
    assert np.array_equal(got["merge"], want["merge"]), (what, "merge", got["merge"][:6], want["merge"][:6])
    assert np.array_equal(bits(got["height"]), bits(want["height"])), (what, "height")
    assert np.array_equal(got["order"], want["order"]), (what, "order")


def random_points_dist(rng, n: int, dim: int = 3) -> np.ndarray:
    """Tie-free input: Euclidean distances of random points, condensed."""
    p = rng.random((n, dim))
    i, j = np.triu_indices(n, 1)
    return np.sqrt(((p[i] - p[j]) ** 2).sum(axis=1))


def line_dist(x) -> np.ndarray:
    x = np.asarray(x, dtype=np.float64)
    i, j = np.triu_indices(x.size, 1)
    return np.abs(x[i] - x[j])


def star_ties(rng, n: int, V: int) -> np.ndarray:
    """Tie-rich input that keeps the rescan lists long: integers from
    {0 .. V-1}, condensed.  Uniform integers do not do that: the cluster of
    row 0 swallows its neighbours in index order and a step lists about one
    row (single linkage at n = 4,097: n + 5 rescans for V = 8, 2.7 n without
    any tie).  Here every pair draws from {V/2 .. V-1}, except within stars:
    with m = V / 2 and G = n // (m + 1), star g holds the rows g + G t,
    t = 0 .. m, the last of them its hub, and D(row t, hub) = m - 1 - t.  All
    m rows of a star have the hub as their nearest neighbour; when the closest
    of them merges with it the other m - 1 are listed at once, for single
    linkage again at every later merge within the star, and every star holds
    the same values.  The members of a star lie G rows apart, so the blocks of
    k_hclust_pair list rows in the same step."""
    m = V // 2
    G = n // (m + 1)
    assert m >= 2 and G >= 1
    D = rng.integers(m, V, size=(n, n)).astype(np.float64)
    for t in range(m):
        g = np.arange(G)
        D[g + G * t, g + G * m] = float(m - 1 - t)
    i, j = np.triu_indices(n, 1)
    return D[i, j].copy()


def test_star_ties_keep_the_lists_long():
    """The property the device test asserts at n = 4,097, at a size that costs
    nothing here: at least 4 n rescans for every method."""
    n, V = 521, 32
    d = star_ties(np.random.default_rng(n), n, V)
    assert d.min() == 0 and d.max() == V - 1 and (d == np.floor(d)).all()
    for method in METHODS:
        assert ref_tree(d, n, method)["n_rescans"] >= 4 * n, method


# -------------------------------------------------------------- known answers

LINE5 = [0.0, 1.0, 3.0, 7.0, 15.0]
# average linkage of the five points, the operations as the contract orders them
_AVG_02 = (1.0 * 3.0 + 1.0 * 2.0) / 2.0                        # {0,1} - 2
_AVG_03 = (1.0 * 7.0 + 1.0 * 6.0) / 2.0                        # {0,1} - 3
_AVG_04 = (1.0 * 15.0 + 1.0 * 14.0) / 2.0                      # {0,1} - 4
_AVG_013 = (2.0 * _AVG_03 + 1.0 * 4.0) / 3.0                   # {0,1,2} - 3
_AVG_014 = (2.0 * _AVG_04 + 1.0 * 12.0) / 3.0                  # {0,1,2} - 4
_AVG_0124 = (3.0 * _AVG_014 + 1.0 * 8.0) / 4.0                 # {0,1,2,3} - 4
LINE5_HEIGHT = {"complete": [1.0, 3.0, 7.0, 15.0], "single": [1.0, 2.0, 4.0, 8.0],
                "average": [1.0, _AVG_02, _AVG_013, _AVG_0124]}
LINE5_MERGE = [[-1, -2], [-3, 1], [-4, 2], [-5, 3]]
LINE5_ORDER = [5, 4, 3, 1, 2]


@pytest.mark.parametrize("method", METHODS)
def test_reference_line_of_five(method):
    """0, 1, 3, 7, 15 on a line: every gap is larger than the span to its
    left, so each method adds the next point to the one growing cluster."""
    t = ref_tree(line_dist(LINE5), 5, method)
    assert t["merge"].tolist() == LINE5_MERGE
    assert t["height"].tolist() == LINE5_HEIGHT[method]
    assert t["order"].tolist() == LINE5_ORDER
    assert LINE5_HEIGHT["average"][1] == 2.5 and abs(LINE5_HEIGHT["average"][3] - 12.25) < 1e-14


@pytest.mark.parametrize("method", METHODS)
def test_reference_all_equal(method):
    """All distances equal: the lowest pair merges, then the lowest remaining
    observation joins that cluster, step after step.  By the header's row rule
    a singleton stands before a cluster, so the rows read (-1, -2), (-3, 1),
    (-4, 2), ... and the leaves from the left are n, n - 1, ..., 3, 1, 2, as R
    prints the same tree."""
    n = 23
    t = ref_tree(np.full(n * (n - 1) // 2, 0.75), n, method)
    want = [[-1, -2]] + [[-(s + 2), s] for s in range(1, n - 1)]
    assert t["merge"].tolist() == want
    assert t["height"].tolist() == [0.75] * (n - 1)
    assert t["order"].tolist() == list(range(n, 2, -1)) + [1, 2]
    assert sorted(t["order"].tolist()) == list(range(1, n + 1))


def test_reference_signed_zeros_tie():
    """-0.0 and +0.0 are one value: the lowest index wins, and the height keeps
    the bits of the entry that won."""
    d = np.array([1.0, 0.0, 2.0, -0.0, 3.0, 4.0])  # pairs 01 02 03 12 13 23: (0,2) and (1,2) at zero
    ia, ib, height, _ = ref_hclust(d, 4, "complete")
    assert (ia[0], ib[0]) == (0, 2) and bits(height)[0] == bits(0.0)[0]
    d = np.array([1.0, -0.0, 2.0, 0.0, 3.0, 4.0])
    ia, ib, height, _ = ref_hclust(d, 4, "complete")
    assert (ia[0], ib[0]) == (0, 2) and bits(height)[0] == bits(-0.0)[0]


# ------------------------------------------------------------- against scipy

def to_linkage(merge, height, n):
    z = np.zeros((n - 1, 4))
    cnt = np.ones(2 * n - 1)
    for s in range(n - 1):
        ids = [(-x - 1) if x < 0 else (n + x - 1) for x in merge[s]]
        cnt[n + s] = cnt[ids[0]] + cnt[ids[1]]
        z[s] = [min(ids), max(ids), height[s], cnt[n + s]]
    return z


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("n", [2, 3, 17, 60])
def test_reference_against_scipy(n, method):
    """Tie-free input: the heights are scipy's bit for bit for complete and
    single linkage; for average within rtol = 1e-12 (fewer than 60 chained
    averagings of three roundings each stay under 2e-14); the cophenetic
    distances of our merge table equal scipy's."""
    hier = pytest.importorskip("scipy.cluster.hierarchy")
    d = random_points_dist(np.random.default_rng(100 * n + len(method)), n)
    t = ref_tree(d, n, method)
    z = hier.linkage(d, method)
    if method == "average":
        np.testing.assert_allclose(t["height"], z[:, 2], rtol=1e-12, atol=0)
    else:
        assert np.array_equal(bits(t["height"]), bits(z[:, 2]))
    ours = to_linkage(t["merge"], t["height"], n)
    assert np.array_equal(ours[:, 3], z[:, 3])
    if method == "average":
        np.testing.assert_allclose(hier.cophenet(ours), hier.cophenet(z), rtol=1e-12, atol=0)
    else:
        assert np.array_equal(bits(hier.cophenet(ours)), bits(hier.cophenet(z)))
    assert sorted(t["order"].tolist()) == list(range(1, n + 1))
    for k in (1, min(3, n), n):
        g = ref_cut(t["merge"], t["height"], n, k=k)
        f = hier.fcluster(z, k, "maxclust")
        assert len(set(zip(g.tolist(), f.tolist()))) == k == len(set(g.tolist())) == len(set(f.tolist()))  # one partition


# ------------------------------------------------------ ks_hclust_cut (host)

def _cut(merge, height, n, k=0, h=0.0, group=True):
    from kmer_spans_amd import _lib
    L = _lib.load()
    m = np.ascontiguousarray(merge, dtype=np.int32) if merge is not None else None
    ht = np.ascontiguousarray(height, dtype=np.float64) if height is not None else None
    g = np.full(max(n, 1), -7, dtype=np.int32)
    rc = L.ks_hclust_cut(m.ctypes.data if m is not None else None, ht.ctypes.data if ht is not None else None, n, k,
                         h, g.ctypes.data if group else None)
    return rc, L.ks_last_error().decode(), g


@pytest.fixture(scope="module")
def tree40():
    return ref_tree(random_points_dist(np.random.default_rng(40), 40), 40, "complete")


def test_cut_every_k(tree40):
    import kmer_spans_amd as K
    n = 40
    for k in range(1, n + 1):
        rc, msg, g = _cut(tree40["merge"], tree40["height"], n, k=k)
        assert rc == 0, msg
        assert np.array_equal(g, ref_cut(tree40["merge"], tree40["height"], n, k=k)), k
        assert g[0] == 1 and set(g.tolist()) == set(range(1, k + 1))
        first = [int(np.flatnonzero(g == c)[0]) for c in range(1, k + 1)]
        assert first == sorted(first), "groups are numbered by first appearance"
        assert np.array_equal(K.cut_tree(tree40, k=k), g)
        assert np.array_equal(K.cut_tree(tree40["merge"], k=k), g)  # k needs no heights


def test_cut_at_heights(tree40):
    import kmer_spans_amd as K
    n, ht = 40, tree40["height"]
    assert (np.diff(ht) > 0).all()
    cases = [(ht[0] / 2, n), ((ht[9] + ht[10]) / 2, n - 10), (ht[10], n - 11), (np.nextafter(ht[10], 0), n - 10),
             (ht[-1], 1), (ht[-1] * 2, 1), (np.inf, 1), (-1.0, n)]
    for h, k in cases:
        rc, msg, g = _cut(tree40["merge"], ht, n, k=0, h=float(h))
        assert rc == 0, msg
        assert len(set(g.tolist())) == k, (h, k)
        assert np.array_equal(g, ref_cut(tree40["merge"], ht, n, h=h))
        assert np.array_equal(g, ref_cut(tree40["merge"], ht, n, k=k))
        assert np.array_equal(K.cut_tree(tree40, h=float(h)), g)
        assert np.array_equal(K.cut_tree(tree40["merge"], height=ht, h=float(h)), g)


def test_cut_bounds_the_diameter(tree40):
    """Complete linkage: no two members of a group are further apart than h."""
    import kmer_spans_amd as K
    n = 40
    d = random_points_dist(np.random.default_rng(40), n)
    m = square(d, n)
    h = float(tree40["height"][25])
    g = K.cut_tree(tree40, h=h)
    same = g[:, None] == g[None, :]
    np.fill_diagonal(same, False)
    assert same.any() and m[same].max() <= h
    # and it is tight: one more merge would pass h
    g2 = K.cut_tree(tree40, k=len(set(g.tolist())) - 1)
    same2 = g2[:, None] == g2[None, :]
    np.fill_diagonal(same2, False)
    assert m[same2].max() > h


def test_cut_rejects_bad_arguments(tree40):
    import kmer_spans_amd as K
    n, merge, ht = 40, tree40["merge"], tree40["height"]
    unsorted = ht.copy()
    unsorted[[5, 6]] = unsorted[[6, 5]]
    rc, msg, g = _cut(merge, unsorted, n, k=0, h=1.0)
    assert rc != 0 and "not sorted" in msg and (g == -7).all()
    with pytest.raises(K.KmerSpansError, match="not sorted"):
        K.cut_tree(merge, height=unsorted, h=1.0)
    for k in (-1, n + 1):
        rc, msg, _ = _cut(merge, ht, n, k=k)
        assert rc != 0 and "1 .. n" in msg
    for k in (0, -1, n + 1, 2.5):
        with pytest.raises(K.KmerSpansError, match="1 .. n"):
            K.cut_tree(tree40, k=k)
    with pytest.raises(K.KmerSpansError, match="exactly one of k and h"):
        K.cut_tree(tree40)
    with pytest.raises(K.KmerSpansError, match="exactly one of k and h"):
        K.cut_tree(tree40, k=3, h=0.5)
    with pytest.raises(K.KmerSpansError, match="needs the heights"):
        K.cut_tree(merge, h=0.5)
    assert _cut(merge, ht, 1, k=1)[0] != 0
    assert _cut(None, ht, n, k=3)[0] != 0
    assert _cut(merge, ht, n, k=3, group=False)[0] != 0
    rc, msg, _ = _cut(merge, ht, n, k=0, h=float("nan"))
    assert rc != 0 and "NaN" in msg
    bad = merge.copy()
    bad[3, 1] = 30  # a step that has not happened yet
    rc, msg, _ = _cut(bad, ht, n, k=2)
    assert rc != 0 and "merge[3][1]" in msg
    bad[3, 1] = -41
    assert _cut(bad, ht, n, k=2)[0] != 0


# ------------------------------------------- device entries: validation only

def _hclust(n, method=0, flags=0, dev=False, diss=True, outs=(True, True, True), d=None):
    """A call that must be refused before any device use: this machine has no GPU."""
    from kmer_spans_amd import _lib
    L = _lib.load()
    d = np.ones(max(1, abs(n) * (abs(n) - 1) // 2)) if d is None else np.ascontiguousarray(d, dtype=np.float64)
    merge, height, order = _lib.hclust_outputs(max(abs(n), 2))
    ptr = [x.ctypes.data if keep else None for x, keep in zip((merge, height, order), outs)]
    dp = d.ctypes.data if diss else None
    if dev:  # the pointer is never followed: the arguments fail first
        rc = L.ks_hclust_dev(None, dp, n, method, flags, ptr[0], ptr[1], ptr[2], None)
    else:
        rc = L.ks_hclust(None, dp, n, method, ptr[0], ptr[1], ptr[2])
    return rc, L.ks_last_error().decode()


@pytest.mark.parametrize("dev", [False, True])
def test_entries_validate_before_any_device_call(dev):
    for n in (1, 0, -3):
        rc, msg = _hclust(n, dev=dev)
        assert rc != 0 and "at least 2 observations" in msg
    for method in (-1, 3, 99):
        rc, msg = _hclust(5, method=method, dev=dev)
        assert rc != 0 and "unknown hclust method" in msg
    assert _hclust(5, dev=dev, diss=False)[0] != 0
    for outs in ((False, True, True), (True, False, True), (True, True, False)):
        rc, msg = _hclust(5, dev=dev, outs=outs)
        assert rc != 0 and "null output" in msg
    if dev:
        for flags in (2, 4, -1):
            rc, msg = _hclust(5, flags=flags, dev=True)
            assert rc != 0 and "unknown hclust flags" in msg


@pytest.mark.parametrize("badval", [np.nan, np.inf, -np.inf])
def test_host_entry_names_the_first_bad_offset(badval):
    """ks_hclust checks every entry on the host before any device call."""
    import kmer_spans_amd as K
    d = np.ones(10)
    d[[4, 7]] = badval
    rc, msg = _hclust(5, d=d)
    assert rc != 0 and msg == "dissimilarity at offset 4 is not finite"
    with pytest.raises(K.KmerSpansError, match="^dissimilarity at offset 4 is not finite$"):
        K.region_hclust(d)


def test_python_argument_checks():
    import kmer_spans_amd as K
    for size in (0, 2, 4, 5, 7):
        with pytest.raises(K.KmerSpansError, match="n\\(n-1\\)/2"):
            K.region_hclust(np.ones(size))
    with pytest.raises(K.KmerSpansError, match="method must be one of"):
        K.region_hclust(np.ones(3), method="ward")
    with pytest.raises(K.KmerSpansError, match="1-d"):
        K.region_hclust(np.ones((3, 1)))
    from kmer_spans_amd import _lib
    assert [_lib.hclust_n(m * (m - 1) // 2) for m in (2, 3, 4, 1000, 24611, 66000)] == [2, 3, 4, 1000, 24611, 66000]
    assert {"region_hclust", "cut_tree"} <= set(K.__all__)
