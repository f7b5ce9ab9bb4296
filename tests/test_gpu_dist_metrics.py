"""The metrics of region_distances and region_knn on the device (manhattan,
maximum, canberra, hellinger beside euclidean) against the host model of
tests/metricref.py.  Every result is compared in its bits (a NaN equals a NaN),
with one exception: where a final square root is taken (euclidean and hellinger
without squared=True) the result is within 1 ulp of np.sqrt of the model's
value, as in tests/test_gpu_spectra_dist.py.  Hellinger's panel root feeds the
accumulator, so its squared form is compared bit for bit.  Runs on an MI355X
(pytest -m gpu)."""
import numpy as np
import pytest

from tests import knnref as R
from tests import metricref as M
from tests.test_gpu_spectra_dist import assert_sqrt_of, same_bits
from tests.test_spectra_dist import bits, condensed_pairs, pair_offsets, profiles, random_counts

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


def assert_bits(got, want, what):
    same = same_bits(got, want)
    assert same.all(), (what, int((~same).sum()), "differ, first at", np.argwhere(~same)[:4].tolist(),
                        np.asarray(got)[~same][:4], np.asarray(want)[~same][:4])


def check_distances(ctx, metric, dc, value, rows=None, rows_b=None, what=""):
    """device.region_distances in both forms of `metric` against the model's value of every pair."""
    from kmer_spans_amd import device as D
    what = f"{metric} {what}"
    d, st = D.region_distances(ctx, dc, rows=rows, rows_b=rows_b, metric=metric)
    got = d.cpu().numpy()
    assert got.shape == value.shape and st["n_pairs"] == value.size, (what, got.shape, value.shape)
    if metric in M.HAS_SQUARED:
        sq, _ = D.region_distances(ctx, dc, rows=rows, rows_b=rows_b, metric=metric, squared=True)
        assert_bits(sq.cpu().numpy(), M.result(metric, value, squared=True), what + " squared")
        assert_sqrt_of(got, M.before_root(metric, value), what)
    else:
        assert_bits(got, value, what)
    return got


# --------------------------------------------- tile edges, chunks, diagonal

SIZES = [(m, ncol) for m in (2, 3, 63, 64, 65, 129) for ncol in (1, 4, 17, 33, 256)] + [(5, 4096)]


@pytest.mark.parametrize("m,ncol", SIZES)
def test_condensed_and_cross(ctx, m, ncol):
    """Either side of the 64-row tile and of the 16-column chunk, one column,
    the largest ncol: the condensed form and a cross form with a descending
    selection that repeats a row."""
    counts = random_counts(np.random.default_rng(1000 * m + ncol), m, ncol)
    dc = to_dev(counts)
    rows_b = np.concatenate([np.arange(m - 1, -1, -2), [0, 0]]).astype(np.int64)
    for metric in M.METRICS:
        check_distances(ctx, metric, dc, M.condensed_value(metric, counts), what=f"m={m} ncol={ncol}")
        check_distances(ctx, metric, dc, M.cross_value(metric, counts, None, rows_b), rows_b=rows_b,
                        what=f"cross m={m} ncol={ncol}")


# ------------------------------------------------------------- special rows

def special_rows(ncol):
    """Row 0 empty; rows 1 .. 4 a row and its multiples x 2, x 3, x 1000; rows
    5 .. 4 + ncol with counts in the first 1 .. ncol columns only, then one more
    with column 0 alone (against it a row with a columns keeps a of them: cnt
    runs from 1 to ncol); then bins of 2^32 - 1: a full row, one with a hole, a
    single huge bin, and the row of ones proportional to the full one; an empty
    row at the end."""
    rng = np.random.default_rng(ncol)
    base = rng.integers(1, 4000, size=ncol).astype(np.uint32)
    base[rng.random(ncol) < 0.3] = 0
    base[0] |= 1
    rows = [np.zeros(ncol, dtype=np.uint32), base, base * 2, base * 3, base * 1000]
    for a in range(1, ncol + 1):
        r = np.zeros(ncol, dtype=np.uint32)
        r[:a] = rng.integers(1, 1000, size=a)
        rows.append(r)
    rows.append(np.array([9] + [0] * (ncol - 1), dtype=np.uint32))
    full = np.full(ncol, 0xFFFFFFFF, dtype=np.uint32)
    hole, huge = full.copy(), np.zeros(ncol, dtype=np.uint32)
    hole[ncol // 2] = 0
    huge[ncol - 1] = 0xFFFFFFFF
    rows += [full, hole, huge, np.ones(ncol, dtype=np.uint32), np.zeros(ncol, dtype=np.uint32)]
    return np.vstack(rows)


@pytest.mark.parametrize("ncol", [17, 70])
def test_special_rows(ctx, ncol):
    counts = special_rows(ncol)
    m = counts.shape[0]
    dc = to_dev(counts)
    i, j = condensed_pairs(m)
    p = profiles(counts)
    cnt = M.canberra_count(p, i, j)
    ok = (i != 0) & (j != m - 1)  # i < j: row 0 is never j, the last row never i
    assert set(range(1, ncol + 1)) <= set(cnt[ok].tolist())
    for metric in M.METRICS:
        got = check_distances(ctx, metric, dc, M.VALUE[metric](p, i, j), what=f"special rows ncol={ncol}")
        assert np.isnan(got[~ok]).all() and not np.isnan(got[ok]).any(), metric
        at = {(a, b): x for a, b, x in zip(i.tolist(), j.tolist(), got.tolist())}
        for a in range(1, 5):
            for b in range(a + 1, 5):
                assert at[(a, b)] == 0.0, (metric, a, b)  # proportional rows
        assert at[(m - 5, m - 2)] == 0.0, metric  # 2^32 - 1 everywhere against 1 everywhere
        x = check_distances(ctx, metric, dc, M.cross_value(metric, counts, [0, 3, m - 1, 7], [1, 0, m - 4, 4]),
                            rows=np.array([0, 3, m - 1, 7]), rows_b=np.array([1, 0, m - 4, 4]),
                            what="special rows, cross")
        assert np.isnan(x[0]).all() and np.isnan(x[2]).all() and np.isnan(x[:, 1]).all()
        assert x[1, 0] == 0.0 and x[1, 3] == 0.0 and not np.isnan(x[[1, 3]][:, [0, 2, 3]]).any()


# --------------------------------------------------------------- selections

def test_selections(ctx):
    """Reversed, repeated and subset selections as numpy and as CUDA tensors;
    the cross form against the condensed form and against its own transpose;
    out= reuse."""
    import torch
    from kmer_spans_amd import device as D
    n, ncol = 150, 33
    counts = random_counts(np.random.default_rng(150), n, ncol)
    dc = to_dev(counts)
    rev = np.arange(n - 1, -1, -1)
    rep = np.array([5, 5, 17, 149, 0, 5, 64, 63, 65])
    sub = np.arange(3, n, 7)
    for metric in M.METRICS:
        for name, rows in (("reversed", rev), ("repeated", rep), ("subset", sub)):
            want = M.condensed_value(metric, counts, rows)
            check_distances(ctx, metric, dc, want, rows=rows, what=name)
            check_distances(ctx, metric, dc, want, rows=torch.from_numpy(rows).cuda(), what=name + ", cuda")
        sq = metric in M.HAS_SQUARED
        cond, _ = D.region_distances(ctx, dc, rows=sub, metric=metric, squared=sq)
        block, _ = D.region_distances(ctx, dc, rows=sub, rows_b=sub, metric=metric, squared=sq)
        i, j = condensed_pairs(sub.size)
        blk = block.cpu().numpy()
        assert np.array_equal(bits(blk[i, j]), bits(cond.cpu().numpy())), metric
        assert np.array_equal(bits(blk), bits(blk.T)) and not bits(np.diag(blk)).any(), metric
        ab, _ = D.region_distances(ctx, dc, rows=rep, rows_b=rev, metric=metric)
        ba, _ = D.region_distances(ctx, dc, rows=rev, rows_b=rep, metric=metric)
        assert np.array_equal(bits(ab.cpu().numpy()), bits(ba.cpu().numpy().T)), metric
        assert not ab.cpu().numpy()[0, n - 1 - 5]  # row 5 against itself
        out = torch.full((rep.size * n,), -7.0, dtype=torch.float64, device="cuda")
        res, _ = D.region_distances(ctx, dc, rows=rep, rows_b=rev, metric=metric, out=out)
        assert res.data_ptr() == out.data_ptr() and tuple(res.shape) == (rep.size, n)
        assert torch.equal(res.view(torch.int64), ab.view(torch.int64)), metric
    with pytest.raises(Exception, match="metric must be one of"):
        D.region_distances(ctx, dc, metric="cityblock")
    with pytest.raises(Exception, match="squared=True has no meaning"):
        D.region_knn(ctx, dc, 3, metric="canberra", squared=True)


def test_host_entries(ctx):
    import kmer_spans_amd as K
    counts = random_counts(np.random.default_rng(77), 70, 17)
    rows, rows_b = np.arange(69, -1, -1), np.array([3, 3, 68, 0])
    for metric in M.METRICS:
        sq = metric in M.HAS_SQUARED
        want = M.result(metric, M.condensed_value(metric, counts, rows), squared=sq)
        assert_bits(K.region_distances(counts, rows=rows, metric=metric, squared=sq), want, metric + ", host")
        wantx = M.cross_value(metric, counts, rows, rows_b)
        assert_bits(K.region_distances(counts.astype(np.int64), rows=rows, rows_b=rows_b, metric=metric, squared=sq),
                    M.result(metric, wantx, squared=sq), metric + ", host cross")
        wi, wv = R.select(wantx, 3)
        gi, gd = K.region_knn(counts, 3, rows=rows, rows_b=rows_b, metric=metric, squared=sq)
        assert np.array_equal(gi, wi), metric
        assert_bits(gd, M.result(metric, wv, squared=sq), metric + ", host knn")


# -------------------------------------------------------------- a larger case

def test_larger_case(ctx):
    """m = 1,000 at ncol = 256: 136 tiles through the triangular mapping, 4,096 sampled pairs per metric."""
    import torch
    from kmer_spans_amd import device as D
    m, ncol = 1000, 256
    counts = random_counts(np.random.default_rng(1000), m, ncol)
    counts[77] = 0
    dc = to_dev(counts)
    p = profiles(counts)
    rng = np.random.default_rng(4096)
    si = rng.integers(0, m - 1, 4096)
    sj = si + 1 + (rng.random(4096) * (m - 1 - si)).astype(np.int64)
    si[:8], sj[:8] = [0, 63, 63, 64, 77, 5, 998, 0], [1, 64, 999, 65, 78, 77, 999, 999]
    assert ((si < sj) & (sj < m)).all()
    off = torch.from_numpy(pair_offsets(si, sj, m)).cuda()
    for metric in M.METRICS:
        sq = metric in M.HAS_SQUARED
        d, st = D.region_distances(ctx, dc, metric=metric, squared=sq)
        assert st["n_pairs"] == m * (m - 1) // 2
        want = M.result(metric, M.VALUE[metric](p, si, sj), squared=sq)
        assert np.isnan(want[4:6]).all()
        assert_bits(d[off].cpu().numpy(), want, f"{metric}, larger case")
        assert int(torch.isnan(d).sum()) == m - 1, metric


# ----------------------------------------------------------------------- knn

def check_knn(ctx, metric, dc, k, value, rows=None, rows_b=None, what=""):
    """device.region_knn against np.lexsort of the model's values, and its
    distances against region_distances gathered at the returned positions."""
    import torch
    from kmer_spans_amd import device as D
    what = f"{metric} k={k} {what}"
    self_form = rows_b is None
    wi, wv = R.select(value, k, np.arange(value.shape[0]) if self_form else None)
    index, d, st = D.region_knn(ctx, dc, k, rows=rows, rows_b=rows_b, metric=metric)
    gi = index.cpu().numpy()
    assert np.array_equal(gi, wi), (what, "index", int((gi != wi).sum()), np.argwhere(gi != wi)[:4].tolist())
    block, _ = D.region_distances(ctx, dc, rows=rows, rows_b=rows if self_form else rows_b, metric=metric)
    assert torch.equal(torch.gather(block, 1, index).view(torch.int64), d.view(torch.int64)), (what, "gathered")
    if metric in M.HAS_SQUARED:
        i2, sq, _ = D.region_knn(ctx, dc, k, rows=rows, rows_b=rows_b, metric=metric, squared=True)
        assert np.array_equal(i2.cpu().numpy(), wi), (what, "index of the squared call")
        assert_bits(sq.cpu().numpy(), M.result(metric, wv, squared=True), what + " squared")
        assert_sqrt_of(d.cpu().numpy(), M.before_root(metric, wv), what)
        blk2, _ = D.region_distances(ctx, dc, rows=rows, rows_b=rows if self_form else rows_b, metric=metric,
                                     squared=True)
        assert torch.equal(torch.gather(blk2, 1, index).view(torch.int64), sq.view(torch.int64)), (what, "gathered")
    else:
        assert_bits(d.cpu().numpy(), wv, what)
    return st


@pytest.mark.parametrize("na,ncol", [(65, 4), (65, 17), (200, 33), (200, 256)])
@pytest.mark.parametrize("metric", M.METRICS)
def test_knn(ctx, metric, na, ncol):
    """Self form, and a cross form with a descending selection that repeats
    rows; ncol below, off and on the 16-column chunk the tile pads to."""
    n = na + 30
    counts = random_counts(np.random.default_rng(na * ncol), n, ncol)
    dc = to_dev(counts)
    rows = np.arange(na, dtype=np.int64)
    rows_b = np.concatenate([np.arange(n - 1, 9, -1), [12, 12, 11, n - 1]]).astype(np.int64)
    self_value = M.cross_value(metric, counts, rows, rows)
    cross_value = M.cross_value(metric, counts, rows, rows_b)
    for k in (1, 10, 64):
        check_knn(ctx, metric, dc, k, self_value, rows=rows, what=f"self na={na} ncol={ncol}")
        check_knn(ctx, metric, dc, k, cross_value, rows=rows, rows_b=rows_b, what=f"cross na={na} ncol={ncol}")


def test_knn_ties_go_to_the_lowest_position(ctx):
    """Proportional rows and exact copies: values of exactly 0 in every metric."""
    from kmer_spans_amd import device as D
    m = 130
    scale = (np.arange(m, dtype=np.uint32) % 7 + 1)[:, None]
    counts = np.tile(np.array([[3, 1, 0, 4, 1]], dtype=np.uint32), (m, 1)) * scale
    dc = to_dev(counts)
    for metric in M.METRICS:
        index, d, _ = D.region_knn(ctx, dc, 17, metric=metric)
        assert not d.cpu().numpy().any(), metric
        got = index.cpu().numpy()
        for s in (0, 5, 16, 17, 18, 63, 64, 129):
            assert got[s].tolist() == [j for j in range(m) if j != s][:17], (metric, s)


def test_knn_split_and_merge(ctx):
    """8,192 candidates, as many as the largest case of tests/test_gpu_knn.py,
    for 130 queries: the candidate tiles are split over the grid and the merge
    kernel writes the result."""
    nb, na, ncol = 8192, 130, 16
    counts = random_counts(np.random.default_rng(8192), nb, ncol)
    dc = to_dev(counts)
    rows, rows_b = np.arange(0, 2 * na, 2, dtype=np.int64), np.arange(nb, dtype=np.int64)
    value = M.cross_value("manhattan", counts, rows, rows_b)
    st = check_knn(ctx, "manhattan", dc, 10, value, rows=rows, rows_b=rows_b, what="split")
    print(f"manhattan, {na} x {nb}: {st['n_splits']} splits of {st['tiles_per_split']} tiles")
    assert st["n_splits"] > 1 and st["work_bytes"] >= 12 * na * 10 * st["n_splits"]


# --------------------------------------------------------- no drift elsewhere

def test_no_drift_elsewhere(ctx):
    """The Euclidean outputs are the model's bits, and PCA and k-means, which
    normalise a panel of their own through the shared kernel, give the same
    bits before and after Hellinger calls on the same context: no root leaks."""
    import torch
    from kmer_spans_amd import device as D
    m, ncol = 200, 33
    counts = random_counts(np.random.default_rng(2033), m, ncol)
    dc = to_dev(counts)
    value = M.condensed_value("euclidean", counts)
    sq, _ = D.region_distances(ctx, dc, squared=True)
    assert_bits(sq.cpu().numpy(), value, "euclidean, default metric")
    sq2, _ = D.region_distances(ctx, dc, squared=True, metric="euclidean")
    assert torch.equal(sq.view(torch.int64), sq2.view(torch.int64))
    wi, wv = R.select(M.cross_value("euclidean", counts, None, None), 10, np.arange(m))
    start = np.arange(0, m, 25, dtype=np.int64)

    def others():
        index, acc, _ = D.region_knn(ctx, dc, 10, squared=True)
        pca, _ = D.region_pca(ctx, dc)
        km, _ = D.region_kmeans(ctx, dc, start, iter_max=5)
        return ([index, acc.view(torch.int64), km["cluster"], km["centers"].view(torch.int64)]
                + [pca[key].view(torch.int64) for key in ("sdev", "rotation", "center", "x")])
    before = others()
    assert np.array_equal(before[0].cpu().numpy(), wi)
    assert_bits(before[1].view(torch.float64).cpu().numpy(), wv, "euclidean knn")
    D.region_distances(ctx, dc, metric="hellinger")
    D.region_distances(ctx, dc, rows_b=np.arange(5), metric="hellinger", squared=True)
    D.region_knn(ctx, dc, 10, metric="hellinger")
    after = others()
    for a, b in zip(before, after):
        assert torch.equal(a, b)


# ------------------------------------------------------------------ pipeline

def test_pipeline_manhattan_single_linkage_cut(ctx):
    """40 regions in two planted clusters: region_distances(metric="manhattan")
    -> region_hclust(method="single") -> cut_tree.  Single linkage only takes
    minima, so every height has the bits of an input entry; the cut between the
    largest height inside a cluster and the last merge separates the two."""
    import kmer_spans_amd as K
    from kmer_spans_amd import device as D
    rng = np.random.default_rng(40)
    counts = np.zeros((40, 16), dtype=np.uint32)
    member = rng.permutation(40) < 20
    counts[member, :8] = rng.integers(50, 100, size=(20, 8))
    counts[~member, 8:] = rng.integers(50, 100, size=(20, 8))
    counts[:, 7:9] += rng.integers(0, 3, size=(40, 2)).astype(np.uint32)  # a little overlap
    d, _ = D.region_distances(ctx, to_dev(counts), metric="manhattan")
    assert_bits(d.cpu().numpy(), M.condensed_value("manhattan", counts), "pipeline")
    tree, _ = D.region_hclust(ctx, d, method="single")
    height = tree["height"]
    assert np.isin(bits(height), bits(d.cpu().numpy())).all()
    assert (np.diff(height) >= 0).all() and height[-1] > 1.5 > height[-2]
    groups = K.cut_tree(tree, h=0.5 * (height[-2] + height[-1]))
    assert set(groups.tolist()) == {1, 2}
    assert len(set(groups[member].tolist())) == 1 and len(set(groups[~member].tolist())) == 1
    assert np.array_equal(groups, K.cut_tree(tree, k=2))
