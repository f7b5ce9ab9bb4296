"""Lloyd k-means and group means on the device (ks_spectra_kmeans_dev /
ks_spectra_group_means_dev and the host entries) against the host model of
tests/kmeansref.py: labels, centres, sizes, withinss, tot_withinss, totss, iter
and converged identical in every bit.  Runs on an MI355X (pytest -m gpu)."""
import ctypes as C

import numpy as np
import pytest

from tests import kmeansref as R
from tests.test_kmeans import LINE, centre_ties, order_pin_case, planted_counts, tie_heavy_case
from tests.test_nj import bits
from tests.test_spectra_dist import random_counts

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


def host_of(res):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in res.items()}


def assert_same_kmeans(got, want, what=""):
    got = host_of(got)
    assert np.array_equal(got["cluster"], want["cluster"]), (what, "cluster",
                                                            int((got["cluster"] != want["cluster"]).sum()))
    assert np.array_equal(got["size"], want["size"]), (what, "size")
    for k in ("centers", "withinss"):
        x, y = bits(got[k]), bits(want[k])
        assert np.array_equal(x, y), (what, k, int((x != y).sum()))
    for k in ("tot_withinss", "totss", "betweenss"):
        assert bits([got[k]])[0] == bits([want[k]])[0], (what, k, got[k], want[k])
    assert (got["iter"], got["converged"]) == (want["iter"], want["converged"]), (what, got["iter"], want["iter"])


def assert_same_means(got, want, what=""):
    got = host_of(got)
    assert np.array_equal(got["size"], want["size"]), (what, "size")
    empty = want["size"] == 0
    assert np.isnan(got["centers"][empty]).all(), (what, "empty groups are NaN rows")
    assert np.array_equal(bits(got["centers"][~empty]), bits(want["centers"][~empty])), (what, "centers")
    assert np.array_equal(bits(got["withinss"]), bits(want["withinss"])), (what, "withinss")


def check_kmeans(ctx, counts, centers, rows=None, iter_max=10, what="", dev=None, want=None):
    """device.region_kmeans against the model; the spectra's bits are unchanged."""
    from kmer_spans_amd import device as D
    dev = to_dev(counts) if dev is None else dev
    res, st = D.region_kmeans(ctx, dev, centers, rows=rows, iter_max=iter_max)
    assert np.array_equal(dev.cpu().numpy().view(np.uint32), np.asarray(counts, dtype=np.uint32)), (what, "spectra")
    hrows = rows.cpu().numpy() if hasattr(rows, "cpu") else rows
    hcen = centers.cpu().numpy() if hasattr(centers, "cpu") else centers
    want = R.kmeans(counts, hcen, rows=hrows, iter_max=iter_max) if want is None else want
    assert_same_kmeans(res, want, what)
    assert st["n_iter"] == want["iter"] and st["panel_bytes"] >= want["cluster"].size * counts.shape[1] * 8
    assert st["work_bytes"] > 0
    return res, st, want


def spread_rows(m: int, g: int) -> np.ndarray:
    """g positions spread over 0 .. m - 1 (they repeat when g > m)."""
    return (np.arange(g, dtype=np.int64) * max(m // g, 1)) % m


# ------------------------------------------------------------- known answers

def test_line(ctx):
    import kmer_spans_amd as K
    res, _, _ = check_kmeans(ctx, LINE, np.array([0, 1]), what="line")
    assert res["cluster"].cpu().tolist() == [1, 1, 2, 2] and res["iter"] == 3 and res["converged"] is True
    assert res["centers"].cpu().tolist() == [[0.0625, 0.9375], [0.875, 0.125]]
    assert res["withinss"].tolist() == [0.015625, 0.0625] and res["totss"] == 1.3984375
    host = K.region_kmeans(LINE, [0, 1])  # api -> host entry
    assert_same_kmeans(host, R.kmeans(LINE, [0, 1]), "host entry")
    gm = K.region_group_means(LINE, [1, 1, 2, 2])
    assert gm["centers"].tolist() == [[0.0625, 0.9375], [0.875, 0.125]] and gm["withinss"].tolist() == [0.015625, 0.0625]


# ---------------------------------- sizes across tile, LDS chunk and sum chunk

@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 255, 256, 257, 513, 1025])
def test_sizes(ctx, m):
    """The tile edge (64 rows, 64 centres) and the sum chunk (256) with one
    either side; g > m where m is small.  Row starts and matrix starts."""
    counts = random_counts(np.random.default_rng(m), m, 16)
    dev = to_dev(counts)
    p = R.profiles(counts)
    for g in (1, 2, 63, 64, 65, 129):
        start = spread_rows(m, g)
        check_kmeans(ctx, counts, start, iter_max=3, what=f"m={m} g={g} rows", dev=dev)
        if g in (2, 65):
            init = p[start] * 0.75 + 0.25 / 16  # not any row's profile
            check_kmeans(ctx, counts, init, iter_max=4, what=f"m={m} g={g} matrix", dev=dev)


@pytest.mark.parametrize("m,g,ncol", [(65, 3, 1), (257, 5, 1), (65, 3, 15), (513, 65, 15), (65, 3, 17), (513, 64, 17),
                                      (257, 5, 256), (1025, 129, 256), (65, 3, 4096)])
def test_column_counts(ctx, m, g, ncol):
    """One column, one either side of the 16-column LDS chunk, the flagship 256, and the largest ncol."""
    counts = random_counts(np.random.default_rng(ncol + m), m, ncol)
    check_kmeans(ctx, counts, spread_rows(m, g), iter_max=3, what=f"m={m} g={g} ncol={ncol}")
    group = (np.arange(m) % g + 1).astype(np.int32)
    check_means(ctx, counts, group, g, what=f"means m={m} g={g} ncol={ncol}")


def check_means(ctx, counts, group, ngroups=None, rows=None, what="", dev=None):
    from kmer_spans_amd import device as D
    dev = to_dev(counts) if dev is None else dev
    res, st = D.region_group_means(ctx, dev, group, ngroups=ngroups, rows=rows)
    want = R.group_means(counts, group, ngroups, rows=rows)
    assert_same_means(res, want, what)
    assert st["work_bytes"] > 0
    return res, st, want


def test_groups_of_exactly_256_257_and_513(ctx):
    """Contiguous and interleaved members; k-means started from these groups' means keeps the sizes' chunks."""
    m = 256 + 257 + 513
    rng = np.random.default_rng(1026)
    counts, _ = planted_counts(rng, m, 16, 3)
    dev = to_dev(counts)
    contiguous = np.repeat([1, 2, 3], [256, 257, 513]).astype(np.int32)
    for name, group in (("contiguous", contiguous), ("interleaved", contiguous[rng.permutation(m)])):
        res, _, want = check_means(ctx, counts, group, 3, what=name, dev=dev)
        assert want["size"].tolist() == [256, 257, 513]
        check_kmeans(ctx, counts, res["centers"], iter_max=2, what=f"k-means from {name}", dev=dev)


# ------------------------------------------- against an existing kernel

@pytest.mark.parametrize("m,g", [(130, 7), (600, 65), (1025, 129)])
def test_assignment_equals_first_minimum_of_region_distances(ctx, m, g):
    """iter_max = 1 from init_rows: the labels are the first-minimum argmin of
    the squared cross distances of the existing kernel, downloaded."""
    import torch
    from kmer_spans_amd import device as D
    counts = random_counts(np.random.default_rng(m * g), m, 16)
    dev = to_dev(counts)
    rows = torch.from_numpy(np.random.default_rng(g).permutation(m).astype(np.int64)).cuda()
    start = spread_rows(m, g)
    rows_b = rows[torch.from_numpy(start).cuda()]
    d, _ = D.region_distances(ctx, dev, rows, rows_b, squared=True)
    res, _ = D.region_kmeans(ctx, dev, start, rows=rows, iter_max=1)
    assert np.array_equal(res["cluster"].cpu().numpy(), np.argmin(d.cpu().numpy(), axis=1) + 1)
    assert res["converged"] is False and res["iter"] == 1


# ------------------------------------------------------------------- pins

def test_order_pin(ctx):
    """Forty binades and a group of 600: only the chunked order gives these bits."""
    counts, group = order_pin_case()
    res, _, _ = check_means(ctx, counts, group, 2, what="order pin")
    p = R.profiles(counts)
    plain = R.update(p, group, np.zeros((2, p.shape[1])), chunk=None)
    assert (bits(res["centers"].cpu().numpy()[0]) != bits(plain[0])).sum() >= p.shape[1] // 4
    check_kmeans(ctx, counts, res["centers"], iter_max=2, what="order pin, k-means")


def test_tie_cases(ctx):
    counts = np.array([[4, 0], [0, 4], [2, 2]], dtype=np.uint32)
    res, _, _ = check_kmeans(ctx, counts, np.array([0, 1]), iter_max=1, what="equidistant")
    assert res["cluster"].cpu().tolist() == [1, 2, 1]
    res, _, _ = check_kmeans(ctx, counts, np.array([1, 0]), iter_max=1, what="equidistant, swapped")
    assert res["cluster"].cpu().tolist() == [2, 1, 1]
    rng = np.random.default_rng(3)
    counts = rng.integers(1, 30, size=(50, 5)).astype(np.uint32)
    res, _, _ = check_kmeans(ctx, counts, np.array([7, 7, 20]), iter_max=1, what="duplicate centres")
    assert res["size"][1] == 0 and bits(res["withinss"])[1] == 0
    assert np.array_equal(bits(res["centers"].cpu().numpy()[1]), bits(R.profiles(counts)[7]))
    check_kmeans(ctx, counts, np.array([7, 7, 20]), iter_max=50, what="duplicate centres, to the end")
    counts = np.array([[9, 1], [8, 2], [1, 9], [2, 8]], dtype=np.uint32)
    far = np.array([[0.9, 0.1], [0.1, 0.9], [5.0, -4.0]])
    res, _, _ = check_kmeans(ctx, counts, far, what="a centre nobody is nearest to")
    assert res["size"].tolist() == [2, 2, 0] and res["iter"] == 2 and res["converged"] is True
    assert np.array_equal(bits(res["centers"].cpu().numpy()[2]), bits(far[2])) and bits(res["withinss"])[2] == 0


@pytest.mark.parametrize("m", [130, 600])
def test_tie_heavy(ctx, m):
    counts, start = tie_heavy_case(m)
    n = centre_ties(counts, start)
    print(f"m = {m}: {n} rows at equal distance from two or more centres")
    assert n > 0
    check_kmeans(ctx, counts, start, iter_max=1, what=f"ties m={m}, one pass")
    check_kmeans(ctx, counts, start, iter_max=30, what=f"ties m={m}")


def test_proportional_rows(ctx):
    counts = np.array([[1, 2, 3], [2, 4, 6], [50, 100, 150], [9, 1, 1], [18, 2, 2]], dtype=np.uint32)
    res, _, _ = check_kmeans(ctx, counts, np.array([0, 3]), what="proportional")
    assert res["cluster"].cpu().tolist() == [1, 1, 1, 2, 2] and not res["withinss"].any()
    assert res["tot_withinss"] == 0.0 and res["converged"] is True


def test_one_group_and_more_groups_than_rows(ctx):
    counts = np.random.default_rng(13).integers(1, 90, size=(600, 6)).astype(np.uint32)
    res, _, _ = check_kmeans(ctx, counts, np.array([5]), what="g = 1")
    assert bits([res["tot_withinss"]])[0] == bits([res["totss"]])[0] and res["iter"] == 2
    res, _, _ = check_kmeans(ctx, counts[:3], np.array([0, 1, 2, 0, 1]), iter_max=5, what="g > m")
    assert res["size"].tolist() == [1, 1, 1, 0, 0]


# -------------------------------------------------------------- selections

def test_selections(ctx):
    """Descending with repeats; a CUDA and a numpy selection; init_rows naming a repeated row."""
    import torch
    m = 300
    counts = random_counts(np.random.default_rng(300), m, 16)
    dev = to_dev(counts)
    rows = np.concatenate([np.arange(m - 1, -1, -2), [5, 5, 17, 299, 0, 5]]).astype(np.int64)
    start = np.array([0, rows.size - 1, rows.size - 5, 40], dtype=np.int64)  # positions 155 and 150 are both row 5
    assert rows[start[1]] == rows[start[2]] == 5
    _, _, want = check_kmeans(ctx, counts, start, rows=rows, iter_max=6, what="numpy selection", dev=dev)
    check_kmeans(ctx, counts, torch.from_numpy(start).cuda(), rows=torch.from_numpy(rows).cuda(), iter_max=6,
                 what="cuda selection", dev=dev, want=want)
    group = (np.arange(rows.size) % 4 + 1).astype(np.int32)
    check_means(ctx, counts, group, 4, rows=rows, what="means of a selection", dev=dev)


# --------------------------------------------------------------- loop state

def test_iter_max_one_two_and_to_convergence(ctx):
    counts, _ = planted_counts(np.random.default_rng(77), 700, 16, 5, depth=300)
    dev = to_dev(counts)
    start = np.arange(5) * 3
    one, _, w1 = check_kmeans(ctx, counts, start, iter_max=1, what="iter_max 1", dev=dev)
    assert one["converged"] is False
    assert np.array_equal(w1["cluster"], R.assign(R.sqdist(R.profiles(counts), R.profiles(counts)[start])))
    check_kmeans(ctx, counts, start, iter_max=2, what="iter_max 2", dev=dev)
    full, st, _ = check_kmeans(ctx, counts, start, iter_max=100, what="to convergence", dev=dev)
    assert full["converged"] is True and full["iter"] >= 3
    print(f"converged after {full['iter']} passes; ms_assign {st['ms_assign']:.3f} ms_update {st['ms_update']:.3f}")


def test_a_group_empty_from_the_first_pass_on(ctx):
    counts, _ = planted_counts(np.random.default_rng(4), 400, 16, 3)
    p = R.profiles(counts)
    init = np.vstack([p[[0, 1, 2]], np.full((1, 16), 7.0)])
    res, _, _ = check_kmeans(ctx, counts, init, iter_max=20, what="empty from the start")
    assert res["size"][3] == 0 and np.array_equal(bits(res["centers"].cpu().numpy()[3]), bits(init[3]))


# ---------------------------------------------------- repeats, aliasing, raw

def raw_kmeans(ctx, sp, m, ncol, g, cluster, cen, init=None, init_rows=None, rows=None, iter_max=3):
    """ks_spectra_kmeans_dev through ctypes on caller-owned tensors."""
    import torch
    from kmer_spans_amd import _lib
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    size, wss, res = np.zeros(g, dtype=np.int32), np.zeros(g), _lib.KmeansResult()
    torch.cuda.current_stream().synchronize()
    rc = _lib.load().ks_spectra_kmeans_dev(ctx.handle, ptr(sp), sp.shape[0], ncol, ptr(rows), m, ptr(init),
                                           ptr(init_rows), g, iter_max, 0, ptr(cluster), ptr(cen), size.ctypes.data,
                                           wss.ctypes.data, C.byref(res), None)
    return rc, _lib.load().ks_last_error().decode(), size, wss, res


def test_repeat_and_alias(ctx):
    """The same call twice gives the same bits; centers_dev may be init_dev."""
    import torch
    m, ncol, g = 513, 16, 7
    counts = random_counts(np.random.default_rng(513), m, ncol)
    dev = to_dev(counts)
    init = R.profiles(counts)[spread_rows(m, g)] * 0.5 + 0.5 / ncol
    first, _, want = check_kmeans(ctx, counts, init, iter_max=4, what="first", dev=dev)
    t_init = torch.from_numpy(init).cuda()
    again, _, _ = check_kmeans(ctx, counts, t_init, iter_max=4, what="again", dev=dev, want=want)
    assert np.array_equal(bits(t_init.cpu().numpy()), bits(init)), "the caller's centres changed"
    assert np.array_equal(bits(again["centers"].cpu().numpy()), bits(first["centers"].cpu().numpy()))
    cluster = torch.zeros(m, dtype=torch.int32, device="cuda")
    rc, msg, size, wss, res = raw_kmeans(ctx, dev, m, ncol, g, cluster, t_init, init=t_init, iter_max=4)
    assert rc == 0, msg
    got = {"cluster": cluster, "centers": t_init, "size": size, "withinss": wss, "tot_withinss": res.tot_withinss,
           "totss": res.totss, "betweenss": res.totss - res.tot_withinss, "iter": res.iter,
           "converged": bool(res.converged)}
    assert_same_kmeans(got, want, "aliased")


def test_rejected_calls_leave_the_outputs_untouched(ctx):
    import torch
    m, ncol, g = 90, 16, 3
    counts = random_counts(np.random.default_rng(90), m, ncol)
    empty = counts.copy()
    empty[37] = 0
    good_init = torch.from_numpy(R.profiles(counts)[[0, 1, 2]]).cuda()
    rows_ok = torch.arange(m, dtype=torch.int64, device="cuda")
    bad_rows = rows_ok.clone()
    bad_rows[[11, 40]] = torch.tensor([m, -1], device="cuda")
    cases = [("bad index", to_dev(counts), bad_rows, good_init, None, "row index 11 out of range"),
             ("empty row", to_dev(empty), rows_ok, good_init, None, "row 37 has no counts"),
             ("index before empty row", to_dev(empty), bad_rows, good_init, None, "row index 11 out of range"),
             ("bad initial row", to_dev(counts), rows_ok, None,
              torch.tensor([0, m, -1], dtype=torch.int64, device="cuda"), "initial row index 1 out of range")]
    for bad in (np.nan, np.inf, -np.inf):
        init = good_init.clone()
        init[1, 5] = bad
        init[2, 0] = float("nan")
        cases.append((f"centre {bad}", to_dev(counts), rows_ok, init, None, "center[1][5] is not finite"))
    for name, sp, rows, init, init_rows, text in cases:
        cluster = torch.full((m,), -77, dtype=torch.int32, device="cuda")
        cen = torch.full((g, ncol), -7.5, dtype=torch.float64, device="cuda")
        rc, msg, size, wss, _ = raw_kmeans(ctx, sp, m, ncol, g, cluster, cen, init=init, init_rows=init_rows, rows=rows)
        assert rc != 0 and msg == text, (name, msg)
        assert (cluster == -77).all() and (cen == -7.5).all(), (name, "an output was written")
        check_kmeans(ctx, counts, np.array([0, 1, 2]), iter_max=2, what=f"after {name}")
    from kmer_spans_amd import device as D
    import kmer_spans_amd as K
    with pytest.raises(K.KmerSpansError, match="^row 37 has no counts$"):
        D.region_group_means(ctx, to_dev(empty), np.ones(m, dtype=np.int32))
    check_means(ctx, counts, (np.arange(m) % 3 + 1).astype(np.int32), 3, what="after a rejected group means")


# ------------------------------------------------------------- group means

@pytest.mark.parametrize("n", [2, 64, 65, 257, 1025])
def test_group_means_of_the_silhouette_labellings(ctx, n):
    from tests.test_gpu_silhouette import labellings
    counts = random_counts(np.random.default_rng(n), n, 16)
    dev = to_dev(counts)
    for name, group, g in labellings(n):
        check_means(ctx, counts, group.astype(np.int32), g, what=f"n={n} {name}", dev=dev)


def test_empty_groups_are_nan_rows_and_no_start_for_kmeans(ctx):
    import kmer_spans_amd as K
    from kmer_spans_amd import device as D
    n = 257
    counts = random_counts(np.random.default_rng(257), n, 16)
    group = np.array([1, 3, 6])[np.random.default_rng(1).integers(0, 3, size=n)].astype(np.int32)
    res, _, want = check_means(ctx, counts, group, 8, what="labels 1 3 6 of 8")
    assert want["size"][[1, 3, 4, 6, 7]].tolist() == [0] * 5 and not res["withinss"][[1, 3, 4, 6, 7]].any()
    with pytest.raises(K.KmerSpansError, match="^center\\[1\\]\\[0\\] is not finite$"):
        D.region_kmeans(ctx, to_dev(counts), res["centers"])
    import torch
    as_tensor, _ = D.region_group_means(ctx, to_dev(counts), torch.from_numpy(group).cuda(), ngroups=8)
    assert_same_means(as_tensor, want, "labels from a tensor")


def test_host_entries(ctx):
    import kmer_spans_amd as K
    m = 257
    counts = random_counts(np.random.default_rng(2570), m, 17)
    rows = np.arange(m - 1, -1, -1)
    start = spread_rows(m, 6)
    assert_same_kmeans(K.region_kmeans(counts, start, rows=rows, iter_max=5),
                       R.kmeans(counts, start, rows=rows, iter_max=5), "host, rows")
    init = R.profiles(counts)[start] * 0.5 + 0.5 / 17
    assert_same_kmeans(K.region_kmeans(counts.astype(np.int64), init), R.kmeans(counts, init), "host, matrix")
    group = np.array([1, 2, 5])[np.arange(m) % 3].astype(np.int32)
    assert_same_means(K.region_group_means(counts, group, ngroups=6, rows=rows),
                      R.group_means(counts, group, 6, rows=rows), "host means")


# ------------------------------------------------------------------ pipeline

def test_pipeline_scan_spectra_distances_hclust_cut_means_kmeans(ctx):
    """The planted-repeat scan of the silhouette chain test, then spectra,
    distances, the complete-linkage tree, cut_tree(k=), region_group_means and
    region_kmeans started from the cut's means: Lloyd passes only lower the
    within sum of squares (up to the rounding of the sums)."""
    import torch
    import kmer_spans_amd as K
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
    m = pos.shape[1]
    assert m >= 4
    sp, _, _ = D.region_spectra(ctx, ds, pos, q=4, both_strands=True, entropy=False)
    dist, _ = D.region_distances(ctx, sp)
    tree, _ = D.region_hclust(ctx, dist)
    ng = min(3, m - 1)
    group = K.cut_tree(tree, k=ng)
    means, _ = D.region_group_means(ctx, sp, group)
    assert means["size"].sum() == m and (means["size"] > 0).all()
    res, st = D.region_kmeans(ctx, sp, means["centers"], iter_max=20)
    ncol = sp.shape[1]
    cut_wss = float(R.sum_in_order(means["withinss"]))
    assert res["size"].sum() == m
    assert res["tot_withinss"] <= cut_wss + 64 * ncol * 2.0 ** -53 * res["totss"]
    host_counts = sp.cpu().numpy().view(np.uint32)
    assert_same_means(means, R.group_means(host_counts, group), "pipeline means")
    assert_same_kmeans(res, R.kmeans(host_counts, means["centers"].cpu().numpy(), iter_max=20), "pipeline k-means")
    print(f"{m} regions, {ng} groups: cut withinss {cut_wss:.6g} -> k-means {res['tot_withinss']:.6g} in "
          f"{res['iter']} passes")


# -------------------------------------------------------- scale: invariants

def test_scale_invariants(ctx):
    """m = 8,192, g = 50, ncol = 256, iter_max = 5: the full model is slow
    here, so what must hold of any result, with the model's pieces."""
    from kmer_spans_amd import device as D
    m, g, ncol = 8192, 50, 256
    counts, _ = planted_counts(np.random.default_rng(8192), m, ncol, g, depth=500)
    dev = to_dev(counts)
    start = spread_rows(m, g)
    prev, _ = D.region_kmeans(ctx, dev, start, iter_max=4)
    res, st = D.region_kmeans(ctx, dev, start, iter_max=5)
    print(f"m = {m}: ms_normalise {st['ms_normalise']:.3f} ms_assign {st['ms_assign']:.3f} ms_update "
          f"{st['ms_update']:.3f} ms_wss {st['ms_wss']:.3f} iter {res['iter']} converged {res['converged']} "
          f"panel {st['panel_bytes']} work {st['work_bytes']}")
    label, cen = res["cluster"].cpu().numpy(), res["centers"].cpu().numpy()
    assert label.min() >= 1 and label.max() <= g
    assert np.array_equal(res["size"], np.bincount(label, minlength=g + 1)[1:])
    p = R.profiles(counts)
    if res["converged"]:
        assert np.array_equal(label, R.assign(R.sqdist(p, cen)))
    else:  # the centres are the chunked means of the returned (last pass's) labels
        assert np.array_equal(bits(cen), bits(R.update(p, label, prev["centers"].cpu().numpy())))
        assert np.array_equal(label, R.assign(R.sqdist(p, prev["centers"].cpu().numpy())))
    assert np.array_equal(bits(res["withinss"]), bits(R.withinss(p, label, cen)))
    assert res["tot_withinss"] <= res["totss"] and bits([res["totss"]])[0] == bits([R.totss(p)])[0]
    assert st["work_bytes"] < st["panel_bytes"]
