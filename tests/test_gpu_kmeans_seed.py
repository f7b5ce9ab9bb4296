"""Maximin and k-means++ starts on the device (ks_spectra_kmeans_seed_dev and
the host entry) against the host model of tests/seedref.py: picked rows,
nearest pick, squared distances, pick distances, potentials, radius and far row
identical in every bit.  Runs on an MI355X (pytest -m gpu)."""
import ctypes as C

import numpy as np
import pytest

from tests import kmeansref as R
from tests import seedref as S
from tests.test_kmeans_seed import (LINE5, assert_same_seed, find_split_u, line_counts, pin_case, planted_groups,
                                    same_partition, separation)
from tests.test_nj import bits
from tests.test_spectra_dist import random_counts

pytestmark = pytest.mark.gpu

METHODS = ("maximin", "kmeans++")


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


def check_seed(ctx, counts, g, method, rows=None, first=0, u=None, what="", dev=None, want=None):
    """device.region_kmeans_seed against the model; the spectra's bits are unchanged."""
    from kmer_spans_amd import device as D
    dev = to_dev(counts) if dev is None else dev
    res, st = D.region_kmeans_seed(ctx, dev, g, method=method, rows=rows, first=first, u=u)
    assert np.array_equal(dev.cpu().numpy().view(np.uint32), np.asarray(counts, dtype=np.uint32)), (what, "spectra")
    hrows = rows.cpu().numpy() if hasattr(rows, "cpu") else rows
    want = S.seed(counts, g, method, rows=hrows, first=first, u=u) if want is None else want
    assert_same_seed(host_of(res), want, what)
    m = want["nearest"].size
    assert st["n_launches"] == 2 * g + 2 and st["panel_bytes"] >= m * counts.shape[1] * 8 and st["work_bytes"] > 0
    return res, st, want


def uniforms(seed, g):
    return np.random.default_rng(seed).random(g)


def both(ctx, counts, g, rows=None, first=0, what="", dev=None):
    dev = to_dev(counts) if dev is None else dev
    m = counts.shape[0] if rows is None else len(rows)
    check_seed(ctx, counts, g, "maximin", rows=rows, first=first, what=f"{what} maximin", dev=dev)
    check_seed(ctx, counts, g, "kmeans++", rows=rows, first=first, u=uniforms(g * 1000 + m, g), what=f"{what} dsq",
               dev=dev)
    check_seed(ctx, counts, g, "kmeans++", rows=rows, first=None, u=uniforms(g * 1000 + m + 1, g),
               what=f"{what} dsq drawn first", dev=dev)


# ------------------------------------------------------------- known answers

def test_line(ctx):
    a, _, _ = check_seed(ctx, LINE5, 3, "maximin", what="line maximin")
    assert a["rows"].cpu().tolist() == [0, 4, 2] and a["pick_dist"].tolist() == [np.inf, 2.0, 0.5]
    assert a["nearest"].cpu().tolist() == [1, 1, 3, 2, 2] and a["far_row"] == 3 and a["radius"] == 0.125
    b, _, _ = check_seed(ctx, LINE5, 3, "kmeans++", first=None, u=[0.5, 0.5, 0.9], what="line dsq")
    assert b["rows"].cpu().tolist() == [2, 1, 4] and b["potential"].tolist() == [np.inf, 45 / 32, 21 / 32]
    assert b["nearest"].cpu().tolist() == [2, 2, 1, 1, 3] and b["potential_final"] == 5 / 32


# -------------------------------------------------------------------- sizes

@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 255, 256, 257, 513, 1025])
def test_sizes(ctx, m):
    counts = random_counts(np.random.default_rng(m), m, 16)
    dev = to_dev(counts)
    for g in (1, 2, 3, 65):
        both(ctx, counts, g, first=m // 3, what=f"m={m} g={g}", dev=dev)


@pytest.mark.parametrize("ncol", [1, 15, 17, 256, 4096])
def test_column_counts(ctx, ncol):
    m = 257
    rng = np.random.default_rng(ncol)
    counts = random_counts(rng, m, ncol) if ncol > 1 else rng.integers(1, 9, size=(m, 1)).astype(np.uint32)
    both(ctx, counts, 4, first=256, what=f"ncol={ncol}")


# -------------------------------------------------------------- chunk seams

SEAMS = [255, 256, 511, 512]  # the last row of chunks 0 and 1, the first of chunks 1 and 2


def test_maximin_picks_on_chunk_seams(ctx):
    """Row 0 is (N, 0, 0, 0, 0), the seam rows are one column each and all other
    rows lie near row 0: the seam rows are at exactly 2 from row 0 and from each
    other, so every pick is a tie between chunks that the lowest position wins."""
    rng = np.random.default_rng(5)
    m = 700
    counts = np.concatenate([np.full((m, 1), 1000), rng.integers(0, 4, size=(m, 4))], axis=1).astype(np.uint32)
    counts[0] = [1000, 0, 0, 0, 0]
    for i, s in enumerate(SEAMS):
        counts[s] = 0
        counts[s, 1 + i] = 7
    want = S.seed(counts, 5, "maximin")
    assert want["rows"].tolist() == [0] + SEAMS and want["pick_dist"][1:].tolist() == [2.0] * 4
    check_seed(ctx, counts, 5, "maximin", what="maximin seams", want=want)


def edge_u(mind, s, upper):
    """The smallest (upper=False) or largest (upper=True) u whose D^2 pick is
    row s: the host search steps u by nextafter around (P[c] + acc) / pot."""
    _, P = S.chunk_prefix(mind)
    c = s // S.CHUNK
    acc = R.sum_in_order(mind[c * S.CHUNK:s + (1 if upper else 0)])
    u = np.float64((P[c] + acc) / P[-1])
    step = -np.inf if upper else np.inf
    for _ in range(64):  # towards the inside of the row's interval
        if 0 <= u < 1 and S.dsq_pick(mind, u)[0] == s:
            break
        u = np.nextafter(u, step)
    assert S.dsq_pick(mind, u)[0] == s
    for _ in range(64):  # back out to the last u that still picks s
        v = np.nextafter(u, -step)
        if not 0 <= v < 1 or S.dsq_pick(mind, v)[0] != s:
            break
        u = v
    other = S.dsq_pick(mind, np.nextafter(u, -step))[0]
    assert other == (s + 1 if upper else s - 1) or mind[other] > 0
    return float(u)


def test_dsq_picks_on_chunk_seams(ctx):
    """u taken from the host search: the last u that still picks the last row
    of a chunk, the first u that picks the first row of the next."""
    m = 700
    counts = random_counts(np.random.default_rng(6), m, 16)
    p = R.profiles(counts)
    mind = R.sqdist(p, p[0:1])[:, 0]
    u = [0.0]
    for s in SEAMS:
        u.append(edge_u(mind, s, upper=s % S.CHUNK == S.CHUNK - 1))
        mind = np.minimum(mind, R.sqdist(p, p[s:s + 1])[:, 0])
    want = S.seed(counts, 5, "kmeans++", u=u)
    assert want["rows"].tolist() == [0] + SEAMS
    check_seed(ctx, counts, 5, "kmeans++", u=u, what="dsq seams", want=want)


# ------------------------------------------------------------------- pins

def test_order_pin(ctx):
    """Forty-one binades of weights: only the chunked prefix gives this
    potential and, for the searched u, this row."""
    counts, weights = pin_case()
    u, by_contract, by_plain, _ = find_split_u(weights)
    res, _, want = check_seed(ctx, counts, 2, "kmeans++", u=[0.0, u], what="order pin")
    plain = S.seed(counts, 2, "kmeans++", u=[0.0, u], chunk=None)
    assert int(res["rows"][1]) == by_contract != by_plain == plain["rows"][1]
    assert bits(res["potential"])[1] != bits(plain["potential"])[1]
    check_seed(ctx, counts, 3, "maximin", what="order pin maximin")


def test_extreme_uniforms(ctx):
    rng = np.random.default_rng(9)
    counts = rng.integers(0, 9, size=(700, 3)).astype(np.uint32)
    counts[counts.sum(axis=1) == 0, 1] = 1
    dev = to_dev(counts)
    for u in ([0.0, 0.0, 0.0], [S.U_MAX, S.U_MAX, S.U_MAX], [0.0, S.U_MAX, 0.0]):
        res, _, _ = check_seed(ctx, counts, 3, "kmeans++", first=None, u=u, what=f"u={u}", dev=dev)
        assert (res["pick_dist"][1:] > 0).all() and int(res["rows"][0]) == (0 if u[0] == 0 else 699)


# ---------------------------------------------------- ties and degenerates

def test_ties_duplicates_identical_rows_and_more_picks_than_rows(ctx):
    base = np.array([[1, 2, 3], [2, 4, 6], [3, 0, 0], [1, 2, 3], [0, 5, 5], [9, 0, 0], [0, 1, 1], [4, 4, 4]],
                    dtype=np.uint32)
    for method, kw in (("maximin", {}), ("kmeans++", {"u": uniforms(1, 8)})):
        res, _, _ = check_seed(ctx, base, 8, method, what=f"duplicates {method}", **kw)
        assert res["n_distinct"] == 4 and res["rows"].cpu().tolist()[4:] == [0, 0, 0, 0]
    same = np.tile(np.array([[2, 4, 6]], dtype=np.uint32), (300, 1)) * np.arange(1, 301, dtype=np.uint32)[:, None]
    for method, kw in (("maximin", {}), ("kmeans++", {"u": [0.3, 0.9, 0.0, 0.5]})):
        res, _, _ = check_seed(ctx, same, 4, method, first=7, what=f"identical {method}", **kw)
        assert res["rows"].cpu().tolist() == [7, 0, 0, 0] and res["n_distinct"] == 1 and res["radius"] == 0.0
    for method, kw in (("maximin", {}), ("kmeans++", {"u": uniforms(2, 7)})):
        res, _, _ = check_seed(ctx, LINE5, 7, method, first=1, what=f"g > m {method}", **kw)
        assert res["n_distinct"] == 5 and res["rows"].cpu().tolist()[5:] == [0, 0]
    tie, _, _ = check_seed(ctx, line_counts([4, 1, 7, 7, 1]), 2, "maximin", what="tie")
    assert tie["rows"].cpu().tolist() == [0, 1] and tie["far_row"] == 2
    m = 600  # many proportional rows: ties in every step, across chunks
    rng = np.random.default_rng(m)
    counts = rng.integers(0, 4, size=(m, 4)).astype(np.uint32)
    counts[counts.sum(axis=1) == 0, 0] = 1
    both(ctx, counts, 40, what="tie heavy")


# -------------------------------------------------------------- selections

def test_selections(ctx):
    """Descending with repeats, as numpy and as a CUDA tensor."""
    import torch
    m = 300
    counts = random_counts(np.random.default_rng(300), m, 16)
    dev = to_dev(counts)
    rows = np.concatenate([np.arange(m - 1, -1, -2), [5, 5, 17, 299, 0, 5]]).astype(np.int64)
    for method, kw in (("maximin", {}), ("kmeans++", {"u": uniforms(3, 9)})):
        _, _, want = check_seed(ctx, counts, 9, method, rows=rows, first=151, what=f"numpy {method}", dev=dev, **kw)
        res, _, _ = check_seed(ctx, counts, 9, method, rows=torch.from_numpy(rows).cuda(), first=151,
                               what=f"cuda {method}", dev=dev, want=want, **kw)
        assert res["mindist"].cpu().numpy()[[150, 151, 155]].tolist() == [0.0, 0.0, 0.0]  # all three are row 5


# ------------------------------------------- against the existing kernels

@pytest.mark.parametrize("m,g", [(130, 7), (600, 65), (1025, 129)])
def test_agrees_with_region_kmeans_and_region_distances(ctx, m, g):
    import torch
    from kmer_spans_amd import device as D
    counts = random_counts(np.random.default_rng(m * g), m, 16)
    dev = to_dev(counts)
    rows = torch.from_numpy(np.random.default_rng(g).permutation(m).astype(np.int64)).cuda()
    for method, kw in (("maximin", {}), ("kmeans++", {"seed": g})):
        res, _ = D.region_kmeans_seed(ctx, dev, g, method=method, rows=rows, **kw)
        km, _ = D.region_kmeans(ctx, dev, res["rows"], rows=rows, iter_max=1)
        assert torch.equal(res["nearest"], km["cluster"]), method
        d, _ = D.region_distances(ctx, dev, rows, rows[res["rows"]], squared=True)
        assert np.array_equal(bits(res["mindist"].cpu().numpy()), bits(d.min(dim=1).values.cpu().numpy())), method


# ------------------------------------------------------- repeats, raw calls

def raw_seed(ctx, sp, m, ncol, g, flags, first, u, rows_out, near, mind, rows=None):
    """ks_spectra_kmeans_seed_dev through ctypes on caller-owned tensors."""
    import torch
    from kmer_spans_amd import _lib
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    pd, pot, res = np.full(g, -3.0), np.full(g, -4.0), _lib.SeedResult()
    res.n_distinct, res.radius = -9, -9.0
    ua = None if u is None else np.ascontiguousarray(u, dtype=np.float64)
    torch.cuda.current_stream().synchronize()
    rc = _lib.load().ks_spectra_kmeans_seed_dev(ctx.handle, ptr(sp), sp.shape[0], ncol, ptr(rows), m, g, flags, first,
                                                None if ua is None else ua.ctypes.data, ptr(rows_out), ptr(near),
                                                ptr(mind), pd.ctypes.data, pot.ctypes.data, C.byref(res), None)
    return rc, _lib.load().ks_last_error().decode(), pd, pot, res


def test_the_same_call_twice_gives_the_same_bits(ctx):
    m, g = 1025, 33
    counts = random_counts(np.random.default_rng(1025), m, 16)
    dev = to_dev(counts)
    for method, kw in (("maximin", {}), ("kmeans++", {"u": uniforms(4, g)})):
        a, _, want = check_seed(ctx, counts, g, method, what=f"first {method}", dev=dev, **kw)
        b, _, _ = check_seed(ctx, counts, g, method, what=f"again {method}", dev=dev, want=want, **kw)
        for k in ("rows", "nearest", "mindist"):
            assert np.array_equal(a[k].cpu().numpy().view(np.uint8), b[k].cpu().numpy().view(np.uint8)), (method, k)


def test_rejected_calls_leave_the_outputs_untouched(ctx):
    import torch
    m, ncol, g = 90, 16, 3
    counts = random_counts(np.random.default_rng(90), m, ncol)
    empty = counts.copy()
    empty[37] = 0
    rows_ok = torch.arange(m, dtype=torch.int64, device="cuda")
    bad_rows = rows_ok.clone()
    bad_rows[[11, 40]] = torch.tensor([m, -1], device="cuda")
    ok_u = [0.1, 0.2, 0.3]
    cases = [("bad index", to_dev(counts), bad_rows, 0, 0, None, "row index 11 out of range"),
             ("empty row", to_dev(empty), rows_ok, 1, -1, ok_u, "row 37 has no counts"),
             ("index before empty row", to_dev(empty), bad_rows, 0, 0, None, "row index 11 out of range"),
             ("bad first", to_dev(counts), rows_ok, 0, m, None, f"first = {m} is not in 0 .. {m - 1}"),
             ("negative first", to_dev(counts), rows_ok, 1, -2, ok_u, f"first = -2 is not in 0 .. {m - 1}"),
             ("bad u", to_dev(counts), rows_ok, 1, 0, [0.1, 1.0, np.nan], "u[1] is not in [0, 1)"),
             ("drawn first with maximin", to_dev(counts), rows_ok, 0, -1, None,
              "first = -1 (a drawn first row) needs KS_SEED_DSQ")]
    for name, sp, rows, flags, first, u, text in cases:
        rows_out = torch.full((g,), -77, dtype=torch.int64, device="cuda")
        near = torch.full((m,), -78, dtype=torch.int32, device="cuda")
        mind = torch.full((m,), -7.5, dtype=torch.float64, device="cuda")
        rc, msg, pd, pot, res = raw_seed(ctx, sp, m, ncol, g, flags, first, u, rows_out, near, mind, rows=rows)
        assert rc != 0 and msg == text, (name, msg)
        assert (rows_out == -77).all() and (near == -78).all() and (mind == -7.5).all(), (name, "an output was written")
        assert (pd == -3.0).all() and (pot == -4.0).all() and res.n_distinct == -9 and res.radius == -9.0, name
        check_seed(ctx, counts, 3, "maximin", what=f"after {name}")
    rows_out = torch.full((g,), -77, dtype=torch.int64, device="cuda")
    near = torch.full((m,), -78, dtype=torch.int32, device="cuda")
    mind = torch.full((m,), -7.5, dtype=torch.float64, device="cuda")
    rc, msg, pd, pot, res = raw_seed(ctx, to_dev(counts), m, ncol, g, 1, -1, ok_u, rows_out, near, mind, rows=rows_ok)
    assert rc == 0, msg
    got = {"rows": rows_out.cpu().numpy(), "nearest": near.cpu().numpy(), "mindist": mind.cpu().numpy(),
           "pick_dist": pd, "potential": pot, "n_distinct": res.n_distinct, "potential_final": res.potential,
           "radius": res.radius, "far_row": res.far_row}
    assert_same_seed(got, S.seed(counts, g, "kmeans++", first=-1, u=ok_u), "raw call")


# ------------------------------------------------------------- host entries

def test_host_entries(ctx):
    import kmer_spans_amd as K
    m = 257
    counts = random_counts(np.random.default_rng(2570), m, 17)
    rows = np.arange(m - 1, -1, -1)
    assert_same_seed(K.region_kmeans_seed(counts, 6, rows=rows, first=256), S.seed(counts, 6, rows=rows, first=256),
                     "host maximin")
    u = uniforms(5, 6)
    assert_same_seed(K.region_kmeans_seed(counts.astype(np.int64), 6, method="kmeans++", u=u, first=None),
                     S.seed(counts, 6, "kmeans++", u=u, first=None), "host dsq, u")
    assert_same_seed(K.region_kmeans_seed(counts, 6, method="kmeans++", seed=12, first=3),
                     S.seed(counts, 6, "kmeans++", u=np.random.default_rng(12).random(6), first=3), "host dsq, seed")
    empty = counts.copy()
    empty[5] = 0
    with pytest.raises(K.KmerSpansError, match="^row 251 has no counts$"):
        K.region_kmeans_seed(empty, 3, rows=rows)


# ------------------------------------------------------------------ pipeline

def test_seed_then_kmeans_recovers_the_planted_groups(ctx):
    from kmer_spans_amd import device as D
    counts, truth = planted_groups()
    between, within = separation(counts, truth)
    assert np.sqrt(between) > 2 * np.sqrt(within)
    dev = to_dev(counts)
    seed, _, want = check_seed(ctx, counts, 5, "maximin", what="planted", dev=dev)
    assert sorted(truth[want["rows"]].tolist()) == [1, 2, 3, 4, 5]
    res, _ = D.region_kmeans(ctx, dev, seed["rows"], iter_max=20)
    assert res["converged"] is True and same_partition(res["cluster"].cpu().numpy(), truth)
    check_seed(ctx, counts, 5, "kmeans++", u=uniforms(6, 5), first=None, what="planted dsq", dev=dev)


# -------------------------------------------------------- scale: invariants

def test_scale_invariants(ctx):
    """m = 8,192, g = 50, ncol = 256: the full model is slow here, so what must
    hold of any result, with the model's pieces."""
    from kmer_spans_amd import device as D
    from tests.test_kmeans import planted_counts
    m, g, ncol = 8192, 50, 256
    counts, _ = planted_counts(np.random.default_rng(8192), m, ncol, g, depth=500)
    dev = to_dev(counts)
    p = R.profiles(counts)
    for method, kw in (("maximin", {}), ("kmeans++", {"seed": 1, "first": None})):
        res, st = D.region_kmeans_seed(ctx, dev, g, method=method, **kw)
        print(f"m = {m} {method}: ms_normalise {st['ms_normalise']:.3f} ms_steps {st['ms_steps']:.3f} launches "
              f"{st['n_launches']} panel {st['panel_bytes']} work {st['work_bytes']}")
        picked = res["rows"].cpu().numpy()
        assert res["n_distinct"] == g and len(set(picked.tolist())) == g
        assert (np.diff(res["potential"][1:]) <= 0).all() and res["potential_final"] <= res["potential"][-1]
        if method == "maximin":
            assert (np.diff(res["pick_dist"][1:]) <= 0).all() and res["radius"] <= res["pick_dist"][-1]
        acc = R.sqdist(p, p[picked])
        mind = res["mindist"].cpu().numpy()
        assert np.array_equal(bits(mind), bits(acc.min(axis=1)))
        assert np.array_equal(res["nearest"].cpu().numpy(), R.assign(acc))
        assert bits([res["potential_final"]])[0] == bits([R.chunked_sum(mind)])[0]
        assert res["radius"] == mind.max() and res["far_row"] == int(np.argmax(mind))
