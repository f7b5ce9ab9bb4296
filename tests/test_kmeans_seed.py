"""Maximin and k-means++ starts for region_kmeans (ks_spectra_kmeans_seed,
include/kmer_spans.h): the host model of tests/seedref.py against answers worked
by hand, against the plain nested loops of the header, its invariants, the pin
of the chunked prefix order, the edge cases, and the argument checks of both
entries and the wrappers, which happen before any device use -- this file runs
without a GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from kmer_spans_amd import _lib
from tests import kmeansref as R
from tests import seedref as S
from tests.test_nj import bits

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kmer_spans.h")
INF = np.inf


# ------------------------------------------------------------------- inputs

def line_counts(x, total=8):
    """Points x on a line as two-column counts (x, total - x): the squared
    distance of two rows is 2 ((x - y) / total)^2, exact for small integers."""
    x = np.asarray(x, dtype=np.uint32)
    return np.stack([x, total - x], axis=1).astype(np.uint32)


LINE5 = line_counts([0, 1, 4, 6, 8])  # squared distances (x - y)^2 / 32


def pin_case(m=700):
    """m rows (a, T - a), T = 3 * 2^29, with row 0 = (0, T): against row 0 the
    squared distance is about 2 (a / T)^2 with a full mantissa (a / T is not
    exact), and a = floor(2^e (1 + r)) with e uniform in 0 .. 20.5, so the
    weights of the first D^2 draw span 41 binades: their sums round differently
    wherever they are cut.  Returns (counts, the weights = mind after picking row 0)."""
    rng = np.random.default_rng(4100)
    e = rng.random(m) * 20.5
    a = np.floor(np.exp2(e) * (1.0 + rng.random(m)) / 2.0 + 1.0).astype(np.int64)
    a[0] = 0
    T = 3 << 29
    counts = np.stack([a, T - a], axis=1).astype(np.uint32)
    p = R.profiles(counts)
    return counts, R.sqdist(p, p[0:1])[:, 0]


def find_split_u(mind, span=8):
    """The host search of the order pin: a u for which the chunked prefix (the
    contract) and the plain left-to-right prefix pick different rows.  For every
    row s the value (P[c] + acc_s) / pot, where the test P[c] + acc_s > t flips,
    is stepped by nextafter `span` doubles each way.  Returns (u, row by the
    contract, row by the plain order, boundaries tried)."""
    mind = np.asarray(mind, dtype=np.float64)
    _, P = S.chunk_prefix(mind)
    pot = P[-1]
    for s in range(S.CHUNK, mind.size):  # from the second chunk on: there the prefix itself is cut differently
        if mind[s] == 0.0:
            continue
        c = s // S.CHUNK
        acc = R.sum_in_order(mind[c * S.CHUNK:s + 1])
        u0 = np.float64((P[c] + acc) / pot)
        cands, lo, hi = [u0], u0, u0
        for _ in range(span):
            lo, hi = np.nextafter(lo, -INF), np.nextafter(hi, INF)
            cands += [lo, hi]
        for v in cands:
            if 0.0 <= v < 1.0:
                a, b = S.dsq_pick(mind, v)[0], S.dsq_pick(mind, v, None)[0]
                if a != b:
                    return float(v), a, b, s
    return None


def planted_groups(m=1025, ncol=16, g=5, depth=20000, seed=77):
    """g Dirichlet base spectra, every row a multinomial draw of `depth` counts
    from one of them; returns (counts, planted labels 1 .. g)."""
    rng = np.random.default_rng(seed)
    base = rng.dirichlet(np.ones(ncol), size=g)
    truth = np.arange(m) % g
    rng.shuffle(truth)
    counts = np.stack([rng.multinomial(depth, base[j]) for j in truth]).astype(np.uint32)
    return counts, (truth + 1).astype(np.int32)


def separation(counts, truth):
    """(smallest squared distance between rows of different groups, largest
    squared distance between rows of one group)."""
    p = R.profiles(counts)
    acc = R.sqdist(p, p)
    same = truth[:, None] == truth[None, :]
    return float(acc[~same].min()), float(acc[same].max())


def same_partition(a, b) -> bool:
    a, b = np.asarray(a), np.asarray(b)
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len(set(a.tolist())) == len(set(b.tolist()))


def assert_same_seed(got, want, what=""):
    for k in ("rows", "nearest"):
        assert np.array_equal(np.asarray(got[k]), want[k]), (what, k, np.asarray(got[k])[:8], want[k][:8])
    for k in ("mindist", "pick_dist", "potential"):
        assert np.array_equal(bits(np.asarray(got[k])), bits(want[k])), (what, k)
    for k in ("potential_final", "radius"):
        assert bits(np.float64(got[k])) == bits(np.float64(want[k])), (what, k, got[k], want[k])
    for k in ("n_distinct", "far_row"):
        assert int(got[k]) == int(want[k]), (what, k, got[k], want[k])


# ------------------------------------------------------------- known answers

def test_five_points_on_a_line():
    """x = 0, 1, 4, 6, 8 as counts (x, 8 - x): acc(s, r) = (x_s - x_r)^2 / 32.

    Maximin, g = 3, first = 0.
      step 0 picks 0.  mind = [0, 1, 16, 36, 64] / 32, near = [1, 1, 1, 1, 1].
      step 1: the largest mind is 64/32 at position 4.  pick_dist = 2,
        potential = 117/32.  Distances to x = 8: [64, 49, 16, 4, 0] / 32, so
        mind = [0, 1, 16, 4, 0] / 32; position 2 is at 16/32 from both picks and
        keeps label 1: near = [1, 1, 1, 2, 2].
      step 2: the largest mind is 16/32 at position 2.  pick_dist = 1/2,
        potential = 21/32.  Distances to x = 4: [16, 9, 0, 4, 16] / 32, so
        mind = [0, 1, 0, 4, 0] / 32; position 3 is at 4/32 from picks 2 and 3
        and keeps label 2: near = [1, 1, 3, 2, 2].
      Result: potential 5/32, radius 4/32 at far_row 3, n_distinct 3.

    k-means++, g = 3, first = -1, u = [0.5, 0.5, 0.9].
      step 0 picks int(0.5 * 5) = 2.  mind = [16, 9, 0, 4, 16] / 32, near all 1.
      step 1: pot = 45/32, t = 22.5/32; the running sums 16, 25 pass t at
        position 1.  pick_dist = 9/32.  Distances to x = 1: [1, 0, 9, 25, 49] / 32:
        mind = [1, 0, 0, 4, 16] / 32, near = [2, 2, 1, 1, 1].
      step 2: pot = 21/32, t = 18.9/32; the running sums 1, 1, 1, 5, 21 pass t at
        position 4.  pick_dist = 16/32.  Distances to x = 8: [64, 49, 16, 4, 0] / 32:
        mind = [1, 0, 0, 4, 0] / 32; position 3 is at 4/32 from picks 1 and 3 and
        keeps label 1: near = [2, 2, 1, 1, 3].
      Result: potential 5/32, radius 4/32 at far_row 3, n_distinct 3."""
    a = S.seed(LINE5, 3, "maximin", first=0)
    assert a["rows"].tolist() == [0, 4, 2]
    assert a["pick_dist"].tolist() == [INF, 2.0, 0.5]
    assert a["potential"].tolist() == [INF, 117 / 32, 21 / 32]
    assert a["nearest"].tolist() == [1, 1, 3, 2, 2]
    assert a["mindist"].tolist() == [0.0, 1 / 32, 0.0, 4 / 32, 0.0]
    assert (a["potential_final"], a["radius"], a["far_row"], a["n_distinct"]) == (5 / 32, 4 / 32, 3, 3)
    b = S.seed(LINE5, 3, "kmeans++", first=-1, u=[0.5, 0.5, 0.9])
    assert b["rows"].tolist() == [2, 1, 4]
    assert b["pick_dist"].tolist() == [INF, 9 / 32, 16 / 32]
    assert b["potential"].tolist() == [INF, 45 / 32, 21 / 32]
    assert b["nearest"].tolist() == [2, 2, 1, 1, 3]
    assert b["mindist"].tolist() == [1 / 32, 0.0, 0.0, 4 / 32, 0.0]
    assert (b["potential_final"], b["radius"], b["far_row"], b["n_distinct"]) == (5 / 32, 4 / 32, 3, 3)


def plain_seed(counts, g, dsq, first, u):
    """The header in nested Python loops on Python floats (IEEE doubles, one rounding per operation)."""
    counts = [[int(v) for v in row] for row in counts]
    m, ncol = len(counts), len(counts[0])
    p = [[float(v) / float(sum(row)) for v in row] for row in counts]
    mind, near = [INF] * m, [0] * m
    picked, pick_dist, potential = [], [INF] * g, [INF] * g

    def prefix():
        Cs = []
        for t0 in range(0, m, 256):
            acc = 0.0
            for s in range(t0, min(t0 + 256, m)):
                acc = acc + mind[s]
            Cs.append(acc)
        P = [0.0]
        for c in Cs:
            P.append(P[-1] + c)
        return P

    if first == -1:
        first = int(u[0] * float(m))
    for j in range(g):
        if j == 0:
            r = first
        else:
            P = prefix()
            pot = P[-1]
            if dsq:
                r = 0
                if pot != 0.0:
                    t = u[j] * pot
                    c = 0
                    while not P[c + 1] > t:
                        c += 1
                    acc, r = 0.0, None
                    for s in range(c * 256, min(c * 256 + 256, m)):
                        acc = acc + mind[s]
                        if P[c] + acc > t:
                            r = s
                            break
                    assert r is not None
            else:
                r = 0
                for s in range(m):
                    if mind[s] > mind[r]:
                        r = s
            pick_dist[j], potential[j] = mind[r], pot
        picked.append(r)
        for s in range(m):
            acc = 0.0
            for c in range(ncol):
                d = p[s][c] - p[r][c]
                acc = acc + d * d
            if acc < mind[s]:
                mind[s], near[s] = acc, j + 1
    far = 0
    for s in range(m):
        if mind[s] > mind[far]:
            far = s
    return {"rows": np.array(picked, dtype=np.int64), "nearest": np.array(near, dtype=np.int32),
            "mindist": np.array(mind), "pick_dist": np.array(pick_dist), "potential": np.array(potential),
            "n_distinct": 1 + sum(1 for v in pick_dist[1:] if v > 0), "potential_final": prefix()[-1],
            "radius": mind[far], "far_row": far}


@pytest.mark.parametrize("m,ncol,g", [(5, 2, 3), (257, 3, 4), (600, 5, 6), (40, 4, 60)])
def test_model_is_the_plain_loops(m, ncol, g):
    rng = np.random.default_rng(m * 31 + g)
    counts = rng.integers(0, 50, size=(m, ncol)).astype(np.uint32)
    counts[counts.sum(axis=1) == 0, 0] = 1
    u = rng.random(g)
    assert_same_seed(S.seed(counts, g, "maximin", first=m // 2), plain_seed(counts, g, False, m // 2, None), "maximin")
    for first in (-1, m - 1):
        assert_same_seed(S.seed(counts, g, "kmeans++", first=first, u=u), plain_seed(counts, g, True, first, u.tolist()),
                         f"dsq first={first}")


# ---------------------------------------------------------------- invariants

def test_maximin_invariants():
    rng = np.random.default_rng(3)
    counts = rng.integers(0, 200, size=(1025, 16)).astype(np.uint32)
    g = 24
    a = S.seed(counts, g, "maximin")
    assert (np.diff(a["pick_dist"][1:]) <= 0).all()
    assert a["radius"] <= a["pick_dist"][g - 1]
    assert (np.diff(a["potential"][1:]) <= 0).all() and a["potential_final"] <= a["potential"][g - 1]
    b = S.seed(counts, g, "kmeans++", u=rng.random(g), first=None)
    assert (np.diff(b["potential"][1:]) <= 0).all() and b["potential_final"] <= b["potential"][g - 1]
    for r in (a, b):
        assert r["n_distinct"] == g and len(set(r["rows"].tolist())) == g
        assert (r["mindist"][r["rows"]] == 0).all()
        assert (r["nearest"][r["rows"]] == np.arange(1, g + 1)).all()  # distinct profiles: a pick is its own nearest


def test_order_pin_chunked_prefix_differs_from_left_to_right():
    """The potential and the D^2 pick depend on where the sum is cut: the
    chunked order of the contract and the plain left-to-right order give
    different bits, and for a searched u a different row."""
    counts, weights = pin_case()
    m = counts.shape[0]
    first = S.seed(counts, 1, "kmeans++", first=0, u=[0.0])
    assert np.array_equal(bits(first["mindist"]), bits(weights))
    e = np.frexp(weights[1:])[1]
    assert e.max() - e.min() >= 40
    assert bits(first["potential_final"]) != bits(R.chunked_sum(weights, None))
    found = find_split_u(weights)
    assert found is not None
    u, by_contract, by_plain, _ = found
    assert by_contract != by_plain
    a = S.seed(counts, 2, "kmeans++", first=0, u=[0.0, u])
    b = S.seed(counts, 2, "kmeans++", first=0, u=[0.0, u], chunk=None)
    assert a["rows"][1] == by_contract and b["rows"][1] == by_plain
    assert S.CHUNK <= by_contract < m and S.CHUNK <= by_plain < m


def test_extreme_uniforms():
    counts = line_counts([3, 3, 3, 5, 0, 8, 8])
    a = S.seed(counts, 2, "kmeans++", first=0, u=[0.0, 0.0])
    assert a["rows"].tolist() == [0, 3] and a["pick_dist"][1] > 0  # positions 1, 2 coincide with the first pick
    b = S.seed(counts, 2, "kmeans++", first=5, u=[0.0, S.U_MAX])
    assert b["rows"].tolist() == [5, 4] and b["pick_dist"][1] > 0  # position 6 coincides with the pick: mind 0
    for m in (1, 5, 7, 255, 256, 1025, 1 << 20, (1 << 31) - 2):
        assert int(np.float64(S.U_MAX) * np.float64(m)) == m - 1
    c = S.seed(counts, 1, "kmeans++", first=-1, u=[S.U_MAX])
    assert c["rows"].tolist() == [6]
    rng = np.random.default_rng(9)
    big = rng.integers(0, 9, size=(700, 3)).astype(np.uint32)
    big[big.sum(axis=1) == 0, 1] = 1
    for u1 in (0.0, S.U_MAX):
        d = S.seed(big, 2, "kmeans++", first=3, u=[0.0, u1])
        assert d["pick_dist"][1] > 0
    d0 = S.seed(big, 2, "kmeans++", first=3, u=[0.0, 0.0])
    md = S.seed(big, 1, "maximin", first=3)["mindist"]
    assert d0["rows"][1] == np.flatnonzero(md > 0)[0]


def test_duplicates_and_proportional_rows_are_not_picked_while_a_positive_distance_remains():
    base = np.array([[1, 2, 3], [2, 4, 6], [3, 0, 0], [1, 2, 3], [0, 5, 5], [9, 0, 0], [0, 1, 1], [4, 4, 4]],
                    dtype=np.uint32)  # four distinct profiles among eight rows
    rng = np.random.default_rng(2)
    for method, kw in (("maximin", {}), ("kmeans++", {"u": rng.random(8)})):
        a = S.seed(base, 8, method, first=0, **kw)
        assert a["n_distinct"] == 4
        assert (a["pick_dist"][1:4] > 0).all() and (a["pick_dist"][4:] == 0).all()
        assert a["rows"][4:].tolist() == [0, 0, 0, 0]
        p = R.profiles(base)
        assert len({p[r].tobytes() for r in a["rows"][:4]}) == 4
        assert a["potential_final"] == 0.0 and a["radius"] == 0.0 and a["far_row"] == 0


def test_degenerate_cases():
    same = np.tile(np.array([[2, 4, 6]], dtype=np.uint32), (300, 1)) * np.arange(1, 301, dtype=np.uint32)[:, None]
    for method, kw in (("maximin", {}), ("kmeans++", {"u": [0.3, 0.9, 0.0, 0.5]})):
        a = S.seed(same, 4, method, first=7, **kw)
        assert a["rows"].tolist() == [7, 0, 0, 0] and a["n_distinct"] == 1
        assert a["pick_dist"].tolist() == [INF, 0.0, 0.0, 0.0] and a["potential"].tolist() == [INF, 0.0, 0.0, 0.0]
        assert (a["nearest"] == 1).all() and (a["mindist"] == 0).all()
    for method, kw in (("maximin", {}), ("kmeans++", {"u": [0.3, 0.9, 0.1, 0.5, 0.2, 0.7, 0.6]})):
        a = S.seed(LINE5, 7, method, first=1, **kw)  # g > m
        assert sorted(a["rows"][:5].tolist()) == [0, 1, 2, 3, 4] and a["rows"][5:].tolist() == [0, 0]
        assert a["n_distinct"] == 5 and a["nearest"].tolist() == (np.argsort(a["rows"][:5]) + 1).tolist()
        one = S.seed(LINE5, 1, method, first=1, **({"u": [0.3]} if kw else {}))
        assert one["rows"].tolist() == [1] and one["pick_dist"].tolist() == [INF] and one["n_distinct"] == 1
        assert one["mindist"].tolist() == [1 / 32, 0.0, 9 / 32, 25 / 32, 49 / 32] and one["far_row"] == 4
    tie = S.seed(line_counts([4, 1, 7, 7, 1]), 2, "maximin", first=0)  # 1 and 7 are equally far from 4
    assert tie["rows"].tolist() == [0, 1] and tie["far_row"] == 2


def test_maximin_hits_every_planted_group_once():
    counts, truth = planted_groups()
    between, within = separation(counts, truth)
    assert np.sqrt(between) > 2 * np.sqrt(within)  # the condition under which farthest-first cannot repeat a group
    a = S.seed(counts, 5, "maximin", first=0)
    assert sorted(truth[a["rows"]].tolist()) == [1, 2, 3, 4, 5]
    assert same_partition(a["nearest"], truth)


# ------------------------------------------------------------ argument checks

def _seed(dev, m=5, ncol=4, g=2, flags=0, first=0, u=None, n=None, rows=None, null=(), sp=None):
    """A ks_spectra_kmeans_seed(_dev) call that must be refused before any device use."""
    L = _lib.load()
    mm, gg = max(m, 1), max(min(g, 64), 1)
    b = {"sp": np.ones((mm, max(min(ncol, 64), 1)), dtype=np.uint32), "rows_out": np.zeros(gg, dtype=np.int64),
         "near": np.zeros(mm, dtype=np.int32), "mind": np.zeros(mm), "pick_dist": np.zeros(gg),
         "potential": np.zeros(gg)}
    if sp is not None:
        b["sp"] = np.ascontiguousarray(sp, dtype=np.uint32)
    ptr = {k: (None if k in null else v.ctypes.data) for k, v in b.items()}
    rp = None if rows is None else np.ascontiguousarray(rows, dtype=np.int64).ctypes.data
    ua = None if u is None else np.ascontiguousarray(u, dtype=np.float64)
    res = _lib.SeedResult()
    args = [None, ptr["sp"], m if n is None else n, ncol, rp, m, g, flags, first,
            None if ua is None else ua.ctypes.data, ptr["rows_out"], ptr["near"], ptr["mind"], ptr["pick_dist"],
            ptr["potential"], None if "res" in null else C.byref(res)]
    rc = L.ks_spectra_kmeans_seed_dev(*args, None) if dev else L.ks_spectra_kmeans_seed(*args)
    untouched = all(not v.any() for k, v in b.items() if k != "sp")
    return rc, L.ks_last_error().decode(), untouched


@pytest.mark.parametrize("dev", [False, True])
def test_seed_entries_validate_before_any_device_call(dev):
    def refused(text, **kw):
        rc, msg, untouched = _seed(dev, **kw)
        assert rc != 0 and text in msg and untouched, (kw, msg)

    for m in (0, -2):
        refused("at least 1 row", m=m)
    for ncol in (0, -1, _lib.KS_DIST_MAX_NCOL + 1):
        refused("ncol must be between 1 and 4096", ncol=ncol)
    for g in (0, -1, _lib.KS_KM_MAX_GROUPS + 1):
        refused("groups must be between 1 and 65536", g=g)
    for flags in (2, 3, -1):
        refused("unknown flags", flags=flags)
    refused("exceeds n = 3", n=3)  # rows NULL and m = 5 > n
    refused("null spectra", null=("sp",))
    refused("KS_SEED_DSQ needs the g uniform numbers u", flags=1)
    refused("u must be NULL with KS_SEED_MAXIMIN", flags=0, u=[0.5, 0.5])
    for bad in (1.0, -0.0 - 1e-300, np.nan, INF, 1.5):
        refused("u[1] is not in [0, 1)", flags=1, u=[0.25, bad])
        refused("u[0] is not in [0, 1)", flags=1, u=[bad, bad])
    refused("u[2] is not in [0, 1)", flags=1, g=3, u=[0.0, S.U_MAX, 1.0])
    refused("first = -1 (a drawn first row) needs KS_SEED_DSQ", first=-1)
    for first in (5, -2, 1 << 40):
        refused(f"first = {first} is not in 0 .. 4", first=first)
        refused(f"first = {first} is not in 0 .. 4", first=first, flags=1, u=[0.5, 0.5])
    for out in ("rows_out", "near", "mind", "pick_dist", "potential", "res"):
        refused("null output", null=(out,))


def test_host_entry_checks_indices_and_sums():
    """The host entry finds a bad index and an empty row before any device
    call, with the texts of ks_spectra_kmeans; the index comes first."""
    sp = np.ones((5, 4), dtype=np.uint32)
    sp[3] = 0
    rc, msg, untouched = _seed(False, sp=sp)
    assert rc != 0 and msg == "row 3 has no counts" and untouched, msg
    rc, msg, untouched = _seed(False, sp=sp, rows=[0, 3, 9, 3, -1])
    assert rc != 0 and msg == "row index 2 out of range" and untouched, msg
    rc, msg, untouched = _seed(False, sp=sp, rows=[4, 4, 3, 3, 0], flags=1, u=[0.1, 0.2], first=-1)
    assert rc != 0 and msg == "row 2 has no counts" and untouched, msg


def test_python_argument_checks():
    import kmer_spans_amd as K
    ok = np.ones((5, 4), dtype=np.uint32)
    for bad in (np.ones(5), np.ones((5, 4)), np.full((5, 4), -1)):
        with pytest.raises(K.KmerSpansError, match="counts"):
            K.region_kmeans_seed(bad, 2)
    for g in (2.0, "3", None, True, 1 << 40):
        with pytest.raises(K.KmerSpansError, match="g "):
            K.region_kmeans_seed(ok, g)
    with pytest.raises(K.KmerSpansError, match="groups must be between 1 and 65536"):
        K.region_kmeans_seed(ok, 0)
    with pytest.raises(K.KmerSpansError, match="method must be one of"):
        K.region_kmeans_seed(ok, 2, method="random")
    with pytest.raises(K.KmerSpansError, match="draws nothing"):
        K.region_kmeans_seed(ok, 2, u=[0.1, 0.2])
    with pytest.raises(K.KmerSpansError, match="draws nothing"):
        K.region_kmeans_seed(ok, 2, seed=1)
    with pytest.raises(K.KmerSpansError, match="needs a first row"):
        K.region_kmeans_seed(ok, 2, first=None)
    with pytest.raises(K.KmerSpansError, match="exactly one of u"):
        K.region_kmeans_seed(ok, 2, method="kmeans++")
    with pytest.raises(K.KmerSpansError, match="exactly one of u"):
        K.region_kmeans_seed(ok, 2, method="kmeans++", u=[0.1, 0.2], seed=3)
    with pytest.raises(K.KmerSpansError, match="u must hold g = 2 numbers"):
        K.region_kmeans_seed(ok, 2, method="kmeans++", u=[0.1, 0.2, 0.3])
    with pytest.raises(K.KmerSpansError, match="^u\\[1\\] is not in \\[0, 1\\)$"):
        K.region_kmeans_seed(ok, 2, method="kmeans++", u=[0.1, 1.0])
    with pytest.raises(K.KmerSpansError, match="^first = 5 is not in 0 .. 4$"):
        K.region_kmeans_seed(ok, 2, first=5)
    with pytest.raises(K.KmerSpansError, match="first must be an integer"):
        K.region_kmeans_seed(ok, 2, first=0.5)
    with pytest.raises(K.KmerSpansError, match="^row index 1 out of range$"):
        K.region_kmeans_seed(ok, 2, rows=[0, 5])
    g, gb, flags, first, u = _lib.seed_args(3, "kmeans++", None, None, 11)
    assert (g, gb, flags, first) == (3, 3, 1, -1)
    assert np.array_equal(u, np.random.default_rng(11).random(3)) and u.dtype == np.float64
    assert _lib.seed_args(2, "maximin", 4, None, None) == (2, 2, 0, 4, None)
    assert list(_lib.SeedStats().as_dict()) == ["ms_total", "ms_normalise", "ms_steps", "n_launches", "panel_bytes",
                                                "work_bytes"]
    hdr = open(HEADER).read()
    assert "#define KS_SEED_MAXIMIN 0\n" in hdr and "#define KS_SEED_DSQ 1\n" in hdr
    assert _lib.SEED_METHODS == {"maximin": 0, "kmeans++": 1}
    assert C.sizeof(_lib.SeedResult) == 32 and C.sizeof(_lib.SeedStats) == 48
    assert "region_kmeans_seed" in K.__all__
    assert {"ks_spectra_kmeans_seed", "ks_spectra_kmeans_seed_dev"} <= set(_lib.EXPORTS)
