"""Windowed k-mer count distributions (csrc/ks_windowed.hip) at the places
where the kernel takes another path.

The reference is tests/histref.py::windowed_ref (prefix sums over "the k-mer
ending here is the query"), pinned on the CPU by tests/test_histref.py, which
also asserts that every corpus used here has windows, non-zero counts in every
group of 16 queries and runs longer than one lane's share where the case is
about that.  The C oracle runs alongside.  Integers throughout: exact.

  LDS limit       the histogram is privatised in LDS up to window 1023 and
                  uses global atomics beyond: 1023, 1024, 1025, with and
                  without per-position scores (all four kernel variants);
  query groups    16 queries per lane: 1, 15, 16, 17, 32, 33 queries, the
                  outputs embedded in larger tensors whose tails must stay;
  large k         k = 9, 12 .. 15 with non-zero counts;
  segment seams   a lane slides R = max(1024, 2 * window) window starts
                  (ks_windowed.hip) and the next lane primes anew: runs with
                  R - 4 .. R + 6 and 2R - 4 .. 2R + 4 window starts;
  inclusion       sequences of exactly the window, one more, and longer ones
                  without a window;
  accumulation    dist is added to.
"""
import functools

import numpy as np
import pytest

from tests import histref as H

pytestmark = pytest.mark.gpu

CASES = H.windowed_cases()
SENTINEL = -77


@pytest.fixture(scope="module")
def ctx():
    from kmer_spans_amd import _lib
    return _lib.context(0)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(sequences, queries, codes, planted, reference dist, reference scores), computed once."""
    c = CASES[name]
    seqs, kmers, planted = H.build_windowed(c)
    codes = [H.encode(q) for q in kmers]
    dist, scores = H.windowed_ref(seqs, codes, c["k"], c["window"])
    return seqs, kmers, codes, planted, dist, scores


def _where(got, want):
    bad = np.argwhere(got != want)
    return [(tuple(int(x) for x in i), int(got[tuple(i)]), int(want[tuple(i)])) for i in bad[:6]]


def _run_device(ctx, seqs, codes, k, window, with_scores=True, calls=1):
    """device.windowed into slices of larger tensors; returns (dist [window + 1, nq],
    included, per-sequence scores or None) after checking that the tails kept their sentinel."""
    import torch
    from kmer_spans_amd import device as D
    ds = D.from_host(seqs)
    nq = len(codes)
    pad = 4096
    dist_all = torch.full((nq * (window + 1) + pad,), SENTINEL, dtype=torch.int32, device="cuda")
    dist = dist_all[:nq * (window + 1)]
    dist.zero_()
    inc_all = torch.full((len(seqs) + 64,), SENTINEL, dtype=torch.int32, device="cuda")
    sc_all = sc = None
    if with_scores:
        sc_all = torch.full((nq * ds.total + pad,), SENTINEL, dtype=torch.int32, device="cuda")
        sc = sc_all[:nq * ds.total]
        sc.zero_()
    for _ in range(calls):
        D.windowed(ctx, ds, codes, k, window, dist, inc_all[:len(seqs)], sc)
    assert bool((dist_all[nq * (window + 1):] == SENTINEL).all()), "dist: written past kmer_n * (window + 1)"
    assert bool((inc_all[len(seqs):] == SENTINEL).all()), "included: written past nseq"
    scores = None
    if with_scores:
        assert bool((sc_all[nq * ds.total:] == SENTINEL).all()), "scores: written past kmer_n * total"
        h = sc.cpu().numpy()
        scores = []
        for q, s in enumerate(seqs):
            a, L = int(ds.offsets[q]), len(s)
            scores.append(h[nq * a:nq * (a + L)].reshape(nq, L).T)
    return dist.cpu().numpy().reshape(nq, window + 1).T, inc_all[:len(seqs)].cpu().numpy(), scores


def _check_device(ctx, name, with_scores=True, oracle=None):
    c = CASES[name]
    k, window = c["k"], c["window"]
    seqs, kmers, codes, planted, rdist, rscores = _case(name)
    dist, inc, scores = _run_device(ctx, seqs, codes, k, window, with_scores)
    assert np.array_equal(dist, rdist), (name, "dist (bin, query), got, want", _where(dist, rdist))
    assert not dist[window - k + 2:].any()  # the rows above window - k + 1 stay zero
    assert inc.tolist() == [int(len(s) > window) for s in seqs]
    if with_scores:
        for q, (got, want) in enumerate(zip(scores, rscores)):
            if want is None:  # an excluded sequence's block stays as the caller zeroed it
                assert not got.any(), (name, "scores of excluded sequence", q)
            else:
                assert np.array_equal(got, want), (name, "scores of sequence", q, "(start, query), got, want",
                                                   _where(got, want), planted[:12])
    if oracle is not None:
        o = oracle.windowed_dist(seqs, kmers, k, window, 1)
        assert np.array_equal(dist, o["dist"]) and inc.tolist() == o["seq_i"].tolist()


def _check_host(name, oracle=None, ret_flag=1):
    import kmer_spans_amd as K
    c = CASES[name]
    seqs, kmers, codes, planted, rdist, rscores = _case(name)
    g = K.window_kmer_dist(seqs, kmers, c["window"], freq=False, ret_flag=ret_flag)
    assert np.array_equal(g["dist"], rdist), (name, _where(g["dist"], rdist))
    assert g["seq_i"].tolist() == [int(len(s) > c["window"]) for s in seqs]
    if ret_flag:
        for a, b in zip(g["scores"], rscores):
            assert (a is None and b is None) or np.array_equal(a, b), name
    else:
        assert g["scores"] is None


# ------------------------------------------------------------------ LDS limit

@pytest.mark.parametrize("with_scores", [True, False])
@pytest.mark.parametrize("window", [1023, 1024, 1025])
def test_lds_limit(ctx, oracle, window, with_scores):
    _check_device(ctx, f"lds-w{window}", with_scores, oracle if with_scores else None)


@pytest.mark.parametrize("window", [1023, 1024])
def test_lds_limit_host_entry(window):
    _check_host(f"lds-w{window}", ret_flag=1)
    _check_host(f"lds-w{window}", ret_flag=0)


# --------------------------------------------------------------- query groups

@pytest.mark.parametrize("nq", [1, 15, 16, 17, 32, 33])
@pytest.mark.parametrize("window", [50, 1024])
def test_query_groups(ctx, oracle, window, nq):
    _check_device(ctx, f"groups-w{window}-q{nq}", True, oracle)


def test_query_groups_host_entry():
    _check_host("groups-w50-q33")
    _check_host("groups-w1024-q17")


# -------------------------------------------------------------------- large k

@pytest.mark.parametrize("wkind", ["2k", "2k+1", "200"])
@pytest.mark.parametrize("k", [9, 12, 13, 14, 15])
def test_large_k(ctx, oracle, k, wkind):
    window = {"2k": 2 * k, "2k+1": 2 * k + 1, "200": 200}[wkind]
    name = f"largek-k{k}-w{window}"
    _check_device(ctx, name, True, oracle if k <= 13 else None)  # (the oracle takes seconds at k = 14, 15)
    if wkind == "2k+1":
        _check_host(name)


# -------------------------------------------------------------- segment seams

@pytest.mark.parametrize("window", [8, 100, 511, 600])
def test_segment_seams(ctx, oracle, window):
    # runs with W = run - window + 1 window starts around R and 2R, R = max(1024, 2 * window)
    # (ks_windowed.hip): 1020 .. 1030 and 2044 .. 2052 below window 512, 1195 .. 1205 at window 600
    name = f"seams-w{window}"
    _check_device(ctx, name, True, oracle)
    _check_device(ctx, name, False)


# ------------------------------------------------------------- inclusion rule

@pytest.mark.parametrize("k,window", [(3, 40), (2, 4), (5, 1030)])
def test_inclusion_rule(ctx, oracle, k, window):
    import kmer_spans_amd as K
    seqs, kmers, included = H.inclusion_corpus(0, k, window)
    codes = [H.encode(q) for q in kmers]
    rdist, rscores = H.windowed_ref(seqs, codes, k, window)
    assert [int(s is not None) for s in rscores] == included
    dist, inc, scores = _run_device(ctx, seqs, codes, k, window)
    assert np.array_equal(dist, rdist), _where(dist, rdist)
    assert inc.tolist() == included
    for got, want in zip(scores, rscores):
        assert np.array_equal(got, want) if want is not None else not got.any()
    assert not scores[2].any()  # longer than the window, no run holds one
    g = K.window_kmer_dist(seqs, kmers, window, freq=False, ret_flag=1)
    o = oracle.windowed_dist(seqs, kmers, k, window, 1)
    assert np.array_equal(g["dist"], rdist) and np.array_equal(o["dist"], rdist)
    assert g["seq_i"].tolist() == included == o["seq_i"].tolist()
    for a, b in zip(g["scores"], rscores):
        assert (a is None and b is None) or np.array_equal(a, b)


# --------------------------------------------------------------- accumulation

@pytest.mark.parametrize("name", ["groups-w50-q17", "lds-w1024"])
def test_dist_accumulates(ctx, name):
    c = CASES[name]
    seqs, kmers, codes, planted, rdist, rscores = _case(name)
    dist, _, _ = _run_device(ctx, seqs, codes, c["k"], c["window"], with_scores=False, calls=2)
    assert np.array_equal(dist, 2 * rdist), _where(dist, 2 * rdist)
