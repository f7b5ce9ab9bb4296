"""The references of tests/histref.py are right, and the inputs the GPU
tests run (test_gpu_count_seams.py, test_gpu_windowed_seams.py) are not
vacuous.  CPU only: the C oracle and the brute-force restatement of
tests/test_windowed.py are the yardsticks here; the kernels are not involved.
"""
import random

import numpy as np
import pytest

from tests import histref as H
from tests.test_windowed import _code, brute_windowed


def _same_counts(oracle, seqs, k, what):
    codes = H.counted_codes(seqs, k)
    n, c = oracle.kmer_counts(seqs, k)
    assert n == len(codes), (what, k)
    assert np.array_equal(np.bincount(codes, minlength=4 ** k), c), (what, k)
    return len(codes)


# ------------------------------------------------------- references are right

def test_counted_codes_golden_and_edges(oracle, golden):
    for case in golden["kmer_counts"]:
        codes = H.counted_codes(case["seq"], case["k"])
        assert len(codes) == case["n"], case
        if "counts" in case:
            assert np.bincount(codes, minlength=4 ** case["k"]).tolist() == case["counts"]
        _same_counts(oracle, case["seq"], case["k"], "golden")
    # the sequences of test_gpu_parity.py::test_edge_inputs
    edges = [[""], ["N" * 50], ["A"], ["ACGT" * 3, "", "NNN", "G"], ["n" * 3 + "acgt" + "N"],
             ["A" * 5000], ["AC" * 3000 + "N" + "GT" * 3000]]
    for seqs in edges:
        for k in (1, 2, 3, 7):
            _same_counts(oracle, seqs, k, seqs)


def test_counted_codes_random_small(oracle):
    rng = random.Random(5)
    for _ in range(200):
        k = rng.randint(1, 9)
        seqs = ["".join(rng.choice(rng.choice(["ACGT", "ACGTNacgtn", "NNNNA", "ACGTRY"]))
                        for _ in range(rng.randint(0, 300))) for _ in range(rng.randint(1, 4))]
        _same_counts(oracle, seqs, k, seqs)


@pytest.mark.parametrize("k", range(1, 13))
def test_tiny_cases(oracle, k):
    for name, seqs, nothing in H.tiny_cases(k):
        n = _same_counts(oracle, seqs, k, name)
        assert (n == 0) == nothing, (name, k, n)
        if name in ("short-list", "short-list-n"):
            assert sum(map(len, seqs)) < 32 and max(map(len, seqs)) > k
        if name.startswith("total"):
            assert sum(map(len, seqs)) == int(name[5:])


@pytest.mark.parametrize("k", (13, 14, 15))
def test_tiny_cases_large_k(k):
    """4^k counters are not built on the CPU here: the word totals alone."""
    for name, seqs, nothing in H.tiny_cases(k):
        assert (len(H.counted_codes(seqs, k)) == 0) == nothing, (name, k)
        if name in ("short-list", "short-list-n"):
            assert sum(map(len, seqs)) < 32 and max(map(len, seqs)) > k


def _check_planted(seqs, planted, k):
    """Every planted Q1 run does drop a window: one more base on that sequence
    makes the run k + 1 long and counts two words where it counted none (the
    word total is a sum over sequences).  A run of k + 1 gains one."""
    for p in planted:
        if p["kind"] in ("q1", "k1"):
            s = seqs[p["seq"]]
            assert s[-k - 1 if p["kind"] == "q1" else -k - 2] == ord("N"), p
            tail = s[-(k + 3):]
            gain = len(H.counted_codes([tail + b"A"], k)) - len(H.counted_codes([tail], k))
            assert gain == (2 if p["kind"] == "q1" else 1), p


def _check_seam_corpus(oracle, k, rot, reps):
    tile = H.count_tile(k)
    seqs, planted = H.seam_corpus(0, k, tile, rot, reps)
    assert sum(map(len, seqs)) == 35 * reps * tile + tile // 2 + 7
    assert sorted(p["d"] for p in planted) == sorted(list(range(-17, 18)) * reps)
    assert all(p["pos"] - p["boundary"] == p["d"] and p["boundary"] % tile == 0 for p in planted)
    _check_planted(seqs, planted, k)
    if k > 12:  # (4^k counters are not built on the CPU here)
        assert len(H.counted_codes(seqs, k)) > 0
        return planted
    assert _same_counts(oracle, seqs, k, ("seam", rot)) > 0
    # the corpus's word total against one more base on a Q1 sequence, in full, once
    q1 = next(p for p in planted if p["kind"] == "q1")
    more = list(seqs)
    more[q1["seq"]] = more[q1["seq"]] + b"A"
    assert oracle.kmer_counts(seqs, k)[0] + 2 == oracle.kmer_counts(more, k)[0]
    return planted


@pytest.mark.parametrize("rot", range(5))
@pytest.mark.parametrize("k", H.SEAM_KS)
def test_seam_corpora(oracle, k, rot):
    _check_seam_corpus(oracle, k, rot, 1)


def test_seam_corpus_k15(oracle):
    """k = 15 runs one corpus that holds every kind at every offset."""
    planted = _check_seam_corpus(oracle, 15, 0, 5)
    assert len({(p["kind"], p["d"]) for p in planted}) == 5 * 35


def test_seam_kinds_cover_every_offset():
    for k in (7, 11):
        seen = set()
        for rot in range(5):
            seen |= {(p["kind"], p["d"]) for p in H.seam_corpus(0, k, H.count_tile(k), rot)[1]}
        assert len(seen) == 5 * 35


@pytest.mark.parametrize("k", H.SEAM_KS)
def test_tail_corpora(oracle, k):
    for kind in H.EVENTS:
        for t in range(18):
            seqs, planted = H.tail_corpus(0, k, H.count_tile(k), kind, t)
            _check_planted(seqs, planted, k)
            total = sum(map(len, seqs))
            assert planted[0]["pos"] == total - t
            if k <= 12:
                assert _same_counts(oracle, seqs, k, (kind, t)) > 0
            else:
                assert len(H.counted_codes(seqs, k)) > 0


@pytest.mark.parametrize("k", H.MANY_KS)
def test_many_seqs_corpus(oracle, k):
    seqs, _ = H.many_seqs_corpus(0, k)
    lens = np.array([len(s) for s in seqs])
    assert len(seqs) + 1 > 4096  # the 64-ary start search narrows twice
    for L in (0, k - 1, k, k + 1):
        assert (lens == L).sum() > 300
    if k <= 12:
        assert _same_counts(oracle, seqs, k, "many") > 40_000
    else:
        assert len(H.counted_codes(seqs, k)) > 40_000 - k


def test_multi_k_reference(oracle):
    """count_multi runs the seam corpora built for one k at other k's."""
    seqs, _ = H.seam_corpus(0, 8, 4096, 2)
    for k in range(1, 11):
        _same_counts(oracle, seqs, k, "multi")
    seqs, _ = H.seam_corpus(0, 11, H.PART_TILE, 1)
    for k in (12, 2, 11):
        _same_counts(oracle, seqs, k, "multi")


def test_geometry_corpora(oracle):
    tiles = sorted((t + H.PART_TILE - 1) // H.PART_TILE for t in H.GEOMETRY_TOTALS)
    assert tiles == [1, 2, 3, 9, 9, 10, 17, 18, 63, 64]
    # block counts whose last group of gs = ceil(G / 8) blocks is short
    assert [g for g in tiles if g % ((g + 7) // 8)] == [9, 9, 17, 63]
    for total in H.GEOMETRY_TOTALS:
        seqs, _ = H.geometry_corpus(0, total)
        assert sum(map(len, seqs)) == total
        assert _same_counts(oracle, seqs, 11, total) > total // 2
    seqs, _ = H.geometry_corpus(0, H.BIG_TOTAL)
    assert (H.BIG_TOTAL + H.PART_TILE - 1) // H.PART_TILE == 520
    assert _same_counts(oracle, seqs, 12, "big") > H.BIG_TOTAL // 2


# ------------------------------------------------------------------- windowed

def test_windowed_ref_matches_brute_force():
    """The 40 random inputs of test_windowed.py::test_oracle_matches_brute_force."""
    rng = random.Random(13)
    for _ in range(40):
        k = rng.randint(1, 4)
        window = rng.randint(2 * k, 2 * k + 12)
        seqs = ["".join(rng.choice("ACGTacgtN" if rng.random() < 0.3 else "ACGT") for _ in range(rng.randint(0, 60)))
                for _ in range(rng.randint(1, 3))]
        kmers = ["".join(rng.choice("ACGTN") for _ in range(k)) for _ in range(rng.randint(1, 5))]
        d, sc = brute_windowed(seqs, kmers, k, window)
        rd, rsc = H.windowed_ref(seqs, [_code(q, k) for q in kmers], k, window)
        assert np.array_equal(rd, d), (seqs, kmers, k, window)
        for a, b in zip(rsc, sc):
            assert (a is None and b is None) or np.array_equal(a, b)


def _oracle_agrees(oracle, seqs, kmers, k, window):
    o = oracle.windowed_dist(seqs, kmers, k, window, 1)
    d, sc = H.windowed_ref(seqs, [H.encode(q) for q in kmers], k, window)
    assert np.array_equal(d, o["dist"])
    assert len(sc) == len(o["scores"])
    for a, b in zip(sc, o["scores"]):
        assert (a is None and b is None) or np.array_equal(a, b)
    assert o["seq_i"].tolist() == [int(len(s) > window) for s in seqs]
    return o


@pytest.mark.parametrize("name", list(H.windowed_cases()))
def test_windowed_corpora(oracle, name):
    case = H.windowed_cases()[name]
    k, window, nq = case["k"], case["window"], case["nq"]
    seqs, kmers, planted = H.build_windowed(case)
    assert len(kmers) == nq and all(len(q) == k for q in kmers)
    d = _oracle_agrees(oracle, seqs, kmers, k, window)["dist"]
    assert d[:, 0].sum() > 0                                   # there are windows
    assert (d.sum(axis=0) == d[:, 0].sum()).all()              # the same number for every query
    assert not d[window - k + 2:].any()                        # no window holds more than window - k + 1
    for g0 in range(0, nq, 16):                                # every query group counts something
        assert d[1:, g0:g0 + 16].sum() > 0, g0
    kinds = {p["kind"] for p in planted}
    assert {"n", "homopolymer", "dinucleotide"} <= kinds
    if nq >= 5:
        assert kmers[0] == "A" * k and kmers[1] == kmers[2] and kmers[3] == H.absent_kmer(k)
        assert np.array_equal(d[:, 1], d[:, 2]) and d[1:, 3].sum() == 0
    if case["seams"]:  # a lane slides R window starts, the next lane primes anew
        assert max(r for runs in case["layout"] for r in runs) - window + 1 > H.window_R(window)
    if case["maxbin"]:
        assert d[window - k + 1, 0] > 0


def test_windowed_seam_sweeps():
    cases = H.windowed_cases()
    for w in (8, 100, 511):
        W = sorted(H.window_starts_per_run(H.build_windowed(cases[f"seams-w{w}"])[0], w))
        assert W == list(range(1020, 1031)) + list(range(2044, 2053))
    W = sorted(H.window_starts_per_run(H.build_windowed(cases["seams-w600"])[0], 600))
    assert W == list(range(1195, 1206)) and H.window_R(600) == 1200


def test_inclusion_corpus(oracle):
    for k, window in ((3, 40), (2, 4), (5, 1030)):
        seqs, kmers, included = H.inclusion_corpus(0, k, window)
        o = _oracle_agrees(oracle, seqs, kmers, k, window)
        assert o["seq_i"].tolist() == included
        # window + 1 bases hold two windows; three runs of exactly `window` one each
        assert H.window_starts_per_run(seqs, window) == [2, 1, 1, 1] and o["dist"][:, 0].sum() == 5
        assert sum(x is not None for x in o["scores"]) == 4
        assert not o["scores"][2].any() and o["scores"][0] is None and o["scores"][3] is None
        assert o["dist"][1:].sum() > 0
