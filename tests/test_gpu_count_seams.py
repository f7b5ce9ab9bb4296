"""k-mer counting (csrc/ks_count.hip) at seams, tiny inputs and every k.

The reference is tests/histref.py::counted_codes, an independent numpy
restatement of the header's counting rules that tests/test_histref.py pins to
the C oracle; the oracle runs alongside it here where its 4^k counters are
affordable (k <= 12).  Everything compared is an integer: every comparison is
exact.  For k >= 13 the dense histogram stays on the device: the bins of the
reference's distinct codes, the number of non-zero bins and the word total
are compared there.

What is pinned (tests/test_histref.py asserts on the CPU that the inputs do
hold these things):
  tiny inputs     every k in 1..15 on a handful of bases, through the device
                  and the host entry: under 32 bases the partitioned counter
                  (k >= 11) leaves its staged scatter, and k = 14, 15 run the
                  two-level counter on one tile;
  seam sweep      a sequence boundary, an N, a Q1 run, a run of k + 1 and an
                  empty sequence at -17 .. +17 around tile boundaries (4096
                  positions for k <= 10 and count_multi, 16384 from k = 11)
                  and before the end of the buffer;
  many sequences  more offsets than the 64-ary start search narrows at once;
  block geometry  tile counts of the partitioned counter whose last group of
                  blocks is short, and more tiles than persistent blocks;
  accumulation    counts are added to what the histogram holds, mod 2^32.
"""
import functools

import numpy as np
import pytest

from tests import histref as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from kmer_spans_amd import _lib
    return _lib.context(0)


@pytest.fixture(scope="module")
def D():
    from kmer_spans_amd import device
    return device


_hist = {}


def _zeros(k):
    """One zeroed int32[4^k] device histogram per k, reused by the tests of this module."""
    import torch
    if k not in _hist:
        for kk in [kk for kk in _hist if kk >= 13]:  # (at most one of the large ones at a time)
            del _hist[kk]
        _hist[k] = torch.zeros(4 ** k, dtype=torch.int32, device="cuda")
    else:
        _hist[k].zero_()
    return _hist[k]


@functools.lru_cache(maxsize=None)
def _corpus(kind, *args):
    seqs, planted = getattr(H, kind)(0, *args)
    return seqs, planted


@functools.lru_cache(maxsize=64)
def _codes(kind, args, k):
    return H.counted_codes(_corpus(kind, *args)[0], k)


def _wrap32(x):
    return np.asarray(x, dtype=np.int64).astype(np.uint32).view(np.int32)


def _check_hist(counts, codes, k, what, times=1, base=0, dense=None):
    """counts (int32[4^k] on the device) holds base + times * histogram(codes) mod 2^32.
    dense (default: k <= 12): against the whole reference histogram; otherwise the bins of the
    reference's distinct codes and the number of bins written, without a 4^k array on the host."""
    import torch
    if (k <= 12) if dense is None else dense:
        want = torch.from_numpy(_wrap32(np.bincount(codes, minlength=4 ** k) * times + base)).to(counts.device)
        if not torch.equal(counts, want):
            bad = torch.nonzero(counts != want).flatten()
            show = [(H.decode(int(c), k), int(counts[c]), int(want[c])) for c in bad[:6]]
            raise AssertionError(f"{what}: k={k}, {bad.numel()} bins differ; (k-mer, got, want): {show}")
        return
    uniq, mult = np.unique(codes, return_counts=True)
    idx = torch.from_numpy(uniq.astype(np.int64)).to(counts.device)
    want = torch.from_numpy(_wrap32(mult * times + base)).to(counts.device)
    got = counts[idx]
    if not torch.equal(got, want):
        bad = torch.nonzero(got != want).flatten()
        show = [(H.decode(int(uniq[i]), k), int(got[i]), int(want[i])) for i in bad[:6]]
        raise AssertionError(f"{what}: k={k}, {bad.numel()} counted k-mers differ; (k-mer, got, want): {show}")
    touched = int(torch.count_nonzero(counts)) if base == 0 else int((counts != base).sum())
    assert touched == len(uniq), (what, k, "bins that no counted k-mer has were written", touched, len(uniq))


def _check_oracle(oracle, seqs, codes, k):
    if k <= 12:
        n, c = oracle.kmer_counts(seqs, k)
        assert n == len(codes) and np.array_equal(c, np.bincount(codes, minlength=4 ** k))


def _count_and_check(ctx, D, seqs, k, codes, what, oracle=None, dense=None):
    counts = _zeros(k)
    n = D.count(ctx, D.from_host(seqs), k, counts)
    assert n == len(codes), (what, k, n, len(codes))
    _check_hist(counts, codes, k, what, dense=dense)
    if oracle is not None:
        _check_oracle(oracle, seqs, codes, k)


def _name(planted):
    """The planted events, shortest form, for a failing assert."""
    return [(p["kind"], p.get("boundary"), p.get("d")) for p in planted[:40]]


# ---------------------------------------------------------------- tiny inputs

@pytest.mark.parametrize("k", range(1, 16))  # small k first
def test_tiny_inputs(ctx, D, oracle, k):
    import kmer_spans_amd as K
    for name, seqs, nothing in H.tiny_cases(k):
        codes = H.counted_codes(seqs, k)
        assert (len(codes) == 0) == nothing
        _count_and_check(ctx, D, seqs, k, codes, (name, seqs), oracle)
        # the host entry: every case up to k = 14; at k = 15 (4 GiB of host counters a call) three of them
        if k <= 14 or name in ("q1", "total31", "short-list-n"):
            r = K.kmer_counts(seqs, k, with_f=False)
            assert r["n"]["n"] == len(codes), (name, seqs, k)
            uniq, mult = np.unique(codes, return_counts=True)
            assert np.array_equal(r["counts"][uniq], mult), (name, seqs, k)
            assert np.count_nonzero(r["counts"]) == len(uniq), (name, seqs, k)
            del r


# ----------------------------------------------------------------- seam sweep

@pytest.mark.parametrize("rot", range(5))
@pytest.mark.parametrize("k", H.SEAM_KS)
def test_tile_seams(ctx, D, oracle, k, rot):
    args = (k, H.count_tile(k), rot)
    seqs, planted = _corpus("seam_corpus", *args)
    _count_and_check(ctx, D, seqs, k, _codes("seam_corpus", args, k), ("seam", rot, _name(planted)), oracle)


def test_tile_seams_k15(ctx, D):
    """Every kind of event at every offset in one corpus of 175 tiles."""
    args = (15, H.PART_TILE, 0, 5)
    seqs, planted = _corpus("seam_corpus", *args)
    _count_and_check(ctx, D, seqs, 15, _codes("seam_corpus", args, 15), "seam k15")
    _hist.pop(15)


@pytest.mark.parametrize("k", H.SEAM_KS)
def test_buffer_end_seams(ctx, D, oracle, k):
    for kind in H.EVENTS:
        for t in range(18):
            seqs, planted = H.tail_corpus(0, k, H.count_tile(k), kind, t)
            # (90 small corpora: from k = 11 without a 4^k reference array each)
            _count_and_check(ctx, D, seqs, k, H.counted_codes(seqs, k), ("buffer end", planted),
                             oracle if k <= 10 else None, dense=k <= 10)


def _multi(ctx, D, seqs, ks, ref, what):
    ds = D.from_host(seqs)
    counts = [_zeros(k) for k in ks]
    words = D.count_multi(ctx, ds, ks, counts)
    for k, c, n in zip(ks, counts, words):
        codes = ref(k)
        assert n == len(codes), (what, k, n, len(codes))
        _check_hist(c, codes, k, what)


@pytest.mark.parametrize("kc,rot", [(1, 0), (7, 1), (8, 2), (10, 3), (10, 4)])
def test_tile_seams_multi_batched(ctx, D, kc, rot):
    """ks = 1 .. 10: a batch of eight and a batch of two over 4096-position tiles."""
    args = (kc, 4096, rot)
    seqs, planted = _corpus("seam_corpus", *args)
    _multi(ctx, D, seqs, list(range(1, 11)), lambda k: _codes("seam_corpus", args, k), ("multi", _name(planted)))


@pytest.mark.parametrize("kc,tile,rot", [(11, H.PART_TILE, 1), (12, H.PART_TILE, 3), (14, H.PART_TILE, 0),
                                         (10, 4096, 2)])
def test_tile_seams_multi_mixed(ctx, D, kc, tile, rot):
    """ks = 14, 12, 2, 11: partitioned counts and a batched one in one call."""
    args = (kc, tile, rot)
    seqs, planted = _corpus("seam_corpus", *args)
    _multi(ctx, D, seqs, [14, 12, 2, 11], lambda k: _codes("seam_corpus", args, k), ("multi", _name(planted)))


# ------------------------------------------------------------- many sequences

@pytest.mark.parametrize("k", H.MANY_KS)
def test_many_sequences(ctx, D, oracle, k):
    seqs, _ = _corpus("many_seqs_corpus", k)
    assert len(seqs) + 1 > 4096
    _count_and_check(ctx, D, seqs, k, _codes("many_seqs_corpus", (k,), k), "many sequences", oracle)


def test_many_sequences_multi(ctx, D):
    seqs, _ = _corpus("many_seqs_corpus", 9)
    _multi(ctx, D, seqs, [5, 9, 11, 14], lambda k: _codes("many_seqs_corpus", (9,), k), "many sequences, multi")


# ------------------------------------------------------------- block geometry

@pytest.mark.parametrize("total", H.GEOMETRY_TOTALS)
@pytest.mark.parametrize("k", H.GEOMETRY_KS)
def test_partitioned_block_geometry(ctx, D, oracle, k, total):
    seqs, _ = _corpus("geometry_corpus", total)
    tiles = (total + H.PART_TILE - 1) // H.PART_TILE
    _count_and_check(ctx, D, seqs, k, _codes("geometry_corpus", (total,), k), ("tiles", tiles), oracle)


def test_partitioned_more_tiles_than_blocks(ctx, D, oracle):
    """520 tiles at k = 12: 512 persistent blocks, eight of them take a second tile."""
    seqs, _ = _corpus("geometry_corpus", H.BIG_TOTAL)
    _count_and_check(ctx, D, seqs, 12, _codes("geometry_corpus", (H.BIG_TOTAL,), 12), "520 tiles", oracle)


# ------------------------------------------------------ accumulation and wrap

@pytest.mark.parametrize("k", H.ACCUM_KS)
def test_accumulates_and_wraps(ctx, D, k):
    args = (k, H.count_tile(k), 0)
    seqs, _ = _corpus("seam_corpus", *args)
    codes = _codes("seam_corpus", args, k)
    ds = D.from_host(seqs)
    counts = _zeros(k)
    for times in (1, 2):
        assert D.count(ctx, ds, k, counts) == len(codes)  # the word total is per call
        _check_hist(counts, codes, k, ("accumulated", times), times=times)
    counts.fill_(-1)  # every bin 0xffffffff
    assert D.count(ctx, ds, k, counts) == len(codes)
    _check_hist(counts, codes, k, "wrap", base=-1)
