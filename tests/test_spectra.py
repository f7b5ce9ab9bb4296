"""Per-region q-mer spectra (ks_region_spectra, include/kmer_spans.h): the
brute-force reference the GPU tests compare against, and the argument checks
of the host entry, which all happen before any device use -- this file runs
without a GPU."""
import ctypes as C
import math

import numpy as np
import pytest

from kmer_spans_amd._lib import KS_SPECTRA_BOTH_STRANDS, KS_SPECTRA_MAX_Q


def rc_code(c: int, q: int) -> int:
    """Reverse complement of a q-digit code (the complement is digit ^ 2)."""
    r = 0
    for _ in range(q):
        r = (r << 2) | ((c & 3) ^ 2)
        c >>= 2
    return r


def brute_spectrum(seq: bytes, beg: int, end: int, q: int, both: bool) -> np.ndarray:
    """Substring seq[beg-1 .. end-1] (1-based inclusive, R's subseq), a loop
    over its windows of q bytes, a dictionary of codes; windows with N/n are
    skipped, every other byte is coded (c >> 1) & 3."""
    sub = seq[beg - 1:end]
    n = {}
    for i in range(len(sub) - q + 1):
        w = sub[i:i + q]
        if b"N" in w or b"n" in w:
            continue
        code = 0
        for ch in w:
            code = (code << 2) | ((ch >> 1) & 3)
        n[code] = n.get(code, 0) + 1
    row = np.zeros(4 ** q, dtype=np.int64)
    for code, v in n.items():
        row[code] += v
        if both:
            row[rc_code(code, q)] += v
    return row


def brute_entropy(row) -> float:
    """-sum p log2 p over the non-zero bins, summed exactly (math.fsum); NaN
    for an empty row."""
    row = np.asarray(row, dtype=np.int64)
    t = int(row.sum())
    if t == 0:
        return float("nan")
    p = row[row > 0] / float(t)  # FP64 terms from the exact integers
    return math.fsum((-(p * np.log2(p))).tolist())


def entropy_bound(q: int) -> float:
    """4^q additions of at most 2q * 2^-53 each, doubled for the terms' own error."""
    return 4 ** q * 2 * q * 2.0 ** -52


def _call(seqs, sid, beg, end, q=2, flags=0, n=None, spectra=True, entropy=True):
    from kmer_spans_amd import _lib
    from kmer_spans_amd.api import _HostSeqs
    L = _lib.load()
    hs = _HostSeqs(seqs)
    sid, beg, end = (np.ascontiguousarray(x, dtype=np.int32) for x in (sid, beg, end))
    n = sid.size if n is None else n
    nb = 4 ** q if 1 <= q <= KS_SPECTRA_MAX_Q else 1
    sp = np.zeros((max(sid.size, 1), nb), dtype=np.uint32)
    en = np.zeros(max(sid.size, 1), dtype=np.float64)
    rc = L.ks_region_spectra(None, hs.ptrs, hs.lens.ctypes.data, hs.n, sid.ctypes.data, beg.ctypes.data,
                             end.ctypes.data, n, q, flags, sp.ctypes.data if spectra else None,
                             en.ctypes.data if entropy else None)
    return rc, L.ks_last_error().decode()


def test_brute_force_known_answer():
    row = brute_spectrum(b"ACGT", 1, 4, 2, False)
    assert sorted(np.nonzero(row)[0].tolist()) == [1, 7, 14] and row.sum() == 3  # AC, CG, GT
    both = brute_spectrum(b"ACGT", 1, 4, 2, True)
    assert sorted(np.nonzero(both)[0].tolist()) == [1, 7, 14]
    assert both[1] == both[7] == both[14] == 2 and both.sum() == 6
    assert brute_entropy(both) == pytest.approx(math.log2(3), abs=1e-15)
    assert math.isnan(brute_entropy(np.zeros(16, dtype=np.int64)))
    import kmer_spans_amd as K
    names = K.kmer_seq(2)
    assert [names[c] for c in (1, 7, 14)] == ["AC", "CG", "GT"]


@pytest.mark.parametrize("q", range(1, KS_SPECTRA_MAX_Q + 1))
def test_rc_is_an_involution(q):
    for c in range(4 ** q):
        assert rc_code(rc_code(c, q), q) == c
    # the complement of A (0) is T (2), of C (1) is G (3)
    assert rc_code(0, 1) == 2 and rc_code(1, 1) == 3


@pytest.mark.parametrize("kw,msg", [
    (dict(q=0), "q must be between 1 and 6"),
    (dict(q=7), "q must be between 1 and 6"),
    (dict(flags=KS_SPECTRA_BOTH_STRANDS << 1), "unknown spectra flags"),
    (dict(flags=5), "unknown spectra flags"),
    (dict(n=-1), "must not be negative"),
    (dict(spectra=False), "null output"),
])
def test_host_entry_rejects_arguments_before_device(kw, msg):
    rc, err = _call(["ACGTACGT"], [0], [1], [8], **kw)
    assert rc == 1 and msg in err, (rc, err)


@pytest.mark.parametrize("sid,beg,end,bad", [
    ([0, 2], [1, 1], [4, 4], 1),      # seq_id = nseq
    ([0, -1], [1, 1], [4, 4], 1),     # seq_id < 0
    ([0, 0, 1], [1, 0, 1], [4, 4, 3], 1),   # beg = 0
    ([1, 0], [1, 1], [4, 4], 0),      # end > len (sequence 1 has 3 bytes)
    ([0, 0], [1, 5], [8, 3], 1),      # end < beg - 1
])
def test_host_entry_rejects_intervals_before_device(sid, beg, end, bad):
    rc, err = _call(["ACGTACGT", "ACG"], sid, beg, end)
    assert rc == 1 and err == f"interval {bad} out of range", (rc, err)


def test_zero_intervals_is_ok():
    from kmer_spans_amd import _lib
    L = _lib.load()
    assert L.ks_region_spectra(None, None, None, 0, None, None, None, 0, 4, 1, None, None) == 0
    assert L.ks_region_spectra_dev(None, None, None, None, None, 0, 4, 0, None, None, None) == 0
    st = _lib.SpectraStats()
    st.n_regions = 7
    assert L.ks_region_spectra_dev(None, None, None, None, None, 0, 4, 0, None, None, C.byref(st)) == 0
    assert st.n_regions == 0
    # the other checks come first
    assert L.ks_region_spectra(None, None, None, 0, None, None, None, 0, 7, 0, None, None) == 1


def test_tile_bases():
    from kmer_spans_amd import _lib
    t = _lib.load().ks_spectra_tile_bases()
    assert t > 0 and t % 64 == 0


def test_api_accepts_both_pos_layouts():
    """[3, R] (kmer_regions) and [R, 3] (kmer_low_comp_regions) name the same
    intervals: the host entry's check rejects the same one of them -- before
    any device use, so this needs no GPU."""
    import kmer_spans_amd as K
    pos = np.array([[0, 0, 0, 0], [1, 2, 9, 1], [4, 8, 9, 8]], dtype=np.int32)  # interval 2: end 9 > len 8
    for p in (pos, pos.T.copy()):
        with pytest.raises(K.KmerSpansError, match="^interval 2 out of range$"):
            K.region_spectra("ACGTACGT", p, q=2)
    # a 3 x 3 matrix is read as [3, R]: column 1 is (0, 2, 9), past the end
    # (read as [R, 3], row 0 = (0, 0, 0) would be the bad one)
    p33 = np.array([[0, 0, 0], [1, 2, 1], [8, 9, 8]], dtype=np.int32)
    with pytest.raises(K.KmerSpansError, match="^interval 1 out of range$"):
        K.region_spectra("ACGTACGT", p33, q=2)
    # 1-based ids of lr_regions
    with pytest.raises(K.KmerSpansError, match="^interval 0 out of range$"):
        K.region_spectra("ACGTACGT", np.array([[0], [1], [4]], dtype=np.int32), q=2, seq_base=1)
    for bad in (np.zeros((2, 4), dtype=np.int32), np.zeros(3, dtype=np.int32)):
        with pytest.raises(K.KmerSpansError, match="pos must be"):
            K.region_spectra("ACGTACGT", bad)
    with pytest.raises(K.KmerSpansError, match="q must be between 1 and 6"):
        K.region_spectra("ACGTACGT", pos[:, :2], q=7)
    assert "region_spectra" in K.__all__
