"""The layout of the kept per-index codes (ks_kept_codes_layout, host
arithmetic of ks_scan_chunked.hip's kc_slot): a step of J scan indices is one
record of (J + 1) / 2 dwords, records lie [tile of 64 chunks][step][lane], so a
wave's 64 records of a step are contiguous, every (chunk, index) has a halfword
of its own and the slot holds them all.  No GPU."""
import numpy as np
import pytest

CH = 256


@pytest.mark.parametrize("J", [4, 5, 6, 7])
@pytest.mark.parametrize("nch", [1, 63, 64, 65, 130])
def test_layout_is_a_bijection_inside_the_slot(J, nch):
    from kmer_spans_amd import device as D
    W, NS = (J + 1) // 2, (CH + J - 1) // J
    tiles = (nch + 63) // 64
    nbytes, _ = D.kept_codes_layout(J, nch, 0, 0)
    assert nbytes == tiles * NS * 64 * W * 4
    chunks = sorted({0, 1, 62, 63, 64, nch - 1} & set(range(nch)))
    hw = np.array([[D.kept_codes_layout(J, nch, c, i)[1] for i in range(CH)] for c in chunks])
    assert hw.min() >= 0 and hw.max() < nbytes // 2
    assert np.unique(hw).size == hw.size
    for row, c in zip(hw, chunks):
        i = np.arange(CH)
        # a chunk's record of step s: dword ((tile * NS + s) * 64 + lane) * W, code t in halfword t
        want = (((c // 64) * NS + i // J) * 64 + c % 64) * W * 2 + i % J
        assert np.array_equal(row, want), (J, nch, c)
    if nch > 1:  # neighbouring lanes of a wave: records W dwords apart in every step
        assert np.array_equal(hw[1] - hw[0], np.full(CH, 2 * W))


def test_layout_refuses_bad_arguments():
    from kmer_spans_amd import _lib, device as D
    for args in [(1, 10, 0, 0), (9, 10, 0, 0), (6, 10, 10, 0), (6, 10, 0, 256), (6, 10, -1, 0)]:
        with pytest.raises(_lib.KmerSpansError):
            D.kept_codes_layout(*args)
