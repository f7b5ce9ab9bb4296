"""CPU checks of the host model of the built table forms (tests/tableref.py).

The scan property is what every pass-1 kernel relies on: reading the entry or
line of the m-mer at position i of a sequence gives, in the slot the following
bases select, the table value of the k-mer at i + j, for every j < J.  Here the
k-mers are sliced from the sequence (never formed by shifts), for every form
and every own / J; pad bits must be zero.  Then the two clamps at their
boundaries, the weight renumbering against an order written out by hand, and
the binade predictor on hand values."""
import numpy as np
import pytest

from tests import tableref as TR


def _num(bases):
    """The index of a word: its bases as base-4 digits, the first one highest."""
    v = 0
    for b in bases:
        v = 4 * v + int(b)
    return v


def _seq(k, seed, n=160):
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 4, n)
    s[:2 * k] = 3  # (the all-ones words: the masks at their top bit)
    s[2 * k:3 * k] = 0
    return s


def _field(line_bytes, bit, width):
    return (int.from_bytes(bytes(line_bytes), "little") >> bit) & ((1 << width) - 1)


KS = [2, 3, 4, 5]


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("J", [2, 3, 4])
def test_scan_property_expanded_u16(k, J):
    rng = np.random.default_rng(100 * k + J)
    codes = rng.integers(0, 65536, 4 ** k).astype(np.uint16)
    codes[-1] = 65535
    s = _seq(k, k + J)
    pos = np.arange(len(s) - (k + J - 1) + 1)
    e = np.array([_num(s[i:i + k + J - 1]) for i in pos])
    got = TR.ext_u16(codes, k, J, e)
    assert got.dtype == (np.uint32 if J == 2 else np.uint64)
    for n, i in enumerate(pos):
        v = int(got[n])
        for j in range(J):
            assert (v >> (16 * j)) & 0xFFFF == codes[_num(s[i + j:i + j + k])], (i, j)
        assert v >> (16 * J) == 0


@pytest.mark.parametrize("k", KS)
def test_scan_property_expanded_c12(k):
    rng = np.random.default_rng(k)
    codes = rng.integers(0, 5000, 4 ** k).astype(np.uint16)
    s = _seq(k, k)
    pos = np.arange(len(s) - (k + 4) + 1)
    got = TR.ext_c12(codes, k, np.array([_num(s[i:i + k + 4]) for i in pos]))
    for n, i in enumerate(pos):
        v = int(got[n])
        for j in range(5):
            assert (v >> (12 * j)) & 0xFFF == min(int(codes[_num(s[i + j:i + j + k])]), 0xFFF), (i, j)
        assert v >> 60 == 0


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("J", [2, 3, 4])
def test_scan_property_expanded_f64(k, J):
    rng = np.random.default_rng(7 * k + J)
    vals = rng.normal(size=4 ** k)
    vals[:4] = [-0.0, np.inf, np.nan, 5e-324]
    vb = vals.view(np.uint64)
    s = _seq(k, 3 * k + J)
    pos = np.arange(len(s) - (k + J - 1) + 1)
    got = TR.ext_f64(vals, k, J, np.array([_num(s[i:i + k + J - 1]) for i in pos]))
    assert got.shape == (len(pos), 2 if J == 2 else 4)
    for n, i in enumerate(pos):
        for j in range(J):
            assert got[n, j] == vb[_num(s[i + j:i + j + k])], (i, j)
        assert not got[n, J:].any()


def _line_checks(s, k, own, levels, i):
    """(slot, position of the k-mer it must hold) for the line of the m-mer at i."""
    m = k + own - 1
    out = [(t, i + t) for t in range(own)]
    base = own
    for lev in range(1, levels + 1):
        out.append((base + _num(s[i + m:i + m + lev]), i + own + lev - 1))
        base += 4 ** lev
    return out


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("own", [2, 3, 4, 5])
def test_scan_property_lines_u16(k, own):
    rng = np.random.default_rng(11 * k + own)
    codes = rng.integers(0, 65536, 4 ** k).astype(np.uint16)
    s = _seq(k, 5 * k + own)
    m = k + own - 1
    pos = np.arange(len(s) - m - 2)
    got = TR.lines_u16(codes, k, own, np.array([_num(s[i:i + m]) for i in pos]))
    assert got.shape == (len(pos), 32) and got.dtype == np.uint16
    for n, i in enumerate(pos):
        for slot, p in _line_checks(s, k, own, 2, i):
            assert got[n, slot] == codes[_num(s[p:p + k])], (i, slot)
        assert not got[n, own + 20:].any()


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("own", [2, 3, 4])
def test_scan_property_lines_f64(k, own):
    rng = np.random.default_rng(13 * k + own)
    vals = rng.normal(size=4 ** k)
    vals[:4] = [-0.0, -np.inf, np.nan, 5e-324]
    vb = vals.view(np.uint64)
    s = _seq(k, 7 * k + own)
    m = k + own - 1
    pos = np.arange(len(s) - m - 1)
    got = TR.lines_f64(vals, k, own, np.array([_num(s[i:i + m]) for i in pos]))
    assert got.shape == (len(pos), 8)
    for n, i in enumerate(pos):
        for slot, p in _line_checks(s, k, own, 1, i):
            assert got[n, slot] == vb[_num(s[p:p + k])], (i, slot)
        assert not got[n, own + 4:].any()


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("own", [1, 2, 3, 4])
def test_scan_property_lines_wide(k, own):
    rng = np.random.default_rng(17 * k + own)
    codes = rng.integers(0, 7168, 4 ** k).astype(np.uint16)
    s = _seq(k, 9 * k + own)
    m = k + own - 1
    pos = np.arange(len(s) - m - 3)
    got = TR.lines_wide(codes, k, own, np.array([_num(s[i:i + m]) for i in pos]))
    assert got.shape == (len(pos), 128) and got.dtype == np.uint8
    for n, i in enumerate(pos):
        for slot, p in _line_checks(s, k, own, 3, i):
            want = int(codes[_num(s[p:p + k])])
            if slot < own + 20:
                assert _field(got[n], 13 * slot, 13) == want, (i, slot)
            else:
                assert _field(got[n], 13 * (own + 20) + 11 * (slot - own - 20), 11) == min(want, 2047), (i, slot)
        assert int.from_bytes(bytes(got[n]), "little") >> (13 * (own + 20) + 11 * 64) == 0


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("own", [1, 2, 3])
def test_scan_property_lines_rank(k, own):
    rng = np.random.default_rng(19 * k + own)
    codes = rng.integers(0, 1 << 32, 4 ** k, dtype=np.uint64).astype(np.uint32)
    s = _seq(k, 11 * k + own)
    m = k + own - 1
    pos = np.arange(len(s) - m - 2)
    x = np.array([_num(s[i:i + m]) for i in pos])
    got = TR.lines_rank(codes, k, own, x)
    assert got.shape == (len(pos), 32) and got.dtype == np.uint32
    slots = TR.line_slot_kmers(x, k, own, 2)
    for n, i in enumerate(pos):
        for slot, p in _line_checks(s, k, own, 2, i):
            assert got[n, slot] == codes[_num(s[p:p + k])], (i, slot)
            assert slots[n, slot] == _num(s[p:p + k])
        assert not got[n, own + 20:].any()


def test_clamp_12_bits():
    k = 2
    codes = np.zeros(16, dtype=np.uint16)
    codes[[1, 2, 3, 4]] = [4094, 4095, 4096, 65535]
    e = np.array([_num([0, 1, 0, 2, 0, 3]), _num([1, 0, 0, 0, 0, 0])])  # k-mers 1, 4, 2, 8, 3 and 4, 0, 0, 0, 0
    got = TR.ext_c12(codes, k, e)
    assert [(int(got[0]) >> (12 * t)) & 0xFFF for t in range(5)] == [4094, 4095, 4095, 0, 4095]
    assert int(got[1]) == 4095


def test_clamp_11_bits():
    k, own = 3, 1
    codes = np.zeros(64, dtype=np.uint16)
    codes[[5, 6, 7, 8]] = [2046, 2047, 2048, 7167]
    got = TR.lines_wide(codes, k, own, np.array([0, 5, 7]))
    b3 = 13 * (own + 20)
    # line 0: its L3 continuations are the k-mers 0..63
    assert [_field(got[0], b3 + 11 * c, 11) for c in (5, 6, 7, 8)] == [2046, 2047, 2047, 2047]
    # the 13-bit fields do not clamp: own k-mer 5 / 7, and L2 of x = 0 are the k-mers 0..15
    assert _field(got[1], 0, 13) == 2046 and _field(got[2], 0, 13) == 2048
    assert [_field(got[0], 13 * (own + 4 + c), 13) for c in (5, 6, 7, 8)] == [2046, 2047, 2048, 7167]


def test_renumbering_by_hand():
    #          code 0  1  2  3  4  5
    weights = [5, 9, 5, 0, 9, 7]
    order, perm = TR.renumber(weights)
    assert order.tolist() == [1, 4, 5, 0, 2, 3]   # 9 (code 1), 9 (code 4), 7, 5 (code 0), 5 (code 2), 0
    assert perm.tolist() == [3, 0, 4, 5, 1, 2]
    assert TR.escape_share(weights, 2) == 17 / 35
    assert TR.escape_share(weights, 6) == 0.0 and TR.escape_share([0, 0], 1) == 0.0
    codes = np.array([0, 1, 1, 2, 5, 5, 4, 0], dtype=np.uint16)
    assert TR.code_weights(codes, 8, 6).tolist() == [2, 2, 1, 0, 1, 2]
    # a hint with zeros and a value >= 2^31 (read as uint32), summed exactly
    freq = np.array([3, 0, 7, 0, -(1 << 31), 1, 2, (1 << 31) - 1], dtype=np.int32)
    assert TR.code_weights(codes, 8, 6, freq).tolist() == [3 + (1 << 31) - 1, 7, 0, 0, 2, (1 << 31) + 1]
    big = np.full(4, (1 << 32) - 1, dtype=np.uint32).view(np.int32)
    assert TR.code_weights(np.zeros(4, dtype=np.uint16), 4, 1, big, slab=2).tolist() == [4 * ((1 << 32) - 1)]


def test_gather_through_a_function():
    a = np.arange(1 << 16, dtype=np.uint16) * 7
    calls = []

    def acc(lo, n):
        calls.append((lo, n))
        return a[lo:lo + n]

    idx = np.array([[5, 60000], [7, 5], [60010, 0]])
    assert np.array_equal(TR.gather(acc, idx, gap=100), a[idx])
    assert calls == [(0, 8), (60000, 11)]
    calls.clear()
    x = np.arange(1000, 1256)
    assert np.array_equal(TR.lines_u16(acc, 8, 2, x), TR.lines_u16(a, 8, 2, x))
    assert all(0 <= lo and lo + n <= a.size for lo, n in calls)


def test_predictor_by_hand():
    # k = 2: the prefix is the k-mer, the value itself (0 when it is not finite or has no weight)
    v = np.arange(16, dtype=np.float64) - 3.5
    v[[2, 5]] = [np.nan, np.inf]
    f = np.ones(16, dtype=np.int32)
    f[7] = 0
    mean, cnt = TR.approx(v, 2, f)
    want = v.copy()
    want[[2, 5, 7]] = 0.0
    assert np.array_equal(mean, want) and cnt.tolist() == [int(i not in (2, 5, 7)) for i in range(16)]
    # k = 8: four k-mers per 7-base prefix
    v = np.zeros(4 ** 8)
    v[:8] = [1.0, 2.0, np.nan, 4.0, -np.inf, np.inf, np.nan, np.nan]
    f = np.ones(4 ** 8, dtype=np.int32)
    f[:4] = [1, -(1 << 31), 5, 0]   # weights 1, 2^31, (left out), 0
    mean, cnt = TR.approx(v, 8, f)
    assert mean[0] == (1.0 + 2.0 * 2 ** 31) / (1 + 2 ** 31) and cnt[0] == 2
    assert mean[1] == 0.0 and cnt[1] == 0
    mean, cnt = TR.approx(lambda lo, n: v[lo:lo + n], 8, None, slab=1 << 10)
    assert mean[0] == 7.0 / 3 and cnt[0] == 3 and cnt[2] == 4
    assert TR.to_f16_bits([1.0, 65520.0, 1e-8, -2.0]).tolist() == [0x3C00, 0x7C00, 0x0000, 0xC000]
    assert TR.f16_ulps([0x3C00, 0x0000, 0x8001], [0x3C01, 0x8000, 0x0001]).tolist() == [1, 1, 3]
