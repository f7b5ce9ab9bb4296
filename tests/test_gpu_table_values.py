"""The values a table holds, read back through the test window: the
compression of ks_table_create (codes + LUT) and the int_exact /
no_nan_posinf / max_abs flags against numpy, and ks_table_from_counts
against the host builders (pinned to the oracle in tests/test_lib.py) with
count arrays placed on its seams: the LDS / global split of the value
histogram at 8,192, the last count whose histogram fits the scratch and the
first that takes the sort, wrapped counts, medians between two values and at
zero, the LDS split of the count map at 8,192 distinct counts, and the
65,536 / 65,537 distinct-value boundary of the compression."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from kmer_spans_amd import _lib, device as D
    c = _lib.context(0)
    D.bind_torch_stream(c)
    return c


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _props_of(s):
    """(int_exact, no_nan_posinf, bits of max_abs) as numpy computes them."""
    fin = np.isfinite(s)
    with np.errstate(invalid="ignore"):
        exact = bool(np.all(fin & (s == np.rint(s)) & (np.abs(s) <= 2.0 ** 20)))
    ok = not bool(np.any(np.isnan(s) | np.isposinf(s)))
    ma = np.float64(np.max(np.abs(s[fin]))) if fin.any() else np.float64(0.0)
    return exact, ok, int(_bits([ma])[0])


def _check_props(t, s, what):
    p = t.debug_props()
    got = (bool(p["int_exact"]), bool(p["no_nan_posinf"]), int(_bits([p["max_abs"]])[0]))
    assert got == _props_of(s), (what, got, _props_of(s))


def _check_values(t, s, what):
    """codes + LUT (ascending in unsigned bit order) or d_vals hold s bitwise."""
    sb = _bits(s)
    nd = np.unique(sb).size
    assert t.distinct in (nd, -1), (what, t.distinct, nd)
    if t.compressed:
        assert t.distinct == nd <= 65536, (what, t.distinct, nd)
        codes, lut = t.debug_read("codes"), t.debug_read("lut", dtype=np.uint64)
        assert lut.size == nd and np.all(lut[1:] > lut[:-1]), what
        assert np.array_equal(lut[codes], sb), what
        assert t.debug_bytes("vals") == 0
    else:
        assert np.array_equal(t.debug_read("vals", dtype=np.uint64), sb), what
        assert t.debug_bytes("codes") == 0 and t.debug_bytes("lut") == 0


def test_window_is_bounds_checked(ctx):
    """ks_table_debug_bytes / ks_table_debug_read: a part the table lacks has
    0 bytes, and a range outside a part is refused before any copy."""
    from kmer_spans_amd import _lib, device as D
    t = D.DeviceTable(ctx, np.arange(16.0), 2, 0.0, compress=True)
    try:
        assert (t.debug_bytes("codes"), t.debug_bytes("lut"), t.debug_bytes("vals"), t.debug_bytes("ext")) == (32, 128, 0, 0)
        assert _lib.load().ks_table_debug_bytes(t._h, 99) == 0
        assert np.array_equal(t.debug_read("codes"), np.arange(16)) and t.debug_read("codes", 16, 0).size == 0
        assert np.array_equal(t.debug_read("lut", 3, 2), [3.0, 4.0])
        for args in (("codes", 0, 17), ("codes", 16, 1), ("codes", -1, 1), ("lut", 0, -1), ("ext", 0, 1), ("vals", 0, 1)):
            with pytest.raises(_lib.KmerSpansError, match="ks_table_debug_read"):
                t.debug_read(*args)
    finally:
        t.close()


NAN_A, NAN_B = 0x7FF8000000000123, 0xFFF8000000000001


def _with_specials(k, seed):
    rng = np.random.default_rng(seed)
    n = 4 ** k
    w = np.round(rng.normal(size=n) * 4) / 4
    at = [i for i in rng.permutation(n) if i not in (n // 2, n // 2 + 1)][:6]
    w[at] = [0.0, -0.0, np.inf, -np.inf, 0.0, 0.0]
    w.view(np.uint64)[[n // 2, n // 2 + 1]] = [NAN_A, NAN_B]
    return w


@pytest.mark.parametrize("k", [2, 4, 8])
@pytest.mark.parametrize("kind", ["specials", "single"])
def test_compression(ctx, k, kind):
    """k = 2: 16 values, less than one wave."""
    from kmer_spans_amd import device as D
    w = _with_specials(k, k) if kind == "specials" else np.full(4 ** k, -1.75)
    for thr in (0.0, 0.25):
        s = w - thr
        t = D.DeviceTable(ctx, w, k, thr, compress=True)
        try:
            assert t.compressed
            _check_values(t, s, (k, kind, thr))
            _check_props(t, s, (k, kind, thr))
            if kind == "specials" and thr == 0.0:  # both zeros and both NaNs are values of their own
                lut = set(t.debug_read("lut", dtype=np.uint64).tolist())
                assert {0, 1 << 63, NAN_A, NAN_B} <= lut
        finally:
            t.close()


@pytest.mark.parametrize("nd", [65536, 65537])
def test_compression_boundary(ctx, nd):
    from kmer_spans_amd import device as D
    k = 9
    rng = np.random.default_rng(nd)
    w = rng.permutation(np.concatenate([np.arange(nd), rng.integers(0, nd, 4 ** k - nd)])) * 0.5 - 1000.0
    t = D.DeviceTable(ctx, w, k, 0.5, compress=True)
    try:
        assert t.distinct == nd and t.compressed == (nd <= 65536)
        _check_values(t, w - 0.5, nd)
        _check_props(t, w - 0.5, nd)
    finally:
        t.close()


@pytest.mark.parametrize("k", [2, 4, 8])
def test_props_one_offender(ctx, k):
    """An all-integer table of magnitude <= 2^20 is int_exact; one offender
    anywhere (first and last lane of a wave and of a block, the last entry)
    is seen, and +-2^20 and -0.0 are none."""
    from kmer_spans_amd import device as D
    n = 4 ** k
    rng = np.random.default_rng(k)
    base = rng.integers(-1000, 1000, n).astype(np.float64)
    plants = [None] + [(i, v) for i in (0, 63, 64, 255, 256, n - 1) if i < n
                       for v in (0.5, 2.0 ** 20 + 1, -np.inf, np.inf, np.nan, 2.0 ** 20, -2.0 ** 20, -0.0)]
    seen = set()
    for j, plant in enumerate(plants):
        w = base.copy()
        if plant:
            w[plant[0]] = plant[1]
        t = D.DeviceTable(ctx, w, k, 0.0, compress=bool(j & 1))
        try:
            _check_props(t, w, (k, plant))
            seen.add(_props_of(w)[:2])
        finally:
            t.close()
    assert seen == {(True, True), (False, True), (False, False)}
    t = D.DeviceTable(ctx, base, k, 0.5, compress=True)   # integers less a half: not exact
    try:
        _check_props(t, base - 0.5, (k, "thr"))
        assert not t.debug_props()["int_exact"]
    finally:
        t.close()


# ------------------------------------------------------------- from_counts

def _host(score, c, k, total):
    import kmer_spans_amd as K
    if score == "log2":
        return np.asarray(K.log2_table(c, k), dtype=np.float64)
    if score == "pm1":
        return np.asarray(K.pm1_table(c, k), dtype=np.float64)
    return np.asarray(K.rank_table(c, k, total), dtype=np.float64)


def _check_from_counts(ctx, c, k, what):
    """All three scores: w_out, the stored values, distinct, the flags."""
    import torch
    from kmer_spans_amd import _lib, device as D
    c = np.ascontiguousarray(c, dtype=np.int32)
    assert c.size == 4 ** k
    dc = torch.from_numpy(c).cuda()
    total = float(np.abs(c.astype(np.int64)).sum()) or 1.0
    out = {}
    for score, thr in (("log2", 0.0), ("pm1", 0.0), ("pm1", 0.5), ("rank", 0.75)):
        try:
            want = _host(score, c, k, total)
        except _lib.KmerSpansError:
            want = None
        w = torch.full((4 ** k,), -7.0, dtype=torch.float64, device="cuda")
        try:
            t = D.DeviceTable.from_counts(ctx, dc, k, score, total=total, thr=thr, w_out=w)
        except _lib.KmerSpansError:
            assert want is None, (what, score, "the device entry refuses what the host builder builds")
            continue
        try:
            assert want is not None, (what, score, "the host builder refuses what the device entry builds")
            assert np.array_equal(_bits(w.cpu().numpy()), _bits(want)), (what, score, "w_out")
            s = want - thr
            nd = np.unique(_bits(s)).size
            assert t.compressed == (score != "rank" and nd <= 65536), (what, score, nd)
            _check_values(t, s, (what, score, thr))
            _check_props(t, s, (what, score, thr))
            out[score, thr] = (t.debug_props(), nd, s)
        finally:
            t.close()
    return out


def _small(k, seed, hi=40):
    return np.random.default_rng(seed).integers(0, hi, 4 ** k).astype(np.int32)


@pytest.mark.parametrize("k", [11, 8])
def test_counts_around_the_lds_split(ctx, k):
    """Counts 8,190 .. 8,194 among small ones: 8,191 is the last value of the
    LDS histogram, 8,192 the first of the global one (k = 11; k = 8 sorts)."""
    rng = np.random.default_rng(k)
    c = _small(k, k)
    at = rng.permutation(4 ** k)[:4 ** k // 3]
    c[at] = rng.integers(8190, 8195, at.size)
    c[:5] = np.arange(8190, 8195)
    _check_from_counts(ctx, c, k, "lds split")


@pytest.mark.parametrize("k", [11, 8])
@pytest.mark.parametrize("value", [0, 1, 8191, 8192])
def test_counts_all_equal(ctx, k, value):
    r = _check_from_counts(ctx, np.full(4 ** k, value, dtype=np.int32), k, ("all", value))
    assert all(nd == 1 for (score, _), (_, nd, _) in r.items() if score != "rank")


@pytest.mark.parametrize("k,top", [(11, (1 << 22) - 1), (11, 1 << 22), (12, (1 << 24) - 1), (12, 1 << 24)])
def test_counts_at_the_scratch_limit(ctx, k, top):
    """The value histogram has 2^end_bit bins of 4 B in a scratch of 4^k x
    4 B: a maximum count of 4^k - 1 is the last that fits, 4^k sorts."""
    c = _small(k, top & 0xFF)
    c[4 ** k // 2 + 1] = top
    c[7] = top - 1
    _check_from_counts(ctx, c, k, ("top", top))


@pytest.mark.parametrize("k", [8, 11])
def test_counts_one_negative(ctx, k):
    """A wrapped count takes the sort (all 32 key bits) and, for the ranks,
    the host's sequential prefix; table or refusal, as the host builders."""
    c = _small(k, 5 + k) + 1
    c[4 ** k // 3] = -5
    _check_from_counts(ctx, c, k, "negative")


@pytest.mark.parametrize("k", [8, 11])
def test_counts_medians(ctx, k):
    n = 4 ** k
    rng = np.random.default_rng(k)
    c = np.where(rng.permutation(n) < n // 2, 3, 5).astype(np.int32)   # the median lies between 3 and 5
    _check_from_counts(ctx, c, k, "median between")
    c = _small(k, k, hi=9) + 1
    c[rng.permutation(n)[:n // 2 + 1]] = 0                              # f_med = 0
    r = _check_from_counts(ctx, c, k, "median zero")
    props, _, s = r["log2", 0.0]
    assert not props["no_nan_posinf"] and (np.isnan(s).any() or np.isposinf(s).any())
    assert r["pm1", 0.0][0]["int_exact"] and not r["pm1", 0.5][0]["int_exact"]


def _distinct_counts(k, nd, seed, lo=0):
    """4^k counts with exactly nd distinct values lo .. lo + nd - 1."""
    rng = np.random.default_rng(seed)
    n = 4 ** k
    assert nd <= n
    c = np.concatenate([np.arange(nd), rng.integers(0, nd, n - nd)]) + lo
    return rng.permutation(c).astype(np.int32)


@pytest.mark.parametrize("k,nd", [(8, 8192), (8, 8193), (10, 8192), (10, 8193), (8, 20000), (10, 70000),
                                  (10, 65536), (10, 65537), (11, 65536), (11, 65537)])
def test_counts_distinct(ctx, k, nd):
    """8,192 / 8,193 distinct counts: the LDS-staged map of k_map_counts and
    its global form (k <= 10 sorts); 65,536 / 65,537 distinct log2 values:
    codes or FP64, on the sort (k = 10) and the histogram (k = 11)."""
    r = _check_from_counts(ctx, _distinct_counts(k, nd, nd + k), k, ("distinct", nd))
    assert r["log2", 0.0][1] == nd and r["pm1", 0.0][1] <= 2
