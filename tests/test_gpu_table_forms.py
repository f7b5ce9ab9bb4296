"""Every built form of a score table, read back through the test window
(ks_table_debug_read) and compared bit for bit with the host model of its
layout (tests/tableref.py): the uint16 / 12-bit / FP64 expanded tables, the
64-B lines with own 2..5, the 128-B wide lines and the 128-B rank-code lines,
and the binade predictor.

A scan reads only the entries its genome reaches, so a wrong line elsewhere
passes every scan test.  Here a table of at most 64 MiB is compared whole; a
larger one in slabs of 4,096 consecutive entries or lines: the first and the
last, slabs straddling the structural seams of its build kernel (lane blocks
and grid rows of k_build_lines, grid strides and kU trips of k_build_ext_*),
and 2^16 random lines as 256 reads of 256.  Each case asserts the table's form
first and the number of lines it compared last."""
import numpy as np
import pytest

from tests import tableref as TR

pytestmark = pytest.mark.gpu

MIB = 1 << 20
SLAB = 4096
WHOLE = 64 * MIB


@pytest.fixture(scope="module")
def ctx():
    from kmer_spans_amd import _lib, device as D
    c = _lib.context(0)
    D.bind_torch_stream(c)
    return c


@pytest.fixture(scope="module")
def cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _form(t):
    p = t.debug_props()
    return (p["line_kind"], p["line_own"], t.positions_per_read, t.code_bits, t.compressed)


def _some_multiples(step, n):
    """A few multiples of step inside (0, n): the first two, the middle one, the last two."""
    cnt = (n - 1) // step
    return sorted({j * step for j in (1, 2, cnt // 2, cnt - 1, cnt) if 0 < j * step < n})


def _ranges(n, entry_bytes, seams, seed):
    """(lo, count) ranges of entries to compare."""
    if n * entry_bytes <= WHOLE:
        return [(lo, min(1 << 18, n - lo)) for lo in range(0, n, 1 << 18)]
    out = [(0, SLAB), (n - SLAB, SLAB)]
    out += [(min(max(s - SLAB // 2, 0), n - SLAB), SLAB) for s in seams]
    rng = np.random.default_rng(seed)
    out += [(int(lo), 256) for lo in rng.integers(0, n - 256, 256)]
    return out


def _compare(t, part, n, entry_bytes, seams, model, seed=1):
    """The part's entries against model(x) (an array whose rows are the
    entries' bytes); returns the number compared."""
    assert t.debug_bytes(part) == n * entry_bytes, (part, t.debug_bytes(part), n, entry_bytes)
    done = 0
    for lo, cnt in _ranges(n, entry_bytes, seams, seed):
        got = t.debug_read(part, lo * entry_bytes, cnt * entry_bytes, dtype=np.uint8).reshape(cnt, entry_bytes)
        want = np.ascontiguousarray(model(np.arange(lo, lo + cnt, dtype=np.int64))).view(np.uint8).reshape(cnt, entry_bytes)
        if not np.array_equal(got, want):
            r, c = np.argwhere(got != want)[0]
            pytest.fail(f"{part}: entry {lo + r} byte {c}: {got[r].tobytes().hex()} != {want[r].tobytes().hex()}")
        done += cnt
    return done


def _line_seams(k, m, lev):
    """Lane-block and grid-row seams of k_build_lines (launch_build_lines)."""
    lb, hb = 2 * k - 2 * lev, 2 * m - (2 * k - 2 * lev)
    ys = 0
    while lb + ys < 22 and ys + 2 < hb:
        ys += 1
    nhi = (1 << hb) >> ys
    n = 4 ** m
    return _some_multiples(1 << lb, n) + _some_multiples(nhi << lb, n)


def _ext_seams(nent, per_entry_num, per_entry_den, kU, cus):
    """Entries at which a lane's unit index (pairs: entry / 2, 16-B halves:
    entry * H) is a multiple of the grid stride S and of kU * S."""
    S = 256 * min((nent + 255) // 256, 32 * cus)
    unit = lambda u: u * per_entry_den // per_entry_num  # noqa: E731  (unit index -> entry)
    nunit = nent * per_entry_num // per_entry_den
    return sorted({unit(u) for u in _some_multiples(S, nunit) + _some_multiples(kU * S, nunit)})


def _check_base(t, s):
    """d_codes / d_lut (or d_vals) against the host values s, bitwise."""
    sb = np.ascontiguousarray(s).view(np.uint64)
    if t.compressed:
        codes, lut = t.debug_read("codes"), t.debug_read("lut", dtype=np.uint64)
        assert lut.size == t.distinct == np.unique(sb).size
        assert np.array_equal(lut[codes], sb)
        return codes, lut.view(np.float64)
    vals = t.debug_read("vals", dtype=np.uint64)
    assert np.array_equal(vals, sb)
    return None, vals.view(np.float64)


# ---------------------------------------------------------------- 64-B lines

def _k8_counts(k, seed, half_zero=False):
    """4^k counts with 2^9 distinct values (more than half zero: f_med = 0,
    so log2 gives NaN for the zeros and +Inf for the rest)."""
    rng = np.random.default_rng(seed)
    n = 4 ** k
    vals = np.sort(rng.choice(np.arange(1, 20000), 512, replace=False)).astype(np.int32)
    c = vals[rng.integers(0, 512, n)]
    c[:512] = vals
    if half_zero:
        c[rng.permutation(n)[:n // 2 + 7]] = 0
    return c


@pytest.mark.parametrize("k,own,cap", [(8, 2, 16 * MIB), (8, 3, 64 * MIB), (8, 4, 256 * MIB), (8, 5, 1024 * MIB),
                                       (11, 2, 1024 * MIB)])
def test_lines_u16(ctx, k, own, cap):
    import torch
    import kmer_spans_amd as K
    from kmer_spans_amd import device as D
    c = _k8_counts(k, 3 + own)
    thr = 0.25
    t = D.DeviceTable.from_counts(ctx, torch.from_numpy(c).cuda(), k, "log2", thr=thr, expand=True, max_ext_bytes=cap)
    try:
        assert _form(t) == (1, own, own + 2, 16, True), _form(t)
        codes, _ = _check_base(t, np.asarray(K.log2_table(c, k)) - thr)
        m = k + own - 1
        ncmp = _compare(t, "ext", 4 ** m, 64, _line_seams(k, m, 2), lambda x: TR.lines_u16(codes, k, own, x), seed=own)
        assert ncmp == (4 ** m if 4 ** m * 64 <= WHOLE else 2 * SLAB + len(_line_seams(k, m, 2)) * SLAB + 65536)
        assert len(_line_seams(k, m, 2)) >= 6
    finally:
        t.close()


@pytest.mark.parametrize("own,cap", [(2, 16 * MIB), (3, 64 * MIB), (4, 256 * MIB)])
def test_lines_f64_from_counts(ctx, own, cap):
    """FP64 lines with own 2, 3, 4 (the budget chooses own); the values are
    NaN and +Inf beside finite ones when the median count is 0."""
    import torch
    import kmer_spans_amd as K
    from kmer_spans_amd import device as D
    k = 8
    c = _k8_counts(k, 30 + own, half_zero=(own != 3))
    t = D.DeviceTable.from_counts(ctx, torch.from_numpy(c).cuda(), k, "log2", thr=0.5, compress=False, expand=True,
                                  max_ext_bytes=cap)
    try:
        assert _form(t) == (2, own, own + 1, 64, False), _form(t)
        s = np.asarray(K.log2_table(c, k)) - 0.5
        assert (np.isnan(s).any() and np.isposinf(s).any()) == (own != 3)
        _, vals = _check_base(t, s)
        m = k + own - 1
        ncmp = _compare(t, "ext", 4 ** m, 64, _line_seams(k, m, 1), lambda x: TR.lines_f64(vals, k, own, x), seed=own)
        assert ncmp >= min(4 ** m, 2 * SLAB + 65536)
    finally:
        t.close()


def _special_values(n, seed):
    """Random FP64 values with -0.0, +-Inf, NaNs of two payloads and
    denormals planted (the builds must copy bits)."""
    rng = np.random.default_rng(seed)
    w = rng.normal(size=n)
    sp = np.array([0x8000000000000000, 0x0000000000000000, 0x7FF0000000000000, 0xFFF0000000000000,
                   0x7FF8000000000123, 0xFFF8000000000001, 0x0000000000000001, 0x800FFFFFFFFFFFFF], dtype=np.uint64)
    at = rng.permutation(n)[:8 * 5]
    w.view(np.uint64)[at] = np.tile(sp, 5)
    w.view(np.uint64)[[0, n - 1]] = sp[[0, 4]]
    return w


def test_lines_f64_copies_bits(ctx):
    from kmer_spans_amd import device as D
    k, own = 8, 4
    w = _special_values(4 ** k, 5)
    t = D.DeviceTable(ctx, w, k, 0.0, compress=False, expand=True)
    try:
        assert _form(t) == (2, own, own + 1, 64, False), _form(t)
        _, vals = _check_base(t, w - 0.0)
        m = k + own - 1
        ncmp = _compare(t, "ext", 4 ** m, 64, _line_seams(k, m, 1), lambda x: TR.lines_f64(vals, k, own, x))
        assert ncmp >= 2 * SLAB + 65536
    finally:
        t.close()


# ----------------------------------------------------------- expanded tables

def _table_with(nd, n, seed, skew=0.97, nhead=None):
    """n k-mers over exactly nd distinct values with skewed multiplicities:
    the first nhead values (all but 1/8 by default) share `skew` of the
    k-mers, with ties among the multiplicities.  Returns (the nd values, the
    value index of every k-mer)."""
    rng = np.random.default_rng(seed)
    vals = np.unique(np.round(rng.normal(size=4 * nd + 64), 6))[:nd * 2:2]
    assert vals.size == nd
    vals = rng.permutation(vals)
    nhead = max(1, nd - nd // 8) if nhead is None else min(nhead, nd)
    mult = np.ones(nd, dtype=np.int64)
    if nd > nhead:
        mult[nhead:] += int((n - nd) * (1 - skew)) // (nd - nhead)
    base = (n - mult.sum()) // nhead
    mult[:nhead] += base
    if base >= 4:
        mult[:nhead] += (np.arange(nhead) % 7) - 3   # ties: seven multiplicities
    mult[0] += n - mult.sum()
    assert mult.min() >= 1 and mult.sum() == n
    rep = np.repeat(np.arange(nd, dtype=np.int32), mult)
    # (scattered by a fixed bijection of the indices: n is a power of two, the factor odd)
    return vals, rep[(np.arange(n, dtype=np.int64) * 2654435761) & (n - 1)]


def _renumbered(vals, idx, thr, freq, ndirect):
    """Model of choose_code12 on the table vals[idx] - thr: (codes, LUT bits,
    escape share).  The codes before it are the values' indices among the
    distinct bit patterns in unsigned order."""
    sb = (vals - thr).view(np.uint64)
    ub = np.unique(sb)
    assert ub.size == vals.size
    old = np.searchsorted(ub, sb)[idx]
    wts = TR.code_weights(old, old.size, ub.size, freq)
    order, perm = TR.renumber(wts)
    return perm[old].astype(np.uint16), ub[order], TR.escape_share(wts, ndirect)


def _set_env(monkeypatch, **env):
    for name in ("KS_NO_LINES", "KS_EXT_MAX_J", "KS_EXT_ESCAPE_MAX", "KS_NO_WIDE_LINES"):
        monkeypatch.delenv(name, raising=False)
    for name, v in env.items():
        monkeypatch.setenv(name, str(v))


@pytest.mark.parametrize("k,J", [(3, 2), (3, 3), (3, 4), (9, 2), (9, 3), (9, 4), (10, 4)])
def test_expanded_u16(ctx, cus, monkeypatch, k, J):
    from kmer_spans_amd import device as D
    _set_env(monkeypatch, KS_NO_LINES=1, KS_EXT_MAX_J=J)
    n = 4 ** k
    w = np.random.default_rng(k * 10 + J).integers(0, min(n, 60000), n) * 0.125
    t = D.DeviceTable(ctx, w, k, 0.375, compress=True, expand=True)
    try:
        assert _form(t) == (0, 0, J, 16, True), _form(t)
        codes, _ = _check_base(t, w - 0.375)
        nent, eb = 4 ** (k + J - 1), 4 if J == 2 else 8
        seams = _ext_seams(nent, 1, 2, 8 if J == 4 else 1, cus)
        ncmp = _compare(t, "ext", nent, eb, seams, lambda e: TR.ext_u16(codes, k, J, e), seed=J)
        assert ncmp == (nent if nent * eb <= WHOLE else (2 + len(seams)) * SLAB + 65536)
        assert nent * eb <= WHOLE or seams
    finally:
        t.close()


@pytest.mark.parametrize("k,J", [(3, 2), (3, 3), (3, 4), (9, 2), (9, 3), (9, 4)])
def test_expanded_f64(ctx, cus, monkeypatch, k, J):
    from kmer_spans_amd import device as D
    _set_env(monkeypatch, KS_NO_LINES=1, KS_EXT_MAX_J=J)
    w = _special_values(4 ** k, k + J)
    t = D.DeviceTable(ctx, w, k, 0.0, compress=False, expand=True)
    try:
        assert _form(t) == (0, 0, J, 64, False), _form(t)
        _, vals = _check_base(t, w - 0.0)
        nent, eb, H = 4 ** (k + J - 1), 16 if J == 2 else 32, 1 if J == 2 else 2
        seams = _ext_seams(nent, H, 1, 8 if J == 4 else 1, cus)
        ncmp = _compare(t, "ext", nent, eb, seams, lambda e: TR.ext_f64(vals, k, J, e), seed=J)
        assert ncmp == (nent if nent * eb <= WHOLE else (2 + len(seams)) * SLAB + 65536)
    finally:
        t.close()


@pytest.mark.parametrize("k,nd,hint", [(3, 40, False), (9, 4095, False), (9, 4096, False), (9, 5000, False),
                                       (9, 5000, True), (9, 300, True)])
def test_expanded_c12(ctx, cus, monkeypatch, k, nd, hint):
    """J = 5 with 12-bit codes: the weight renumbering (d_codes, d_lut,
    d_lut12, d_map12, the escape share) and the table, at the 4,095 / 4,096
    distinct-value boundary, with and without a hint that has zeros and one
    value >= 2^31."""
    import torch
    from kmer_spans_amd import device as D
    n = 4 ** k
    vals, idx = _table_with(nd, n, 7 * k + nd + hint)
    w, thr = vals[idx], 0.5
    freq = None
    if hint:
        rng = np.random.default_rng(nd)
        freq = rng.geometric(0.05, n).astype(np.int64)
        freq[rng.permutation(n)[:n // 3]] = 0
        freq[n // 2] = (1 << 31) + 12345
        freq = freq.astype(np.uint32).view(np.int32)
    codes, lutb, share = _renumbered(vals, idx, thr, freq, 4095)
    _set_env(monkeypatch, KS_NO_LINES=1, KS_EXT_MAX_J=5, **({"KS_EXT_ESCAPE_MAX": "1.0"} if share > 0.01 else {}))
    assert (share == 0.0) == (nd <= 4095)
    t = D.DeviceTable(ctx, w, k, thr, compress=True, expand=True,
                      freq=torch.from_numpy(freq).cuda() if hint else None)
    try:
        assert _form(t) == (0, 0, 5, 12, True), _form(t)
        assert t.distinct == nd
        assert abs(t.escape_fraction - share) <= 1e-12, (t.escape_fraction, share)
        got_codes = t.debug_read("codes")
        assert np.array_equal(t.debug_read("lut", dtype=np.uint64), lutb)
        assert np.array_equal(got_codes, codes)
        lut12 = np.zeros(4096, dtype=np.uint64)
        lut12[:min(nd, 4096)] = lutb[:4096]
        assert np.array_equal(t.debug_read("lut12", dtype=np.uint64), lut12)
        assert np.array_equal(t.debug_read("map12"), np.arange(4096, dtype=np.uint16))
        nent = 4 ** (k + 4)
        seams = _ext_seams(nent, 1, 2, 8, cus)
        ncmp = _compare(t, "ext", nent, 8, seams, lambda e: TR.ext_c12(got_codes, k, e), seed=nd)
        assert ncmp == (nent if nent * 8 <= WHOLE else (2 + len(seams)) * SLAB + 65536)
        if nd > 4095:  # some compared entry holds an escape, and the code 4094 beside it
            assert (got_codes >= 4095).any() and (got_codes == 4094).any()
    finally:
        t.close()


# ---------------------------------------------------------- 128-B wide lines

def _wide_check(t, k, codes_acc, seed):
    own = 16 - k
    n = 1 << 30
    seams = _line_seams(k, 15, 3)
    ncmp = _compare(t, "ext", n, 128, seams, lambda x: TR.lines_wide(codes_acc, k, own, x), seed=seed)
    assert ncmp == (2 + len(seams)) * SLAB + 65536 and len(seams) >= 4
    return ncmp


@pytest.mark.parametrize("k,nd", [(12, 2047), (12, 2048), (12, 5000), (13, 7168), (13, 7169)])
def test_wide_lines_host(ctx, monkeypatch, k, nd):
    """Wide lines from a host table: at most 2,047 distinct values (no
    escape), exactly 2,048, about 5,000 with an escape share in (0.01, 0.10]
    computed by the model before the build, 7,168 (the last wide form) and
    7,169 (64-B lines)."""
    from kmer_spans_amd import device as D
    _set_env(monkeypatch)
    n = 4 ** k
    vals, idx = _table_with(nd, n, k + nd, skew=0.95, nhead=2047)
    w, thr = vals[idx], 0.02
    codes, lutb, share = _renumbered(vals, idx, thr, None, 2047)
    if nd <= 2047:
        assert share == 0.0
    elif nd == 2048:
        assert 0.0 < share < 0.01
    else:
        assert 0.01 < share <= 0.10, share
    t = D.DeviceTable(ctx, w, k, thr, compress=True, expand=True)
    try:
        if nd > 7168:
            own = 16 - k
            assert _form(t) == (1, own, own + 2, 16, True), _form(t)
            base, _ = _check_base(t, w - thr)   # (not renumbered)
            m = k + own - 1
            ncmp = _compare(t, "ext", 4 ** m, 64, _line_seams(k, m, 2), lambda x: TR.lines_u16(base, k, own, x))
            assert ncmp == (2 + len(_line_seams(k, m, 2))) * SLAB + 65536
            return
        assert _form(t) == (3, 16 - k, 16 - k + 3, 13, True), _form(t)
        assert t.distinct == nd and abs(t.escape_fraction - share) <= 1e-12, (t.escape_fraction, share)
        assert np.array_equal(t.debug_read("lut", dtype=np.uint64), lutb)
        got_codes = t.debug_read("codes")
        assert np.array_equal(got_codes, codes)
        assert t.debug_bytes("lut12") == 0 and t.debug_bytes("map12") == 0
        _wide_check(t, k, got_codes, nd)
    finally:
        t.close()


def _device_counts(k, nd, tail_share, seed):
    """4^k device counts with nd distinct values: the first 2,047 values take
    all but tail_share of the k-mers.  No host array of 4^k."""
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    n = 4 ** k
    values = torch.cat([torch.arange(1000, 1000 + 2047), torch.arange(4000, 4000 + nd - 2047)]).to(torch.int32).cuda()
    idx = torch.randint(0, 2047, (n,), generator=g, device="cuda", dtype=torch.int32)
    step = 1 << 26
    for lo in range(0, n, step):  # (in steps: the mask and the tail draw stay small)
        tail = torch.rand(step, generator=g, device="cuda") < tail_share
        alt = torch.randint(2047, nd, (step,), generator=g, device="cuda", dtype=torch.int32)
        idx[lo:lo + step] = torch.where(tail, alt, idx[lo:lo + step])
    counts = values[idx.long()] if n <= (1 << 28) else torch.cat([values[idx[lo:lo + step].long()]
                                                                   for lo in range(0, n, step)])
    return counts


@pytest.mark.parametrize("k", [14, 15])
def test_wide_lines_from_device_counts(ctx, monkeypatch, k):
    """k = 14, 15 (own 2, 1): counts drawn on the device, the log2 table from
    them; the hint is the counts, so the weight of a value is count x
    multiplicity.  The model takes the multiplicities from a device histogram
    and reads code slabs through the window."""
    import torch
    from kmer_spans_amd import device as D
    _set_env(monkeypatch)
    torch.cuda.empty_cache()
    nd = 5000
    counts = _device_counts(k, nd, 0.03, k)
    mult = torch.bincount(counts).cpu().numpy()
    dv = np.flatnonzero(mult)
    assert dv.size == nd
    share = TR.escape_share(dv * mult[dv], 2047)
    assert 0.01 < share <= 0.10, share
    t = D.DeviceTable.from_counts(ctx, counts, k, "log2", expand=True)
    try:
        assert _form(t) == (3, 16 - k, 16 - k + 3, 13, True), _form(t)
        assert t.distinct == nd and abs(t.escape_fraction - share) <= 1e-12, (t.escape_fraction, share)
        # log2 rises with the count: the LUT in value order is the counts in order; the old codes
        # are the values in unsigned bit order, the new ones by weight with ties by old code
        lut = t.debug_read("lut")
        assert np.isfinite(lut).all() and np.unique(lut).size == nd
        by_value = np.argsort(lut)                                   # new code of the i-th smallest count
        old_of_new = np.argsort(np.argsort(lut.view(np.uint64)))     # old code of each new code
        wt_new = np.empty(nd, dtype=np.int64)
        wt_new[by_value] = dv * mult[dv]
        wt_old = np.empty(nd, dtype=np.int64)
        wt_old[old_of_new] = wt_new
        order, _ = TR.renumber(wt_old)
        assert np.array_equal(order, old_of_new), "d_lut is not in weight order (ties by old code)"
        code_of_count = np.zeros(int(dv[-1]) + 1, dtype=np.uint16)
        code_of_count[dv] = by_value

        def codes_acc(lo, cnt):
            got = t.debug_read("codes", lo, cnt)
            assert np.array_equal(got, code_of_count[counts[lo:lo + cnt].cpu().numpy()]), ("d_codes", lo, cnt)
            return got

        _wide_check(t, k, codes_acc, k)
    finally:
        t.close()
        del counts
        torch.cuda.empty_cache()


# ------------------------------------------------------------ rank-code lines

@pytest.mark.parametrize("k", [13, 14, 15])
def test_rank_code_lines(ctx, cus, monkeypatch, k):
    """Every sampled 128-B line's 32-bit codes decode through d_rpieces
    (base[piece] + offset x inc) to the bits of w_out of the k-mer the layout
    gives that dword; dwords past own + 19 are zero.  The FP64 form beside
    them is sampled the same way against w_out - thr."""
    import torch
    from kmer_spans_amd import device as D
    _set_env(monkeypatch)
    torch.cuda.empty_cache()
    g = torch.Generator(device="cuda")
    g.manual_seed(k)
    n, own, thr = 4 ** k, 16 - k, 0.75
    counts = torch.randint(0, 4, (n,), generator=g, device="cuda", dtype=torch.int32)
    counts[::4099] = 77
    counts[5::65537] = 30000
    total = float(counts.sum(dtype=torch.int64).item())
    w = torch.empty(n, dtype=torch.float64, device="cuda")
    t = D.DeviceTable.from_counts(ctx, counts, k, "rank", total=total, thr=thr, expand=True, w_out=w)
    try:
        p = t.debug_props()
        assert t.line_kind == 4 and t.positions_per_read == 18 - k and not t.compressed
        assert (p["line_kind"], p["line_own"], p["ext_J"], p["ext_bits"]) == ((2, 3, 4, 64) if k == 13 else (0, 0, 2, 64)), p
        pieces = t.debug_read("rpieces").reshape(-1, 2)
        assert pieces.shape[0] == p["n_rpieces"] > 0

        def wbits(idx, sub=0.0):
            v = w[torch.from_numpy(np.ascontiguousarray(idx)).cuda()]
            return (v - sub if sub else v).cpu().numpy().view(np.uint64)

        nl = 1 << 30
        seams = _line_seams(k, 15, 2)
        done = 0
        for lo, cnt in _ranges(nl, 128, seams, k):
            x = np.arange(lo, lo + cnt, dtype=np.int64)
            got = t.debug_read("rlines", lo * 32, cnt * 32).reshape(cnt, 32)
            assert not got[:, own + 20:].any(), ("pad", lo)
            c = got[:, :own + 20].astype(np.uint64)
            piece, off = c >> np.uint64(18), c & np.uint64((1 << 18) - 1)
            assert int(piece.max()) < pieces.shape[0]
            pi = piece.astype(np.int64)
            bits = pieces[pi, 0] + off * pieces[pi, 1]
            want = wbits(TR.line_slot_kmers(x, k, own, 2))
            if not np.array_equal(bits, want):
                r, s = np.argwhere(bits != want)[0]
                pytest.fail(f"rank line {lo + r} dword {s}: decodes to {bits[r, s]:#x}, w_out has {want[r, s]:#x}")
            done += cnt
        assert done == (2 + len(seams)) * SLAB + 65536 and len(seams) >= 4
        # the FP64 form of the later passes
        vals = lambda lo_, n_: (w[lo_:lo_ + n_] - thr).cpu().numpy()  # noqa: E731
        if k == 13:
            m = 15
            ncmp = _compare(t, "ext", 4 ** m, 64, _line_seams(k, m, 1), lambda x: TR.lines_f64(vals, k, 3, x), seed=k)
        else:
            nent = 4 ** (k + 1)
            ncmp = _compare(t, "ext", nent, 16, _ext_seams(nent, 1, 1, 1, cus), lambda e: TR.ext_f64(vals, k, 2, e),
                            seed=k)
        assert ncmp >= 2 * SLAB + 65536
    finally:
        t.close()
        del counts, w
        torch.cuda.empty_cache()


# ----------------------------------------------------------- binade predictor

@pytest.mark.parametrize("hint", [False, True])
@pytest.mark.parametrize("k", [5, 8, 9, 10, 13])
def test_binade_predictor(ctx, monkeypatch, k, hint):
    """kp = k (the values themselves), the lane walk (k = 8, 9) and the wave
    walk (k >= 10).  The kernel sums the mean in FP64 in another order than
    the model, so the two agree to about 1e-13 relative before the rounding
    to FP16 and may land on either side of a rounding boundary, no further:
    one FP16 ulp.  Exact where one k-mer enters the mean; 0 where none does."""
    import torch
    from kmer_spans_amd import device as D
    _set_env(monkeypatch, KS_NO_LINES=1, KS_EXT_MAX_J=2)
    rng = np.random.default_rng(k + 100 * hint)
    n, kp = 4 ** k, min(k, 7)
    sub = 4 ** (k - kp)
    w = rng.integers(-400, 400, n) / 16.0 + 1.0
    w[rng.integers(0, n, n // 50)] = np.nan
    w[rng.integers(0, n, n // 50)] = -np.inf
    freq = None
    if hint:
        freq = rng.geometric(0.2, n).astype(np.int64)
        freq[rng.integers(0, n, n // 4)] = 0
        freq[n // 3] = (1 << 31) + 5
    if sub > 1:  # prefix 1: one finite k-mer; prefix 2: none; prefix 3: finite ones without weight
        w[sub:2 * sub] = np.nan
        w[sub + sub // 2] = 0.3
        w[2 * sub:3 * sub] = [np.nan, np.inf, -np.inf, np.nan] * (sub // 4)
        if hint:
            freq[sub + sub // 2] = 7
            freq[3 * sub:4 * sub] = 0
            w[3 * sub:4 * sub] = 2.0
    fi = None if freq is None else freq.astype(np.uint32).view(np.int32)
    thr = 0.25
    t = D.DeviceTable(ctx, w, k, thr, compress=True, expand=True, freq=torch.from_numpy(fi).cuda() if hint else None)
    try:
        assert _form(t) == (0, 0, 2, 16, True) and t.debug_props()["approx_k"] == kp
        got = t.debug_read("approx")
        assert got.size == 4 ** kp
        mean, cnt = TR.approx(w - thr, k, fi)
        want = TR.to_f16_bits(mean)
        assert int(TR.f16_ulps(got, want).max()) <= 1
        one = cnt == 1
        assert one.any() and np.array_equal(got[one], want[one])
        assert np.array_equal(got[cnt == 0], np.zeros(int((cnt == 0).sum()), dtype=np.uint16))
        if sub > 1:
            assert cnt[1] == 1 and cnt[2] == 0 and (not hint or cnt[3] == 0)
        else:
            assert (cnt <= 1).all() and (cnt == 0).any()
    finally:
        t.close()
