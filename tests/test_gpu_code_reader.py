"""The kept-code reader's walk (ks_scan_chunked.hip, k_pass1c, code_index): a
wave walks its steps without bounds tests when its 64 lanes are full chunks,
walks the carried heads as selects on a carried mask, classifies values only
when the LUT holds a non-finite one, derives open and close from a carried
S > 0 mask and evaluates the candidate test only behind a condition it
implies.  None of that is a result: every scan below is compared
bit for bit with the CPU oracle (regions, score bits, visit histogram), and
ks_seq_index_codes_info / ks_seq_index_entry_info say that the scans under test
did read the codes and fell back nowhere.

The tables depend on the k-mer's last base only (tests/scanplant.py), so the
value at a scan index is chosen by one byte: a run is k - 1 bytes of lead-in
and one byte per scan index (kmer_regions: and one byte nothing scores; tr_lr:
index 0 takes the first-k-mer table's value of its byte).  Runs are laid out so
that chunk c is lane c % 64 of wave c / 64: every tile below is 64 chunks."""
import numpy as np
import pytest

from tests import test_gpu_entry_hint as H
from tests import test_gpu_kept_codes as KC

pytestmark = pytest.mark.gpu

CH = 256
D = 2  # kCodeDepth: steps per batch of the reader
INF, NAN = float("inf"), float("nan")
# (A, C, T, G): the value of the k-mer's last base
VALS = {
    "DY": (1.0, -1.0, -1e6, 0.5),         # exact sums; T resets
    "DRIFT": (0.7, -0.6, -1e6, 0.35),     # inexact sums
    "ZERO": (1.25, -1.25, -0.0, 0.0),     # both zeros in the LUT, no reset (not integers: those take the exact pass)
    "PINF": (1.0, -1.0, -1e6, INF),
    "NINF": (1.0, -1.0, -1e6, -INF),
    "NAN": (1.0, -1.0, -1e6, NAN),
}
# tr_lr's first-k-mer table.  (tr_lr with a NaN or +Inf in either table is the lane-per-run scan's, scan_algo 0:
# of the non-finite values only -Inf reaches the chunked scan and so the reader.)
INIT = {"FIN": (2.0, -1.0, -1e6, 0.25), "NINF": (2.0, -1.0, -1e6, -INF)}
# (min_width, min_score), tr_lr: min_length.  The first of each keeps the most candidates: the general scan runs
# with it, so the candidate and rescan buffers have grown before the scans under test (a call that has to grow
# them runs again on the general path, which reads no codes).  Planted: 'A' * w + 'T' has width w - 1 and score
# w (DY), w = 3 .. 7.
REGION_PARAMS = [(1, 0.5), (4, 5.0), (5, 5.0), (4, 6.0)]
TRLR_PARAMS = [1, 4, 5, 100]


def _table(v, k):
    return np.array(v, dtype=np.float64)[np.arange(4 ** k, dtype=np.int64) & 3]


@pytest.fixture(scope="module")
def ctx():
    from kmer_spans_amd import _lib, device as Dv
    c = _lib.Context(0)
    Dv.bind_torch_stream(c)
    c.set_scan_algo(1)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for name in KC.SWITCHES:
        monkeypatch.delenv(name, raising=False)


class _Tabs:
    """One score table at a time (the k = 12 line table is large), by (form, value set)."""

    def __init__(self):
        self.key, self.tab = None, None

    def get(self, ctx, form, wname):
        from kmer_spans_amd import device as Dv
        if self.key != (form, wname):
            self.close()
            k, _, kernel, line_kind = H.FORMS[form]
            t = Dv.DeviceTable(ctx, _table(VALS[wname], k), k, 0.0, compress=True, expand=True)
            assert (t.pass1_kernel, t.line_kind, t.compressed) == (kernel, line_kind, True), (form, wname)
            self.key, self.tab = (form, wname), t
        return self.tab

    def close(self):
        if self.tab is not None:
            self.tab.close()
        self.key, self.tab = None, None


@pytest.fixture(scope="module")
def tabs():
    t = _Tabs()
    yield t
    t.close()


# ------------------------------------------------------------------ corpus

class _Plant:
    """Runs of planted bytes, tile by tile.  rare_g: G (the value sets' fourth
    value, the non-finite one) occurs only where it is planted."""

    def __init__(self, J, seed, rare_g):
        self.J, self.rng, self.rare_g = J, np.random.default_rng(seed), rare_g
        self.runs = []   # bytes per run: one byte per scan index
        self.nch = 0

    def rand(self, n):
        p = (0.40, 0.50, 0.10, 0.0) if self.rare_g else (0.34, 0.32, 0.04, 0.30)
        return np.frombuffer(b"ACTG", dtype=np.uint8)[self.rng.choice(4, size=n, p=p)].tobytes()

    def open_end(self, n=CH):
        """n indices that end inside an excursion whose first argmax is the last index."""
        return self.rand(n - 3) + b"AAA"

    def clamp(self, q):
        """A full chunk whose carried head clamps at index q, open at its end (q = 255: clean at its end)."""
        body = b"A" * q + b"T"
        rest = CH - len(body)
        return body + (self.rand(rest - 3) + b"AAA" if rest >= 3 else b"A" * rest)

    def run(self, *chunks):
        body = b"".join(chunks)
        self.runs.append(bytearray(body))
        self.nch += (len(body) + CH - 1) // CH
        return self.runs[-1]

    def end_tile(self):
        assert self.nch % 64 == 0, self.nch

    # -- tiles
    def tile_full(self):
        """64 full chunks of one run: all heads but the first, clamping within a few indices at random."""
        self.run(*[self.open_end() if j % 3 else self.rand(CH) for j in range(64)])
        self.end_tile()

    def tile_heads(self):
        """One run of 64 full chunks: the heads of its lanes clamp at index 0, 1,
        J - 1, J, D J - 1, D J and 255, and over three chunks never ('G' * 256,
        'AC' * 128 -- its maximum ties from index 0 on, and on the clean
        trajectory every index opens or closes -- and 'G' * 256)."""
        J = self.J
        qs = [0, 1, J - 1, J, D * J - 1, D * J, 255]
        chunks = [self.open_end()]
        for j in range(1, 64):
            if j in (20, 40):
                chunks.append(b"A" * CH if self.rare_g else b"G" * CH)
            elif j in (21, 41):
                chunks.append(b"AC" * (CH // 2))
            elif j in (22, 42):
                chunks.append(b"A" * CH if self.rare_g else b"G" * CH)
            else:
                chunks.append(self.clamp(qs[j % 7]))
        r = self.run(*chunks)
        self.end_tile()
        return r

    def tile_one_head(self, lane):
        """63 clean lanes and one (lane) whose head never clamps."""
        for _ in range(lane - 1):
            self.run(self.rand(CH))
        self.run(self.open_end(), b"A" * 100 + b"AC" * 78)
        for _ in range(63 - lane):
            self.run(self.rand(CH))
        self.end_tile()

    def tile_short(self, lane, n):
        """Full chunks but lane's, which has n indices (and, lane > 0, a carried head)."""
        self.run(*([self.open_end() for _ in range(lane)] + [self.open_end(n) if n >= 3 else b"A" * n]))
        if lane < 63:
            self.run(*[self.open_end() for _ in range(63 - lane)])
        self.end_tile()

    def tile_clean(self):
        """64 one-chunk runs (every lane enters at 0): excursions that open and
        close at every position of a step, on consecutive indices, at the last
        index; ties; exact cancellation; widths and scores at the thresholds."""
        J = self.J
        pats = [b"AC" * (CH // 2), b"C" + b"AC" * 127 + b"A", self.rand(250) + b"AAAAAT", self.open_end()]
        for o in range(2 * J):  # 'A' * w + 'C' * w returns to exactly 0, at every offset of a step
            body = b"T" * o
            w = 1
            while len(body) < CH:
                body += b"A" * w + b"C" * w
                w = w % 7 + 1
            pats.append(body[:CH])
        for o in range(J):  # width w - 1 and score w, w = 3 .. 7, around (4, 5.0)
            body = b"C" * o
            while len(body) < CH:
                for w in (3, 4, 5, 6, 7):
                    body += b"A" * w + b"T"
            pats.append(body[:CH])
        pats.append((b"AACA" + b"T") * 51 + b"T")          # equal maxima: the first is kept
        pats.append((b"GT" * 3 + b"ACGTCA") * 21 + b"GTGT")  # zeros of both signs between and inside excursions
        assert len(pats) <= 64 and all(len(p) == CH for p in pats), [len(p) for p in pats]
        for p in pats:
            self.run(p)
        for _ in range(64 - len(pats)):
            self.run(self.rand(CH))
        self.end_tile()

    def tail(self, m):
        """m one-chunk runs: the last wave is partly dead."""
        for j in range(m):
            self.run(self.rand(CH) if j % 2 else self.open_end(CH - j % 5))


def _corpus(J, tail, rare_g, seed):
    """The runs (one byte per scan index) of the whole corpus, and those that go
    to the second sequence."""
    P = _Plant(J, seed, rare_g)
    P.tile_full()
    heads = P.tile_heads()
    P.tile_one_head(17)
    lanes = [0, 31, 63]
    for j, n in enumerate([1, J - 1, J, J + 1, D * J - 1, D * J, 252, 253, 255]):
        P.tile_short(lanes[j % 3], n)
    for lane in (31, 63, 0):  # every lane with an n of its own kind as well
        P.tile_short(lane, 1)
    P.tile_clean()
    if rare_g:  # the fourth value inside a head's walk (chunk 5 clamps at index J), after it, and on clean lanes
        heads[5 * CH + 1] = ord("G")
        heads[9 * CH + 100] = ord("G")
        heads[30 * CH + 255] = ord("G")
        P.runs[-3][7] = ord("G")
        P.runs[-2][0] = ord("G")  # (tr_lr: the first k-mer of a run, the first-k-mer table's value)
    first = len(P.runs)
    P.tail(tail)
    assert P.nch % 64 == tail
    return P.runs, first


def _sequences(runs, first, k, trlr):
    lead = b"T" * (k - 1)
    end = b"" if trlr else b"T"
    a = b"N".join(lead + bytes(r) + end for r in runs[:first])
    b = b"NN" + b"NNN".join(lead + bytes(r) + end for r in runs[first:]) + b"N"
    return [a, b]


# ------------------------------------------------------------------ the checked scans

def _check_case(oracle, ctx, tabs, form, mode, wname, iname, tail):
    from kmer_spans_amd import device as Dv
    k = H.FORMS[form][0]
    tab = tabs.get(ctx, form, wname)
    J = tab.positions_per_read
    trlr = mode == "tr_lr"
    rare_g = wname in ("PINF", "NINF", "NAN") or iname != "FIN"
    runs, first = _corpus(J, tail, rare_g, 17 * J + tail)
    seqs = _sequences(runs, first, k, trlr)
    ds = Dv.from_host(seqs, "cuda")
    w = _table(VALS[wname], k)
    init = Dv.DeviceTable(ctx, _table(INIT[iname], k), k, 0.0, compress=False, expand=False) if trlr else None
    params = [(m, 0.0) for m in TRLR_PARAMS] if trlr else REGION_PARAMS
    try:
        def scan(mw, ms, visits, what):
            if trlr:
                o = oracle.tr_lr_regions(seqs, k, mw, _table(INIT[iname], k), w)
                pos, sc, st = Dv.tr_lr(ctx, ds, k, tab, init, mw)
                vis = None
            else:
                o = oracle.scan(seqs, k, w, 0.0, mw, ms, visits=True)
                if visits:
                    pos, sc, st, vis = H._scan(ctx, ds, k, tab, mw, ms)
                else:
                    pos, sc, st = Dv.scan(ctx, ds, k, tab, mw, ms, None)
                    vis = None
            assert st["scan_algo"] == 1
            H._equal(pos, sc, vis, o, what)
            return pos.shape[1]

        tag = f"{form} {mode} {wname}/{iname} J={J} tail={tail}"
        # the general scan (which runs again where it has to grow a buffer) and the writer
        for i in range(3):
            scan(*params[0], False, tag + f" scan {i}")
        assert KC._codes(ds)["code_builds"] == 1, (tag, KC._codes(ds))

        def reader(mw, ms, visits):
            """A scan that must read the kept codes: code_reuses advances, nothing falls back."""
            before, e0 = KC._codes(ds), KC._entry(ds)
            found = scan(mw, ms, visits, tag + f" reader {mw}/{ms} visits={visits}")
            want = dict(before, code_reuses=before["code_reuses"] + 1)
            assert want["code_fallbacks"] == 0 and want["code_alloc_failures"] == 0, (tag, before)
            assert KC._codes(ds) == want, (tag, mw, ms, visits)
            assert KC._entry(ds) == {"entry_reuses": e0["entry_reuses"] + 1, "entry_fallbacks": 0}, (tag, mw, ms)
            return found

        found = sum(reader(mw, ms, False) for mw, ms in params)
        if not trlr:
            found += reader(*params[1], True)
        assert found > 0, tag  # (the thresholds are not past every plant)
    finally:
        if init is not None:
            init.close()


_REGIONS = [(f, w, t) for f in ("lines-u16", "wide")
            for w, t in (("DY", 1), ("DRIFT", 63), ("ZERO", 1), ("PINF", 63), ("NINF", 1), ("NAN", 63))]


@pytest.mark.parametrize("form,wname,tail", _REGIONS, ids=[f"{f}-{w}-tail{t}" for f, w, t in _REGIONS])
def test_reader_walks_kmer_regions(oracle, ctx, tabs, form, wname, tail):
    """Wave variants (full tiles, one short chunk of every length class at lane
    0, 31 or 63, a partly dead last wave), the head phase (clamps at every
    index class, never, one unclamped lane among 63 clean ones), the lean clean
    step's plants and thresholds, and tables with and without non-finite
    values: four thresholds without the visit histogram and one scan with it,
    all reading the kept codes."""
    _check_case(oracle, ctx, tabs, form, "kmer_regions", wname, "FIN", tail)


_TRLR = [("lines-u16", "DY", "FIN", 1), ("lines-u16", "DRIFT", "FIN", 63), ("lines-u16", "ZERO", "FIN", 63),
         ("lines-u16", "NINF", "FIN", 63), ("lines-u16", "DY", "NINF", 1), ("lines-u16", "NINF", "NINF", 63),
         ("wide", "DY", "FIN", 63), ("wide", "DY", "NINF", 1)]


@pytest.mark.parametrize("form,wname,iname,tail", _TRLR, ids=[f"{f}-{w}-{i}-tail{t}" for f, w, i, t in _TRLR])
def test_reader_walks_tr_lr(oracle, ctx, tabs, form, wname, iname, tail):
    """The same corpus as tr_lr scans, min_length 1, 4, 5 and 100: every run's
    first chunk takes the first-k-mer table's value at index 0 (iname NINF: a
    non-finite one, also where the transition table's LUT has none)."""
    _check_case(oracle, ctx, tabs, form, "tr_lr", wname, iname, tail)


@pytest.mark.parametrize("wname,iname", [("NAN", "FIN"), ("PINF", "FIN"), ("DY", "NAN")])
def test_tr_lr_nan_and_plus_inf_are_the_lane_scans(oracle, ctx, tabs, wname, iname):
    """The premise of _TRLR's value sets: a tr_lr call with a NaN or +Inf in
    either table is routed to the lane-per-run scan (scan_algo 0), reads no
    codes however often it is repeated, and equals the oracle."""
    from kmer_spans_amd import device as Dv
    form = "lines-u16"
    k = H.FORMS[form][0]
    tab = tabs.get(ctx, form, wname)
    runs, first = _corpus(tab.positions_per_read, 1, True, 5)
    seqs = _sequences(runs, first, k, True)
    ds = Dv.from_host(seqs, "cuda")
    vi = dict(INIT, NAN=(2.0, -1.0, -1e6, NAN))[iname]
    init = Dv.DeviceTable(ctx, _table(vi, k), k, 0.0, compress=False, expand=False)
    try:
        o = oracle.tr_lr_regions(seqs, k, 4, _table(vi, k), _table(VALS[wname], k))
        for i in range(3):
            pos, sc, st = Dv.tr_lr(ctx, ds, k, tab, init, 4)
            assert st["scan_algo"] == 0, (wname, iname, i)
            H._equal(pos, sc, None, o, f"tr_lr {wname}/{iname} scan {i}")
        assert KC._codes(ds) == KC._c(0, 0)
    finally:
        init.close()


@pytest.mark.parametrize("form", ["lines-u16", "wide"])
def test_two_parts_then_visits(oracle, ctx, tabs, monkeypatch, form):
    """Four copies of the tile corpus in two parts (KS_SPLIT_MIN_CHUNKS=0):
    readers without the visit histogram, then one with it."""
    from kmer_spans_amd import device as Dv
    tabs.close()  # (one k = 12 line table at a time)
    tables = H._Tables()
    try:
        c = KC._case(oracle, ctx, tables, monkeypatch, form, "tile", "DRIFT", 2)
        for i in range(4):
            mw, ms = KC.PARAMS[i % 3]
            o = H._oracle(oracle, c.seqs_key, c.seqs, c.k, "A", "DRIFT", "kmer_regions", mw, ms)
            pos, sc, st = Dv.scan(ctx, c.ds, c.k, c.tab("A"), mw, ms, None)
            H._equal(pos, sc, None, o, f"{form} two parts without visits {i}")
        assert KC._codes(c.ds) == KC._c(1, 2)
        c.regions("A", *KC.PARAMS[1], f"{form} two parts with visits")
        assert KC._codes(c.ds) == KC._c(1, 3)
        assert KC._entry(c.ds) == {"entry_reuses": 4, "entry_fallbacks": 0}
    finally:
        tables.close()
