"""The kept per-index codes (ks_scan_chunked.hip, ChunkKeep::codes_ok): the
first scan of a sequence index that starts from exact entries -- scan #2 of a
genome / table pair -- also writes the uint16 value code of every scan index
(k_pass1w / k_pass1l, kStore), and the scans after it stream those codes
(k_pass1c) instead of reading the table's lines.

The codes are never a result: every scan below -- general path, writer, reader,
with spoilt codes (KS_TEST_KEPT_CODES) and after every change of key -- is
compared bit for bit with the CPU oracle (regions, score bits, visit
histogram), and ks_seq_index_codes_info says which path each call took.  The
writer is pinned apart from the reader: the read window gives the kept codes in
index order, and they must be the table's base codes at the k-mers sliced from
the sequences.  Corpora, tables and the oracle's results are tests/scanplant.py's
and test_gpu_entry_hint.py's; the seam corpus below is this file's."""
import numpy as np
import pytest

from tests import test_gpu_entry_hint as H

pytestmark = pytest.mark.gpu

PARAMS = H.PARAMS
CORPORA = H.CORPORA
CODE_SWITCHES = ("KS_NO_KEPT_CODES", "KS_TEST_KEPT_CODES", "KS_TEST_KEPT_CODES_NOMEM", "KS_NO_EXACT_ENTRY")
SWITCHES = H.SWITCHES + CODE_SWITCHES
FOUR = 4  # copies of the tile corpus that make a scan split in two parts (test_gpu_exact_entry.py)
CH = 256


@pytest.fixture(scope="module")
def ctx():
    from kmer_spans_amd import _lib, device as D
    c = _lib.Context(0)
    D.bind_torch_stream(c)
    c.set_scan_algo(1)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


@pytest.fixture(scope="module")
def tables():
    t = H._Tables()
    yield t
    t.close()


def _case(oracle, ctx, tables, monkeypatch, form, seam, vset, parts):
    if parts == 2:
        monkeypatch.setenv("KS_SPLIT_MIN_CHUNKS", "0")
    c = H._Case(oracle, ctx, tables, monkeypatch, form, seam, vset, repeat=FOUR if parts == 2 else 1)
    if parts == 2:
        assert sum(len(s) for s in c.seqs) // 256 > 2 * 3072
    return c


def _codes(ds):
    return ds.seq_index().codes_info()


def _c(builds, reuses, fallbacks=0, nomem=0):
    return {"code_builds": builds, "code_reuses": reuses, "code_fallbacks": fallbacks, "code_alloc_failures": nomem}


def _entry(ds):
    return ds.seq_index().entry_info()


# ------------------------------------------------------------------ 1. path sequence

_FOUR_SCANS = [(f, s, v, 1, "kmer_regions") for f in ("lines-u16", "wide") for s, v in CORPORA] + \
              [("lines-u16", s, v, 1, "tr_lr") for s, v in CORPORA] + \
              [("lines-u16", "tile", "DRIFT", 2, "kmer_regions"), ("wide", "tile", "DRIFT", 2, "kmer_regions"),
               ("lines-u16", "tile", "DRIFT", 2, "tr_lr")]


@pytest.mark.parametrize("form,seam,vset,parts,mode", _FOUR_SCANS, ids=["-".join(map(str, x)) for x in _FOUR_SCANS])
def test_four_scans_general_writer_reader_reader(oracle, ctx, tables, monkeypatch, form, seam, vset, parts, mode):
    """One DeviceSeqs, one table, three thresholds and a fourth scan (the first
    thresholds again; kmer_regions scans all carry the visit histogram, which
    k_pass1c then counts from its own key walk).  Scan 0: general path.  Scan 1:
    exact entries, writes the codes.  Scans 2 and 3 read them and replay nothing."""
    c = _case(oracle, ctx, tables, monkeypatch, form, seam, vset, parts)
    for i, (mw, ms) in enumerate(PARAMS + PARAMS[:1]):
        what = f"{seam}/{vset} {form} parts {parts} {mode} scan {i}"
        st = c.regions("A", mw, ms, what) if mode == "kmer_regions" else c.tr_lr("A", "init", mw, what)
        assert (st["n_replay"] > 0) == (i == 0), (what, st["n_replay"])
        assert _codes(c.ds) == _c(min(i, 1), max(i - 1, 0)), what
        assert _entry(c.ds) == {"entry_reuses": i, "entry_fallbacks": 0}, what
        assert H._info(c.ds) == H._counts(i, i, 1), what


@pytest.mark.parametrize("form", ["lines-u16", "wide"])
def test_reader_without_then_with_visits(oracle, ctx, tables, monkeypatch, form):
    """The visit histogram is no part of the key: both flavours of the reader."""
    from kmer_spans_amd import device as D
    c = _case(oracle, ctx, tables, monkeypatch, form, "tile", "DRIFT", 1)
    mw, ms = PARAMS[0]
    o = H._oracle(oracle, c.seqs_key, c.seqs, c.k, "A", "DRIFT", "kmer_regions", mw, ms)
    for i in range(3):
        pos, sc, st = D.scan(ctx, c.ds, c.k, c.tab("A"), mw, ms, None)
        H._equal(pos, sc, None, o, f"{form} without visits {i}")
    assert _codes(c.ds) == _c(1, 1)
    c.regions("A", mw, ms, f"{form} with visits")
    assert _codes(c.ds) == _c(1, 2)


# ------------------------------------------------------------------ 2, 3. the writer pinned, seams

# Lengths in scan indices (kmer_regions) of the seam corpus's runs: the chunk
# lengths n of the issue, one index alone, 256 = 42 x 6 + 4 (the partial last
# step of J = 6; every n below is partial for some J of 4 .. 7), two- and
# three-chunk runs whose last chunk is short, and a tile and a bit.
_SEAM_RUNS = [1, 3, 4, 5, 15, 16, 17, 255, 256, 257, 256 + 15, 512 + 1, 2, 64 * 256 + 5, 7, 255, 256 * 3]


def _seam_seqs(k, nch_mod, rng):
    """Runs of random bases separated by N, in two sequences, padded with
    one-chunk runs until the chunk count is nch_mod modulo 64."""
    lens = list(_SEAM_RUNS)
    nch = sum((p + CH - 1) // CH for p in lens)
    while nch % 64 != nch_mod:
        lens.append(int(rng.integers(1, 257)))
        nch += 1
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)
    runs = [bases[rng.integers(0, 4, size=p + k)].tobytes() for p in lens]
    runs.append(bases[rng.integers(0, 4, size=k)].tobytes())  # exactly k bases: no index (tr_lr: one)
    half = len(runs) // 2
    return [b"NN".join(runs[:half]), b"N" + b"N".join(runs[half:]) + b"NNN"], lens


def _expected_codes(seqs, k, base_codes, trlr):
    """Chunk by chunk, the base code of the k-mer of every live scan index:
    index i of a run [a, b) scores the k-mer of bytes [i - k, i), i = a + k ..
    b - 1 (tr_lr: .. b)."""
    enc = np.zeros(256, dtype=np.int64)
    for j, ch in enumerate(b"ACTG"):  # the library's base order
        enc[ch] = j
        enc[ch | 0x20] = j
    chunks = []
    for s in seqs:
        b = np.frombuffer(s if isinstance(s, bytes) else s.encode("latin-1"), dtype=np.uint8)
        isn = (b | 0x20) == ord("n")
        edges = np.flatnonzero(np.diff(np.concatenate(([1], isn.astype(np.int8), [1]))))
        for a, e in zip(edges[::2], edges[1::2]):
            if e - a <= k:  # (a run of exactly k bases: no index; tr_lr's one comes last and is not compared)
                continue
            P = e - a - k + (1 if trlr else 0)
            x = enc[b[a:e]]
            km = np.zeros(e - a - k + 1, dtype=np.int64)
            for t in range(k):
                km = km * 4 + x[t:t + len(km)]
            code = base_codes[km][:P]
            for c0 in range(0, P, CH):
                chunks.append(code[c0:c0 + CH])
    return chunks


_PINNED = [("lines-u16", "kmer_regions", 1), ("lines-u16", "kmer_regions", 0), ("lines-u16", "tr_lr", 63),
           ("wide", "kmer_regions", 63), ("wide", "kmer_regions", 0), ("wide", "kmer_regions", 1)]


@pytest.mark.parametrize("form,mode,nch_mod", _PINNED, ids=[f"{f}-{m}-nch{n}" for f, m, n in _PINNED])
def test_writer_pinned_at_seams(oracle, ctx, tables, monkeypatch, form, mode, nch_mod):
    """After scan 1 the read window's codes of every live index of every chunk
    are the table's base codes at the k-mer sliced from the sequence; scans 2
    (without visits) and 3 (with) read them and equal the oracle.  One part: the
    corpus is far below the 2,048 chunks a split needs (two parts, with a run
    boundary at the part cut: test_writer_pinned_in_two_parts)."""
    from kmer_spans_amd import device as D
    monkeypatch.setenv("KS_SPLIT_MIN_CHUNKS", "0")
    k = H.FORMS[form][0]
    rng = np.random.default_rng(100 * k + nch_mod)
    seqs, lens = _seam_seqs(k, nch_mod, rng)
    trlr = mode == "tr_lr"
    if form == "wide":  # the module's one wide table (128 GiB of lines: a second does not fit the budget)
        w = H._weights("A", "DRIFT", k)
        tab = tables.get(ctx, "wide", "DRIFT", "A", monkeypatch)
    else:               # 61 distinct values that depend on the whole k-mer
        w = ((np.arange(4 ** k, dtype=np.int64) * 2654435761 >> 7) % 61 - 33).astype(np.float64) / 8.0
        tab = D.DeviceTable(ctx, w, k, 0.0, compress=True, expand=True)
    init = D.DeviceTable(ctx, H._weights("init", "DRIFT", k), k, 0.0, compress=False, expand=False) if trlr else None
    try:
        assert tab.pass1_kernel == H.FORMS[form][2]
        ds = D.from_host(seqs, "cuda")
        mw, ms = 3, 2.0
        if trlr:
            o = oracle.tr_lr_regions(seqs, k, mw, H._weights("init", "DRIFT", k), w)
        else:
            o = oracle.scan(seqs, k, w, 0.0, mw, ms, visits=True)

        def scan(visits, what):
            if trlr:
                pos, sc, st = D.tr_lr(ctx, ds, k, tab, init, mw)
                vis = None
            elif visits:
                pos, sc, st, vis = H._scan(ctx, ds, k, tab, mw, ms)
            else:
                pos, sc, st = D.scan(ctx, ds, k, tab, mw, ms, None)
                vis = None
            H._equal(pos, sc, vis, o, what)

        scan(True, "scan 0")
        scan(True, "scan 1 (writer)")
        assert _codes(ds) == _c(1, 0)
        want = _expected_codes(seqs, k, tab.debug_read("codes"), trlr)
        assert len(want) % 64 == nch_mod or trlr
        got, J = D.kept_codes_read(ctx, 0, len(want))
        assert J == tab.positions_per_read
        for c, wc in enumerate(want):
            assert np.array_equal(got[c, :len(wc)], wc), (form, mode, "chunk", c, len(wc))
        with pytest.raises(Exception, match="outside the scan"):
            D.kept_codes_read(ctx, 0, len(want) + 2)  # (tr_lr: the run of exactly k bases is one more chunk)
        scan(False, "scan 2 (reader)")
        scan(True, "scan 3 (reader, visits)")
        assert _codes(ds) == _c(1, 2)
    finally:
        if form != "wide":
            tab.close()
        if init is not None:
            init.close()


@pytest.mark.parametrize("form", ["lines-u16", "wide"])
def test_writer_pinned_in_two_parts(oracle, ctx, tables, monkeypatch, form):
    """Four copies of the tile corpus split in two parts at a run boundary
    (KS_SPLIT_MIN_CHUNKS=0, more than 2 x 3,072 chunks): after the writer scan the
    read window of every chunk of both parts holds the table's base codes."""
    from kmer_spans_amd import device as D
    c = _case(oracle, ctx, tables, monkeypatch, form, "tile", "DRIFT", 2)
    for i in range(2):
        c.regions("A", *PARAMS[i], f"{form} two parts scan {i}")
    assert _codes(c.ds) == _c(1, 0)
    want = _expected_codes(c.seqs, c.k, c.tab("A").debug_read("codes"), False)
    assert len(want) > 2 * 3072
    got, J = D.kept_codes_read(ctx, 0, len(want))
    assert J == c.tab("A").positions_per_read
    for ci, wc in enumerate(want):
        assert np.array_equal(got[ci, :len(wc)], wc), (form, "chunk", ci, len(wc))
    with pytest.raises(Exception, match="outside the scan"):
        D.kept_codes_read(ctx, 0, len(want) + 1)
    c.regions("A", *PARAMS[2], f"{form} two parts reader")
    assert _codes(c.ds) == _c(1, 1)


# ------------------------------------------------------------------ 4. spoilt codes

_SPOILT = [("lines-u16", 1, "sample"), ("lines-u16", 2, "all"), ("lines-u16", 1, "one"), ("wide", 1, "sample"),
           ("wide", 1, "all"), ("wide", 2, "one")]


@pytest.mark.parametrize("form,parts,how", _SPOILT, ids=[f"{f}-{p}-{h}" for f, p, h in _SPOILT])
def test_spoilt_codes_fall_back(oracle, ctx, tables, monkeypatch, form, parts, how):
    """The kept codes spoilt before a reading call's pass 1: the sampled code
    (the tripwire, bit 128), every code, or one unsampled code of a chunk of the
    DRIFT corpus, whose carried sums do not clamp (the exact-entry check, bit
    64).  The call falls back to the hint path and equals the oracle; the next
    call writes the codes again and the one after reads them."""
    c = _case(oracle, ctx, tables, monkeypatch, form, "tile", "DRIFT", parts)
    for i in range(2):
        c.regions("A", *PARAMS[i], f"{form} scan {i}")
    assert _codes(c.ds) == _c(1, 0)
    monkeypatch.setenv("KS_TEST_KEPT_CODES", how)
    c.regions("A", *PARAMS[2], f"{form} codes spoilt: {how}")
    assert _codes(c.ds) == _c(1, 0, 1)
    assert _entry(c.ds) == {"entry_reuses": 1, "entry_fallbacks": 1}
    c.regions("A", *PARAMS[0], f"{form} rebuild (the hook spoils reading calls only)")
    assert _codes(c.ds) == _c(2, 0, 1)
    monkeypatch.delenv("KS_TEST_KEPT_CODES")
    st = c.regions("A", *PARAMS[1], f"{form} reads the rebuilt codes")
    assert st["n_replay"] == 0
    assert _codes(c.ds) == _c(2, 1, 1)


def test_spoilt_entries_on_a_reading_call_clear_the_codes(oracle, ctx, tables, monkeypatch):
    c = _case(oracle, ctx, tables, monkeypatch, "lines-u16", "tile", "DRIFT", 1)
    for i in range(3):
        c.regions("A", *PARAMS[i], f"scan {i}")
    assert _codes(c.ds) == _c(1, 1)
    monkeypatch.setenv("KS_TEST_ENTRY_HINT", "shift")
    c.regions("A", *PARAMS[0], "entries spoilt on a reading call")
    monkeypatch.delenv("KS_TEST_ENTRY_HINT")
    assert _codes(c.ds) == _c(1, 1, 1)
    c.regions("A", *PARAMS[1], "writes the codes again")
    assert _codes(c.ds) == _c(2, 1, 1)
    c.regions("A", *PARAMS[2], "and reads them")
    assert _codes(c.ds) == _c(2, 2, 1)


# ------------------------------------------------------------------ 5. keys

def _three(c, name="A"):
    for i in range(3):
        c.regions(name, *PARAMS[i], f"table {name} scan {i}")


def test_aba_tables_never_read_the_other_tables_codes(oracle, ctx, tables, monkeypatch):
    c = _case(oracle, ctx, tables, monkeypatch, "lines-u16", "tile", "DRIFT", 1)
    _three(c, "A")
    assert _codes(c.ds) == _c(1, 1)
    for i, name in enumerate("BAB"):
        c.regions(name, *PARAMS[i], f"table {name} after another")
        assert _codes(c.ds) == _c(1, 1), name
    c.regions("B", *PARAMS[0], "B again: writes")
    assert _codes(c.ds) == _c(2, 1)
    c.regions("B", *PARAMS[1], "B once more: reads")
    assert _codes(c.ds) == _c(2, 2)


def test_destroyed_table_is_another_table(oracle, ctx, tables, monkeypatch):
    from kmer_spans_amd import device as D
    c = _case(oracle, ctx, tables, monkeypatch, "lines-u16", "tile", "DRIFT", 1)
    k = c.k
    tab = D.DeviceTable(ctx, H._weights("A", "DRIFT", k), k, 0.0, compress=True, expand=True)
    try:
        for i in range(3):
            c.regions("A", *PARAMS[i], f"table A scan {i}", tab=tab)
        assert _codes(c.ds) == _c(1, 1)
        tab.close()
        tab = D.DeviceTable(ctx, H._weights("B", "DRIFT", k), k, 0.0, compress=True, expand=True)
        c.regions("B", *PARAMS[0], "table A'", tab=tab)
        assert _codes(c.ds) == _c(1, 1)
        c.regions("B", *PARAMS[1], "table A' again", tab=tab)
        assert _codes(c.ds) == _c(2, 1)
    finally:
        tab.close()


def test_tr_lr_keys_on_both_tables(oracle, ctx, tables, monkeypatch):
    c = _case(oracle, ctx, tables, monkeypatch, "lines-u16", "tile", "DRIFT", 1)
    for i in range(3):
        c.tr_lr("A", "init", PARAMS[i][0], f"init scan {i}")
    assert _codes(c.ds) == _c(1, 1)
    c.tr_lr("A", "init2", 1, "init2")
    assert _codes(c.ds) == _c(1, 1)
    c.tr_lr("A", "init2", 5, "init2 again")
    assert _codes(c.ds) == _c(2, 1)


def test_another_k_or_scan_kind_in_between(oracle, ctx, tables, monkeypatch):
    from kmer_spans_amd import device as D
    c = _case(oracle, ctx, tables, monkeypatch, "lines-u16", "tile", "DRIFT", 1)
    _three(c)
    t6 = D.DeviceTable(ctx, H._weights("A", "DRIFT", 6), 6, 0.0, compress=True, expand=True)
    try:
        c.regions("A", *PARAMS[0], "k 6", tab=t6, k=6)
    finally:
        t6.close()
    c.regions("A", *PARAMS[0], "k 9 again")
    c.tr_lr("A", "init", 1, "tr_lr")
    c.regions("A", *PARAMS[1], "kmer_regions after tr_lr")
    assert _codes(c.ds) == _c(1, 1)
    c.regions("A", *PARAMS[2], "once more: writes")
    assert _codes(c.ds) == _c(2, 1)


def test_larger_genome_in_between(oracle, ctx, tables, monkeypatch):
    small = H._Case(oracle, ctx, tables, monkeypatch, "lines-u16", "chunk", "DRIFT")
    big = H._Case(oracle, ctx, tables, monkeypatch, "lines-u16", "tile", "DRIFT", repeat=2)
    _three(small)
    assert _codes(small.ds) == _c(1, 1)
    _three(big)
    assert _codes(big.ds) == _c(1, 1)
    small.regions("A", *PARAMS[2], "small after big")
    assert _codes(small.ds) == _c(1, 1)
    small.regions("A", *PARAMS[0], "small again: writes")
    small.regions("A", *PARAMS[1], "small once more: reads")
    assert _codes(small.ds) == _c(2, 2)


def test_torch_write_gives_a_new_index_and_no_codes(oracle, ctx, tables, monkeypatch):
    c = _case(oracle, ctx, tables, monkeypatch, "lines-u16", "chunk", "DRIFT", 1)
    _three(c)
    old = c.ds.seq_index()
    c.ds.seq[40:43] = ord("N")
    c.seqs = [c.ds.host_seq(q) for q in range(c.ds.nseq)]
    c.seqs_key = c.seqs_key + ("written",)
    c.regions("A", *PARAMS[0], "after the write")
    assert c.ds.seq_index() is not old
    assert _codes(c.ds) == _c(0, 0)
    c.regions("A", *PARAMS[1], "writes")
    c.regions("A", *PARAMS[2], "reads")
    assert _codes(c.ds) == _c(1, 1)


class _DefaultCtx:
    """The process default context, the one the host entries and ks_release_cache work on."""

    def __init__(self, lib):
        import ctypes as C
        self.handle = C.c_void_p(lib.load().ks_default_ctx())
        self.stream = -1
        assert self.handle.value


def test_release_cache_leaves_no_codes(oracle, tables, monkeypatch):
    """ks_release_cache frees the default context's slots, the kept codes'
    among them, once a host entry has listed it."""
    import kmer_spans_amd as K
    from kmer_spans_amd import _lib, device as D
    dctx = _DefaultCtx(_lib)
    L = _lib.load()
    K.kmer_regions([b"ACGTTGCANNACGTACGTACGGGGTTTACA" * 50], 3, np.arange(64, dtype=np.float64) - 31.0, 2, 1.0)
    _lib.check(L.ks_ctx_set_scan_algo(dctx.handle, 1))
    c = _case(oracle, dctx, tables, monkeypatch, "lines-u16", "chunk", "DRIFT", 1)
    tab = D.DeviceTable(dctx, H._weights("A", "DRIFT", c.k), c.k, 0.0, compress=True, expand=True)
    try:
        for i in range(3):
            c.regions("A", *PARAMS[i], f"scan {i}", tab=tab)
        assert _codes(c.ds) == _c(1, 1)
        L.ks_release_cache()
        c.regions("A", *PARAMS[0], "after the release: general path", tab=tab)
        assert _codes(c.ds) == _c(1, 1)
        c.regions("A", *PARAMS[1], "writes", tab=tab)
        c.regions("A", *PARAMS[2], "reads", tab=tab)
        assert _codes(c.ds) == _c(2, 2)
    finally:
        tab.close()
        L.ks_ctx_set_scan_algo(dctx.handle, -1)


_POISON_CHILD = r"""
import ctypes as C, sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
import kmer_spans_amd as K
from kmer_spans_amd import _lib, device as D
from oracle import oracle as O
from tests import scanplant as SP

class Ctx:  # the default context: the one the host entries poison
    def __init__(self):
        self.handle = C.c_void_p(_lib.load().ks_default_ctx())
        self.stream = -1

k = 9
L = _lib.load()
small = [b"ACGTTGCANNACGTACGTACGGGGTTTACA" * 50]
w3 = np.arange(64, dtype=np.float64) - 31.0
K.kmer_regions(small, 3, w3, 2, 1.0)
ctx = Ctx()
_lib.check(L.ks_ctx_set_scan_algo(ctx.handle, 1))
seqs = SP.corpus("tile", "DRIFT").sequences(k)
w = SP.table("DRIFT", k)
ds = D.from_host(seqs, "cuda")
tab = D.DeviceTable(ctx, w, k, 0.0, compress=True, expand=True)
assert tab.pass1_kernel == "k_pass1l"
params = [(1, 2.0), (5, 3.0), (3, 6.0)]

def scan(i, what):
    mw, ms = params[i]
    o = O.scan(seqs, k, w, 0.0, mw, ms, visits=True)
    vis = torch.zeros(4 ** k, dtype=torch.int32, device="cuda")
    pos, sc, st = D.scan(ctx, ds, k, tab, mw, ms, vis)
    assert st["scan_algo"] == 1, what
    assert np.array_equal(pos, o["pos"]), (what, "regions")
    assert np.array_equal(sc.view(np.uint64), o["score"].view(np.uint64)), (what, "score bits")
    assert np.array_equal(vis.cpu().numpy(), o["counts"]), (what, "visits")
    return ds.seq_index().codes_info()

for i in range(3):
    info = scan(i, f"scan {i}")
assert (info["code_builds"], info["code_reuses"]) == (1, 1), info
g = K.kmer_regions(small, 3, w3, 2, 1.0)  # a host entry: poisons the context's workspace, the kept codes' slot too
assert np.array_equal(g["pos"], O.kmer_regions(small, 3, w3, 2, 1.0)["pos"])
info = scan(0, "after the poison: general path")
assert (info["code_builds"], info["code_reuses"]) == (1, 1), info
info = scan(1, "writes again")
info = scan(2, "reads")
assert (info["code_builds"], info["code_reuses"]) == (2, 2), info
print("POISON_CHILD_OK")
"""


def test_poisoned_workspace_leaves_no_codes():
    """KS_DEBUG_POISON is read once per process, so a fresh child runs with it:
    three indexed scans on the default context (general, writer, reader), a
    host entry, which poisons every slot of that context -- the kept codes'
    too -- and clears the tags, then a scan: it reads no codes (code_reuses
    does not move), and every scan equals the oracle."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, KS_DEBUG_POISON="0xa5")
    for name in SWITCHES:
        env.pop(name, None)
    r = subprocess.run([sys.executable, "-c", _POISON_CHILD, root], cwd=root, env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and "POISON_CHILD_OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


# ------------------------------------------------------------------ 6. switches

@pytest.mark.parametrize("switch", ["KS_NO_KEPT_CODES", "KS_NO_EXACT_ENTRY", "KS_NO_ENTRY_HINT", "KS_NO_CHUNK_REUSE",
                                    "KS_NO_SEQ_INDEX", "KS_TEST_KEPT_CODES_NOMEM"])
def test_switches_keep_the_path_off(oracle, ctx, tables, monkeypatch, switch):
    c = _case(oracle, ctx, tables, monkeypatch, "lines-u16", "tile", "DRIFT", 1)
    monkeypatch.setenv(switch, "1")
    for i in range(3):
        c.regions("A", *PARAMS[i], f"{switch} scan {i}")
    nomem = 3 if switch == "KS_TEST_KEPT_CODES_NOMEM" else 0
    assert _codes(c.ds) == _c(0, 0, 0, nomem), switch  # (KS_NO_SEQ_INDEX: plain calls, the handle counts nothing)
    monkeypatch.delenv(switch)
    for i in range(3):
        c.regions("A", *PARAMS[i], f"after {switch} scan {i}")
    assert _codes(c.ds)["code_reuses"] >= 1


def test_a_lut_past_the_lds_copy_keeps_no_codes(oracle, ctx, monkeypatch):
    """More distinct values than kLineLutMax = 7168: the uint16 line pass reads
    the LUT from memory and the form keeps no codes."""
    from kmer_spans_amd import device as D
    k = 9
    w = (np.arange(4 ** k, dtype=np.int64) % 8000).astype(np.float64) / 64.0 - 60.0
    seqs, _ = _seam_seqs(k, 1, np.random.default_rng(5))
    tab = D.DeviceTable(ctx, w, k, 0.0, compress=True, expand=True)
    try:
        assert tab.distinct > 7168 and tab.pass1_kernel == "k_pass1l"
        ds = D.from_host(seqs, "cuda")
        o = oracle.scan(seqs, k, w, 0.0, 3, 2.0, visits=True)
        for i in range(3):
            pos, sc, st, vis = H._scan(ctx, ds, k, tab, 3, 2.0)
            H._equal(pos, sc, vis, o, f"large LUT scan {i}")
        assert _codes(ds) == _c(0, 0)
        assert _entry(ds)["entry_reuses"] == 2
    finally:
        tab.close()
