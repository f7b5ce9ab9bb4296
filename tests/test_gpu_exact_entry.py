"""Pass 1 from exact entries (ks_scan_chunked.hip, ScanPlan::entry_reuse): a
scan of a sequence index with the table(s) of the context's previous scan
starts every chunk from the exact entry that scan left in the kept slot, walks
the carried head itself and verifies every kept entry against the exact exit of
the chunk before it -- no predictor, summaries, carry or heads.

The kept entries are never a result: every scan below -- on the new path, on
the general path, with spoilt entries (KS_TEST_ENTRY_HINT) and after every
change of key -- is compared bit for bit with the CPU oracle (regions, score
bits, visit histogram), and ks_seq_index_entry_info says which path each call
took.  Corpora, tables and the oracle's results are tests/scanplant.py's and
test_gpu_entry_hint.py's (one oracle run per input, shared)."""
import numpy as np
import pytest

from tests import test_gpu_entry_hint as H

pytestmark = pytest.mark.gpu

PARAMS = H.PARAMS
CORPORA = H.CORPORA
SWITCHES = H.SWITCHES + ("KS_NO_EXACT_ENTRY",)
FOUR = 4  # copies of the tile corpus that make a scan split in two parts (6,808 chunks)


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
    """One corpus on one form; parts = 2: four copies, split at any size."""
    if parts == 2:
        monkeypatch.setenv("KS_SPLIT_MIN_CHUNKS", "0")
    c = H._Case(oracle, ctx, tables, monkeypatch, form, seam, vset, repeat=FOUR if parts == 2 else 1)
    if parts == 2:
        assert sum(len(s) for s in c.seqs) // 256 > 2 * 3072
    return c


def _entry(ds):
    return ds.seq_index().entry_info()


def _e(reuses, fallbacks):
    return {"entry_reuses": reuses, "entry_fallbacks": fallbacks}


_THREE = [(f, s, v, 1, "kmer_regions") for f in ("lines-u16", "wide") for s, v in CORPORA] + \
         [("lines-u16", s, v, 1, "tr_lr") for s, v in CORPORA] + \
         [("lines-u16", "tile", "DRIFT", 2, "kmer_regions"), ("wide", "tile", "DRIFT", 2, "kmer_regions"),
          ("lines-u16", "tile", "DRIFT", 2, "tr_lr")]


@pytest.mark.parametrize("form,seam,vset,parts,mode", _THREE, ids=["-".join(map(str, x)) for x in _THREE])
def test_three_scans_one_carry(oracle, ctx, tables, monkeypatch, form, seam, vset, parts, mode):
    """Case 1: one DeviceSeqs, one table, three thresholds.  Scan 0 takes the
    general path and replays (the corpus exercises the carry); scans 1 and 2
    start from its exact entries and replay nothing."""
    c = _case(oracle, ctx, tables, monkeypatch, form, seam, vset, parts)
    for i, (mw, ms) in enumerate(PARAMS):
        what = f"{seam}/{vset} {form} parts {parts} {mode} scan {i}"
        st = c.regions("A", mw, ms, what) if mode == "kmer_regions" else c.tr_lr("A", "init", mw, what)
        print(f"EXACTSTAT {what} n_replay={st['n_replay']} ms_predict={st['ms_predict']:.3f} "
              f"ms_carry={st['ms_carry']:.3f}")
        if i == 0:
            assert st["n_replay"] > 0, what
        else:
            assert st["n_replay"] == 0, (what, st["n_replay"])
        assert _entry(c.ds) == _e(i, 0), what
        assert H._info(c.ds) == H._counts(i, i, 1), what
    assert c.ds.seq_index().info() == {"builds": 1, "hits": 2, "layout_builds": 1, "guard_failures": 0}


_SPOILT = [("lines-u16", 1), ("lines-u16", 2), ("wide", 1)]


@pytest.mark.parametrize("form,parts", _SPOILT, ids=[f"{f}-{p}" for f, p in _SPOILT])
def test_spoilt_entries_fall_back(oracle, ctx, tables, monkeypatch, form, parts):
    """Case 2: the kept entries overwritten before a reusing call's pass 1 --
    all zero, all 1e14, all NaN, every chunk its neighbour's.  The verification
    fails, the call is rerun on the hint path (whose hint the hook spoils too)
    and equals the oracle; the next unspoilt call takes the new path again."""
    c = _case(oracle, ctx, tables, monkeypatch, form, "tile", "DRIFT", parts)
    c.regions("A", *PARAMS[0], f"{form} parts {parts} first")
    for i, how in enumerate(("zero", "huge", "nan", "shift")):
        monkeypatch.setenv("KS_TEST_ENTRY_HINT", how)
        c.regions("A", *PARAMS[i % 3], f"{form} parts {parts} entries {how}")
        assert _entry(c.ds) == _e(0, i + 1), how
        assert H._info(c.ds) == H._counts(i + 1, i + 1, 1), how
    monkeypatch.delenv("KS_TEST_ENTRY_HINT")
    st = c.regions("A", *PARAMS[2], f"{form} parts {parts} after the spoilt entries")
    assert st["n_replay"] == 0
    assert _entry(c.ds) == _e(1, 4)
    assert H._info(c.ds) == H._counts(5, 5, 1)


def test_another_table_reuses_no_entry(oracle, ctx, tables, monkeypatch):
    """Case 3: table A, B (other values, same k), A again, A once more."""
    c = _case(oracle, ctx, tables, monkeypatch, "lines-u16", "tile", "DRIFT", 1)
    for i, name in enumerate("ABA"):
        c.regions(name, *PARAMS[i], f"table {name} call {i}")
        assert _entry(c.ds) == _e(0, 0), (name, i)
    c.regions("A", *PARAMS[0], "table A once more")
    assert _entry(c.ds) == _e(1, 0)


def test_destroyed_table_is_another_table(oracle, ctx, tables, monkeypatch):
    """Case 3: A destroyed, A' created with other values, perhaps at the same addresses."""
    from kmer_spans_amd import device as D
    c = _case(oracle, ctx, tables, monkeypatch, "lines-u16", "tile", "DRIFT", 1)
    k = c.k
    tab = D.DeviceTable(ctx, H._weights("A", "DRIFT", k), k, 0.0, compress=True, expand=True)
    try:
        c.regions("A", *PARAMS[0], "table A", tab=tab)
        c.regions("A", *PARAMS[1], "table A again", tab=tab)
        assert _entry(c.ds) == _e(1, 0)
        tab.close()
        tab = D.DeviceTable(ctx, H._weights("B", "DRIFT", k), k, 0.0, compress=True, expand=True)
        c.regions("B", *PARAMS[1], "table A'", tab=tab)
        assert _entry(c.ds) == _e(1, 0)
        c.regions("B", *PARAMS[2], "table A' again", tab=tab)
        assert _entry(c.ds) == _e(2, 0)
    finally:
        tab.close()


def test_tr_lr_keys_on_both_tables(oracle, ctx, tables, monkeypatch):
    """Case 3: another first-k-mer table under the same transition table."""
    c = _case(oracle, ctx, tables, monkeypatch, "lines-u16", "tile", "DRIFT", 1)
    c.tr_lr("A", "init", 1, "init")
    c.tr_lr("A", "init2", 1, "init2")
    assert _entry(c.ds) == _e(0, 0)
    c.tr_lr("A", "init2", 5, "init2 again")
    assert _entry(c.ds) == _e(1, 0)


def test_another_k_or_scan_kind_in_between(oracle, ctx, tables, monkeypatch):
    """Case 3: k 9, k 6, k 9, tr_lr, kmer_regions on one index."""
    from kmer_spans_amd import device as D
    c = _case(oracle, ctx, tables, monkeypatch, "lines-u16", "tile", "DRIFT", 1)
    c.regions("A", *PARAMS[0], "k 9")
    t6 = D.DeviceTable(ctx, H._weights("A", "DRIFT", 6), 6, 0.0, compress=True, expand=True)
    try:
        c.regions("A", *PARAMS[0], "k 6", tab=t6, k=6)
    finally:
        t6.close()
    c.regions("A", *PARAMS[0], "k 9 again")
    c.tr_lr("A", "init", 1, "tr_lr")
    c.regions("A", *PARAMS[1], "kmer_regions after tr_lr")
    assert _entry(c.ds) == _e(0, 0)
    c.regions("A", *PARAMS[2], "and once more")
    assert _entry(c.ds) == _e(1, 0)


def test_larger_genome_in_between(oracle, ctx, tables, monkeypatch):
    """Case 3: a larger genome on the same context regrows and overwrites the kept slot."""
    small = H._Case(oracle, ctx, tables, monkeypatch, "lines-u16", "chunk", "DRIFT")
    big = H._Case(oracle, ctx, tables, monkeypatch, "lines-u16", "tile", "DRIFT", repeat=2)
    small.regions("A", *PARAMS[0], "small")
    small.regions("A", *PARAMS[1], "small again")
    assert _entry(small.ds) == _e(1, 0)
    big.regions("A", *PARAMS[0], "big")
    small.regions("A", *PARAMS[2], "small after big")
    assert _entry(small.ds) == _e(1, 0)
    assert _entry(big.ds) == _e(0, 0)
    small.regions("A", *PARAMS[0], "small once more")
    assert _entry(small.ds) == _e(2, 0)


@pytest.mark.parametrize("parts", [1, 2])
def test_switches(oracle, ctx, tables, monkeypatch, parts):
    """Case 4: KS_NO_EXACT_ENTRY takes the hint path; KS_NO_ENTRY_HINT disables both."""
    c = _case(oracle, ctx, tables, monkeypatch, "lines-u16", "tile", "DRIFT", parts)
    monkeypatch.setenv("KS_NO_EXACT_ENTRY", "1")
    for i, (mw, ms) in enumerate(PARAMS):
        c.regions("A", mw, ms, f"parts {parts} no exact entry, scan {i}")
        assert _entry(c.ds) == _e(0, 0)
        assert H._info(c.ds) == H._counts(i, i, 1)
    monkeypatch.delenv("KS_NO_EXACT_ENTRY")
    monkeypatch.setenv("KS_NO_ENTRY_HINT", "1")
    c.regions("A", *PARAMS[0], f"parts {parts} no entry hint")
    assert _entry(c.ds) == _e(0, 0)
    assert H._info(c.ds) == H._counts(3, 2, 2)
    monkeypatch.delenv("KS_NO_ENTRY_HINT")
    st = c.regions("A", *PARAMS[1], f"parts {parts} no switch")
    assert st["n_replay"] == 0
    assert _entry(c.ds) == _e(1, 0)
    assert H._info(c.ds) == H._counts(4, 3, 2)


@pytest.mark.parametrize("form", ["lines-u16", "wide"])
def test_without_then_with_visits(oracle, ctx, tables, monkeypatch, form):
    """Case 5: the visit histogram is no part of the key."""
    from kmer_spans_amd import device as D
    c = _case(oracle, ctx, tables, monkeypatch, form, "tile", "DRIFT", 1)
    mw, ms = PARAMS[0]
    o = H._oracle(oracle, c.seqs_key, c.seqs, c.k, "A", "DRIFT", "kmer_regions", mw, ms)
    pos, sc, st = D.scan(ctx, c.ds, c.k, c.tab("A"), mw, ms, None)
    assert st["scan_algo"] == 1 and st["n_replay"] > 0
    H._equal(pos, sc, None, o, f"{form} without visits")
    st = c.regions("A", mw, ms, f"{form} with visits")
    assert st["n_replay"] == 0
    assert _entry(c.ds) == _e(1, 0)
    pos, sc, st = D.scan(ctx, c.ds, c.k, c.tab("A"), mw, ms, None)
    H._equal(pos, sc, None, o, f"{form} without visits again")
    assert _entry(c.ds) == _e(2, 0)
