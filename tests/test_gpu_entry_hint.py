"""The chunked scan's kept slot (ks_scan_chunked.hip, ChunkKeep): a scan of a
sequence index takes the chunk table of the context's previous scan of that
index (same k and scan kind), and with the same table(s) its entry hint -- the
previous scan's P2 prediction -- instead of running the predictor.

A hint is never a result: every scan below, with a kept, a recomputed or a
deliberately spoilt hint (KS_TEST_ENTRY_HINT), is compared bit for bit with
the CPU oracle (regions, score bits, visit histogram), and the counters of
ks_seq_index_info say which path each call took.  The planted genomes are
tests/scanplant.py's: the DRIFT drift-span plant climbs to about 1,938, past
kP1SumMin = 1024 and within 12.5 % of the 2048 binade edge, so pass 1 writes
summaries for the predicted binade and for its neighbour."""
import numpy as np
import pytest

from tests import scanplant as SP

pytestmark = pytest.mark.gpu

# id -> k, environment at table build, pass-1 kernel, line kind (all compressed and expanded:
# the pass-1-summary forms of plan_scan)
FORMS = {
    "lines-u16": (9, {}, "k_pass1l", 1),
    "lds-predictor": (6, {}, "k_pass1_lds", 0),
    "expanded-u16": (9, {"KS_NO_LINES": "1"}, "k_pass1p", 0),
    "wide": (12, {}, "k_pass1w", 3),
}
SMALL_FORMS = ["lines-u16", "lds-predictor", "expanded-u16"]
CORPORA = [("tile", "DRIFT"), ("chunk", "DYADIC")]
SPLITS = ["two-parts", "default"]
PARAMS = [(1, 2.0), (5, 3.0), (3, 6.0)]  # (min_width, min_score); tr_lr: min_length = min_width
OTHER = (0.65, -0.55, -1e6, 0.3)         # table B: other values on the same bases (A, C, T, G)
SWITCHES = ("KS_NO_ENTRY_HINT", "KS_NO_CHUNK_REUSE", "KS_TEST_ENTRY_HINT", "KS_SPLIT_MIN_CHUNKS", "KS_NO_SEQ_INDEX",
            "KS_NO_LINES")


def _weights(name, vset, k):
    """Table "A": the corpus's own values; "B": OTHER; "init": tr_lr's random first-k-mer scores."""
    if name == "A":
        return SP.table(vset, k)
    if name == "B":
        return np.array(OTHER, dtype=np.float64)[np.arange(4 ** k, dtype=np.int64) & 3]
    return np.random.default_rng({"init": 7, "init2": 8}[name] + k).normal(size=4 ** k)


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


class _Tables:
    """The tables of one (form, value set) at a time (the k = 12 line table is 2 GiB)."""

    def __init__(self):
        self.key, self.tabs = None, {}

    def get(self, ctx, form, vset, name, monkeypatch):
        from kmer_spans_amd import device as D
        k, env, kernel, line_kind = FORMS[form]
        if self.key != (form, vset):
            self.close()
            self.key = (form, vset)
        if name not in self.tabs:
            for var, value in env.items():  # (read at table build)
                monkeypatch.setenv(var, value)
            init = name.startswith("init")
            t = D.DeviceTable(ctx, _weights(name, vset, k), k, 0.0, compress=not init, expand=not init)
            if not init:
                assert (t.pass1_kernel, t.line_kind, t.compressed) == (kernel, line_kind, True), (form, name)
            self.tabs[name] = t
        return self.tabs[name]

    def close(self):
        for t in self.tabs.values():
            t.close()
        self.key, self.tabs = None, {}


@pytest.fixture(scope="module")
def tables():
    t = _Tables()
    yield t
    t.close()


_ORACLE = {}


def _oracle(oracle, seqs_key, seqs, k, wname, vset, mode, mw, ms):
    """Computed once per (sequences, k, table, mode, thresholds) and never changed."""
    key = (seqs_key, k, wname, vset, mode, mw, ms)
    if key not in _ORACLE:
        w = _weights(wname[0] if mode == "tr_lr" else wname, vset, k)
        if mode == "kmer_regions":
            _ORACLE[key] = oracle.scan(seqs, k, w, 0.0, mw, ms, visits=True)
        else:
            _ORACLE[key] = oracle.tr_lr_regions(seqs, k, mw, _weights(wname[1], vset, k), w)
    return _ORACLE[key]


def _equal(pos, sc, vis, o, what):
    assert pos.shape == o["pos"].shape, (what, pos.shape, o["pos"].shape)
    assert np.array_equal(pos, o["pos"]), (what, "regions")
    assert np.array_equal(sc.view(np.uint64), o["score"].view(np.uint64)), (what, "score bits")
    if vis is not None:
        assert np.array_equal(vis, o["counts"]), (what, "visits")


def _scan(ctx, ds, k, tab, mw, ms):
    import torch
    from kmer_spans_amd import device as D
    vis = torch.zeros(4 ** k, dtype=torch.int32, device="cuda")
    pos, sc, st = D.scan(ctx, ds, k, tab, mw, ms, vis)
    assert st["scan_algo"] == 1
    return pos, sc, st, vis.cpu().numpy()


def _split(monkeypatch, split):
    if split == "two-parts":
        monkeypatch.setenv("KS_SPLIT_MIN_CHUNKS", "0")


def _info(ds):
    return ds.seq_index().scan_info()


def _counts(chunk, hint, pred):
    return {"chunk_reuses": chunk, "hint_reuses": hint, "predictor_builds": pred}


class _Case:
    """One corpus on one form: the device sequences and a checked scan."""

    def __init__(self, oracle, ctx, tables, monkeypatch, form, seam, vset, repeat=1):
        from kmer_spans_amd import device as D
        self.oracle, self.ctx, self.tables, self.mp, self.form, self.vset = oracle, ctx, tables, monkeypatch, form, vset
        self.k = FORMS[form][0]
        self.seqs_key = (seam, vset, self.k, repeat)
        self.seqs = SP.corpus(seam, vset).sequences(self.k) * repeat
        self.ds = D.from_host(self.seqs, "cuda")

    def tab(self, name, form=None):
        return self.tables.get(self.ctx, form or self.form, self.vset, name, self.mp)

    def regions(self, wname, mw, ms, what, tab=None, k=None):
        k = k or self.k
        o = _oracle(self.oracle, self.seqs_key, self.seqs, k, wname, self.vset, "kmer_regions", mw, ms)
        pos, sc, st, vis = _scan(self.ctx, self.ds, k, tab or self.tab(wname), mw, ms)
        print(f"HINTSTAT {what} n_replay={st['n_replay']} n_regions={pos.shape[1]} ms_layout={st['ms_layout']:.3f}")
        _equal(pos, sc, vis, o, what)
        return st

    def tr_lr(self, wname, iname, mw, what):
        from kmer_spans_amd import device as D
        o = _oracle(self.oracle, self.seqs_key, self.seqs, self.k, (wname, iname), self.vset, "tr_lr", mw, 0.0)
        pos, sc, st = D.tr_lr(self.ctx, self.ds, self.k, self.tab(wname), self.tab(iname), mw)
        assert st["scan_algo"] == 1
        print(f"HINTSTAT {what} n_replay={st['n_replay']} n_regions={pos.shape[1]}")
        _equal(pos, sc, None, o, what)
        return st


_THREE = [(f, s, v, sp, "kmer_regions") for f in SMALL_FORMS for s, v in CORPORA for sp in SPLITS] + \
         [("lines-u16", s, v, sp, "tr_lr") for s, v in CORPORA for sp in SPLITS] + \
         [("wide", "tile", "DRIFT", "default", "kmer_regions")]


@pytest.mark.parametrize("form,seam,vset,split,mode", _THREE, ids=["-".join(x) for x in _THREE])
def test_three_scans_one_predictor(oracle, ctx, tables, monkeypatch, form, seam, vset, split, mode):
    """Case 1: one DeviceSeqs, one table, three thresholds: the predictor runs
    once, the second and third scan take the chunk table and the hint."""
    _split(monkeypatch, split)
    c = _Case(oracle, ctx, tables, monkeypatch, form, seam, vset)
    for i, (mw, ms) in enumerate(PARAMS):
        what = f"{seam}/{vset} {form} {split} {mode} scan {i}"
        if mode == "kmer_regions":
            c.regions("A", mw, ms, what)
        else:
            c.tr_lr("A", "init", mw, what)
        assert _info(c.ds) == _counts(i, i, 1), what
    assert c.ds.seq_index().info() == {"builds": 1, "hits": 2, "layout_builds": 1, "guard_failures": 0}


_SMALL = [(f, sp) for f in SMALL_FORMS for sp in SPLITS]
_SMALL_IDS = ["-".join(x) for x in _SMALL]


@pytest.mark.parametrize("form,split", _SMALL, ids=_SMALL_IDS)
def test_another_table_keeps_the_chunks_only(oracle, ctx, tables, monkeypatch, form, split):
    """Case 2: table A, B (other values, same k), A again: the chunk table is
    taken at calls 2 and 3, a hint never (it is the other table's)."""
    _split(monkeypatch, split)
    c = _Case(oracle, ctx, tables, monkeypatch, form, "tile", "DRIFT")
    for i, name in enumerate("ABA"):
        c.regions(name, *PARAMS[i], f"{form} {split} table {name} call {i}")
        assert _info(c.ds) == _counts(i, 0, i + 1), (form, split, i)


@pytest.mark.parametrize("form,split", _SMALL, ids=_SMALL_IDS)
def test_destroyed_table_is_another_table(oracle, ctx, tables, monkeypatch, form, split):
    """Case 3: A destroyed, A' created with other values (the allocator may
    hand out the same addresses): tables are told apart by id, so no hint."""
    from kmer_spans_amd import device as D
    _split(monkeypatch, split)
    c = _Case(oracle, ctx, tables, monkeypatch, form, "tile", "DRIFT")
    k, env = FORMS[form][0], FORMS[form][1]
    for var, value in env.items():
        monkeypatch.setenv(var, value)
    tab = D.DeviceTable(ctx, _weights("A", "DRIFT", k), k, 0.0, compress=True, expand=True)
    try:
        c.regions("A", *PARAMS[0], f"{form} {split} table A", tab=tab)
        c.regions("A", *PARAMS[1], f"{form} {split} table A again", tab=tab)
        assert _info(c.ds) == _counts(1, 1, 1)
        tab.close()
        tab = D.DeviceTable(ctx, _weights("B", "DRIFT", k), k, 0.0, compress=True, expand=True)
        c.regions("B", *PARAMS[1], f"{form} {split} table A'", tab=tab)
        assert _info(c.ds) == _counts(2, 1, 2)
    finally:
        tab.close()


@pytest.mark.parametrize("form,split", _SMALL, ids=_SMALL_IDS)
def test_spoilt_hint_changes_no_result(oracle, ctx, tables, monkeypatch, form, split):
    """Case 4: the hint overwritten on the device before a reusing call's pass
    1 -- all zero, all 1e14, all NaN, every chunk its neighbour's value.
    Regions, score bits and visits stay the oracle's (n_replay may not)."""
    _split(monkeypatch, split)
    c = _Case(oracle, ctx, tables, monkeypatch, form, "tile", "DRIFT")
    c.regions("A", *PARAMS[0], f"{form} {split} first")
    for i, how in enumerate(("zero", "huge", "nan", "shift")):
        monkeypatch.setenv("KS_TEST_ENTRY_HINT", how)
        c.regions("A", *PARAMS[i % 3], f"{form} {split} hint {how}")
        assert _info(c.ds) == _counts(i + 1, i + 1, 1), how  # (the hook runs on a reusing call only)
    monkeypatch.delenv("KS_TEST_ENTRY_HINT")
    c.regions("A", *PARAMS[2], f"{form} {split} after the spoilt hints")
    assert _info(c.ds) == _counts(5, 5, 1)


def test_unknown_hook_value_is_refused(oracle, ctx, tables, monkeypatch):
    from kmer_spans_amd import _lib
    c = _Case(oracle, ctx, tables, monkeypatch, "lines-u16", "chunk", "DYADIC")
    c.regions("A", *PARAMS[0], "first")
    monkeypatch.setenv("KS_TEST_ENTRY_HINT", "other")
    with pytest.raises(_lib.KmerSpansError, match="KS_TEST_ENTRY_HINT"):
        _scan(ctx, c.ds, c.k, c.tab("A"), *PARAMS[0])
    monkeypatch.delenv("KS_TEST_ENTRY_HINT")
    c.regions("A", *PARAMS[1], "after the refused call")  # (a failed call leaves no tag: nothing reused)
    assert _info(c.ds) == _counts(0, 0, 2)


@pytest.mark.parametrize("form,split", _SMALL, ids=_SMALL_IDS)
def test_switches_recompute(oracle, ctx, tables, monkeypatch, form, split):
    """Case 5: KS_NO_ENTRY_HINT and KS_NO_CHUNK_REUSE: the results of case 1, nothing reused."""
    _split(monkeypatch, split)
    c = _Case(oracle, ctx, tables, monkeypatch, form, "tile", "DRIFT")
    monkeypatch.setenv("KS_NO_ENTRY_HINT", "1")
    monkeypatch.setenv("KS_NO_CHUNK_REUSE", "1")
    for i, (mw, ms) in enumerate(PARAMS):
        c.regions("A", mw, ms, f"{form} {split} switches scan {i}")
        assert _info(c.ds) == _counts(0, 0, i + 1)
    monkeypatch.delenv("KS_NO_ENTRY_HINT")  # each switch on its own
    c.regions("A", *PARAMS[0], f"{form} {split} hint without chunk reuse")
    assert _info(c.ds) == _counts(0, 1, 3)
    monkeypatch.delenv("KS_NO_CHUNK_REUSE")
    monkeypatch.setenv("KS_NO_ENTRY_HINT", "1")
    c.regions("A", *PARAMS[1], f"{form} {split} chunk reuse without hint")
    assert _info(c.ds) == _counts(1, 1, 4)
    assert c.ds.seq_index().info()["hits"] == 4


@pytest.mark.parametrize("split", SPLITS)
def test_another_k_or_scan_kind_reuses_nothing(oracle, ctx, tables, monkeypatch, split):
    """Case 6: k 9, k 6, k 9, tr_lr, kmer_regions on one index: every call has a
    new layout, so neither the chunk table nor the hint of the call before."""
    from kmer_spans_amd import device as D
    _split(monkeypatch, split)
    c = _Case(oracle, ctx, tables, monkeypatch, "lines-u16", "tile", "DRIFT")
    c.regions("A", *PARAMS[0], f"{split} k 9")
    t6 = D.DeviceTable(ctx, _weights("A", "DRIFT", 6), 6, 0.0, compress=True, expand=True)
    try:
        c.regions("A", *PARAMS[0], f"{split} k 6", tab=t6, k=6)
    finally:
        t6.close()
    c.regions("A", *PARAMS[0], f"{split} k 9 again")
    c.tr_lr("A", "init", 1, f"{split} tr_lr")
    c.regions("A", *PARAMS[1], f"{split} kmer_regions after tr_lr")
    assert _info(c.ds) == _counts(0, 0, 5)
    c.regions("A", *PARAMS[2], f"{split} and once more")
    assert _info(c.ds) == _counts(1, 1, 5)


@pytest.mark.parametrize("split", SPLITS)
def test_tr_lr_keys_on_both_tables(oracle, ctx, tables, monkeypatch, split):
    """Another first-k-mer table under the same transition table: no hint."""
    _split(monkeypatch, split)
    c = _Case(oracle, ctx, tables, monkeypatch, "lines-u16", "tile", "DRIFT")
    c.tr_lr("A", "init", 1, f"{split} init")
    c.tr_lr("A", "init2", 1, f"{split} init2")
    assert _info(c.ds) == _counts(1, 0, 2)
    c.tr_lr("A", "init2", 5, f"{split} init2 again")
    assert _info(c.ds) == _counts(2, 1, 2)


@pytest.mark.parametrize("split", SPLITS)
def test_larger_genome_in_between(oracle, ctx, tables, monkeypatch, split):
    """Case 7: a larger genome scanned on the same context regrows and
    overwrites the kept slot; the first genome's next scan reuses nothing."""
    _split(monkeypatch, split)
    small = _Case(oracle, ctx, tables, monkeypatch, "lines-u16", "chunk", "DRIFT")
    big = _Case(oracle, ctx, tables, monkeypatch, "lines-u16", "tile", "DRIFT", repeat=2)
    small.regions("A", *PARAMS[0], f"{split} small")
    small.regions("A", *PARAMS[1], f"{split} small again")
    assert _info(small.ds) == _counts(1, 1, 1)
    big.regions("A", *PARAMS[0], f"{split} big")
    small.regions("A", *PARAMS[2], f"{split} small after big")
    assert _info(small.ds) == _counts(1, 1, 2)
    assert _info(big.ds) == _counts(0, 0, 1)
    assert small.ds.seq_index().info()["builds"] == 2


def test_two_parts_for_real(oracle, ctx, tables, monkeypatch):
    """The planted corpora are below the 3,072 chunks a two-part scan needs
    (plan_scan); four copies of the tile corpus as twelve sequences (6,808
    chunks) split.  The first part's P2 then writes its prediction under the
    second part's pass 1, which reads the kept hint: the other array."""
    monkeypatch.setenv("KS_SPLIT_MIN_CHUNKS", "0")
    c = _Case(oracle, ctx, tables, monkeypatch, "lines-u16", "tile", "DRIFT", repeat=4)
    assert sum(len(s) for s in c.seqs) // 256 > 2 * 3072
    for i, (mw, ms) in enumerate(PARAMS):
        c.regions("A", mw, ms, f"two parts scan {i}")
        assert _info(c.ds) == _counts(i, i, 1)
    monkeypatch.setenv("KS_TEST_ENTRY_HINT", "shift")
    c.regions("A", *PARAMS[0], "two parts, shifted hint")
    assert _info(c.ds) == _counts(3, 3, 1)
