"""The chunked scan (scan_algo 1) on planted trajectories (tests/scanplant.py):
excursions that begin, peak, tie, clamp or stay open exactly on a chunk seam
(256 scan indices of a run), a tile seam (64 chunks) and a step seam (64
tiles, one trip of the per-run wave loops), through every pass-1 table form,
one and two parts, kmer_regions and tr_lr, and a cached sequence index.

Everything is compared bit for bit with the CPU oracle (regions, score bits,
visit histogram) and, for the INT and DYADIC value sets, with the regions the
plant itself predicts; a difference names the planted instance.  The path
taken is asserted from the scan statistics: integer tables on the exact carry
replay nothing, the tied-span plants of the other value sets are replayed."""
import numpy as np
import pytest

from tests import scanplant as SP

pytestmark = pytest.mark.gpu

MW, MS = 1, 2.0

# id, k, compress, expand, environment at table build -> pass-1 kernel, line kind, compressed
FORMS = {
    "lds": (6, True, False, {}, "k_pass1_lds", 0, True),               # no predictor, no pass-1 summaries
    "lds-predictor": (6, True, True, {}, "k_pass1_lds", 0, True),      # pass-1 summaries: the two-part scan
    "plain-u16": (9, True, False, {}, "k_pass1", 0, True),
    "plain-f64": (9, False, False, {}, "k_pass1", 0, False),
    "expanded-u16": (9, True, True, {"KS_NO_LINES": "1"}, "k_pass1p", 0, True),
    "expanded-f64": (9, False, True, {"KS_NO_LINES": "1"}, "k_pass1pf", 0, False),
    "lines-u16": (9, True, True, {}, "k_pass1l", 1, True),
    "lines-f64": (9, False, True, {}, "k_pass1l", 2, False),
    "wide": (12, True, True, {}, "k_pass1w", 3, True),
}
# The exact integer carry (k_carry_exact, k_pass1_lds_int) serves integer
# tables on the LDS, line and expanded forms (plan_scan); an unexpanded table
# at k > 7 takes the general carry whatever its values.
EXACT_FORMS = {"lds", "lds-predictor", "expanded-u16", "expanded-f64", "lines-u16", "lines-f64", "wide"}
STEP_FORMS = ["lds", "lds-predictor", "plain-u16"]


@pytest.fixture(scope="module")
def units():
    from kmer_spans_amd import _lib
    L = _lib.load()
    u = int(L.ks_scan_chunk_indices()), int(L.ks_scan_tile_chunks())
    assert u == (256, 64) == (SP.CHUNK, SP.TILE_CHUNKS)
    return u


@pytest.fixture(scope="module")
def ctx():
    from kmer_spans_amd import _lib, device as D
    c = _lib.context(0)
    D.bind_torch_stream(c)
    yield c
    c.set_scan_algo(-1)


class _Tables:
    """One table (and its tr_lr first-k-mer table) alive at a time: the cases
    are ordered by form and value set, and the 128-B line table takes most of
    the card's memory budget."""

    def __init__(self):
        self.key, self.tab, self.init, self.ks = None, None, None, None

    def get(self, ctx, form, vset, monkeypatch):
        from kmer_spans_amd import device as D
        k, compress, expand, env, kernel, line_kind, compressed = FORMS[form]
        if self.key != (form, vset):
            self.close()
            for name, value in env.items():  # (read at table build)
                monkeypatch.setenv(name, value)
            self.tab = D.DeviceTable(ctx, SP.table(vset, k), k, 0.0, compress=compress, expand=expand)
            self.key = (form, vset)
        t = self.tab
        got = (t.pass1_kernel, t.line_kind, t.compressed, t.positions_per_read > 1)
        assert got == (kernel, line_kind, compressed, expand), (form, vset, got, t.positions_per_read)
        return t

    def first(self, ctx, form):
        """The random first-k-mer table of tr_lr beside the current table."""
        from kmer_spans_amd import device as D
        if self.init is None:
            k = FORMS[form][0]
            self.ks = np.random.default_rng(7 + k).normal(size=4 ** k)
            self.init = D.DeviceTable(ctx, self.ks, k, 0.0, compress=False)
        return self.init, self.ks

    def close(self):
        for t in (self.tab, self.init):
            if t is not None:
                t.close()
        self.key, self.tab, self.init, self.ks = None, None, None, None


@pytest.fixture(scope="module")
def tables():
    t = _Tables()
    yield t
    t.close()


_ORACLE = {}


def _oracle(oracle, c, k, mode, mw, ms, ks=None):
    key = (c.seam, c.vset, k, mode, mw, ms)
    if key not in _ORACLE:
        w = SP.table(c.vset, k)
        if mode == "kmer_regions":
            _ORACLE[key] = oracle.scan(c.sequences(k), k, w, 0.0, mw, ms, visits=True)
        else:
            _ORACLE[key] = oracle.tr_lr_regions(c.sequences(k), k, mw, ks, w)
    return _ORACLE[key]


def _same(c, k, pos, sc, o, what, base=0):
    """Regions and score bits equal the oracle's; the message names the
    planted instances that differ."""
    if pos.shape == o["pos"].shape and np.array_equal(pos, o["pos"]) and \
            np.array_equal(sc.view(np.uint64), o["score"].view(np.uint64)):
        return
    lines = c.explain(k, pos, sc, o["pos"], o["score"], base)
    pytest.fail("\n".join([f"{what}: {pos.shape[1]} regions, oracle {o['pos'].shape[1]}"] + lines[:12]))


def _predicted(c, k, pos, sc, mw, ms, what):
    """The regions the plant predicts, instance by instance."""
    got = c.by_instance(k, pos, sc)
    bits = lambda regs: [(q, b, e, int(np.float64(s).view(np.uint64))) for q, b, e, s in regs]  # noqa: E731
    for name, regs in c.predict(k, mw, ms).items():
        assert bits(got[name]) == bits(regs), (what, name, got[name], regs)


def _scan(ctx, c, k, tab, mw, ms, ds=None):
    import torch
    from kmer_spans_amd import device as D
    ds = ds if ds is not None else D.from_host(c.sequences(k), "cuda")
    vis = torch.zeros(4 ** k, dtype=torch.int32, device="cuda")
    ctx.set_scan_algo(1)
    try:
        pos, sc, st = D.scan(ctx, ds, k, tab, mw, ms, vis)
    finally:
        ctx.set_scan_algo(-1)
    assert st["scan_algo"] == 1
    return pos, sc, st, vis.cpu().numpy()


def _regions_case(oracle, ctx, c, form, tab, what, mw=MW, ms=MS):
    k = FORMS[form][0]
    o = _oracle(oracle, c, k, "kmer_regions", mw, ms)
    pos, sc, st, vis = _scan(ctx, c, k, tab, mw, ms)
    print(f"SEAMSTAT {what} n_replay={st['n_replay']} n_regions={pos.shape[1]} n_rescan={st['n_rescan']}")
    _same(c, k, pos, sc, o, what)
    assert np.array_equal(vis, o["counts"]), (what, "visits")
    if c.vset != "DRIFT":
        _predicted(c, k, pos, sc, mw, ms, what)
    assert (st["n_scored"], st["n_runs"]) == (c.n_scored, c.n_runs), (what, st["n_scored"], st["n_runs"])
    return st


def _path(c, form, st, what):
    """The carry's path from the statistics: the exact integer carry replays
    nothing; the tied-span plant of the other value sets enters every chunk
    it spans at a small positive S with no certain clamp, which the general
    carry can only replay."""
    if c.vset == "INT":
        if form in EXACT_FORMS:
            assert st["n_replay"] == 0, (what, st["n_replay"])
    else:
        assert st["n_replay"] > 0, (what, st["n_replay"])


def _cases(seams, forms, trlr):
    out = []
    for form in forms:
        for vset in SP.VALUES:
            for seam in seams:
                if form == "wide" and seam == "step":
                    continue
                for split in ("two-parts", "default"):
                    out.append((form, vset, seam, split, "kmer_regions"))
                    if trlr and vset != "INT":
                        out.append((form, vset, seam, split, "tr_lr"))
    return out


def _ids(cases):
    return ["-".join(x) for x in cases]


_SMALL = _cases(("chunk", "tile"), [f for f in FORMS if f != "lds-predictor"], True)
_STEP = _cases(("step",), STEP_FORMS, False)


@pytest.mark.parametrize("form,vset,seam,split,mode", _SMALL, ids=_ids(_SMALL))
def test_chunk_and_tile_seams(oracle, ctx, units, tables, monkeypatch, form, vset, seam, split, mode):
    from kmer_spans_amd import device as D
    if split == "two-parts":
        monkeypatch.setenv("KS_SPLIT_MIN_CHUNKS", "0")
    c = SP.corpus(seam, vset, *units)
    tab = tables.get(ctx, form, vset, monkeypatch)
    what = f"{seam}/{vset} {form} {split} {mode}"
    if mode == "kmer_regions":
        _path(c, form, _regions_case(oracle, ctx, c, form, tab, what), what)
        return
    k = FORMS[form][0]
    init, ks = tables.first(ctx, form)
    o = _oracle(oracle, c, k, "tr_lr", MW, 0.0, ks)
    ds = D.from_host(c.sequences(k), "cuda")
    ctx.set_scan_algo(1)
    try:
        pos, sc, st = D.tr_lr(ctx, ds, k, tab, init, MW)
    finally:
        ctx.set_scan_algo(-1)
    assert st["scan_algo"] == 1 and st["n_runs"] == c.n_runs
    print(f"SEAMSTAT {what} n_replay={st['n_replay']} n_regions={pos.shape[1]} n_scored={st['n_scored']}")
    _same(c, k, pos, sc, o, what, base=1)
    assert o["pos"].shape[1] > 20


@pytest.mark.parametrize("form,vset,seam,split,mode", _STEP, ids=_ids(_STEP))
def test_step_seam(oracle, ctx, units, tables, monkeypatch, form, vset, seam, split, mode):
    """The hand-over between two trips of the per-run wave loops (k_stitch_runs,
    k_ascan_runs, k_approx_scan, the carry): relative index 1,048,576."""
    if split == "two-parts":
        monkeypatch.setenv("KS_SPLIT_MIN_CHUNKS", "0")
    c = SP.corpus(seam, vset, *units)
    assert c.sigma == units[0] * units[1] * 64
    tab = tables.get(ctx, form, vset, monkeypatch)
    what = f"{seam}/{vset} {form} {split}"
    _path(c, form, _regions_case(oracle, ctx, c, form, tab, what), what)


_THRESHOLDS = [(form, vset, seam, mw, ms, n) for form in ("lds", "plain-u16", "lines-u16") for vset in SP.VALUES
               for seam in ("chunk", "tile") for mw, ms, n in [(5, 6.0, 1), (6, 6.0, 0), (5, 6.5, 0)]]


@pytest.mark.parametrize("form,vset,seam,mw,ms,n", _THRESHOLDS, ids=["-".join(map(str, x[:5])) for x in _THRESHOLDS])
def test_threshold_equality(oracle, ctx, units, tables, monkeypatch, form, vset, seam, mw, ms, n):
    """Width 5 and score 6 exactly, across the seam: emitted at (5, 6.0), not
    at (6, 6.0) and not at (5, 6.5)."""
    c = SP.corpus(seam, vset, *units)
    tab = tables.get(ctx, form, vset, monkeypatch)
    what = f"{seam}/{vset} {form} thresholds ({mw}, {ms})"
    _regions_case(oracle, ctx, c, form, tab, what, mw, ms)
    if vset != "DRIFT":
        assert len(c.predict(FORMS[form][0], mw, ms)["threshold-equality"]) == n


@pytest.mark.parametrize("seam", list(SP.SEAMS))
@pytest.mark.parametrize("vset", ["INT", "DYADIC"])
def test_cached_layout_meets_the_seams(oracle, ctx, units, tables, monkeypatch, seam, vset):
    """One DeviceSeqs scanned twice, a build and then a hit of its sequence
    index, at another min_width: the cached run segmentation, packed bases
    and chunk layout meet the seams like the fresh ones."""
    from kmer_spans_amd import device as D
    form = "lds"
    k = FORMS[form][0]
    c = SP.corpus(seam, vset, *units)
    tab = tables.get(ctx, form, vset, monkeypatch)
    ds = D.from_host(c.sequences(k), "cuda")
    for i, (mw, ms) in enumerate([(MW, MS), (5, 3.0)]):
        what = f"{seam}/{vset} {form} index scan {i}"
        o = _oracle(oracle, c, k, "kmer_regions", mw, ms)
        pos, sc, st, vis = _scan(ctx, c, k, tab, mw, ms, ds)
        assert (st["ms_runs"] > 0) == (i == 0), (what, st["ms_runs"])
        _same(c, k, pos, sc, o, what)
        assert np.array_equal(vis, o["counts"]), (what, "visits")
        _predicted(c, k, pos, sc, mw, ms, what)
        assert (st["n_scored"], st["n_runs"]) == (c.n_scored, c.n_runs), what
    assert ds.seq_index().info() == {"builds": 1, "hits": 1, "layout_builds": 1, "guard_failures": 0}
