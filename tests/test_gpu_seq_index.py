"""Sequence index (ks_seq_index, include/kmer_spans.h): repeated scans of one
DeviceSeqs reuse the previous scan's run segmentation, packed codes and chunk
layout from the context's slots.  Every reuse must give the regions, FP64
scores and visits of the oracle bit for bit, every event that rewrites or
frees those slots must turn the next scan into a build, and a change of the
bytes under a live handle must be refused by the guard with a status.

"Equal" below: regions and scores bitwise equal to oracle.scan /
oracle.tr_lr_regions (and visits where taken)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KS_ERR_ARG = 1


def _same(pos, sc, o, what):
    assert pos.shape == o["pos"].shape, (what, pos.shape, o["pos"].shape)
    assert np.array_equal(pos, o["pos"]), what
    assert np.array_equal(sc.view(np.uint64), o["score"].view(np.uint64)), what


def _contigs(torch, genome, seed):
    """Two contigs of 600 / 300 kbp (37 stitch tiles in the longest run's
    neighbourhood) with interior N gaps, a lower-case stretch, and one contig
    shorter than k."""
    a = genome.contig(600_000, seed, device="cuda")
    b = genome.contig(300_017, seed + 1, device="cuda")
    n = ord("N")
    a[150_000:150_700] = n
    a[420_003:420_010] = n
    a[200_000:201_000] |= 0x20  # lower case
    b[0:33] = n
    b[120_000:121_111] = n
    short = torch.tensor(list(b"ACGTA"), dtype=torch.uint8, device="cuda")
    return [a, b, short]


class _Setup:
    pass


@pytest.fixture(scope="module")
def setup(oracle):
    """The inputs, their tables and the oracle's results, computed once."""
    import torch
    from kmer_spans_amd import _lib, api, device as D, genome
    S = _Setup()
    S.torch, S.D, S.lib, S.api = torch, D, _lib, api
    S.ctx = _lib.Context(0)
    D.bind_torch_stream(S.ctx)
    parts = _contigs(torch, genome, 41)
    S.lens = [int(p.numel()) for p in parts]
    S.parts = parts
    S.A = D.from_parts(parts, S.lens, "cuda")
    S.host = [S.A.host_seq(q) for q in range(S.A.nseq)]
    partsb = _contigs(torch, genome, 57)[:2]
    S.B = D.from_parts(partsb, [int(p.numel()) for p in partsb], "cuda")
    S.hostb = [S.B.host_seq(q) for q in range(S.B.nseq)]
    S.w, S.tab, S.o = {}, {}, {}
    for k in (9, 11):
        counts = torch.zeros(4 ** k, dtype=torch.int32, device="cuda")
        D.count(S.ctx, S.A, k, counts)
        c = counts.cpu().numpy()
        for score, mw, ms in (("log2", 30, 3.0), ("pm1", 20, 5.0)):
            w = api.log2_table(c, k) if score == "log2" else api.pm1_table(c, k)
            S.w[k, score] = w
            S.tab[k, score] = D.DeviceTable(S.ctx, w, k, 0.0, compress=True, expand=True)
            S.o[k, score] = oracle.scan(S.host, k, w, 0.0, mw, ms, visits=True)
    S.par = {"log2": (30, 3.0), "pm1": (20, 5.0)}
    S.ob = oracle.scan(S.hostb, 9, S.w[9, "log2"], 0.0, 30, 3.0)
    S.init = D.DeviceTable(S.ctx, S.w[9, "pm1"], 9, 0.0, compress=False)
    S.otr = oracle.tr_lr_regions(S.host, 9, 25, S.w[9, "pm1"], S.w[9, "pm1"])
    yield S
    for t in list(S.tab.values()) + [S.init]:
        t.close()
    S.ctx.close()


@pytest.fixture(autouse=True)
def _chunked(setup, monkeypatch):
    monkeypatch.delenv("KS_NO_SEQ_INDEX", raising=False)
    setup.ctx.set_scan_algo(1)
    yield
    setup.ctx.set_scan_algo(-1)


def _fresh(S):
    """A's bytes and offsets under a new DeviceSeqs (so a new handle)."""
    return S.D.from_parts(S.parts, S.lens, "cuda")


def _scan(S, ds, k=9, score="log2", vis=None, ctx=None):
    mw, ms = S.par[score]
    return S.D.scan(ctx or S.ctx, ds, k, S.tab[k, score], mw, ms, vis)


def test_three_scans_one_build(setup, monkeypatch):
    S = setup
    ds = _fresh(S)
    for i in range(3):
        pos, sc, st = _scan(S, ds)
        _same(pos, sc, S.o[9, "log2"], ("scan", i))
        assert st["scan_algo"] == 1
        assert (st["ms_runs"] > 0) if i == 0 else (st["ms_runs"] == 0), (i, st["ms_runs"])
    assert ds.seq_index().info() == {"builds": 1, "hits": 2, "layout_builds": 1, "guard_failures": 0}
    monkeypatch.setenv("KS_NO_SEQ_INDEX", "1")  # the plain entry: recomputes, counts nothing
    pos, sc, st = _scan(S, ds)
    _same(pos, sc, S.o[9, "log2"], "no index")
    assert st["ms_runs"] > 0
    assert ds.seq_index().info()["builds"] == 1 and ds.seq_index().info()["hits"] == 2


@pytest.mark.parametrize("score", ["log2", "pm1"])
def test_k_changes_rebuild_the_layout_only(setup, score):
    S = setup
    ds = _fresh(S)
    for i, k in enumerate((9, 11, 9)):
        pos, sc, st = _scan(S, ds, k, score)
        _same(pos, sc, S.o[k, score], ("k", k, i))
    # one run segmentation; a layout for the first scan and one per change of k
    assert ds.seq_index().info() == {"builds": 1, "hits": 2, "layout_builds": 3, "guard_failures": 0}


def test_scan_trlr_scan(setup):
    S = setup
    ds = _fresh(S)
    pos, sc, _ = _scan(S, ds, 9, "pm1")
    _same(pos, sc, S.o[9, "pm1"], "scan 1")
    pos, sc, st = S.D.tr_lr(S.ctx, ds, 9, S.tab[9, "pm1"], S.init, 25)
    _same(pos, sc, S.otr, "tr_lr")
    assert st["ms_runs"] == 0
    pos, sc, _ = _scan(S, ds, 9, "pm1")
    _same(pos, sc, S.o[9, "pm1"], "scan 2")
    pos, sc, _ = S.D.tr_lr(S.ctx, ds, 9, S.tab[9, "pm1"], S.init, 25)
    _same(pos, sc, S.otr, "tr_lr 2")
    # the layout differs by the scan kind: rebuilt at every switch
    assert ds.seq_index().info() == {"builds": 1, "hits": 3, "layout_builds": 4, "guard_failures": 0}


def test_two_genomes_alternating(setup):
    S = setup
    a = _fresh(S)
    pos, sc, _ = _scan(S, a)
    _same(pos, sc, S.o[9, "log2"], "A")
    pos, sc, _ = _scan(S, S.B)
    _same(pos, sc, S.ob, "B")
    pos, sc, st = _scan(S, a)
    _same(pos, sc, S.o[9, "log2"], "A again")
    assert st["ms_runs"] > 0
    assert a.seq_index().info() == {"builds": 2, "hits": 0, "layout_builds": 2, "guard_failures": 0}


class _DefaultCtx:
    """The process default context (the one api.kmer_regions runs on)."""

    def __init__(self, lib):
        self.handle = C.c_void_p(lib.load().ks_default_ctx())
        self.stream = -1
        assert self.handle.value


@pytest.mark.parametrize("between", ["windowed", "host_entry", "release_cache"])
def test_invalidation_between_scans(setup, oracle, between):
    S = setup
    torch, D = S.torch, S.D
    ctx = S.ctx
    tab, close = S.tab[9, "log2"], []
    if between != "windowed":  # the host entries of device 0 run on the default context
        ctx = _DefaultCtx(S.lib)
        check = S.lib.check
        check(S.lib.load().ks_ctx_set_scan_algo(ctx.handle, 1))
        tab = D.DeviceTable(ctx, S.w[9, "log2"], 9, 0.0, compress=True, expand=True)
        close.append(tab)
    try:
        ds = _fresh(S)
        small = [b"ACGTTGCANNACGTACGTACGGGGTTTACA" * 50]
        if between == "release_cache":  # lists the context for ks_release_cache
            S.api.kmer_regions(small, 3, np.arange(64, dtype=np.float64) - 31.0, 2, 1.0)
        for i in range(2):
            pos, sc, st = D.scan(ctx, ds, 9, tab, 30, 3.0)
            _same(pos, sc, S.o[9, "log2"], (between, i))
        assert ds.seq_index().info()["hits"] == 1 and st["ms_runs"] == 0
        if between == "windowed":
            dist = torch.zeros(2 * 51, dtype=torch.int32, device="cuda")
            D.windowed(ctx, ds, np.array([0, 27], dtype=np.uint32), 4, 50, dist)
        elif between == "host_entry":
            w3 = np.arange(64, dtype=np.float64) - 31.0
            g = S.api.kmer_regions(small, 3, w3, 2, 1.0)
            assert np.array_equal(g["pos"], oracle.kmer_regions(small, 3, w3, 2, 1.0)["pos"])
        else:
            S.lib.load().ks_release_cache()
        pos, sc, st = D.scan(ctx, ds, 9, tab, 30, 3.0)
        _same(pos, sc, S.o[9, "log2"], (between, "after"))
        assert st["ms_runs"] > 0
        assert ds.seq_index().info() == {"builds": 2, "hits": 1, "layout_builds": 2, "guard_failures": 0}
    finally:
        for t in close:
            t.close()
        if between != "windowed":
            S.lib.load().ks_ctx_set_scan_algo(ctx.handle, -1)


def test_torch_write_gives_a_new_index(setup, oracle):
    S = setup
    ds = _fresh(S)
    pos, sc, _ = _scan(S, ds)
    _same(pos, sc, S.o[9, "log2"], "before")
    old = ds.seq_index()
    ds.seq[300_000:300_050] = ord("N")
    pos, sc, st = _scan(S, ds)
    assert ds.seq_index() is not old and st["ms_runs"] > 0
    host = [ds.host_seq(q) for q in range(ds.nseq)]
    assert host[0][300_000:300_050] == b"N" * 50
    _same(pos, sc, oracle.scan(host, 9, S.w[9, "log2"], 0.0, 30, 3.0), "after the write")
    assert ds.seq_index().info() == {"builds": 1, "hits": 0, "layout_builds": 1, "guard_failures": 0}


def _scan_c(S, s, ixh, k=9):
    """ks_scan_dev_indexed directly: (status, message, regions struct)."""
    L = S.lib.load()
    r = S.lib.Regions()
    st = S.lib.ScanStats()
    S.torch.cuda.synchronize()
    rc = L.ks_scan_dev_indexed(S.ctx.handle, C.byref(s), ixh, k, S.tab[k, "log2"]._h, 30, 3.0, None, C.byref(r),
                               C.byref(st))
    return rc, L.ks_last_error().decode(errors="replace"), r


def test_guard_refuses_changed_bytes(setup, oracle):
    """A contract violation: the first N of a gap becomes a base while the
    handle lives.  The hit call is refused by the guard's flag, a status."""
    S = setup
    ds = _fresh(S)
    pos, sc, _ = _scan(S, ds)
    _same(pos, sc, S.o[9, "log2"], "before")
    h = ds.seq_index()  # kept: the C entry is called with it after the write
    assert S.host[0][150_000:150_001] == b"N" and S.host[0][149_999:150_000] != b"N"
    ds.seq[150_000] = ord("A")
    rc, msg, r = _scan_c(S, ds.struct(), h._h)
    assert rc == KS_ERR_ARG and "sequence bytes changed under a sequence index" in msg, (rc, msg)
    assert r.n == 0 and not r.seq_id
    assert h.info() == {"builds": 1, "hits": 1, "layout_builds": 1, "guard_failures": 1}
    pos, sc, st = _scan(S, ds)  # (a fresh handle: the tensor's version moved)
    assert ds.seq_index() is not h and st["ms_runs"] > 0
    host = [ds.host_seq(q) for q in range(ds.nseq)]
    _same(pos, sc, oracle.scan(host, 9, S.w[9, "log2"], 0.0, 30, 3.0), "fresh handle")


def test_visits_on_a_hit(setup):
    S = setup
    ds = _fresh(S)
    for i in range(2):
        vis = S.torch.zeros(4 ** 9, dtype=S.torch.int32, device="cuda")
        pos, sc, st = _scan(S, ds, vis=vis)
        _same(pos, sc, S.o[9, "log2"], ("visits", i))
        assert np.array_equal(vis.cpu().numpy(), S.o[9, "log2"]["counts"]), i
    assert ds.seq_index().info()["hits"] == 1


def test_lane_kernel_on_a_hit(setup):
    S = setup
    ds = _fresh(S)
    S.ctx.set_scan_algo(0)
    for i in range(2):
        vis = S.torch.zeros(4 ** 9, dtype=S.torch.int32, device="cuda")
        pos, sc, st = _scan(S, ds, vis=vis)
        assert st["scan_algo"] == 0
        _same(pos, sc, S.o[9, "log2"], ("lane", i))
        assert np.array_equal(vis.cpu().numpy(), S.o[9, "log2"]["counts"]), i
    assert ds.seq_index().info()["hits"] == 1 and st["ms_runs"] == 0


@pytest.mark.parametrize("seqs", [[b"N" * 5000, b"NNN"], [b"ACGTA", b"ACG", b"NNACGTNN"]])
def test_nothing_to_scan(setup, seqs):
    S = setup
    ds = S.D.from_host(seqs, "cuda")
    for i in range(2):
        pos, sc, st = _scan(S, ds)
        assert pos.shape == (3, 0) and sc.shape == (2, 0)
    assert ds.seq_index().info() == {"builds": 1, "hits": 1, "layout_builds": 1, "guard_failures": 0}


def test_handle_and_seqs_must_match(setup):
    S = setup
    ds = _fresh(S)
    h = ds.seq_index()
    s = ds.struct()
    s.seq += 16
    rc, msg, r = _scan_c(S, s, h._h)
    assert rc == KS_ERR_ARG and "do not match the sequence index" in msg and r.n == 0, (rc, msg)
    s = ds.struct()
    s.nseq -= 1
    rc, msg, r = _scan_c(S, s, h._h)
    assert rc == KS_ERR_ARG and "do not match the sequence index" in msg, (rc, msg)
    offs = ds.offsets.copy()
    offs[1] -= 1
    s = ds.struct()
    s.offsets_host = offs.ctypes.data
    rc, msg, r = _scan_c(S, s, h._h)
    assert rc == KS_ERR_ARG and "do not match the sequence index" in msg, (rc, msg)
    assert h.info() == {"builds": 0, "hits": 0, "layout_builds": 0, "guard_failures": 0}
    rc, msg, r = _scan_c(S, ds.struct(), None)  # no handle: the plain entry
    assert rc == 0, msg
    pos, sc = S.lib.regions_to_numpy(r)
    _same(pos, sc, S.o[9, "log2"], "NULL index")
    assert h.info()["builds"] == 0


def test_buffers_grow_on_a_hit(setup, oracle):
    """A fresh context's region, candidate and rescan lists hold 65,536
    entries (1,024 per segment).  The first scan (a build) finds nothing and
    leaves them at that; the tr_lr scan after it is a hit with more closed
    excursions than they hold, so it reruns on the cached runs with grown
    lists (KS_INTERNAL_RETRY) and must still end equal."""
    S = setup
    k = 6
    rng = np.random.default_rng(12)
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=3_000_003)].tobytes()
    seqs = [seq[:1_700_001], seq[1_700_001:]]
    tr = rng.normal(size=4 ** k) - 0.05
    ks = rng.normal(size=4 ** k)
    o = oracle.tr_lr_regions(seqs, k, 1, ks, tr)
    assert o["pos"].shape[1] > 65536, o["pos"].shape
    ctx = S.lib.Context(0)
    S.D.bind_torch_stream(ctx)
    ctx.set_scan_algo(1)
    ttr = S.D.DeviceTable(ctx, tr, k, 0.0, compress=True, expand=True)
    tks = S.D.DeviceTable(ctx, ks, k, 0.0, compress=False)
    try:
        ds = S.D.from_host(seqs, "cuda")
        pos, sc, st = S.D.scan(ctx, ds, k, ttr, 100_000, 1e12)
        assert pos.shape == (3, 0) and st["scan_algo"] == 1
        pos, sc, st = S.D.tr_lr(ctx, ds, k, ttr, tks, 1)
        assert st["scan_algo"] == 1 and st["ms_runs"] == 0
        _same(pos, sc, o, "tr_lr after growth")
        assert ds.seq_index().info() == {"builds": 1, "hits": 1, "layout_builds": 2, "guard_failures": 0}
    finally:
        ttr.close()
        tks.close()
        ctx.close()
