"""The planted-trajectory generator (tests/scanplant.py) against both CPU
oracles, and every plant against the seam its name claims.  No GPU.

The expectations below are written out per family in terms of the seam size
S alone, not taken from the generator: a plant that misses its seam by one
index fails here."""
import numpy as np
import pytest

from tests import scanplant as SP

K = 9
MW, MS = 1, 2.0
UNITS = (256, 16384, 1048576)


def _units():
    """(chunk, tile chunks): the library's when it loads, else the constants."""
    try:
        from kmer_spans_amd import _lib
        L = _lib.load()
    except (ImportError, OSError):
        return SP.CHUNK, SP.TILE_CHUNKS
    return int(L.ks_scan_chunk_indices()), int(L.ks_scan_tile_chunks())


def test_units_match_library():
    assert (SP.CHUNK, SP.TILE_CHUNKS, SP.WAVE) == (256, 64, 64)
    assert _units() == (SP.CHUNK, SP.TILE_CHUNKS)
    assert tuple(SP.seam_size(s, *_units()) for s in SP.SEAMS) == UNITS


def test_tables():
    for k in (1, 6, 9):
        for vset, v in SP.VALUES.items():
            w = SP.table(vset, k)
            assert w.size == 4 ** k and all(w[c] == v[c & 3] for c in (0, 1, 2, 3, 4 ** k - 1, 4 ** k // 2 + 1))
    assert SP.int_exact(SP.table("INT", 6))
    assert not SP.int_exact(SP.table("DYADIC", 6)) and not SP.int_exact(SP.table("DRIFT", 6))
    assert not SP.int_exact([1.0, 2.0 ** 20 + 1]) and not SP.int_exact([np.inf]) and SP.int_exact([-2.0 ** 20, 0.0])


# Regions (relative beg, relative end, score) each instance must give with
# (min_width, min_score) = (1, 2.0), and where its named feature sits.
def _expected(S):
    j0 = S - 41
    r_last = 3 if (2 * S - 1 - 3 - j0) % 2 == 0 else 4
    r_first = 3 if (2 * S - 3 - j0) % 2 == 0 else 4
    return {
        "closed-in-place": [(S - 1, S, 2.0)],
        "tie-across": [(S - 3, S - 2, 2.0)],
        "tied-span": [(j0, j0 + 1, 2.0)],
        "argmax-at-seam/last": [(j0, 2 * S - 1, 1.0 + r_last)],
        "argmax-at-seam/first": [(j0, 2 * S, 1.0 + r_first)],
        "reset-at-seam/on": [(S - 5, S - 1, 5.0), (S + 1, S + 3, 3.0)],
        "reset-at-seam/before": [(S - 6, S - 2, 5.0), (S, S + 2, 3.0)],
        "touch-zero/clamp": [(S - 5, S - 3, 3.0), (S + 1, S + 4, 4.0)],
        "touch-zero/twin": [(S - 4, S + 4, 5.0)],
        "open-at-end/-1": [(2 * S - 31, 2 * S - 2, 30.0)],
        "open-at-end/+0": [(2 * S - 30, 2 * S - 1, 30.0)],
        "open-at-end/+1": [(2 * S - 29, 2 * S, 30.0)],
        "threshold-equality": [(S - 3, S + 2, 6.0)],
    }


def _trajectory(body, v, lo, hi):
    """S over relative indices lo .. hi - 1 of a body, entered at a T."""
    assert lo == 0 or body[lo - 1] == ord("T")
    S, out = 0.0, {}
    for j in range(lo, hi):
        S = max(S + v[SP.BASES.index(int(body[j]))], 0.0)
        out[j] = S
    return out


@pytest.mark.parametrize("seam", SP.SEAMS)
def test_features_sit_on_their_seams(seam):
    """From the bytes themselves: the DYADIC trajectory around each planted
    event, the unit (chunk, tile or step of the run) of every begin, peak,
    tie and clamp, and the planted excursions against the written-out list."""
    c = SP.corpus(seam, "DYADIC", *_units())
    S = c.sigma
    assert S == UNITS[SP.SEAMS.index(seam)]
    v = SP.VALUES["DYADIC"]
    exp = _expected(S)
    inst = {x.name: x for x in c.instances}
    if seam != "step":
        assert set(exp) <= set(inst)
    for name, x in inst.items():
        if name in exp:
            assert x.exc == exp[name], name
    unit = lambda j: j // S  # noqa: E731

    def traj(name, lo, hi):
        return _trajectory(inst[name].body, v, lo, hi)

    if seam != "step":
        t = traj("closed-in-place", S - 2, S + 3)
        assert [t[j] for j in (S - 2, S - 1, S, S + 1)] == [0, 1, 2, 0]  # begins at the unit's last index, peaks on the next's first
        assert unit(S - 1) + 1 == unit(S) and S % S == 0
        t = traj("tie-across", S - 4, S + 3)
        assert [t[j] for j in range(S - 3, S + 2)] == [1, 2, 1, 2, 0] and unit(S - 2) != unit(S)
        t = traj("threshold-equality", S - 4, S + 5)
        assert [t[j] for j in range(S - 3, S + 4)] == [1, 2, 3, 4, 5, 6, 0]
        assert (S + 2) - (S - 3) == 5 and unit(S - 3) != unit(S + 2)
    # tied-span: 1, 2, 1, 2 ... from S - 41 over the whole of unit 1 and into unit 2
    x = inst["tied-span"]
    j0, end = S - 41, x.marks["clamp"]
    assert x.body[j0 - 1] == ord("T") and x.body[j0] == ord("A") and x.body[end] == ord("T")
    assert np.array_equal(x.body[j0 + 1:end], np.tile(np.frombuffer(b"AC", dtype=np.uint8), (end - j0 - 1) // 2))
    assert unit(j0) == 0 and end > 2 * S + 40 and unit(end) == 2 and (end - j0) % 2 == 1
    for c0 in range(S // 256, 2 * S // 256 + 1, max(1, S // 256 // 7)):  # entry of spanned chunks: S = 1 or 2, never 0
        assert x.body[256 * c0 - 1] in b"AC" and 256 * c0 > j0
    # argmax-at-seam: the only maximum on the last index of unit 1, and on the first of unit 2
    for tag, tpos in (("last", 2 * S - 1), ("first", 2 * S)):
        x = inst[f"argmax-at-seam/{tag}"]
        (b, e, s), = x.exc
        assert (b, e) == (S - 41, tpos) and x.body[e + 1] == ord("T") and x.body[b - 1] == ord("T")
        r = int(s) - 1
        assert bytes(x.body[e - r + 1:e + 1]) == b"A" * r and x.body[e - r] == ord("C")
        assert np.array_equal(x.body[b + 1:e - r + 1], np.tile(np.frombuffer(b"AC", dtype=np.uint8), (e - r - b) // 2))
        assert (e - r - b) % 2 == 0 and s > 2.0
    assert unit(2 * S - 1) == 1 and unit(2 * S) == 2 and (2 * S - 1) % 256 == 255 and (2 * S) % 256 == 0
    # reset-at-seam: the clamp on the first index of unit 1 (hq == 0), and on the last of unit 0
    for tag, cpos in (("on", S), ("before", S - 1)):
        x = inst[f"reset-at-seam/{tag}"]
        t = _trajectory(x.body, v, cpos - 6, cpos + 6)
        assert [t[j] for j in range(cpos - 5, cpos + 5)] == [1, 2, 3, 4, 5, 0, 1, 2, 3, 0], tag
        assert x.marks["clamp"] == cpos and x.body[cpos] == ord("T")
    assert S % 256 == 0 and S % S == 0 and (S - 1) % 256 == 255
    # touch-zero: exactly 0 on S without a negative sum; the twin is at 1 there
    x = inst["touch-zero/clamp"]
    raw, t = 0.0, _trajectory(x.body, v, S - 6, S + 7)
    for j in range(S - 5, S + 1):
        raw += v[SP.BASES.index(int(x.body[j]))]
        assert raw >= 0
    assert raw == 0 and [t[j] for j in range(S - 5, S + 6)] == [1, 2, 3, 2, 1, 0, 1, 2, 3, 4, 0]
    t = _trajectory(inst["touch-zero/twin"].body, v, S - 5, S + 7)
    assert [t[j] for j in range(S - 4, S + 6)] == [1, 2, 3, 2, 1, 2, 3, 4, 5, 0] and t[S] == 1
    # open-at-end: the run's last scan index is the last of unit 1, or the first or second of unit 2
    for d in (-1, 0, 1):
        x = inst[f"open-at-end/{d:+d}"]
        assert x.P == 2 * S + d and bytes(x.body[-30:]) == b"A" * 30 and x.body[-31] == ord("T")
        assert np.all(x.body[:-30] == ord("T"))
    # run-length: the last unit holds 255, 256, 1 and 2 members (chunk) or is missing
    ds = (-1, 0, 1) if seam == "step" else (-2, -1, 0, 1, 2)
    assert [inst[f"run-length/{d:+d}"].P for d in ds] == [S + d for d in ds]
    for d in ds:
        assert set(bytes(inst[f"run-length/{d:+d}"].body)) == set(b"ACGT")
    # the step corpus holds the spanning and seam-index families only
    fams = {x.family for x in c.instances}
    if seam == "step":
        assert fams == {"lead", "tied-span", "argmax-at-seam", "reset-at-seam", "touch-zero", "open-at-end",
                        "run-length"}
    else:
        assert fams == {"lead", "closed-in-place", "tie-across", "tied-span", "argmax-at-seam", "reset-at-seam",
                        "touch-zero", "open-at-end", "threshold-equality", "run-length"}
    d = SP.corpus(seam, "DRIFT", *_units())
    x = {y.name: y for y in d.instances}["drift-span"]
    n = S + 3000
    assert np.all(x.body[:1000] == ord("T")) and x.body[1000 + 2 * n] == ord("T")
    assert np.array_equal(x.body[1000:1000 + 2 * n], np.tile(np.frombuffer(b"AC", dtype=np.uint8), n))
    assert all(y.exc is None for y in d.instances)


@pytest.mark.parametrize("seam", SP.SEAMS)
@pytest.mark.parametrize("vset", list(SP.VALUES))
def test_layout(seam, vset):
    """Runs, gaps and counts: every run of the genome is one instance at the
    position the layout says; the long runs start inside a global tile; sizes
    stay small."""
    from oracle import pyoracle as P
    c = SP.corpus(seam, vset, *_units())
    total = {}
    for k in (6, 9, 12):
        seqs = c.sequences(k)
        total[k] = sum(len(s) for s in seqs)
        lay = c.layout(k)
        assert len({x.name for x, _, _ in lay}) == len(lay) == c.n_runs
        assert c.n_scored == sum(x.P for x, _, _ in lay)
        if seam != "step":
            runs = [(q, a, b) for q, s in enumerate(seqs) for a, b in P.runs(s, k)]
            assert runs == [(q, a, a + x.P + k) for x, q, a in lay]
        chunks = 0
        for x, q, a in lay:
            s = seqs[q]
            assert s[a:a + k - 1] == b"T" * (k - 1) and s[a + k - 1:a + k - 1 + x.P] == x.body.tobytes()
            assert (a == 0 or s[a - 1:a] == b"N") and (a + x.P + k == len(s) or s[a + x.P + k:a + x.P + k + 1] == b"N")
            if x.P > 2 * c.sigma and seam != "chunk":
                assert chunks % 64 != 0, x.name  # starts inside a global tile
            chunks += -(-x.P // c.chunk)
        assert len(seqs) >= 2 and seqs[1][:1] == b"N" and seqs[0][:1] != b"N" and seqs[-1][-1:] != b"N"
    limit = {"chunk": 100_000, "tile": 1_000_000, "step": 40_000_000}[seam]
    assert total[12] <= limit, total


def _as_list(r):
    return [(int(r["pos"][0, i]), int(r["pos"][1, i]), int(r["pos"][2, i]),
             int(r["score"][0:1].view(np.uint64)[0, i])) for i in range(r["pos"].shape[1])]


def _bits(regs):
    return [(q, b, e, int(np.float64(s).view(np.uint64))) for q, b, e, s in regs]


# (the step corpus has no threshold-equality instance: one threshold pair there)
_THRESHOLDS = [(seam, mw, ms) for seam in SP.SEAMS for mw, ms in [(MW, MS), (5, 6.0), (6, 6.0), (5, 6.5)]
               if seam != "step" or (mw, ms) == (MW, MS)]


@pytest.mark.parametrize("seam,mw,ms", _THRESHOLDS)
@pytest.mark.parametrize("vset", ["INT", "DYADIC"])
def test_prediction_and_oracles_agree(oracle, seam, vset, mw, ms):
    """The planted prediction, the C oracle and (chunk and tile seams) the
    pure-Python oracle: same regions, same score bits, same visits."""
    c = SP.corpus(seam, vset, *_units())
    seqs = c.sequences(K)
    w = SP.table(vset, K)
    o = oracle.scan(seqs, K, w, 0.0, mw, ms, visits=True)
    assert int(o["counts"].astype(np.int64).sum()) >= c.n_scored
    if seam != "step":
        from oracle import pyoracle as P
        regs, vis = P.regions(seqs, K, w, 0.0, mw, ms)
        assert _as_list(o) == _bits(regs)
        assert np.array_equal(o["counts"], vis)
    got = c.by_instance(K, o["pos"], o["score"])
    want = c.predict(K, mw, ms)
    rel = {x.name: a + K for x, _, a in c.layout(K)}
    exp = _expected(c.sigma)
    for name, regs in want.items():
        assert _bits(got[name]) == _bits(regs), (seam, vset, name, got[name], regs)
        if (mw, ms) == (MW, MS):  # and the list written out above, relative to the run
            assert [(b - rel[name], e - rel[name], s) for _, b, e, s in regs] == exp[name], name
    if seam != "step":
        n = len(want["threshold-equality"])
        assert n == (1 if (mw, ms) in ((MW, MS), (5, 6.0)) else 0)
    assert set(want) == {x.name for x in c.instances if x.family not in ("lead", "run-length")}


@pytest.mark.parametrize("seam", SP.SEAMS)
def test_drift_corpus_oracles_agree(oracle, seam):
    """DRIFT has no prediction: the two oracles agree (chunk and tile seams),
    the tied plants and the drift span each give regions, and the drift span
    is one excursion across more than a whole unit."""
    c = SP.corpus(seam, "DRIFT", *_units())
    seqs = c.sequences(K)
    w = SP.table("DRIFT", K)
    o = oracle.scan(seqs, K, w, 0.0, MW, MS, visits=True)
    if seam != "step":
        from oracle import pyoracle as P
        regs, vis = P.regions(seqs, K, w, 0.0, MW, MS)
        assert _as_list(o) == _bits(regs) and np.array_equal(o["counts"], vis)
    got = c.by_instance(K, o["pos"], o["score"])
    rel = {x.name: a + K for x, _, a in c.layout(K)}
    (q, b, e, s), = got["drift-span"][:1]
    assert b - rel["drift-span"] == 1000 and e - b > c.sigma and s > 0.09 * c.sigma
    assert got["tied-span"] and got["argmax-at-seam/last"] and got["argmax-at-seam/first"]


def test_explain_names_the_instance(oracle):
    c = SP.corpus("chunk", "DYADIC", *_units())
    o = oracle.scan(c.sequences(K), K, SP.table("DYADIC", K), 0.0, MW, MS)
    assert c.explain(K, o["pos"], o["score"], o["pos"], o["score"]) == []
    pos = o["pos"].copy()
    lay = {x.name: (q, a) for x, q, a in c.layout(K)}
    q, a = lay["tie-across"]
    hit = np.flatnonzero((pos[0] == q) & (pos[1] == a + K + c.sigma - 3))
    assert hit.size == 1
    pos[2, hit[0]] += 2  # the later of the tied maxima
    lines = c.explain(K, pos, o["score"], o["pos"], o["score"])
    assert len(lines) == 1 and "tie-across" in lines[0] and f"({c.sigma - 3}, {c.sigma}, 2.0)" in lines[0]
