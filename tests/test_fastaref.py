"""The books of tests/fastaref.py are right, and the texts the GPU test runs
(test_gpu_ingest_seams.py) are not vacuous.  CPU only: the C oracle's
sequential reader (orc_fasta_parse) is the yardstick here; the device reader
is not involved.
"""
import gzip
import hashlib

import numpy as np
import pytest

from tests import fastaref as F
from tests.fastaref import L, T, W


def _pin(oracle, c, min_lens=None):
    """The oracle reads c.text as the builder's books say, at every min_len the GPU test uses."""
    if c.error is not None:
        kind, pos = c.error
        word = {"invalid": "invalid byte", "before": "sequence before description"}[kind]
        with pytest.raises(oracle.OracleError) as e:
            oracle.fasta_parse(c.text)
        assert str(e.value) == f"{word} at {pos}", c.id
        return
    for ml in (0, c.min_len) if min_lens is None else min_lens:
        assert oracle.fasta_parse(c.text, ml) == c.expected(ml), (c.id, ml)


def _line_start(text, p):
    return p == 0 or text[p - 1:p] == b"\n"


# ------------------------------------------------------------------ line starts

@pytest.mark.parametrize("event", F.LINE_EVENTS)
def test_line_start_cases(oracle, event):
    seam = set()
    for o in F.O:
        c = F.place(event, o)
        _pin(oracle, c)
        p = c.marks["line"]
        assert p == o and _line_start(c.text, p), c.id
        first = {"desc": b">", "comment": b";", "empty": b"\n", "crlf_only": b"\r\n"}.get(event)
        if first is None:
            assert c.text[p] in F.VALID
        else:
            assert c.text[p:p + len(first)] == first, c.id
        if event == "desc":
            assert "at the seam" in c.names and c.text[p:].split(b"\n")[1][:1] not in (b">", b";", b"")
        e = c.expected(c.min_len)
        assert 0 < len(e["seqs"]) < e["n_records"], c.id   # the non-zero min_len runs the selection
        seam |= {("lane", o % L == 0), ("tile", o % T == 0), ("wave", o % W == 0),
                 ("lane end", o % L == L - 1), ("tile end", o % T == T - 1)}
    assert {k for k, v in seam if v} == {"lane", "tile", "wave", "lane end", "tile end"}


# ------------------------------------------------------------------------ CR/LF

@pytest.mark.parametrize("event", F.CR_EVENTS)
def test_crlf_cases(oracle, event):
    lane_end = tile_end = 0
    for o in F.O:
        c = F.place_cr(event, o)
        _pin(oracle, c)
        assert c.marks["cr"] == o and c.text[o:o + 1] == b"\r", c.id
        lane_end += o % L == L - 1
        tile_end += o % T == T - 1
        if event in ("crlf_seq", "crlf_desc"):
            assert c.text[o + 1:o + 2] == b"\n" and len(c.text) > o + 2
        if event in ("cr_eof_seq", "cr_eof_desc"):
            assert len(c.text) == o + 1
        if event in ("crlf_desc", "cr_eof_desc"):
            assert c.text[o - 4:o] == b">abc" and "abc" in c.names and c.error is None
        if event in ("crlf_seq", "cr_eof_seq"):
            assert c.text[o - 1] in F.VALID and c.error is None
        if event == "cr_lone":
            assert c.error == ("invalid", o) and c.text[o + 1] in F.VALID and c.text[o - 1] in F.VALID
    # the 17th byte comes from the next lane, and from the next tile
    assert lane_end >= 2 and tile_end >= 2


# -------------------------------------------------------------------------- EOF

@pytest.mark.parametrize("event", F.EOF_EVENTS)
def test_eof_cases(oracle, event):
    for n in F.EOF_N:
        c = F.place_eof(event, n)
        _pin(oracle, c)
        assert len(c.text) == n, c.id
        last = c.text[-1:]
        if event == "eof_base":
            assert last[0] in F.VALID
            assert (c.error == ("before", 0)) == (n < 15)
            if c.error is None:
                assert c.seqs[-1][-1:] == last.upper()
        elif event == "eof_nl":
            assert last == b"\n" and c.error is None
        elif event == "eof_desc":
            line = c.text.split(b"\n")[-1]
            assert line[:1] == b">" and c.error is None and c.names[-1] == line[1:].decode() and c.seqs[-1] == b""
        elif event == "eof_gt":
            assert last == b">" and _line_start(c.text, n - 1) and c.names[-1] == "" and c.seqs[-1] == b""
    # the three ways the 16 + 1 byte load ends: 16k + 15, 16k + 16, 16k + 17 bytes
    assert {n % L for n in F.EOF_N} >= {L - 1, 0, 1}


# ------------------------------------------------------------------- long lines

def test_long_line_cases(oracle):
    cases = F.long_line_cases()
    assert len(cases) == 3 * len(F.LONG_LENS) * len(F.LONG_STARTS) + len(F.LONG_STARTS)
    for c in cases:
        _pin(oracle, c)
        kind, length, start = c.tags["kind"], c.tags["length"], c.tags["start"]
        assert c.marks["line"] == start and _line_start(c.text, start), c.id
        line = c.text[start:].split(b"\n")[0]
        assert len(line) == length, c.id
        # a whole tile without a line break lives on the carried value: every line that covers
        # one has it (all but the lines of T - 1 bytes, and of T bytes off a tile edge)
        nl = np.flatnonzero(np.frombuffer(c.text, dtype=np.uint8) == 10)
        tiles = np.setdiff1d(np.arange(len(c.text) // T), nl // T)
        covers = -(-start // T) * T + T <= start + length
        assert (tiles.size > 0) == covers == (length > T or (length == T and start % T == 0)), c.id
        if kind == "seq":
            assert c.error is None and any(len(s) >= length for s in c.seqs)
            continue
        for b in (b">", b";", b"\r", b"*", b"\xff") + ((b"\0",) if kind != "desc" else ()):
            assert b in line[1:], (c.id, b)
        # a '>' on the first byte of every tile the line reaches, and no error from any of it
        for t in range(start // T + 1, (start + length - 4) // T + 1):
            assert c.text[t * T:t * T + 1] == b">", (c.id, t)
        assert c.error is None and b"\r\n" not in line
        if kind == "desc":
            assert line[1:].decode("latin-1") in c.names and b"\0" not in line
        if kind == "desc_nul":
            assert line.index(b"\0") == length - 3 and line[1:length - 3].decode("latin-1") in c.names
        if kind == "comment":
            assert line[:1] == b";" and len(c.names) == 3
    assert sum(1 for c in cases if c.tags["length"] > T) >= 20


# ---------------------------------------------------------------- dense records

def test_dense_cases(oracle):
    cases = {c.id: c for c in F.dense_cases()}
    assert len(cases) == 4
    for c in cases.values():
        _pin(oracle, c, (0, 1, 2))
    c = cases["dense-empty-records"]
    assert c.text == b">\n" * 5000 and c.names == [""] * 5000 and c.seqs == [b""] * 5000
    assert F.lanes_with_two_descriptions(c.text) == len(c.text) // L   # 8 per lane
    c = cases["dense-one-base"]
    assert c.text == b">x\nA\n" * 3000 and F.lanes_with_two_descriptions(c.text) > 900
    assert c.expected(1)["seqs"] == [b"A"] * 3000 and c.expected(2)["seqs"] == []
    c = cases["dense-newline-tile"]
    assert c.text[T:2 * T] == b"\n" * T and c.text[T - 1:T] == b"\n" and c.text[2 * T:2 * T + 1] != b"\n"
    c = cases["dense-mix"]
    a = np.frombuffer(c.text, dtype=np.uint8)
    assert c.text[:2 * T] == b">\n" * T                                  # tiles that keep no byte
    assert not (a[2 * T:4 * T] == ord(">")).any()                        # tiles without a record
    assert c.text[4 * T:5 * T] == b";" + b"c" * (T - 2) + b"\n"
    assert set(c.text[5 * T:6 * T]) == {10, 13}
    assert F.lanes_with_two_descriptions(c.text) >= 2 * T // L
    assert {len(s) for s in c.seqs} >= {0, 1, 2}
    for ml in (1, 2):
        e = c.expected(ml)
        assert 0 < len(e["seqs"]) < e["n_records"]


# -------------------------------------------------------------------- selection

def test_select_cases(oracle):
    seen = set()
    for c in F.select_cases():
        assert sorted(set(map(len, c.seqs))) == sorted(F.SELECT_LENGTHS), c.id
        _pin(oracle, c, (0,) + F.SELECT_MIN_LEN)
        assert len(set(c.seqs[q] for q in range(len(c.seqs)) if c.seqs[q])) == len([s for s in c.seqs if s])
        assert any(ch in s for s in c.seqs for ch in b"RYKMSWBDHVN-+.")     # upper-cased IUPAC, not only ACGT
        assert any(ch in c.text for ch in b"acgtn")
        for ml in F.SELECT_MIN_LEN:
            lens = [len(s) for s in c.seqs]
            kept = [n >= ml for n in lens]
            if not any(kept):
                seen.add("all dropped")
                assert ml == 10 ** 9
                continue
            assert not all(kept), (c.id, ml)
            seen |= {"first dropped"} if not kept[0] else set()
            seen |= {"last dropped"} if not kept[-1] else set()
            seen |= {"one kept"} if sum(kept) == 1 else set()
            seen |= {f"start {s}" for s in c.kept_starts(ml) if s in (4095, 4096, 4097)}
    assert seen == {"all dropped", "first dropped", "last dropped", "one kept", "start 4095", "start 4096",
                    "start 4097"}


# ------------------------------------------------------------- error precedence

def test_error_cases(oracle):
    cases = {c.id: c for c in F.error_cases()}
    for c in cases.values():
        _pin(oracle, c)
    assert cases["err-before-small-0"].text == b"AC\n>a\nAZ\n" and cases["err-before-small-0"].error == ("before", 0)
    assert cases["err-before-small-1"].text == b"Z\n>a\nAC\n" and cases["err-before-small-1"].error == ("before", 0)
    for key, tiles in (("err-tiles-0-5", (0, 5)), ("err-tiles-5-9", (5, 9)), ("err-every-tile-40", range(40)),
                       ("err-0x80", (1, 2)), ("err-0x00", (1, 2))):
        c = cases[key]
        bad = [p for p, ch in enumerate(c.text) if ch not in F.VALID and ch not in b"\n>" and p > 2]
        assert sorted({p // T for p in bad}) == list(tiles), key
        assert c.error == ("invalid", bad[0]) and bad[0] // T == min(tiles)
    assert cases["err-0x80"].text[cases["err-0x80"].error[1]] == 0x80
    assert cases["err-0x00"].text[cases["err-0x00"].error[1]] == 0
    c = cases["err-before-late-desc"]
    assert c.error == ("before", 4) and c.text.index(b"\n>") + 1 == 3 * T + 5
    assert all(ch in F.VALID or ch == 10 for ch in c.text[4:3 * T + 5])
    c = cases["err-before-then-invalid"]
    assert c.error == ("before", 1) and c.text.index(b"*") < T < c.text.index(b"\n>")
    assert cases["err-before-no-desc"].error == ("before", 0) and cases["err-before-no-desc"].text == b"*\n"
    c = cases["err-none-comment-first"]
    assert c.error is None and c.text[:1] == b";" and c.text.index(b"\n>") > T and c.names[0] == "first"


# ---------------------------------------------------------------------- padding

def test_padding_cases(oracle):
    for c in F.padding_cases():
        _pin(oracle, c)
        r = c.tags["residue"]
        all_, kept = c.expected(0), c.expected(c.min_len)
        assert sum(map(len, all_["seqs"])) % 32 == r and sum(map(len, kept["seqs"])) % 32 == r
        assert len(kept["seqs"]) == len(all_["seqs"]) - 1 and all_["seqs"][-1].endswith(b"AAAA")
        assert len(c.text) > T


# ------------------------------------------------------------------ upload ring

def test_ring_text(oracle):
    text, names, digests = F.ring_text()
    assert len(text) == 2 * (64 << 20) + (5 << 20)
    o = oracle.fasta_parse(text)
    assert o["names"] == names and len(names) >= 16
    assert [(len(s), hashlib.sha256(s).hexdigest()) for s in o["seqs"]] == digests
    assert o["bases_all"] == sum(n for n, _ in digests)
    # every 64 MiB piece differs and carries a record boundary
    pieces = [text[i:i + F.RING_PIECE] for i in range(0, len(text), F.RING_PIECE)]
    assert len(pieces) == 3 and len(pieces[2]) >= 4 << 20      # (the threaded copy takes pieces >= 4 MiB)
    assert all(b"\n>" in p for p in pieces)
    assert pieces[0][:len(pieces[2])] != pieces[2] and pieces[0] != pieces[1]
    assert len(set(d for _, d in digests)) == len(digests)


# ------------------------------------------------------------------------- gzip

def test_gzip_text(oracle):
    z = gzip.compress(F.GZIP_TEXT)
    assert len(F.GZIP_TEXT) > 4 * len(z) and len(F.GZIP_TEXT) > 1 << 20   # outgrows the first buffer
    o = oracle.fasta_parse(F.GZIP_TEXT)
    assert o["names"] == ["a"] and o["seqs"] == [b"ACGT" * 750_000]
    assert gzip.decompress(gzip.compress(b"")) == b"" and gzip.compress(b"")[:2] == b"\x1f\x8b"
    assert oracle.fasta_parse(b">") == {"names": [""], "seqs": [b""], "n_records": 1, "bases_all": 0}
