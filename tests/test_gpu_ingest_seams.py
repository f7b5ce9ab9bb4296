"""The device FASTA reader (csrc/ks_ingest.hip, fasta_from_view / upload in
csrc/ks_io.cpp) at tile, lane and upload seams.

The reference is the C oracle's sequential reader (oracle.fasta_parse); the
texts come from tests/fastaref.py, whose own books tests/test_fastaref.py
pins to the oracle on the CPU, together with the claim that every text holds
what it is built for.  Everything compared is a byte, an integer or a name:
every comparison is exact.

What is pinned:
  line starts   a description, a comment, a sequence line, an empty line and
                a CR LF line whose first byte is at 15 .. 3T around lane
                (16), wave (1024) and tile (4096) edges;
  CR LF         the CR on the last byte of a lane and of a tile (the LF is the
                lane's 17th byte), a CR that ends the file, a CR in mid-line;
  end of file   files of 1 .. 2T + 1 bytes ending in a base, a line break, a
                description line and a lone '>';
  long lines    descriptions, comments and sequence lines of T - 1 .. 3T + 1
                bytes: tiles without a line break, which live on the carried
                value, with '>' ';' CR '*' 0x00 0xff inside them;
  dense records eight description lines per lane, tiles that keep no byte,
                tiles without a record;
  selection     min_len against record lengths around 16, 32 and 4096, kept
                records starting at output offsets 4095, 4096, 4097;
  errors        the error is the sequential reader's: its kind, its line,
                its byte;
  padding       the 32 N after the bases, by counting over the parsed records;
  upload        a file of three 64 MiB staging pieces (the third reuses the
                first pinned half), a gzip file that outgrows its first buffer.
"""
import gzip
import hashlib
import re

import numpy as np
import pytest

from tests import fastaref as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from kmer_spans_amd import _lib
    return _lib.context(0)


@pytest.fixture(scope="module")
def D():
    from kmer_spans_amd import device
    return device


def _raises_like_oracle(D, ctx, text, err):
    """The device refuses text as the sequential reader does: err is the oracle's message."""
    import kmer_spans_amd as K
    m = re.fullmatch(r"(invalid byte|sequence before description) at (\d+)", err)
    pos = int(m.group(2))
    line = 1 + text[:pos].count(b"\n")
    with pytest.raises(K.KmerSpansError) as e:
        D.parse_fasta(ctx, text).close()
    msg = str(e.value)
    if m.group(1) == "invalid byte":
        c = text[pos]
        want = f"invalid one-letter sequence code '{chr(c) if 32 <= c <= 126 else '?'}' (0x{c:02x}) at line {line}"
    else:
        want = f"sequence data before the first description line (line {line})"
    assert msg.endswith(want), (msg, want)


def _check(D, ctx, oracle, text, min_lens, what):
    """D.parse_fasta(text) == oracle.fasta_parse(text) at every min_len; returns the oracle's results."""
    out = []
    for ml in min_lens:
        try:
            o = oracle.fasta_parse(text, ml)
        except oracle.OracleError as e:
            _raises_like_oracle(D, ctx, text, str(e))
            out.append(None)
            continue
        fa = D.parse_fasta(ctx, text, ml)
        try:
            assert fa.n_records == o["n_records"], (what, ml)
            assert fa.bases_all == o["bases_all"], (what, ml)
            assert fa.bases_kept == sum(map(len, o["seqs"])), (what, ml)
            assert fa.names == o["names"], (what, ml)
            got = fa.host_seqs()
            if got != o["seqs"]:
                bad = [q for q, (a, b) in enumerate(zip(got, o["seqs"])) if a != b]
                raise AssertionError(f"{what}, min_len {ml}: {len(got)} records against {len(o['seqs'])}, "
                                     f"differing records {bad[:8]}")
        finally:
            fa.close()
        out.append(o)
    return out


def _check_case(D, ctx, oracle, c, min_lens=None):
    res = _check(D, ctx, oracle, c.text, (0, c.min_len) if min_lens is None else min_lens, c.id)
    assert (res[0] is None) == (c.error is not None), c.id   # (the books agree on whether it is an error)


@pytest.mark.parametrize("o", F.O)
@pytest.mark.parametrize("event", F.LINE_EVENTS)
def test_line_start_seams(D, ctx, oracle, event, o):
    _check_case(D, ctx, oracle, F.place(event, o))


@pytest.mark.parametrize("o", F.O)
def test_crlf_seams(D, ctx, oracle, o):
    for event in F.CR_EVENTS:
        c = F.place_cr(event, o)
        _check_case(D, ctx, oracle, c)
        if event == "crlf_desc":   # (what the comparison with the oracle already says, spelled out)
            fa = D.parse_fasta(ctx, c.text)
            assert "abc" in fa.names and not any("\r" in n for n in fa.names)
            fa.close()


@pytest.mark.parametrize("n", F.EOF_N)
def test_eof_seams(D, ctx, oracle, n):
    for event in F.EOF_EVENTS:
        _check_case(D, ctx, oracle, F.place_eof(event, n))


def test_long_lines(D, ctx, oracle):
    for c in F.long_line_cases():
        _check_case(D, ctx, oracle, c)
        if c.tags["kind"] in ("desc", "desc_nul"):
            fa = D.parse_fasta(ctx, c.text)
            want = c.tags["length"] - (1 if c.tags["kind"] == "desc" else 4)
            assert max(map(len, fa.names)) == want, c.id
            fa.close()


def test_dense_records(D, ctx, oracle):
    for c in F.dense_cases():
        _check_case(D, ctx, oracle, c, (0, 1, 2))


@pytest.mark.parametrize("order", sorted(F.SELECT_ORDERS))
def test_select_seams(D, ctx, oracle, order):
    _check_case(D, ctx, oracle, F.select_case(order), (0,) + F.SELECT_MIN_LEN)


def test_error_precedence(D, ctx, oracle):
    for c in F.error_cases():
        _check_case(D, ctx, oracle, c)


@pytest.mark.parametrize("residue", F.PAD_RESIDUES)
def test_padding_is_scannable(D, ctx, oracle, residue):
    import ctypes as C

    import torch
    from kmer_spans_amd import _lib
    c = F.padding_case(residue)
    k = 3
    for ml in (0, c.min_len):
        o = oracle.fasta_parse(c.text, ml)
        assert sum(map(len, o["seqs"])) % 32 == residue
        fa = D.parse_fasta(ctx, c.text, ml)
        try:
            assert fa.host_seqs() == o["seqs"]
            # every consumer masks what it loads beyond the last base, so counting alone cannot
            # tell what the pad holds: read the 32 bytes themselves (inside the allocation,
            # ks_internal.h: "total + 32 bytes, 'N' padded"), through the library's own HIP runtime
            pad = C.create_string_buffer(32)
            hip_memcpy = _lib.load().hipMemcpy
            hip_memcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            hip_memcpy.restype = C.c_int
            assert hip_memcpy(pad, C.c_void_p(fa.struct().seq + fa.total), 32, 2) == 0   # device to host
            assert pad.raw == b"N" * 32, (residue, ml, pad.raw)
            counts = torch.zeros(4 ** k, dtype=torch.int32, device="cuda")
            words = D.count(ctx, fa, k, counts)
            n, oc = oracle.kmer_counts(o["seqs"], k)
            assert words == n, (residue, ml)
            assert np.array_equal(counts.cpu().numpy(), oc), (residue, ml)
        finally:
            fa.close()


def test_upload_ring(D, ctx, oracle, tmp_path):
    """2 x 64 MiB + 5 MiB: three staging pieces, the third through the first pinned half again."""
    text, names, digests = F.ring_text()
    o = oracle.fasta_parse(text)
    want = [(len(s), hashlib.sha256(s).hexdigest()) for s in o["seqs"]]
    assert o["names"] == names and want == digests
    p = tmp_path / "ring.fa"
    p.write_bytes(text)
    fa = D.load_fasta(ctx, str(p))
    try:
        assert fa.names == o["names"]
        assert fa.n_records == o["n_records"] and fa.bases_all == o["bases_all"] == fa.bases_kept
        assert [(len(s), hashlib.sha256(s).hexdigest()) for s in fa.host_seqs()] == want
    finally:
        fa.close()


def test_gzip_growth(D, ctx, oracle, tmp_path):
    def load(name, data, ml=0):
        p = tmp_path / name
        p.write_bytes(data)
        fa = D.load_fasta(ctx, str(p), ml)
        try:
            return {"names": fa.names, "seqs": fa.host_seqs(), "n_records": fa.n_records, "bases_all": fa.bases_all}
        finally:
            fa.close()

    z = gzip.compress(F.GZIP_TEXT)
    assert len(F.GZIP_TEXT) > 4 * len(z)
    o = oracle.fasta_parse(F.GZIP_TEXT)
    assert load("big.fa", F.GZIP_TEXT) == o
    assert load("big.fa.gz", z) == o
    none = oracle.fasta_parse(F.GZIP_TEXT, 10 ** 7)
    assert none["seqs"] == [] and load("big.fa.gz", z, 10 ** 7) == none
    empty = oracle.fasta_parse(b"")
    assert empty["n_records"] == 0
    assert load("empty.fa", b"") == empty
    assert load("empty.fa.gz", gzip.compress(b"")) == empty
    assert load("gt.fa", b">") == oracle.fasta_parse(b">") and oracle.fasta_parse(b">")["names"] == [""]
