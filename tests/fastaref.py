"""Builders of FASTA byte strings with an event at an exact absolute offset,
for the device FASTA reader (csrc/ks_ingest.hip, driven by csrc/ks_io.cpp).

The reader works on tiles of T = 4096 bytes, 256 lanes of L = 16 bytes each,
four waves of W = 1024 bytes; a lane reads a 17th byte for the "\\r\\n" rule,
the last line break before a tile is carried across tiles, and the record
selection (min_len) gathers in blocks of 4096 output bytes.  Every builder
here puts a byte of interest at a stated offset against that geometry.

A text is written through Doc, which keeps its own books while it appends
lines: the records (name, upper-cased bases) and the first error a
sequential reader meets.  The rules are those of DESIGN.md section 6b, stated
here from the document and not from the kernels:

  * a line ends at "\\n"; one "\\r" before it, or before the end of the file,
    is dropped; a line that is empty after that is skipped;
  * a line starting with ">" opens a record, the rest of the line is its
    name; a line starting with ";" is a comment;
  * every other line is sequence: IUPAC DNA letters of either case and
    "-", "+", "." are kept upper-cased; the first byte that is anything else
    is an error, and so is the first sequence byte met before any record.

Names travel as C strings (ks_fasta.names, the oracle's orc_fasta.names): a
name ends at its first 0x00 byte, and the books say so.

tests/test_fastaref.py pins these books to the C oracle and asserts that
every case holds what it is built for.  Plain module: no fixtures, no device.
"""
import hashlib
import zlib
from dataclasses import dataclass, field

import numpy as np

T = 4096   # bytes per tile
L = 16     # bytes per lane
W = 1024   # bytes per wave

# the offsets every seam family is swept over
O = (15, 16, 17, W - 1, W, W + 1, T - 17, T - 16, T - 15, T - 2, T - 1, T, T + 1, T + 15, T + 16,
     2 * T - 1, 2 * T, 3 * T)
EOF_N = (1, 2, 15, 16, 17, T - 1, T, T + 1, 2 * T, 2 * T + 1)

ALPHABET = b"ACGTMRWSYKVHDBNacgtmrwsykvhdbn-+."
VALID = frozenset(ALPHABET)
_ALPHA = np.frombuffer(ALPHABET, dtype=np.uint8)


@dataclass
class Case:
    id: str
    text: bytes
    names: list            # every record's name (str, latin-1), in file order
    seqs: list             # every record's bases (bytes, upper-cased)
    error: tuple = None    # (kind, pos): kind "invalid" or "before"; the records are void then
    min_len: int = 8       # the non-zero min_len the GPU test also runs
    marks: dict = field(default_factory=dict)   # what was planted -> absolute offset
    tags: dict = field(default_factory=dict)

    def expected(self, min_len=0):
        """What a parse with min_len returns (as oracle.fasta_parse's dict)."""
        assert self.error is None
        keep = [q for q, s in enumerate(self.seqs) if len(s) >= min_len]
        return {"names": [self.names[q] for q in keep], "seqs": [self.seqs[q] for q in keep],
                "n_records": len(self.seqs), "bases_all": sum(map(len, self.seqs))}

    def kept_starts(self, min_len):
        """Output offset of every kept record after the selection."""
        lens = [len(s) for s in self.seqs if len(s) >= min_len]
        return [int(x) for x in np.cumsum([0] + lens[:-1])] if lens else []


class Doc:
    """A FASTA text under construction, with its own books."""

    def __init__(self, key):
        self.buf = bytearray()
        self.recs = []      # [name bytes, bytearray of bases]
        self.error = None
        self.marks = {}
        self.key = key
        self.rng = np.random.default_rng(zlib.crc32(key.encode()))

    @property
    def n(self):
        return len(self.buf)

    def _bol(self):
        assert not self.buf or self.buf.endswith(b"\n"), "not at the start of a line"

    def mark(self, name, off=None):
        self.marks[name] = self.n if off is None else off

    def bases(self, m):
        """m random valid bytes: mixed case, all IUPAC letters and - + ."""
        return _ALPHA[self.rng.integers(0, _ALPHA.size, size=m)].tobytes()

    def desc(self, name=b"", eol=b"\n"):
        self._bol()
        assert b"\n" not in name and not name.endswith(b"\r") and eol in (b"\n", b"\r\n", b"\r", b"")
        self.buf += b">" + name + eol
        self.recs.append([name.split(b"\0")[0], bytearray()])

    def comment(self, body=b"", eol=b"\n"):
        self._bol()
        assert b"\n" not in body and not body.endswith(b"\r")
        self.buf += b";" + body + eol

    def blank(self, eol=b"\n"):
        self._bol()
        assert eol in (b"\n", b"\r\n", b"\r")
        self.buf += eol

    def seq(self, s, eol=b"\n"):
        """A sequence line: s may hold invalid bytes (the books note the first error)."""
        self._bol()
        assert s and s[0] not in b">;" and b"\n" not in s and not s.endswith(b"\r")
        pos = self.n
        self.buf += s + eol
        if self.error is None:
            if not self.recs:
                self.error = ("before", pos)
            else:
                bad = [i for i, c in enumerate(s) if c not in VALID]
                if bad:
                    self.error = ("invalid", pos + bad[0])
                else:
                    self.recs[-1][1] += s.upper()

    def fill_to(self, target, width=60):
        """Valid sequence lines (and, for a last odd byte, one empty line) up to offset target."""
        self._bol()
        assert self.recs and target >= self.n, (self.key, self.n, target)
        while self.n < target:
            r = target - self.n
            if r == 1:
                self.blank()
            else:
                self.seq(self.bases(min(r, width + 1) - 1))
        assert self.n == target

    def case(self, min_len=8, **tags):
        return Case(self.key, bytes(self.buf), [r[0].decode("latin-1") for r in self.recs],
                    [bytes(r[1]) for r in self.recs], self.error, min_len, dict(self.marks), tags)


def _start(key, offset, room=3):
    """A Doc opened with ">f\\n" and filled with sequence lines up to offset."""
    d = Doc(key)
    assert offset >= room
    d.desc(b"f")
    d.fill_to(offset)
    return d


def _tail(d):
    """More sequence, a short record (dropped at min_len 8) and a longer one."""
    d.seq(d.bases(23))
    d.desc(b"t1 short")
    d.seq(d.bases(5))
    d.desc(b"t2")
    d.seq(d.bases(40))


# ------------------------------------------------------------------ line starts

LINE_EVENTS = ("desc", "comment", "seq", "empty", "crlf_only")


def place(event, offset):
    """A text in which the first byte of the event's line is at offset."""
    d = _start(f"line-{event}-{offset}", offset)
    d.mark("line", offset)
    if event == "desc":
        d.desc(b"at the seam")
        d.seq(d.bases(33))
    elif event == "comment":
        d.comment(b" >not a record")
    elif event == "seq":
        d.seq(d.bases(37))
    elif event == "empty":
        d.blank()
    elif event == "crlf_only":
        d.blank(b"\r\n")
    else:
        raise ValueError(event)
    _tail(d)
    return d.case(event=event, offset=offset)


def line_start_cases():
    return [place(e, o) for e in LINE_EVENTS for o in O]


# ------------------------------------------------------------------------ CR/LF

CR_EVENTS = ("crlf_seq", "crlf_desc", "cr_eof_seq", "cr_eof_desc", "cr_lone")


def place_cr(event, offset):
    """A text whose "\\r" of interest is at offset."""
    key = f"{event}-{offset}"
    if event == "crlf_seq":
        d = _start(key, offset - 5)
        d.seq(d.bases(5), b"\r\n")
        _tail(d)
    elif event == "crlf_desc":
        d = _start(key, offset - 4)
        d.desc(b"abc", b"\r\n")
        _tail(d)
    elif event == "cr_eof_seq":
        d = _start(key, offset - 5)
        d.seq(d.bases(5), b"\r")
    elif event == "cr_eof_desc":
        d = _start(key, offset - 4)
        d.desc(b"abc", b"\r")
    elif event == "cr_lone":
        d = _start(key, offset - 5)
        d.seq(d.bases(5) + b"\r" + d.bases(3))
        _tail(d)
    else:
        raise ValueError(event)
    d.mark("cr", offset)
    return d.case(event=event, offset=offset)


def crlf_cases():
    return [place_cr(e, o) for e in CR_EVENTS for o in O]


# -------------------------------------------------------------------------- EOF

EOF_EVENTS = ("eof_base", "eof_nl", "eof_desc", "eof_gt")


def place_eof(event, n):
    """A text of exactly n bytes that ends as the event says."""
    key = f"{event}-{n}"
    d = Doc(key)
    if n >= 15:
        d.desc(b"f")
    if event == "eof_base":
        if n < 15:
            d.seq(d.bases(n), b"")          # no room for a description: the reader must refuse it
        else:
            d.fill_to(n - 3)
            d.seq(d.bases(3), b"")
    elif event == "eof_nl":
        if n == 1:
            d.blank()
        elif n == 2:
            d.desc(b"")
        else:
            d.fill_to(n)
    elif event == "eof_desc":
        if n < 15:
            d.desc(b"x" * (n - 1), b"")
        else:
            d.fill_to(n - 3)
            d.desc(b"zz", b"")
    elif event == "eof_gt":
        if n == 2:
            d.blank()
        elif n >= 15:
            d.fill_to(n - 1)
        d.desc(b"", b"")
    else:
        raise ValueError(event)
    assert d.n == n
    return d.case(event=event, n=n)


def eof_cases():
    return [place_eof(e, n) for e in EOF_EVENTS for n in EOF_N]


# ------------------------------------------------------------------- long lines

LONG_LENS = (T - 1, T, 2 * T + 5, 3 * T + 1)
LONG_STARTS = (T - 5, T, 5)
_SPECIALS = (b">", b";", b"\r", b"*", b"\xff")


def _long_body(d, start, length, nul):
    """length - 1 bytes to follow a line's first byte at offset start: letters and blanks, with
    > ; CR * 0xff at the first bytes of every tile and lane seam the line covers and in mid-line,
    and (nul) a 0x00 three bytes before the end."""
    body = bytearray(np.frombuffer(b"abcXYZ  >;*", dtype=np.uint8)[d.rng.integers(0, 11, size=length - 1)].tobytes())
    for i in range(1, length - 3):
        p = start + i            # absolute offset of body[i - 1]
        if p % T < len(_SPECIALS):
            body[i - 1:i] = _SPECIALS[p % T]
        elif p % T in (L, L + 1, W, W + 1) or i in (7, 8, 9, 10, 11):
            body[i - 1:i] = _SPECIALS[(p + i) % len(_SPECIALS)]
    body[-2:] = b"zz"
    if nul:
        body[-3:-2] = b"\0"
    return bytes(body)


def place_long(kind, length, start):
    """One line of length bytes (its line break not counted) whose first byte is at start."""
    key = f"long-{kind}-{length}-{start}"
    d = Doc(key)
    d.desc(b"f")
    d.seq(b"a")
    d.fill_to(start)
    d.mark("line", start)
    if kind in ("desc", "desc_nul"):
        d.desc(_long_body(d, start, length, kind == "desc_nul"))
        d.seq(d.bases(19))
    elif kind == "comment":
        d.comment(_long_body(d, start, length, True))
    elif kind == "seq":
        d.seq(d.bases(length))
    else:
        raise ValueError(kind)
    _tail(d)
    return d.case(kind=kind, length=length, start=start)


def long_line_cases():
    out = [place_long(k, n, s) for k in ("desc", "desc_nul", "comment") for n in LONG_LENS for s in LONG_STARTS]
    return out + [place_long("seq", 3 * T + 1, s) for s in LONG_STARTS]


# ---------------------------------------------------------------- dense records

def dense_cases():
    out = []
    d = Doc("dense-empty-records")
    for _ in range(5000):
        d.desc(b"")
    out.append(d.case())
    d = Doc("dense-one-base")
    for _ in range(3000):
        d.desc(b"x")
        d.seq(b"A")
    out.append(d.case())
    d = _start("dense-newline-tile", T)
    for _ in range(T):
        d.blank()
    d.mark("newlines", T)
    _tail(d)
    out.append(d.case())
    # tile 0 and 1: description lines only (no byte kept); tiles 2, 3: sequence only (no record);
    # tile 4: one comment; tile 5: blank lines and CR LF; then records of 0, 1 and 2 bases
    d = Doc("dense-mix")
    for i in range(T):
        d.desc(b"")
    d.fill_to(4 * T)
    d.comment(b"c" * (T - 2))
    for i in range(T // 4):
        d.blank()
        d.blank(b"\r\n")
        d.blank()
    assert d.n == 6 * T
    for i in range(700):
        d.desc(b"r%d" % i)
        if i % 3:
            d.seq(d.bases(i % 3))
    out.append(d.case())
    return out


def lanes_with_two_descriptions(text):
    """How many 16-byte lanes hold the first byte of two or more description lines."""
    a = np.frombuffer(text, dtype=np.uint8)
    gt = np.flatnonzero(a == ord(">"))
    gt = gt[(gt == 0) | (a[np.maximum(gt, 1) - 1] == ord("\n"))]
    return int((np.bincount(gt // L) >= 2).sum())


# -------------------------------------------------------------------- selection

SELECT_LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 4095, 4096, 4097)
SELECT_MIN_LEN = (1, 16, 17, 4096, 4097, 10 ** 9)
SELECT_ORDERS = {
    # min_len 1: the first and the last record go; kept records start at 4095 and 4096
    "a": (0, 4095, 1, 15, 16, 17, 31, 32, 33, 4096, 4097, 0),
    # min_len 4096: 4097 and 4096 stay, the second starts at 4097; min_len 4097: one record stays
    "b": (17, 4097, 16, 0, 1, 15, 31, 32, 33, 4095, 4096),
    # min_len 17: the last record goes, the second kept record starts at 4096
    "c": (4096, 0, 33, 4097, 32, 1, 4095, 31, 15, 17, 16),
}


def select_case(order):
    d = Doc(f"select-{order}")
    for i, n in enumerate(SELECT_ORDERS[order]):
        d.desc(b"rec%d len %d" % (i, n))
        width = (70, 4096, 17)[i % 3]
        s = d.bases(n)
        for j in range(0, n, width):
            d.seq(s[j:j + width])
    return d.case(order=order)


def select_cases():
    return [select_case(o) for o in SELECT_ORDERS]


# ------------------------------------------------------------- error precedence

def error_cases():
    out = []
    for i, text in enumerate((b"AC\n>a\nAZ\n", b"Z\n>a\nAC\n")):
        d = Doc(f"err-before-small-{i}")
        for line in text.split(b"\n")[:-1]:
            d.desc(line[1:]) if line[:1] == b">" else d.seq(line)
        assert bytes(d.buf) == text
        out.append(d.case())

    def bad_in_tiles(key, tiles, bad=b"*"):
        d = Doc(key)
        d.desc(b"f")
        for t in tiles:
            d.fill_to(t * T + 100 + 7 * (t % 5))
            d.seq(d.bases(9) + bad + d.bases(4))
        d.fill_to((max(tiles) + 2) * T)
        return d.case(tiles=tuple(tiles))

    out.append(bad_in_tiles("err-tiles-0-5", (0, 5)))
    out.append(bad_in_tiles("err-tiles-5-9", (5, 9)))
    out.append(bad_in_tiles("err-every-tile-40", tuple(range(40))))
    out.append(bad_in_tiles("err-0x80", (1, 2), b"\x80"))
    out.append(bad_in_tiles("err-0x00", (1, 2), b"\0"))
    # sequence before the first description line, which sits three tiles on
    d = Doc("err-before-late-desc")
    d.comment(b"c")
    d.blank()
    d.seq(d.bases(50))
    d.recs.append([b"", bytearray()])   # (filler only; the books are void after the error)
    d.fill_to(3 * T + 5)
    d.recs.clear()
    d.desc(b"late")
    d.seq(d.bases(20))
    out.append(d.case())
    # the same with an invalid byte after it: the earlier condition is still the one reported
    d = Doc("err-before-then-invalid")
    d.blank()
    d.seq(b"ACGT")
    d.seq(b"AC*T")
    d.recs.append([b"", bytearray()])
    d.fill_to(2 * T + 1)
    d.recs.clear()
    d.desc(b"late")
    d.seq(b"AZ")
    out.append(d.case())
    # an invalid byte as the very first kept byte, no description anywhere
    d = Doc("err-before-no-desc")
    d.seq(b"*")
    out.append(d.case())
    # comments, empty and CR LF lines before the first description line: no error
    d = Doc("err-none-comment-first")
    d.comment(b"AC*Z not sequence")
    d.blank()
    d.blank(b"\r\n")
    d.comment(b"x" * (T + 3))
    d.blank()
    d.desc(b"first")
    d.seq(d.bases(30))
    _tail(d)
    out.append(d.case())
    return out


# ---------------------------------------------------------------------- padding

PAD_RESIDUES = (0, 15, 16)


def padding_case(residue):
    """Kept bytes total = residue (mod 32) before and after the selection at min_len 33 (the one
    record it drops has 32 bases); the last record ends in a run of A, so bytes read as bases
    after the end would be counted."""
    d = Doc(f"pad-{residue}")
    d.desc(b"drop me")
    d.seq(d.bases(32))
    d.desc(b"a")
    d.fill_to(T + 7)
    d.desc(b"b")
    d.seq(d.bases(64))
    have = sum(len(r[1]) for r in d.recs)
    d.seq(b"ACGT" + b"A" * ((residue - have - 4) % 32 + 32))
    c = d.case(min_len=33, residue=residue)
    assert c.expected()["bases_all"] % 32 == residue
    return c


def padding_cases():
    return [padding_case(r) for r in PAD_RESIDUES]


# ------------------------------------------------------------------ upload ring

RING_PIECE = 64 << 20
RING_BYTES = 2 * RING_PIECE + (5 << 20)


def ring_text(total=RING_BYTES, every=(8 << 20) + 300_000):
    """total bytes of 70-column random ACGT lines with a description line about every `every`
    bytes.  Returns (text, names, [(length, sha256 hex)] per record)."""
    rng = np.random.default_rng(20)
    parts, names, digests = [], [], []
    left, i = total, 0
    while left > 0:
        head = b">piece %d of the ring\n" % i
        room = left - len(head)
        last = room < every + 200                 # the last record takes what is left
        nlines = (room if last else every) // 71
        lines = np.empty((nlines, 71), dtype=np.uint8)
        lines[:, :70] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(nlines, 70), dtype=np.uint8)]
        lines[:, 70] = ord("\n")
        body = lines.tobytes()
        seq = lines[:, :70].tobytes()
        if last:                                  # a partial line, no final line break
            extra = b"G" * (room - len(body))
            body += extra
            seq += extra
        parts += [head, body]
        names.append(head[1:-1].decode())
        digests.append((len(seq), hashlib.sha256(seq).hexdigest()))
        left -= len(head) + len(body)
        i += 1
    text = b"".join(parts)
    assert len(text) == total
    return text, names, digests


# ------------------------------------------------------------------------- gzip

GZIP_TEXT = b">a\n" + b"ACGT" * 750_000
