"""Independent references and corpus builders for the two integer-histogram
kernel families: k-mer counting (csrc/ks_count.hip) and windowed count
distributions (csrc/ks_windowed.hip).

The references are vectorised numpy restatements of the rules in
include/kmer_spans.h, written from the header's wording and not from the
kernels:

  * bytes N/n split runs; every other byte is coded (c >> 1) & 3
    (A=0, C=1, T=2, G=3), the first base most significant;
  * a k-mer is counted at its last base, once, when its k bases lie in one
    N-free run of one sequence;
  * Q1 (counting only): the first window of a run is dropped when it ends
    exactly at the end of the string;
  * windowed: in every N-free run of a sequence longer than `window`, every
    window [s, s + window) inside the run holds the k-mers ending at
    s + k - 1 .. s + window - 1; no end-of-run quirk applies.

tests/test_histref.py pins them to the C oracle and to the brute-force
restatement of tests/test_windowed.py, and asserts that the corpora built
here exercise what they are built for.  Every builder takes a seed and
returns the sequences together with the list of what it planted where, so a
failing assert can name the offset.

Plain module: no fixtures, no device.
"""
import numpy as np

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_N = ord("N")


def _bytes(s) -> bytes:
    return s.encode("latin-1") if isinstance(s, str) else bytes(s)


def _as_list(seqs):
    return [seqs] if isinstance(seqs, (str, bytes, bytearray)) else list(seqs)


def encode(kmer) -> int:
    """The 2-bit code of an N-free k-mer, first base most significant."""
    c = 0
    for b in _bytes(kmer):
        c = (c << 2) | ((b >> 1) & 3)
    return c


def decode(code: int, k: int) -> str:
    return "".join("ACTG"[(int(code) >> (2 * (k - 1 - j))) & 3] for j in range(k))


def _concat(seqs):
    bs = [_bytes(s) for s in _as_list(seqs)]
    offs = np.zeros(len(bs) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(b) for b in bs])
    return np.frombuffer(b"".join(bs), dtype=np.uint8), offs


def _run_len(buf, offs):
    """Per position: the number of consecutive non-N bytes of its own
    sequence that end there (0 at an N)."""
    n = buf.size
    pos = np.arange(n, dtype=np.int64)
    isn = (buf | 0x20) == ord("n")
    brk = np.where(isn, pos, -1)          # an N breaks the run at itself
    starts = offs[:-1][offs[:-1] < n]
    brk[starts] = np.maximum(brk[starts], starts - 1)  # a sequence start breaks it just before
    return pos - np.maximum.accumulate(brk)


def _kmer_codes(buf, k):
    """Per position p >= k - 1: the code of bytes p - k + 1 .. p (whatever they are)."""
    n = buf.size
    code = np.zeros(n, dtype=np.uint32)
    if n < k:
        return code
    enc = ((buf >> 1) & 3).astype(np.uint32)
    for j in range(k):
        code[k - 1:] |= enc[k - 1 - j:n - j] << np.uint32(2 * j)
    return code


def counted_codes(seqs, k: int) -> np.ndarray:
    """The code of every counted k-mer, in order of its last base.  The dense
    histogram is np.bincount(codes, minlength=4**k), the word total len(codes)."""
    buf, offs = _concat(seqs)
    if buf.size < k:
        return np.zeros(0, dtype=np.uint32)
    rl = _run_len(buf, offs)
    last = np.zeros(buf.size, dtype=bool)  # last byte of a (non-empty) sequence
    ends = offs[1:][offs[1:] > 0]
    last[ends - 1] = True
    keep = (rl >= k) & ~((rl == k) & last)  # Q1
    return _kmer_codes(buf, k)[keep]


def count_hist(seqs, k: int) -> np.ndarray:
    return np.bincount(counted_codes(seqs, k), minlength=4 ** k)


def windowed_ref(seqs, codes, k: int, window: int):
    """(dist int64 [(window + 1), nq], scores: per sequence int64 [len, nq]
    or None where the sequence is not longer than the window)."""
    codes = np.asarray(codes, dtype=np.uint32).ravel()
    nq = codes.size
    dist = np.zeros((window + 1, nq), dtype=np.int64)
    scores = []
    for s in _as_list(seqs):
        buf = np.frombuffer(_bytes(s), dtype=np.uint8)
        L = buf.size
        if L <= window:
            scores.append(None)
            continue
        sc = np.zeros((L, nq), dtype=np.int64)
        scores.append(sc)
        rl = _run_len(buf, np.array([0, L], dtype=np.int64))
        # s starts a window iff the N-free run ending at s + window - 1 reaches back to s
        starts = np.flatnonzero(rl[window - 1:] >= window)
        if starts.size == 0:
            continue
        kc = _kmer_codes(buf, k)
        valid = rl >= k
        for i in range(nq):
            cs = np.zeros(L + 1, dtype=np.int64)  # cs[p + 1]: hits ending at 0 .. p
            cs[1:] = np.cumsum(valid & (kc == codes[i]))
            c = cs[starts + window] - cs[starts + k - 1]
            dist[:, i] += np.bincount(c, minlength=window + 1)
            sc[starts, i] = c
    return dist, scores


def window_starts_per_run(seqs, window: int):
    """Window-start counts W = run - window + 1 of every N-free run that holds
    a window, over the sequences longer than the window."""
    out = []
    for s in _as_list(seqs):
        buf = np.frombuffer(_bytes(s), dtype=np.uint8)
        if buf.size <= window:
            continue
        rl = _run_len(buf, np.array([0, buf.size], dtype=np.int64))
        run_end = np.flatnonzero((rl > 0) & np.append(rl[1:] == 0, True))
        out += [int(rl[e]) - window + 1 for e in run_end if rl[e] >= window]
    return out


# --------------------------------------------------------------- count corpora

EVENTS = ("seq", "n", "q1", "k1", "empty")


def _random_bases(rng, n):
    return _ACGT[rng.integers(0, 4, size=n)].copy()


def _plant(buf, cuts, kind, P, k):
    """One event anchored at buffer position P (0 < P <= len(buf)):
    seq    a sequence ends at P (the next one starts there);
    n      a single N at P (at P - 1 when P is the end of the buffer);
    q1     N, exactly k bases, end of sequence at P (counts nothing);
    k1     N, exactly k + 1 bases, end of sequence at P (counts two);
    empty  a sequence ends at P, an empty one follows.
    At the end of the buffer the sequence end is the buffer's own."""
    at_end = P == buf.size
    if kind == "n":
        buf[P - 1 if at_end else P] = _N
        return
    if kind == "q1":
        buf[P - k - 1] = _N
    elif kind == "k1":
        buf[P - k - 2] = _N
    if kind == "empty":
        cuts.append(P)
    if not at_end:
        cuts.append(P)


def _split(buf, cuts, planted):
    """Cut the buffer into sequences; fills in the index of the sequence that
    ends at each planted event."""
    bounds = [0] + sorted(cuts) + [buf.size]
    seqs = [buf[a:b].tobytes() for a, b in zip(bounds[:-1], bounds[1:])]
    ends = {}
    for j, b in enumerate(bounds[1:]):
        ends.setdefault(b, j)
    for p in planted:
        if p["kind"] != "n":
            p["seq"] = ends[p["pos"]]
    return seqs


def seam_corpus(seed: int, k: int, tile: int, rot: int = 0, reps: int = 1):
    """Random ACGT over 35 * reps tiles and a ragged half tile.  Tile boundary
    number i (at i * tile) gets one event at offset d = -17 .. +17; the event
    kinds cycle with the boundary number, shifted by rot, so rot = 0 .. 4 puts
    every kind at every offset; reps = 5 does the same within one corpus."""
    rng = np.random.default_rng([seed, k, tile, rot, reps])
    nt = 35 * reps
    buf = _random_bases(rng, nt * tile + tile // 2 + 7)
    cuts, planted = [], []
    for i in range(1, nt + 1):
        d = (i - 1) % 35 - 17
        kind = EVENTS[(i + (i - 1) // 35 + rot) % 5]
        P = i * tile + d
        _plant(buf, cuts, kind, P, k)
        planted.append({"kind": kind, "boundary": i * tile, "d": d, "pos": P})
    return _split(buf, cuts, planted), planted


def tail_corpus(seed: int, k: int, tile: int, kind: str, t: int):
    """Two tiles and a ragged piece of random ACGT with one event t positions
    before the end of the buffer (t = 0: at the end itself)."""
    rng = np.random.default_rng([seed, k, tile, EVENTS.index(kind), t])
    buf = _random_bases(rng, 2 * tile + 100 + int(rng.integers(0, 16)))
    cuts = [tile // 2 + 3]
    P = buf.size - t
    planted = [{"kind": kind, "boundary": int(buf.size), "d": -t, "pos": P}]
    _plant(buf, cuts, kind, P, k)
    return _split(buf, cuts, planted), planted


def many_seqs_corpus(seed: int, k: int, nseq: int = 6000, tail: int = 40_000):
    """nseq sequences of 0 .. 40 bases, many of them empty or k - 1, k and
    k + 1 long, some with an N, then one long sequence: more offsets than the
    counting kernels' 64-ary start search narrows in one step."""
    rng = np.random.default_rng([seed, k, nseq])
    special = np.array([0, 0, k - 1, k, k + 1])
    lens = np.where(rng.random(nseq) < 0.6, special[rng.integers(0, special.size, nseq)],
                    rng.integers(0, 41, nseq))
    seqs, planted = [], []
    for j, L in enumerate(lens):
        b = _random_bases(rng, int(L))
        if L > 2 and rng.random() < 0.1:
            p = int(rng.integers(0, L))
            b[p] = _N
            planted.append({"kind": "n", "seq": j, "pos": p})
        seqs.append(b.tobytes())
    seqs.append(_random_bases(rng, tail).tobytes())
    return seqs, planted


def geometry_corpus(seed: int, total: int):
    """`total` random bases in sequences of about 50 kbases with an N about
    every 20 kbases: content for the block-geometry cases, whose point is the
    tile count."""
    rng = np.random.default_rng([seed, total])
    buf = _random_bases(rng, total)
    cuts = sorted(set(int(x) for x in rng.integers(1, total, size=total // 50_000))) if total > 1 else []
    ns = rng.integers(0, total, size=total // 20_000)
    buf[ns] = _N
    planted = [{"kind": "seq", "pos": c} for c in cuts] + [{"kind": "n", "pos": int(p)} for p in ns]
    bounds = [0] + cuts + [total]
    return [buf[a:b].tobytes() for a, b in zip(bounds[:-1], bounds[1:])], planted


def tiny_cases(k: int, seed: int = 0):
    """(name, sequences, counts nothing) for the tiny inputs: around k bases,
    and around the 32 bases below which the partitioned counter leaves its
    staged scatter.  The two short lists stay under 32 bases for every k."""
    rng = np.random.default_rng([seed, k, 77])

    def rnd(n):
        return _random_bases(rng, n).tobytes().decode()

    def split3(n):  # three random strings of n bases in all, the first longer than k
        a = min(n - 2, max(k + 1, n // 2))
        b = (n - a) // 2
        return [rnd(a), rnd(b), rnd(n - a - b)]

    return [
        ("k-1", ["A" * (k - 1)], True),
        ("q1", ["A" * k], True),
        ("k+1", [rnd(k + 1)], False),
        ("total31", split3(31), False),
        ("total32", split3(32), False),
        ("total33", split3(33), False),
        ("short-list", [rnd(3), rnd(k + 1), "", rnd(2), rnd(min(k, 5))], False),
        ("short-list-n", [rnd(1) + "n" + rnd(1), rnd(1) + "N" + rnd(k + 1), "", rnd(2), rnd(min(k, 5))], False),
        ("run-k-at-end", [rnd(k + 3) + "N" + rnd(k)], False),
    ]


# ------------------------------------------------------------ windowed corpora

def absent_kmer(k: int) -> str:
    """The k-mer that windowed_corpus removes from its sequences."""
    return ("CG" * 8)[:k]


def _remove_kmer(buf, k, rng):
    """Mutate bases until no k-mer of buf equals absent_kmer(k) (stretches of
    A and AT hold none, so they stay as planted)."""
    q = np.uint32(encode(absent_kmer(k)))
    others = np.frombuffer(b"AT", dtype=np.uint8)
    for _ in range(64):
        rl = _run_len(buf, np.array([0, buf.size], dtype=np.int64))
        hit = np.flatnonzero((_kmer_codes(buf, k) == q) & (rl >= k))  # (an N codes like G: N-free k-mers only)
        if hit.size == 0:
            return
        buf[hit] = others[rng.integers(0, 2, size=hit.size)]
    raise AssertionError("absent_kmer still present")


def windowed_corpus(seed: int, k: int, window: int, nq: int, layout):
    """layout: per sequence the list of its N-free run lengths (runs are
    separated by single Ns).  Random ACGT; the longest run gets a stretch of
    window + 5 A and, where it fits, one of AT just as long.  Queries: k-mers
    of the longest run at fixed strides; from five queries on the first four are
    A*k, a drawn k-mer, its duplicate, and a k-mer that never occurs.
    Returns (sequences, query strings, planted)."""
    rng = np.random.default_rng([seed, k, window, nq])
    seqs_b, planted = [], []
    longest = max(((r, si, ri) for si, runs in enumerate(layout) for ri, r in enumerate(runs)), default=(0, 0, 0))
    st = window + 5
    for si, runs in enumerate(layout):
        parts = []
        off = 0
        for ri, r in enumerate(runs):
            b = _random_bases(rng, r)
            if (r, si, ri) == longest:
                if r >= st + 6:
                    b[3:3 + st] = ord("A")
                    planted.append({"kind": "homopolymer", "seq": si, "pos": off + 3, "len": st})
                if r >= 2 * st + 20:
                    b[st + 10:2 * st + 10] = np.resize(np.frombuffer(b"AT", dtype=np.uint8), st)
                    planted.append({"kind": "dinucleotide", "seq": si, "pos": off + st + 10, "len": st})
            parts.append(b)
            off += r
            if ri + 1 < len(runs):
                parts.append(np.array([_N], dtype=np.uint8))
                planted.append({"kind": "n", "seq": si, "pos": off})
                off += 1
        seqs_b.append(np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8))
    for b in seqs_b:
        _remove_kmer(b, k, rng)
    # queries: k-mers at fixed strides over the longest run (it holds windows)
    r, si, ri = longest
    b = seqs_b[si]
    a = sum(layout[si][:ri]) + ri
    ok = np.arange(a + k - 1, a + r)
    kc = _kmer_codes(b, k)
    ndraw = nq if nq < 5 else nq - 3
    drawn = []
    for j in range(ndraw):
        p = ok[((2 * j + 1) * ok.size // (2 * ndraw) + ok.size // 2) % ok.size]  # the first from mid-run
        drawn.append(decode(kc[p], k))
    if nq < 5:
        kmers = drawn
    else:
        kmers = ["A" * k, drawn[0], drawn[0], absent_kmer(k)] + drawn[1:]
    return [b.tobytes() for b in seqs_b], kmers, planted


def inclusion_corpus(seed: int, k: int, window: int):
    """The inclusion rule of the windowed distributions, one sequence each:
    0  exactly `window` N-free bases: excluded (a run of `window` bases in a
       sequence that is not longer than the window);
    1  window + 1 N-free bases, the shortest included sequence: two windows;
    2  longer than the window, every run shorter: included, contributes nothing;
    3  as 0 in lower case, after included ones;
    4  empty;
    5  window - 1 bases and an N: `window` bytes, excluded;
    6  two runs of `window` bases: one window each;
    7  `window` bases and an N: window + 1 bytes, exactly one window."""
    rng = np.random.default_rng([seed, k, window, 99])

    def rnd(n):
        return _random_bases(rng, n)

    n = np.array([_N], dtype=np.uint8)
    bufs = [rnd(window), rnd(window + 1), np.concatenate([rnd(window - 1), n, rnd(window - 1), n, rnd(k)]),
            rnd(window) | 0x20, rnd(0), np.concatenate([rnd(window - 1), n]),
            np.concatenate([rnd(window), n, rnd(window)]), np.concatenate([rnd(window), n])]
    for b in bufs:
        _remove_kmer(b, k, rng)
    q = bufs[1]
    kmers = [decode(_kmer_codes(q, k)[k - 1 + j], k) for j in (0, window // 2)] + [absent_kmer(k)]
    kmers.append(decode(_kmer_codes(bufs[6] & 0xdf, k)[window - 1], k))
    included = [0, 1, 1, 0, 0, 0, 1, 1]
    return [b.tobytes() for b in bufs], kmers, included


# ------------------------------------------------------------- the case lists
# (shared by tests/test_histref.py, which checks the references and the
# inputs on the CPU, and the two GPU files, which run them)

SEAM_KS = (1, 7, 8, 10, 11, 12, 13, 14)
MANY_KS = (5, 9, 11, 14)
GEOMETRY_KS = (11, 13, 14)
ACCUM_KS = (7, 9, 12, 14)
PART_TILE = 16384  # positions per tile of the partitioned counter (k >= 11)
# tiles of the partitioned counter: N whole tiles and 5 bases (N + 1 tiles),
# and N tiles of which the last holds 5 bases, for the block counts 9, 17 and
# 63 whose last group of ceil(G / 8) blocks is short; one exact tile.
GEOMETRY_TOTALS = tuple(sorted([n * PART_TILE + 5 for n in (1, 2, 8, 9, 17, 63)] +
                               [(n - 1) * PART_TILE + 5 for n in (9, 17, 63)] + [PART_TILE]))
BIG_TOTAL = 519 * PART_TILE + 5  # 520 tiles: the 512 persistent blocks loop, 8 of them twice


def count_tile(k: int) -> int:
    """Positions per tile of the kernel that counts this k alone."""
    return 4096 if k <= 10 else PART_TILE


def window_R(window: int) -> int:
    """Window starts per lane of k_window (ks_windowed.hip: R = max(1024, 2 * window))."""
    return max(1024, 2 * window)


def windowed_cases():
    """name -> dict(seed, k, window, nq, layout, seams, maxbin)."""
    cases = {}

    def add(name, k, window, nq, layout, seams=False, maxbin=False):
        cases[name] = dict(seed=len(cases), k=k, window=window, nq=nq, layout=layout, seams=seams, maxbin=maxbin)

    for w in (1023, 1024, 1025):  # 16 * (window + 1) * 4 <= 65536 up to window 1023
        add(f"lds-w{w}", 3, w, 5, [[w + 2 * window_R(w) + 100, 700], [w + 1], [300, w + 50]], seams=True, maxbin=True)
    for w in (50, 1024):
        for nq in (1, 15, 16, 17, 32, 33):
            add(f"groups-w{w}-q{nq}", 4, w, nq, [[3000, 40], [w + 1], [60, w + 300]])
    for k in (9, 12, 13, 14, 15):
        for w in (2 * k, 2 * k + 1, 200):
            add(f"largek-k{k}-w{w}", k, w, 17, [[2500, 900], [w + 1], [w]])
    for w in (8, 100, 511):
        add(f"seams-w{w}", 4, w, 5, [[W + w - 1 for W in range(1020, 1031)], [W + w - 1 for W in range(2044, 2053)]],
            seams=True)
    add("seams-w600", 4, 600, 5, [[W + 599 for W in range(1195, 1206)]], seams=True)
    return cases


def build_windowed(case):
    return windowed_corpus(case["seed"], case["k"], case["window"], case["nq"], case["layout"])
