"""Planted trajectories for the chunked scan's seams (no GPU, no torch).

The chunked scan cuts every N-free run into chunks of CH scan indices, groups
64 chunks into a tile and takes 64 tiles per trip of its per-run wave loops
(a "step"); the carry and the stitch have code of their own for the first and
last index, lane and trip of each unit.  This module builds genomes whose
excursions begin, peak, tie, clamp or stay open exactly on those indices.

The score table depends on the LAST base of the k-mer only, w[code] =
v[code & 3] in the library's base order A, C, T, G, so the trajectory
S_i = max(fl(S_{i-1} + w), 0) is a function of single bytes for every k: in a
run [a, b) scan index i = a + k + j (j = 0 .. P - 1, P = b - a - k) scores
byte i - 1.  A run is therefore k - 1 bytes of lead-in, the P scored bytes
(the instance's "body", the same for every k) and one byte nothing scores.
T is the reset (a large negative value) and the fill between planted events.

An Instance is one run with one event placed against a seam size sigma (256,
16,384 or 1,048,576 relative indices); a Corpus joins instances by N gaps
into a few sequences, each behind a run of three chunks so that the long runs
start inside a global 64-chunk tile.  For the INT and DYADIC value sets every
planted excursion (beg, first argmax, maximum) is known from the plant, which
gives the regions without any scan (Corpus.predict); DRIFT (inexact sums) and
the random run-length instances have the oracle as their only reference.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

CHUNK = 256        # ks_scan_chunk_indices()
TILE_CHUNKS = 64   # ks_scan_tile_chunks()
WAVE = 64          # tiles per trip of the per-run wave loops

BASES = b"ACTG"  # the library's 2-bit base order: (byte >> 1) & 3
VALUES = {  # (A, C, T, G)
    "INT": (1.0, -1.0, -(2.0 ** 20), 2.0),
    "DYADIC": (1.0, -1.0, -1e6, 0.5),
    "DRIFT": (0.7, -0.6, -1e6, 0.35),
}
SEAMS = ("chunk", "tile", "step")
_A, _C, _T = (np.uint8(c) for c in b"ACT")
_PAD = 37  # fill after the last planted byte of an instance


def seam_size(seam: str, chunk: int = CHUNK, tile_chunks: int = TILE_CHUNKS) -> int:
    return {"chunk": chunk, "tile": chunk * tile_chunks, "step": chunk * tile_chunks * WAVE}[seam]


def table(vset: str, k: int) -> np.ndarray:
    """w[code] = v[last base of code], float64[4^k]."""
    return np.array(VALUES[vset], dtype=np.float64)[np.arange(4 ** k, dtype=np.int64) & 3]


def int_exact(w) -> bool:
    """The library's rule for the exact integer carry (ks_table::int_exact):
    every value a finite integer of magnitude <= 2^20."""
    w = np.asarray(w, dtype=np.float64)
    return bool(np.all(np.isfinite(w)) and np.all(w == np.rint(w)) and np.all(np.abs(w) <= 2.0 ** 20))


@dataclass
class Instance:
    name: str      # family/variant
    family: str
    body: np.ndarray                 # uint8[P]: the byte scored at relative index j
    exc: list | None                 # planted top-level excursions (beg, first argmax, max), relative; None: oracle only
    marks: dict = field(default_factory=dict)  # where the named features were put (relative indices)

    @property
    def P(self) -> int:
        return int(self.body.size)


def _fill(P: int) -> np.ndarray:
    return np.full(P, _T, dtype=np.uint8)


def _placed(name, family, P, at, text, exc, **marks) -> Instance:
    body = _fill(P)
    t = np.frombuffer(text, dtype=np.uint8) if isinstance(text, bytes) else text
    assert 0 <= at and at + t.size <= P, (name, at, t.size, P)
    body[at:at + t.size] = t
    return Instance(name, family, body, exc, dict(marks))


def _ac(n: int) -> np.ndarray:
    return np.tile(np.array([_A, _C], dtype=np.uint8), n)


def _cat(*parts) -> np.ndarray:
    return np.concatenate([np.frombuffer(p, dtype=np.uint8) if isinstance(p, bytes) else p for p in parts])


def _random(rng, P: int) -> np.ndarray:
    return np.frombuffer(BASES, dtype=np.uint8)[rng.integers(0, 4, size=P)]


def closed_in_place(S):
    """AAT, the first A on S - 1: begins before the seam, peaks on it."""
    return [_placed("closed-in-place", "closed-in-place", S + 2 + _PAD, S - 1, b"AAT", [(S - 1, S, 2.0)],
                    beg=S - 1, peak=S, clamp=S + 1)]


def tie_across(S):
    """AACAT from S - 3: maxima 2 at S - 2 and at S, the first one counts."""
    return [_placed("tie-across", "tie-across", S + 2 + _PAD, S - 3, b"AACAT", [(S - 3, S - 2, 2.0)],
                    beg=S - 3, peak=S - 2, tie=S, clamp=S + 1)]


def tied_span(S):
    """A + AC x n + T from j0 = S - 41 to beyond 2 S + 40: S runs 1, 2, 1, 2 ..."""
    j0 = S - 41
    n = (2 * S + 40 - j0 + 1) // 2 + 1
    end = j0 + 1 + 2 * n  # the T
    return [_placed("tied-span", "tied-span", end + 1 + _PAD, j0, _cat(b"A", _ac(n), b"T"), [(j0, j0 + 1, 2.0)],
                    beg=j0, peak=j0 + 1, clamp=end)]


def argmax_at_seam(S):
    """The carried excursion of tied_span, then A x r so that the last A, the
    only maximum, is the last index of a unit (2 S - 1) or the first of the
    next (2 S)."""
    out = []
    j0 = S - 41
    for tag, t in (("last", 2 * S - 1), ("first", 2 * S)):
        r = 3 if (t - 3 - j0) % 2 == 0 else 4
        n = (t - r - j0) // 2
        assert j0 + 2 * n + r == t
        out.append(_placed(f"argmax-at-seam/{tag}", "argmax-at-seam", t + 2 + _PAD, j0,
                           _cat(b"A", _ac(n), b"A" * r, b"T"), [(j0, t, 1.0 + r)], beg=j0, peak=t, clamp=t + 1))
    return out


def reset_at_seam(S):
    """AAAAA T AAA T with the first T (a clamp) on S, and on S - 1: the second
    excursion opens on the index right after the clamp."""
    out = []
    for tag, c in (("on", S), ("before", S - 1)):
        out.append(_placed(f"reset-at-seam/{tag}", "reset-at-seam", c + 5 + _PAD, c - 5, b"AAAAATAAAT",
                           [(c - 5, c - 1, 5.0), (c + 1, c + 3, 3.0)], clamp=c, beg2=c + 1))
    return out


def touch_zero(S):
    """AAACCC AAAA T: S reaches exactly 0 on the seam index without going
    negative; the twin AAACC AAAA T stays at 1 there (no clamp)."""
    return [_placed("touch-zero/clamp", "touch-zero", S + 6 + _PAD, S - 5, b"AAACCCAAAAT",
                    [(S - 5, S - 3, 3.0), (S + 1, S + 4, 4.0)], clamp=S, beg2=S + 1),
            _placed("touch-zero/twin", "touch-zero", S + 6 + _PAD, S - 4, b"AAACCAAAAT",
                    [(S - 4, S + 4, 5.0)], low=S, peak=S + 4)]


def open_at_end(S, ds=(-1, 0, 1)):
    """P = 2 S + d scored indices, the last 30 all A: open at the run's end."""
    out = []
    for d in ds:
        P = 2 * S + d
        out.append(_placed(f"open-at-end/{d:+d}", "open-at-end", P, P - 30, b"A" * 30, [(P - 30, P - 1, 30.0)],
                           beg=P - 30, peak=P - 1, last=P - 1))
    return out


def threshold_equality(S):
    """AAAAAA T from S - 3: width 5 and score 6 exactly."""
    return [_placed("threshold-equality", "threshold-equality", S + 4 + _PAD, S - 3, b"AAAAAAT",
                    [(S - 3, S + 2, 6.0)], beg=S - 3, peak=S + 2)]


def run_length(S, rng, ds):
    """Plain random runs of S + d scored indices."""
    return [Instance(f"run-length/{d:+d}", "run-length", _random(rng, S + d), None, {"last": S + d - 1}) for d in ds]


def drift_span(S):
    """AC x (S + 3000) + T from j = 1000: under DRIFT one excursion that
    climbs 0.1 per pair across more than a whole unit."""
    n = S + 3000
    return [_placed("drift-span", "drift-span", 1000 + 2 * n + 1 + _PAD, 1000, _cat(_ac(n), b"T"), None,
                    beg=1000, clamp=1000 + 2 * n)]


class Corpus:
    """The instances of one seam and value set, laid out as sequences."""

    def __init__(self, seam: str, vset: str, chunk: int = CHUNK, tile_chunks: int = TILE_CHUNKS):
        self.seam, self.vset, self.chunk = seam, vset, chunk
        self.sigma = S = seam_size(seam, chunk, tile_chunks)
        rng = np.random.default_rng(1000 * SEAMS.index(seam) + sorted(VALUES).index(vset))
        if seam == "step":
            inst = tied_span(S) + argmax_at_seam(S) + reset_at_seam(S) + touch_zero(S) + open_at_end(S) + \
                run_length(S, rng, (-1, 0, 1))
            nseq = 2
        else:
            inst = closed_in_place(S) + tie_across(S) + tied_span(S) + argmax_at_seam(S) + reset_at_seam(S) + \
                touch_zero(S) + open_at_end(S) + threshold_equality(S) + run_length(S, rng, (-2, -1, 0, 1, 2))
            nseq = 3
        if vset == "DRIFT":
            inst += drift_span(S)
            for x in inst:  # inexact sums: the oracle is the only reference
                x.exc = None
        # per sequence: a run of three chunks first, then instances in turn
        self.seq_items = [[Instance(f"lead/{q}", "lead", _random(rng, 3 * chunk - 5), None)] for q in range(nseq)]
        for n, x in enumerate(inst):
            self.seq_items[n % nseq].append(x)
        self.gaps = [[int(g) for g in rng.integers(1, 6, size=len(items) + 1)] for items in self.seq_items]
        self.instances = [x for items in self.seq_items for x in items]
        self.n_runs = len(self.instances)
        self.n_scored = sum(x.P for x in self.instances)

    @functools.lru_cache(maxsize=None)
    def layout(self, k: int):
        """[(instance, sequence, a)]: the run of the instance is bytes
        [a, a + P + k) of the sequence; relative index j is scan index
        a + k + j."""
        out = []
        for q, items in enumerate(self.seq_items):
            at = self.gaps[q][0] if q % 2 else 0  # odd sequences begin with Ns
            for n, x in enumerate(items):
                out.append((x, q, at))
                at += x.P + k + self.gaps[q][n + 1]
        return out

    def sequences(self, k: int) -> list[bytes]:
        """The genome for k-mer size k: the last sequence ends with its last
        run, the others with an N gap."""
        parts = [[] for _ in self.seq_items]
        lead = np.full(k - 1, _T, dtype=np.uint8)
        one = np.full(1, _T, dtype=np.uint8)
        nn = lambda n: np.full(n, np.uint8(ord("N")), dtype=np.uint8)  # noqa: E731
        for q, items in enumerate(self.seq_items):
            if q % 2:
                parts[q].append(nn(self.gaps[q][0]))
            for n, x in enumerate(items):
                parts[q] += [lead, x.body, one]
                if n + 1 < len(items) or q + 1 < len(self.seq_items):
                    parts[q].append(nn(self.gaps[q][n + 1]))
        return [np.concatenate(p).tobytes() for p in parts]

    def predict(self, k: int, min_width: int, min_score: float):
        """Regions of the instances that have a prediction, in the oracle's
        order: {instance name: [(seq, beg, end, score)]}.  A planted excursion
        is emitted when its width and score pass; none of the plants leaves an
        excursion wider than 0 for the rescan behind an emitted region, so
        min_width >= 1 is required."""
        assert min_width >= 1
        out = {}
        for x, q, a in self.layout(k):
            if x.exc is None:
                continue
            out[x.name] = [(q, a + k + b, a + k + e, s) for b, e, s in x.exc if e - b >= min_width and s >= min_score]
        return out

    def by_instance(self, k: int, pos, score, base: int = 0) -> dict:
        """Split a result (pos int32[3, R], score[>= 1, R]; base = 1 for the
        1-based tr_lr records) by instance: {name: [(seq, beg, end, score)]}."""
        lay = self.layout(k)
        out = {x.name: [] for x, _, _ in lay}
        per_seq = {}
        for x, q, a in lay:
            per_seq.setdefault(q, []).append((a, x.name))
        starts = {q: np.array([a for a, _ in v]) for q, v in per_seq.items()}
        for n in range(pos.shape[1]):
            q, b, e = int(pos[0, n]) - base, int(pos[1, n]) - base, int(pos[2, n]) - base
            name = per_seq[q][int(np.searchsorted(starts[q], b, side="right")) - 1][1]
            out[name].append((q, b, e, float(score[0, n])))
        return out

    def explain(self, k: int, got_pos, got_score, want_pos, want_score, base: int = 0) -> list[str]:
        """One line per instance whose regions or score bits differ, with the
        differing records as (relative beg, relative end, score)."""
        g = self.by_instance(k, got_pos, got_score, base)
        w = self.by_instance(k, want_pos, want_score, base)
        rel = {x.name: a + k for x, _, a in self.layout(k)}
        bits = lambda r: (r[0], r[1], r[2], np.float64(r[3]).view(np.uint64))  # noqa: E731
        lines = []
        for name in g:
            if [bits(r) for r in g[name]] != [bits(r) for r in w[name]]:
                gs, ws = {bits(r): r for r in g[name]}, {bits(r): r for r in w[name]}
                only = lambda a, b: [(r[1] - rel[name], r[2] - rel[name], r[3])  # noqa: E731
                                     for key, r in a.items() if key not in b][:4]
                lines.append(f"{self.seam}/{self.vset} k={k} {name}: got {len(g[name])} want {len(w[name])} regions; "
                             f"only got {only(gs, ws)} only want {only(ws, gs)}")
        return lines


@functools.lru_cache(maxsize=None)
def corpus(seam: str, vset: str, chunk: int = CHUNK, tile_chunks: int = TILE_CHUNKS) -> Corpus:
    return Corpus(seam, vset, chunk, tile_chunks)
