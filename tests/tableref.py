"""Host model of the built score-table forms (kmer_spans_amd/csrc/ks_table.hip),
in plain numpy integer arithmetic, written from the layout comments there and
not from the kernels: given the base table (uint16 codes, FP64 values or 32-bit
rank codes) it returns the expected bytes of the entry or line of any index.

The base table is an *accessor*: an array, or a function (lo, n) -> array of
the entries [lo, lo + n), so that a 4^15 table is only ever read in slabs.

k-mer rules (x is the m-mer of a line, m = k + own - 1; e the (k + J - 1)-mer
of an expanded entry; the first base is the most significant):
  own k-mer t of x                 (x >> 2 (own - 1 - t)) & mask
  level-l continuation c of x      ((x << 2 l) | c) & mask, c < 4^l
  k-mer t of e                     (e >> 2 (J - 1 - t)) & mask
Lines and entries lie index-major in memory: line x at byte x * line bytes."""
from fractions import Fraction

import numpy as np

ESC12 = 0xFFF   # 12-bit escape code of the J = 5 expanded table
ESC11 = 0x7FF   # 11-bit escape code of the L3 field of a wide line


def gather(acc, idx, gap=1 << 14):
    """acc's entries at the indices idx (any shape).  An array is indexed; a
    function is read once per cluster of the distinct indices (sorted, split
    where two neighbours are more than gap apart)."""
    idx = np.asarray(idx, dtype=np.int64)
    if not callable(acc):
        return np.asarray(acc)[idx]
    u, inv = np.unique(idx.ravel(), return_inverse=True)
    cuts = np.flatnonzero(np.diff(u) > gap) + 1
    out = None
    for a, b in zip(np.concatenate(([0], cuts)), np.concatenate((cuts, [u.size]))):
        lo = int(u[a])
        slab = np.asarray(acc(lo, int(u[b - 1]) - lo + 1))
        if out is None:
            out = np.empty(u.size, dtype=slab.dtype)
        out[a:b] = slab[u[a:b] - lo]
    return out[inv].reshape(idx.shape)


def _mask(k):
    return (1 << (2 * k)) - 1


def own_kmers(x, k, own):
    """[n, own]: the k-mers inside the m-mer x, first to last."""
    x = np.asarray(x, dtype=np.int64)
    return np.stack([(x >> (2 * (own - 1 - t))) & _mask(k) for t in range(own)], axis=1)


def cont_kmers(x, k, lev):
    """[n, 4^lev]: the k-mer lev bases past x's last one, per continuation."""
    x = np.asarray(x, dtype=np.int64)
    return ((x[:, None] << (2 * lev)) | np.arange(4 ** lev, dtype=np.int64)[None, :]) & _mask(k)


def ext_kmers(e, k, J):
    """[n, J]: the J k-mers of the (k + J - 1)-mer e, first to last."""
    e = np.asarray(e, dtype=np.int64)
    return np.stack([(e >> (2 * (J - 1 - t))) & _mask(k) for t in range(J)], axis=1)


def _bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


# ---------------------------------------------------------------- expanded

def ext_u16(codes, k, J, e):
    """uint16 codes, J = 2 (uint32 entries) and 3, 4 (uint64): the code of
    k-mer t at bits 16 t."""
    c = gather(codes, ext_kmers(e, k, J)).astype(np.uint64)
    v = np.zeros(c.shape[0], dtype=np.uint64)
    for t in range(J):
        v |= c[:, t] << np.uint64(16 * t)
    return v.astype(np.uint32) if J == 2 else v


def ext_c12(codes, k, e):
    """12-bit codes, J = 5: min(code, 0xFFF) of k-mer t at bits 12 t of a
    uint64; the top four bits are zero."""
    c = np.minimum(gather(codes, ext_kmers(e, k, 5)).astype(np.uint64), np.uint64(ESC12))
    v = np.zeros(c.shape[0], dtype=np.uint64)
    for t in range(5):
        v |= c[:, t] << np.uint64(12 * t)
    return v


def ext_f64(vals, k, J, e):
    """FP64 values as bits, [n, 2] for J = 2 (16-B entries) and [n, 4] for
    J = 3, 4 (32-B entries, zero pad)."""
    b = _bits(gather(vals, ext_kmers(e, k, J)))
    out = np.zeros((b.shape[0], 2 if J <= 2 else 4), dtype=np.uint64)
    out[:, :J] = b
    return out


# ------------------------------------------------------------------- lines

def lines_u16(codes, k, own, x):
    """64-B uint16 lines [n, 32]: [own][L1 x4][L2 x16], zeros after."""
    out = np.zeros((len(x), 32), dtype=np.uint16)
    out[:, :own] = gather(codes, own_kmers(x, k, own))
    out[:, own:own + 4] = gather(codes, cont_kmers(x, k, 1))
    out[:, own + 4:own + 20] = gather(codes, cont_kmers(x, k, 2))
    return out


def lines_f64(vals, k, own, x):
    """64-B FP64 lines as bits [n, 8]: [own][L1 x4], zeros after."""
    out = np.zeros((len(x), 8), dtype=np.uint64)
    out[:, :own] = _bits(gather(vals, own_kmers(x, k, own)))
    out[:, own:own + 4] = _bits(gather(vals, cont_kmers(x, k, 1)))
    return out


def _pack(fields, width):
    """[n, f] integers -> [n, f * width] bits, the low bit of a field first."""
    f = np.asarray(fields, dtype=np.uint32)
    return ((f[:, :, None] >> np.arange(width, dtype=np.uint32)) & 1).astype(np.uint8).reshape(f.shape[0], -1)


def lines_wide(codes, k, own, x):
    """128-B wide lines as bytes [n, 128]: the 13-bit codes of own / L1 / L2
    at bit 13 j, the 64 L3 codes as min(code, 2047) in 11 bits from bit
    13 (own + 20), zeros to bit 1024."""
    head = np.concatenate([gather(codes, own_kmers(x, k, own)), gather(codes, cont_kmers(x, k, 1)),
                           gather(codes, cont_kmers(x, k, 2))], axis=1).astype(np.uint32) & 0x1FFF
    l3 = np.minimum(gather(codes, cont_kmers(x, k, 3)).astype(np.uint32), ESC11)
    bits = np.zeros((len(x), 1024), dtype=np.uint8)
    nb = 13 * (own + 20)
    bits[:, :nb] = _pack(head, 13)
    bits[:, nb:nb + 11 * 64] = _pack(l3, 11)
    return np.packbits(bits, axis=1, bitorder="little")


def lines_rank(codes32, k, own, x):
    """128-B rank-code lines [n, 32] uint32: the codes of own / L1 / L2 at
    dwords 0 .. own + 19, zeros after."""
    out = np.zeros((len(x), 32), dtype=np.uint32)
    out[:, :own] = gather(codes32, own_kmers(x, k, own))
    out[:, own:own + 4] = gather(codes32, cont_kmers(x, k, 1))
    out[:, own + 4:own + 20] = gather(codes32, cont_kmers(x, k, 2))
    return out


def line_slot_kmers(x, k, own, levels):
    """[n, own + 4 + 16 (+ 64)]: the k-mer whose value each slot of x's line
    holds, in slot order."""
    return np.concatenate([own_kmers(x, k, own)] + [cont_kmers(x, k, lev) for lev in range(1, levels + 1)], axis=1)


# -------------------------------------------------------------- renumbering

def code_weights(codes, n, ncodes, freq=None, slab=1 << 22):
    """Position weight of every code, exact (int64): the number of k-mers
    with the code, or the sum of their hint read as uint32."""
    w = np.zeros(ncodes, dtype=np.int64)
    for lo in range(0, n, slab):
        m = min(slab, n - lo)
        c = gather(codes, np.arange(lo, lo + m)) if callable(codes) else np.asarray(codes)[lo:lo + m]
        if freq is None:
            w += np.bincount(c, minlength=ncodes).astype(np.int64)
        else:
            f = (gather(freq, np.arange(lo, lo + m)) if callable(freq) else np.asarray(freq)[lo:lo + m])
            f = np.ascontiguousarray(f, dtype=np.int32).view(np.uint32).astype(np.int64)
            # (exact: bincount's float64 weights would round sums above 2^53)
            order = np.argsort(c, kind="stable")
            cs, fs = c[order], f[order]
            starts = np.flatnonzero(np.concatenate(([True], cs[1:] != cs[:-1])))
            w[cs[starts]] += np.add.reduceat(fs, starts)
    return w


def renumber(weights):
    """The weight renumbering of the codes: order[i] = the old code that
    becomes code i (weight descending, ties by old code); perm[old] = new."""
    w = np.asarray(weights, dtype=np.int64)
    order = np.argsort(-w, kind="stable")
    perm = np.empty(w.size, dtype=np.int64)
    perm[order] = np.arange(w.size)
    return order, perm


def escape_share(weights, ndirect):
    """Share of the weight outside the ndirect heaviest codes (exact
    integers, rounded once)."""
    w = sorted((int(v) for v in weights), reverse=True)
    tot = sum(w)
    return float(Fraction(tot - sum(w[:ndirect]), tot)) if tot else 0.0


# ---------------------------------------------------------- binade predictor

def approx(vals, k, freq=None, slab=1 << 22):
    """Per min(k, 7)-base prefix: the weighted mean of s over the k-mers
    extending it (weight: the hint as uint32, or 1), non-finite values and
    zero weights left out.  Returns (mean FP64, number of k-mers that
    entered); the mean is 0 where none did."""
    kp = min(k, 7)
    n, sub = 4 ** k, 4 ** (k - kp)
    slab = max(slab // sub, 1) * sub
    num, den, cnt = [], [], []
    for lo in range(0, n, slab):
        m = min(slab, n - lo)
        v = np.asarray(vals(lo, m) if callable(vals) else np.asarray(vals)[lo:lo + m], dtype=np.float64)
        if freq is None:
            wt = np.ones(m)
        else:
            f = freq(lo, m) if callable(freq) else np.asarray(freq)[lo:lo + m]
            wt = np.ascontiguousarray(f, dtype=np.int32).view(np.uint32).astype(np.float64)
        use = np.isfinite(v) & (wt > 0)
        v = np.where(use, v, 0.0).reshape(-1, sub)
        wt = np.where(use, wt, 0.0).reshape(-1, sub)
        num.append((wt * v).sum(axis=1))
        den.append(wt.sum(axis=1))
        cnt.append(use.reshape(-1, sub).sum(axis=1))
    num, den, cnt = np.concatenate(num), np.concatenate(den), np.concatenate(cnt)
    return np.where(den > 0, num / np.where(den > 0, den, 1.0), 0.0), cnt


def to_f16_bits(mean):
    """FP64 -> FP32 -> FP16, as bits."""
    with np.errstate(over="ignore"):
        return np.asarray(mean, dtype=np.float64).astype(np.float32).astype(np.float16).view(np.uint16)


def f16_ulps(a, b):
    """Distance of two arrays of FP16 bits in representable values (+0 and
    -0 are one value apart)."""
    def key(u):
        u = np.asarray(u, dtype=np.uint16).astype(np.int32)
        return np.where(u & 0x8000, -(u & 0x7FFF) - 1, u)
    return np.abs(key(a) - key(b))
