"""The reference's user API (kmer_spans.R) on top of the C ABI.

Same function names (dots become underscores), argument meaning, return
layout and error behaviour as /root/reference/kmer_spans.R:

  kmer_counts(seq, k, with_f=True)               kmer_spans.R:18-27
  kmer_regions(seq, k, kmer_scores, min_width, min_score)   :41-52
  kmer_low_comp_regions(seq, k, min_w, min_score, thr=0.75) :72-79
  kmer_seq(k)                                     :84-86
  lr_regions(seq, params, kmers, kmer_scores, trans_scores)  :88-99
  kmers_to_file(seq_f, out_prefix, k, min_l=1e5, magic)      :127-160
  read_kmers(fname, magic)                        :162-186
  read_fasta(path, min_len=0)   (readDNAStringSet + as.character, :136-144)
  window_kmer_dist(seq, kmers, window, freq=True, ret_flag=0)  :103-118
  region_spectra(seq, pos, q=4, both_strands=True)   (test.R:703-720: subseq +
                 oligonucleotideFrequency on both strands + Shannon entropy)
  region_distances(counts, rows=None, rows_b=None, squared=False)   (test.R:
                 762-807: dist() of the row-normalised spectra)

Sequences are a str/bytes or a list of them (R character vectors).  Results
come from libkmerspans.so on the GPU; nothing here computes a result on the
CPU.  Table builders for the README score functions are exposed as
``log2_table`` / ``pm1_table`` / ``rank_table``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import KmerSpansError, Regions, check, host_ptr, load, regions_to_numpy


class _HostSeqs:
    """(char* const*, int64 lens) view of a list of byte strings."""

    def __init__(self, seq):
        if isinstance(seq, (str, bytes, bytearray, memoryview, np.ndarray)):
            seq = [seq]
        self.bufs = []
        for s in seq:
            if isinstance(s, np.ndarray):
                b = np.ascontiguousarray(s, dtype=np.uint8)
            elif isinstance(s, str):
                b = np.frombuffer(s.encode("latin-1"), dtype=np.uint8)
            else:
                b = np.frombuffer(bytes(s), dtype=np.uint8)
            self.bufs.append(b)
        self.n = len(self.bufs)
        self._empty = np.zeros(1, dtype=np.uint8)
        self.ptrs = (C.c_void_p * max(self.n, 1))()
        for i, b in enumerate(self.bufs):
            self.ptrs[i] = b.ctypes.data if b.size else self._empty.ctypes.data
        self.lens = np.array([b.size for b in self.bufs] or [0], dtype=np.int64)


def set_devices(devices) -> None:
    """Devices the host entry points (kmer_counts, kmer_regions,
    kmer_low_comp_regions on device 0, i.e. the library's default) spread a
    call over (ks_set_devices: LPT shards, one context and host thread per
    entry, counts added, regions merged into the caller's order).  [] or one
    device: device 0 alone.  The list may repeat a device."""
    d = np.ascontiguousarray(np.asarray(list(devices), dtype=np.int32))
    check(load().ks_set_devices(d.ctypes.data if d.size else None, int(d.size)))


def get_devices() -> list:
    n = int(load().ks_get_devices(None, 0))
    d = np.zeros(max(n, 1), dtype=np.int32)
    load().ks_get_devices(d.ctypes.data, n)
    return d[:n].tolist()


def _ctx(device):
    """Device 0 uses the library's lazily created default context, so that
    argument errors surface before any HIP call (kmer_spans.c validates before
    allocating); other devices get an explicit context."""
    return None if int(device) == 0 else _lib.context(device).handle


def kmer_seq(k: int) -> list[str]:
    """k-mer strings in the internal A,C,T,G code order (kmer_seq_r)."""
    k = int(k)
    if k < 1 or k > _lib.KS_MAX_K:
        check(load().ks_kmer_seq(k, None, 0))
    n = 4 ** k
    buf = C.create_string_buffer(n * (k + 1))
    check(load().ks_kmer_seq(k, buf, n * (k + 1)))
    raw = buf.raw
    return [raw[i * (k + 1):i * (k + 1) + k].decode() for i in range(n)]


def kmer_counts(seq, k: int, with_f: bool = True, device: int = 0) -> dict:
    """kmer.counts: {'n': {'k': k, 'n': words}, 'counts': int32[4^k], 'f': ...}."""
    k = int(k)
    hs = _HostSeqs(seq)
    counts = np.zeros(4 ** k if 1 <= k <= _lib.KS_MAX_K else 1, dtype=np.int32)
    n = C.c_double(0)
    check(load().ks_kmer_counts(_ctx(device), hs.ptrs, hs.lens.ctypes.data, hs.n, k,
                                counts.ctypes.data, C.byref(n)))
    out = {"n": {"k": k, "n": n.value}, "counts": counts}
    if with_f:
        with np.errstate(invalid="ignore", divide="ignore"):
            out["f"] = counts / float(counts.astype(np.int64).sum())
    return out


def _ordered_scores(k: int, kmer_scores):
    """kmer.regions reorders a named score vector by kmer.seq(k)
    (kmer_spans.R:42-47); an unnamed array is taken as internal order."""
    if isinstance(kmer_scores, dict):
        if len(kmer_scores) != 4 ** k:
            raise KmerSpansError("There should be a total of 4^k scores")
        names = kmer_seq(k)
        if any(nm not in kmer_scores for nm in names):
            raise KmerSpansError("all kmers not defined")
        return np.array([kmer_scores[nm] for nm in names], dtype=np.float64)
    if hasattr(kmer_scores, "index") and hasattr(kmer_scores, "values"):  # pandas Series
        return _ordered_scores(k, dict(zip(kmer_scores.index, kmer_scores.values)))
    w = np.ascontiguousarray(kmer_scores, dtype=np.float64).ravel()
    if w.size != 4 ** k:
        raise KmerSpansError("There should be a total of 4^k scores")
    return w


def kmer_regions(seq, k: int, kmer_scores, min_width: int, min_score: float, visits: bool = True,
                 device: int = 0) -> dict:
    """kmer.regions: {'n', 'counts' (visit histogram), 'pos' int32[3, R]
    (seq_id, beg, end), 'score' float64[2, R] (score, 0)} -- not transposed,
    exactly as kmer_spans.R:48-51 returns it."""
    k = int(k)
    w = _ordered_scores(k, kmer_scores)
    hs = _HostSeqs(seq)
    vis = np.zeros(4 ** k, dtype=np.int32) if visits else None
    n = C.c_double(0)
    r = Regions()
    check(load().ks_kmer_regions(_ctx(device), hs.ptrs, hs.lens.ctypes.data, hs.n, k, w.ctypes.data,
                                 w.size, int(min_width), float(min_score), host_ptr(vis), C.byref(n), C.byref(r)))
    pos, score = regions_to_numpy(r)
    return {"n": n.value, "counts": vis, "pos": pos, "score": score}


def kmer_low_comp_regions(seq, k: int, min_w: int, min_score: float, thr: float = 0.75,
                          device: int = 0) -> dict:
    """kmer.low.comp.regions: {'n' [#words, 0], 'counts', 'w_rank',
    'pos' int32[R, 3], 'score' float64[R, 2]} (pos/score transposed as
    kmer_spans.R:76-77 does)."""
    k = int(k)
    hs = _HostSeqs(seq)
    nk = 4 ** k if 1 <= k <= _lib.KS_MAX_K else 1
    counts = np.zeros(nk, dtype=np.int32)
    ranks = np.zeros(nk, dtype=np.float64)
    n = np.zeros(2, dtype=np.float64)
    r = Regions()
    check(load().ks_low_comp_regions(_ctx(device), hs.ptrs, hs.lens.ctypes.data, hs.n, k, int(min_w),
                                     float(min_score), float(thr), counts.ctypes.data,
                                     ranks.ctypes.data, n.ctypes.data, C.byref(r)))
    pos, score = regions_to_numpy(r)
    return {"n": n, "counts": counts, "w_rank": ranks, "pos": pos.T.copy(), "score": score.T.copy()}


def lr_regions(seq, params, kmers, kmer_scores, trans_scores, device: int = 0) -> dict:
    """lr.regions (kmer_spans.R:88-99) -> tr_lr_regions_r (kmer_spans.c:649-713):
    {'kmer_scores': float64[4^k, 2] (the scores remapped to 2-bit code order,
    rows named by kmer_seq(k)), 'reg': {'seq_i', 'beg', 'end', 'score', 'null'}}
    with 1-based sequence indices and positions, as the reference returns them.
    params = (k, min_length); kmers[i] spells entry i of both score vectors."""
    if len(params) != 2:
        raise KmerSpansError("params_r should have two integers (k, and min_length)")
    k, min_length = int(params[0]), int(params[1])
    hs = _HostSeqs(seq)
    ks_in = np.ascontiguousarray(kmer_scores, dtype=np.float64).ravel()
    tr_in = np.ascontiguousarray(trans_scores, dtype=np.float64).ravel()
    n = len(kmers)
    if ks_in.size != n or tr_in.size != n:
        raise KmerSpansError("kmers_r, freq_a, freq_b should all be 4^k long")
    bufs = [C.create_string_buffer(x.encode("latin-1") if isinstance(x, str) else bytes(x)) for x in kmers]
    kptrs = (C.c_char_p * max(n, 1))(*[C.cast(b, C.c_char_p) for b in bufs])
    nk = 4 ** k if 1 <= k <= _lib.KS_MAX_K else 1
    spectra = np.zeros(2 * nk, dtype=np.float64)
    r = Regions()
    check(load().ks_tr_lr_regions(_ctx(device), hs.ptrs, hs.lens.ctypes.data, hs.n, k, min_length, kptrs,
                                  ks_in.ctypes.data, tr_in.ctypes.data, n, spectra.ctypes.data, C.byref(r)))
    pos, score = regions_to_numpy(r)
    reg = {"seq_i": pos[0], "beg": pos[1], "end": pos[2], "score": score[0], "null": score[1]}
    return {"kmer_scores": spectra.reshape(2, nk).T.copy(), "reg": reg, "pos": pos, "score": score}


def _pos_rows(pos):
    """(seq_id, beg, end) int32 rows of a region matrix given as [3, R]
    (kmer_regions) or [R, 3] (kmer_low_comp_regions).  A 3 x 3 input is read
    as [3, R]."""
    a = np.asarray(pos)
    if a.ndim != 2 or 3 not in a.shape:
        raise KmerSpansError("pos must be a [3, R] or [R, 3] matrix of (seq_id, beg, end)")
    if a.shape[0] != 3:
        a = a.T
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a[0], a[1], a[2]


def region_spectra(seq, pos, q: int = 4, both_strands: bool = True, seq_base: int = 0, device: int = 0) -> dict:
    """The q-mer spectrum and Shannon entropy of every region (what test.R:
    703-720 computes with subseq + oligonucleotideFrequency, on the GPU).

    pos: the regions as kmer_regions returns them ([3, R]: seq_id, beg, end)
    or as kmer_low_comp_regions does ([R, 3]); both are accepted by shape, a
    3 x 3 matrix is read as [3, R].  seq_id is 0-based (seq_base=1 for the
    1-based ids of lr_regions), beg..end 1-based inclusive.  Returns
    {'kmers': kmer_seq(q), 'counts': uint32[R, 4^q] (columns in kmer_seq(q)
    order -- internal A,C,T,G, not alphabetical; both strands folded,
    n[c] + n[rc(c)], when both_strands), 'freq': float64[R, 4^q] = counts /
    row sum (NaN rows where the sum is 0), 'entropy': float64[R] (NaN there
    too)}.  Windows holding N/n are skipped; unlike Biostrings, other non-ACGT
    letters are coded (c >> 1) & 3 like everywhere in this library."""
    q = int(q)
    sid, beg, end = _pos_rows(pos)
    if seq_base:
        sid = sid - np.int32(seq_base)
    n = int(sid.size)
    hs = _HostSeqs(seq)
    nb = 4 ** q if 1 <= q <= _lib.KS_SPECTRA_MAX_Q else 1
    counts = np.zeros((n, nb), dtype=np.uint32)
    ent = np.zeros(n, dtype=np.float64)
    sid, beg, end = (np.ascontiguousarray(x, dtype=np.int32) for x in (sid, beg, end))
    check(load().ks_region_spectra(_ctx(device), hs.ptrs, hs.lens.ctypes.data, hs.n, sid.ctypes.data,
                                   beg.ctypes.data, end.ctypes.data, n, q,
                                   _lib.KS_SPECTRA_BOTH_STRANDS if both_strands else 0,
                                   counts.ctypes.data, ent.ctypes.data))
    with np.errstate(invalid="ignore", divide="ignore"):
        freq = counts / counts.sum(axis=1, dtype=np.float64)[:, None]
    return {"kmers": kmer_seq(q), "counts": counts, "freq": freq, "entropy": ent}


def region_distances(counts, rows=None, rows_b=None, squared: bool = False, device: int = 0,
                     metric: str = "euclidean") -> np.ndarray:
    """Distances between row-normalised spectra (R's dist() on reg.kmer.sp,
    test.R:762-807) from the counts region_spectra returns; Euclidean unless
    metric= says otherwise.

    counts: [n, ncol] non-negative integers (uint32 range), 1 <= ncol <= 4096.
    A row's profile is counts / row sum; the distance of two rows is the FP64
    sum over the columns, in order, of the squared profile differences --
    squared=True returns that sum, otherwise its square root.  An empty row
    is NaN against every row; rows with proportional counts are at exactly 0.
    metric: "euclidean", or "manhattan", "maximum", "canberra" as in R's
    dist(method=) (canberra omits the columns where both profiles are 0 and
    scales the sum by ncol / columns kept), or "hellinger": sqrt(0.5 * the
    squared Euclidean distance of the profiles' square roots), in [0, 1].
    squared=True needs "euclidean" or "hellinger".  Every metric is a fixed
    order of FP64 operations (include/kmer_spans.h).
    rows / rows_b: optional integer row indices (any order, repeats allowed).
    rows_b is None: the condensed form, float64[m(m-1)/2] over the pairs i < j
    of the selected rows (all rows when rows is None) in the order of R's dist
    object and scipy's pdist.  Otherwise the dense float64[na, nb] block of
    rows (all rows when None) against rows_b."""
    c, n, ncol = _lib.counts_arg(counts)
    ra, na = _lib.rows_arg(rows, "rows", n)
    rb, nb = _lib.rows_arg(rows_b, "rows_b", 0)
    flags = _lib.dist_flags(metric, squared)
    L = load()
    if rows_b is None:
        out = np.zeros(na * (na - 1) // 2 if na > 1 else 0, dtype=np.float64)
        check(L.ks_spectra_dist(_ctx(device), c.ctypes.data, n, ncol, host_ptr(ra), na, flags, out.ctypes.data))
        return out
    out = np.zeros((na, nb), dtype=np.float64)
    check(L.ks_spectra_cross_dist(_ctx(device), c.ctypes.data, n, ncol, host_ptr(ra), na, rb.ctypes.data, nb, flags,
                                  out.ctypes.data))
    return out


def region_pca(counts, rows=None, center: bool = True, ncomp=None, scores: bool = True, device: int = 0) -> dict:
    """Principal components of row-normalised spectra (R's prcomp() on
    reg.kmer.sp, test.R:734-736 and :811) from the counts region_spectra
    returns, computed on the device.

    counts: [n, ncol] non-negative integers (uint32 range), 1 <= ncol <= 1024
    (q <= 5).  rows: optional integer row indices (any order, repeats allowed;
    at least 2 rows); None = all rows.  A row's profile is counts / row sum; a
    selected row without counts is an error naming its position.  center=False
    is prcomp's center=FALSE.  ncomp: components kept (default all ncol).
    Returns {'sdev': float64[ncol] (R's sdev, over m - 1), 'rotation':
    float64[ncol, ncomp] (loadings, columns by descending variance, each with
    its largest entry positive), 'center': float64[ncol] (zeros when not
    centred), 'x': float64[m, ncomp] scores, or None with scores=False}.  The
    centre and the scores are fixed orders of FP64 operations
    (include/kmer_spans.h); the same input gives the same bits on every run."""
    c, n, ncol = _lib.counts_arg(counts)
    r, m = _lib.rows_arg(rows, "rows", n)
    k = ncol if ncomp is None else int(ncomp)
    kk = max(0, min(k, ncol))  # a bad ncomp is the library's error; the buffers only need a size
    cen, sdev = np.zeros(ncol, dtype=np.float64), np.zeros(ncol, dtype=np.float64)
    rot = np.zeros((ncol, kk), dtype=np.float64)
    x = np.zeros((max(m, 0), kk), dtype=np.float64) if scores else None
    check(load().ks_spectra_pca(_ctx(device), c.ctypes.data, n, ncol, host_ptr(r), m,
                                0 if center else _lib.KS_PCA_NO_CENTER, k, cen.ctypes.data, sdev.ctypes.data,
                                rot.ctypes.data, host_ptr(x), None))
    return {"sdev": sdev, "rotation": rot, "center": cen, "x": x}


def region_kmeans(counts, centers, rows=None, iter_max: int = 10, device: int = 0) -> dict:
    """R's kmeans(x, centers, iter.max, algorithm="Lloyd") on row-normalised
    spectra, from the counts region_spectra returns, computed on the device
    without any distance matrix: memory is O((m + g) ncol).

    counts: [n, ncol] non-negative integers (uint32 range), 1 <= ncol <= 4096.
    rows: optional integer row indices (any order, repeats allowed); None = all
    rows.  A row's profile is counts / row sum; a selected row without counts
    is an error naming its position.  centers: a [g, ncol] float matrix of
    initial centres (every entry finite), or a 1-d sequence of g integer
    positions into the selection whose profiles are the initial centres
    (region_kmeans_seed chooses such positions).  Duplicate centres
    are allowed; the lowest label wins every tie.  1 <= g <= 65536.  Returns
    {'cluster': int32[m] labels 1 .. g, 'centers': float64[g, ncol], 'size':
    int32[g], 'withinss': float64[g], 'tot_withinss', 'totss', 'betweenss'
    (totss - tot_withinss): float, 'iter': assignment passes run, 'converged':
    bool}.  A group that loses all its members keeps its centre (R stops
    there).  As in R, after iter_max passes without convergence the centres
    are one update ahead of the labels.  Every sum is a fixed order of FP64
    operations (include/kmer_spans.h): the same input gives the same bits on
    every run."""
    c, n, ncol = _lib.counts_arg(counts)
    r, m = _lib.rows_arg(rows, "rows", n)
    init, init_rows, g = _lib.kmeans_centers(centers, ncol)
    cluster = np.zeros(max(m, 0), dtype=np.int32)
    cen = np.zeros((g, ncol), dtype=np.float64)
    size, wss = np.zeros(g, dtype=np.int32), np.zeros(g, dtype=np.float64)
    res = _lib.KmeansResult()
    check(load().ks_spectra_kmeans(_ctx(device), c.ctypes.data, n, ncol, host_ptr(r), m, host_ptr(init),
                                   host_ptr(init_rows), g, int(iter_max), 0, cluster.ctypes.data, cen.ctypes.data,
                                   size.ctypes.data, wss.ctypes.data, C.byref(res)))
    return dict({"cluster": cluster, "centers": cen, "size": size, "withinss": wss}, **_lib.kmeans_result(res))


def region_group_means(counts, group, ngroups=None, rows=None, device: int = 0) -> dict:
    """The mean spectrum of every group of a labelling of row-normalised
    spectra (for instance the groups of cut_tree), with the groups' sizes and
    within sums of squares: the update and withinss steps of region_kmeans as
    a call of their own, on the device.

    counts, rows: as for region_kmeans.  group: one integer label in 1 ..
    ngroups per selected row; ngroups defaults to the largest label.  Returns
    {'centers': float64[g, ncol] (a row of NaN for a group without members),
    'size': int32[g], 'withinss': float64[g] (0 for an empty group)}.  The
    centres can start region_kmeans when no group is empty."""
    c, n, ncol = _lib.counts_arg(counts)
    r, m = _lib.rows_arg(rows, "rows", n)
    g, ng = _lib.silhouette_group(group, m, ngroups)
    ngb = min(ng, _lib.KS_KM_MAX_GROUPS)  # a larger ngroups is the library's error; the buffers only need a size
    cen = np.zeros((ngb, ncol), dtype=np.float64)
    size, wss = np.zeros(ngb, dtype=np.int32), np.zeros(ngb, dtype=np.float64)
    check(load().ks_spectra_group_means(_ctx(device), c.ctypes.data, n, ncol, host_ptr(r), m, g.ctypes.data, ng, 0,
                                        cen.ctypes.data, size.ctypes.data, wss.ctypes.data))
    return {"centers": cen, "size": size, "withinss": wss}


def region_kmeans_seed(counts, g, method: str = "maximin", rows=None, first=0, u=None, seed=None,
                       device: int = 0) -> dict:
    """g rows of the selection to start region_kmeans from, chosen on the
    device in O(m ncol) memory: no distance matrix and nothing of size m x g.

    counts, rows: as for region_kmeans.  method="maximin": farthest-first
    traversal from row `first`; every later pick is the row farthest from the
    rows picked so far (the lowest position on a tie).  Nothing is drawn, and
    'pick_dist' is the squared covering radius as a function of the number of
    centres: where it flattens, more groups buy little.  method="kmeans++": D^2
    sampling; pick j is drawn with probability proportional to the squared
    distance to the nearest earlier pick, from the uniform number u[j].  Give u
    (g numbers in [0, 1)) or seed; with seed, u is
    np.random.default_rng(seed).random(g), drawn here: the library has no
    generator.  first=None (k-means++ only) draws the first row as
    int(u[0] * m).  1 <= g <= 65536; g > m is allowed (the surplus picks repeat
    position 0 at distance 0).  Returns {'rows': int64[g] positions into the
    selection (region_kmeans(..., centers=res['rows'])), 'nearest': int32[m]
    the 1-based pick nearest to every row (the lowest on a tie), 'mindist':
    float64[m] its squared distance, 'pick_dist': float64[g] the squared
    distance of every pick to the earlier picks (inf for the first),
    'potential': float64[g] the sum of mindist before every pick (inf for the
    first), 'n_distinct': picks that differ from all earlier ones,
    'potential_final', 'radius' and 'far_row': the sum and the largest mindist
    after the last pick and its row}.  Every value is a fixed order of FP64
    operations (include/kmer_spans.h): the same input gives the same bits on
    every run."""
    c, n, ncol = _lib.counts_arg(counts)
    r, m = _lib.rows_arg(rows, "rows", n)
    g, gb, flags, first, u = _lib.seed_args(g, method, first, u, seed)
    picked = np.zeros(gb, dtype=np.int64)
    near, mind = np.zeros(max(m, 0), dtype=np.int32), np.zeros(max(m, 0), dtype=np.float64)
    pd, pot = np.zeros(gb, dtype=np.float64), np.zeros(gb, dtype=np.float64)
    res = _lib.SeedResult()
    check(load().ks_spectra_kmeans_seed(_ctx(device), c.ctypes.data, n, ncol, host_ptr(r), m, g, flags, first,
                                        host_ptr(u), picked.ctypes.data, near.ctypes.data, mind.ctypes.data,
                                        pd.ctypes.data, pot.ctypes.data, C.byref(res)))
    return dict({"rows": picked, "nearest": near, "mindist": mind, "pick_dist": pd, "potential": pot},
                **_lib.seed_result(res))


def region_knn(counts, k, rows=None, rows_b=None, squared: bool = False, device: int = 0,
               metric: str = "euclidean"):
    """The k nearest regions of every region by spectrum, computed on the
    device without the distance matrix: memory is the profile panel plus
    O(na k), and nothing of size na x nb is written or sorted.

    counts: [n, ncol] non-negative integers (uint32 range), 1 <= ncol <= 4096.
    rows: the queries, optional integer row indices (any order, repeats
    allowed); None = all rows.  rows_b: the candidates.  None is the self form:
    the candidates are the queries themselves and position s is left out of its
    own list (by position: a row named twice finds its other copy at exactly
    0).  Otherwise every row of rows_b counts.  1 <= k <= 64, and k may not
    exceed the number of candidates (na - 1 in the self form).  A selected row
    without counts is an error naming its position.  The distance is
    region_distances': squared=True returns the FP64 sum of squared profile
    differences, otherwise its square root; metric= names another metric as in
    region_distances, and every returned distance has the bits region_distances
    gives for that pair.  Returns (index, dist): int64
    [na, k] positions into the candidate selection (not row indices) and
    float64 [na, k], column 0 the nearest; the k candidates with the smallest
    (squared distance, position), ascending, so ties go to the lowest position
    and the same input gives the same bits on every run ("manhattan",
    "maximum" and "canberra" rank by the distance itself)."""
    c, n, ncol = _lib.counts_arg(counts)
    ra, na = _lib.rows_arg(rows, "rows", n)
    rb, nb = _lib.rows_arg(rows_b, "rows_b", 0)
    k, kb = _lib.knn_k(k)
    flags = _lib.dist_flags(metric, squared)
    index = np.zeros((max(na, 0), kb), dtype=np.int64)
    dist = np.zeros((max(na, 0), kb), dtype=np.float64)
    check(load().ks_spectra_knn(_ctx(device), c.ctypes.data, n, ncol, host_ptr(ra), na, host_ptr(rb), nb, k,
                                flags, index.ctypes.data, dist.ctypes.data))
    return index, dist


def region_hclust(dist, method: str = "complete", device: int = 0) -> dict:
    """R's hclust() of a condensed dissimilarity vector (test.R:776), run on
    the device.

    dist: float64[n(n-1)/2], the condensed form region_distances returns (R's
    dist object, scipy's pdist); n is solved from its length.  Every entry
    must be finite.  method: "complete" (R's default), "single" or "average".
    The nearest-neighbour-list agglomeration with every tie going to the
    lowest index (include/kmer_spans.h): complete and single heights carry the
    bits of input entries.  Returns {'merge': int32[n-1, 2], 'height':
    float64[n-1], 'order': int32[n], 'method'} as in R's hclust object:
    observation i (0-based) is -(i+1), the cluster of step t is t+1, order
    lists the leaves 1-based from left to right."""
    d, n = _lib.condensed_arg(dist, 2)
    merge, height, order = _lib.hclust_outputs(n)
    check(load().ks_hclust(_ctx(device), d.ctypes.data, n, _lib.hclust_method(method), merge.ctypes.data,
                           height.ctypes.data, order.ctypes.data))
    return {"merge": merge, "height": height, "order": order, "method": method}


def cut_tree(tree_or_merge, height=None, k=None, h=None) -> np.ndarray:
    """R's cutree(): the groups of a tree from region_hclust, on the host.

    tree_or_merge: the dict region_hclust returns, or its merge table with
    height=.  Give exactly one of k (the number of groups, 1 .. n) and h (a
    height: every merge at or below it is applied; the heights must be
    non-decreasing).  Returns int32[n] group numbers 1 .. k in order of first
    appearance: observation 0 is in group 1.  With complete linkage h bounds
    every group's diameter."""
    if isinstance(tree_or_merge, dict):
        merge, height = tree_or_merge["merge"], tree_or_merge["height"]
    else:
        merge = tree_or_merge
    if (k is None) == (h is None):
        raise KmerSpansError("give exactly one of k and h")
    merge = np.ascontiguousarray(merge, dtype=np.int32)
    if merge.ndim != 2 or merge.shape[1] != 2:
        raise KmerSpansError("merge must be an int32 [n-1, 2] table")
    n = int(merge.shape[0]) + 1
    hp = None
    if height is not None:
        height = np.ascontiguousarray(height, dtype=np.float64)
        if height.shape != (n - 1,):
            raise KmerSpansError("height must hold one value per row of merge")
        hp = height.ctypes.data
    if k is not None:
        if int(k) != k or not 1 <= int(k) <= n:
            raise KmerSpansError(f"k = {k} is not in 1 .. n = {n}")
    group = np.zeros(n, dtype=np.int32)
    check(load().ks_hclust_cut(merge.ctypes.data, hp, n, int(k) if k is not None else 0,
                               float(h) if h is not None else 0.0, group.ctypes.data))
    return group


def region_nj(dist, device: int = 0) -> dict:
    """ape's nj() of a condensed dissimilarity vector (the tree test.R:770-775
    and :861-864 give up on as far too slow), run on the device.

    dist: float64[n(n-1)/2], the condensed form region_distances returns; n >=
    3 is solved from its length.  Every entry must be finite.  Canonical
    neighbour joining with every tie going to the lowest pair and the row sums
    updated incrementally (include/kmer_spans.h has the order of operations;
    last bits may differ from ape's, which recomputes the sums).  Returns
    {'join': int32[n-3, 2], 'length': float64[n-3, 2], 'root': int32[3],
    'root_length': float64[3]}: step t joins the nodes join[t] by edges of
    length[t] into node t+1, observation i (0-based) is -(i+1), and root names
    the three children of the final trifurcation.  Negative lengths are
    returned as computed."""
    d, n = _lib.condensed_arg(dist, 3)
    join, length, root, root_length = _lib.nj_outputs(n)
    check(load().ks_nj(_ctx(device), d.ctypes.data, n, join.ctypes.data, length.ctypes.data, root.ctypes.data,
                       root_length.ctypes.data))
    return {"join": join, "length": length, "root": root, "root_length": root_length}


def region_silhouette(dist, group, ngroups=None, sums: bool = False, device: int = 0) -> dict:
    """R's cluster::silhouette(cutree(hc, k), d) of a condensed dissimilarity
    vector and a grouping of its observations, with each group's medoid and
    diameter, run on the device.

    dist: float64[n(n-1)/2], the condensed form region_distances returns; n >=
    2 is solved from its length.  Every entry must be finite.  group: n integer
    labels in 1 .. ngroups, as cut_tree returns them; ngroups defaults to the
    largest label, groups without members are allowed, at least two must have
    some.  Returns {'width', 'a', 'b': float64[n] (a the mean distance to the
    own group, b to the nearest other one, width (b - a) / max(a, b), 0 for a
    group of one), 'neighbor': int32[n] (the label of that nearest group),
    'size', 'medoid': int32[g] (the 0-based member with the smallest sum of
    distances to its group, -1 for an empty group), 'diameter', 'avg_width':
    float64[g] (NaN for an empty group), 'avg_width_all': float}; with
    sums=True also 'sums': float64[n, g], the sum of D(i, j) over the members j
    of each group.  Every sum is a fixed order of FP64 additions
    (include/kmer_spans.h): the same input gives the same bits on every run."""
    d, n = _lib.condensed_arg(dist, 2)
    g, ng = _lib.silhouette_group(group, n, ngroups)
    res = _lib.silhouette_outputs(n, ng)
    s = np.zeros((n, ng), dtype=np.float64) if sums else None
    check(load().ks_silhouette(_ctx(device), d.ctypes.data, n, g.ctypes.data, ng, 0, *_lib.silhouette_out_args(res),
                               host_ptr(s)))
    res["avg_width_all"] = float(res["avg_width_all"][0])
    if sums:
        res["sums"] = s
    return res


def _nj_tables(tree):
    """(join, length, root, root_length, n) of a region_nj tree, shapes checked."""
    join = np.ascontiguousarray(tree["join"], dtype=np.int32)
    length = np.ascontiguousarray(tree["length"], dtype=np.float64)
    root = np.ascontiguousarray(tree["root"], dtype=np.int32)
    root_length = np.ascontiguousarray(tree["root_length"], dtype=np.float64)
    if (join.ndim != 2 or join.shape[1] != 2 or length.shape != join.shape or root.shape != (3,)
            or root_length.shape != (3,)):
        raise KmerSpansError("a tree holds join and length [n-3, 2], root and root_length [3]")
    return join, length, root, root_length, int(join.shape[0]) + 3


def nj_edges(tree) -> dict:
    """The tree of region_nj in the layout of ape's phylo object (test.R:824),
    on the host: tips 1 .. n, the trifurcation n+1, the node of step t as
    2n-2-t.  Returns {'edge': int32[2n-3, 2] (parent, child), 'edge_length':
    float64[2n-3], 'Nnode': n-2, 'n_tip': n}, in preorder from the
    trifurcation with children in stored order."""
    join, length, root, root_length, n = _nj_tables(tree)
    edge = np.zeros((2 * n - 3, 2), dtype=np.int32)
    edge_length = np.zeros(2 * n - 3, dtype=np.float64)
    check(load().ks_nj_edges(join.ctypes.data if n > 3 else None, length.ctypes.data if n > 3 else None,
                             root.ctypes.data, root_length.ctypes.data, n, edge.ctypes.data,
                             edge_length.ctypes.data))
    return {"edge": edge, "edge_length": edge_length, "Nnode": n - 2, "n_tip": n}


def nj_newick(tree, labels=None) -> str:
    """The tree of region_nj as a Newick string, '(a:1.0,(b:0.5,c:0.25):2.0,d:1.5);'.
    Lengths are written with repr(), so they read back as the same doubles.
    labels: n strings without Newick punctuation (default '1' .. 'n')."""
    join, length, root, root_length, n = _nj_tables(tree)
    if labels is None:
        labels = [str(i + 1) for i in range(n)]
    labels = [str(x) for x in labels]
    if len(labels) != n:
        raise KmerSpansError(f"{n} labels are needed, {len(labels)} were given")
    for x in labels:
        if not x or any(c in x for c in "():,; \t\n'[]"):
            raise KmerSpansError(f"label {x!r} is empty or holds Newick punctuation")
    nj_edges(tree)  # rejects a malformed table, so the walk below ends
    # an explicit stack (a caterpillar tree is n deep): strings are emitted as
    # they are, (code, length) pairs are expanded
    out = []
    stack = [";", ")"]
    for c in (2, 1, 0):
        stack.append((int(root[c]), float(root_length[c])))
        stack.append("," if c else "(")
    while stack:
        item = stack.pop()
        if isinstance(item, str):
            out.append(item)
            continue
        code, ln = item
        if code < 0:
            out.append(f"{labels[-code - 1]}:{ln!r}")
        else:
            t = code - 1
            stack.append(f"):{ln!r}")
            stack.append((int(join[t, 1]), float(length[t, 1])))
            stack.append(",")
            stack.append((int(join[t, 0]), float(length[t, 0])))
            stack.append("(")
    return "".join(out)


# ------------------------------------------------------------ table builders

def _table(fn, counts, k):
    counts = np.ascontiguousarray(counts, dtype=np.int32)
    out = np.zeros(4 ** int(k), dtype=np.float64)
    check(fn(counts.ctypes.data, int(k), out.ctypes.data))
    return out


def log2_table(counts, k: int) -> np.ndarray:
    """log2(f / f_med) with f = counts / sum(counts) (README.md:27-29)."""
    return _table(load().ks_log2_table, counts, k)


def pm1_table(counts, k: int) -> np.ndarray:
    """ifelse(f >= f_med, 1, -1) (README.md:37-42)."""
    return _table(load().ks_pm1_table, counts, k)


def rank_table(counts, k: int, total: float) -> np.ndarray:
    """Weighted rank (rank_kmers_w, kmer_spans.c:189-202)."""
    counts = np.ascontiguousarray(counts, dtype=np.int32)
    out = np.zeros(4 ** int(k), dtype=np.float64)
    check(load().ks_rank_table(counts.ctypes.data, int(k), float(total), out.ctypes.data))
    return out


KMER_MAGIC = 310572  # kmer.magic(), kmer_spans.R:5


def kmer_magic() -> int:
    return KMER_MAGIC


def read_fasta(path, min_len: int = 0, device: int = 0):
    """Read a (plain or gzip) FASTA file, parsed on the GPU: returns
    (names, sequences) with the sequences upper-cased, records shorter than
    min_len dropped."""
    from . import device as D
    fa = D.load_fasta(None if int(device) == 0 else _lib.context(device), path, min_len)
    try:
        return fa.names, [b.decode("latin-1") for b in fa.host_seqs()]
    finally:
        fa.close()


def kmers_to_file(seq_f, out_prefix, k, min_l=1e5, magic: int = KMER_MAGIC, device: int = 0) -> list:
    """kmers.to.file: count every k of seq_f's records of length >= min_l into
    <out_prefix>counts_<k...>.bin.  Returns [seq_f, out_f or None (R's NA),
    seq.size, seq.fsize, seq.fl] like the reference's list."""
    ks = np.atleast_1d(np.asarray(k)).astype(np.int32)
    info = _lib.KmerFileInfo()
    check(load().ks_kmers_to_file(_ctx(device), str(seq_f).encode(), str(out_prefix).encode(), ks.ctypes.data,
                                  int(ks.size), float(min_l), int(magic), C.byref(info)))
    out_f = info.out_path.decode() if info.written else None
    return [seq_f, out_f, info.seq_size, info.seq_fsize, info.seq_fl]


def read_kmers(fname, magic: int = KMER_MAGIC):
    """read.kmers: {'k': int array, 'counts': [int32 arrays]} or False."""
    cf = _lib.CountFile()
    check(load().ks_count_file_read(str(fname).encode(), int(magic), C.byref(cf)))
    try:
        if not cf.valid:
            return False
        nk = int(cf.nk)
        ks = np.array([cf.k[i] for i in range(nk)], dtype=np.int32)
        counts = [np.ctypeslib.as_array(cf.counts[i], shape=(int(cf.lens[i]),)).copy() if cf.lens[i] else
                  np.zeros(0, dtype=np.int32) for i in range(nk)]
        return {"k": ks, "counts": counts}
    finally:
        load().ks_count_file_free(C.byref(cf))


def write_kmers(fname, ks, counts, magic: int = KMER_MAGIC) -> None:
    """Write a count file in kmers.to.file's format from host count vectors."""
    ks = np.atleast_1d(np.asarray(ks)).astype(np.int32)
    arrs = [np.ascontiguousarray(c, dtype=np.int32) for c in counts]
    for kk, a in zip(ks, arrs):
        if a.size != 4 ** int(kk):
            raise KmerSpansError(f"counts for k={int(kk)} must have 4^k entries")
    ptrs = (C.c_void_p * max(len(arrs), 1))(*[a.ctypes.data for a in arrs])
    check(load().ks_count_file_write(str(fname).encode(), int(magic), int(ks.size), ks.ctypes.data, ptrs))


def r_recycled_freq(dist: np.ndarray) -> np.ndarray:
    """window.kmer.dist's `dist / colSums(dist)` (kmer_spans.R:116) with R's
    recycling: the column-major elements are divided by colSums repeated
    along them, so element [r, c] of an (n x m) matrix is divided by
    colSums[(r + c * n) % m] -- per-column normalisation only when n % m == 0
    happens to align, as R computes it."""
    dist = np.asarray(dist, dtype=np.float64)
    flat = dist.flatten(order="F")
    cs = dist.sum(axis=0)
    return (flat / np.resize(cs, flat.size)).reshape(dist.shape, order="F")


def window_kmer_dist(seq, kmers, window: int, freq: bool = True, ret_flag: int = 0, device: int = 0) -> dict:
    """window.kmer.dist: {'dist': (window + 1) x kmer_n (counts, or R's
    recycled ratios when freq), 'seq_i': int per sequence, 'scores': None or
    per sequence an int32 [len x kmer_n] matrix (None where excluded)}.
    Column j corresponds to kmers[j]."""
    kmers = [kmers] if isinstance(kmers, (str, bytes)) else list(kmers)
    kb = [x.encode() if isinstance(x, str) else bytes(x) for x in kmers]
    if len(set(len(x) for x in kb)) != 1:
        raise KmerSpansError("All kmers must be of the same size")
    k = len(kb[0])
    hs = _HostSeqs(seq)
    n = len(kb)
    window = int(window)
    if window < 0:
        raise KmerSpansError("The window size must be at least two times k")
    dist = np.zeros((n, window + 1), dtype=np.int32)
    inc = np.zeros(max(hs.n, 1), dtype=np.int32)
    kp = (C.c_char_p * n)(*kb)
    scores = None
    sp = None
    if ret_flag & 1:
        scores = [np.zeros((n, int(L)), dtype=np.int32) if L > window else None for L in hs.lens[:hs.n]]
        sp = (C.c_void_p * max(hs.n, 1))(*[host_ptr(s) for s in scores])
    check(load().ks_windowed_dist(_ctx(device), hs.ptrs, hs.lens.ctypes.data, hs.n, kp, n, k, window,
                                  int(ret_flag), dist.ctypes.data, inc.ctypes.data, sp))
    d = dist.T.copy()
    if freq:
        d = r_recycled_freq(d)
    return {"dist": d, "seq_i": inc[:hs.n].copy(),
            "scores": [s.T.copy() if s is not None else None for s in scores] if scores is not None else None}
