"""Device-resident sequences and tables (the hot path with inputs in HBM).

PyTorch is used only as the device allocator and stream provider: a genome is
one ``torch.uint8`` CUDA tensor holding the concatenated sequences plus an
int64 offsets array (host and device copies).  All compute goes through
libkmerspans.so (ks_scan_dev / ks_count_dev / ks_table_create).
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._lib import DevSeqs, Fasta, Regions, ScanStats, SpectraStats, check, load, regions_to_numpy


class SeqIndex:
    """A ks_seq_index handle: lets repeated scans of the same device-resident
    sequences reuse the previous scan's run segmentation and packed codes (see
    include/kmer_spans.h for the contract: the bytes and offsets do not change
    while the handle lives).  Holds no device memory."""

    def __init__(self, s: DevSeqs):
        self._h = C.c_void_p()
        check(load().ks_seq_index_create(C.byref(s), C.byref(self._h)))

    def _info(self) -> _lib.SeqIndexInfo:
        inf = _lib.SeqIndexInfo()
        check(load().ks_seq_index_info_get(self._h, C.byref(inf)))
        return inf

    def info(self) -> dict:
        """The index's own counters: builds, hits, layout_builds, guard_failures."""
        return self._info().as_dict(_lib.SeqIndexInfo.INDEX_FIELDS)

    def scan_info(self) -> dict:
        """What the chunked scans with this index took from the previous scan:
        chunk_reuses, hint_reuses, predictor_builds (ks_seq_index_info)."""
        return self._info().as_dict(_lib.SeqIndexInfo.SCAN_FIELDS)

    def entry_info(self) -> dict:
        """Scans that started pass 1 from the previous scan's exact chunk entries
        and verified them (entry_reuses), and calls whose verification failed
        and that were rerun on the hint path (entry_fallbacks)."""
        r, f = C.c_int64(), C.c_int64()
        check(load().ks_seq_index_entry_info(self._h, C.byref(r), C.byref(f)))
        return {"entry_reuses": int(r.value), "entry_fallbacks": int(f.value)}

    def codes_info(self) -> dict:
        """The kept per-index codes: scans that wrote them (code_builds), scans
        that streamed them instead of reading table lines (code_reuses), reading
        calls rerun on the hint path (code_fallbacks) and calls that went
        without the slot for want of memory (code_alloc_failures)."""
        v = [C.c_int64() for _ in range(4)]
        check(load().ks_seq_index_codes_info(self._h, *[C.byref(x) for x in v]))
        names = ("code_builds", "code_reuses", "code_fallbacks", "code_alloc_failures")
        return {n: int(x.value) for n, x in zip(names, v)}

    def close(self):
        if self._h:
            load().ks_seq_index_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@dataclass
class DeviceSeqs:
    seq: torch.Tensor          # uint8 [total + pad] on cuda
    offsets: np.ndarray        # int64 [nseq + 1] host
    offsets_dev: torch.Tensor  # int64 [nseq + 1] on cuda

    def seq_index(self) -> SeqIndex:
        """The sequence index of these sequences, created on first use and
        again whenever a tensor was replaced or written in place through torch
        (its version counter moved) or the host offsets changed -- so a torch
        write to ds.seq gives a new index, and the next scan recomputes."""
        key = (self.seq.data_ptr(), self.seq._version, self.offsets_dev.data_ptr(), self.offsets_dev._version,
               self.offsets.tobytes())
        if getattr(self, "_index_key", None) != key:
            old = getattr(self, "_index", None)
            if old is not None:
                old.close()
            self._index = SeqIndex(self.struct())
            self._index_key = key
        return self._index

    def __del__(self):
        try:
            ix = getattr(self, "_index", None)
            if ix is not None:
                ix.close()
        except Exception:  # (interpreter shutdown: the module globals may be gone)
            pass

    @property
    def nseq(self) -> int:
        return int(self.offsets.size - 1)

    @property
    def total(self) -> int:
        return int(self.offsets[-1])

    def struct(self) -> DevSeqs:
        s = DevSeqs()
        s.seq = self.seq.data_ptr()
        s.offsets_host = self.offsets.ctypes.data
        s.offsets_dev = self.offsets_dev.data_ptr()
        s.nseq = self.nseq
        return s

    def host_seq(self, q: int) -> bytes:
        a, b = int(self.offsets[q]), int(self.offsets[q + 1])
        return self.seq[a:b].cpu().numpy().tobytes()

    def subset(self, ids) -> "DeviceSeqs":
        """A new DeviceSeqs holding the given sequences (device copy)."""
        parts = [self.seq[int(self.offsets[q]):int(self.offsets[q + 1])] for q in ids]
        lens = [int(self.offsets[q + 1] - self.offsets[q]) for q in ids]
        return from_parts(parts, lens, self.seq.device)


def _pad16(n: int) -> int:
    return (n + 16 + 15) // 16 * 16


def from_parts(parts, lens, device) -> DeviceSeqs:
    offs = np.zeros(len(lens) + 1, dtype=np.int64)
    offs[1:] = np.cumsum(np.asarray(lens, dtype=np.int64))
    buf = torch.empty(_pad16(int(offs[-1])), dtype=torch.uint8, device=device)
    buf[int(offs[-1]):] = ord("N")
    for p, a, b in zip(parts, offs[:-1], offs[1:]):
        if b > a:
            buf[int(a):int(b)].copy_(p)
    return DeviceSeqs(buf, offs, torch.from_numpy(offs).to(device))


def from_host(seqs, device="cuda") -> DeviceSeqs:
    """Upload a list of str/bytes sequences."""
    bs = [s.encode("latin-1") if isinstance(s, str) else bytes(s) for s in seqs]
    lens = [len(b) for b in bs]
    parts = [torch.frombuffer(bytearray(b), dtype=torch.uint8) if b else torch.empty(0, dtype=torch.uint8)
             for b in bs]
    return from_parts(parts, lens, device)


class DeviceTable:
    """A score table s = w - thr on the device (ks_table)."""

    def __init__(self, ctx: _lib.Context, w, k: int, thr: float = 0.0, compress: bool = True,
                 expand: bool = False, freq: torch.Tensor | None = None):
        """freq: optional k-mer counts (int32[4^k], cuda) of the sequences to be
        scanned -- a hint for the expanded table's short codes, never the results."""
        w = np.ascontiguousarray(w, dtype=np.float64)
        if w.size != 4 ** k:
            raise _lib.KmerSpansError(f"kmer_w contains {w.size} elements but should have {4 ** k}")
        if freq is not None and (freq.dtype != torch.int32 or freq.numel() != 4 ** k or not freq.is_cuda):
            raise _lib.KmerSpansError("freq must be an int32 cuda tensor of 4^k counts")
        self.k = k
        self._h = C.c_void_p()
        flags = (1 if compress else 0) | (2 if expand else 0)
        if freq is not None:
            _order(ctx)
        check(load().ks_table_create_hint(ctx.handle, w.ctypes.data, k, float(thr), flags,
                                          C.c_void_p(freq.data_ptr()) if freq is not None else None,
                                          C.byref(self._h)))

    @classmethod
    def from_counts(cls, ctx: _lib.Context, counts: torch.Tensor, k: int, score: str, total: float = 0.0,
                    thr: float = 0.0, compress: bool = True, expand: bool = False, max_ext_bytes: int = 0,
                    w_out: torch.Tensor | None = None) -> "DeviceTable":
        """ks_table_from_counts: the log2 / pm1 / rank table of device counts
        (int32[4^k] cuda) built on the device; w_out (float64[4^k] cuda, optional)
        receives w.  total: the word count (rank only)."""
        if counts.dtype != torch.int32 or counts.numel() != 4 ** k or not counts.is_cuda:
            raise _lib.KmerSpansError("counts must be an int32 cuda tensor of 4^k counts")
        if w_out is not None and (w_out.dtype != torch.float64 or w_out.numel() != 4 ** k or not w_out.is_cuda):
            raise _lib.KmerSpansError("w_out must be a float64 cuda tensor of 4^k values")
        self = cls.__new__(cls)
        self.k = k
        self._h = C.c_void_p()
        flags = (1 if compress else 0) | (2 if expand else 0)
        _order(ctx)
        check(load().ks_table_from_counts(ctx.handle, C.c_void_p(counts.data_ptr()), int(k), _lib.SCORES[score],
                                          float(total), float(thr), flags, int(max_ext_bytes),
                                          C.c_void_p(w_out.data_ptr()) if w_out is not None else None,
                                          C.byref(self._h)))
        return self

    def info(self) -> dict:
        """ks_table_get_info: shape and setup cost (ms) of the table."""
        inf = _lib.TableInfo()
        check(load().ks_table_get_info(self._h, C.byref(inf)))
        return inf.as_dict()

    def setup_ms(self) -> dict:
        """Setup time of this table by phase (ms; host wall clock around the
        synchronised device work)."""
        inf = self.info()
        return {key[3:]: round(v, 3) for key, v in inf.items() if key.startswith("ms_")}

    @property
    def code_bits(self) -> int:
        return int(load().ks_table_code_bits(self._h))

    @property
    def escape_fraction(self) -> float:
        return float(load().ks_table_escape_fraction(self._h))

    @property
    def compressed(self) -> bool:
        return bool(load().ks_table_is_compressed(self._h))

    @property
    def positions_per_read(self) -> int:
        return int(load().ks_table_positions_per_read(self._h))

    @property
    def line_kind(self) -> int:
        """0: no line table; 1: uint16 64-B lines (k_pass1l); 2: FP64 64-B lines
        (k_pass1l); 3: 128-B lines (k_pass1w); 4: weighted-rank 128-B code lines
        for pass 1 (k_pass1r) beside FP64 64-B lines for the later passes."""
        return int(self.info()["line_kind"])

    @property
    def pass1_kernel(self) -> str:
        """The pass-1 kernel the chunked scan runs on this table."""
        lk = self.line_kind
        if self.k <= 7 and not os.environ.get("KS_NO_LDS_TABLE"):  # (scan_chunked: the table staged in LDS first)
            return "k_pass1_lds"
        if lk == 3:
            return "k_pass1w"
        if lk == 4:
            return "k_pass1r"
        if lk:
            return "k_pass1l"
        if self.positions_per_read > 1:
            return "k_pass1p" if self.compressed else "k_pass1pf"
        return "k_pass1"

    @property
    def distinct(self) -> int:
        return int(load().ks_table_distinct(self._h))

    def debug_bytes(self, part: str) -> int:
        """ks_table_debug_bytes: bytes of a part (_lib.TABLE_PARTS), 0 when the table has none."""
        return int(load().ks_table_debug_bytes(self._h, _lib.TABLE_PARTS[part][0]))

    def debug_read(self, part: str, lo: int = 0, n: int | None = None, dtype=None) -> np.ndarray:
        """ks_table_debug_read: elements [lo, lo + n) of a part (to its end by
        default) as a numpy array of the part's element type, or of dtype."""
        pid, dt = _lib.TABLE_PARTS[part]
        dt = np.dtype(dtype or dt)
        if n is None:
            n = self.debug_bytes(part) // dt.itemsize - lo
        out = np.empty(max(int(n), 1), dtype=dt)  # (a bad range is the library's error, an empty one too)
        check(load().ks_table_debug_read(self._h, pid, int(lo) * dt.itemsize, int(n) * dt.itemsize, out.ctypes.data))
        return out[:max(int(n), 0)]

    def debug_props(self) -> dict:
        """ks_table_debug_props: the flags and the raw form of the built table."""
        p = _lib.TableProps()
        check(load().ks_table_debug_props(self._h, C.byref(p)))
        return p.as_dict()

    def close(self):
        if self._h:
            load().ks_table_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def kept_codes_layout(J: int, nch: int, c: int, i: int) -> tuple[int, int]:
    """ks_kept_codes_layout: (bytes of the kept codes of nch chunks in steps of
    J, halfword offset of scan index i of chunk c).  Host arithmetic only."""
    b, h = C.c_int64(), C.c_int64()
    check(load().ks_kept_codes_layout(int(J), int(nch), int(c), int(i), C.byref(b), C.byref(h)))
    return int(b.value), int(h.value)


def kept_codes_read(ctx: _lib.Context, c0: int, nchunks: int) -> tuple[np.ndarray, int]:
    """ks_kept_codes_debug_read: the kept codes of chunks [c0, c0 + nchunks) of
    ctx's last chunked scan as uint16 [nchunks, 256] in index order, and the
    step J they were written in (tests)."""
    out = np.zeros((int(nchunks), 256), dtype=np.uint16)
    j = C.c_int32()
    check(load().ks_kept_codes_debug_read(_handle(ctx), int(c0), int(nchunks), out.ctypes.data, C.byref(j)))
    return out, int(j.value)


def _handle(ctx):
    """The ks_ctx of a Context; None is the library's default context on device 0."""
    return None if ctx is None else ctx.handle


def _ptr(t):
    """The device address of an optional tensor (None and an empty one are the C NULL)."""
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def bind_torch_stream(ctx: _lib.Context) -> None:
    """Run library work on torch's current stream (ordering with torch ops)."""
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)


def _order(ctx) -> None:
    """Make torch's pending work on the buffers we are handed visible to the
    ctx's stream: a no-op when the ctx runs on torch's current stream (see
    bind_torch_stream), otherwise a wait for torch's stream.  Every library
    call synchronises its own stream before returning, so results are ready
    for torch afterwards."""
    if ctx is None or getattr(ctx, "stream", -1) != torch.cuda.current_stream().cuda_stream:
        torch.cuda.current_stream().synchronize()


def scan(ctx: _lib.Context, ds: DeviceSeqs, k: int, table: DeviceTable, min_width: int, min_score: float,
         visits: torch.Tensor | None = None):
    """ks_scan_dev_indexed with ds's sequence index (repeated scans of one ds
    reuse its run segmentation): returns (pos int32[3, R], score float64[2, R],
    stats dict)."""
    st = ScanStats()
    r = Regions()
    s = ds.struct()
    _order(ctx)
    check(load().ks_scan_dev_indexed(ctx.handle, C.byref(s), ds.seq_index()._h, int(k), table._h, int(min_width),
                                     float(min_score),
                                     C.c_void_p(visits.data_ptr()) if visits is not None else None, C.byref(r),
                                     C.byref(st)))
    pos, score = regions_to_numpy(r)
    return pos, score, st.as_dict()


def tr_lr(ctx: _lib.Context, ds: DeviceSeqs, k: int, trans: DeviceTable, init: DeviceTable, min_length: int):
    """ks_tr_lr_dev_indexed: tr_lr regions (1-based, as tr_lr_regions_r) of
    device-resident sequences; trans / init tables with threshold 0 (init
    built with compress=False).  Returns (pos int32[3, R], score float64[2, R], stats)."""
    st = ScanStats()
    r = Regions()
    s = ds.struct()
    _order(ctx)
    check(load().ks_tr_lr_dev_indexed(ctx.handle, C.byref(s), ds.seq_index()._h, int(k), trans._h, init._h,
                                      int(min_length), C.byref(r), C.byref(st)))
    pos, score = regions_to_numpy(r)
    return pos, score, st.as_dict()


def count(ctx: _lib.Context, ds: DeviceSeqs, k: int, counts: torch.Tensor) -> float:
    """ks_count_dev: accumulates into counts (int32[4^k] cuda); returns #words."""
    n = C.c_double(0)
    s = ds.struct()
    _order(ctx)
    check(load().ks_count_dev(ctx.handle, C.byref(s), int(k), C.c_void_p(counts.data_ptr()), C.byref(n)))
    return n.value


class FastaSeqs:
    """Records of a FASTA file parsed on the device (ks_fasta_load /
    ks_fasta_parse): usable wherever a DeviceSeqs is (scan, tr_lr, count).
    The device buffers belong to the library and are freed by close()."""

    def __init__(self, f: Fasta):
        self._f = f
        n = int(f.seqs.nseq)
        self.offsets = (np.ctypeslib.as_array(C.cast(f.seqs.offsets_host, C.POINTER(C.c_int64)), shape=(n + 1,)).copy()
                        if n else np.zeros(1, dtype=np.int64))
        self.names = [f.names[q].decode("latin-1") for q in range(n)]
        self.n_records = int(f.n_records)
        self.bases_all = int(f.bases_all)
        self.bases_kept = int(f.bases_kept)
        self.ms_upload = float(f.ms_upload)
        self.ms_parse = float(f.ms_parse)
        self._index = None

    def seq_index(self) -> SeqIndex:
        """The sequence index of the records (their buffers are the library's
        and never change), created on first use."""
        if self._index is None:
            self._index = SeqIndex(self.struct())
        return self._index

    @property
    def nseq(self) -> int:
        return int(self.offsets.size - 1)

    @property
    def total(self) -> int:
        return int(self.offsets[-1])

    def struct(self) -> DevSeqs:
        if self._f is None:
            raise ValueError("FastaSeqs is closed")
        return self._f.seqs

    def host_bytes(self) -> bytes:
        """All kept records' bytes, concatenated (device -> host copy)."""
        buf = np.empty(max(self.total, 1), dtype=np.uint8)
        check(load().ks_fasta_copy_seqs(C.byref(self._f), buf.ctypes.data))
        return buf[:self.total].tobytes()

    def host_seqs(self) -> list[bytes]:
        b = self.host_bytes()
        return [b[int(a):int(e)] for a, e in zip(self.offsets[:-1], self.offsets[1:])]

    def close(self):
        if self._index is not None:
            self._index.close()
            self._index = None
        if self._f is not None:
            load().ks_fasta_free(C.byref(self._f))
            self._f = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def load_fasta(ctx: _lib.Context | None, path: str, min_len: int = 0) -> FastaSeqs:
    """ks_fasta_load: plain or gzip FASTA -> device-resident records."""
    f = Fasta()
    check(load().ks_fasta_load(_handle(ctx), str(path).encode(), int(min_len), C.byref(f)))
    return FastaSeqs(f)


def parse_fasta(ctx: _lib.Context | None, text, min_len: int = 0) -> FastaSeqs:
    """ks_fasta_parse: FASTA text (str/bytes) -> device-resident records."""
    b = text.encode("latin-1") if isinstance(text, str) else bytes(text)
    f = Fasta()
    check(load().ks_fasta_parse(_handle(ctx), b, len(b), int(min_len), C.byref(f)))
    return FastaSeqs(f)


def count_multi(ctx: _lib.Context, ds, ks, counts) -> list[float]:
    """ks_count_multi_dev: one pass for several k; counts[i] int32[4^ks[i]]
    cuda tensors (accumulated).  Returns the words counted per k."""
    ks = np.ascontiguousarray(ks, dtype=np.int32)
    ptrs = (C.c_void_p * max(len(ks), 1))(*[c.data_ptr() for c in counts])
    words = np.zeros(max(len(ks), 1), dtype=np.float64)
    s = ds.struct()
    _order(ctx)
    check(load().ks_count_multi_dev(ctx.handle, C.byref(s), ks.ctypes.data, len(ks), ptrs, words.ctypes.data))
    return [float(w) for w in words[:len(ks)]]


def windowed(ctx: _lib.Context, ds, kmer_codes, k: int, window: int, dist: torch.Tensor,
             included: torch.Tensor | None = None, scores: torch.Tensor | None = None) -> None:
    """ks_windowed_dev: dist int32 [kmer_n, window + 1] cuda (accumulated; row
    i = query i), included int32 [nseq] cuda or None, scores int32 cuda
    [kmer_n * total] (zeroed; per sequence q the [kmer_n][len_q] block at
    kmer_n * offsets[q]) or None."""
    codes = np.ascontiguousarray(kmer_codes, dtype=np.uint32)
    if dist.dtype != torch.int32 or dist.numel() != codes.size * (int(window) + 1) or not dist.is_cuda:
        raise _lib.KmerSpansError("dist must be an int32 cuda tensor of kmer_n * (window + 1)")
    if scores is not None and (scores.dtype != torch.int32 or scores.numel() < codes.size * ds.total):
        raise _lib.KmerSpansError("scores must be an int32 cuda tensor of kmer_n * total")
    if included is not None and (included.dtype != torch.int32 or included.numel() < ds.nseq):
        raise _lib.KmerSpansError("included must be an int32 cuda tensor of nseq")
    s = ds.struct()
    _order(ctx)
    check(load().ks_windowed_dev(ctx.handle, C.byref(s), codes.ctypes.data, int(codes.size), int(k), int(window),
                                 C.c_void_p(dist.data_ptr()),
                                 C.c_void_p(included.data_ptr()) if included is not None else None,
                                 C.c_void_p(scores.data_ptr()) if scores is not None else None))


def region_spectra(ctx: _lib.Context, ds, pos, q: int = 4, both_strands: bool = True, entropy: bool = True,
                   seq_base: int = 0, out: torch.Tensor | None = None):
    """ks_region_spectra_dev: the q-mer spectrum and Shannon entropy of every
    region of device-resident sequences (ds: DeviceSeqs or FastaSeqs).

    pos: the int32[3, R] array scan() / tr_lr() return (rows seq_id, beg, end;
    beg..end 1-based inclusive), as numpy (uploaded) or as an int32 CUDA tensor
    (used in place).  seq_base=1 subtracts 1 from the sequence ids (tr_lr
    regions carry 1-based ids).  Returns (counts, entropy, stats):
    counts  int32 CUDA tensor [R, 4**q] holding the library's uint32 bits
            (torch has no uint32 arithmetic; a bin above 2^31 - 1 reads
            negative -- view the host copy as np.uint32), columns in
            kmer_seq(q) order, both strands folded when both_strands;
            out= (int32 CUDA, contiguous, R * 4**q elements) is reused for it;
            every row is overwritten;
    entropy float64 CUDA tensor [R] (NaN where a row is empty), or None;
    stats   dict of ks_spectra_stats."""
    q = int(q)
    dev = ds.seq.device if hasattr(ds, "seq") else torch.device("cuda", getattr(ctx, "device", 0))
    if isinstance(pos, torch.Tensor):
        if pos.dtype != torch.int32 or not pos.is_cuda or pos.dim() != 2 or pos.shape[0] != 3:
            raise _lib.KmerSpansError("pos must be an int32 [3, R] array (numpy or cuda tensor)")
        if hasattr(ds, "seq") and pos.device != ds.seq.device:
            raise _lib.KmerSpansError(f"pos is on {pos.device}, the sequences are on {ds.seq.device}")
        p = pos.contiguous()
    else:
        a = np.asarray(pos)
        if a.ndim != 2 or a.shape[0] != 3:
            raise _lib.KmerSpansError("pos must be an int32 [3, R] array (numpy or cuda tensor)")
        p = torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
    n = int(p.shape[1])
    ids = p[0] - int(seq_base) if seq_base else p[0]
    nb = 4 ** q if 1 <= q <= _lib.KS_SPECTRA_MAX_Q else 1
    if out is not None:
        if out.dtype != torch.int32 or not out.is_cuda or not out.is_contiguous() or out.numel() != n * nb:
            raise _lib.KmerSpansError("out must be a contiguous int32 cuda tensor of R * 4^q elements")
        counts = out.view(n, nb)
    else:
        counts = torch.empty((n, nb), dtype=torch.int32, device=p.device)
    ent = torch.empty(n, dtype=torch.float64, device=p.device) if entropy else None
    st = SpectraStats()
    s = ds.struct()
    _order(ctx)
    check(load().ks_region_spectra_dev(_handle(ctx), C.byref(s), C.c_void_p(ids.data_ptr()),
                                       C.c_void_p(p[1].data_ptr()), C.c_void_p(p[2].data_ptr()), n, q,
                                       _lib.KS_SPECTRA_BOTH_STRANDS if both_strands else 0,
                                       C.c_void_p(counts.data_ptr()), _ptr(ent), C.byref(st)))
    return counts, ent, st.as_dict()


def _counts_dev(counts):
    """(device, n, ncol) of a counts tensor, which the library reads in place."""
    if (not isinstance(counts, torch.Tensor) or counts.dtype != torch.int32 or not counts.is_cuda
            or counts.dim() != 2 or not counts.is_contiguous()):
        raise _lib.KmerSpansError("counts must be a contiguous int32 [n, ncol] cuda tensor")
    return counts.device, int(counts.shape[0]), int(counts.shape[1])


def _rows_dev(rows, what, dev, n):
    """(contiguous int64 CUDA tensor or None, rows selected) of a row
    selection (numpy is uploaded): None selects n rows."""
    if rows is None:
        return None, n
    if isinstance(rows, torch.Tensor):
        if rows.dtype != torch.int64 or not rows.is_cuda or rows.dim() != 1:
            raise _lib.KmerSpansError(f"{what} must be a 1-d int64 array (numpy or cuda tensor)")
        if rows.device != dev:
            raise _lib.KmerSpansError(f"{what} is on {rows.device}, the counts are on {dev}")
        return rows.contiguous(), int(rows.numel())
    a = np.asarray(rows)
    if a.ndim != 1 or (a.size and a.dtype.kind not in "iu"):
        raise _lib.KmerSpansError(f"{what} must be a 1-d int64 array (numpy or cuda tensor)")
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(dev), int(a.size)


def _dist_dev(dist, least):
    """n >= least of a condensed distance tensor, which the library reads in place."""
    if (not isinstance(dist, torch.Tensor) or dist.dtype != torch.float64 or not dist.is_cuda or dist.dim() != 1
            or not dist.is_contiguous()):
        raise _lib.KmerSpansError("dist must be a contiguous 1-d float64 cuda tensor")
    return _lib.condensed_n(int(dist.numel()), least)


def region_distances(ctx: _lib.Context, counts: torch.Tensor, rows=None, rows_b=None, squared: bool = False,
                     out: torch.Tensor | None = None, metric: str = "euclidean"):
    """ks_spectra_dist_dev / ks_spectra_cross_dist_dev: distances between the
    row-normalised spectra of region_spectra, on the device; Euclidean unless
    metric= names "manhattan", "maximum", "canberra" or "hellinger" (as in
    api.region_distances; squared=True needs "euclidean" or "hellinger").

    counts: the int32 CUDA tensor [n, ncol] region_spectra returns (uint32
    bits), used in place.  rows / rows_b: optional selections of row indices,
    int64 CUDA tensors (used in place) or numpy (uploaded); any order, repeats
    allowed; None = all rows.  rows_b is None: the condensed form, a float64
    CUDA tensor [m(m-1)/2] over the pairs i < j of the selected rows in the
    order of R's dist object (scipy's pdist).  Otherwise the dense [na, nb]
    block of rows against rows_b.  squared=True skips the square root.  out=
    (float64 CUDA, contiguous, as many elements) is reused for the result.
    Returns (distances, stats dict of ks_dist_stats)."""
    dev, n, ncol = _counts_dev(counts)
    ra, na = _rows_dev(rows, "rows", dev, n)
    rb, nb = _rows_dev(rows_b, "rows_b", dev, 0)
    if rb is None:
        shape = (na * (na - 1) // 2 if na > 1 else 0,)
    else:
        shape = (na, nb)
    numel = int(np.prod(shape, dtype=np.int64))
    if out is not None:
        if out.dtype != torch.float64 or not out.is_cuda or not out.is_contiguous() or out.numel() != numel:
            raise _lib.KmerSpansError(f"out must be a contiguous float64 cuda tensor of {numel} elements")
        if out.device != dev:
            raise _lib.KmerSpansError(f"out is on {out.device}, the counts are on {dev}")
        res = out.view(shape)
    else:
        res = torch.empty(shape, dtype=torch.float64, device=dev)
    st = _lib.DistStats()
    flags = _lib.dist_flags(metric, squared)
    _order(ctx)
    if rb is None:
        check(load().ks_spectra_dist_dev(_handle(ctx), C.c_void_p(counts.data_ptr()), n, ncol, _ptr(ra), na, flags,
                                         _ptr(res), C.byref(st)))
    else:
        check(load().ks_spectra_cross_dist_dev(_handle(ctx), C.c_void_p(counts.data_ptr()), n, ncol, _ptr(ra), na,
                                               _ptr(rb), nb, flags, _ptr(res), C.byref(st)))
    return res, st.as_dict()


def region_hclust(ctx: _lib.Context, dist: torch.Tensor, method: str = "complete", keep_input: bool = True):
    """ks_hclust_dev: agglomerative clustering (R's hclust) of the condensed
    distances region_distances returns, on the device.

    dist: a contiguous float64 CUDA tensor of n(n-1)/2 entries, n >= 2, every
    entry finite (a NaN from an empty spectrum row is an error naming its
    offset; the tensor is untouched then).  method: "complete" (R's default),
    "single" or "average".  keep_input=True clusters a device copy and leaves
    dist's bits unchanged; keep_input=False updates dist in place and consumes
    it.  Returns (tree, stats): tree is a dict of merge int32 [n-1, 2], height
    float64 [n-1], order int32 [n] (numpy, as R's hclust object: observation i
    is -(i+1), step t is t+1, order is 1-based) and method; stats the dict of
    ks_hclust_stats."""
    n = _dist_dev(dist, 2)
    merge, height, order = _lib.hclust_outputs(n)
    st = _lib.HclustStats()
    _order(ctx)
    check(load().ks_hclust_dev(_handle(ctx), C.c_void_p(dist.data_ptr()), n,
                               _lib.hclust_method(method), _lib.KS_HCLUST_KEEP_INPUT if keep_input else 0,
                               merge.ctypes.data, height.ctypes.data, order.ctypes.data, C.byref(st)))
    return {"merge": merge, "height": height, "order": order, "method": method}, st.as_dict()


def region_nj(ctx: _lib.Context, dist: torch.Tensor, keep_input: bool = True, compact: bool = True):
    """ks_nj_dev: the neighbour-joining tree (ape's nj, test.R:770-775) of the
    condensed distances region_distances returns, on the device.

    dist: a contiguous float64 CUDA tensor of n(n-1)/2 entries, n >= 3, every
    entry finite (a NaN from an empty spectrum row is an error naming its
    offset; the tensor is untouched then).  keep_input=True joins a device copy
    and leaves dist's bits unchanged; keep_input=False updates dist in place
    and consumes it.  compact=False keeps the matrix at n rows throughout (the
    same tree; for measurements).  Returns (tree, stats): tree is a dict of
    join int32 [n-3, 2], length float64 [n-3, 2], root int32 [3] and
    root_length float64 [3] (numpy; observation i is -(i+1), the node of step t
    is t+1); stats the dict of ks_nj_stats."""
    n = _dist_dev(dist, 3)
    join, length, root, root_length = _lib.nj_outputs(n)
    st = _lib.NjStats()
    flags = (_lib.KS_NJ_KEEP_INPUT if keep_input else 0) | (0 if compact else _lib.KS_NJ_NO_COMPACT)
    _order(ctx)
    check(load().ks_nj_dev(_handle(ctx), C.c_void_p(dist.data_ptr()), n, flags, join.ctypes.data, length.ctypes.data,
                           root.ctypes.data, root_length.ctypes.data, C.byref(st)))
    return {"join": join, "length": length, "root": root, "root_length": root_length}, st.as_dict()


def region_silhouette(ctx: _lib.Context, dist: torch.Tensor, group, ngroups=None, sums: bool = False):
    """ks_silhouette_dev: silhouette widths (R's cluster::silhouette), medoids
    and diameters of the groups of cut_tree, from the condensed distances
    region_distances returns, on the device.

    dist: a contiguous float64 CUDA tensor of n(n-1)/2 entries, n >= 2, every
    entry finite (a NaN from an empty spectrum row is an error naming its
    offset); it is only read.  group: n integer labels in 1 .. ngroups as
    cut_tree returns them, a numpy array or a tensor (a CUDA tensor is
    downloaded, 4 n bytes); ngroups defaults to the largest label, groups
    without members are allowed, at least two must have some.  Returns (res,
    stats): res is a dict of numpy arrays 'width', 'a', 'b' float64 [n],
    'neighbor' int32 [n], 'size', 'medoid' int32 [g], 'diameter', 'avg_width'
    float64 [g] (medoid -1 and NaN for an empty group) and the float
    'avg_width_all'; with sums=True also 'sums', a float64 CUDA tensor [n, g]
    of the group sums S(i, c) (include/kmer_spans.h has the order of every
    addition).  stats is the dict of ks_silhouette_stats."""
    n = _dist_dev(dist, 2)
    if isinstance(group, torch.Tensor):
        group = group.detach().cpu().numpy()
    g, ng = _lib.silhouette_group(group, n, ngroups)
    res = _lib.silhouette_outputs(n, ng)
    s = torch.empty((n, ng), dtype=torch.float64, device=dist.device) if sums else None
    st = _lib.SilhouetteStats()
    _order(ctx)
    check(load().ks_silhouette_dev(_handle(ctx), C.c_void_p(dist.data_ptr()), n, g.ctypes.data, ng, 0,
                                   *_lib.silhouette_out_args(res), _ptr(s), C.byref(st)))
    res["avg_width_all"] = float(res["avg_width_all"][0])
    if sums:
        res["sums"] = s
    return res, st.as_dict()


def region_pca(ctx: _lib.Context, counts: torch.Tensor, rows=None, center: bool = True, ncomp=None,
               scores: bool = True, gram: bool = False):
    """ks_spectra_pca_dev: principal components (R's prcomp, test.R:734-736,
    :811) of the row-normalised spectra of region_spectra, on the device.

    counts: the int32 CUDA tensor [n, ncol] region_spectra returns (uint32
    bits), used in place; 1 <= ncol <= 1024.  rows: an optional selection of
    row indices, an int64 CUDA tensor (used in place) or numpy (uploaded); any
    order, repeats allowed, at least 2; None = all rows.  A selected row
    without counts or a bad index is an error naming its position, and nothing
    is written then.  center=False is prcomp's center=FALSE.  ncomp: components
    kept (default ncol).  Returns (res, stats): res is a dict of float64 CUDA
    tensors 'sdev' [ncol], 'rotation' [ncol, ncomp], 'center' [ncol], 'x'
    [m, ncomp] (None with scores=False) and, with gram=True, 'G' [ncol, ncol],
    the cross-product matrix of the (centred) profiles; stats the dict of
    ks_pca_stats."""
    dev, n, ncol = _counts_dev(counts)
    r, m = _rows_dev(rows, "rows", dev, n)
    k = ncol if ncomp is None else int(ncomp)
    kk = max(0, min(k, ncol))  # a bad ncomp is the library's error; the buffers only need a size
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)  # noqa: E731
    res = {"sdev": new(ncol), "rotation": new(ncol, kk), "center": new(ncol), "x": new(m, kk) if scores else None}
    if gram:
        res["G"] = new(ncol, ncol)
    st = _lib.PcaStats()
    _order(ctx)
    check(load().ks_spectra_pca_dev(_handle(ctx), C.c_void_p(counts.data_ptr()), n, ncol, _ptr(r), m,
                                    0 if center else _lib.KS_PCA_NO_CENTER, k, _ptr(res["center"]), _ptr(res["sdev"]),
                                    _ptr(res["rotation"]), _ptr(res["x"]), _ptr(res.get("G")), C.byref(st)))
    return res, st.as_dict()


def region_kmeans(ctx: _lib.Context, counts: torch.Tensor, centers, rows=None, iter_max: int = 10):
    """ks_spectra_kmeans_dev: R's kmeans(x, centers, iter.max, algorithm="Lloyd")
    on the row-normalised spectra of region_spectra, on the device and without
    any distance matrix (memory O((m + g) ncol)).

    counts: the int32 CUDA tensor [n, ncol] region_spectra returns (uint32
    bits), used in place; 1 <= ncol <= 4096.  rows: an optional selection of
    row indices, an int64 CUDA tensor (used in place) or numpy (uploaded); any
    order, repeats allowed; None = all rows.  centers: a float64 [g, ncol]
    matrix of finite initial centres (a CUDA tensor, read only, or numpy), or a
    1-d integer sequence or tensor of g positions into the selection whose
    profiles start the run.  A selected row without counts, a bad index or a
    non-finite centre is an error naming its position, and nothing is written
    then.  Returns (res, stats): res is a dict of 'cluster' (int32 CUDA tensor
    [m], labels 1 .. g), 'centers' (float64 CUDA tensor [g, ncol]), 'size'
    (int32 numpy [g]), 'withinss' (float64 numpy [g]) and the scalars
    'tot_withinss', 'totss', 'betweenss', 'iter', 'converged'; stats the dict
    of ks_kmeans_stats.  include/kmer_spans.h has the order of every
    operation; one 4-byte read-back per pass is the only host round trip."""
    dev, n, ncol = _counts_dev(counts)
    r, m = _rows_dev(rows, "rows", dev, n)
    init = init_rows = None
    if isinstance(centers, torch.Tensor) and centers.dim() == 2:
        if centers.dtype != torch.float64 or centers.shape[1] != ncol or not centers.shape[0]:
            raise _lib.KmerSpansError(f"a centers tensor must be float64 [g, {ncol}]")
        init = centers.to(dev).contiguous()
        g = int(init.shape[0])
    elif isinstance(centers, torch.Tensor):
        init_rows, g = _rows_dev(centers, "centers", dev, 0)
        if not g:
            raise _lib.KmerSpansError("centers names no row")
    else:
        hi, hr, g = _lib.kmeans_centers(centers, ncol)
        if hi is not None:
            init = torch.from_numpy(hi).to(dev)
        else:
            init_rows = torch.from_numpy(hr).to(dev)
    cluster = torch.empty(m, dtype=torch.int32, device=dev)
    cen = torch.empty((g, ncol), dtype=torch.float64, device=dev)
    size, wss = np.zeros(g, dtype=np.int32), np.zeros(g, dtype=np.float64)
    out, st = _lib.KmeansResult(), _lib.KmeansStats()
    _order(ctx)
    check(load().ks_spectra_kmeans_dev(_handle(ctx), C.c_void_p(counts.data_ptr()), n, ncol, _ptr(r), m, _ptr(init),
                                       _ptr(init_rows), g, int(iter_max), 0, _ptr(cluster), _ptr(cen),
                                       size.ctypes.data, wss.ctypes.data, C.byref(out), C.byref(st)))
    res = dict({"cluster": cluster, "centers": cen, "size": size, "withinss": wss}, **_lib.kmeans_result(out))
    return res, st.as_dict()


def region_group_means(ctx: _lib.Context, counts: torch.Tensor, group, ngroups=None, rows=None):
    """ks_spectra_group_means_dev: the mean spectrum, size and within sum of
    squares of every group of a labelling (for instance cut_tree's) of the
    row-normalised spectra, on the device: the bridge from a tree cut to
    region_kmeans.

    counts, rows: as for region_kmeans.  group: one integer label in 1 ..
    ngroups per selected row, a numpy array or a tensor (a CUDA tensor is
    downloaded, 4 m bytes); ngroups defaults to the largest label; groups
    without members are allowed.  Returns (res, stats): res is a dict of
    'centers' (float64 CUDA tensor [g, ncol], a row of NaN for an empty group),
    'size' (int32 numpy [g]) and 'withinss' (float64 numpy [g]); stats the dict
    of ks_kmeans_stats."""
    dev, n, ncol = _counts_dev(counts)
    r, m = _rows_dev(rows, "rows", dev, n)
    if isinstance(group, torch.Tensor):
        group = group.detach().cpu().numpy()
    g, ng = _lib.silhouette_group(group, m, ngroups)
    ngb = min(ng, _lib.KS_KM_MAX_GROUPS)  # a larger ngroups is the library's error; the buffers only need a size
    cen = torch.empty((ngb, ncol), dtype=torch.float64, device=dev)
    size, wss = np.zeros(ngb, dtype=np.int32), np.zeros(ngb, dtype=np.float64)
    st = _lib.KmeansStats()
    _order(ctx)
    check(load().ks_spectra_group_means_dev(_handle(ctx), C.c_void_p(counts.data_ptr()), n, ncol, _ptr(r), m,
                                            g.ctypes.data, ng, 0, C.c_void_p(cen.data_ptr()), size.ctypes.data,
                                            wss.ctypes.data, C.byref(st)))
    return {"centers": cen, "size": size, "withinss": wss}, st.as_dict()


def region_kmeans_seed(ctx: _lib.Context, counts: torch.Tensor, g, method: str = "maximin", rows=None, first=0,
                       u=None, seed=None):
    """ks_spectra_kmeans_seed_dev: g rows of the selection to start
    region_kmeans from, by maximin (farthest-first) or k-means++ (D^2
    sampling), on the device in O(m ncol) memory.

    counts, rows: as for region_kmeans.  g, method, first, u, seed: as for
    api.region_kmeans_seed (u is a host array: the library reads it before any
    device call).  A selected row without counts or a bad index is an error
    naming its position, and nothing is written then.  Returns (res, stats):
    res is a dict of 'rows' (int64 CUDA tensor [g], positions into the
    selection: region_kmeans(ctx, counts, centers=res['rows'], rows=rows)),
    'nearest' (int32 CUDA tensor [m]), 'mindist' (float64 CUDA tensor [m],
    squared), 'pick_dist' and 'potential' (float64 numpy [g]) and the scalars
    'n_distinct', 'potential_final', 'radius', 'far_row'; stats the dict of
    ks_seed_stats.  The g steps are queued without a host round trip."""
    dev, n, ncol = _counts_dev(counts)
    r, m = _rows_dev(rows, "rows", dev, n)
    g, gb, flags, first, u = _lib.seed_args(g, method, first, u, seed)
    picked = torch.empty(gb, dtype=torch.int64, device=dev)
    near = torch.empty(m, dtype=torch.int32, device=dev)
    mind = torch.empty(m, dtype=torch.float64, device=dev)
    pd, pot = np.zeros(gb, dtype=np.float64), np.zeros(gb, dtype=np.float64)
    out, st = _lib.SeedResult(), _lib.SeedStats()
    _order(ctx)
    check(load().ks_spectra_kmeans_seed_dev(_handle(ctx), C.c_void_p(counts.data_ptr()), n, ncol, _ptr(r), m, g, flags,
                                            first, _lib.host_ptr(u), _ptr(picked), _ptr(near), _ptr(mind),
                                            pd.ctypes.data, pot.ctypes.data, C.byref(out), C.byref(st)))
    res = dict({"rows": picked, "nearest": near, "mindist": mind, "pick_dist": pd, "potential": pot},
               **_lib.seed_result(out))
    return res, st.as_dict()


def region_knn(ctx: _lib.Context, counts: torch.Tensor, k, rows=None, rows_b=None, squared: bool = False,
               metric: str = "euclidean"):
    """ks_spectra_knn_dev: the k nearest rows of a candidate selection for
    every selected row of the spectra of region_spectra, on the device and
    without any distance matrix (memory: the profile panel plus O(na k)).

    counts: the int32 CUDA tensor [n, ncol] region_spectra returns (uint32
    bits), used in place; 1 <= ncol <= 4096.  rows (the queries) / rows_b (the
    candidates): optional selections of row indices, int64 CUDA tensors (used
    in place) or numpy (uploaded); any order, repeats allowed.  rows None = all
    rows.  rows_b None is the self form: the candidates are the queries and
    position s is left out of its own list (by position, not by row index).
    1 <= k <= 64, at most the number of candidates.  A selected row without
    counts, a bad index or a k above the candidates is an error, and nothing is
    written then.  Returns (index, dist, stats): an int64 CUDA tensor [na, k]
    of positions into the candidate selection, a float64 CUDA tensor [na, k]
    (the squared sum with squared=True, otherwise its root), column 0 the
    nearest, ordered by (squared distance, position); stats the dict of
    ks_knn_stats.  metric= as in region_distances: "manhattan", "maximum" and
    "canberra" rank by the distance itself, "hellinger" by the squared
    Euclidean distance of the rooted profiles; every returned distance has the
    bits region_distances gives for that pair."""
    dev, n, ncol = _counts_dev(counts)
    ra, na = _rows_dev(rows, "rows", dev, n)
    rb, nb = _rows_dev(rows_b, "rows_b", dev, 0)
    if rb is not None and not nb:
        raise _lib.KmerSpansError("rows_b names no row")
    k, kb = _lib.knn_k(k)
    flags = _lib.dist_flags(metric, squared)
    index = torch.empty((na, kb), dtype=torch.int64, device=dev)
    dist = torch.empty((na, kb), dtype=torch.float64, device=dev)
    st = _lib.KnnStats()
    _order(ctx)
    check(load().ks_spectra_knn_dev(_handle(ctx), C.c_void_p(counts.data_ptr()), n, ncol, _ptr(ra), na, _ptr(rb), nb,
                                    k, flags, C.c_void_p(index.data_ptr()),
                                    C.c_void_p(dist.data_ptr()), C.byref(st)))
    return index, dist, st.as_dict()
