"""ctypes binding of libkmerspans.so (the C ABI in include/kmer_spans.h).

The shared library is built in-tree by ``__graft_entry__.build()``
(kmer_spans_amd/csrc/Makefile).  There is no fallback: importing this module
without the library raises, so a missing build can never silently turn into
a CPU path.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# KS_LIB_PATH: an alternative build of the same library (kernel-variant
# experiments); the in-tree build is the default.
LIB_PATH = os.environ.get("KS_LIB_PATH") or os.path.join(_HERE, "libkmerspans.so")

KS_OK = 0
KS_MAX_K = 15


class KmerSpansError(RuntimeError):
    """An error reported by libkmerspans (the reference's error() strings)."""


class Regions(C.Structure):
    _fields_ = [("n", C.c_int64), ("seq_id", C.POINTER(C.c_int32)), ("beg", C.POINTER(C.c_int32)),
                ("end", C.POINTER(C.c_int32)), ("score", C.POINTER(C.c_double))]


class DevSeqs(C.Structure):
    _fields_ = [("seq", C.c_void_p), ("offsets_host", C.c_void_p), ("offsets_dev", C.c_void_p),
                ("nseq", C.c_int32)]


class Stats(C.Structure):
    """Base of the statistics blocks the library fills in: a subclass gives
    only its _fields_ (the header's, in order)."""

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class ScanStats(Stats):
    _fields_ = [("ms_total", C.c_double), ("ms_runs", C.c_double), ("ms_scan", C.c_double),
                ("ms_rescan", C.c_double), ("ms_finish", C.c_double), ("n_bases", C.c_int64),
                ("n_scored", C.c_int64), ("n_runs", C.c_int64), ("n_regions", C.c_int64),
                ("n_rescan", C.c_int64), ("scan_algo", C.c_int32),
                ("n_replay", C.c_int64), ("ms_layout", C.c_double), ("ms_predict", C.c_double),
                ("ms_carry", C.c_double), ("ms_stitch", C.c_double)]


class SeqIndexInfo(C.Structure):
    _fields_ = [("builds", C.c_int64), ("hits", C.c_int64), ("layout_builds", C.c_int64),
                ("guard_failures", C.c_int64), ("chunk_reuses", C.c_int64), ("hint_reuses", C.c_int64),
                ("predictor_builds", C.c_int64)]
    INDEX_FIELDS = ("builds", "hits", "layout_builds", "guard_failures")
    SCAN_FIELDS = ("chunk_reuses", "hint_reuses", "predictor_builds")

    def as_dict(self, fields=None):
        return {f: int(getattr(self, f)) for f in (fields or [f for f, _ in self._fields_])}


class TableInfo(Stats):
    _fields_ = [("k", C.c_int32), ("compressed", C.c_int32), ("positions_per_read", C.c_int32),
                ("code_bits", C.c_int32), ("distinct", C.c_int64), ("ext_bytes", C.c_int64),
                ("escape_fraction", C.c_double), ("ms_upload", C.c_double), ("ms_compress", C.c_double),
                ("ms_codes12", C.c_double), ("ms_ext_alloc", C.c_double), ("ms_ext_build", C.c_double),
                ("ms_total", C.c_double), ("line_kind", C.c_int32), ("line_own", C.c_int32)]


class TableProps(Stats):
    _fields_ = [("int_exact", C.c_int32), ("no_nan_posinf", C.c_int32), ("max_abs", C.c_double),
                ("ext_J", C.c_int32), ("ext_bits", C.c_int32), ("line_kind", C.c_int32), ("line_own", C.c_int32),
                ("approx_k", C.c_int32), ("n_rpieces", C.c_int32)]


# KS_TABLE_PART_* of ks_table_debug_bytes / ks_table_debug_read, with the element type of each part
TABLE_PARTS = {"vals": (0, np.float64), "codes": (1, np.uint16), "lut": (2, np.float64), "ext": (3, np.uint8),
               "rlines": (4, np.uint32), "rpieces": (5, np.uint64), "lut12": (6, np.float64),
               "map12": (7, np.uint16), "approx": (8, np.uint16)}


class SpectraStats(Stats):
    _fields_ = [("ms_total", C.c_double), ("ms_plan", C.c_double), ("ms_count", C.c_double),
                ("ms_entropy", C.c_double), ("n_regions", C.c_int64), ("n_bases", C.c_int64),
                ("n_words", C.c_int64), ("n_tiles", C.c_int64)]


class DistStats(Stats):
    _fields_ = [("ms_total", C.c_double), ("ms_normalise", C.c_double), ("ms_distance", C.c_double),
                ("n_pairs", C.c_int64), ("bytes_written", C.c_int64), ("panel_bytes", C.c_int64)]


class HclustStats(Stats):
    _fields_ = [("ms_total", C.c_double), ("ms_check", C.c_double), ("ms_init", C.c_double),
                ("ms_merge", C.c_double), ("n", C.c_int64), ("n_rescans", C.c_int64), ("work_bytes", C.c_int64)]


class NjStats(Stats):
    _fields_ = [("ms_total", C.c_double), ("ms_check", C.c_double), ("ms_init", C.c_double),
                ("ms_join", C.c_double), ("n", C.c_int64), ("n_compactions", C.c_int64), ("work_bytes", C.c_int64)]


class SilhouetteStats(Stats):
    _fields_ = [("ms_total", C.c_double), ("ms_check", C.c_double), ("ms_sums", C.c_double),
                ("ms_widths", C.c_double), ("n", C.c_int64), ("ngroups", C.c_int64), ("n_chunks", C.c_int64),
                ("work_bytes", C.c_int64)]


class PcaStats(Stats):
    _fields_ = [("ms_total", C.c_double), ("ms_normalise", C.c_double), ("ms_gram", C.c_double),
                ("ms_eigen", C.c_double), ("ms_project", C.c_double), ("n_sweeps", C.c_int64),
                ("n_rotations", C.c_int64), ("panel_bytes", C.c_int64)]


class KmeansStats(Stats):
    _fields_ = [("ms_total", C.c_double), ("ms_normalise", C.c_double), ("ms_assign", C.c_double),
                ("ms_update", C.c_double), ("ms_wss", C.c_double), ("n_iter", C.c_int64),
                ("panel_bytes", C.c_int64), ("work_bytes", C.c_int64)]


class KnnStats(Stats):
    _fields_ = [("ms_total", C.c_double), ("ms_normalise", C.c_double), ("ms_select", C.c_double),
                ("ms_merge", C.c_double), ("n_splits", C.c_int64), ("tiles_per_split", C.c_int64),
                ("panel_bytes", C.c_int64), ("work_bytes", C.c_int64)]


class KmeansResult(C.Structure):
    _fields_ = [("iter", C.c_int32), ("converged", C.c_int32), ("tot_withinss", C.c_double), ("totss", C.c_double)]


class SeedResult(C.Structure):
    _fields_ = [("n_distinct", C.c_int32), ("reserved", C.c_int32), ("potential", C.c_double),
                ("radius", C.c_double), ("far_row", C.c_int64)]


class SeedStats(Stats):
    _fields_ = [("ms_total", C.c_double), ("ms_normalise", C.c_double), ("ms_steps", C.c_double),
                ("n_launches", C.c_int64), ("panel_bytes", C.c_int64), ("work_bytes", C.c_int64)]


class Fasta(C.Structure):
    _fields_ = [("seqs", DevSeqs), ("names", C.POINTER(C.c_char_p)), ("n_records", C.c_int64),
                ("bases_all", C.c_int64), ("bases_kept", C.c_int64), ("device", C.c_int32),
                ("ms_upload", C.c_double), ("ms_parse", C.c_double)]


class CountFile(C.Structure):
    _fields_ = [("valid", C.c_int32), ("nk", C.c_int32), ("k", C.POINTER(C.c_int32)),
                ("lens", C.POINTER(C.c_int64)), ("counts", C.POINTER(C.POINTER(C.c_int32)))]


class KmerFileInfo(C.Structure):
    _fields_ = [("written", C.c_int32), ("seq_size", C.c_double), ("seq_fsize", C.c_double),
                ("seq_fl", C.c_double), ("out_path", C.c_char * 4096), ("message", C.c_char * 512)]


KS_SPECTRA_MAX_Q = 6
KS_SPECTRA_BOTH_STRANDS = 1
KS_DIST_MAX_NCOL = 4096
KS_DIST_SQUARED = 1
KS_DIST_METRIC_MASK = 0xf00
KS_DIST_EUCLIDEAN = 0x000
KS_DIST_MANHATTAN = 0x100
KS_DIST_MAXIMUM = 0x200
KS_DIST_CANBERRA = 0x300
KS_DIST_HELLINGER = 0x400
DIST_METRICS = {"euclidean": KS_DIST_EUCLIDEAN, "manhattan": KS_DIST_MANHATTAN, "maximum": KS_DIST_MAXIMUM,
                "canberra": KS_DIST_CANBERRA, "hellinger": KS_DIST_HELLINGER}
HCLUST_METHODS = {"complete": 0, "single": 1, "average": 2}  # KS_HCLUST_*
KS_HCLUST_KEEP_INPUT = 1
KS_NJ_KEEP_INPUT = 1
KS_NJ_NO_COMPACT = 2
KS_SIL_CHUNK = 256
KS_PCA_MAX_NCOL = 1024
KS_PCA_MAX_SWEEPS = 64
KS_PCA_NO_CENTER = 1
KS_KM_CHUNK = 256
KS_KM_MAX_GROUPS = 65536
KS_KNN_MAX_K = 64
SEED_METHODS = {"maximin": 0, "kmeans++": 1}  # KS_SEED_MAXIMIN, KS_SEED_DSQ

SCORES = {"log2": 1, "pm1": 2, "rank": 3}  # KS_SCORE_* of ks_table_from_counts

# The C ABI: name -> (argtypes, restype) of every function include/kmer_spans.h
# declares.  Written by hand; tests/test_bindings.py parses the header and
# compares the arity and the kind of every parameter and return value.  A
# pointer of any type is P (a numpy address, a data_ptr(), a byref()).
P, I32, I64, D = C.c_void_p, C.c_int32, C.c_int64, C.c_double
SIGNATURES = {
    "ks_last_error": ([], C.c_char_p),
    "ks_version": ([], C.c_char_p),
    "ks_regions_free": ([P], None),
    "ks_ctx_create": ([I32, P], I32),
    "ks_ctx_destroy": ([P], None),
    "ks_ctx_set_stream": ([P, P], I32),
    "ks_default_ctx": ([], P),
    "ks_ctx_set_scan_algo": ([P, I32], I32),
    "ks_kmer_counts": ([P, P, P, I32, I32, P, P], I32),
    "ks_kmer_regions": ([P, P, P, I32, I32, P, I64, I32, D, P, P, P], I32),
    "ks_low_comp_regions": ([P, P, P, I32, I32, I32, D, D, P, P, P, P], I32),
    "ks_kmer_seq": ([I32, P, C.c_size_t], I32),
    "ks_rank_table": ([P, I32, D, P], I32),
    "ks_log2_table": ([P, I32, P], I32),
    "ks_pm1_table": ([P, I32, P], I32),
    "ks_table_create": ([P, P, I32, D, I32, P], I32),
    "ks_table_destroy": ([P], None),
    "ks_table_is_compressed": ([P], I32),
    "ks_table_distinct": ([P], I64),
    "ks_table_positions_per_read": ([P], I32),
    "ks_table_create_hint": ([P, P, I32, D, I32, P, P], I32),
    "ks_table_code_bits": ([P], I32),
    "ks_table_escape_fraction": ([P], D),
    "ks_table_get_info": ([P, P], I32),
    "ks_table_debug_bytes": ([P, I32], I64),
    "ks_table_debug_read": ([P, I32, I64, I64, P], I32),
    "ks_table_debug_props": ([P, P], I32),
    "ks_scan_dev": ([P, P, I32, P, I32, D, P, P, P], I32),
    "ks_count_dev": ([P, P, I32, P, P], I32),
    "ks_tr_lr_regions": ([P, P, P, I32, I32, I32, P, P, P, I64, P, P], I32),
    "ks_tr_lr_dev": ([P, P, I32, P, P, I32, P, P], I32),
    "ks_fasta_load": ([P, C.c_char_p, I64, P], I32),
    "ks_fasta_parse": ([P, C.c_char_p, I64, I64, P], I32),
    "ks_fasta_copy_seqs": ([P, P], I32),
    "ks_fasta_free": ([P], None),
    "ks_count_multi_dev": ([P, P, P, I32, P, P], I32),
    "ks_count_file_write": ([C.c_char_p, I32, I32, P, P], I32),
    "ks_count_file_read": ([C.c_char_p, I32, P], I32),
    "ks_count_file_free": ([P], None),
    "ks_kmers_to_file": ([P, C.c_char_p, C.c_char_p, P, I32, D, I32, P], I32),
    "ks_windowed_dist": ([P, P, P, I32, P, I32, I32, I32, I32, P, P, P], I32),
    "ks_windowed_dev": ([P, P, P, I32, I32, I32, P, P, P], I32),
    "ks_table_from_counts": ([P, P, I32, I32, D, D, I32, I64, P, P], I32),
    "ks_release_cache": ([], None),
    "ks_set_fork_broker": ([I32], I32),
    "ks_set_host_cache": ([I32], I32),
    "ks_set_devices": ([P, I32], I32),
    "ks_set_host_cache_idle": ([D], I32),
    "ks_get_devices": ([P, I32], I32),
    "ks_shard_plan": ([P, P, I32, I32, P, I64], I64),
    "ks_merge_parts": ([P, I64, I32, P, P], I32),
    "ks_multi_last_stats": ([P, I32], I32),
    "ks_region_spectra": ([P, P, P, I32, P, P, P, I64, I32, I32, P, P], I32),
    "ks_region_spectra_dev": ([P, P, P, P, P, I64, I32, I32, P, P, P], I32),
    "ks_spectra_tile_bases": ([], I32),
    "ks_spectra_dist": ([P, P, I64, I32, P, I64, I32, P], I32),
    "ks_spectra_dist_dev": ([P, P, I64, I32, P, I64, I32, P, P], I32),
    "ks_spectra_cross_dist": ([P, P, I64, I32, P, I64, P, I64, I32, P], I32),
    "ks_spectra_cross_dist_dev": ([P, P, I64, I32, P, I64, P, I64, I32, P, P], I32),
    "ks_dist_pair_offsets": ([P, P, I64, I64, P], None),
    "ks_dist_tiles_of": ([P, I64, I64, P, P], None),
    "ks_dist_tile_rows": ([], I32),
    "ks_hclust": ([P, P, I64, I32, P, P, P], I32),
    "ks_hclust_dev": ([P, P, I64, I32, I32, P, P, P, P], I32),
    "ks_hclust_cut": ([P, P, I64, I32, D, P], I32),
    "ks_nj": ([P, P, I64, P, P, P, P], I32),
    "ks_nj_dev": ([P, P, I64, I32, P, P, P, P, P], I32),
    "ks_nj_edges": ([P, P, P, P, I64, P, P], I32),
    "ks_silhouette": ([P, P, I64, P, I32, I32, P, P, P, P, P, P, P, P, P, P], I32),
    "ks_silhouette_dev": ([P, P, I64, P, I32, I32, P, P, P, P, P, P, P, P, P, P, P], I32),
    "ks_spectra_pca": ([P, P, I64, I32, P, I64, I32, I32, P, P, P, P, P], I32),
    "ks_spectra_pca_dev": ([P, P, I64, I32, P, I64, I32, I32, P, P, P, P, P, P], I32),
    "ks_pca_round_pairs": ([I32, I32, P, P], I32),
    "ks_spectra_kmeans": ([P, P, I64, I32, P, I64, P, P, I32, I32, I32, P, P, P, P, P], I32),
    "ks_spectra_kmeans_dev": ([P, P, I64, I32, P, I64, P, P, I32, I32, I32, P, P, P, P, P, P], I32),
    "ks_spectra_group_means": ([P, P, I64, I32, P, I64, P, I32, I32, P, P, P], I32),
    "ks_spectra_group_means_dev": ([P, P, I64, I32, P, I64, P, I32, I32, P, P, P, P], I32),
    "ks_spectra_kmeans_seed": ([P, P, I64, I32, P, I64, I32, I32, I64, P, P, P, P, P, P, P], I32),
    "ks_spectra_kmeans_seed_dev": ([P, P, I64, I32, P, I64, I32, I32, I64, P, P, P, P, P, P, P, P], I32),
    "ks_spectra_knn": ([P, P, I64, I32, P, I64, P, I64, I32, I32, P, P], I32),
    "ks_spectra_knn_dev": ([P, P, I64, I32, P, I64, P, I64, I32, I32, P, P, P], I32),
    "ks_seq_index_create": ([P, P], I32),
    "ks_seq_index_destroy": ([P], None),
    "ks_seq_index_info_get": ([P, P], I32),
    "ks_seq_index_entry_info": ([P, P, P], I32),
    "ks_seq_index_codes_info": ([P, P, P, P, P], I32),
    "ks_kept_codes_layout": ([I32, I64, I64, I32, P, P], I32),
    "ks_kept_codes_debug_read": ([P, I64, I64, P, P], I32),
    "ks_scan_dev_indexed": ([P, P, P, I32, P, I32, D, P, P, P], I32),
    "ks_tr_lr_dev_indexed": ([P, P, P, I32, P, P, I32, P, P], I32),
    "ks_scan_chunk_indices": ([], I32),
    "ks_scan_tile_chunks": ([], I32),
}
EXPORTS = list(SIGNATURES)

_lib = None


def _type_library(L, table=SIGNATURES):
    """Set argtypes and restype of every table entry L has.  A name L lacks is
    skipped (KS_LIB_PATH may name an earlier build, for A/B runs, without a
    newer symbol); calling it fails at the call."""
    for name, (args, res) in table.items():
        f = getattr(L, name, None)
        if f is not None:
            f.argtypes, f.restype = args, res


def load():
    """Load and type the library (raises if it is missing)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: run __graft_entry__.build() (no CPU fallback exists)")
    L = C.CDLL(LIB_PATH)
    _type_library(L)
    _lib = L
    return L


def version() -> str:
    return load().ks_version().decode()


def build_id() -> str:
    """Hash of the library's sources and build flags (csrc/Makefile)."""
    v = version()
    return v.rsplit("build ", 1)[1] if "build " in v else "unknown"


def check(rc: int) -> None:
    if rc != KS_OK:
        msg = load().ks_last_error().decode(errors="replace")
        raise KmerSpansError(msg or f"libkmerspans error {rc}")


class _RegionBlock:
    """Owns a ks_regions block; freed when the last numpy view of it dies."""

    def __init__(self, r: Regions):
        self.r = r

    def __del__(self):
        if _lib is not None:
            _lib.ks_regions_free(C.byref(self.r))


def regions_to_numpy(r: Regions):
    """(pos int32[3, n], score float64[2, n]) as views of the library's output
    block (seq_id|beg|end contiguous, score followed by zeros: include/
    kmer_spans.h), which is freed with the last view -- no host copy."""
    n = int(r.n)
    if n == 0:
        load().ks_regions_free(C.byref(r))
        return np.empty((3, 0), dtype=np.int32), np.empty((2, 0), dtype=np.float64)
    holder = _RegionBlock(r)
    ib = (C.c_char * (3 * n * 4)).from_address(C.cast(r.seq_id, C.c_void_p).value)
    sb = (C.c_char * (2 * n * 8)).from_address(C.cast(r.score, C.c_void_p).value)
    ib._holder = holder
    sb._holder = holder
    pos = np.frombuffer(ib, dtype=np.int32).reshape(3, n)
    score = np.frombuffer(sb, dtype=np.float64).reshape(2, n)
    return pos, score


def shard_plan(seqs, nparts: int):
    """ks_shard_plan (csrc/ks_multi.cpp): the pieces nparts devices take, as
    (part, sequence, lo, hi) rows -- whole sequences by LPT on length, cut in
    the middle of N gaps of >= 1000 bases when whole sequences leave a part
    more than 0.5 % above the fair share.  seqs: uint8 numpy arrays or bytes
    (host memory; the gap scan runs on the host, no device is touched)."""
    arrs = [np.ascontiguousarray(np.frombuffer(s, dtype=np.uint8) if isinstance(s, (bytes, bytearray)) else s,
                                 dtype=np.uint8) for s in seqs]
    ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data if a.size else None for a in arrs])
    lens = np.array([a.size for a in arrs], dtype=np.int64)
    L = load()
    n = L.ks_shard_plan(ptrs, lens.ctypes.data, len(arrs), int(nparts), None, 0)
    if n < 0:
        raise KmerSpansError("ks_shard_plan: bad argument")
    out = np.zeros((max(n, 1), 4), dtype=np.int64)
    L.ks_shard_plan(ptrs, lens.ctypes.data, len(arrs), int(nparts), out.ctypes.data, n)
    return [tuple(int(x) for x in row) for row in out[:n]]


def multi_last_stats():
    """Phases of the last multi-device host call (ks_multi_last_stats, ms).
    host_sum_ms is the sum of the parts' histograms: on the host for
    kmer_counts and kmer_regions, but for kmer_low_comp_regions the count sum
    on the devices (reduce-scatter and all-gather of stripes); the key keeps
    its name."""
    L = load()
    n = L.ks_multi_last_stats(None, 0)
    v = (C.c_double * n)()
    L.ks_multi_last_stats(v, n)
    v = list(v)
    parts = int(v[5])
    return {"total_ms": v[0], "phase1_ms": v[1], "host_sum_ms": v[2], "phase2_ms": v[3], "merge_ms": v[4],
            "parts": [{"body_ms": v[6 + 4 * p], "stage_count_ms": v[7 + 4 * p], "table_upload_ms": v[8 + 4 * p],
                       "scan_ms": v[9 + 4 * p]} for p in range(parts)]}


class Context:
    """One GPU + HIP stream + device workspace (ks_ctx).  Created lazily, so a
    process that only forks workers never touches HIP in the parent."""

    def __init__(self, device: int = 0):
        self.device = device
        self.stream = -1  # -1: the ctx's own non-blocking stream
        self._h = C.c_void_p()
        check(load().ks_ctx_create(device, C.byref(self._h)))

    @property
    def handle(self):
        return self._h

    def set_stream(self, stream_ptr: int | None):
        """hipStream_t as an int; 0/None = HIP's default (null) stream."""
        check(load().ks_ctx_set_stream(self._h, C.c_void_p(stream_ptr) if stream_ptr else None))
        self.stream = int(stream_ptr or 0)

    def set_scan_algo(self, algo: int):
        check(load().ks_ctx_set_scan_algo(self._h, int(algo)))

    def close(self):
        if self._h:
            load().ks_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_contexts: dict[int, Context] = {}


def context(device: int = 0) -> Context:
    ctx = _contexts.get(device)
    if ctx is None:
        ctx = _contexts[device] = Context(device)
    return ctx


def host_ptr(a):
    """The address of an optional numpy array (None stays None, the C NULL)."""
    return None if a is None else a.ctypes.data


def counts_arg(counts):
    """(contiguous uint32 [n, ncol], n, ncol) of a counts matrix, or an error."""
    c = np.asarray(counts)
    if c.ndim != 2 or c.dtype.kind not in "iu":
        raise KmerSpansError("counts must be a [n, ncol] matrix of integer counts")
    if c.dtype != np.uint32:
        if c.size and (int(c.min()) < 0 or int(c.max()) > 0xFFFFFFFF):
            raise KmerSpansError("counts must be in the uint32 range")
        c = c.astype(np.uint32)
    return np.ascontiguousarray(c), int(c.shape[0]), int(c.shape[1])


def rows_arg(rows, what: str, n: int):
    """(int64 row indices or None, rows selected) of a row selection: None
    selects n rows (the library reads that as rows 0 .. n - 1)."""
    if rows is None:
        return None, n
    r = np.asarray(rows)
    if r.ndim != 1 or (r.size and r.dtype.kind not in "iu"):
        raise KmerSpansError(f"{what} must be a 1-d array of integer row indices")
    return np.ascontiguousarray(r, dtype=np.int64), int(r.size)


def condensed_n(length: int, least: int) -> int:
    """n of a condensed vector of n(n-1)/2 entries (n >= least), or an error."""
    n = (1 + int(np.sqrt(1.0 + 8.0 * length))) // 2
    for m in (n - 1, n, n + 1):
        if m >= least and m * (m - 1) // 2 == length:
            return m
    raise KmerSpansError(f"a condensed vector holds n(n-1)/2 entries for some n >= {least}; {length} is no such "
                         "number")


def condensed_arg(dist, least: int):
    """(float64 condensed vector, its n >= least) of a dist argument."""
    d = np.ascontiguousarray(dist, dtype=np.float64)
    if d.ndim != 1:
        raise KmerSpansError("dist must be a 1-d condensed dissimilarity vector")
    return d, condensed_n(int(d.size), least)


def hclust_n(length: int) -> int:
    return condensed_n(length, 2)


def hclust_method(method) -> int:
    if method not in HCLUST_METHODS:
        raise KmerSpansError(f"method must be one of {sorted(HCLUST_METHODS)}, not {method!r}")
    return HCLUST_METHODS[method]


def dist_flags(metric, squared) -> int:
    """The flags of a distance or nearest-neighbour call: the metric's field
    and KS_DIST_SQUARED, which only euclidean and hellinger have a form for."""
    if metric not in DIST_METRICS:
        raise KmerSpansError(f"metric must be one of {sorted(DIST_METRICS)}, not {metric!r}")
    if squared and metric not in ("euclidean", "hellinger"):
        raise KmerSpansError(f"squared=True has no meaning for metric={metric!r}: it needs 'euclidean' or 'hellinger'")
    return DIST_METRICS[metric] | (KS_DIST_SQUARED if squared else 0)


def hclust_outputs(n: int):
    return np.zeros((n - 1, 2), dtype=np.int32), np.zeros(n - 1, dtype=np.float64), np.zeros(n, dtype=np.int32)


def nj_n(length: int) -> int:
    return condensed_n(length, 3)


def nj_outputs(n: int):
    return (np.zeros((n - 3, 2), dtype=np.int32), np.zeros((n - 3, 2), dtype=np.float64),
            np.zeros(3, dtype=np.int32), np.zeros(3, dtype=np.float64))


def silhouette_group(group, n: int, ngroups=None):
    """(int32[n] labels, ngroups) of a group argument: ngroups defaults to the
    largest label (the library checks the labels themselves)."""
    g = np.asarray(group)
    if g.ndim != 1 or g.dtype.kind not in "iu" or g.size != n:
        raise KmerSpansError(f"group must hold one integer label for each of the {n} observations")
    if g.size and (int(g.min()) < -0x80000000 or int(g.max()) > 0x7fffffff):
        raise KmerSpansError("group labels must be in the int32 range")
    g = np.ascontiguousarray(g, dtype=np.int32)
    if ngroups is None:
        ngroups = max(int(g.max()), 1)
    elif int(ngroups) != ngroups or not 1 <= int(ngroups) <= 0x7fffffff:
        raise KmerSpansError(f"ngroups = {ngroups} is not a positive int32")
    return g, int(ngroups)


def kmeans_centers(centers, ncol: int):
    """(init float64[g, ncol] or None, init_rows int64[g] or None, g) of a
    centers argument: a 2-d float array is the matrix form, a 1-d integer
    sequence names positions of the row selection (the library checks both)."""
    c = np.asarray(centers)
    if c.ndim == 1 and c.dtype.kind in "iu" and c.size:
        return None, np.ascontiguousarray(c, dtype=np.int64), int(c.size)
    if c.ndim == 2 and c.dtype.kind in "fiu" and c.shape[0] and c.shape[1] == ncol:
        return np.ascontiguousarray(c, dtype=np.float64), None, int(c.shape[0])
    raise KmerSpansError(f"centers must be a [g, {ncol}] matrix of initial centres or a 1-d sequence of integer "
                         "row positions")


def knn_k(k) -> tuple[int, int]:
    """(k as the library gets it, the k the output buffers are sized by) of a
    k argument: the library checks the range, the buffers only need a size."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise KmerSpansError(f"k must be an integer number of neighbours, not {k!r}")
    k = int(k)
    if not -0x80000000 <= k <= 0x7fffffff:
        raise KmerSpansError(f"k = {k} is not an int32")
    return k, max(1, min(k, KS_KNN_MAX_K))


def seed_args(g, method, first, u, seed):
    """(g, the g the buffers are sized by, flags, first, u float64[g] or None)
    of the arguments of region_kmeans_seed.  The library checks the ranges of
    g, first and u; a seed is turned into np.random.default_rng(seed).random(g)
    here, so the library itself draws nothing."""
    if isinstance(g, bool) or not isinstance(g, (int, np.integer)):
        raise KmerSpansError(f"g must be an integer number of centres, not {g!r}")
    g = int(g)
    if not -0x80000000 <= g <= 0x7fffffff:
        raise KmerSpansError(f"g = {g} is not an int32")
    gb = max(1, min(g, KS_KM_MAX_GROUPS))
    if method not in SEED_METHODS:
        raise KmerSpansError(f"method must be one of {sorted(SEED_METHODS)}, not {method!r}")
    flags = SEED_METHODS[method]
    if flags == 0:
        if u is not None or seed is not None:
            raise KmerSpansError("method='maximin' draws nothing: u and seed must be None")
        if first is None:
            raise KmerSpansError("method='maximin' needs a first row (first=None is a drawn row of 'kmeans++')")
    else:
        if (u is None) == (seed is None):
            raise KmerSpansError("method='kmeans++' needs exactly one of u (g uniform numbers in [0, 1)) and seed")
        if u is None:
            u = np.random.default_rng(seed).random(gb)
        u = np.ascontiguousarray(u, dtype=np.float64)
        if u.ndim != 1 or u.size != gb:
            raise KmerSpansError(f"u must hold g = {g} numbers")
    if first is None:
        first = -1
    if isinstance(first, bool) or not isinstance(first, (int, np.integer)):
        raise KmerSpansError(f"first must be an integer row position or None, not {first!r}")
    first = int(first)
    if not -0x8000000000000000 <= first <= 0x7fffffffffffffff:
        raise KmerSpansError(f"first = {first} is not an int64")
    return g, gb, flags, first, u


def seed_result(res: SeedResult) -> dict:
    return {"n_distinct": int(res.n_distinct), "potential_final": float(res.potential), "radius": float(res.radius),
            "far_row": int(res.far_row)}


def kmeans_result(res: KmeansResult) -> dict:
    """The scalar outputs of ks_spectra_kmeans as the dict entries of R's kmeans object."""
    return {"tot_withinss": float(res.tot_withinss), "totss": float(res.totss),
            "betweenss": float(res.totss) - float(res.tot_withinss), "iter": int(res.iter),
            "converged": bool(res.converged)}


def silhouette_outputs(n: int, ngroups: int) -> dict:
    return {"width": np.zeros(n, dtype=np.float64), "a": np.zeros(n, dtype=np.float64),
            "b": np.zeros(n, dtype=np.float64), "neighbor": np.zeros(n, dtype=np.int32),
            "size": np.zeros(ngroups, dtype=np.int32), "medoid": np.zeros(ngroups, dtype=np.int32),
            "diameter": np.zeros(ngroups, dtype=np.float64), "avg_width": np.zeros(ngroups, dtype=np.float64),
            "avg_width_all": np.zeros(1, dtype=np.float64)}


def silhouette_out_args(res: dict):
    """The nine output pointers of ks_silhouette / ks_silhouette_dev, in order."""
    return [res[k].ctypes.data for k in ("width", "a", "b", "neighbor", "size", "medoid", "diameter", "avg_width",
                                         "avg_width_all")]
