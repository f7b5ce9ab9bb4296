/*
 * kmer_spans.h -- C ABI of the MI355X-native k-mer span scanner
 * (libkmerspans.so, built from kmer_spans_amd/csrc/).
 *
 * This is the drop-in boundary for the span-scan path of lmjakt/kmer_spans
 * (reference snapshot /root/reference, 2025-03-21).  Every entry point is plain
 * C: pointers, sizes and status codes; no torch or HIP types in signatures
 * (HIP streams travel as void*).  The R `.Call` shim
 * (kmer_spans_amd/rcall/kmer_spans_call.c) maps the reference's six
 * registered routines (kmer_spans.c:795-808) onto these functions; see
 * INTEGRATION.md for that binding and for the ctypes binding Python uses.
 *
 * Conventions
 *  - Sequences are byte strings given as (pointer, length); like R CHARSXPs
 *    they contain no NUL.  Bytes N/n split runs; every other byte is encoded
 *    as (c >> 1) & 3 (A/a=0, C/c=1, T/t=2, G/g=3), kmer_spans.c:34-35.
 *  - k-mer codes: first base in the most significant bits, 4^k entries in
 *    the internal A,C,T,G order (kmer_spans.c:41, kmer_seq :161-171).
 *  - 1 <= k <= 15.  The reference admits k = 16 in kmer_counts (UB shift,
 *    Q2), has no lower bound in kmer_regions_r (k = 0 loops forever on an N)
 *    and no check in kmer_low_comp_regions (Q7); those are errors here.
 *  - Every function validates all arguments before touching the device and
 *    returns KS_OK or an error code; ks_last_error() returns the message
 *    (the reference's error() strings where one exists).
 *  - Output regions are allocated by the library; free with ks_regions_free.
 *  - Results are bit-exact with the reference: region triples and their
 *    order, scores (FP64, 0 ulp), counts and visit histograms.
 */
#ifndef KMER_SPANS_H
#define KMER_SPANS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int32_t ks_status;
#define KS_OK 0
#define KS_ERR_ARG 1         /* invalid argument (reference: error()) */
#define KS_ERR_DEVICE 2      /* HIP runtime failure */
#define KS_ERR_NOMEM 3       /* host or device allocation failed */
#define KS_ERR_INTERNAL 4    /* internal consistency check failed */

#define KS_MAX_K 15

/* Thread-local message of the last failing call. */
const char *ks_last_error(void);
/* Library version string, e.g. "kmer_spans_amd 0.2 gfx950 build 1a2b3c4d5e6f"
 * (the build id is a hash of the library's sources, see csrc/Makefile). */
const char *ks_version(void);

/* Region list in the reference's record layout (seq_regions, kmer_spans.c:
 * 46-58): per region (seq_id, beg, end) int32 and score double; the second
 * double the reference stores ("entropy") is always 0.0 and is not kept.
 * Regions are ordered by (seq_id, beg), the reference's emission order. */
/* The four arrays live in one library-allocated block: seq_id, beg, end are
 * consecutive (a column-major 3 x n int32 matrix, the reference's `pos`
 * before kmer_spans.R:76 transposes it), score is followed by n zeros (the
 * 2 x n `score` matrix, second row 0.0, kmer_spans.c:280). */
typedef struct ks_regions {
  int64_t n;
  int32_t *seq_id; /* 0-based index into the input sequences (:536, :610) */
  int32_t *beg;    /* scan index of the first positive k-mer (:272)       */
  int32_t *end;    /* scan index of the first maximum (:289)              */
  double *score;   /* maximum score (:280, :302)                          */
} ks_regions;
void ks_regions_free(ks_regions *r);

/* Execution context: one GPU, one HIP stream, a grow-only device workspace.
 * Created lazily per process (fork-safe: never touches HIP until first use,
 * test.R:550-567 forks with mclapply).  One call at a time per context, like
 * the reference on R's main thread: a call entered from a second thread while
 * another is inside one on the same context returns KS_ERR_ARG ("in use by
 * another thread"); use one context per thread. */
typedef struct ks_ctx ks_ctx;
ks_status ks_ctx_create(int32_t device, ks_ctx **out);
void ks_ctx_destroy(ks_ctx *ctx);
/* Run the ctx's work on an external HIP stream (hipStream_t as void*).
 * NULL is HIP's default (null) stream, e.g. torch's default stream; a new
 * ctx starts on a non-blocking stream of its own. */
ks_status ks_ctx_set_stream(ks_ctx *ctx, void *hip_stream);
/* Process-wide default context on device 0 (what the .Call shim uses). */
ks_ctx *ks_default_ctx(void);

/* ---------------------------------------------------------------------
 * Host-buffer entry points: one per reference .Call routine on the path.
 * Sequences are host pointers; the library stages them to the device.
 * --------------------------------------------------------------------- */

/* kmer_counts(seq_r, k_r) -- replaces kmer_spans.c:453-487.
 * counts: int32[4^k] (overwritten), *n_words: words counted over sequences
 * with length >= k (sequence_kmer_count :135-155, incl. quirk Q1). */
ks_status ks_kmer_counts(ks_ctx *ctx, const char *const *seqs, const int64_t *lens,
                         int32_t nseq, int32_t k, int32_t *counts, double *n_words);

/* kmer_regions_r(seq_r, k_r, kmer_w_r, min_width_r, min_score_r) -- replaces
 * kmer_spans.c:490-546.  w: double[4^k] in internal order; threshold 0.
 * visits: int32[4^k] visit histogram incl. restart re-visits (Q6), may be NULL
 * to skip it; *n_bases: total length of sequences with length >= k. */
ks_status ks_kmer_regions(ks_ctx *ctx, const char *const *seqs, const int64_t *lens,
                          int32_t nseq, int32_t k, const double *w, int64_t w_len,
                          int32_t min_width, double min_score, int32_t *visits,
                          double *n_bases, ks_regions *out);

/* kmer_low_comp_regions(seq_r, k_r, min_width_r, min_score_r, threshold_r) --
 * replaces kmer_spans.c:548-621: count -> weighted rank (rank_kmers_w
 * :189-202, stable (count, index) order) -> scan with threshold thr in (0,1).
 * counts int32[4^k], ranks double[4^k], n[2] = {#words, 0} (Q8). */
ks_status ks_low_comp_regions(ks_ctx *ctx, const char *const *seqs, const int64_t *lens,
                              int32_t nseq, int32_t k, int32_t min_width, double min_score,
                              double thr, int32_t *counts, double *ranks, double *n,
                              ks_regions *out);

/* tr_lr_regions_r(seq_r, params_r = (k, min_length), kmers_r, kmer_scores_r,
 * trans_scores_r) -- replaces kmer_spans.c:649-713 (find_kmer_tr_lr_regions
 * :329-395).  kmers[i] spells the k-mer of entry i of kmer_scores and
 * trans_scores (n_scores = 4^k entries, user order); they are remapped to
 * 2-bit code order as the reference does (:677-690; entries no string maps
 * to are 0 here, uninitialised there).  spectra (optional, 2 x 4^k,
 * column-major) receives the remapped kmer then transition scores.  Regions
 * are 1-based like the reference's: seq_id = sequence index + 1, beg and end
 * = 1 + region begin / max position, score = region maximum. */
ks_status ks_tr_lr_regions(ks_ctx *ctx, const char *const *seqs, const int64_t *lens, int32_t nseq,
                           int32_t k, int32_t min_length, const char *const *kmers,
                           const double *kmer_scores, const double *trans_scores, int64_t n_scores,
                           double *spectra, ks_regions *out);

/* ---------------------------------------------------------------------
 * Several GPUs of one node behind the same entry points.  With a device list
 * of two or more entries, ks_kmer_counts, ks_kmer_regions and
 * ks_low_comp_regions called with ctx == NULL (what the .Call shim does)
 * spread the call: the sequences -- a sequence longer than half a fair share
 * cut in the middle of its N gaps of >= 1000 bases when whole sequences leave
 * a part more than 0.5 % above the fair share -- are dealt to the devices by LPT on length, each device
 * stages, counts and scans its share on a context of its own from a host
 * thread of its own, counts and visit histograms are added exactly (uint32
 * wrap-around), kmer_low_comp_regions builds every device's weighted-rank
 * table from the summed counts, and the regions come back in the caller's
 * coordinates and (seq_id, beg) order: the results equal the one-device
 * call's.  The list may repeat a device (two contexts on one card).  A call
 * with an explicit ctx runs on that ctx's device only.  A call owns every
 * context of the list from its start to its end; a second thread's
 * multi-device call meanwhile returns KS_ERR_ARG (busy).  The reference runs
 * these routines on R's main thread (kmer_spans.c:452-621); this replaces the
 * mclapply-over-sequences pattern of test.R:550-567 inside one call. */
/* devices: n device ordinals (n = 0: device 0 alone, the default).  Read from
 * KS_DEVICES ("0,1,2,3") at first use unless set here. */
ks_status ks_set_devices(const int32_t *devices, int32_t n);
/* The list's length; its first cap entries into devices. */
int32_t ks_get_devices(int32_t *devices, int32_t cap);
/* The shard plan (host only, no device): the pieces nparts devices take, rows
 * (part, sequence, lo, hi) of int64 in out[4 * cap], each part's rows ordered
 * by (sequence, lo); returns the number of pieces (> cap: only cap written),
 * -1 on a bad argument. */
int64_t ks_shard_plan(const char *const *seqs, const int64_t *lens, int32_t nseq, int32_t nparts,
                      int64_t *out, int64_t cap);
/* Phases of the last multi-device call (ms, host wall clock), into out[cap]:
 * [0] whole call, [1] the parts' first phase (kmer_counts / kmer_regions: the
 * whole per-device body; low_comp: staging + count), [2] the sum of the count
 * / visit histograms (on the host; low_comp: the count sum on the devices, a
 * reduce-scatter and an all-gather of stripes), [3] low_comp: rank table + scan, [4] region
 * merge, [5] parts P, then per part p: [6 + 4p] body, [7 + 4p] staging +
 * count, [8 + 4p] score-table upload + compression, [9 + 4p] scan
 * (kmer_regions only).  Returns the number of values available. */
int32_t ks_multi_last_stats(double *out, int32_t cap);
/* Merge of the parts' regions (parts[p] in the coordinates of part p's pieces
 * passed as sequences in plan order, as a call on them returns them) into the
 * caller's coordinates and (seq_id, beg) order (host only). */
ks_status ks_merge_parts(const int64_t *plan, int64_t npieces, int32_t nparts, const ks_regions *parts,
                         ks_regions *out);

/* kmer_seq_r(k_r) -- replaces kmer_spans.c:623-639.  out: 4^k * (k+1) bytes,
 * NUL-terminated k-char strings in internal code order. Host only. */
ks_status ks_kmer_seq(int32_t k, char *out, size_t out_len);

/* ---------------------------------------------------------------------
 * Score-table builders (host, exact).  The reference computes the weighted
 * rank in C (rank_kmers_w :189-202) and leaves log2(f/f_med) and +-1 to user
 * R code (README.md:27-42, kmer.counts()$f kmer_spans.R:25).
 * --------------------------------------------------------------------- */
ks_status ks_rank_table(const int32_t *counts, int32_t k, double total, double *ranks);
ks_status ks_log2_table(const int32_t *counts, int32_t k, double *w);
ks_status ks_pm1_table(const int32_t *counts, int32_t k, double *w);

/* ---------------------------------------------------------------------
 * Device-resident entry points (inputs already in HBM).  Used by bench.py,
 * the multi-GPU driver and callers that keep a genome resident.
 * --------------------------------------------------------------------- */

/* A batch of sequences concatenated in one device buffer.
 * seq: device bytes; offsets_host/offsets_dev: nseq+1 int64 offsets (host
 * and device copies of the same array); sequence q is
 * seq[offsets[q] .. offsets[q+1]). */
typedef struct ks_dev_seqs {
  const uint8_t *seq;
  const int64_t *offsets_host;
  const int64_t *offsets_dev;
  int32_t nseq;
} ks_dev_seqs;

/* A score table resident on the device, s = w[code] - thr precomputed
 * bitwise as the reference computes it (kmer_spans.c:268).  Flags:
 *  KS_TABLE_COMPRESS  if the table has at most 65536 distinct values, store
 *                     it as a uint16 code table plus an FP64 value LUT
 *                     (exact: the LUT holds the very same doubles);
 *  KS_TABLE_EXPAND    also build an expanded table, so the scan issues one
 *                     random read per J scan indices (up to 128 GiB of the
 *                     GPU's HBM; skipped when it does not fit):
 *                     k = 8..13: a line table, one 64-B line per m-mer (m =
 *                     k + own - 1 <= 15) holding the codes / values of its
 *                     own k-mers and of every one- and two-base (FP64: one-
 *                     base) continuation, J = own + 2 (own + 1); at k = 12,
 *                     13 with <= 7168 distinct values, 128-B lines with
 *                     13-bit codes and the three-base continuations as
 *                     11-bit codes (escape to the base table), J = own + 3
 *                     (6 at k = 13);
 *                     other k: one entry per (k+J-1)-mer holding the J
 *                     codes / values of its J consecutive k-mers (J <= 5;
 *                     J = 5 with 12-bit codes and an escape). */
#define KS_TABLE_COMPRESS 1
#define KS_TABLE_EXPAND 2
typedef struct ks_table ks_table;
ks_status ks_table_create(ks_ctx *ctx, const double *w_host, int32_t k, double thr,
                          int32_t flags, ks_table **out);
/* As ks_table_create, with the k-mer counts of the sequences to be scanned
 * (device pointer, 4^k int32; NULL = none) as a position-frequency hint:
 * it only decides which values get the short codes of the expanded table,
 * never the results. */
ks_status ks_table_create_hint(ks_ctx *ctx, const double *w_host, int32_t k, double thr,
                               int32_t flags, const int32_t *freq_dev, ks_table **out);
/* Score table built on the device from device-resident k-mer counts
 * (counts_dev: int32[4^k], e.g. ks_count_dev's), with no 4^k-sized host
 * round trip.  score:
 *   KS_SCORE_LOG2  w = log2(f / f_med), f = counts / sum(counts), f_med = R
 *                  median(f) (README.md:27-42, kmer.counts()$f kmer_spans.R:25)
 *   KS_SCORE_PM1   w = f >= f_med ? 1 : -1 (README.md:37-42)
 *   KS_SCORE_RANK  w = rank_kmers_w(counts, total) (kmer_spans.c:189-202;
 *                  total = the word count, as kmer_low_comp_regions :600-602)
 * total is ignored for LOG2 / PM1.  The table holds s = w - thr; it is
 * bitwise the table ks_table_create_hint(ks_log2_table / ks_pm1_table /
 * ks_rank_table(...), thr, flags, counts_dev) builds: log2 and +-1 are
 * evaluated once per distinct count on the host (glibc log2), the ranks by
 * a closed-form exact evaluation of the sequential FP64 prefix.  counts_dev
 * also serves as the position-frequency hint.  max_ext_bytes caps the
 * expanded table (<= 0: the default cap).  w_dev: optional device
 * double[4^k] receiving w.  In ks_table_info, ms_upload is the sort + value
 * phase and ms_compress the code/value mapping. */
#define KS_SCORE_LOG2 1
#define KS_SCORE_PM1 2
#define KS_SCORE_RANK 3
ks_status ks_table_from_counts(ks_ctx *ctx, const int32_t *counts_dev, int32_t k, int32_t score,
                               double total, double thr, int32_t flags, int64_t max_ext_bytes,
                               double *w_dev, ks_table **out);
void ks_table_destroy(ks_table *t);
/* The library keeps the buffer of the last destroyed expanded table (one
 * per device) for the next table that fits in it: a fresh 32-128 GiB
 * hipMalloc can take seconds (the driver clears new VRAM).  Like a caching
 * allocator, it stays allocated after the call that destroyed the table
 * returns (up to 128 GiB at k = 13 for a device-API table, 32 GiB for the
 * host entry points' J = 4 tables).  This returns it to the driver; so does
 * ks_ctx_destroy for its device; environment KS_EXT_POOL=0 disables the
 * pool.  Workspace retained by a context (scan scratch, the table builder's
 * sort scratch of ~20 B x 4^k) is freed by ks_ctx_destroy.  The last two freed region
 * output blocks of >= 1 MiB (ks_regions_free) are kept for reuse and freed here too. */
void ks_release_cache(void);
/* Memory policy of the host-buffer entry points (ks_kmer_counts,
 * ks_kmer_regions, ks_low_comp_regions, ks_tr_lr_regions, ks_windowed_dist,
 * ks_kmers_to_file): what happens to a call's device memory -- the context's
 * workspace and the pooled table buffer -- when it ends.
 *   keep = 2 (the default): kept while calls keep coming, returned once the
 *            context has been idle for the idle time (ks_set_host_cache_idle,
 *            20 s by default; a library thread returns it), so a session that
 *            calls kmer_regions_r in a loop pays for fresh VRAM once (the
 *            driver clears new VRAM: seconds for tens of GiB) and one that
 *            called it once gets its VRAM back shortly after;
 *   keep = 0: returned when the call ends (VRAM at its pre-call level on
 *            return; every call allocates again);
 *   keep = 1: kept until ks_release_cache() or ks_ctx_destroy.
 * Environment KS_HOST_CACHE=0/1/2 and KS_HOST_CACHE_SECONDS set them at first
 * use.  The pinned host staging buffer is kept either way. */
ks_status ks_set_host_cache(int32_t keep);
ks_status ks_set_host_cache_idle(double seconds);

/* Fork broker (mclapply after use, test.R:351 then :554-565).  On: right
 * before this process's first HIP use the library forks a broker process (a
 * copy that never touched HIP; not started if HIP is already open in the
 * process, e.g. by torch); children forked later send their host-buffer calls
 * (ks_kmer_counts, ks_kmer_regions, ks_low_comp_regions, ks_tr_lr_regions,
 * ks_windowed_dist, ks_kmers_to_file) to it over a Unix socket instead of
 * being refused.  Off by default (KS_FORK_BROKER=1 turns it on); the R shim's
 * R_init_kmer_spans turns it on.  Call before the first HIP use. */
ks_status ks_set_fork_broker(int32_t on);
/* 1 if the table is stored compressed (uint16 codes + LUT), else 0. */
int32_t ks_table_is_compressed(const ks_table *t);
int64_t ks_table_distinct(const ks_table *t);
/* Scan indices served per random table read (J of the expanded table, 1 if
 * it was not built). */
int32_t ks_table_positions_per_read(const ks_table *t);
/* Bits per value code in the expanded table (12, 13 for 128-B lines, 16),
 * 16 for a compressed table without one, 64 for an FP64 table. */
int32_t ks_table_code_bits(const ks_table *t);
/* Share of positions (by the hint, else by k-mer multiplicity) whose value
 * escapes the short codes: the 12-bit codes (code bits 12, every index) or
 * the 11-bit three-base continuations of 128-B lines (code bits 13, one
 * index per line); 0 otherwise. */
double ks_table_escape_fraction(const ks_table *t);

/* Shape and setup cost of a device table (host wall clock around the
 * synchronised device work of ks_table_create*, milliseconds). */
typedef struct ks_table_info {
  int32_t k, compressed, positions_per_read, code_bits;
  int64_t distinct, ext_bytes;
  double escape_fraction;
  double ms_upload;    /* w to the device, s = w - thr, finiteness scan          */
  double ms_compress;  /* distinct values (radix sort + unique), uint16 codes    */
  double ms_codes12;   /* 12-bit code choice: position-weight histogram, renumber */
  double ms_ext_alloc; /* hipMalloc of the expanded table                        */
  double ms_ext_build; /* expanded-table build kernel                            */
  double ms_total;
  int32_t line_kind;   /* 0: no line table; 1: uint16 64-B lines, 2: FP64 64-B lines, 3: 128-B lines */
  int32_t line_own;    /* own k-mers per line (m = k + line_own - 1)              */
} ks_table_info;
ks_status ks_table_get_info(const ks_table *t, ks_table_info *out);

/* A read-only window into a built table (tests compare every built form
 * with a host model of its layout).  None of these launches a kernel or
 * writes to the device.  Parts: */
#define KS_TABLE_PART_VALS 0    /* FP64 s, 4^k (uncompressed tables)                  */
#define KS_TABLE_PART_CODES 1   /* uint16 codes, 4^k (compressed tables)              */
#define KS_TABLE_PART_LUT 2     /* FP64 value of every code, distinct entries         */
#define KS_TABLE_PART_EXT 3     /* the expanded table or the line table               */
#define KS_TABLE_PART_RLINES 4  /* weighted-rank 128-B code lines                     */
#define KS_TABLE_PART_RPIECES 5 /* rank pieces: pairs of uint64 (base bits, increment) */
#define KS_TABLE_PART_LUT12 6   /* FP64[4096]: the values of the 12-bit codes         */
#define KS_TABLE_PART_MAP12 7   /* uint16[4096]: 12-bit code -> uint16 code           */
#define KS_TABLE_PART_APPROX 8  /* FP16 bits per approx_k-base prefix                 */
/* Bytes of a part; 0 when the table does not have it (or part is unknown). */
int64_t ks_table_debug_bytes(const ks_table *t, int32_t part);
/* Synchronous copy of bytes [offset, offset + nbytes) of a part to host
 * memory, on the table's device; a range outside the part is KS_ERR_ARG. */
ks_status ks_table_debug_read(const ks_table *t, int32_t part, int64_t offset, int64_t nbytes, void *dst_host);
typedef struct ks_table_props {
  int32_t int_exact;      /* every s is a finite integer of magnitude <= 2^20   */
  int32_t no_nan_posinf;  /* no s is NaN or +Inf                                */
  double max_abs;         /* max |s| over the finite values                     */
  int32_t ext_J, ext_bits;        /* as built (1, 16 without an expanded form) */
  int32_t line_kind, line_own;    /* of the table in KS_TABLE_PART_EXT         */
  int32_t approx_k, n_rpieces;
} ks_table_props;
ks_status ks_table_debug_props(const ks_table *t, ks_table_props *out);

/* Scan statistics of the last ks_scan_dev call (device time of each phase,
 * measured with hipEvents on the ctx stream). */
typedef struct ks_scan_stats {
  double ms_total;      /* whole scan (runs + kernels + compaction) */
  double ms_runs;       /* run segmentation */
  double ms_scan;       /* dominant scan kernel(s) */
  double ms_rescan;     /* rescan rounds */
  double ms_finish;     /* region ordering + D2H */
  int64_t n_bases;      /* bytes of sequences with length >= k */
  int64_t n_scored;     /* top-level scored positions */
  int64_t n_runs;       /* N-free runs with scored positions */
  int64_t n_regions;
  int64_t n_rescan;     /* rescan ranges processed */
  int32_t scan_algo;    /* 0 = lane per run, 1 = chunked carry scan */
  int64_t n_replay;     /* chunks whose carry needed an exact replay */
  /* chunked scan (scan_algo 1) phases inside the step; ms_scan is P1 */
  double ms_layout;     /* chunk table (k_make_chunks) */
  double ms_predict;    /* P2: approximate carry scan, segment marks, binade summaries */
  double ms_carry;      /* P3/P4: exact carry, heads */
  double ms_stitch;     /* P5: excursion stitch, candidates */
} ks_scan_stats;
/* The chunked scan's units (tests place seams with them): scan indices per
 * chunk, one lane each, and chunks per tile of the carry, the prescan and the
 * stitch.  One trip of the per-run wave loops takes 64 tiles. */
int32_t ks_scan_chunk_indices(void);
int32_t ks_scan_tile_chunks(void);

/* Span scan of device-resident sequences (the hot path).  visits_dev: device
 * int32[4^k] accumulated (caller zeroes), or NULL.  Regions are returned in
 * host memory.  stats may be NULL. */
ks_status ks_scan_dev(ks_ctx *ctx, const ks_dev_seqs *seqs, int32_t k, const ks_table *table,
                      int32_t min_width, double min_score, int32_t *visits_dev,
                      ks_regions *out, ks_scan_stats *stats);

/* tr_lr scan of device-resident sequences: trans = transition scores, init
 * = first-k-mer scores, both ks_tables in 2-bit code order built with
 * threshold 0 (init without KS_TABLE_COMPRESS).  Tables with non-finite
 * values are scanned by the literal per-run kernel (the reference keeps NaN
 * through its clamp); all others by the chunked scan. */
ks_status ks_tr_lr_dev(ks_ctx *ctx, const ks_dev_seqs *seqs, int32_t k, const ks_table *trans,
                       const ks_table *init, int32_t min_length, ks_regions *out, ks_scan_stats *stats);

/* Sequence index: a handle that lets repeated scans of the same
 * device-resident sequences reuse the run segmentation, the packed 2-bit
 * codes and (for the same k and scan kind) the chunk layout of the previous
 * scan instead of recomputing them from the bytes on every call.
 *
 * The handle is a small host object: create does no device work and
 * allocates no device memory.  It records a process-unique id, seqs->seq,
 * seqs->offsets_dev, seqs->nseq and a copy of seqs->offsets_host.  What it
 * indexes lives in the workspace of the context that scanned last: a scan
 * with the handle is a hit when that context's workspace still holds the
 * data of the same handle's previous scan, and a build (the work of a plain
 * call) otherwise -- after a scan of other sequences, a plain scan, a
 * ks_windowed_dev call, a host-buffer entry point or a release of the
 * workspace on that context.
 *
 * Contract: from create to destroy the caller changes neither the sequence
 * bytes nor the offsets (host or device).  Changed sequences need a new
 * index.  A hit call runs a cheap check of the cached runs and of a sample of
 * the packed codes against the bytes; a mismatch fails the call with
 * KS_ERR_ARG ("sequence bytes changed under a sequence index"), returns no
 * regions, counts in guard_failures and makes the next call with the handle
 * a build.  The check is a tripwire for contract violations, not a proof: a
 * change inside a run and outside the sampled units passes it.
 *
 * The _indexed entries return KS_ERR_ARG when seqs does not match the handle
 * (pointers, nseq, offsets).  ix == NULL, or KS_NO_SEQ_INDEX set in the
 * environment (read per call), makes them the plain entries.  ks_scan_dev
 * and ks_tr_lr_dev always recompute.  On a hit ks_scan_stats.ms_runs is 0.
 *
 * The chunked scan keeps two more things of a handle's last scan on the
 * context, in a workspace slot of their own.  The chunk table (start, length
 * and run of every 256-index chunk, the run of every tile) depends on the
 * runs, k and the scan kind only: a hit with the same k and scan kind takes it
 * as it is (chunk_reuses).  The entry hint is the value each chunk was
 * predicted to be entered with, from which pass 1 picks the binade it
 * summarises in; a scan with the same table(s) as the previous one takes the
 * prediction that scan made from its exact pass-1 results instead of running
 * the predictor (hint_reuses).  Tables are told apart by a process-unique id,
 * never by address.  A hint is only a hint: a wrong one costs gathered
 * summaries or replays (ks_scan_stats.n_replay may differ from a scan without
 * it), never a region, a score or a visit count.  KS_NO_CHUNK_REUSE=1 and
 * KS_NO_ENTRY_HINT=1 (read per call) switch either off.
 *
 * On the wide-line and uint16-line table forms the slot also keeps the exact
 * value every chunk was entered with.  The next scan with the same table(s)
 * starts each chunk's pass 1 from it, walks the carried head itself and checks,
 * bit for bit, that its exact exit is the kept entry of the next chunk of the
 * run; a run's first chunk enters at 0, so when every check passes every kept
 * entry is proved exact and the predictor, the summaries, the carry and the
 * heads are not run at all (ks_seq_index_entry_info: entry_reuses; such a call
 * also counts as a hint_reuses).  A failed check reruns the call on the hint
 * path (entry_fallbacks).  The thresholds and the visit histogram are not part
 * of the key: every index is scored and every excursion emitted under the
 * call's own.  KS_NO_EXACT_ENTRY=1 (read per call) switches it off.
 *
 * The first scan from exact entries (the second scan of a genome with a
 * table) also writes the uint16 value code of every scan index into a slot of
 * its own, 2 B per scan index of the genome (about 6.2 GB at 3.1 Gbp); the
 * scans after it stream those codes instead of reading the table's lines
 * (ks_seq_index_codes_info: code_builds, code_reuses).  The codes depend on
 * the bytes, k, the scan kind and the table(s) only, the key of the exact
 * entries, and go wherever those go.  Every exact entry is still verified, and
 * one code in 64 chunks is compared with the table; a failure reruns the call
 * on the hint path (code_fallbacks) and the codes are written again.  That
 * check is a tripwire for contract violations, as the check against the bytes
 * is, not a proof.  Only compressed wide-line and uint16-line tables whose
 * distinct values fit the LDS copy keep codes; a new threshold inside the
 * table (thr) or another k is another table and starts over.  Without the
 * memory for the slot the scan goes on without it (code_alloc_failures).
 * KS_NO_KEPT_CODES=1 (read per call) switches the path and the slot off. */
typedef struct ks_seq_index ks_seq_index;
ks_status ks_seq_index_create(const ks_dev_seqs *seqs, ks_seq_index **out);
void ks_seq_index_destroy(ks_seq_index *ix);
typedef struct ks_seq_index_info {
  int64_t builds;         /* indexed calls that ran the run segmentation            */
  int64_t hits;           /* indexed calls that reused it                           */
  int64_t layout_builds;  /* indexed calls that computed the chunk layout (every
                             build, and a hit with another k or scan kind)          */
  int64_t guard_failures; /* hit calls failed by the check against the bytes        */
  /* chunked scans with the handle that succeeded (see below) */
  int64_t chunk_reuses;     /* took the chunk table of the context's previous scan  */
  int64_t hint_reuses;      /* took its entry hint too: no predictor                */
  int64_t predictor_builds; /* ran the predictor (pass-1-summary tables only)       */
} ks_seq_index_info;
ks_status ks_seq_index_info_get(const ks_seq_index *ix, ks_seq_index_info *out);
/* Chunked scans with the handle that started pass 1 from the kept exact
 * entries and verified them (entry_reuses), and calls whose verification
 * failed and that were rerun on the hint path (entry_fallbacks). */
ks_status ks_seq_index_entry_info(const ks_seq_index *ix, int64_t *entry_reuses, int64_t *entry_fallbacks);
/* The kept codes: scans that wrote them, scans that read them, reading calls
 * rerun on the hint path, calls that went without the slot for want of memory. */
ks_status ks_seq_index_codes_info(const ks_seq_index *ix, int64_t *code_builds, int64_t *code_reuses,
                                  int64_t *code_fallbacks, int64_t *code_alloc_failures);
/* Diagnostics for tests.  ks_kept_codes_layout: the bytes of the kept codes of
 * nch chunks in steps of J scan indices and the halfword offset of scan index
 * i of chunk c (host arithmetic).  ks_kept_codes_debug_read: the kept codes of
 * chunks [c0, c0 + nchunks) of the context's last chunked scan in index order,
 * 256 per chunk (indices past a chunk's length hold anything), and the step J;
 * a synchronous copy, nothing is written to the device; KS_ERR_ARG when the
 * context keeps no codes.  ctx NULL: the default context. */
ks_status ks_kept_codes_layout(int32_t J, int64_t nch, int64_t c, int32_t i, int64_t *bytes, int64_t *halfword);
ks_status ks_kept_codes_debug_read(ks_ctx *ctx, int64_t c0, int64_t nchunks, uint16_t *dst_host, int32_t *steps_J);
ks_status ks_scan_dev_indexed(ks_ctx *ctx, const ks_dev_seqs *seqs, ks_seq_index *ix, int32_t k,
                              const ks_table *table, int32_t min_width, double min_score, int32_t *visits_dev,
                              ks_regions *out, ks_scan_stats *stats);
ks_status ks_tr_lr_dev_indexed(ks_ctx *ctx, const ks_dev_seqs *seqs, ks_seq_index *ix, int32_t k,
                               const ks_table *trans, const ks_table *init, int32_t min_length, ks_regions *out,
                               ks_scan_stats *stats);

/* k-mer counting of device-resident sequences into counts_dev (int32[4^k],
 * accumulated: the caller zeroes it).  *n_words as in ks_kmer_counts. */
ks_status ks_count_dev(ks_ctx *ctx, const ks_dev_seqs *seqs, int32_t k, int32_t *counts_dev,
                       double *n_words);

/* ---------------------------------------------------------------------
 * Ingest: sequence files -> device-resident records,
 * batched multi-k counting and the reference's binary count files.
 * --------------------------------------------------------------------- */

/* Records of a FASTA file resident on the device.  The reference reads
 * sequence files with Biostrings::readDNAStringSet (kmers.to.file,
 * kmer_spans.R:127-160); here the raw bytes go to HBM and are parsed there
 * (description lines '>', ';' comments, one '\r' before '\n' dropped, empty
 * lines skipped, IUPAC DNA letters of either case plus '-', '+', '.'; other
 * bytes, or sequence before the first description line, are errors).  Kept
 * bytes are upper-cased (as.character(DNAStringSet)).  seqs can be passed to
 * ks_scan_dev / ks_tr_lr_dev / ks_count_dev directly. */
typedef struct ks_fasta {
  ks_dev_seqs seqs;   /* records with length >= min_len, device bytes + offsets */
  char **names;       /* seqs.nseq descriptions (the line after '>')            */
  int64_t n_records;  /* records in the file                                    */
  int64_t bases_all;  /* bases of all records (seq.size, kmer_spans.R:139)      */
  int64_t bases_kept; /* bases of the kept records (seq.fsize, :141)            */
  int32_t device;
  double ms_upload;   /* host read + H2D (overlapped)                           */
  double ms_parse;    /* device parse + record selection                        */
} ks_fasta;
/* path: plain or gzip FASTA.  Keeps records with length >= min_len (:141). */
ks_status ks_fasta_load(ks_ctx *ctx, const char *path, int64_t min_len, ks_fasta *out);
/* The same from an in-memory FASTA text of n bytes. */
ks_status ks_fasta_parse(ks_ctx *ctx, const char *buf, int64_t n, int64_t min_len, ks_fasta *out);
/* Copy the kept records' bytes (offsets_host[nseq] bytes) to host memory. */
ks_status ks_fasta_copy_seqs(const ks_fasta *f, uint8_t *dst);
void ks_fasta_free(ks_fasta *f);

/* k-mer counting for several k in one pass over device-resident sequences
 * (kmer.counts per k, kmer_spans.R:149-151).  counts_dev[i]: device
 * int32[4^ks[i]] accumulated (caller zeroes); n_words[i] as ks_kmer_counts. */
ks_status ks_count_multi_dev(ks_ctx *ctx, const ks_dev_seqs *seqs, const int32_t *ks, int32_t nk,
                             int32_t *const *counts_dev, double *n_words);

/* Count file of kmers.to.file / read.kmers (kmer_spans.R:113-186): int32
 * magic, int32 n, n x int32 4^k, then the n count vectors (int32, native
 * order). */
ks_status ks_count_file_write(const char *path, int32_t magic, int32_t nk, const int32_t *ks,
                              const int32_t *const *counts);
typedef struct ks_count_file {
  int32_t valid;      /* 0: wrong magic or n < 1 (read.kmers returns FALSE)   */
  int32_t nk;
  int32_t *k;         /* as.integer(log2(4^k) / 2) (:184); -1 for length 0    */
  int64_t *lens;      /* entries actually read (readBin stops at EOF)         */
  int32_t **counts;
} ks_count_file;
ks_status ks_count_file_read(const char *path, int32_t magic, ks_count_file *out);
void ks_count_file_free(ks_count_file *f);

/* kmers.to.file(seq.f, out.prefix, k, min.l, magic) -- kmer_spans.R:127-160:
 * load, drop records shorter than min_l, count every k (ks_count_multi_dev),
 * write <out_prefix>counts_<k1>_<k2>...bin.  A file that cannot be read, a
 * bad k, or no record left is the reference's NA result: KS_OK with
 * written = 0 and the reason in message. */
typedef struct ks_kmer_file_info {
  int32_t written;
  double seq_size, seq_fsize, seq_fl; /* :139-142 */
  char out_path[4096];
  char message[512];
} ks_kmer_file_info;
ks_status ks_kmers_to_file(ks_ctx *ctx, const char *seq_path, const char *out_prefix, const int32_t *ks,
                           int32_t nk, double min_l, int32_t magic, ks_kmer_file_info *info);

/* ---------------------------------------------------------------------
 * Windowed k-mer count distributions.
 * --------------------------------------------------------------------- */

/* windowed_kmer_count_distributions_r(seq_r, kmers_r, k_r, window_r,
 * ret_flag_r) -- replaces kmer_spans.c:717-793 (window.kmer.dist,
 * kmer_spans.R:103-118).  In every N-free run of every sequence longer than
 * window, each window of `window` bases holds window - k + 1 k-mers; for
 * query k-mer i (kmers[i], k characters, coded by init_kmer :757-758)
 * dist[i * (window + 1) + c] counts the windows holding it c times
 * (column-major (window + 1) x kmer_n, overwritten).  seq_included[q] = 1 if
 * lens[q] > window.  ret_flag & 1: scores[q] (int32 [lens[q] x kmer_n],
 * column-major, for included q; may be NULL to skip one) receives the count
 * at every window start, 0 elsewhere.  1 <= k <= 15, window >= 2k. */
ks_status ks_windowed_dist(ks_ctx *ctx, const char *const *seqs, const int64_t *lens, int32_t nseq,
                           const char *const *kmers, int32_t kmer_n, int32_t k, int32_t window, int32_t ret_flag,
                           int32_t *dist, int32_t *seq_included, int32_t *const *scores);
/* Device-resident form: kmer_codes are 2-bit codes (< 4^k); dist_dev
 * accumulated (caller zeroes); included_dev may be NULL; scores_dev (NULL =
 * none, zeroed by the caller) holds per sequence q the [len_q x kmer_n]
 * matrix at element offset kmer_n * offsets[q]. */
ks_status ks_windowed_dev(ks_ctx *ctx, const ks_dev_seqs *seqs, const uint32_t *kmer_codes, int32_t kmer_n,
                          int32_t k, int32_t window, int32_t *dist_dev, int32_t *included_dev, int32_t *scores_dev);

/* ---------------------------------------------------------------------
 * Per-region q-mer spectra and Shannon entropy (csrc/ks_spectra.hip).
 * --------------------------------------------------------------------- */

/* What the reference's user script does with the regions next (test.R:703-720:
 * subseq per region, oligonucleotideFrequency on both strands, -sum p log2 p),
 * without taking the genome back to the host.
 *
 * Intervals: n triples (seq_id, beg, end); seq_id is a 0-based sequence index,
 * beg..end are 1-based and inclusive in that sequence's coordinates -- the
 * numbers ks_scan_dev / ks_kmer_regions return, read as test.R:706 reads them
 * (subseq(seq[id + 1], beg, end)); ks_tr_lr_* regions carry seq_id + 1, so
 * subtract 1 from those.  An interval covers bytes seq[beg-1 .. end-1]; it is
 * valid when 0 <= seq_id < nseq, beg >= 1, end <= length and end >= beg - 1
 * (width 0 is valid).  Intervals may overlap, repeat and come in any order;
 * row i of the outputs belongs to interval i.
 * Words: every window of q consecutive bytes wholly inside the interval that
 * holds no N/n counts once; no end-of-run quirks apply (Q1 and Q5 belong to
 * the scan).  Bytes are coded (c >> 1) & 3 as everywhere here.  Biostrings'
 * oligonucleotideFrequency skips windows holding any non-ACGT letter; this
 * skips only N/n and codes every other byte as it falls.
 * Columns: spectra is n x 4^q uint32, row-major; bin c is the word with code
 * c, first base most significant, in the order of ks_kmer_seq(q) (internal
 * A,C,T,G, not Biostrings' alphabetical order).  1 <= q <= KS_SPECTRA_MAX_Q.
 * flags & KS_SPECTRA_BOTH_STRANDS: row[c] = n[c] + n[rc(c)], rc(c) = the q
 * two-bit digits reversed and each XORed with 2 (proportional to fwd + rev of
 * test.R:707-709); otherwise row[c] = n[c].  A sequence has < 2^31 bytes, so
 * no bin wraps: the counts are exact.
 * Entropy: T = sum(row), H = -sum over row[c] > 0 of (row[c] / T) log2(row[c]
 * / T) in FP64 (device log2; within 4^q * 2q * 2^-52 of the exactly summed
 * value); NaN when T = 0 (width < q or all N), as R's 0/0 gives.
 * n = 0 is KS_OK and touches nothing.  ctx == NULL is the default context on
 * device 0; the call is never spread over a device list (ks_set_devices) and
 * is not forwarded by the fork broker: it takes the usual context-entry
 * checks only. */
#define KS_SPECTRA_MAX_Q 6
#define KS_SPECTRA_BOTH_STRANDS 1
typedef struct ks_spectra_stats { /* hipEvent times on the ctx stream, ms */
  double ms_total, ms_plan, ms_count, ms_entropy;
  int64_t n_regions;
  int64_t n_bases; /* sum of widths */
  int64_t n_words; /* sum of single-strand counts */
  int64_t n_tiles; /* work tiles of the counting kernel */
} ks_spectra_stats;

/* Device-resident: the three interval arrays, spectra_dev (n x 4^q uint32,
 * row-major, OVERWRITTEN -- the caller need not zero it) and entropy_dev (n
 * doubles, may be NULL: the entropy pass is skipped) are device pointers.
 * The intervals are checked on the device before any kernel reads a
 * sequence through them: a bad one returns KS_ERR_ARG ("interval i out of
 * range", the first such i) with no kernel launched on the sequences and the
 * outputs untouched.  stats may be NULL. */
ks_status ks_region_spectra_dev(ks_ctx *ctx, const ks_dev_seqs *seqs, const int32_t *seq_id_dev,
                                const int32_t *beg_dev, const int32_t *end_dev, int64_t n, int32_t q,
                                int32_t flags, uint32_t *spectra_dev, double *entropy_dev,
                                ks_spectra_stats *stats);
/* Host buffers: validates everything, intervals included, before any device
 * call; stages the sequences like ks_kmer_counts does, uploads the intervals,
 * runs the device entry, copies spectra (n x 4^q) and entropy (n, may be
 * NULL) back. */
ks_status ks_region_spectra(ks_ctx *ctx, const char *const *seqs, const int64_t *lens, int32_t nseq,
                            const int32_t *seq_id, const int32_t *beg, const int32_t *end, int64_t n,
                            int32_t q, int32_t flags, uint32_t *spectra, double *entropy);
/* Bases per work tile of the counting kernel (tests place seams with it). */
int32_t ks_spectra_tile_bases(void);

/* ---------------------------------------------------------------------
 * Pairwise distances between region spectra (csrc/ks_spectra_dist.hip).
 * --------------------------------------------------------------------- */

/* What the reference's author does with the spectra next (test.R:762-807):
 * dist() of the strand-folded, row-normalised tetramer spectra -- the
 * Euclidean distance between every pair of rows -- for all regions and for a
 * row subset, without taking the counts back to the host.
 *
 * Input: a spectra matrix as ks_region_spectra_dev writes it, n x ncol uint32,
 * row-major.  1 <= ncol <= KS_DIST_MAX_NCOL (4^6); ncol is not tied to a q.
 * Profile of a row: p[k] = (double)c[k] / (double)T, T the row sum accumulated
 * in 64-bit integers (below 2^44, so its conversion is exact); one IEEE
 * division per element.  For a both-strands row this is the (fwd + rev) / 2
 * of test.R:707-709.
 * Distance of rows i and j, fixed as an order of operations: acc = 0; for
 * k = 0 .. ncol - 1 ascending: d = p_i[k] - p_j[k]; acc = acc + d * d, with the
 * subtraction, the multiplication and the addition separate FP64 operations
 * (no FMA) and one accumulator per pair.  flags & KS_DIST_SQUARED returns acc,
 * otherwise the result is sqrt(acc).  A row with T = 0 gives NaN against every
 * row (the natural 0 / 0).  It follows that the bits can be predicted on the
 * host, that d(i, j) and d(j, i) are the same bits, that a row against itself
 * is exactly 0, and that rows whose counts are proportional (c_j = f * c_i)
 * are at exactly 0: the correctly rounded division gives both the same p.
 *
 * Row selections: an optional array of int64 row indices into the matrix, in
 * any order, repeats allowed.  NULL with a count of m means rows 0 .. m - 1 in
 * order (pass m = n for all rows; m > n is an error then).
 * Condensed form: all pairs i < j of the m selected rows; out holds
 * m (m - 1) / 2 doubles in the order of R's dist object (scipy's pdist): pair
 * (i < j) at i * m - i (i + 1) / 2 + (j - i - 1).  m = 0 or 1 is valid and
 * writes nothing.
 * Cross form: selected rows A (na) against selected rows B (nb), a dense
 * na x nb row-major block -- the way to walk a list too large for one matrix
 * block by block, or to measure regions against a few centroids.  na = 0 or
 * nb = 0 writes nothing.
 * All output offsets are 64-bit (the condensed form passes 2^31 entries at
 * m = 65,537).  The caller owns the output.  ctx == NULL is the default
 * context on device 0; the calls are never spread over a device list and are
 * not forwarded by the fork broker.
 *
 * Metrics (R's dist(method=), and the Hellinger distance): bits 8 .. 11 of
 * flags name the metric, KS_DIST_EUCLIDEAN (0, the text above) by default.
 * The allowed bits are KS_DIST_SQUARED | KS_DIST_METRIC_MASK; a field value
 * above KS_DIST_HELLINGER is "unknown distance metric N", and KS_DIST_SQUARED
 * with manhattan, maximum or canberra is refused (the flag needs euclidean or
 * hellinger).  p is the profile above; every operation below is a separate
 * FP64 instruction, one accumulator per pair, k ascending:
 *   manhattan: acc = 0; acc = acc + |p_i[k] - p_j[k]|.  The result is acc
 *              (twice the total variation distance of the two profiles).
 *   maximum:   acc = 0; t = |p_i[k] - p_j[k]|; acc = t > acc ? t : acc.  A NaN
 *              t makes the result NaN.
 *   canberra:  acc = 0, cnt = 0; s = p_i[k] + p_j[k]; a column with s == 0 is
 *              omitted, otherwise acc = acc + |p_i[k] - p_j[k]| / s and
 *              cnt = cnt + 1.  The result is acc if cnt == ncol, otherwise
 *              acc / ((double)cnt / (double)ncol): R's rule (distance.c).
 *   hellinger: q[k] = sqrt(p[k]), one correctly rounded root per profile
 *              entry; acc is the Euclidean loop over q.  The result is
 *              0.5 * acc with KS_DIST_SQUARED, otherwise sqrt(0.5 * acc): 0
 *              between proportional rows, at most 1.
 * In every metric d(i, j) has the bits of d(j, i), d(i, i) = 0, and a pair
 * that involves a row with T = 0 is NaN. */
#define KS_DIST_MAX_NCOL 4096
#define KS_DIST_SQUARED 1
#define KS_DIST_METRIC_MASK 0xf00
#define KS_DIST_EUCLIDEAN 0x000
#define KS_DIST_MANHATTAN 0x100
#define KS_DIST_MAXIMUM 0x200
#define KS_DIST_CANBERRA 0x300
#define KS_DIST_HELLINGER 0x400
typedef struct ks_dist_stats { /* hipEvent times on the ctx stream, ms */
  double ms_total, ms_normalise, ms_distance;
  int64_t n_pairs;       /* distances computed and written */
  int64_t bytes_written; /* 8 * n_pairs */
  int64_t panel_bytes;   /* the FP64 profile panel the call allocated and freed */
} ks_dist_stats;

/* Device-resident: spectra_dev, the selections and out_dev are device
 * pointers.  The indices are checked on the device before anything is
 * written: a bad one returns KS_ERR_ARG ("row index s out of range", s the
 * first such position in its selection) with the output untouched.  The only
 * allocation is the FP64 profile panel of the selected rows ((m or na + nb) x
 * ncol x 8 bytes; KS_ERR_NOMEM if it fails), freed before return.  stats may
 * be NULL. */
ks_status ks_spectra_dist_dev(ks_ctx *ctx, const uint32_t *spectra_dev, int64_t n, int32_t ncol,
                              const int64_t *rows_dev, int64_t m, int32_t flags, double *out_dev,
                              ks_dist_stats *stats);
ks_status ks_spectra_cross_dist_dev(ks_ctx *ctx, const uint32_t *spectra_dev, int64_t n, int32_t ncol,
                                    const int64_t *rows_a_dev, int64_t na, const int64_t *rows_b_dev,
                                    int64_t nb, int32_t flags, double *out_dev, ks_dist_stats *stats);
/* Host buffers: validates every argument and every index before any device
 * call, then uploads, runs the device entry and copies the result back. */
ks_status ks_spectra_dist(ks_ctx *ctx, const uint32_t *spectra, int64_t n, int32_t ncol, const int64_t *rows,
                          int64_t m, int32_t flags, double *out);
ks_status ks_spectra_cross_dist(ks_ctx *ctx, const uint32_t *spectra, int64_t n, int32_t ncol,
                                const int64_t *rows_a, int64_t na, const int64_t *rows_b, int64_t nb,
                                int32_t flags, double *out);
/* The kernels' index arithmetic on the host (csrc/ks_dist_index.h; tests walk
 * it where a GPU run would need terabytes of output): off[x] = the condensed
 * offset of pair (i[x] < j[x]) of m rows; (row[x], col[x]) = the tile that
 * linear id t[x] names among the tiles on or above the diagonal of a
 * tiles x tiles grid; the rows (= columns) of pairs per tile. */
void ks_dist_pair_offsets(const int64_t *i, const int64_t *j, int64_t cnt, int64_t m, int64_t *off);
void ks_dist_tiles_of(const int64_t *t, int64_t cnt, int64_t tiles, int64_t *row, int64_t *col);
int32_t ks_dist_tile_rows(void);

/* ---------------------------------------------------------------------
 * Hierarchical clustering of a condensed dissimilarity vector
 * (csrc/ks_hclust.hip).
 * --------------------------------------------------------------------- */

/* The line after dist() in the reference author's analysis (test.R:776,
 * :805): hclust() of the distances, then a cut of the tree into groups of
 * bounded diameter (test.R:826-859) -- without taking the matrix to the host.
 *
 * Input: a condensed dissimilarity vector as ks_spectra_dist_dev writes it,
 * n (n - 1) / 2 doubles, pair i < j at i * n - i (i + 1) / 2 + (j - i - 1)
 * (64-bit offsets).  n >= 2.  Every entry must be finite: a NaN (an empty
 * spectrum row gives one) or an infinity is KS_ERR_ARG, "dissimilarity at
 * offset o is not finite", o the first such offset.  The device entry checks
 * that on the device before anything is modified; after a rejected call the
 * input is untouched and the context usable.
 *
 * Algorithm: the nearest-neighbour-list agglomeration of R's hclust
 * (F. Murtagh's), fixed here in 0-based terms so that a short host loop
 * reproduces it exactly.  State: live[i] (all true), size[i] (all 1.0), the
 * matrix D(i, j), and for i = 0 .. n - 2 the pair nn[i], dnn[i]: nn[i] is the
 * j > i with live[j] that has the smallest D(i, j), scanning j ascending with
 * a strict <, so the lowest j wins a tie; dnn[i] is that value, +inf if no
 * such j exists.  Step s = 0 .. n - 2:
 *   1. im = the live i in 0 .. n - 2 with the smallest dnn[i] (ascending,
 *      strict <: the lowest i wins);
 *   2. jm = nn[im], a = min(im, jm), b = max(im, jm);
 *   3. ia[s] = a, ib[s] = b, height[s] = dnn[im]; live[b] = false;
 *   4. for every live k != a:
 *        complete: D(a, k) = D(b, k) if D(b, k) > D(a, k), else unchanged;
 *        single:   D(a, k) = D(b, k) if D(b, k) < D(a, k), else unchanged;
 *        average:  D(a, k) = (size[a] * D(a, k) + size[b] * D(b, k))
 *                            / (size[a] + size[b]),
 *                  two multiplications, an addition and a division as separate
 *                  FP64 operations (no FMA);
 *   5. size[a] += size[b];
 *   6. nn / dnn are recomputed by the scan above for row a and for every live
 *      i whose nn[i] was a or b, and for no other row.
 * -0.0 and +0.0 compare equal, so the index decides between them.  For
 * complete and single linkage every height has the bits of an input entry.
 * If average linkage overflows until no finite minimum is left the call fails
 * with KS_ERR_ARG.
 *
 * Outputs (host pointers, 16 n bytes in all), as in R's hclust object:
 *   merge  [n - 1][2] int32, row-major.  Observation i (0-based) appears as
 *          -(i + 1), the cluster made at step t (0-based) as t + 1.  Within a
 *          row a singleton comes before a cluster; of two singletons the
 *          smaller observation comes first, of two clusters the earlier step.
 *   height n - 1 doubles in step order.
 *   order  n int32, 1-based: the leaves of the final tree from left to right,
 *          merge[s][0] on the left (R's $order).
 * The step loop, ia / ib and height are device work; the O(n) conversion to
 * merge and order is host code. */
#define KS_HCLUST_COMPLETE 0
#define KS_HCLUST_SINGLE 1
#define KS_HCLUST_AVERAGE 2
#define KS_HCLUST_KEEP_INPUT 1 /* flags: cluster a device copy, leave diss_dev untouched */
typedef struct ks_hclust_stats { /* hipEvent times on the ctx stream, ms */
  double ms_total; /* first check launch to the end of the merge kernel */
  double ms_check; /* the finiteness pass */
  double ms_init;  /* the KEEP_INPUT copy, if any, and the initial nearest-neighbour list */
  double ms_merge; /* the n - 1 steps */
  int64_t n;
  int64_t n_rescans;  /* rows whose nearest neighbour was recomputed after the start (row a of every step included) */
  int64_t work_bytes; /* device memory the call allocated and freed: the KEEP_INPUT copy */
} ks_hclust_stats;

/* diss_dev is a device pointer.  Without KS_HCLUST_KEEP_INPUT it is
 * OVERWRITTEN (the matrix is updated in place); with the flag the call
 * allocates a copy (KS_ERR_NOMEM if it cannot) and the input's bits are
 * unchanged afterwards.  The O(n) state (41 n bytes) comes from the context
 * workspace and is not counted in work_bytes.  All arguments are validated
 * before any device call (n < 2, an unknown method, unknown flag bits, null
 * pointers).  stats may be NULL.  ctx == NULL is the default context on device
 * 0; the calls are never spread over a device list and are not forwarded by
 * the fork broker. */
ks_status ks_hclust_dev(ks_ctx *ctx, double *diss_dev, int64_t n, int32_t method, int32_t flags, int32_t *merge,
                        double *height, int32_t *order, ks_hclust_stats *stats);
/* Host buffers: validates every argument and every entry before any device
 * call, then uploads, runs the device entry on the upload and converts. */
ks_status ks_hclust(ks_ctx *ctx, const double *diss, int64_t n, int32_t method, int32_t *merge, double *height,
                    int32_t *order);
/* Cut the tree into groups: host only, no context.  k in 1 .. n groups, or
 * k = 0 and a height h: k = n - #{s : height[s] <= h}; the heights must then
 * be non-decreasing (KS_ERR_ARG otherwise; height may be NULL when k > 0).
 * The first n - k merges are applied.  group[i] in 1 .. k, numbered in order
 * of first appearance by observation index: observation 0 is in group 1, the
 * next observation not in group 1 opens group 2, and so on.  With complete
 * linkage h bounds every group's diameter. */
ks_status ks_hclust_cut(const int32_t *merge, const double *height, int64_t n, int32_t k, double h, int32_t *group);

/* ---------------------------------------------------------------------
 * Neighbour-joining tree of a condensed dissimilarity vector
 * (csrc/ks_nj.hip).
 * --------------------------------------------------------------------- */

/* The tree the reference's author wanted of the region distances and left
 * commented out as "way too slow" on the host (ape's nj, test.R:770-775,
 * :861-864) -- without taking the matrix to the host.
 *
 * Input: a condensed dissimilarity vector as ks_spectra_dist_dev writes it,
 * n (n - 1) / 2 doubles, pair i < j at i * n - i (i + 1) / 2 + (j - i - 1)
 * (64-bit offsets).  n >= 3.  Every entry must be finite, checked as for
 * ks_hclust_dev and with its error text: KS_ERR_ARG, "dissimilarity at offset
 * o is not finite", o the first such offset, before anything is modified;
 * after a rejected call the input is untouched and the context usable.
 *
 * Algorithm: canonical neighbour joining (Saitou & Nei; Studier & Keppler's
 * criterion), fixed here in 0-based terms so that a short host loop reproduces
 * it exactly.  All arithmetic is separate FP64 operations (no FMA).
 * State: live[i] (all true), r = n, node[i] = -(i + 1), the matrix D(i, j),
 * and S[i] = the sum of D(i, j) over j != i, summed with j ascending in one
 * accumulator started at +0.0.  While r > 3, step s = 0, 1, ...:
 *   1. over the live pairs i < j in lexicographic order
 *        q = ((double)(r - 2) * D(i, j) - S[i]) - S[j];
 *      the smallest q wins with a strict <, so the lowest (i, j) wins a tie
 *      (-0.0 and +0.0 compare equal: the pair decides).  If no pair has
 *      q < +inf (the sums overflowed) the call fails with KS_ERR_ARG;
 *   2. a = i, b = j, dab = D(a, b);
 *        delta = (S[a] - S[b]) / (double)(r - 2);
 *        la = 0.5 * (dab + delta);  lb = 0.5 * (dab - delta);
 *   3. join[s] = (node[a], node[b]), length[s] = (la, lb);
 *   4. for every live k other than a and b, with the old values of D:
 *        dn = 0.5 * ((D(a, k) + D(b, k)) - dab);
 *        S[k] = ((S[k] - D(a, k)) - D(b, k)) + dn;
 *        D(a, k) = dn;
 *   5. S[a] = 0.5 * ((S[a] + S[b]) - (double)r * dab), with the old values of
 *      S: in exact arithmetic the sum of the new row, so nothing is summed;
 *   6. live[b] = false, node[a] = s + 1, r = r - 1.
 * At the end the three live rows x < y < z give
 *   root = (node[x], node[y], node[z]),
 *   root_length = (0.5 * ((D(x,y) + D(x,z)) - D(y,z)),
 *                  0.5 * ((D(x,y) + D(y,z)) - D(x,z)),
 *                  0.5 * ((D(x,z) + D(y,z)) - D(x,y))).
 * Negative lengths are returned as computed.  n = 3 has no join.
 * S is updated incrementally (steps 4 and 5) where ape's nj recomputes the row
 * sums at every step: last bits, and with them the choice among near-ties,
 * may differ from ape's.  The tree is a function of the input alone: the
 * implementation may drop dead rows and columns from the stored matrix as
 * long as the order of the live rows is kept, which changes no comparison and
 * no operand.
 *
 * Outputs (host pointers), coded as merge of ks_hclust: observation i
 * (0-based) appears as -(i + 1), the node made at step t (0-based) as t + 1.
 *   join        [n - 3][2] int32, row-major, in step order
 *   length      [n - 3][2] double: the edges from the step's node to the two
 *   root        [3] int32: the children of the final trifurcation
 *   root_length [3] double */
#define KS_NJ_KEEP_INPUT 1 /* flags: join a device copy, leave diss_dev untouched */
#define KS_NJ_NO_COMPACT 2 /* flags: never compact the matrix (same tree; for measurements) */
typedef struct ks_nj_stats { /* hipEvent times on the ctx stream, ms */
  double ms_total; /* first check launch to the end of the last kernel */
  double ms_check; /* the finiteness pass */
  double ms_init;  /* the KEEP_INPUT copy, if any, and the row sums */
  double ms_join;  /* the n - 3 steps, compactions included, and the root */
  int64_t n;
  int64_t n_compactions; /* times the live rows were copied to a smaller matrix */
  int64_t work_bytes;    /* device memory the call allocated and freed: the KEEP_INPUT copy and the compaction buffer */
} ks_nj_stats;

/* diss_dev is a device pointer.  Without KS_NJ_KEEP_INPUT it is OVERWRITTEN;
 * with the flag the call allocates a copy (KS_ERR_NOMEM if it cannot) and the
 * input's bits are unchanged afterwards.  Compaction: whenever a join leaves
 * r <= m / 2 live rows of the m stored ones (and r >= 8) the live rows are
 * copied, in order, to a matrix of r rows; the copies alternate between the
 * matrix and one buffer of (n / 2)(n / 2 - 1) / 2 doubles, under a quarter of
 * the matrix, allocated when n >= 16 and counted in work_bytes.  The O(n)
 * state (53 n bytes + 32 KiB) comes from the context workspace and is not
 * counted.  All arguments are validated before any device call (n < 3,
 * unknown flag bits, null pointers).  stats may be NULL.  ctx == NULL is the
 * default context on device 0; the calls are never spread over a device list
 * and are not forwarded by the fork broker. */
ks_status ks_nj_dev(ks_ctx *ctx, double *diss_dev, int64_t n, int32_t flags, int32_t *join, double *length,
                    int32_t *root, double *root_length, ks_nj_stats *stats);
/* Host buffers: validates every argument and every entry before any device
 * call, then uploads and runs the device entry on the upload. */
ks_status ks_nj(ks_ctx *ctx, const double *diss, int64_t n, int32_t *join, double *length, int32_t *root,
                double *root_length);
/* The tree as an edge table: host only, no context, O(n).  The layout of
 * ape's phylo object (what the author converts trees to, test.R:824): tips
 * 1 .. n, the trifurcation n + 1, the node of step t as 2n - 2 - t (so
 * n - 2 internal nodes n + 1 .. 2n - 2); edge [2n - 3][2] int32 (parent,
 * child) and edge_length [2n - 3], in preorder from the trifurcation with
 * children in stored order.  join and length may be NULL when n = 3.
 * KS_ERR_ARG for a malformed table: a code that is neither an observation nor
 * (in join[t]) an earlier step, or a node used twice -- a table that leaves a
 * node out uses another twice. */
ks_status ks_nj_edges(const int32_t *join, const double *length, const int32_t *root, const double *root_length,
                      int64_t n, int32_t *edge, double *edge_length);

/* ---------------------------------------------------------------------
 * Silhouette widths, medoids and diameters of a grouping
 * (csrc/ks_silhouette.hip).
 * --------------------------------------------------------------------- */

/* What the reference author's script asks of the groups a tree cut gives
 * (test.R:788-859: which height to cut at, which sequence represents a group,
 * :791, how tight a group is, get.ph.groups' max.dist) -- without taking the
 * matrix to the host: R's cluster::silhouette(cutree(hc, k), d), and with it
 * each group's medoid and diameter.
 *
 * Inputs: diss, a condensed dissimilarity vector of n >= 2 observations as
 * ks_spectra_dist_dev writes it (64-bit offsets).  Every entry must be finite,
 * checked as for ks_hclust_dev and with its error text: KS_ERR_ARG,
 * "dissimilarity at offset o is not finite", o the first such offset.  The
 * vector is never modified.  group, a HOST int32[n] of labels in 1 .. ngroups
 * as ks_hclust_cut writes it.  A label outside the range is KS_ERR_ARG,
 * "group[i] = v is not in 1 .. g", i the first such index.  Empty groups are
 * allowed (ngroups may exceed the largest label); fewer than two non-empty
 * groups is KS_ERR_ARG.  The labels are checked on the host before any device
 * call.
 *
 * Definitions, each a separate FP64 operation (no FMA), so that a short host
 * loop reproduces every output bit for bit:
 *   D(i, j) is the condensed entry of the pair (min, max); D(i, i) = +0.0 and
 *   is added like any other entry, so that the chunk boundaries do not depend
 *   on i.
 *   Group sum.  The members of group c in ascending index order are cut into
 *   chunks of KS_SIL_CHUNK consecutive members.  Chunk partial: P = +0.0, then
 *   P = P + D(i, j) for each member j of the chunk, ascending.  S(i, c) = +0.0,
 *   then S = S + P_q over the chunks q of c, ascending.  (The chunks give the
 *   kernel n / 256 + g independent walks per row instead of g.)
 *   Widths.  n_c is the size of group c, o the group of i.
 *     a(i) = S(i, o) / (double)(n_o - 1), +0.0 when n_o == 1;
 *     mean(i, c) = S(i, c) / (double)n_c for c != o with n_c > 0;
 *     b(i) = the smallest such mean, scanning c ascending with a strict <, so
 *     the lowest label wins a tie; neighbor[i] is that label;
 *     width[i] = 0.0 when n_o == 1; otherwise (b - a) / b if a < b,
 *     (b - a) / a if a > b, and 0.0 if neither holds (a definition of this
 *     library for a == b, no claim about R).
 *   Far.  far(i) = the largest D(i, j) over the members j of o, from +0.0 with
 *   a strict >: exact in any order.
 *   Per group c = 1 .. ngroups, at index c - 1: size = n_c; medoid = the
 *   0-based member with the smallest S(i, c), ascending with a strict <, -1
 *   for an empty group; diameter = the largest far over the members, from +0.0
 *   with a strict >, NaN for an empty group; avg_width = the left-to-right sum
 *   of width over the members, ascending from +0.0, divided by (double)n_c,
 *   NaN for an empty group.
 *   Overall.  avg_width_all = the left-to-right sum of width over all i,
 *   ascending from +0.0, divided by (double)n.
 * Everything that touches the matrix is device work; the O(n) per-group folds
 * are host code on the per-row values.  With complete linkage and groups from
 * ks_hclust_cut(h) every diameter is <= h. */
#define KS_SIL_CHUNK 256
typedef struct ks_silhouette_stats { /* hipEvent times on the ctx stream, ms */
  double ms_total;  /* first check launch to the end of the widths kernel */
  double ms_check;  /* the finiteness pass: one read of the matrix */
  double ms_sums;   /* the chunked group sums, b, neighbor and far of every row */
  double ms_widths; /* a and width of every row */
  int64_t n;
  int64_t ngroups;
  int64_t n_chunks;   /* the sum over the groups of ceil(n_c / KS_SIL_CHUNK) */
  int64_t work_bytes; /* device memory the call works in besides its arguments: the member list, the chunk table and
                         the per-row values, 52 n + 8 n_chunks + 4 ngroups bytes and a few words, taken from the
                         context workspace.  Nothing of size n x ngroups unless sums_dev is given. */
} ks_silhouette_stats;

/* diss_dev is a device pointer and is only read; group is a host pointer.
 * Outputs are host pointers: width, a, b double[n]; neighbor int32[n]; size,
 * medoid int32[ngroups]; diameter, avg_width double[ngroups]; avg_width_all
 * one double.  sums_dev: an optional device buffer [n][ngroups] doubles,
 * row-major, that receives S(i, c) at [i][c - 1] (+0.0 for an empty group);
 * NULL for none.  flags must be 0.  All arguments are validated before any
 * device call (n < 2, flag bits, null pointers, the labels).  If the work
 * memory cannot be allocated the call fails with KS_ERR_NOMEM before anything
 * is written on the device.  stats may be NULL.  ctx == NULL is the default
 * context on device 0; the calls are never spread over a device list and are
 * not forwarded by the fork broker. */
ks_status ks_silhouette_dev(ks_ctx *ctx, const double *diss_dev, int64_t n, const int32_t *group, int32_t ngroups,
                            int32_t flags, double *width, double *a, double *b, int32_t *neighbor, int32_t *size,
                            int32_t *medoid, double *diameter, double *avg_width, double *avg_width_all,
                            double *sums_dev, ks_silhouette_stats *stats);
/* Host buffers: validates every argument and every entry before any device
 * call, then uploads and runs the device entry on the upload.  sums: an
 * optional host buffer [n][ngroups]. */
ks_status ks_silhouette(ks_ctx *ctx, const double *diss, int64_t n, const int32_t *group, int32_t ngroups,
                        int32_t flags, double *width, double *a, double *b, int32_t *neighbor, int32_t *size,
                        int32_t *medoid, double *diameter, double *avg_width, double *avg_width_all, double *sums);

/* ---------------------------------------------------------------------
 * Principal components of region spectra (csrc/ks_pca.hip).
 * --------------------------------------------------------------------- */

/* The other thing the reference's author does with the spectra (test.R:734-736
 * prcomp(x, center=FALSE) of every spectra matrix, "but this is really slow!!";
 * :811 prcomp of the high-entropy subset, centred): the principal components
 * of the row-normalised profiles -- without taking the counts to the host.
 *
 * Input: a spectra matrix as ks_region_spectra_dev writes it, n x ncol uint32,
 * row-major, and an optional int64 row selection as in ks_spectra_dist_dev
 * (any order, repeats allowed; NULL with a count of m means rows 0 .. m - 1,
 * m > n is an error then).  m >= 2.  1 <= ncol <= KS_PCA_MAX_NCOL (q <= 5);
 * 1 <= ncomp <= ncol.  Row s below is position s of the selection.
 * Profile: p[s][c] = (double)cnt / (double)T, T the row sum in 64-bit integers,
 * one IEEE division: the profile of ks_spectra_dist.  A selected row with
 * T = 0 has no profile: KS_ERR_ARG, "row s has no counts", s the first such
 * position.  A bad row index is KS_ERR_ARG, "row index s out of range", s the
 * first such position, and is reported before an empty row.
 * Centre: acc = 0; for s = 0 .. m - 1 ascending: acc = acc + p[s][c];
 * center[c] = acc / (double)m; xc[s][c] = p[s][c] - center[c].  With
 * KS_PCA_NO_CENTER (R's center=FALSE) center is written as zeros and xc = p.
 * Cross-product: G[a][b]: acc = 0; for s ascending: acc = acc + xc[s][a] *
 * xc[s][b], the multiplication and the addition separate FP64 operations (no
 * FMA), one accumulator per entry.  G[a][b] and G[b][a] carry the same bits.
 * So center and G can be predicted bit for bit by a host loop.
 *
 * Eigen-decomposition of G: cyclic two-sided Jacobi in the round-robin
 * (tournament) order.  P = ncol rounded up to even; index P - 1 is a dummy
 * when ncol is odd.  A sweep is the rounds r = 0 .. P - 2; round r holds the
 * P / 2 disjoint pairs of slot 0: (P - 1, r) and slot i = 1 .. P / 2 - 1:
 * ((r + i) mod (P - 1), (r - i) mod (P - 1)), each taken as (p, q) with p < q;
 * the pair holding the dummy is skipped.  (ks_pca_round_pairs lists them.)
 * State: A = G, V = I, floor = 2^-52 * max over c of |G[c][c]|.  For a pair, with
 * app = A[p][p], aqq = A[q][q], apq = A[p][q] read before the round:
 *   skip rule: the pair is skipped (c = 1, s = 0) unless |apq| > floor and
 *     apq * apq > 2^-104 * |app * aqq|.  The second is the usual test relative to
 *     sqrt(|app aqq|); the floor stops the rotation of rounding noise among
 *     the (near-)zero eigenvalues that centring, duplicate columns (column c of
 *     a both-strands spectrum equals column rc(c)), all-zero columns and
 *     m <= ncol leave, where the relative test alone never tires.  An all-zero
 *     G has floor = 0 and every pair is skipped;
 *   rotation: theta = (aqq - app) / (2 apq);
 *     t = 1 / (|theta| + sqrt(theta * theta + 1)), negated if theta < 0
 *     (theta = 0, the duplicate-column case, gives t = 1);
 *     c = 1 / sqrt(t * t + 1);  s = t * c.
 * All the round's rotations J (J[p][p] = J[q][q] = c, J[p][q] = s, J[q][p] =
 * -s) are applied at once, A <- J^T A J and V <- V J: an entry A[i][j] with i in
 * pair k1 and j in pair k2 (slots k1 < k2) first takes pair k2's column step
 *   (x_ip, x_iq) <- (c x_ip - s x_iq, s x_ip + c x_iq),
 * then pair k1's row step of the same form, and is stored at [i][j] and [j][i]
 * (A stays symmetric in bits); a pair's own block is set in closed form, A[p][p]
 * = app - t apq, A[q][q] = aqq + t apq, A[p][q] = A[q][p] = 0; V's columns p and
 * q take the column step.  A block or a row of V none of whose pairs rotates is
 * left as it is.
 * Termination: the loop ends with the first sweep in which no pair is rotated
 * (n_sweeps counts that sweep too: an all-zero G ends with n_sweeps = 1,
 * n_rotations = 0).  Every rotation removes 2 apq^2 > 2 floor^2 from the
 * off-diagonal norm, so the loop ends; more than KS_PCA_MAX_SWEEPS sweeps is
 * KS_ERR_INTERNAL.  lambda[j] = A[j][j], its vector is column j of V.  This
 * stage uses sqrt and division: its bits are not promised, its error is
 * (DESIGN.md 6k).
 * Order and sign: components by lambda descending, equal values in Jacobi
 * column order.  Each loading vector is negated if needed so that its entry
 * of largest absolute value is positive; among equal absolute values the
 * lowest index decides.
 *
 * Outputs:
 *   center   ncol doubles.
 *   sdev     ncol doubles, sdev[j] = sqrt(max(lambda_j, 0) / (double)(m - 1)):
 *            R's sdev (prcomp divides by m - 1 without centring too).
 *   rotation ncol x ncomp doubles, row-major: component j is column j.  The
 *            first k columns of any call are the bits of the first k columns
 *            of the full call (ncomp = ncol).
 *   x        m x ncomp doubles, row-major, may be NULL: the scores, x[s][j]:
 *            acc = 0; for c = 0 .. ncol - 1 ascending: acc = acc + xc[s][c] *
 *            rotation[c][j], separate operations, one accumulator per entry:
 *            predictable bit for bit from the returned center and rotation.
 *   gram     ncol x ncol doubles, may be NULL: G.
 * The result is a function of the input alone, with the same bits on every
 * run: no atomics on doubles, no reduction that depends on arrival order.
 * ctx == NULL is the default context on device 0; the calls are never spread
 * over a device list and are not forwarded by the fork broker. */
#define KS_PCA_MAX_NCOL 1024
#define KS_PCA_MAX_SWEEPS 64
#define KS_PCA_NO_CENTER 1
typedef struct ks_pca_stats { /* hipEvent times on the ctx stream, ms */
  double ms_total;
  double ms_normalise; /* check, profiles, centre */
  double ms_gram;
  double ms_eigen;     /* Jacobi (its read-backs included), order and sign */
  double ms_project;
  int64_t n_sweeps;
  int64_t n_rotations;
  int64_t panel_bytes; /* device memory the call allocated and freed: the m x ncol FP64 panel and three P x P matrices */
} ks_pca_stats;

/* Device-resident: spectra_dev, rows_dev and the five outputs are device
 * pointers.  Indices and row sums are checked on the device before any output
 * is written: after a rejected call the outputs are untouched and the context
 * usable.  The only allocation is the work memory counted in panel_bytes
 * (KS_ERR_NOMEM if it fails), freed before return.  All other arguments are
 * validated before any device call.  stats may be NULL. */
ks_status ks_spectra_pca_dev(ks_ctx *ctx, const uint32_t *spectra_dev, int64_t n, int32_t ncol,
                             const int64_t *rows_dev, int64_t m, int32_t flags, int32_t ncomp, double *center_dev,
                             double *sdev_dev, double *rotation_dev, double *x_dev, double *gram_dev,
                             ks_pca_stats *stats);
/* Host buffers: validates every argument, every index and every row sum
 * before any device call, then uploads, runs the device entry and copies the
 * results back. */
ks_status ks_spectra_pca(ks_ctx *ctx, const uint32_t *spectra, int64_t n, int32_t ncol, const int64_t *rows,
                         int64_t m, int32_t flags, int32_t ncomp, double *center, double *sdev, double *rotation,
                         double *x, double *gram);
/* The Jacobi schedule on the host: the pairs of round `round` (0 .. P - 2) of
 * ncol columns in slot order, p[i] < q[i], the dummy's pair left out; p and q
 * hold P / 2 entries.  Returns the pair count, -1 for a bad argument. */
int32_t ks_pca_round_pairs(int32_t ncol, int32_t round, int32_t *p, int32_t *q);

/* ---------------------------------------------------------------------
 * Lloyd k-means and group mean spectra of region spectra
 * (csrc/ks_kmeans.hip).
 * --------------------------------------------------------------------- */

/* Every other way of grouping regions here goes through the condensed distance
 * matrix (ks_spectra_dist -> ks_hclust / ks_nj -> ks_hclust_cut ->
 * ks_silhouette), n(n-1)/2 doubles.  These entries work on the counts: the mean
 * spectrum of every group of a labelling, and R's kmeans(x, centers, iter.max,
 * algorithm = "Lloyd") on the row-normalised profiles, in O((m + g) ncol)
 * memory, with nothing of size m x g or m x m.
 *
 * Input: a spectra matrix as ks_region_spectra_dev writes it, n x ncol uint32,
 * row-major, 1 <= ncol <= KS_DIST_MAX_NCOL, and an optional int64 row selection
 * as in ks_spectra_pca_dev (any order, repeats allowed; NULL with a count of m
 * means rows 0 .. m - 1, m > n is an error then).  m >= 1.  Row s below is
 * position s of the selection.
 * Profile: p[s][c] = (double)cnt / (double)T, T the row sum in 64-bit integers,
 * one IEEE division: the profile of ks_spectra_dist.  A selected row with
 * T = 0 is KS_ERR_ARG, "row s has no counts"; a bad index is KS_ERR_ARG, "row
 * index s out of range"; each names the first such position, and the index
 * error is reported before the empty row.
 *
 * Definitions, each a separate FP64 operation (no FMA), so that a short host
 * loop reproduces every output bit for bit:
 *   Squared distance of row s and centre j: acc = +0.0; for c ascending:
 *   d = p[s][c] - cen[j][c]; acc = acc + d * d.  One accumulator per (s, j): the
 *   inner loop of ks_spectra_dist.  Where cen[j] is the profile of a row r the
 *   value carries the bits of ks_spectra_cross_dist(..., KS_DIST_SQUARED) for
 *   (s, r).  (No Gram form, no MFMA: see csrc/ks_spectra_dist.hip.)
 *   Assignment: label[s] = the j with the smallest acc, scanning j ascending
 *   from +inf with a strict <, so the lowest label wins a tie.  Labels are
 *   1 .. g, as ks_hclust_cut writes them.
 *   Group sum of a value v(s) over group j: the members of j in ascending
 *   position order are cut into chunks of KS_KM_CHUNK consecutive members.
 *   Chunk partial: P = +0.0, then P = P + v(s) over the chunk's members,
 *   ascending.  S = +0.0, then S = S + P_q over the chunks, ascending.  (The
 *   order of ks_silhouette's sums.)
 *   Centre: cen[j][c] = S_j[c] / (double)n_j with v(s) = p[s][c], n_j the size.
 *   In k-means a group without members keeps the bits of its previous centre
 *   (a definition of this library: R stops with "empty cluster"); in the
 *   group-means entries it gets a row of NaN.
 *   withinss[j] = the group sum with v(s) = acc(s, j) against the returned
 *   centres, +0.0 for an empty group.  tot_withinss = the left-to-right sum of
 *   withinss over j from +0.0.  totss = the same two definitions for the
 *   single group of all m rows: its chunked centre, then its chunked sum.
 *   Loop (R's kmeans_Lloyd): the labels start at 0.  For iter = 1 .. iter_max:
 *   assign; if no label changed, stop with converged = 1; otherwise recompute
 *   every centre.  iter is the number of assignment passes run.  After the
 *   iter_max-th pass the centres are still updated, so, as in R, the labels of
 *   a run that did not converge need not be the nearest centres of the
 *   returned centres; withinss uses the returned labels and centres always.
 * Initial centres: exactly one of init (g x ncol doubles, row-major; every
 * entry finite, otherwise KS_ERR_ARG, "center[j][c] is not finite", the first
 * such entry in row-major order) and init_rows (g int64 positions into the
 * selection: the centre is that row's profile, bit for bit; a position outside
 * 0 .. m - 1 is KS_ERR_ARG, "initial row index j out of range", the first such
 * j).  Neither or both is KS_ERR_ARG.  Duplicate centres are allowed: the tie
 * rule decides.  1 <= g <= KS_KM_MAX_GROUPS; g > m is allowed; iter_max >= 1;
 * flags must be 0.
 * The result is a function of the input alone, with the same bits on every
 * run: no atomics on doubles, no reduction that depends on arrival order. */
#define KS_KM_CHUNK 256
#define KS_KM_MAX_GROUPS 65536
typedef struct ks_kmeans_result {
  int32_t iter;        /* assignment passes run */
  int32_t converged;   /* 1: the last pass changed no label */
  double tot_withinss;
  double totss;
} ks_kmeans_result;
typedef struct ks_kmeans_stats { /* hipEvent times on the ctx stream, ms */
  double ms_total;
  double ms_normalise; /* checks, profiles, initial centres */
  double ms_assign;    /* summed over the passes (each with its 4-byte read-back queued behind it) */
  double ms_update;    /* member list and centres, summed over the passes; group means: the one update */
  double ms_wss;       /* withinss, and totss in k-means */
  int64_t n_iter;
  int64_t panel_bytes; /* the m x ncol FP64 profile panel */
  int64_t work_bytes;  /* the rest of the call's one allocation: chunk partials ((m / 256 + g) x ncol doubles), the
                          member list and sort buffers (O(m)), the split minima of the assignment (12 m bytes
                          per split; splits only while there are fewer than 32 workgroups per CU) and O(g) tables.  Allocated and freed by the call. */
} ks_kmeans_stats;

/* Device-resident: spectra_dev, rows_dev, init_dev, init_rows_dev, cluster_dev
 * (int32[m]) and centers_dev (double[g * ncol]) are device pointers; size
 * (int32[g]), withinss (double[g]) and res are host pointers.  centers_dev may
 * be the same buffer as init_dev.  Indices, row sums and centres are checked
 * on the device before any output is written: after a rejected call the
 * outputs are untouched and the context usable.  The only allocation is the
 * work memory counted in panel_bytes + work_bytes (KS_ERR_NOMEM if it fails),
 * freed before return.  All other arguments are validated before any device
 * call.  One 4-byte read-back per pass is the loop's only host round trip.
 * stats may be NULL.  ctx == NULL is the default context on device 0; the
 * calls are never spread over a device list and are not forwarded by the fork
 * broker. */
ks_status ks_spectra_kmeans_dev(ks_ctx *ctx, const uint32_t *spectra_dev, int64_t n, int32_t ncol,
                                const int64_t *rows_dev, int64_t m, const double *init_dev,
                                const int64_t *init_rows_dev, int32_t g, int32_t iter_max, int32_t flags,
                                int32_t *cluster_dev, double *centers_dev, int32_t *size, double *withinss,
                                ks_kmeans_result *res, ks_kmeans_stats *stats);
/* Host buffers: validates every argument, every index, every row sum and every
 * centre before any device call, then uploads, runs the device entry and
 * copies the results back. */
ks_status ks_spectra_kmeans(ks_ctx *ctx, const uint32_t *spectra, int64_t n, int32_t ncol, const int64_t *rows,
                            int64_t m, const double *init, const int64_t *init_rows, int32_t g, int32_t iter_max,
                            int32_t flags, int32_t *cluster, double *centers, int32_t *size, double *withinss,
                            ks_kmeans_result *res);
/* The update and the withinss step as an entry of their own (the bridge from
 * ks_hclust_cut): group is a HOST int32[m] of labels in 1 .. ngroups, checked
 * on the host before any device call with the text of ks_silhouette ("group[i]
 * = v is not in 1 .. g"); 1 <= ngroups <= KS_KM_MAX_GROUPS; empty groups are
 * allowed (a NaN row, size 0, withinss +0.0) and one non-empty group is enough.
 * centers_dev: double[ngroups * ncol] on the device; size, withinss: host. */
ks_status ks_spectra_group_means_dev(ks_ctx *ctx, const uint32_t *spectra_dev, int64_t n, int32_t ncol,
                                     const int64_t *rows_dev, int64_t m, const int32_t *group, int32_t ngroups,
                                     int32_t flags, double *centers_dev, int32_t *size, double *withinss,
                                     ks_kmeans_stats *stats);
ks_status ks_spectra_group_means(ks_ctx *ctx, const uint32_t *spectra, int64_t n, int32_t ncol, const int64_t *rows,
                                 int64_t m, const int32_t *group, int32_t ngroups, int32_t flags, double *centers,
                                 int32_t *size, double *withinss);

/* ---------------------------------------------------------------------
 * Starts for ks_spectra_kmeans: maximin and k-means++ seeding
 * (csrc/ks_kmeans_seed.hip).
 * --------------------------------------------------------------------- */

/* ks_spectra_kmeans takes its initial centres from the caller.  These entries
 * choose g rows of the selection as centres, in O(m ncol) memory and g
 * dependent steps, each one pass "distance of every row to one centre" over
 * the profile panel; nothing of size m x g exists.  rows_out is what init_rows
 * of ks_spectra_kmeans_dev takes.
 *   KS_SEED_MAXIMIN: farthest-first traversal (Gonzalez' 2-approximation of
 *   k-centre): every pick is the row farthest from the rows picked so far.  No
 *   random numbers; pick_dist[j] is the squared covering radius of the first j
 *   picks, a curve over the number of groups.
 *   KS_SEED_DSQ: k-means++ (D^2 sampling, one candidate per step).  The
 *   uniform numbers come from the caller: the library has no generator and the
 *   result is a function of (spectra, rows, g, first, u) alone.
 *
 * Input, profile and their errors: those of ks_spectra_kmeans above (n x ncol
 * uint32 spectra, 1 <= ncol <= KS_DIST_MAX_NCOL, an optional int64 selection of
 * m >= 1 rows in any order, repeats allowed; "row index s out of range" is
 * reported before "row s has no counts").  1 <= g <= KS_KM_MAX_GROUPS; g > m is
 * allowed.  Row s below is position s of the selection.
 *
 * Definitions, each a separate FP64 operation (no FMA):
 *   Squared distance acc(s, r) of row s and picked row r: that of
 *   ks_spectra_kmeans with cen = the profile of row r, bit for bit: acc = +0.0;
 *   for c ascending: d = p[s][c] - p[r][c]; acc = acc + d * d.  It carries the
 *   bits of ks_spectra_cross_dist(..., KS_DIST_SQUARED) for (s, r), and
 *   acc(r, r) is exactly +0.0.
 *   State: mind[s] = +inf and near[s] = 0 for every s.
 *   Step j = 0 .. g - 1: a row r_j is picked (below) and rows_out[j] = r_j.
 *   Then for every s: if acc(s, r_j) < mind[s] (strict), mind[s] = acc(s, r_j)
 *   and near[s] = j + 1.  The lowest label keeps a tie, as in the assignment
 *   of ks_spectra_kmeans.
 *   Potential: pot = the chunked sum of mind over all rows: the rows in
 *   ascending position are cut into chunks of KS_KM_CHUNK; C[c] = the chunk's
 *   left-to-right sum from +0.0; P[0] = +0.0, P[c + 1] = P[c] + C[c];
 *   pot = P[nchunks].  (The group sum of ks_spectra_kmeans for the single
 *   group of all rows.)
 *   Pick of step 0: `first` if 0 <= first < m.  first = -1 is allowed only
 *   with KS_SEED_DSQ and means (int64)(u[0] * (double)m).  Any other first is
 *   KS_ERR_ARG.  pick_dist[0] = potential[0] = +inf.
 *   Pick of step j >= 1, KS_SEED_MAXIMIN: the s with the largest mind[s], the
 *   lowest position on a tie.  pick_dist[j] = mind[s], potential[j] = pot.
 *   Pick of step j >= 1, KS_SEED_DSQ: t = u[j] * pot (one multiplication).
 *   c* = the first chunk with P[c* + 1] > t.  Inside it acc = +0.0 and for s
 *   ascending acc = acc + mind[s]; the pick is the first s with
 *   P[c*] + acc > t (one addition for the comparison).  pick_dist[j] =
 *   mind[s], potential[j] = pot.  At the chunk's last row acc is C[c*] and
 *   the test is P[c* + 1] > t, so a row is always found; P[c*] <= t and acc
 *   does not move on a zero, so the picked row has mind > 0; u[j] * pot < pot
 *   for 0 <= u[j] <= 1 - 2^-53, so the chunk exists.
 *   Degenerate picks: when pot == +0.0 (KS_SEED_DSQ) or the largest mind is
 *   +0.0 (KS_SEED_MAXIMIN) every row coincides with a picked one: the pick is
 *   position 0 and pick_dist[j] = +0.0.
 *   (pick_dist and potential of step j are taken BEFORE the update of step j.)
 * The uniforms: u is a host array of g doubles, required with KS_SEED_DSQ and
 * NULL with KS_SEED_MAXIMIN (u[0] is used only by first = -1).  Every entry
 * must satisfy 0 <= u < 1, otherwise KS_ERR_ARG, "u[j] is not in [0, 1)", the
 * first such j, before any device call.
 * Result: n_distinct = 1 + the number of j >= 1 with pick_dist[j] > 0;
 * potential = pot after the last step; radius and far_row = the largest mind
 * after the last step and its lowest position: the squared covering radius,
 * the value the next maximin pick would have had.
 * The result is a function of the input alone, with the same bits on every
 * run: no atomics on doubles, no reduction that depends on arrival order. */
#define KS_SEED_MAXIMIN 0
#define KS_SEED_DSQ 1
typedef struct ks_seed_result {
  int32_t n_distinct;
  int32_t reserved;
  double potential;
  double radius;
  int64_t far_row;
} ks_seed_result;
typedef struct ks_seed_stats { /* hipEvent times on the ctx stream, ms */
  double ms_total;
  double ms_normalise; /* checks and profiles, with the one read-back before the first step */
  double ms_steps;     /* the g picks and updates and the closing reduction, queued back to back */
  int64_t n_launches;  /* kernels launched by the call */
  int64_t panel_bytes; /* the m x ncol FP64 profile panel */
  int64_t work_bytes;  /* the rest of the call's one allocation: three records per chunk of 256 rows, the
                          chunk prefix, the uniforms and the two host-bound sequences (O(g)).  Allocated and
                          freed by the call. */
} ks_seed_stats;

/* Device-resident: spectra_dev, rows_dev, rows_out_dev (int64[g], positions
 * into the selection), near_dev (int32[m]) and mind_dev (double[m], squared)
 * are device pointers; u, pick_dist (double[g]), potential (double[g]) and res
 * are host pointers.  flags: KS_SEED_MAXIMIN or KS_SEED_DSQ.  Indices and row
 * sums are checked on the device and one read-back ends a rejected call before
 * the first step: the outputs are untouched then and the context usable.  All
 * other arguments are validated before any device call.  The g steps are
 * queued without a host round trip; one read-back at the end brings pick_dist,
 * potential and the result.  The only allocation is the work memory counted in
 * panel_bytes + work_bytes (KS_ERR_NOMEM if it fails), freed before return.
 * stats may be NULL.  ctx == NULL is the default context on device 0; the
 * calls are never spread over a device list and are not forwarded by the fork
 * broker. */
ks_status ks_spectra_kmeans_seed_dev(ks_ctx *ctx, const uint32_t *spectra_dev, int64_t n, int32_t ncol,
                                     const int64_t *rows_dev, int64_t m, int32_t g, int32_t flags, int64_t first,
                                     const double *u, int64_t *rows_out_dev, int32_t *near_dev, double *mind_dev,
                                     double *pick_dist, double *potential, ks_seed_result *res,
                                     ks_seed_stats *stats);
/* Host buffers: validates every argument, every index and every row sum before
 * any device call, then uploads, runs the device entry and copies the results
 * back. */
ks_status ks_spectra_kmeans_seed(ks_ctx *ctx, const uint32_t *spectra, int64_t n, int32_t ncol, const int64_t *rows,
                                 int64_t m, int32_t g, int32_t flags, int64_t first, const double *u,
                                 int64_t *rows_out, int32_t *near, double *mind, double *pick_dist,
                                 double *potential, ks_seed_result *res);

/* ---------------------------------------------------------------------
 * k nearest regions by spectrum, without the distance matrix
 * (csrc/ks_knn.hip).
 * --------------------------------------------------------------------- */

/* For every selected row, the k rows of a candidate selection nearest to it
 * in ks_spectra_dist's metric, in O((na + nb) ncol + na k) memory: nothing of
 * size na x nb is written or sorted.
 *
 * Input: a spectra matrix as ks_region_spectra_dev writes it, n x ncol uint32,
 * row-major, 1 <= ncol <= KS_DIST_MAX_NCOL.
 * Queries: an optional int64 selection `rows` of na >= 1 row indices (any
 * order, repeats allowed; NULL with a count of na means rows 0 .. na - 1,
 * na > n is an error then).  Query s below is position s of that selection.
 * Candidates: an optional int64 selection `rows_b` of nb >= 1 row indices.
 *   Self form (rows_b NULL; nb is ignored): the candidates are the query
 *   selection itself, and position s is left out of the list of query s.  The
 *   exclusion is by POSITION, not by row index: a row named twice finds its
 *   other copy at a distance of exactly 0.  There are na - 1 candidates.
 *   Cross form: every one of the nb candidates counts.
 * 1 <= k <= KS_KNN_MAX_K, and k may not exceed the number of candidates
 * (na - 1 or nb).  flags: 0 or KS_DIST_SQUARED.
 *
 * Errors of the selections are KS_ERR_ARG, each names the first offending
 * position, and they take precedence in this order:
 *   1. "row index s out of range" (the queries, then the candidates: "row
 *      index s of the second selection out of range");
 *   2. "row s has no counts" (the queries, then "row s of the second selection
 *      has no counts"): an empty row has no profile and is refused, as in
 *      ks_spectra_kmeans;
 *   3. "k exceeds the number of candidate rows".
 * Any of them is raised before an output byte is written.
 *
 * Distance: the profile is p[c] = (double)cnt / (double)T, T the row sum in
 * 64-bit integers.  For query a and candidate b: acc = +0.0; for c ascending:
 * d = p_a[c] - p_b[c]; acc = acc + d * d, each a separate FP64 operation (no
 * FMA), one accumulator per pair: acc has the bits of ks_spectra_cross_dist(
 * ..., KS_DIST_SQUARED) for the pair.  (No Gram form, no MFMA: see
 * csrc/ks_spectra_dist.hip.)
 * Selection: the k candidates with the smallest (acc, position) pairs in
 * lexicographic order, ascending; position is the candidate's position in its
 * selection.  The comparison is made on acc, the squared value, before any
 * root is taken (two different acc can share a square root).  acc is never
 * -0.0 or NaN, so this is a total order and the result is a function of the
 * input alone: no tile shape, grid or split of the candidates shows in it, and
 * a host sort of (acc, position) predicts every output.
 * Outputs, row-major, column 0 the nearest:
 *   index: int64 [na][k], 0-based positions into the candidate selection (not
 *          row indices);
 *   dist:  double [na][k], acc with KS_DIST_SQUARED, otherwise sqrt(acc).
 *
 * Metrics: flags takes the metric field of ks_spectra_dist (KS_DIST_METRIC_MASK),
 * with the same checks, directly after the check of unknown flags.  The list
 * is ordered by (value, position) as above.  The value is acc for euclidean
 * and hellinger (the Euclidean loop over the rooted profiles; dist is then
 * 0.5 * acc or sqrt(0.5 * acc)), and the returned distance for manhattan,
 * maximum and canberra -- for canberra the result scaled by ncol / cnt.  Every
 * value is non-negative and no NaN occurs (empty rows are refused).  Every
 * returned distance carries the bits of ks_spectra_cross_dist with the same
 * flags for that pair. */
#define KS_KNN_MAX_K 64
typedef struct ks_knn_stats { /* hipEvent times on the ctx stream, ms */
  double ms_total;
  double ms_normalise;     /* checks and profiles, with the one read-back */
  double ms_select;        /* k_knn_select */
  double ms_merge;         /* k_knn_merge; 0 with one split */
  int64_t n_splits;        /* parts the candidate tiles were cut into (grid y of the selection) */
  int64_t tiles_per_split; /* candidate tiles of 64 per split; the last split may hold fewer */
  int64_t panel_bytes;     /* the FP64 profile panel: na x ncol, and nb x ncol more in the cross form */
  int64_t work_bytes;      /* the rest of the call's one allocation: with more than one split the splits'
                              lists, 12 bytes x na x k x n_splits.  Allocated and freed by the call. */
} ks_knn_stats;

/* Device-resident: spectra_dev, rows_dev, rows_b_dev, index_dev (int64
 * [na * k]) and dist_dev (double [na * k]) are device pointers.  Indices and
 * row sums are checked on the device and one read-back ends a rejected call
 * before any output is written: the outputs are untouched then and the
 * context usable.  The only allocation is the work memory counted in
 * panel_bytes + work_bytes (KS_ERR_NOMEM if it fails), freed before return.
 * All other arguments are validated before any device call.  stats may be
 * NULL.  ctx == NULL is the default context on device 0; the call is never
 * spread over a device list and is not forwarded by the fork broker. */
ks_status ks_spectra_knn_dev(ks_ctx *ctx, const uint32_t *spectra_dev, int64_t n, int32_t ncol,
                             const int64_t *rows_dev, int64_t na, const int64_t *rows_b_dev, int64_t nb, int32_t k,
                             int32_t flags, int64_t *index_dev, double *dist_dev, ks_knn_stats *stats);
/* Host buffers: validates every argument, every index and every row sum before
 * any device call, then uploads, runs the device entry and copies the results
 * back. */
ks_status ks_spectra_knn(ks_ctx *ctx, const uint32_t *spectra, int64_t n, int32_t ncol, const int64_t *rows,
                         int64_t na, const int64_t *rows_b, int64_t nb, int32_t k, int32_t flags, int64_t *index,
                         double *dist);

/* Scan algorithm selection (testing/benchmarking): -1 auto, 0 lane-per-run,
 * 1 chunked carry scan. */
ks_status ks_ctx_set_scan_algo(ks_ctx *ctx, int32_t algo);

#ifdef __cplusplus
}
#endif
#endif /* KMER_SPANS_H */
