// ks_spectra_dist.hip -- pairwise Euclidean distances between row-normalised
// region spectra (ks_spectra_dist / ks_spectra_cross_dist and their _dev
// forms, include/kmer_spans.h).
//
// What the reference's author does with the spectra next (test.R:762-807):
// dist(reg.kmer.sp[[1]]) over all 24,611 regions and over a row subset, then
// clustering.  Here the spectra stay in HBM as ks_region_spectra_dev wrote
// them; the input is that n x ncol uint32 matrix and optional row selections.
//
// The result is fixed as an order of operations (the header comment):
// p[k] = (double)c[k] / (double)T with T the row's 64-bit integer sum, then per
// pair acc = 0; for k ascending: d = p_i[k] - p_j[k]; acc = acc + d * d, every
// operation a separate FP64 instruction (-ffp-contract=off, csrc/Makefile), one
// accumulator per pair.  So the bits do not depend on tile shape or grid, a
// host loop predicts them, d(i, j) = d(j, i), d(i, i) = 0, and rows with
// proportional counts are at exactly 0 (the correctly rounded division gives
// both the same p).  The Gram form |a|^2 + |b|^2 - 2ab, and with it MFMA, is
// deliberately not used: it cancels for near-equal rows, which is what repeats
// of one unit at different lengths are.
//
// Check:     k_dist_check tests every selected row index against n before
//            anything is written; one 16-byte read-back ends a call with a bad
//            index there.
// Normalise: k_dist_normalise gathers 64 selected rows per block, sums each in
//            uint64 (a wave per row, lanes along the columns) and writes the
//            FP64 panel K-MAJOR: panel[k * ld + s], s the position in the
//            selection.  The counts pass through LDS so that both the reads
//            (along k) and the writes (along s) are coalesced.
// Distance:  k_dist_tile: a block of 256 threads owns a 64 x 64 tile of pairs,
//            a thread a 4 x 4 register block of accumulators.  Chunks of 16 k
//            of both row sets are staged in LDS ([k][64 rows]: the k-major
//            panel makes that a coalesced 512-byte load per k and a
//            conflict-free LDS write) and reused by every pair of the tile.
//            The condensed form launches the T(T + 1)/2 tiles on or above the
//            diagonal as a linear grid (ks_dist_index.h); diagonal tiles mask
//            i >= j; ragged edges are masked, no load leaves the panel.
// Metrics:   bits 8 .. 11 of flags (KS_DIST_METRIC_MASK).  The
//            distance kernel is a template on the metric and takes its
//            per-column step and its last step from ks_dist_metric.h; the
//            Euclidean instantiation is the kernel described above.  Hellinger
//            is that loop over a panel of roots (k_dist_normalise<true>) and a
//            final 0.5 *; canberra keeps a count per pair next to acc; the
//            maximum reads both rows' first panel entry in its last step,
//            because the hardware maximum drops the NaN of an empty row.
#include <cmath>
#include <cstring>

#include "ks_panel.h"
// after hip_runtime.h (ks_internal.h): the header's functions are __host__ __device__ here
#include "ks_dist_index.h"
#include "ks_dist_metric.h"

namespace ks {
namespace {

constexpr int kDT = 64;        // tile edge (pairs)
constexpr int kDK = 16;        // k per LDS chunk: 2 x 16 x 64 x 8 B = 16 KiB per block
constexpr int kDThreads = 256; // 16 x 16 threads, 4 x 4 pairs each
#ifdef KS_DIST_NAIVE
constexpr int kNaive = 16;     // comparison build: 16 x 16 pairs per block, one per thread
constexpr int64_t kEdge = kNaive;
#else
constexpr int64_t kEdge = kDT; // pairs along a block's edge
#endif

__global__ void __launch_bounds__(256) k_dist_check(const int64_t *__restrict__ rows, int64_t cnt, int64_t n,
                                                    unsigned long long *__restrict__ bad) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= cnt) return;
  const int64_t r = rows[s];
  if (r < 0 || r >= n) atomicMax(bad, (unsigned long long)(cnt - s));
}

// Rows [s0, s0 + 64) of a selection (rows == nullptr: the rows themselves) ->
// panel[k * ld + poff + s], k-major.  kRoot: the entry is sqrt(p), the Hellinger panel.
template <bool kRoot>
__global__ void __launch_bounds__(256) k_dist_normalise(const uint32_t *__restrict__ sp, int ncol,
                                                        const int64_t *__restrict__ rows, int64_t cnt,
                                                        double *__restrict__ panel, int64_t ld, int64_t poff) {
  __shared__ double tot[kDT];
  __shared__ int64_t ridx[kDT];
  __shared__ uint32_t tile[kDT][kDT + 1];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t s0 = (int64_t)blockIdx.x * kDT;
  for (int rr = wv; rr < kDT; rr += 4) {
    const int64_t s = s0 + rr;
    if (s >= cnt) continue;  // wave-uniform
    const int64_t r = rows ? rows[s] : s;
    const uint32_t *row = sp + (size_t)r * ncol;
    unsigned long long t = 0;
    for (int c = lane; c < ncol; c += 64) t += row[c];
    for (int d = 32; d > 0; d >>= 1) t += __shfl_xor(t, d);
    if (lane == 0) {
      tot[rr] = (double)t;  // below 2^44: exact
      ridx[rr] = r;
    }
  }
  __syncthreads();
  for (int c0 = 0; c0 < ncol; c0 += kDT) {
    for (int rr = wv; rr < kDT; rr += 4) {
      const int c = c0 + lane;
      tile[rr][lane] = (s0 + rr < cnt && c < ncol) ? sp[(size_t)ridx[rr] * ncol + c] : 0u;
    }
    __syncthreads();
    for (int kk = wv; kk < kDT; kk += 4) {
      const int k = c0 + kk;
      if (k < ncol && s0 + lane < cnt) {
        const double p = (double)tile[lane][kk] / tot[lane];  // 0 / 0 = NaN: an empty row
        panel[(size_t)k * ld + poff + s0 + lane] = kRoot ? sqrt(p) : p;
      }
    }
    __syncthreads();
  }
}

// Pair (i, j) = (row a0 + i of the panel, row b0 + j of the panel), i < ma,
// j < mb.  kCondensed: a0 = b0 = 0, ma = mb = m, blockIdx.x is a linear id over
// the tiles on or above the diagonal, only i < j is stored, at
// dist_pair_offset.  Otherwise blockIdx.x = tile row * tiles_b + tile column
// and the output is the dense ma x mb block.  M: the metric (ks_dist_metric.h); the
// panel holds the roots for hellinger.
template <int M, bool kCondensed>
__global__ void __launch_bounds__(kDThreads) k_dist_tile(const double *__restrict__ panel, int64_t ld, int ncol,
                                                         int64_t a0, int64_t ma, int64_t b0, int64_t mb, int64_t tiles_b,
                                                         int squared, double *__restrict__ out) {
  __shared__ __attribute__((aligned(16))) double As[kDK][kDT];
  __shared__ __attribute__((aligned(16))) double Bs[kDK][kDT];
  int64_t tr, tc;
  if (kCondensed) {
    dist_tile_of((int64_t)blockIdx.x, tiles_b, &tr, &tc);
  } else {
    tr = (int64_t)blockIdx.x / tiles_b;
    tc = (int64_t)blockIdx.x - tr * tiles_b;
  }
  const int64_t i0 = tr * kDT, j0 = tc * kDT;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  double acc[4][4];
  int cnt[4][4];  // canberra's columns kept; no register in the other metrics
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[r][e] = 0.0, cnt[r][e] = 0;

  for (int k0 = 0; k0 < ncol; k0 += kDK) {
    const int kc = min(kDK, ncol - k0);
#pragma unroll
    for (int e = 0; e < kDK * kDT / kDThreads; ++e) {
      const int idx = tid + kDThreads * e;
      const int kk = idx >> 6, r = idx & 63;
      const bool in_k = kk < kc;
      const size_t base = (size_t)(k0 + kk) * ld;
      As[kk][r] = (in_k && i0 + r < ma) ? panel[base + a0 + i0 + r] : 0.0;
      Bs[kk][r] = (in_k && j0 + r < mb) ? panel[base + b0 + j0 + r] : 0.0;
    }
    __syncthreads();
    if (kc == kDK) {
#pragma unroll
      for (int kk = 0; kk < kDK; ++kk) {
        double a[4], b[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) a[r] = As[kk][ty * 4 + r];
#pragma unroll
        for (int e = 0; e < 4; ++e) b[e] = Bs[kk][tx + 16 * e];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int e = 0; e < 4; ++e) metric_step<M>(acc[r][e], cnt[r][e], a[r], b[e]);
      }
    } else {
      for (int kk = 0; kk < kc; ++kk) {
        double a[4], b[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) a[r] = As[kk][ty * 4 + r];
#pragma unroll
        for (int e = 0; e < 4; ++e) b[e] = Bs[kk][tx + 16 * e];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int e = 0; e < 4; ++e) metric_step<M>(acc[r][e], cnt[r][e], a[r], b[e]);
      }
    }
    __syncthreads();
  }

  // stores run along j: 16 lanes write 128 contiguous bytes of one output row
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t i = i0 + ty * 4 + r;
    if (i >= ma) continue;
    // maximum: a row without counts is NaN in every column, so its first entry tells
    double nan_i = 0.0;
    if constexpr (M == KS_DIST_MAXIMUM) nan_i = panel[a0 + i];
    // condensed: row i's entries start at pair (i, i + 1); its j-th sits j - i - 1 further
    const int64_t row0 = kCondensed ? dist_pair_offset(i, i + 1, ma) - (i + 1) : i * mb;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int64_t j = j0 + tx + 16 * e;
      if (j >= mb || (kCondensed && i >= j)) continue;
      double v = metric_value<M>(acc[r][e], cnt[r][e], ncol);
      if constexpr (M == KS_DIST_MAXIMUM) {
        const double mark = nan_i + panel[b0 + j];  // NaN where either row is
        v = mark != mark ? mark : v;
      }
      out[row0 + j] = metric_result<M>(v, squared);
    }
  }
}

#ifdef KS_DIST_NAIVE
// Comparison build (tools/spectra_dist_bench.py): one thread per
// pair, both rows read from the panel in global memory for every pair.  The
// same operation order, so the same bits.
template <int M, bool kCondensed>
__global__ void __launch_bounds__(kNaive *kNaive) k_dist_naive(const double *__restrict__ panel, int64_t ld, int ncol,
                                                               int64_t a0, int64_t ma, int64_t b0, int64_t mb,
                                                               int64_t tiles_b, int squared, double *__restrict__ out) {
  int64_t tr, tc;
  if (kCondensed) {
    dist_tile_of((int64_t)blockIdx.x, tiles_b, &tr, &tc);
  } else {
    tr = (int64_t)blockIdx.x / tiles_b;
    tc = (int64_t)blockIdx.x - tr * tiles_b;
  }
  const int64_t i = tr * kNaive + (threadIdx.x >> 4), j = tc * kNaive + (threadIdx.x & 15);
  if (i >= ma || j >= mb || (kCondensed && i >= j)) return;
  const double *pa = panel + a0 + i, *pb = panel + b0 + j;
  double acc = 0.0;
  int cnt = 0;
  for (int k = 0; k < ncol; ++k) metric_step<M>(acc, cnt, pa[(size_t)k * ld], pb[(size_t)k * ld]);
  double v = metric_value<M>(acc, cnt, ncol);
  if constexpr (M == KS_DIST_MAXIMUM) {
    const double mark = pa[0] + pb[0];  // NaN where either row is
    v = mark != mark ? mark : v;
  }
  out[kCondensed ? dist_pair_offset(i, j, ma) : i * mb + j] = metric_result<M>(v, squared);
}
#endif

// Blocks of the distance launch (a linear grid), -1 when one launch cannot hold them.
int64_t dist_grid(bool cross, int64_t ma, int64_t mb, int64_t *tiles_b) {
  const int64_t ta = (ma + kEdge - 1) / kEdge, tb = cross ? (mb + kEdge - 1) / kEdge : ta;
  *tiles_b = tb;
  if (ta > ((int64_t)1 << 24) || tb > ((int64_t)1 << 24)) return -1;
  const int64_t g = cross ? ta * tb : dist_tile_count(ta);
  return g > 0x7fffffffLL ? -1 : g;
}

ks_status check_dist_args(bool cross, int64_t n, int32_t ncol, int64_t ma, int64_t mb, int32_t flags) {
  KS_TRY(panel_check_ncol(ncol, KS_DIST_MAX_NCOL));
  if (flags & ~(KS_DIST_SQUARED | KS_DIST_METRIC_MASK))
    return fail(KS_ERR_ARG, "unknown distance flags 0x%x", (unsigned)flags);
  KS_TRY(dist_check_metric(flags));
  KS_TRY(panel_check_n(n));
  if (ma < 0 || mb < 0) return fail(KS_ERR_ARG, "the number of selected rows must not be negative");
  int64_t tb;
  if (dist_grid(cross, ma, mb, &tb) < 0)  // beyond 2^31 - 1 tiles: tens of terabytes of output
    return fail(KS_ERR_ARG, "too many selected rows for one call: walk the list in blocks");
  return KS_OK;
}

// cross = false: the condensed form of the ma selected rows (rows_b, mb unused).
ks_status dist_impl(ks_ctx *ctx, const uint32_t *sp, int64_t n, int ncol, const int64_t *rows_a, int64_t ma,
                    const int64_t *rows_b, int64_t mb, bool cross, int flags, double *out, ks_dist_stats *stats) {
  hipStream_t st = ctx->stream;
  if (!cross) mb = 0, rows_b = nullptr;
  // every index is checked before anything is written
  if (rows_a || rows_b) {
    void *scal = nullptr;
    KS_TRY(ensure(ctx, SLOT_SCALARS, 4096, &scal));
    unsigned long long *bad = static_cast<unsigned long long *>(scal) + kScDistBad;
    KS_HIP(hipMemsetAsync(bad, 0, 16, st));
    if (rows_a && ma) {
      hipLaunchKernelGGL(k_dist_check, dim3((unsigned)((ma + 255) / 256)), dim3(256), 0, st, rows_a, ma, n, bad);
      KS_HIP(hipGetLastError());
    }
    if (rows_b && mb) {
      hipLaunchKernelGGL(k_dist_check, dim3((unsigned)((mb + 255) / 256)), dim3(256), 0, st, rows_b, mb, n, bad + 1);
      KS_HIP(hipGetLastError());
    }
    unsigned long long hbad[4] = {0, 0, 0, 0};  // both selections' index words; no row is refused for its sum here
    KS_HIP(hipMemcpyAsync(hbad, bad, 16, hipMemcpyDeviceToHost, st));
    KS_HIP(hipStreamSynchronize(st));
    KS_TRY(panel_report(hbad, 2, ma, mb));
  }
  const int64_t pairs = cross ? ma * mb : dist_pair_count(ma);
  if (pairs == 0) return KS_OK;

  const int64_t ld = ma + mb;
  DevFree panel_mem;
  const size_t panel_bytes = (size_t)ld * ncol * 8;
  KS_TRY(dev_alloc(&panel_mem, panel_bytes, "the profile panel"));
  double *panel = static_cast<double *>(panel_mem.p);

  KS_HIP(hipEventRecord(ctx->ev[0], st));
  const bool root = (flags & KS_DIST_METRIC_MASK) == KS_DIST_HELLINGER;
  const auto normalise = root ? k_dist_normalise<true> : k_dist_normalise<false>;
  hipLaunchKernelGGL(normalise, dim3((unsigned)((ma + kDT - 1) / kDT)), dim3(256), 0, st, sp, ncol, rows_a, ma, panel,
                     ld, (int64_t)0);
  KS_HIP(hipGetLastError());
  if (cross) {
    hipLaunchKernelGGL(normalise, dim3((unsigned)((mb + kDT - 1) / kDT)), dim3(256), 0, st, sp, ncol, rows_b, mb, panel,
                       ld, ma);
    KS_HIP(hipGetLastError());
  }
  KS_HIP(hipEventRecord(ctx->ev[1], st));
  const int sq = (flags & KS_DIST_SQUARED) ? 1 : 0;
  int64_t tb = 0;
  const int64_t grid = dist_grid(cross, ma, mb, &tb);  // (check_dist_args: it fits)
  metric_dispatch(flags, [&](auto metric) {
    constexpr int M = decltype(metric)::value;
#ifdef KS_DIST_NAIVE
    const auto kernel = cross ? k_dist_naive<M, false> : k_dist_naive<M, true>;
    const dim3 block(kNaive * kNaive);
#else
    const auto kernel = cross ? k_dist_tile<M, false> : k_dist_tile<M, true>;
    const dim3 block(kDThreads);
#endif
    // the cross form's B rows sit behind the A rows in the panel; the condensed form has one set
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), block, 0, st, panel, ld, ncol, (int64_t)0, ma,
                       cross ? ma : (int64_t)0, cross ? mb : ma, tb, sq, out);
    return KS_OK;
  });
  KS_HIP(hipGetLastError());
  KS_HIP(hipEventRecord(ctx->ev[2], st));
  KS_HIP(hipStreamSynchronize(st));  // the panel is freed on return
  if (stats) {
    KS_TRY(event_ms(ctx, 0, 2, &stats->ms_total));
    KS_TRY(event_ms(ctx, 0, 1, &stats->ms_normalise));
    KS_TRY(event_ms(ctx, 1, 2, &stats->ms_distance));
    stats->n_pairs = pairs;
    stats->bytes_written = pairs * 8;
    stats->panel_bytes = (int64_t)panel_bytes;
  }
  return KS_OK;
}

// Host-buffer body: everything validated; uploads, runs dist_impl, copies back.
ks_status dist_host(ks_ctx *ctx, const uint32_t *sp, int64_t n, int ncol, const int64_t *rows_a, int64_t ma,
                    const int64_t *rows_b, int64_t mb, bool cross, int flags, double *out) {
  KS_TRY(default_ctx(&ctx));
  KS_ENTER(ctx);
  const HostEnd host_end{ctx};  // (ks_set_host_cache)
  const int64_t pairs = cross ? ma * mb : dist_pair_count(ma);
  void *d_out = nullptr;
  KS_TRY(ensure(ctx, SLOT_REG_TMP, (size_t)pairs * 8, &d_out));
  SpectraUpload up;
  KS_TRY(upload_spectra(ctx, sp, n, ncol, rows_a, ma, cross ? rows_b : nullptr, mb, 0, &up));
  hipStream_t st = ctx->stream;
  KS_TRY(dist_impl(ctx, up.sp, n, ncol, up.rows, ma, up.rows_b, mb, cross, flags, static_cast<double *>(d_out),
                   nullptr));
  KS_HIP(hipMemcpyAsync(out, d_out, (size_t)pairs * 8, hipMemcpyDeviceToHost, st));
  KS_HIP(hipStreamSynchronize(st));
  return KS_OK;
}

}  // namespace
}  // namespace ks

using namespace ks;

extern "C" ks_status ks_spectra_dist_dev(ks_ctx *ctx, const uint32_t *spectra_dev, int64_t n, int32_t ncol,
                                         const int64_t *rows_dev, int64_t m, int32_t flags, double *out_dev,
                                         ks_dist_stats *stats) {
  if (stats) memset(stats, 0, sizeof(*stats));
  KS_TRY(check_dist_args(false, n, ncol, m, 0, flags));
  if (m == 0) return KS_OK;
  KS_TRY(panel_check_null_rows(rows_dev, m, n, "rows_dev", "m"));
  if (!spectra_dev) return fail(KS_ERR_ARG, "null spectra");
  if (m > 1 && !out_dev) return fail(KS_ERR_ARG, "null output");
  KS_TRY(default_ctx(&ctx));
  KS_ENTER(ctx);
  return dist_impl(ctx, spectra_dev, n, ncol, rows_dev, m, nullptr, 0, false, flags, out_dev, stats);
}

extern "C" ks_status ks_spectra_cross_dist_dev(ks_ctx *ctx, const uint32_t *spectra_dev, int64_t n, int32_t ncol,
                                               const int64_t *rows_a_dev, int64_t na, const int64_t *rows_b_dev,
                                               int64_t nb, int32_t flags, double *out_dev, ks_dist_stats *stats) {
  if (stats) memset(stats, 0, sizeof(*stats));
  KS_TRY(check_dist_args(true, n, ncol, na, nb, flags));
  if (na == 0 && nb == 0) return KS_OK;
  KS_TRY(panel_check_null_rows(rows_a_dev, na, n, "rows_a_dev", "m"));
  KS_TRY(panel_check_null_rows(rows_b_dev, nb, n, "rows_b_dev", "m"));
  if (!spectra_dev) return fail(KS_ERR_ARG, "null spectra");
  if (na > 0 && nb > 0 && !out_dev) return fail(KS_ERR_ARG, "null output");
  KS_TRY(default_ctx(&ctx));
  KS_ENTER(ctx);
  return dist_impl(ctx, spectra_dev, n, ncol, rows_a_dev, na, rows_b_dev, nb, true, flags, out_dev, stats);
}

extern "C" ks_status ks_spectra_dist(ks_ctx *ctx, const uint32_t *spectra, int64_t n, int32_t ncol,
                                     const int64_t *rows, int64_t m, int32_t flags, double *out) {
  KS_TRY(check_dist_args(false, n, ncol, m, 0, flags));
  if (m == 0) return KS_OK;
  KS_TRY(panel_check_null_rows(rows, m, n, "rows", "m"));
  if (!spectra) return fail(KS_ERR_ARG, "null spectra");
  KS_TRY(panel_check_index_host(rows, m, n, 0));
  if (m == 1) return KS_OK;  // no pair: nothing to write
  if (!out) return fail(KS_ERR_ARG, "null output");
  return dist_host(ctx, spectra, n, ncol, rows, m, nullptr, 0, false, flags, out);
}

extern "C" ks_status ks_spectra_cross_dist(ks_ctx *ctx, const uint32_t *spectra, int64_t n, int32_t ncol,
                                           const int64_t *rows_a, int64_t na, const int64_t *rows_b, int64_t nb,
                                           int32_t flags, double *out) {
  KS_TRY(check_dist_args(true, n, ncol, na, nb, flags));
  if (na == 0 && nb == 0) return KS_OK;
  KS_TRY(panel_check_null_rows(rows_a, na, n, "rows_a", "m"));
  KS_TRY(panel_check_null_rows(rows_b, nb, n, "rows_b", "m"));
  if (!spectra) return fail(KS_ERR_ARG, "null spectra");
  KS_TRY(panel_check_index_host(rows_a, na, n, 0));
  KS_TRY(panel_check_index_host(rows_b, nb, n, 1));
  if (na == 0 || nb == 0) return KS_OK;
  if (!out) return fail(KS_ERR_ARG, "null output");
  return dist_host(ctx, spectra, n, ncol, rows_a, na, rows_b, nb, true, flags, out);
}

// The index header on the host (tests/test_spectra_dist.py): cnt pairs / tile ids at a time.
extern "C" void ks_dist_pair_offsets(const int64_t *i, const int64_t *j, int64_t cnt, int64_t m, int64_t *off) {
  for (int64_t x = 0; x < cnt; ++x) off[x] = dist_pair_offset(i[x], j[x], m);
}

extern "C" void ks_dist_tiles_of(const int64_t *t, int64_t cnt, int64_t tiles, int64_t *row, int64_t *col) {
  for (int64_t x = 0; x < cnt; ++x) dist_tile_of(t[x], tiles, &row[x], &col[x]);
}

extern "C" int32_t ks_dist_tile_rows(void) { return kDT; }
