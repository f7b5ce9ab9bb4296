// ks_knn.hip -- the k nearest rows of a candidate selection for every selected
// row of a spectra matrix (ks_spectra_knn / ks_spectra_knn_dev); the contract
// is in include/kmer_spans.h.
//
// The neighbour list of region spectra without the distance matrix: memory is
// the profile panel plus O(na k) per candidate split; nothing of size na x nb
// is written or sorted.  The squared distance is the inner loop of
// ks_spectra_dist, an order of separate FP64 operations (-ffp-contract=off,
// csrc/Makefile), one accumulator per pair, so every acc carries the bits of
// ks_spectra_cross_dist(..., KS_DIST_SQUARED).  The selection is by the
// lexicographic order of (acc, position), a total order: the result does not
// depend on the tile shape, the grid or the split of the candidates.
//
// Normalise: the shared row-major profile panel (ks_panel.hip), one per side
//            (the select kernel stages 16 consecutive columns of a row, a
//            128-byte segment, for both sides, as k_km_assign does).  One
//            32-byte read-back of both sides' words ends the call before any
//            output is written.
// Select:    k_knn_select: a block of 256 threads keeps 64 query rows and
//            walks candidate tiles of 64, a thread a 4 x 4 register block of
//            accumulators as in k_dist_tile / k_km_assign; chunks of 16 columns
//            of both sides are staged in LDS, transposed on the way in.  Every
//            query row has a sorted list of its k best (acc, position) so far
//            in LDS, 12 bytes per entry.  The 16 threads of a row are 16
//            consecutive lanes, so the 16 rows of a wave belong to that wave
//            alone and the lists need no block barrier.  After a tile a thread
//            tests its 16 values, four steps of one value per thread, against
//            the row's k-th entry (kept in registers, read again after a step
//            that inserted); the survivors of the wave are taken one at a time
//            (ballot, lowest lane first) and inserted by the whole wave: lane
//            l reads entries l and l - 1 (k <= 64), the rank is a ballot's
//            popcount, lane l writes the entry that belongs at l.  An
//            insertion behind the k-th entry writes nothing, so a stale
//            threshold only costs time.
//            The candidate tiles are split over blockIdx.y where that fills
//            the device better (split_plan) and every split writes its list.
// Merge:     k_knn_merge, a wave per query row: the splits' lists are merged
//            in registers by the same insertion, a split's walk ending at its
//            first entry that does not beat the k-th.  It takes the root if
//            asked and writes index and dist.  With one split k_knn_select
//            writes them itself.
// Metrics:   the kernels are templates on the metric field of flags
//            (ks_dist_metric.h).  The lists hold the value a
//            pair is ranked by: acc for euclidean and hellinger (the panel
//            holds the roots then), the distance itself for manhattan, maximum
//            and canberra (canberra's acc is scaled by its count after a
//            tile's last chunk).  All values are >= +0 and never NaN, so the
//            insertion and the merge are the same code for every metric; only
//            the last step (root, 0.5 *) differs.
// No kernel waits on another workgroup; stream order is the only
// synchronisation between them.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

#include "ks_panel.h"
// after hip_runtime.h (ks_internal.h)
#include "ks_dist_metric.h"

namespace ks {
namespace {

constexpr int kNT = 64;     // tile edge: query rows x candidates
constexpr int kNK = 16;     // columns per LDS chunk
constexpr int kNPadA = 66;  // row stride of the query image: 16-byte aligned rows, 128-bit reads of 4 rows
constexpr int kNPadB = 65;  // row stride of the candidate image: conflict-free transposed stores
constexpr int kNoPos = 0x7fffffff;  // the position of an unused list entry (positions are below it)
// split_plan's estimates in units of a block's 256-column tile, from the select times at 24,611 rows with the
// split count forced to 1 .. 55: what an expected insertion per row adds, and what a block adds
constexpr double kInsertTiles = 0.05;
constexpr double kBlockTiles = 0.5;
constexpr size_t kSplitBytes = (size_t)1 << 30;  // split_plan: no more splits than lists fit in this

struct KnnState {
  // cnt - position of the first: bad query index / bad candidate index / empty query row / empty candidate row
  unsigned long long bad[4];
};

__device__ __forceinline__ bool knn_before(double v, int p, double w, int q) { return v < w || (v == w && p < q); }

// (v, j) into the sorted list whose entry l lane l < k holds; the entries behind it move up a lane and the
// last one leaves.  Returns the rank; k or more: nothing changed.  The whole wave calls it.
__device__ __forceinline__ int knn_insert(double &lv, int &lp, double v, int j, int lane, int k) {
  const int p = (int)__popcll(__ballot(lane < k && knn_before(lv, lp, v, j)));  // the list is sorted: a prefix
  const double uv = __shfl_up(lv, 1);
  const int up = __shfl_up(lp, 1);
  if (lane == p)
    lv = v, lp = j;
  else if (lane > p)
    lv = uv, lp = up;
  return p;
}

// Block (x, y): query rows [64 x, 64 x + 64) against the candidate tiles [y tps, (y + 1) tps).
// direct: index / dist [na][k] are written; otherwise pval / ppos [y][na][k], the split's sorted list,
// unused entries (+inf, kNoPos).  self: candidate position == query position is left out.
// M: the metric (ks_dist_metric.h); the lists hold metric_value, the value the pairs are ranked by.
template <int M>
__global__ void __launch_bounds__(256) k_knn_select(const double *__restrict__ pa, int64_t na,
                                                    const double *__restrict__ pb, int64_t nb, int ncol, int k,
                                                    int self, int tps, int direct, int take_root,
                                                    double *__restrict__ pval, int *__restrict__ ppos,
                                                    int64_t *__restrict__ index, double *__restrict__ dist) {
  __shared__ __attribute__((aligned(16))) double As[kNK][kNPadA];  // [c][query row]: transposed on the way in
  __shared__ double Bs[kNK][kNPadB];                               // [c][candidate]
  extern __shared__ __attribute__((aligned(16))) unsigned char knn_lds[];
  double *lval = reinterpret_cast<double *>(knn_lds);  // [64][k]
  int *lpos = reinterpret_cast<int *>(lval + kNT * k);  // [64][k]
  const int64_t i0 = (int64_t)blockIdx.x * kNT;
  const int ctiles = (int)((nb + kNT - 1) / kNT);
  const int t0 = blockIdx.y * tps, t1 = min(t0 + tps, ctiles);
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, lane = tid & 63, wrow = (tid >> 6) * 16;
  const double inf = std::numeric_limits<double>::infinity();
  // the lists of rows wrow .. wrow + 15 are this wave's alone
  if (lane < k)
    for (int q = 0; q < 16; ++q) lval[(wrow + q) * k + lane] = inf, lpos[(wrow + q) * k + lane] = kNoPos;
  double tv[4];  // the k-th entry of the thread's rows as of the last refresh: never before the list's
  int tp[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) tv[r] = inf, tp[r] = kNoPos;
  for (int t = t0; t < t1; ++t) {
    const int64_t j0 = (int64_t)t * kNT;
    double acc[4][4];
    int cnt[4][4];  // canberra's columns kept; no register in the other metrics
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[r][e] = 0.0, cnt[r][e] = 0;
    for (int k0 = 0; k0 < ncol; k0 += kNK) {
#pragma unroll
      for (int e = 0; e < kNK * kNT / 256; ++e) {
        const int idx = tid + 256 * e;
        const int ra = idx >> 4, ka = idx & 15;  // 16 consecutive columns of one row
        const bool in_k = k0 + ka < ncol;
        As[ka][ra] = (in_k && i0 + ra < na) ? pa[(size_t)(i0 + ra) * ncol + k0 + ka] : 0.0;
        Bs[ka][ra] = (in_k && j0 + ra < nb) ? pb[(size_t)(j0 + ra) * ncol + k0 + ka] : 0.0;
      }
      __syncthreads();
      // columns past ncol are staged as zeros on both sides: they leave acc's bits in every metric, and
      // canberra omits them without counting them (metric_step)
#pragma unroll
      for (int kk = 0; kk < kNK; ++kk) {
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
      __syncthreads();
    }
    if constexpr (M == KS_DIST_CANBERRA) {  // ranked by the scaled result (a pair past the edges: 0 / 0, masked below)
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[r][e] = metric_value<M>(acc[r][e], cnt[r][e], ncol);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t i = i0 + ty * 4 + r;
      const int kth = (ty * 4 + r) * k + k - 1;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int64_t j = j0 + tx + 16 * e;
        const bool pass = i < na && j < nb && !(self && i == j) && knn_before(acc[r][e], (int)j, tv[r], tp[r]);
        unsigned long long todo = __ballot(pass);
        const bool touched = todo != 0;  // wave-uniform
        while (todo) {  // wave-uniform: one survivor at a time, the whole wave inserts it
          const int src = __ffsll(todo) - 1;  // a scalar: the survivor's value comes by v_readlane
          todo &= todo - 1;
          const double v = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(acc[r][e]), src),
                                            __builtin_amdgcn_readlane(__double2loint(acc[r][e]), src));
          const int cj = (int)j0 + (src & 15) + 16 * e;
          const int at = (wrow + (src >> 4) * 4 + r) * k + lane;
          // the stores of the insertion before are behind this one's loads: LDS operations of a wave execute in order
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
          __builtin_amdgcn_wave_barrier();
          double lv = inf, bv = inf;  // entry `lane` and the entry below it: all four loads are in flight together
          int lp = kNoPos, bp = kNoPos;
          if (lane < k) {
            lv = lval[at], lp = lpos[at];
            if (lane > 0) bv = lval[at - 1], bp = lpos[at - 1];
          }
          const int p = (int)__popcll(__ballot(lane < k && knn_before(lv, lp, v, cj)));  // sorted: a prefix
          if (lane < k && lane >= p) lval[at] = lane == p ? v : bv, lpos[at] = lane == p ? cj : bp;
        }
        if (touched) {
          // the k-th entry again, so that the next 16 candidates of the row meet the bar these ones raised (a
          // list's first tile would otherwise insert all 64).  The wave's stores are behind its loads, as above.
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
          __builtin_amdgcn_wave_barrier();
          tv[r] = lval[kth], tp[r] = lpos[kth];
        }
      }
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  if (lane >= k) return;
  for (int q = 0; q < 16; ++q) {
    const int64_t i = i0 + wrow + q;
    if (i >= na) break;
    const double v = lval[(wrow + q) * k + lane];
    const int p = lpos[(wrow + q) * k + lane];
    if (direct) {
      index[(size_t)i * k + lane] = p;
      dist[(size_t)i * k + lane] = metric_result<M>(v, !take_root);
    } else {
      const size_t o = ((size_t)blockIdx.y * na + i) * k + lane;
      pval[o] = v, ppos[o] = p;
    }
  }
}

// A wave per query row: the nsplit sorted lists pval / ppos [y][na][k] into index / dist [na][k].
template <int M>
__global__ void __launch_bounds__(256) k_knn_merge(const double *__restrict__ pval, const int *__restrict__ ppos,
                                                   int64_t na, int k, int nsplit, int take_root,
                                                   int64_t *__restrict__ index, double *__restrict__ dist) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= na) return;  // wave-uniform
  const double inf = std::numeric_limits<double>::infinity();
  double lv = inf;
  int lp = kNoPos;
  if (lane < k) lv = pval[(size_t)i * k + lane], lp = ppos[(size_t)i * k + lane];
  for (int y = 1; y < nsplit; ++y) {
    const size_t o = ((size_t)y * na + i) * k + lane;
    double cv = inf;
    int cp = kNoPos;
    if (lane < k) cv = pval[o], cp = ppos[o];
    for (int t = 0; t < k; ++t) {
      const double v = __shfl(cv, t);
      const int j = __shfl(cp, t);
      if (!knn_before(v, j, __shfl(lv, k - 1), __shfl(lp, k - 1))) break;  // nor does any later entry of this split
      knn_insert(lv, lp, v, j, lane, k);
    }
  }
  if (lane >= k) return;
  index[(size_t)i * k + lane] = lp;
  dist[(size_t)i * k + lane] = metric_result<M>(lv, !take_root);
}

// The work memory of a call, one allocation: the panel, then the rest.
struct KnnWork {
  double *pa = nullptr, *pb = nullptr, *pval = nullptr;
  int *ppos = nullptr;
  KnnState *state = nullptr;
  size_t panel_bytes = 0, bytes = 0;
  int nsplit = 1, tps = 1;

  // base null: only the sizes.  nb 0: the self form, the candidates are the query panel.
  void lay(char *base, int64_t na, int64_t nb, int ncol, int k) {
    Arena a{base};
    pa = a.take<double>((size_t)na * ncol);
    pb = nb ? a.take<double>((size_t)nb * ncol) : pa;
    panel_bytes = a.off;
    state = a.take<KnnState>(1);
    if (nsplit > 1) {
      pval = a.take<double>((size_t)nsplit * na * k);
      ppos = a.take<int>((size_t)nsplit * na * k);
    }
    bytes = a.off;
  }
};

ks_status check_knn_args(const void *spectra, int64_t n, int32_t ncol, const void *rows, int64_t na,
                         const void *rows_b, int64_t nb, int32_t k, int32_t flags, const void *index,
                         const void *dist) {
  KS_TRY(panel_check_count(na, 1, "a nearest-neighbour call", "query row", "na"));
  if (rows_b) KS_TRY(panel_check_count(nb, 1, "a nearest-neighbour call", "candidate row", "nb"));
  KS_TRY(panel_check_most(na, 0x7ffffffeLL));
  if (rows_b) KS_TRY(panel_check_most(nb, 0x7ffffffeLL));
  KS_TRY(panel_check_ncol(ncol, KS_DIST_MAX_NCOL));
  if (k < 1 || k > KS_KNN_MAX_K)
    return fail(KS_ERR_ARG, "k must be between 1 and %d (k = %d)", KS_KNN_MAX_K, (int)k);
  if (flags & ~(KS_DIST_SQUARED | KS_DIST_METRIC_MASK))
    return fail(KS_ERR_ARG, "unknown flags 0x%x for a nearest-neighbour call", (unsigned)flags);
  KS_TRY(dist_check_metric(flags));
  KS_TRY(panel_check_n(n));
  KS_TRY(panel_check_null_rows(rows, na, n, "rows", "na"));
  if (!spectra) return fail(KS_ERR_ARG, "null spectra");
  if (!index || !dist) return fail(KS_ERR_ARG, "null output");
  return KS_OK;
}

ks_status check_knn_k(bool self, int64_t na, int64_t nb, int k) {
  const int64_t cand = self ? na - 1 : nb;
  if (k > cand)
    return fail(KS_ERR_ARG, "k exceeds the number of candidate rows (k = %d, %lld candidate%s)", k, (long long)cand,
                cand == 1 ? "" : "s");
  return KS_OK;
}

// How the candidate tiles are cut over blockIdx.y.  One workgroup per 64 query rows leaves CUs idle when the
// rows are few, and workgroups that all walk as many tiles run in rounds of `slots` (the workgroups the device
// holds at once), the last round as long as a full one: at 385 row tiles and 768 slots, 6 splits make 3.01
// rounds and cost 4.  Every split keeps a list of its own, and a list costs about k (1 + ln(candidates / k))
// insertions per row.  So: the number of splits with the least rounds x (tiles + what the block and its
// insertions add) by that estimate, among those whose lists fit in kSplitBytes.  The lists returned do not
// depend on the choice.
void split_plan(int64_t na, int64_t ncand, int ncol, int k, int64_t slots, int *tps_out, int *nsplit_out) {
  const int64_t rtiles = (na + kNT - 1) / kNT;
  const int64_t ctiles = (ncand + kNT - 1) / kNT;
  const int64_t fit = std::max<int64_t>(1, (int64_t)(kSplitBytes / ((size_t)12 * na * k)));
  const int64_t most = std::min<int64_t>(std::min<int64_t>(ctiles, fit), 2048);
  double best = std::numeric_limits<double>::infinity();
  for (int64_t ns = 1; ns <= most; ++ns) {
    const int64_t tps = (ctiles + ns - 1) / ns;
    if ((ctiles + tps - 1) / tps != ns) continue;  // the same walk as a smaller ns
    const int64_t rounds = (rtiles * ns + slots - 1) / slots;
    const double cand = (double)std::min<int64_t>(ncand, tps * kNT);
    const double inserts = k * (1.0 + std::log(std::max(1.0, cand / k)));
    const double cost = (double)rounds * ((double)tps + (kBlockTiles + kInsertTiles * inserts) * 256.0 / ncol);
    if (cost < best) best = cost, *tps_out = (int)tps, *nsplit_out = (int)ns;
  }
}

// Everything but the device-side checks validated; all pointers are device pointers.
template <int M>
ks_status knn_metric(ks_ctx *ctx, const uint32_t *sp, int64_t n, int ncol, const int64_t *rows, int64_t na,
                   const int64_t *rows_b, int64_t nb, int k, int flags, int64_t *index, double *dist,
                   ks_knn_stats *stats) {
  hipStream_t st = ctx->stream;
  const bool self = rows_b == nullptr;
  const int64_t ncand = self ? na : nb;  // candidate positions, the masked one included
  KnnWork w;
  DevFree mem;
  const size_t lds = (size_t)kNT * k * 12;
  KS_HIP(hipFuncSetAttribute((const void *)k_knn_select<M>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  int per_cu = 1;  // workgroups of k_knn_select a CU holds at this k (registers, and the lists' LDS)
  KS_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)k_knn_select<M>, 256, lds));
  split_plan(na, ncand, ncol, k, (int64_t)ctx->num_cus * std::max(per_cu, 1), &w.tps, &w.nsplit);
  w.lay(nullptr, na, self ? 0 : nb, ncol, k);
  KS_TRY(dev_alloc(&mem, w.bytes, "the profile panel"));
  w.lay(static_cast<char *>(mem.p), na, self ? 0 : nb, ncol, k);

  KS_HIP(hipEventRecord(ctx->ev[0], st));
  KS_HIP(hipMemsetAsync(w.state, 0, sizeof(KnnState), st));
  const PanelRoot root = M == KS_DIST_HELLINGER ? PanelRoot::kSqrt : PanelRoot::kNone;
  KS_TRY(panel_normalise(ctx, sp, n, ncol, rows, na, root, w.pa, nullptr, &w.state->bad[0], &w.state->bad[2]));
  if (!self)
    KS_TRY(panel_normalise(ctx, sp, n, ncol, rows_b, nb, root, w.pb, nullptr, &w.state->bad[1], &w.state->bad[3]));
  unsigned long long hbad[4] = {0, 0, 0, 0};
  KS_HIP(hipMemcpyAsync(hbad, w.state->bad, sizeof(hbad), hipMemcpyDeviceToHost, st));
  KS_HIP(hipStreamSynchronize(st));
  KS_TRY(panel_report(hbad, 2, na, nb));
  KS_TRY(check_knn_k(self, na, nb, k));
  // from here on the outputs are written
  KS_HIP(hipEventRecord(ctx->ev[1], st));
  const int take_root = (flags & KS_DIST_SQUARED) ? 0 : 1;
  hipLaunchKernelGGL(k_knn_select<M>, dim3((unsigned)((na + kNT - 1) / kNT), (unsigned)w.nsplit), dim3(256), lds, st,
                     w.pa, na, w.pb, ncand, ncol, k, self ? 1 : 0, w.tps, w.nsplit == 1 ? 1 : 0, take_root, w.pval,
                     w.ppos, index, dist);
  KS_HIP(hipGetLastError());
  KS_HIP(hipEventRecord(ctx->ev[2], st));
  if (w.nsplit > 1) {
    hipLaunchKernelGGL(k_knn_merge<M>, dim3((unsigned)((na + 3) / 4)), dim3(256), 0, st, w.pval, w.ppos, na, k, w.nsplit,
                       take_root, index, dist);
    KS_HIP(hipGetLastError());
  }
  KS_HIP(hipEventRecord(ctx->ev[3], st));
  KS_HIP(hipStreamSynchronize(st));  // the work memory is freed on return
  if (stats) {
    KS_TRY(event_ms(ctx, 0, 3, &stats->ms_total));
    KS_TRY(event_ms(ctx, 0, 1, &stats->ms_normalise));
    KS_TRY(event_ms(ctx, 1, 2, &stats->ms_select));
    KS_TRY(event_ms(ctx, 2, 3, &stats->ms_merge));
    if (w.nsplit == 1) stats->ms_merge = 0.0;
    stats->n_splits = w.nsplit;
    stats->tiles_per_split = w.tps;
    stats->panel_bytes = (int64_t)w.panel_bytes;
    stats->work_bytes = (int64_t)(w.bytes - w.panel_bytes);
  }
  return KS_OK;
}

ks_status knn_impl(ks_ctx *ctx, const uint32_t *sp, int64_t n, int ncol, const int64_t *rows, int64_t na,
                   const int64_t *rows_b, int64_t nb, int k, int flags, int64_t *index, double *dist,
                   ks_knn_stats *stats) {
  return metric_dispatch(flags, [&](auto metric) {
    return knn_metric<decltype(metric)::value>(ctx, sp, n, ncol, rows, na, rows_b, nb, k, flags, index, dist, stats);
  });
}

}  // namespace
}  // namespace ks

using namespace ks;

extern "C" ks_status ks_spectra_knn_dev(ks_ctx *ctx, const uint32_t *spectra_dev, int64_t n, int32_t ncol,
                                        const int64_t *rows_dev, int64_t na, const int64_t *rows_b_dev, int64_t nb,
                                        int32_t k, int32_t flags, int64_t *index_dev, double *dist_dev,
                                        ks_knn_stats *stats) {
  if (stats) memset(stats, 0, sizeof(*stats));
  KS_TRY(check_knn_args(spectra_dev, n, ncol, rows_dev, na, rows_b_dev, nb, k, flags, index_dev, dist_dev));
  KS_TRY(default_ctx(&ctx));
  KS_ENTER(ctx);
  return knn_impl(ctx, spectra_dev, n, ncol, rows_dev, na, rows_b_dev, nb, k, flags, index_dev, dist_dev, stats);
}

extern "C" ks_status ks_spectra_knn(ks_ctx *ctx, const uint32_t *spectra, int64_t n, int32_t ncol, const int64_t *rows,
                                    int64_t na, const int64_t *rows_b, int64_t nb, int32_t k, int32_t flags,
                                    int64_t *index, double *dist) {
  KS_TRY(check_knn_args(spectra, n, ncol, rows, na, rows_b, nb, k, flags, index, dist));
  KS_TRY(panel_check_rows_host(spectra, n, ncol, rows, na, rows_b, nb));
  KS_TRY(check_knn_k(rows_b == nullptr, na, nb, k));
  KS_TRY(default_ctx(&ctx));
  KS_ENTER(ctx);
  const HostEnd host_end{ctx};  // (ks_set_host_cache)
  void *d_out = nullptr;
  const size_t out_elems = (size_t)na * k;
  KS_TRY(ensure(ctx, SLOT_REG_TMP, out_elems * 16, &d_out));
  SpectraUpload up;
  KS_TRY(upload_spectra(ctx, spectra, n, ncol, rows, na, rows_b, rows_b ? nb : 0, 0, &up));
  hipStream_t st = ctx->stream;
  int64_t *d_idx = static_cast<int64_t *>(d_out);
  double *d_dist = reinterpret_cast<double *>(d_idx + out_elems);
  KS_TRY(knn_impl(ctx, up.sp, n, ncol, up.rows, na, up.rows_b, nb, k, flags, d_idx, d_dist, nullptr));
  KS_HIP(hipMemcpyAsync(index, d_idx, out_elems * 8, hipMemcpyDeviceToHost, st));
  KS_HIP(hipMemcpyAsync(dist, d_dist, out_elems * 8, hipMemcpyDeviceToHost, st));
  KS_HIP(hipStreamSynchronize(st));
  return KS_OK;
}
