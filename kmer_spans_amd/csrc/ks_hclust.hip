// ks_hclust.hip -- agglomerative clustering of a condensed dissimilarity
// vector on the device (ks_hclust_dev / ks_hclust) and the host-only tree
// cut (ks_hclust_cut); the contract is in include/kmer_spans.h.
//
// What the reference's author does with dist() of the spectra next
// (test.R:776, :805): hclust(), then a cut into groups of bounded diameter
// (test.R:826-859).  Here the condensed matrix stays in HBM as
// ks_spectra_dist_dev wrote it and is updated in place.
//
// The algorithm is the nearest-neighbour-list agglomeration of R's hclust,
// fixed in the header as a sequence of comparisons (strict <, ascending
// index: the lowest index wins every tie).  Complete and single linkage copy
// bits; average linkage is two multiplications, an addition and a division as
// separate FP64 operations (-ffp-contract=off, csrc/Makefile).
//
// Check:  k_hclust_check (ks_finite_check.h, shared with ks_nj.hip) reads the
//         matrix once (16-byte loads, grid-stride) and keeps the lowest offset
//         of a non-finite entry (atomicMin); one 8-byte read-back ends a call
//         with a bad entry before anything is modified.
// Init:   k_hclust_init: a block of 256 threads per row i scans the contiguous
//         segment D(i, i+1 .. n-1) for (min, lowest j).
// Merge:  two launches per step, 2 (n - 1) in all, queued on the stream with no
//         read-back between them: the device picks the pair and the rows to
//         rescan.  No kernel waits on another workgroup; stream order is the
//         only synchronisation between workgroups.
//           k_hclust_pair    up to 8 blocks of 1024 threads.  Every block
//                            repeats the arg-min over dnn (value, index; the
//                            lower index on equal values in every shuffle and
//                            LDS stage) -- the kernel writes none of what the
//                            arg-min reads, so all blocks agree without
//                            talking.  The blocks then share the k of the
//                            update of D(a, k) against D(b, k) and list the
//                            rows k < b whose nearest neighbour was a or b.
//           k_hclust_rescan  16 blocks of 1024 threads: a block per listed
//                            row, and one for row a, on the row's contiguous
//                            segment; block 0 then retires b.
//         The O(n) state (nn, dnn, size, live, the list, ia / ib / height) is
//         in global memory and stays in the L2; the matrix is touched at n
//         scattered entries and a few contiguous rows per step.  Why several
//         workgroups and not one that loops over the steps: the rescans need
//         more than one CU's bandwidth (DESIGN.md 6h has the measurement).
#include <cmath>
#include <cstring>
#include <vector>

#include "ks_internal.h"
// after hip_runtime.h (ks_internal.h): the header's functions are __host__ __device__ here
#include "ks_dist_index.h"
#include "ks_finite_check.h"

namespace ks {
namespace {

constexpr int kHcThreads = 1024;  // the merge workgroup: 16 waves
constexpr int kHcWaves = kHcThreads / 64;
constexpr int kHcChunk = 4;       // entries of row a a thread loads before its first store
constexpr int kHcPairRows = 4096; // k_hclust_pair: a block per so many k of the update,
constexpr int kHcPairBlocks = 8;  //   at most so many (each block repeats the arg-min)
constexpr int kHcRescanBlocks = 16;  // k_hclust_rescan: rows rescanned side by side
constexpr int kNone = 0x7fffffff; // "no index": loses every tie, equals no row

// (value, index) ordering of every reduction here: the smaller value, the
// lower index on equal values (-0.0 == +0.0: the index decides).
__device__ __forceinline__ bool hc_before(double v, int i, double bv, int bi) { return v < bv || (v == bv && i < bi); }

__device__ __forceinline__ void hc_wave_min(double &v, int &i, int width) {
  for (int d = width >> 1; d > 0; d >>= 1) {
    const double ov = __shfl_xor(v, d);
    const int oi = __shfl_xor(i, d);
    if (hc_before(ov, oi, v, i)) v = ov, i = oi;
  }
}

// Block arg-min of kHcThreads threads; every thread gets the result.  One
// barrier; sv / si (kHcWaves entries) must not be written again before every
// wave has passed a later barrier.
__device__ __forceinline__ void hc_block_min(double &v, int &i, double *sv, int *si) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  hc_wave_min(v, i, 64);
  if (lane == 0) sv[wave] = v, si[wave] = i;
  __syncthreads();
  v = lane < kHcWaves ? sv[lane] : INFINITY;
  i = lane < kHcWaves ? si[lane] : kNone;
  hc_wave_min(v, i, kHcWaves);
  v = __shfl(v, 0);
  i = __shfl(i, 0);
}

// The O(n) state of a call, one allocation (HcState::bytes).
struct HcState {
  double *dnn, *size, *height;
  int32_t *nn, *ia, *ib, *list;
  unsigned long long *tail;  // [0] rows rescanned, [1] 1: no finite minimum was left (overflow in average linkage)
  int *cnt;                  // [2] rows listed for a rescan, by step parity
  uint8_t *live;
  static size_t bytes(int64_t n) { return (size_t)n * (3 * 8 + 4 * 4 + 1) + 32 + 64; }
  HcState(void *base, int64_t n) {
    char *p = static_cast<char *>(base);
    dnn = reinterpret_cast<double *>(p), p += n * 8;
    size = reinterpret_cast<double *>(p), p += n * 8;
    height = reinterpret_cast<double *>(p), p += n * 8;
    tail = reinterpret_cast<unsigned long long *>(p), p += 16;
    cnt = reinterpret_cast<int *>(p), p += 16;
    nn = reinterpret_cast<int32_t *>(p), p += n * 4;
    ia = reinterpret_cast<int32_t *>(p), p += n * 4;
    ib = reinterpret_cast<int32_t *>(p), p += n * 4;
    list = reinterpret_cast<int32_t *>(p), p += n * 4;
    live = reinterpret_cast<uint8_t *>(p);
  }
};

// Block i: nn[i], dnn[i] of row i < n - 1 from D(i, i+1 .. n-1); live, size of
// row i (block n - 1 only does that).
__global__ void __launch_bounds__(256) k_hclust_init(const double *__restrict__ d, int n, HcState st) {
  __shared__ double sv[4];
  __shared__ int si[4];
  const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) {
    st.live[i] = 1;
    st.size[i] = 1.0;
    if (i == 0) st.tail[0] = 0, st.tail[1] = 0, st.cnt[0] = 0, st.cnt[1] = 0;
  }
  if (i == n - 1) return;  // block-uniform
  const double *row = d + (dist_pair_offset(i, i + 1, n) - (i + 1));  // row[j] = D(i, j)
  double bv = INFINITY;
  int bi = kNone;
#pragma unroll 4
  for (int j = i + 1 + tid; j < n; j += 256) {
    const double v = row[j];
    if (v < bv) bv = v, bi = j;  // ascending j: strict < keeps the lowest
  }
  hc_wave_min(bv, bi, 64);
  if (lane == 0) sv[wave] = bv, si[wave] = bi;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w)
      if (hc_before(sv[w], si[w], bv, bi)) bv = sv[w], bi = si[w];
    st.nn[i] = bi;
    st.dnn[i] = bv;
  }
}

// D(i, j) of the condensed matrix, i != j
__device__ __forceinline__ int64_t hc_at(int i, int j, int n) {
  return i < j ? dist_pair_offset(i, j, n) : dist_pair_offset(j, i, n);
}

// Step s, first half: the closest pair and the update of row a.  Every block
// finds the pair for itself from the same dnn (nothing here writes dnn, nn,
// live or size, so all blocks agree); block 0 records it.  The blocks share
// the k of the update and list the rows to rescan (st.cnt[s & 1], zeroed by
// the previous step's second half).
template <int kMethod>
__global__ void __launch_bounds__(kHcThreads) k_hclust_pair(double *d, int n, int s, HcState st) {
  __shared__ double sv[kHcWaves];
  __shared__ int si[kHcWaves];
  if (st.tail[1]) return;  // an earlier step found nothing to merge
  const int tid = threadIdx.x;
  double hv = INFINITY;
  int im = kNone;
#pragma unroll 8
  for (int i = tid; i < n - 1; i += kHcThreads) {  // dead rows hold +inf
    const double v = st.dnn[i];
    if (v < hv) hv = v, im = i;  // ascending i: strict < keeps the lowest
  }
  hc_block_min(hv, im, sv, si);
  if (im == kNone) {  // uniform over the grid: nothing finite left (average linkage overflowed)
    if (blockIdx.x == 0 && tid == 0) st.tail[1] = 1;
    return;
  }
  const int jm = st.nn[im];  // dnn[im] is finite: nn[im] is a row
  const int a = min(im, jm), b = max(im, jm);
  const double sa = st.size[a], sb = st.size[b];
  const double ssum = sa + sb;
  if (blockIdx.x == 0 && tid == 0) {
    st.ia[s] = a;
    st.ib[s] = b;
    st.height[s] = hv;
  }
  int *cnt = st.cnt + (s & 1);
  // kHcChunk k per thread at a time: every load of a chunk (dead k included:
  // their entries exist) is issued before its first store, so the scattered
  // reads overlap instead of queueing behind stores they might alias
  const int stride = gridDim.x * kHcThreads;
  // no test reaches a second pass of this loop: it needs n > kHcChunk * kHcPairBlocks * kHcThreads = 32,768 (4.3 GB)
  for (int k0 = blockIdx.x * kHcThreads + tid; k0 < n; k0 += kHcChunk * stride) {
    double x[kHcChunk], y[kHcChunk];
    int t[kHcChunk];
    bool lv[kHcChunk];
#pragma unroll
    for (int u = 0; u < kHcChunk; ++u) {
      const int64_t k = (int64_t)k0 + (int64_t)u * stride;
      lv[u] = false, t[u] = kNone, x[u] = y[u] = 0.0;
      if (k < n && k != a && k != b) {
        x[u] = d[hc_at(a, (int)k, n)];
        y[u] = d[hc_at(b, (int)k, n)];
        lv[u] = st.live[k] != 0;
        t[u] = k < b ? st.nn[k] : kNone;  // nn[k] > k: no row from b on points at a or b
      }
    }
#pragma unroll
    for (int u = 0; u < kHcChunk; ++u) {
      if (!lv[u]) continue;
      const int k = k0 + u * stride;
      double r;
      if (kMethod == KS_HCLUST_COMPLETE) {
        r = y[u] > x[u] ? y[u] : x[u];
      } else if (kMethod == KS_HCLUST_SINGLE) {
        r = y[u] < x[u] ? y[u] : x[u];
      } else {
        const double p = sa * x[u], q = sb * y[u];
        r = (p + q) / ssum;
      }
      d[hc_at(a, k, n)] = r;
      if (t[u] == a || t[u] == b) st.list[atomicAdd(cnt, 1)] = k;
    }
  }
}

// Step s, second half: the listed rows and row a rescanned, a block per row
// on its contiguous segment (b is dead here whatever live[b] says: block 0
// writes that flag while others read the array).  Block 0 then retires b.
__global__ void __launch_bounds__(kHcThreads) k_hclust_rescan(const double *d, int n, int s, HcState st) {
  __shared__ double sv[kHcWaves];
  __shared__ int si[kHcWaves];
  if (st.tail[1]) return;
  const int tid = threadIdx.x;
  const int a = st.ia[s], b = st.ib[s], cnt = st.cnt[s & 1];
  for (int r = blockIdx.x; r <= cnt; r += gridDim.x) {  // block-uniform
    const int i = r < cnt ? st.list[r] : a;
    const double *row = d + (dist_pair_offset(i, i + 1, n) - (i + 1));  // row[j] = D(i, j)
    double bv = INFINITY;
    int bi = kNone;
#pragma unroll 8
    for (int j = i + 1 + tid; j < n; j += kHcThreads) {
      const double v = row[j];
      const bool lv = st.live[j] != 0 && j != b;
      if (lv && v < bv) bv = v, bi = j;  // ascending j: strict < keeps the lowest
    }
    hc_block_min(bv, bi, sv, si);
    if (tid == 0) {
      st.nn[i] = bi;
      st.dnn[i] = bv;
    }
    __syncthreads();  // sv / si are free again
  }
  if (blockIdx.x == 0 && tid == 0) {  // b is on nobody's list, and nobody here reads dnn, size or the other counter
    st.live[b] = 0;
    if (b < n - 1) st.dnn[b] = INFINITY;
    st.size[a] = st.size[a] + st.size[b];
    st.cnt[(s + 1) & 1] = 0;
    st.tail[0] += (unsigned long long)cnt + 1;
  }
}

// ------------------------------------------------------------------- host

// ia / ib (0-based rows, a < b; the cluster keeps a's row) -> R's merge and order.
void merge_and_order(const int32_t *ia, const int32_t *ib, int64_t n, int32_t *merge, int32_t *order) {
  std::vector<int32_t> lab((size_t)n);
  for (int64_t i = 0; i < n; ++i) lab[(size_t)i] = -(int32_t)(i + 1);
  for (int64_t s = 0; s < n - 1; ++s) {
    int32_t x = lab[(size_t)ia[s]], y = lab[(size_t)ib[s]];
    // singleton before cluster; two singletons: a < b already; two clusters: the earlier step first
    if ((x > 0 && y < 0) || (x > 0 && y > 0 && y < x)) std::swap(x, y);
    merge[2 * s] = x;
    merge[2 * s + 1] = y;
    lab[(size_t)ia[s]] = (int32_t)(s + 1);
  }
  // leaves left to right, merge[s][0] on the left: an explicit stack, the tree can be a chain
  std::vector<int32_t> stack;
  stack.push_back((int32_t)(n - 1));  // the last step, 1-based
  int64_t o = 0;
  while (!stack.empty()) {
    const int32_t x = stack.back();
    stack.pop_back();
    if (x < 0) {
      order[o++] = -x;
    } else {
      stack.push_back(merge[2 * (int64_t)(x - 1) + 1]);
      stack.push_back(merge[2 * (int64_t)(x - 1)]);
    }
  }
}

ks_status check_hclust_args(int64_t n, int32_t method, int32_t flags, const void *diss, const void *merge,
                            const void *height, const void *order) {
  if (n < 2) return fail(KS_ERR_ARG, "hclust needs at least 2 observations, n = %lld", (long long)n);
  if (n > 0x7ffffffeLL) return fail(KS_ERR_ARG, "n = %lld does not fit the int32 merge table", (long long)n);
  if (method != KS_HCLUST_COMPLETE && method != KS_HCLUST_SINGLE && method != KS_HCLUST_AVERAGE)
    return fail(KS_ERR_ARG, "unknown hclust method %d", (int)method);
  if (flags & ~KS_HCLUST_KEEP_INPUT) return fail(KS_ERR_ARG, "unknown hclust flags 0x%x", (unsigned)flags);
  if (!diss) return fail(KS_ERR_ARG, "null dissimilarities");
  if (!merge || !height || !order) return fail(KS_ERR_ARG, "null output");
  return KS_OK;
}

// Everything validated; diss is a device pointer.
ks_status hclust_impl(ks_ctx *ctx, double *diss, int64_t n, int method, int flags, int32_t *merge, double *height,
                      int32_t *order, ks_hclust_stats *stats) {
  hipStream_t st = ctx->stream;
  const int64_t total = dist_pair_count(n);
  void *scal = nullptr, *state_mem = nullptr;
  KS_TRY(ensure(ctx, SLOT_SCALARS, 4096, &scal));
  KS_TRY(ensure(ctx, SLOT_WORK_A, HcState::bytes(n), &state_mem));
  unsigned long long *bad = static_cast<unsigned long long *>(scal) + kScHclustBad;

  // every entry is checked before anything is modified
  KS_TRY(check_all_finite(ctx, diss, total, bad));

  DevFree copy;
  double *d = diss;
  if (flags & KS_HCLUST_KEEP_INPUT) {
    KS_TRY(dev_alloc(&copy, (size_t)total * 8, "the copy of the dissimilarities"));
    d = static_cast<double *>(copy.p);
  }
  KS_HIP(hipEventRecord(ctx->ev[2], st));
  if (d != diss) KS_HIP(hipMemcpyAsync(d, diss, (size_t)total * 8, hipMemcpyDeviceToDevice, st));
  const HcState hs(state_mem, n);
  hipLaunchKernelGGL(k_hclust_init, dim3((unsigned)n), dim3(256), 0, st, d, (int)n, hs);
  KS_HIP(hipGetLastError());
  KS_HIP(hipEventRecord(ctx->ev[3], st));
  // the step loop stays on the stream: two launches per step, no read-back
  // between them; the device picks the pair and the rows to rescan
  const dim3 pair_grid((unsigned)std::min<int64_t>((n + kHcPairRows - 1) / kHcPairRows, kHcPairBlocks));
  auto *pair_kernel = method == KS_HCLUST_COMPLETE ? k_hclust_pair<KS_HCLUST_COMPLETE>
                      : method == KS_HCLUST_SINGLE ? k_hclust_pair<KS_HCLUST_SINGLE>
                                                   : k_hclust_pair<KS_HCLUST_AVERAGE>;
  for (int s = 0; s < (int)n - 1; ++s) {
    hipLaunchKernelGGL(pair_kernel, pair_grid, dim3(kHcThreads), 0, st, d, (int)n, s, hs);
    hipLaunchKernelGGL(k_hclust_rescan, dim3(kHcRescanBlocks), dim3(kHcThreads), 0, st, d, (int)n, s, hs);
    KS_HIP(hipGetLastError());
  }
  KS_HIP(hipEventRecord(ctx->ev[4], st));

  std::vector<int32_t> iab((size_t)(2 * n));
  unsigned long long tail[2] = {0, 0};
  KS_HIP(hipMemcpyAsync(height, hs.height, (size_t)(n - 1) * 8, hipMemcpyDeviceToHost, st));
  KS_HIP(hipMemcpyAsync(iab.data(), hs.ia, (size_t)(2 * n) * 4, hipMemcpyDeviceToHost, st));  // ia, then ib
  KS_HIP(hipMemcpyAsync(tail, hs.tail, 16, hipMemcpyDeviceToHost, st));
  KS_HIP(hipStreamSynchronize(st));  // the copy is freed on return
  if (tail[1])
    return fail(KS_ERR_ARG, "no finite dissimilarity was left to merge: the averages overflowed");
  merge_and_order(iab.data(), iab.data() + n, n, merge, order);
  if (stats) {
    KS_TRY(event_ms(ctx, 0, 4, &stats->ms_total));
    KS_TRY(event_ms(ctx, 0, 1, &stats->ms_check));
    KS_TRY(event_ms(ctx, 2, 3, &stats->ms_init));
    KS_TRY(event_ms(ctx, 3, 4, &stats->ms_merge));
    stats->n = n;
    stats->n_rescans = (int64_t)tail[0];
    stats->work_bytes = copy.p ? total * 8 : 0;
  }
  return KS_OK;
}

}  // namespace
}  // namespace ks

using namespace ks;

extern "C" ks_status ks_hclust_dev(ks_ctx *ctx, double *diss_dev, int64_t n, int32_t method, int32_t flags,
                                   int32_t *merge, double *height, int32_t *order, ks_hclust_stats *stats) {
  if (stats) memset(stats, 0, sizeof(*stats));
  KS_TRY(check_hclust_args(n, method, flags, diss_dev, merge, height, order));
  KS_TRY(default_ctx(&ctx));
  KS_ENTER(ctx);
  return hclust_impl(ctx, diss_dev, n, method, flags, merge, height, order, stats);
}

extern "C" ks_status ks_hclust(ks_ctx *ctx, const double *diss, int64_t n, int32_t method, int32_t *merge,
                               double *height, int32_t *order) {
  KS_TRY(check_hclust_args(n, method, 0, diss, merge, height, order));
  const int64_t total = dist_pair_count(n);
  for (int64_t o = 0; o < total; ++o)
    if (!std::isfinite(diss[o])) return not_finite((unsigned long long)o);
  KS_TRY(default_ctx(&ctx));
  KS_ENTER(ctx);
  const HostEnd host_end{ctx};  // (ks_set_host_cache)
  void *d = nullptr;
  KS_TRY(ensure(ctx, SLOT_REG_TMP, (size_t)total * 8, &d));
  KS_HIP(hipMemcpyAsync(d, diss, (size_t)total * 8, hipMemcpyHostToDevice, ctx->stream));
  return hclust_impl(ctx, static_cast<double *>(d), n, method, 0, merge, height, order, nullptr);  // the upload is consumed
}

extern "C" ks_status ks_hclust_cut(const int32_t *merge, const double *height, int64_t n, int32_t k, double h,
                                   int32_t *group) {
  if (n < 2) return fail(KS_ERR_ARG, "hclust needs at least 2 observations, n = %lld", (long long)n);
  if (n > 0x7ffffffeLL) return fail(KS_ERR_ARG, "n = %lld does not fit the int32 merge table", (long long)n);
  if (!merge || !group) return fail(KS_ERR_ARG, "null merge table or output");
  if (k < 0 || k > n) return fail(KS_ERR_ARG, "k = %d is not in 1 .. n = %lld", (int)k, (long long)n);
  if (k == 0) {
    if (!height) return fail(KS_ERR_ARG, "a cut at a height needs the heights");
    if (std::isnan(h)) return fail(KS_ERR_ARG, "the cut height is NaN");
    int64_t below = 0;
    for (int64_t s = 0; s < n - 1; ++s) {
      if (std::isnan(height[s]) || (s > 0 && height[s] < height[s - 1]))
        return fail(KS_ERR_ARG, "the heights are not sorted: step %lld lies below step %lld", (long long)s,
                    (long long)(s - 1));
      if (height[s] <= h) ++below;
    }
    k = (int32_t)(n - below);
  }
  // nodes: observation i is node i, step t is node n + t; the first n - k steps are applied
  const int64_t applied = n - k;
  std::vector<int32_t> parent((size_t)(n + applied), -1);
  for (int64_t t = 0; t < applied; ++t)
    for (int c = 0; c < 2; ++c) {
      const int32_t x = merge[2 * t + c];
      if (x == 0 || x < -n || x > t)
        return fail(KS_ERR_ARG, "merge[%lld][%d] = %d is neither an observation nor an earlier step", (long long)t, c,
                    (int)x);
      parent[(size_t)(x < 0 ? -x - 1 : n + x - 1)] = (int32_t)(n + t);
    }
  // a step's parent is a later step: roots settle from the last node down
  std::vector<int32_t> root((size_t)(n + applied));
  for (int64_t v = n + applied - 1; v >= 0; --v)
    root[(size_t)v] = parent[(size_t)v] < 0 ? (int32_t)v : root[(size_t)parent[(size_t)v]];
  std::vector<int32_t> number((size_t)(n + applied), 0);  // groups numbered by first appearance
  int32_t next = 0;
  for (int64_t i = 0; i < n; ++i) {
    int32_t &g = number[(size_t)root[(size_t)i]];
    if (!g) g = ++next;
    group[i] = g;
  }
  return KS_OK;
}
