// ks_nj.hip -- neighbour joining of a condensed dissimilarity vector on the
// device (ks_nj_dev / ks_nj) and the host-only conversion to an edge table
// (ks_nj_edges); the contract is in include/kmer_spans.h.
//
// The tree the reference's author wanted of dist() of the spectra and found
// "far, far to slow" on the host (test.R:770-775, :861-864).  The condensed
// matrix stays in HBM as ks_spectra_dist_dev wrote it and is updated in place.
//
// The algorithm is canonical neighbour joining, fixed in the header as an
// order of FP64 operations (no FMA: -ffp-contract=off, csrc/Makefile) and of
// comparisons (strict <, lexicographic (i, j): the lowest pair wins every tie).
//
// Check:  the finiteness pass of hclust (ks_finite_check.h).
// Init:   k_nj_init: a thread per row i sums D(i, j) with j ascending in one
//         accumulator.  The j < i part reads D(j, i), consecutive across the
//         threads; the j > i part walks the thread's own row, so a wave reads
//         64 rows at once, 8 bytes of each (a cache line serves 16 consecutive
//         j of a lane).  It runs once per call; DESIGN.md 6j has what it costs.
// Join:   two launches per step, 2 (n - 3) in all, queued on the stream with no
//         read-back between them.  No kernel waits on another workgroup; stream
//         order is the only synchronisation between workgroups.
//           k_nj_min   up to 2,048 blocks of 256 threads over the live rows,
//                      rows i and m - 2 - i to a block so that every block has
//                      the same number of entries.  q of every pair of the row
//                      segment D(i, i+1 .. m-1) (16-byte loads past a head
//                      entry where the segment starts at an odd offset), S of
//                      a dead column being NaN, so that its q wins no
//                      comparison; a dead row's segment is never read.  Per
//                      row ascending j with a strict <, then (q, i, j) with
//                      the lower pair on equal q in every merge, wave shuffle
//                      and LDS stage.  One (q, i, j) per block.
//           k_nj_join  up to 8 blocks of 1,024 threads.  Every block repeats
//                      the reduction over the blocks' minima -- the kernel
//                      writes none of them, so all blocks agree without
//                      talking.  Block 0 records the join, the lengths and
//                      S[a], and retires b (no other thread reads those); the
//                      blocks share the k of the row update D(a, k) and of
//                      S[k].  D(k, a) for k < a is strided: a thread loads
//                      four k before its first store.
// Compaction: dead columns inside live rows are read and rejected, a waste
//         that grows as r falls.  When the live count drops to half the
//         stored dimension m, k_nj_rank lists the live rows in order and
//         k_nj_compact writes the matrix of those rows to the other of two
//         buffers (the matrix itself and one of a quarter of its size); S and
//         node move with it.  The order of the rows is kept, so the stored
//         order is the original order and every tie falls as before; the host
//         knows r = n - s and with it the steps at which to compact.
#include <cmath>
#include <cstring>
#include <vector>

#include "ks_internal.h"
// after hip_runtime.h (ks_internal.h): the header's functions are __host__ __device__ here
#include "ks_dist_index.h"
#include "ks_finite_check.h"

namespace ks {
namespace {

constexpr int kNjMinThreads = 256;  // k_nj_min: 4 waves
constexpr int kNjMinBlocks = 2048;  //   grid cap = the minima k_nj_join reduces
constexpr int kNjThreads = 1024;    // k_nj_join, k_nj_rank, k_nj_root: 16 waves
constexpr int kNjWaves = kNjThreads / 64;
constexpr int kNjChunk = 4;         // k of the row update a thread loads before its first store
constexpr int kNjJoinRows = 4096;   // k_nj_join: a block per so many k of the update,
constexpr int kNjJoinBlocks = 8;    //   at most so many (each block repeats the reduction)
constexpr int kNjMinDim = 8;        // no compaction to fewer rows than this
constexpr int kNoCol = 0x7fffffff;
constexpr unsigned long long kNoKey = ~0ULL;  // "no pair": loses every tie

// (q, i, j) ordering of every reduction here, key = i << 32 | j: the smaller
// q, the lower pair on equal q (-0.0 == +0.0: the pair decides).
__device__ __forceinline__ bool nj_before(double v, unsigned long long k, double bv, unsigned long long bk) {
  return v < bv || (v == bv && k < bk);
}

__device__ __forceinline__ void nj_wave_min(double &v, unsigned long long &k, int width) {
  for (int d = width >> 1; d > 0; d >>= 1) {
    const double ov = __shfl_xor(v, d);
    const unsigned long long ok = __shfl_xor(k, d);
    if (nj_before(ov, ok, v, k)) v = ov, k = ok;
  }
}

// Block minimum of kWaves * 64 threads; every thread gets the result.  One barrier.
template <int kWaves>
__device__ __forceinline__ void nj_block_min(double &v, unsigned long long &k, double *sv, unsigned long long *sk) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  nj_wave_min(v, k, 64);
  if (lane == 0) sv[wave] = v, sk[wave] = k;
  __syncthreads();
  v = lane < kWaves ? sv[lane] : INFINITY;
  k = lane < kWaves ? sk[lane] : kNoKey;
  nj_wave_min(v, k, kWaves);
  v = __shfl(v, 0);
  k = __shfl(k, 0);
}

// The O(n) state of a call, one allocation (NjState::bytes).  S and node exist
// twice: a compaction writes the other copy and the host swaps them.
struct NjState {
  double *S, *S_alt, *length, *minv, *root_length;
  unsigned long long *minkey, *tail;  // tail[0] != 0: the call failed (1: no pair had q < +inf)
  int32_t *node, *node_alt, *map, *join, *root;
  uint8_t *live;
  static size_t bytes(int64_t n) {
    return (size_t)n * (4 * 8 + 5 * 4 + 1) + (size_t)kNjMinBlocks * 16 + 4 * 8 + 2 * 8 + 4 * 4 + 64;
  }
  NjState(void *base, int64_t n) {
    char *p = static_cast<char *>(base);
    S = reinterpret_cast<double *>(p), p += n * 8;
    S_alt = reinterpret_cast<double *>(p), p += n * 8;
    length = reinterpret_cast<double *>(p), p += 2 * n * 8;
    minv = reinterpret_cast<double *>(p), p += kNjMinBlocks * 8;
    root_length = reinterpret_cast<double *>(p), p += 4 * 8;
    minkey = reinterpret_cast<unsigned long long *>(p), p += kNjMinBlocks * 8;
    tail = reinterpret_cast<unsigned long long *>(p), p += 2 * 8;
    node = reinterpret_cast<int32_t *>(p), p += n * 4;
    node_alt = reinterpret_cast<int32_t *>(p), p += n * 4;
    map = reinterpret_cast<int32_t *>(p), p += n * 4;
    join = reinterpret_cast<int32_t *>(p), p += 2 * n * 4;
    root = reinterpret_cast<int32_t *>(p), p += 4 * 4;
    live = reinterpret_cast<uint8_t *>(p);
  }
};

// Thread i: S[i] = the sum of D(i, j), j ascending, one accumulator from +0.0;
// live, node of row i.
__global__ void __launch_bounds__(256) k_nj_init(const double *__restrict__ d, int n, NjState st) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double acc = 0.0;
  int64_t off = i - 1;  // D(0, i); D(j + 1, i) lies n - j - 2 further on
#pragma unroll 8
  for (int j = 0; j < i; ++j) {
    acc = acc + d[off];
    off += n - j - 2;
  }
  if (i < n - 1) {
    const double *row = d + (dist_pair_offset(i, i + 1, n) - (i + 1));  // row[j] = D(i, j)
#pragma unroll 8
    for (int j = i + 1; j < n; ++j) acc = acc + row[j];
  }
  st.S[i] = acc;
  st.live[i] = 1;
  st.node[i] = -(i + 1);
  if (i == 0) st.tail[0] = 0, st.tail[1] = 0;
}

// Step s, first half: the smallest q = ((r - 2) D(i, j) - S[i]) - S[j] of the
// block's live rows, as (q, i << 32 | j), into minv / minkey[blockIdx.x].
// m: the stored dimension, r: the live rows.
__global__ void __launch_bounds__(kNjMinThreads) k_nj_min(const double *__restrict__ d, int m, int r, NjState st) {
  __shared__ double sv[kNjMinThreads / 64];
  __shared__ unsigned long long sk[kNjMinThreads / 64];
  if (st.tail[0]) return;
  const int tid = threadIdx.x;
  const double rm2 = (double)(r - 2);
  const double *__restrict__ S = st.S;
  double bq = INFINITY;
  unsigned long long bk = kNoKey;
  const int nhalf = m / 2;  // rows 0 .. m - 2 taken as p and m - 2 - p
  for (int p = blockIdx.x; p < nhalf; p += gridDim.x) {
    for (int h = 0; h < 2; ++h) {
      const int i = h ? m - 2 - p : p;
      if (h && i == p) break;
      if (!st.live[i]) continue;  // block-uniform
      const double si = S[i];
      const double *row = d + (dist_pair_offset(i, i + 1, m) - (i + 1));  // row[j] = D(i, j)
      double rq = INFINITY;
      int rj = kNoCol;
      // ascending j per thread, strict <: the lowest j of the smallest q.  A dead
      // column has S = NaN: its q is NaN and wins no comparison.
      int j0 = i + 1;
      if (reinterpret_cast<uintptr_t>(row + j0) & 15) {  // block-uniform: one entry up to the 16-byte boundary
        if (tid == 0) {
          const double q = (rm2 * row[j0] - si) - S[j0];
          if (q < rq) rq = q, rj = j0;
        }
        ++j0;
      }
      const int n2 = (m - j0) >> 1;
      const double2 *row2 = reinterpret_cast<const double2 *>(row + j0);
#pragma unroll 4
      for (int t = tid; t < n2; t += kNjMinThreads) {
        const double2 x = row2[t];
        const int j = j0 + 2 * t;
        const double q0 = (rm2 * x.x - si) - S[j], q1 = (rm2 * x.y - si) - S[j + 1];
        if (q0 < rq) rq = q0, rj = j;
        if (q1 < rq) rq = q1, rj = j + 1;
      }
      if (((m - j0) & 1) && tid == 0) {  // the last entry of an odd remainder: the thread's highest j
        const double q = (rm2 * row[m - 1] - si) - S[m - 1];
        if (q < rq) rq = q, rj = m - 1;
      }
      const unsigned long long key = (unsigned long long)(unsigned)i << 32 | (unsigned)rj;
      if (rj != kNoCol && nj_before(rq, key, bq, bk)) bq = rq, bk = key;
    }
  }
  nj_block_min<kNjMinThreads / 64>(bq, bk, sv, sk);
  if (tid == 0) st.minv[blockIdx.x] = bq, st.minkey[blockIdx.x] = bk;
}

// D(i, j) of the condensed matrix of m rows, i != j
__device__ __forceinline__ int64_t nj_at(int i, int j, int m) {
  return i < j ? dist_pair_offset(i, j, m) : dist_pair_offset(j, i, m);
}

// Step s, second half: the pair, the join and the update of row a and of S.
// Every block finds the pair for itself from the same nmin minima; block 0
// records it.  What block 0's first thread writes (S[a], S[b], live[b],
// node[a], the outputs) no other thread reads: they touch k != a, b only.
__global__ void __launch_bounds__(kNjThreads) k_nj_join(double *d, int m, int r, int s, int nmin, NjState st) {
  __shared__ double sv[kNjWaves];
  __shared__ unsigned long long sk[kNjWaves];
  if (st.tail[0]) return;
  const int tid = threadIdx.x;
  double bq = INFINITY;
  unsigned long long bk = kNoKey;
  for (int t = tid; t < nmin; t += kNjThreads) {
    const double v = st.minv[t];
    const unsigned long long k = st.minkey[t];
    if (nj_before(v, k, bq, bk)) bq = v, bk = k;
  }
  nj_block_min<kNjWaves>(bq, bk, sv, sk);
  if (bk == kNoKey) {  // uniform over the grid: no pair has q < +inf (the sums overflowed)
    if (blockIdx.x == 0 && tid == 0) st.tail[0] = 1;
    return;
  }
  const int a = (int)(bk >> 32), b = (int)(bk & 0xffffffffu);
  const double dab = d[dist_pair_offset(a, b, m)];
  if (blockIdx.x == 0 && tid == 0) {
    const double sa = st.S[a], sb = st.S[b];
    const double delta = (sa - sb) / (double)(r - 2);
    st.join[2 * s] = st.node[a];
    st.join[2 * s + 1] = st.node[b];
    st.length[2 * s] = 0.5 * (dab + delta);
    st.length[2 * s + 1] = 0.5 * (dab - delta);
    st.S[a] = 0.5 * ((sa + sb) - (double)r * dab);
    st.S[b] = NAN;  // a dead column's q loses every comparison in k_nj_min
    st.live[b] = 0;
    st.node[a] = s + 1;
  }
  // kNjChunk k per thread at a time: every load of a chunk is issued before
  // its first store, so the scattered reads overlap
  const int stride = gridDim.x * kNjThreads;
  // no test reaches a second pass of this loop: it needs m > kNjChunk * kNjJoinBlocks * kNjThreads = 32,768 (4.3 GB)
  for (int k0 = blockIdx.x * kNjThreads + tid; k0 < m; k0 += kNjChunk * stride) {
    double x[kNjChunk], y[kNjChunk], sk_[kNjChunk];
    bool lv[kNjChunk];
#pragma unroll
    for (int u = 0; u < kNjChunk; ++u) {
      const int64_t k = (int64_t)k0 + (int64_t)u * stride;
      lv[u] = false, x[u] = y[u] = sk_[u] = 0.0;
      if (k < m && k != a && k != b && st.live[k]) {
        lv[u] = true;
        x[u] = d[nj_at(a, (int)k, m)];
        y[u] = d[nj_at(b, (int)k, m)];
        sk_[u] = st.S[k];
      }
    }
#pragma unroll
    for (int u = 0; u < kNjChunk; ++u) {
      if (!lv[u]) continue;
      const int k = k0 + u * stride;
      const double dn = 0.5 * ((x[u] + y[u]) - dab);
      st.S[k] = ((sk_[u] - x[u]) - y[u]) + dn;
      d[nj_at(a, k, m)] = dn;
    }
  }
}

// Compaction, first half (one block): the live rows of 0 .. m - 1 in order.
// map[new] = old; S and node of the live rows go to the other copy; live is
// true for rows 0 .. r - 1 of the compacted state.
__global__ void __launch_bounds__(kNjThreads) k_nj_rank(int m, int r, NjState st) {
  __shared__ int sc[kNjThreads];
  const int tid = threadIdx.x;
  const int per = (m + kNjThreads - 1) / kNjThreads;
  const int lo = min(tid * per, m), hi = min(lo + per, m);
  int cnt = 0;
  for (int p = lo; p < hi; ++p) cnt += st.live[p] != 0;
  sc[tid] = cnt;
  __syncthreads();
  for (int off = 1; off < kNjThreads; off <<= 1) {  // inclusive scan
    const int v = tid >= off ? sc[tid - off] : 0;
    __syncthreads();
    sc[tid] += v;
    __syncthreads();
  }
  int at = sc[tid] - cnt;
  for (int p = lo; p < hi; ++p)
    if (st.live[p]) {
      st.map[at] = p;
      st.S_alt[at] = st.S[p];
      st.node_alt[at] = st.node[p];
      ++at;
    }
  __syncthreads();  // every read of live is done
  for (int p = tid; p < r; p += kNjThreads) st.live[p] = 1;
}

// Compaction, second half: block p writes row p of the r live rows,
// dst(p, q) = src(map[p], map[q]); map ascends, so the pair stays in the
// upper triangle.
__global__ void __launch_bounds__(256) k_nj_compact(const double *__restrict__ src, double *__restrict__ dst, int m,
                                                    int r, NjState st) {
  const int p = blockIdx.x;  // < r - 1
  const int op = st.map[p];
  const double *srow = src + (dist_pair_offset(op, op + 1, m) - (op + 1));
  double *drow = dst + (dist_pair_offset(p, p + 1, r) - (p + 1));
#pragma unroll 4
  for (int q = p + 1 + threadIdx.x; q < r; q += 256) drow[q] = srow[st.map[q]];
}

// After the last join (one block): the three live rows x < y < z and the
// lengths of their edges to the trifurcation.
__global__ void __launch_bounds__(kNjThreads) k_nj_root(const double *__restrict__ d, int m, NjState st) {
  __shared__ int cnt;
  __shared__ int idx[3];
  const int tid = threadIdx.x;
  if (tid == 0) cnt = 0;
  __syncthreads();
  for (int k = tid; k < m; k += kNjThreads)
    if (st.live[k]) {
      const int t = atomicAdd(&cnt, 1);
      if (t < 3) idx[t] = k;
    }
  __syncthreads();
  if (tid != 0 || st.tail[0]) return;
  if (cnt != 3) {
    st.tail[0] = 2;
    return;
  }
  int x = idx[0], y = idx[1], z = idx[2], t;
  if (x > y) t = x, x = y, y = t;
  if (y > z) t = y, y = z, z = t;
  if (x > y) t = x, x = y, y = t;
  const double dxy = d[dist_pair_offset(x, y, m)], dxz = d[dist_pair_offset(x, z, m)], dyz = d[dist_pair_offset(y, z, m)];
  st.root[0] = st.node[x], st.root[1] = st.node[y], st.root[2] = st.node[z];
  st.root_length[0] = 0.5 * ((dxy + dxz) - dyz);
  st.root_length[1] = 0.5 * ((dxy + dyz) - dxz);
  st.root_length[2] = 0.5 * ((dxz + dyz) - dxy);
}

// ------------------------------------------------------------------- host

ks_status check_nj_args(int64_t n, int32_t flags, const void *diss, const void *join, const void *length,
                        const void *root, const void *root_length) {
  if (n < 3) return fail(KS_ERR_ARG, "neighbour joining needs at least 3 observations, n = %lld", (long long)n);
  if (n > 0x7ffffffeLL) return fail(KS_ERR_ARG, "n = %lld does not fit the int32 join table", (long long)n);
  if (flags & ~(KS_NJ_KEEP_INPUT | KS_NJ_NO_COMPACT)) return fail(KS_ERR_ARG, "unknown nj flags 0x%x", (unsigned)flags);
  if (!diss) return fail(KS_ERR_ARG, "null dissimilarities");
  if (!join || !length || !root || !root_length) return fail(KS_ERR_ARG, "null output");
  return KS_OK;
}

// Everything validated; diss is a device pointer.
ks_status nj_impl(ks_ctx *ctx, double *diss, int64_t n, int flags, int32_t *join, double *length, int32_t *root,
                  double *root_length, ks_nj_stats *stats) {
  hipStream_t st = ctx->stream;
  const int64_t total = dist_pair_count(n);
  void *scal = nullptr, *state_mem = nullptr;
  KS_TRY(ensure(ctx, SLOT_SCALARS, 4096, &scal));
  KS_TRY(ensure(ctx, SLOT_WORK_A, NjState::bytes(n), &state_mem));

  // every entry is checked before anything is modified
  KS_TRY(check_all_finite(ctx, diss, total, static_cast<unsigned long long *>(scal) + kScNjBad));

  DevFree copy, half;
  double *cur = diss, *other = nullptr;
  int64_t work = 0;
  if (flags & KS_NJ_KEEP_INPUT) {
    KS_TRY(dev_alloc(&copy, (size_t)total * 8, "the copy of the dissimilarities"));
    cur = static_cast<double *>(copy.p);
    work += total * 8;
  }
  // the first compaction is to at most n / 2 rows, each later one fits the buffer it left two before
  const bool compacting = !(flags & KS_NJ_NO_COMPACT) && n / 2 >= kNjMinDim;
  if (compacting) {
    const int64_t half_bytes = dist_pair_count(n / 2) * 8;
    KS_TRY(dev_alloc(&half, (size_t)half_bytes, "the compaction buffer"));
    other = static_cast<double *>(half.p);
    work += half_bytes;
  }
  KS_HIP(hipEventRecord(ctx->ev[2], st));
  if (cur != diss) KS_HIP(hipMemcpyAsync(cur, diss, (size_t)total * 8, hipMemcpyDeviceToDevice, st));
  NjState ns(state_mem, n);
  hipLaunchKernelGGL(k_nj_init, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, cur, (int)n, ns);
  KS_HIP(hipGetLastError());
  KS_HIP(hipEventRecord(ctx->ev[3], st));
  // the step loop stays on the stream: two launches per step, no read-back;
  // r = n - s is known here, and with it when to compact
  int m = (int)n;
  int64_t n_compactions = 0;
  for (int s = 0; s < (int)n - 3; ++s) {
    const int r = (int)n - s;
    const int nmin = std::min(m / 2, kNjMinBlocks);
    const int join_grid = std::min((m + kNjJoinRows - 1) / kNjJoinRows, kNjJoinBlocks);
    hipLaunchKernelGGL(k_nj_min, dim3((unsigned)nmin), dim3(kNjMinThreads), 0, st, cur, m, r, ns);
    hipLaunchKernelGGL(k_nj_join, dim3((unsigned)join_grid), dim3(kNjThreads), 0, st, cur, m, r, s, nmin, ns);
    const int left = r - 1;
    if (compacting && 2 * left <= m && left >= kNjMinDim) {
      hipLaunchKernelGGL(k_nj_rank, dim3(1), dim3(kNjThreads), 0, st, m, left, ns);
      hipLaunchKernelGGL(k_nj_compact, dim3((unsigned)(left - 1)), dim3(256), 0, st, cur, other, m, left, ns);
      std::swap(cur, other);
      std::swap(ns.S, ns.S_alt);
      std::swap(ns.node, ns.node_alt);
      m = left;
      ++n_compactions;
    }
    KS_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(k_nj_root, dim3(1), dim3(kNjThreads), 0, st, cur, m, ns);
  KS_HIP(hipGetLastError());
  KS_HIP(hipEventRecord(ctx->ev[4], st));

  unsigned long long tail[2] = {0, 0};
  if (n > 3) {
    KS_HIP(hipMemcpyAsync(join, ns.join, (size_t)(n - 3) * 2 * 4, hipMemcpyDeviceToHost, st));
    KS_HIP(hipMemcpyAsync(length, ns.length, (size_t)(n - 3) * 2 * 8, hipMemcpyDeviceToHost, st));
  }
  KS_HIP(hipMemcpyAsync(root, ns.root, 3 * 4, hipMemcpyDeviceToHost, st));
  KS_HIP(hipMemcpyAsync(root_length, ns.root_length, 3 * 8, hipMemcpyDeviceToHost, st));
  KS_HIP(hipMemcpyAsync(tail, ns.tail, 16, hipMemcpyDeviceToHost, st));
  KS_HIP(hipStreamSynchronize(st));  // the buffers are freed on return
  if (tail[0] == 1) return fail(KS_ERR_ARG, "no pair with a criterion below +inf was left to join: the row sums overflowed");
  if (tail[0]) return fail(KS_ERR_DEVICE, "neighbour joining did not end with three live rows");
  if (stats) {
    KS_TRY(event_ms(ctx, 0, 4, &stats->ms_total));
    KS_TRY(event_ms(ctx, 0, 1, &stats->ms_check));
    KS_TRY(event_ms(ctx, 2, 3, &stats->ms_init));
    KS_TRY(event_ms(ctx, 3, 4, &stats->ms_join));
    stats->n = n;
    stats->n_compactions = n_compactions;
    stats->work_bytes = work;
  }
  return KS_OK;
}

}  // namespace
}  // namespace ks

using namespace ks;

extern "C" ks_status ks_nj_dev(ks_ctx *ctx, double *diss_dev, int64_t n, int32_t flags, int32_t *join, double *length,
                               int32_t *root, double *root_length, ks_nj_stats *stats) {
  if (stats) memset(stats, 0, sizeof(*stats));
  KS_TRY(check_nj_args(n, flags, diss_dev, join, length, root, root_length));
  KS_TRY(default_ctx(&ctx));
  KS_ENTER(ctx);
  return nj_impl(ctx, diss_dev, n, flags, join, length, root, root_length, stats);
}

extern "C" ks_status ks_nj(ks_ctx *ctx, const double *diss, int64_t n, int32_t *join, double *length, int32_t *root,
                           double *root_length) {
  KS_TRY(check_nj_args(n, 0, diss, join, length, root, root_length));
  const int64_t total = dist_pair_count(n);
  for (int64_t o = 0; o < total; ++o)
    if (!std::isfinite(diss[o])) return not_finite((unsigned long long)o);
  KS_TRY(default_ctx(&ctx));
  KS_ENTER(ctx);
  const HostEnd host_end{ctx};  // (ks_set_host_cache)
  void *d = nullptr;
  KS_TRY(ensure(ctx, SLOT_REG_TMP, (size_t)total * 8, &d));
  KS_HIP(hipMemcpyAsync(d, diss, (size_t)total * 8, hipMemcpyHostToDevice, ctx->stream));
  return nj_impl(ctx, static_cast<double *>(d), n, 0, join, length, root, root_length, nullptr);  // the upload is consumed
}

extern "C" ks_status ks_nj_edges(const int32_t *join, const double *length, const int32_t *root,
                                 const double *root_length, int64_t n, int32_t *edge, double *edge_length) {
  if (n < 3) return fail(KS_ERR_ARG, "neighbour joining needs at least 3 observations, n = %lld", (long long)n);
  if (n > 0x3ffffffeLL) return fail(KS_ERR_ARG, "n = %lld does not fit the int32 edge table", (long long)n);
  if (!root || !root_length || !edge || !edge_length) return fail(KS_ERR_ARG, "null tree table or output");
  if (n > 3 && (!join || !length)) return fail(KS_ERR_ARG, "null tree table or output");
  const int64_t steps = n - 3;
  // a code names a tip, -n .. -1, or a step, 1 .. steps (in join[t]: an earlier
  // one, 1 .. t); the 2n - 3 slots hold the n tips and the n - 3 steps, so a
  // table that leaves a node out uses another twice, and is rejected for that
  std::vector<uint8_t> used((size_t)(n + steps), 0);  // tip i at i, step t at n + t
  auto claim = [&](int32_t x, int64_t max_step, const char *table, long long row, int col) -> ks_status {
    if (x == 0 || x < -n || x > max_step)
      return fail(KS_ERR_ARG, "%s[%lld][%d] = %d is neither an observation nor an earlier step", table, row, col, (int)x);
    uint8_t &u = used[(size_t)(x < 0 ? -x - 1 : n + x - 1)];
    if (u) return fail(KS_ERR_ARG, "%s[%lld][%d] = %d: the node is used twice", table, row, col, (int)x);
    u = 1;
    return KS_OK;
  };
  for (int64_t t = 0; t < steps; ++t)
    for (int c = 0; c < 2; ++c) KS_TRY(claim(join[2 * t + c], t, "join", (long long)t, c));
  for (int c = 0; c < 3; ++c) KS_TRY(claim(root[c], steps, "root", 0, c));
  // preorder from the trifurcation, children in stored order: an explicit
  // stack, the tree can be a chain n deep
  struct Item {
    int32_t code, parent;
    double len;
  };
  auto id_of = [n](int32_t x) { return x < 0 ? -x : (int32_t)(2 * n - 2 - (x - 1)); };
  std::vector<Item> stack;
  for (int c = 2; c >= 0; --c) stack.push_back({root[c], (int32_t)(n + 1), root_length[c]});
  int64_t e = 0;
  while (!stack.empty()) {
    const Item it = stack.back();
    stack.pop_back();
    const int32_t id = id_of(it.code);
    edge[2 * e] = it.parent;
    edge[2 * e + 1] = id;
    edge_length[e++] = it.len;
    if (it.code > 0) {
      const int64_t t = it.code - 1;
      stack.push_back({join[2 * t + 1], id, length[2 * t + 1]});
      stack.push_back({join[2 * t], id, length[2 * t]});
    }
  }
  return KS_OK;
}
