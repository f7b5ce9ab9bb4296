// ks_kmeans.hip -- Lloyd k-means and group mean spectra of row-normalised
// region spectra (ks_spectra_kmeans / ks_spectra_group_means and their _dev
// forms); the contract is in include/kmer_spans.h.
//
// The one way of grouping regions that does not go through the condensed
// distance matrix: R's kmeans(x, centers, iter.max, algorithm = "Lloyd") on the
// profiles, and the mean spectrum of every group of a labelling (the bridge
// from ks_hclust_cut).  Memory is O((m + g) ncol); nothing of size m x g or
// m x m exists.
//
// Every value is fixed in the header as an order of separate FP64 operations
// (-ffp-contract=off, csrc/Makefile): the squared distance is the inner loop of
// ks_spectra_dist, one accumulator per (row, centre), columns ascending; a sum
// over a group takes its members in ascending position order, cut into chunks
// of KS_KM_CHUNK, a partial per chunk, the partials added in chunk order.
//
// Normalise: the shared row-major profile panel [m][ncol] (ks_panel.hip; the
//            update reads whole member rows).  Non-finite centres and bad
//            initial rows are recorded beside the panel's own two words, in the
//            same way, and one 32-byte read-back ends the call before any
//            output is written.
// Assign:    k_km_assign: a block of 256 threads keeps 64 rows and walks centre
//            tiles of 64, a thread a 4 x 4 register block of accumulators as in
//            k_dist_tile; chunks of 16 columns of both are staged in LDS,
//            transposed on the way in.  After a tile every thread folds its 16
//            values into a running (value, label) minimum per row; the minimum
//            over (value, label) pairs is lexicographic and so exact in any
//            order: the 16 threads of a row merge with shuffles.  With few rows
//            the centre tiles are split over blockIdx.y; k_km_merge merges the
//            splits by the same rule, writes the labels and counts the changed
//            ones (an integer atomic per wave).
// Members:   hipcub::DeviceRadixSort::SortPairs (stable) of (label, position);
//            k_km_bounds finds every group's start in the sorted labels by
//            binary search (no histogram atomics), k_km_cscan scans the chunk
//            counts in one block.  Nothing comes back to the host.
// Sums:      k_km_partial: lanes along the columns, a thread runs the <= 256
//            long chain of its column over its chunk's member rows (512-byte
//            row segments per wave); the launch covers the bound m / 256 + g on
//            the chunk count and a block finds its group by binary search in
//            the chunk bases.  k_km_fold adds a group's partials in chunk order
//            and divides.  withinss runs the same pair over one value per
//            member (k_km_rowdist: the distance of a row to its own centre).
// The host loop reads back 4 bytes per pass: the changed count.
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include <hipcub/hipcub.hpp>

#include "ks_internal.h"
#include "ks_panel.h"

namespace ks {
namespace {

constexpr int kKT = 64;   // tile edge: rows x centres
constexpr int kKK = 16;   // columns per LDS chunk
constexpr int kKPadA = 66;  // row stride of the row image: 16-byte aligned rows, 128-bit reads of 4 rows
constexpr int kKPadB = 65;  // row stride of the centre image: conflict-free transposed stores
constexpr int kFoldBatch = 8;

enum FoldMode : int { kFoldMeanKeep = 0, kFoldMeanNan = 1, kFoldSum = 2 };

struct KmState {
  // cnt - position of the first bad row index / empty row / non-finite centre entry / bad initial row (0: none)
  unsigned long long bad[4];
  int changed;
  int pad;
};

__global__ void __launch_bounds__(256) k_km_check_init(const double *__restrict__ init, int64_t total,
                                                       KmState *__restrict__ state) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride)
    if (!isfinite(init[i])) atomicMax(&state->bad[2], (unsigned long long)(total - i));
}

__global__ void __launch_bounds__(256) k_km_check_init_rows(const int64_t *__restrict__ init_rows, int g, int64_t m,
                                                            KmState *__restrict__ state) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= g) return;
  const int64_t r = init_rows[j];
  if (r < 0 || r >= m) atomicMax(&state->bad[3], (unsigned long long)(g - j));
}

// cen[j][c] = panel[init_rows[j]][c]: a centre that is a row's profile, bit for bit.
__global__ void __launch_bounds__(256) k_km_gather_init(const double *__restrict__ panel, int ncol,
                                                        const int64_t *__restrict__ init_rows, int64_t total,
                                                        double *__restrict__ cen) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int64_t j = i / ncol;
    const int c = (int)(i - j * ncol);
    cen[i] = panel[(size_t)init_rows[j] * ncol + c];
  }
}

// Block (x, y): rows [64 x, 64 x + 64) against the centre tiles [y tps, (y + 1) tps).
// pval / plab [y][m]: the lexicographic minimum of (acc, label) over those centres.
__global__ void __launch_bounds__(256) k_km_assign(const double *__restrict__ panel, int64_t m, int ncol,
                                                   const double *__restrict__ cen, int g, int tps,
                                                   double *__restrict__ pval, int *__restrict__ plab) {
  __shared__ __attribute__((aligned(16))) double As[kKK][kKPadA];  // [c][row]: transposed on the way in
  __shared__ double Bs[kKK][kKPadB];                               // [c][centre]
  const int64_t i0 = (int64_t)blockIdx.x * kKT;
  const int ctiles = (g + kKT - 1) / kKT;
  const int t0 = blockIdx.y * tps, t1 = min(t0 + tps, ctiles);
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  double best[4];
  int bl[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) best[r] = std::numeric_limits<double>::infinity(), bl[r] = 0x7fffffff;
  for (int t = t0; t < t1; ++t) {
    const int j0 = t * kKT;
    double acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[r][e] = 0.0;
    for (int k0 = 0; k0 < ncol; k0 += kKK) {
#pragma unroll
      for (int e = 0; e < kKK * kKT / 256; ++e) {
        const int idx = tid + 256 * e;
        const int ra = idx >> 4, ka = idx & 15;  // 16 consecutive columns of one row
        const bool in_k = k0 + ka < ncol;
        As[ka][ra] = (in_k && i0 + ra < m) ? panel[(size_t)(i0 + ra) * ncol + k0 + ka] : 0.0;
        Bs[ka][ra] = (in_k && j0 + ra < g) ? cen[(size_t)(j0 + ra) * ncol + k0 + ka] : 0.0;
      }
      __syncthreads();
      // columns past ncol are staged as zeros on both sides: acc + 0 * 0 leaves acc's bits
#pragma unroll
      for (int kk = 0; kk < kKK; ++kk) {
        double a[4], b[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) a[r] = As[kk][ty * 4 + r];
#pragma unroll
        for (int e = 0; e < 4; ++e) b[e] = Bs[kk][tx + 16 * e];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const double d = a[r] - b[e];
            acc[r][e] = acc[r][e] + d * d;
          }
      }
      __syncthreads();
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int j = j0 + tx + 16 * e;
      if (j >= g) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (acc[r][e] < best[r] || (acc[r][e] == best[r] && j + 1 < bl[r])) best[r] = acc[r][e], bl[r] = j + 1;
    }
  }
  // the 16 threads that share a row are 16 consecutive lanes
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int d = 1; d < 16; d <<= 1) {
      const double ov = __shfl_xor(best[r], d);
      const int ol = __shfl_xor(bl[r], d);
      if (ov < best[r] || (ov == best[r] && ol < bl[r])) best[r] = ov, bl[r] = ol;
    }
  if (tx != 0) return;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t i = i0 + ty * 4 + r;
    if (i >= m) continue;
    pval[(size_t)blockIdx.y * m + i] = best[r];
    plab[(size_t)blockIdx.y * m + i] = bl[r];
  }
}

__global__ void __launch_bounds__(256) k_km_merge(const double *__restrict__ pval, const int *__restrict__ plab,
                                                  int64_t m, int nsplit, int *__restrict__ label,
                                                  KmState *__restrict__ state) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool changed = false;
  if (s < m) {
    double best = pval[s];
    int bl = plab[s];
    for (int y = 1; y < nsplit; ++y) {
      const double ov = pval[(size_t)y * m + s];
      const int ol = plab[(size_t)y * m + s];
      if (ov < best || (ov == best && ol < bl)) best = ov, bl = ol;
    }
    changed = label[s] != bl;
    label[s] = bl;
  }
  const unsigned long long b = __ballot(changed);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(&state->changed, (int)__popcll(b));
}

// dval[s] = acc(s, label[s]) (label null: centre 0, the single group of totss).
__global__ void __launch_bounds__(256) k_km_rowdist(const double *__restrict__ panel, int64_t m, int ncol,
                                                    const double *__restrict__ cen, const int *__restrict__ label,
                                                    double *__restrict__ dval) {
  __shared__ double As[kKK][kKPadB];
  __shared__ double Bs[kKK][kKPadB];
  __shared__ int lab[kKT];
  const int64_t i0 = (int64_t)blockIdx.x * kKT;
  const int tid = threadIdx.x;
  if (tid < kKT) lab[tid] = (label && i0 + tid < m) ? label[i0 + tid] - 1 : 0;
  __syncthreads();
  double acc = 0.0;
  for (int k0 = 0; k0 < ncol; k0 += kKK) {
#pragma unroll
    for (int e = 0; e < kKK * kKT / 256; ++e) {
      const int idx = tid + 256 * e;
      const int ra = idx >> 4, ka = idx & 15;
      const bool in = k0 + ka < ncol && i0 + ra < m;
      As[ka][ra] = in ? panel[(size_t)(i0 + ra) * ncol + k0 + ka] : 0.0;
      Bs[ka][ra] = in ? cen[(size_t)lab[ra] * ncol + k0 + ka] : 0.0;
    }
    __syncthreads();
    if (tid < kKT) {
#pragma unroll
      for (int kk = 0; kk < kKK; ++kk) {
        const double d = As[kk][tid] - Bs[kk][tid];
        acc = acc + d * d;
      }
    }
    __syncthreads();
  }
  if (tid < kKT && i0 + tid < m) dval[i0 + tid] = acc;
}

// gstart[j], j = 0 .. g: the first sorted position whose label exceeds j (labels are 1 .. g).
__global__ void __launch_bounds__(256) k_km_bounds(const int *__restrict__ skeys, int m, int g,
                                                   int *__restrict__ gstart) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j > g) return;
  int lo = 0, hi = m;  // the first t with skeys[t] >= j + 1
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (skeys[mid] >= j + 1)
      hi = mid;
    else
      lo = mid + 1;
  }
  gstart[j] = lo;
}

__device__ __forceinline__ int km_chunks_of(int members) { return (members + KS_KM_CHUNK - 1) / KS_KM_CHUNK; }

// One block: cbase[j] = the chunks of the groups before j, cbase[g] = all chunks.
__global__ void __launch_bounds__(1024) k_km_cscan(const int *__restrict__ gstart, int g, int *__restrict__ cbase) {
  __shared__ int tot[1024];
  const int tid = threadIdx.x, per = (g + 1023) / 1024;
  const int a = min(tid * per, g), b = min(a + per, g);
  int s = 0;
  for (int j = a; j < b; ++j) s += km_chunks_of(gstart[j + 1] - gstart[j]);
  tot[tid] = s;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {
    const int v = tid >= d ? tot[tid - d] : 0;
    __syncthreads();
    tot[tid] += v;
    __syncthreads();
  }
  int run = tot[tid] - s;
  for (int j = a; j < b; ++j) {
    cbase[j] = run;
    run += km_chunks_of(gstart[j + 1] - gstart[j]);
  }
  if (tid == 1023) cbase[g] = tot[1023];
}

// The single group of all m rows (totss): gstart = {0, m}, cbase = {0, chunks}.
__global__ void k_km_one_group(int m, int *__restrict__ gstart, int *__restrict__ cbase) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  gstart[0] = 0, gstart[1] = m;
  cbase[0] = 0, cbase[1] = km_chunks_of(m);
}

// part[q][c] = the partial of chunk q over v[member][c], members ascending.  W (a
// power of two, 16 .. 256) columns and 256 / W chunks per block.
__global__ void __launch_bounds__(256) k_km_partial(const double *__restrict__ v, int64_t ld, int ncolv,
                                                    const int *__restrict__ perm, const int *__restrict__ gstart,
                                                    const int *__restrict__ cbase, int g, int W,
                                                    double *__restrict__ part) {
  const int cpb = 256 / W;
  const int q = blockIdx.x * cpb + (int)threadIdx.x / W;
  const int c = blockIdx.y * W + ((int)threadIdx.x & (W - 1));
  if (q >= cbase[g] || c >= ncolv) return;
  int lo = 0, hi = g;  // cbase[lo] <= q < cbase[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (cbase[mid] <= q)
      lo = mid;
    else
      hi = mid;
  }
  const int t0 = gstart[lo] + (q - cbase[lo]) * KS_KM_CHUNK, t1 = min(t0 + KS_KM_CHUNK, gstart[lo + 1]);
  double P = 0.0;
#pragma unroll 8
  for (int t = t0; t < t1; ++t) P = P + v[(size_t)perm[t] * ld + c];
  part[(size_t)q * ncolv + c] = P;
}

// out[j][c]: the partials of group j added in chunk order; a mean divides by the
// size; an empty group keeps out's bits (kFoldMeanKeep), is NaN or is +0.0 (a sum).
__global__ void __launch_bounds__(256) k_km_fold(const double *__restrict__ part, int ncolv,
                                                 const int *__restrict__ gstart, const int *__restrict__ cbase, int g,
                                                 int mode, double *__restrict__ out) {
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int j = (int)(id / ncolv), c = (int)(id - (int64_t)j * ncolv);
  if (j >= g) return;
  const int q0 = cbase[j], q1 = cbase[j + 1];
  if (q0 == q1) {
    if (mode == kFoldMeanNan) out[id] = std::numeric_limits<double>::quiet_NaN();
    if (mode == kFoldSum) out[id] = 0.0;
    return;
  }
  double S = 0.0;
  int q = q0;
  for (; q + kFoldBatch <= q1; q += kFoldBatch) {  // the loads of a batch are in flight together
    double x[kFoldBatch];
#pragma unroll
    for (int e = 0; e < kFoldBatch; ++e) x[e] = part[(size_t)(q + e) * ncolv + c];
#pragma unroll
    for (int e = 0; e < kFoldBatch; ++e) S = S + x[e];
  }
  for (; q < q1; ++q) S = S + part[(size_t)q * ncolv + c];
  out[id] = mode == kFoldSum ? S : S / (double)(gstart[j + 1] - gstart[j]);
}

// The work memory of a call, one allocation: the panel, then everything else.
struct KmWork {
  double *panel, *part, *dval, *wpart, *wss, *tcen, *tot, *pval;
  int *plab, *skeys, *perm, *iota, *lab, *gstart, *cbase, *one;
  KmState *state;
  void *sort_tmp;
  size_t panel_bytes = 0, bytes = 0, sort_bytes = 0;
  int64_t max_chunks = 0;
  int nsplit = 1, tps = 1;

  // base null: only the sizes
  void lay(char *base, int64_t m, int ncol, int g) {
    Arena a{base};
    panel = a.take<double>((size_t)m * ncol);
    panel_bytes = a.off;
    part = a.take<double>((size_t)max_chunks * ncol);
    dval = a.take<double>((size_t)m);
    wpart = a.take<double>((size_t)max_chunks);
    wss = a.take<double>((size_t)g);
    tcen = a.take<double>((size_t)ncol);
    tot = a.take<double>(1);
    pval = a.take<double>((size_t)nsplit * m);
    plab = a.take<int>((size_t)nsplit * m);
    skeys = a.take<int>((size_t)m);
    perm = a.take<int>((size_t)m);
    iota = a.take<int>((size_t)m);
    lab = a.take<int>((size_t)m);
    gstart = a.take<int>((size_t)(g + 1));
    cbase = a.take<int>((size_t)(g + 1));
    one = a.take<int>(4);
    state = a.take<KmState>(1);
    sort_tmp = a.take<char>(sort_bytes);
    bytes = a.off;
  }
};

int bits_for(int g) {  // the key bits that hold the labels 1 .. g
  int b = 1;
  while ((g >> b) != 0) ++b;
  return b;
}

ks_status km_alloc(ks_ctx *ctx, int64_t m, int ncol, int g, bool assign, KmWork *w, DevFree *mem) {
  w->max_chunks = m / KS_KM_CHUNK + std::max<int64_t>(g, 1);  // >= the chunks of any labelling, and of the one group
  if (assign) {
    // one workgroup per 64 rows leaves CUs idle when the rows are few, and long walks leave a long tail
    // behind the last round of workgroups: split the centre tiles until there are some 32 workgroups per CU
    const int64_t rtiles = (m + kKT - 1) / kKT;
    const int ctiles = (g + kKT - 1) / kKT;
    const int64_t want = ((int64_t)ctx->num_cus * 32 + rtiles - 1) / rtiles;
    const int ns = (int)std::max<int64_t>(1, std::min<int64_t>(ctiles, want));
    w->tps = (ctiles + ns - 1) / ns;
    w->nsplit = (ctiles + w->tps - 1) / w->tps;
  } else {
    w->nsplit = 0;
  }
  KS_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, w->sort_bytes, (const uint32_t *)nullptr, (uint32_t *)nullptr,
                                            (const int *)nullptr, (int *)nullptr, (int)m, 0, bits_for(g),
                                            ctx->stream));
  w->lay(nullptr, m, ncol, g);
  KS_TRY(dev_alloc(mem, w->bytes, "the profile panel"));
  w->lay(static_cast<char *>(mem->p), m, ncol, g);
  return KS_OK;
}

// Profiles and checks; the 32-byte read-back.  init / init_rows: device pointers or null.
ks_status km_normalise(ks_ctx *ctx, const KmWork &w, const uint32_t *sp, int64_t n, int ncol, const int64_t *rows,
                       int64_t m, const double *init, const int64_t *init_rows, int g) {
  hipStream_t st = ctx->stream;
  KS_HIP(hipMemsetAsync(w.state, 0, sizeof(KmState), st));
  KS_TRY(panel_normalise(ctx, sp, n, ncol, rows, m, PanelRoot::kNone, w.panel, w.iota, &w.state->bad[0],
                         &w.state->bad[1]));
  if (init) {
    const int64_t total = (int64_t)g * ncol;
    const unsigned grid = (unsigned)std::min<int64_t>((total + 255) / 256, (int64_t)ctx->num_cus * 8);
    hipLaunchKernelGGL(k_km_check_init, dim3(grid), dim3(256), 0, st, init, total, w.state);
    KS_HIP(hipGetLastError());
  }
  if (init_rows) {
    hipLaunchKernelGGL(k_km_check_init_rows, dim3((unsigned)((g + 255) / 256)), dim3(256), 0, st, init_rows, g, m,
                       w.state);
    KS_HIP(hipGetLastError());
  }
  unsigned long long hbad[4] = {0, 0, 0, 0};
  KS_HIP(hipMemcpyAsync(hbad, w.state->bad, sizeof(hbad), hipMemcpyDeviceToHost, st));
  KS_HIP(hipStreamSynchronize(st));
  KS_TRY(panel_report(hbad, 1, m, 0));
  if (hbad[2]) {
    const int64_t at = (int64_t)g * ncol - (int64_t)hbad[2];
    return fail(KS_ERR_ARG, "center[%lld][%lld] is not finite", (long long)(at / ncol), (long long)(at % ncol));
  }
  if (hbad[3]) return fail(KS_ERR_ARG, "initial row index %lld out of range", (long long)(g - (int64_t)hbad[3]));
  return KS_OK;
}

// The member list of a labelling: perm (positions by (label, position)), gstart, cbase.
ks_status km_members(ks_ctx *ctx, KmWork &w, const int *label, int64_t m, int g) {
  hipStream_t st = ctx->stream;
  KS_HIP(hipcub::DeviceRadixSort::SortPairs(w.sort_tmp, w.sort_bytes, reinterpret_cast<const uint32_t *>(label),
                                            reinterpret_cast<uint32_t *>(w.skeys), (const int *)w.iota, w.perm, (int)m,
                                            0, bits_for(g), st));
  hipLaunchKernelGGL(k_km_bounds, dim3((unsigned)((g + 1 + 255) / 256)), dim3(256), 0, st, w.skeys, (int)m, g,
                     w.gstart);
  hipLaunchKernelGGL(k_km_cscan, dim3(1), dim3(1024), 0, st, w.gstart, g, w.cbase);
  KS_HIP(hipGetLastError());
  return KS_OK;
}

// out[j][c] over the groups of (perm, gstart, cbase): the chunked sums of v[s][c], folded by `mode`.
ks_status km_group_sums(ks_ctx *ctx, const double *v, int64_t ld, int ncolv, const int *perm, const int *gstart,
                        const int *cbase, int g, int64_t max_chunks, double *part, int mode, double *out) {
  hipStream_t st = ctx->stream;
  int W = 16;
  while (W < ncolv && W < 256) W <<= 1;
  const int cpb = 256 / W;
  hipLaunchKernelGGL(k_km_partial, dim3((unsigned)((max_chunks + cpb - 1) / cpb), (unsigned)((ncolv + W - 1) / W)),
                     dim3(256), 0, st, v, ld, ncolv, perm, gstart, cbase, g, W, part);
  hipLaunchKernelGGL(k_km_fold, dim3((unsigned)(((int64_t)g * ncolv + 255) / 256)), dim3(256), 0, st, part, ncolv,
                     gstart, cbase, g, mode, out);
  KS_HIP(hipGetLastError());
  return KS_OK;
}

// withinss of the labelling whose member list w holds, against cen: w.wss [g].
ks_status km_wss(ks_ctx *ctx, KmWork &w, int64_t m, int ncol, const double *cen, const int *label, int g) {
  hipLaunchKernelGGL(k_km_rowdist, dim3((unsigned)((m + kKT - 1) / kKT)), dim3(256), 0, ctx->stream, w.panel, m, ncol,
                     cen, label, w.dval);
  KS_HIP(hipGetLastError());
  return km_group_sums(ctx, w.dval, 1, 1, w.perm, w.gstart, w.cbase, g, w.max_chunks, w.wpart, kFoldSum, w.wss);
}

// size and withinss to the host (synchronises).
ks_status km_download(ks_ctx *ctx, const KmWork &w, int g, int32_t *size, double *withinss) {
  std::vector<int> gs((size_t)g + 1);
  KS_HIP(hipMemcpyAsync(gs.data(), w.gstart, (size_t)(g + 1) * 4, hipMemcpyDeviceToHost, ctx->stream));
  KS_HIP(hipMemcpyAsync(withinss, w.wss, (size_t)g * 8, hipMemcpyDeviceToHost, ctx->stream));
  KS_HIP(hipStreamSynchronize(ctx->stream));
  for (int j = 0; j < g; ++j) size[j] = gs[j + 1] - gs[j];
  return KS_OK;
}

ks_status check_kmeans_args(const void *spectra, int64_t n, int32_t ncol, const void *rows, int64_t m, const void *init,
                            const void *init_rows, int32_t g, int32_t iter_max, int32_t flags, const void *cluster,
                            const void *centers, const void *size, const void *withinss, const void *res) {
  KS_TRY(panel_check_common(n, ncol, rows, m, flags, "a k-means call"));
  if (g < 1 || g > KS_KM_MAX_GROUPS)
    return fail(KS_ERR_ARG, "the number of groups must be between 1 and %d (g = %d)", KS_KM_MAX_GROUPS, (int)g);
  if (iter_max < 1) return fail(KS_ERR_ARG, "iter_max = %d is not positive", (int)iter_max);
  if (!spectra) return fail(KS_ERR_ARG, "null spectra");
  if ((init != nullptr) == (init_rows != nullptr))
    return fail(KS_ERR_ARG, "give exactly one of the initial centres and the initial rows (%s)",
                init ? "both are set" : "both are NULL");
  if (!cluster || !centers || !size || !withinss || !res) return fail(KS_ERR_ARG, "null output");
  return KS_OK;
}

// size: [ngroups], filled.
ks_status check_means_args(const void *spectra, int64_t n, int32_t ncol, const void *rows, int64_t m,
                           const int32_t *group, int32_t ngroups, int32_t flags, const void *centers, int32_t *size,
                           const void *withinss) {
  KS_TRY(panel_check_common(n, ncol, rows, m, flags, "a group-means call"));
  if (ngroups < 1 || ngroups > KS_KM_MAX_GROUPS)
    return fail(KS_ERR_ARG, "ngroups = %d is not in 1 .. %d", (int)ngroups, KS_KM_MAX_GROUPS);
  if (!spectra) return fail(KS_ERR_ARG, "null spectra");
  if (!group) return fail(KS_ERR_ARG, "null group");
  if (!centers || !size || !withinss) return fail(KS_ERR_ARG, "null output");
  for (int64_t i = 0; i < m; ++i) {
    const int32_t v = group[i];
    if (v < 1 || v > ngroups)
      return fail(KS_ERR_ARG, "group[%lld] = %d is not in 1 .. %d", (long long)i, (int)v, (int)ngroups);
  }
  return KS_OK;
}

// Everything but the device-side checks validated; all pointers but size, withinss, res are device pointers.
ks_status kmeans_impl(ks_ctx *ctx, const uint32_t *sp, int64_t n, int ncol, const int64_t *rows, int64_t m,
                      const double *init, const int64_t *init_rows, int g, int iter_max, int *cluster, double *cen,
                      int32_t *size, double *withinss, ks_kmeans_result *res, ks_kmeans_stats *stats) {
  hipStream_t st = ctx->stream;
  KmWork w;
  DevFree mem;
  KS_TRY(km_alloc(ctx, m, ncol, g, true, &w, &mem));
  KS_HIP(hipEventRecord(ctx->ev[0], st));
  KS_TRY(km_normalise(ctx, w, sp, n, ncol, rows, m, init, init_rows, g));
  // from here on the outputs are written
  if (init_rows) {
    const int64_t total = (int64_t)g * ncol;
    const unsigned grid = (unsigned)std::min<int64_t>((total + 255) / 256, (int64_t)ctx->num_cus * 8);
    hipLaunchKernelGGL(k_km_gather_init, dim3(grid), dim3(256), 0, st, w.panel, ncol, init_rows, total, cen);
    KS_HIP(hipGetLastError());
  } else if (init != cen) {
    KS_HIP(hipMemcpyAsync(cen, init, (size_t)g * ncol * 8, hipMemcpyDeviceToDevice, st));
  }
  KS_HIP(hipMemsetAsync(cluster, 0, (size_t)m * 4, st));
  KS_HIP(hipEventRecord(ctx->ev[1], st));

  double ms_assign = 0, ms_update = 0;
  bool update_pending = false;
  int iter = 0, converged = 0;
  const dim3 agrid((unsigned)((m + kKT - 1) / kKT), (unsigned)w.nsplit);
  for (int it = 1; it <= iter_max; ++it) {
    KS_HIP(hipMemsetAsync(&w.state->changed, 0, 4, st));
    KS_HIP(hipEventRecord(ctx->ev[2], st));
    hipLaunchKernelGGL(k_km_assign, agrid, dim3(256), 0, st, w.panel, m, ncol, cen, g, w.tps, w.pval, w.plab);
    hipLaunchKernelGGL(k_km_merge, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, w.pval, w.plab, m, w.nsplit,
                       cluster, w.state);
    KS_HIP(hipGetLastError());
    KS_HIP(hipEventRecord(ctx->ev[3], st));
    int changed = 0;
    KS_HIP(hipMemcpyAsync(&changed, &w.state->changed, 4, hipMemcpyDeviceToHost, st));
    KS_HIP(hipStreamSynchronize(st));  // the pass's one round trip
    double ms = 0;
    if (update_pending) {
      KS_TRY(event_ms(ctx, 4, 5, &ms));
      ms_update += ms;
      update_pending = false;
    }
    KS_TRY(event_ms(ctx, 2, 3, &ms));
    ms_assign += ms;
    iter = it;
    if (changed == 0) {
      converged = 1;  // the member list of the previous pass is that of these labels
      break;
    }
    KS_HIP(hipEventRecord(ctx->ev[4], st));
    KS_TRY(km_members(ctx, w, cluster, m, g));
    KS_TRY(km_group_sums(ctx, w.panel, ncol, ncol, w.perm, w.gstart, w.cbase, g, w.max_chunks, w.part, kFoldMeanKeep,
                         cen));
    KS_HIP(hipEventRecord(ctx->ev[5], st));
    update_pending = true;
  }

  KS_HIP(hipEventRecord(ctx->ev[6], st));
  KS_TRY(km_wss(ctx, w, m, ncol, cen, cluster, g));
  KS_TRY(km_download(ctx, w, g, size, withinss));  // before the member list is overwritten
  // totss: the single group of all rows, its chunked centre, then its chunked sum
  hipLaunchKernelGGL(k_km_one_group, dim3(1), dim3(64), 0, st, (int)m, w.one, w.one + 2);
  KS_HIP(hipGetLastError());
  KS_TRY(km_group_sums(ctx, w.panel, ncol, ncol, w.iota, w.one, w.one + 2, 1, w.max_chunks, w.part, kFoldMeanKeep,
                       w.tcen));
  hipLaunchKernelGGL(k_km_rowdist, dim3((unsigned)((m + kKT - 1) / kKT)), dim3(256), 0, st, w.panel, m, ncol, w.tcen,
                     (const int *)nullptr, w.dval);
  KS_HIP(hipGetLastError());
  KS_TRY(km_group_sums(ctx, w.dval, 1, 1, w.iota, w.one, w.one + 2, 1, w.max_chunks, w.wpart, kFoldSum, w.tot));
  KS_HIP(hipEventRecord(ctx->ev[7], st));
  double totss = 0;
  KS_HIP(hipMemcpyAsync(&totss, w.tot, 8, hipMemcpyDeviceToHost, st));
  KS_HIP(hipStreamSynchronize(st));  // the work memory is freed on return
  double tw = 0.0;
  for (int j = 0; j < g; ++j) tw = tw + withinss[j];
  res->iter = iter;
  res->converged = converged;
  res->tot_withinss = tw;
  res->totss = totss;
  if (stats) {
    if (update_pending) {
      double ms = 0;
      KS_TRY(event_ms(ctx, 4, 5, &ms));
      ms_update += ms;
    }
    KS_TRY(event_ms(ctx, 0, 7, &stats->ms_total));
    KS_TRY(event_ms(ctx, 0, 1, &stats->ms_normalise));
    KS_TRY(event_ms(ctx, 6, 7, &stats->ms_wss));
    stats->ms_assign = ms_assign;
    stats->ms_update = ms_update;
    stats->n_iter = iter;
    stats->panel_bytes = (int64_t)w.panel_bytes;
    stats->work_bytes = (int64_t)(w.bytes - w.panel_bytes);
  }
  return KS_OK;
}

// group: a HOST pointer, validated; cen a device pointer.
ks_status means_impl(ks_ctx *ctx, const uint32_t *sp, int64_t n, int ncol, const int64_t *rows, int64_t m,
                     const int32_t *group, int g, double *cen, int32_t *size, double *withinss,
                     ks_kmeans_stats *stats) {
  hipStream_t st = ctx->stream;
  KmWork w;
  DevFree mem;
  KS_TRY(km_alloc(ctx, m, ncol, g, false, &w, &mem));
  KS_HIP(hipEventRecord(ctx->ev[0], st));
  KS_TRY(km_normalise(ctx, w, sp, n, ncol, rows, m, nullptr, nullptr, g));
  KS_HIP(hipMemcpyAsync(w.lab, group, (size_t)m * 4, hipMemcpyHostToDevice, st));
  KS_HIP(hipEventRecord(ctx->ev[1], st));
  KS_TRY(km_members(ctx, w, w.lab, m, g));
  KS_TRY(km_group_sums(ctx, w.panel, ncol, ncol, w.perm, w.gstart, w.cbase, g, w.max_chunks, w.part, kFoldMeanNan,
                       cen));
  KS_HIP(hipEventRecord(ctx->ev[2], st));
  KS_TRY(km_wss(ctx, w, m, ncol, cen, w.lab, g));
  KS_HIP(hipEventRecord(ctx->ev[3], st));
  KS_TRY(km_download(ctx, w, g, size, withinss));
  if (stats) {
    KS_TRY(event_ms(ctx, 0, 3, &stats->ms_total));
    KS_TRY(event_ms(ctx, 0, 1, &stats->ms_normalise));
    KS_TRY(event_ms(ctx, 1, 2, &stats->ms_update));
    KS_TRY(event_ms(ctx, 2, 3, &stats->ms_wss));
    stats->panel_bytes = (int64_t)w.panel_bytes;
    stats->work_bytes = (int64_t)(w.bytes - w.panel_bytes);
  }
  return KS_OK;
}

}  // namespace
}  // namespace ks

using namespace ks;

extern "C" ks_status ks_spectra_kmeans_dev(ks_ctx *ctx, const uint32_t *spectra_dev, int64_t n, int32_t ncol,
                                           const int64_t *rows_dev, int64_t m, const double *init_dev,
                                           const int64_t *init_rows_dev, int32_t g, int32_t iter_max, int32_t flags,
                                           int32_t *cluster_dev, double *centers_dev, int32_t *size, double *withinss,
                                           ks_kmeans_result *res, ks_kmeans_stats *stats) {
  if (stats) memset(stats, 0, sizeof(*stats));
  KS_TRY(check_kmeans_args(spectra_dev, n, ncol, rows_dev, m, init_dev, init_rows_dev, g, iter_max, flags, cluster_dev,
                           centers_dev, size, withinss, res));
  KS_TRY(default_ctx(&ctx));
  KS_ENTER(ctx);
  return kmeans_impl(ctx, spectra_dev, n, ncol, rows_dev, m, init_dev, init_rows_dev, g, iter_max, cluster_dev,
                     centers_dev, size, withinss, res, stats);
}

extern "C" ks_status ks_spectra_kmeans(ks_ctx *ctx, const uint32_t *spectra, int64_t n, int32_t ncol,
                                       const int64_t *rows, int64_t m, const double *init, const int64_t *init_rows,
                                       int32_t g, int32_t iter_max, int32_t flags, int32_t *cluster, double *centers,
                                       int32_t *size, double *withinss, ks_kmeans_result *res) {
  KS_TRY(check_kmeans_args(spectra, n, ncol, rows, m, init, init_rows, g, iter_max, flags, cluster, centers, size,
                           withinss, res));
  KS_TRY(panel_check_rows_host(spectra, n, ncol, rows, m, nullptr, 0));
  if (init) {
    for (int64_t i = 0; i < (int64_t)g * ncol; ++i)
      if (!std::isfinite(init[i]))
        return fail(KS_ERR_ARG, "center[%lld][%lld] is not finite", (long long)(i / ncol), (long long)(i % ncol));
  } else {
    for (int32_t j = 0; j < g; ++j)
      if (init_rows[j] < 0 || init_rows[j] >= m)
        return fail(KS_ERR_ARG, "initial row index %lld out of range", (long long)j);
  }
  KS_TRY(default_ctx(&ctx));
  KS_ENTER(ctx);
  const HostEnd host_end{ctx};  // (ks_set_host_cache)
  void *d_out = nullptr;
  const size_t cen_bytes = (size_t)g * ncol * 8;
  KS_TRY(ensure(ctx, SLOT_REG_TMP, cen_bytes + (size_t)m * 4, &d_out));
  SpectraUpload up;
  KS_TRY(upload_spectra(ctx, spectra, n, ncol, rows, m, nullptr, 0, g, &up));
  hipStream_t st = ctx->stream;
  int64_t *d_ir = nullptr;
  double *d_cen = static_cast<double *>(d_out);
  int *d_cl = reinterpret_cast<int *>(static_cast<char *>(d_out) + cen_bytes);
  if (init) {  // the initial centres go up into the output buffer: the device entry allows the alias
    KS_HIP(hipMemcpyAsync(d_cen, init, cen_bytes, hipMemcpyHostToDevice, st));
  } else {
    d_ir = up.extra;
    KS_HIP(hipMemcpyAsync(d_ir, init_rows, (size_t)g * 8, hipMemcpyHostToDevice, st));
  }
  KS_TRY(kmeans_impl(ctx, up.sp, n, ncol, up.rows, m, init ? d_cen : nullptr, d_ir, g, iter_max, d_cl, d_cen, size,
                     withinss, res, nullptr));
  KS_HIP(hipMemcpyAsync(centers, d_cen, cen_bytes, hipMemcpyDeviceToHost, st));
  KS_HIP(hipMemcpyAsync(cluster, d_cl, (size_t)m * 4, hipMemcpyDeviceToHost, st));
  KS_HIP(hipStreamSynchronize(st));
  return KS_OK;
}

extern "C" ks_status ks_spectra_group_means_dev(ks_ctx *ctx, const uint32_t *spectra_dev, int64_t n, int32_t ncol,
                                                const int64_t *rows_dev, int64_t m, const int32_t *group,
                                                int32_t ngroups, int32_t flags, double *centers_dev, int32_t *size,
                                                double *withinss, ks_kmeans_stats *stats) {
  if (stats) memset(stats, 0, sizeof(*stats));
  KS_TRY(check_means_args(spectra_dev, n, ncol, rows_dev, m, group, ngroups, flags, centers_dev, size, withinss));
  KS_TRY(default_ctx(&ctx));
  KS_ENTER(ctx);
  return means_impl(ctx, spectra_dev, n, ncol, rows_dev, m, group, ngroups, centers_dev, size, withinss, stats);
}

extern "C" ks_status ks_spectra_group_means(ks_ctx *ctx, const uint32_t *spectra, int64_t n, int32_t ncol,
                                            const int64_t *rows, int64_t m, const int32_t *group, int32_t ngroups,
                                            int32_t flags, double *centers, int32_t *size, double *withinss) {
  KS_TRY(check_means_args(spectra, n, ncol, rows, m, group, ngroups, flags, centers, size, withinss));
  KS_TRY(panel_check_rows_host(spectra, n, ncol, rows, m, nullptr, 0));
  KS_TRY(default_ctx(&ctx));
  KS_ENTER(ctx);
  const HostEnd host_end{ctx};  // (ks_set_host_cache)
  void *d_out = nullptr;
  const size_t cen_bytes = (size_t)ngroups * ncol * 8;
  KS_TRY(ensure(ctx, SLOT_REG_TMP, cen_bytes, &d_out));
  SpectraUpload up;
  KS_TRY(upload_spectra(ctx, spectra, n, ncol, rows, m, nullptr, 0, 0, &up));
  hipStream_t st = ctx->stream;
  KS_TRY(means_impl(ctx, up.sp, n, ncol, up.rows, m, group, ngroups, static_cast<double *>(d_out), size, withinss,
                    nullptr));
  KS_HIP(hipMemcpyAsync(centers, d_out, cen_bytes, hipMemcpyDeviceToHost, st));
  KS_HIP(hipStreamSynchronize(st));
  return KS_OK;
}
