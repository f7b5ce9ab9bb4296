// ks_silhouette.hip -- silhouette widths, medoids and diameters of a grouping
// of the observations of a condensed dissimilarity vector on the device
// (ks_silhouette_dev / ks_silhouette); the contract is in include/kmer_spans.h.
//
// What the reference author's script asks of the groups cutree() gives
// (test.R:788-859: which height, which representative, how tight) without
// taking the matrix to the host: R's cluster::silhouette(cutree(hc, k), d).
// The matrix stays in HBM as ks_spectra_dist_dev wrote it and is only read.
//
// The sums are fixed in the header as an order of FP64 additions (no FMA:
// -ffp-contract=off, csrc/Makefile): the members of a group in ascending index
// order, cut into chunks of KS_SIL_CHUNK; a partial per chunk, the partials
// added in chunk order.
//
// Check:  the finiteness pass of hclust (ks_finite_check.h).
// Host:   a stable counting sort of the observations by (group, index) gives
//         the member list; the chunk table cuts it at group ends and every
//         KS_SIL_CHUNK members.  Both go up with the labels and the group
//         sizes: 4 (2 n + 2 chunks + g) bytes.
// Sums:   k_sil_sums: a workgroup owns a strip of 64 consecutive rows, lane =
//         row, and walks every chunk: batches of kSilBatch chunks, the waves
//         taking the chunks of a batch in turn.  A wave walks its chunk's
//         members with the column j wave-uniform: for j below the strip the
//         lanes read D(j, i), 512 consecutive bytes; for j above it they read
//         D(i, j), one entry of each of 64 rows (DESIGN.md 6l has what that
//         half costs).  The partials of a batch go to LDS; wave 0 folds them in
//         ascending chunk order and keeps, per row, the running group sum, the
//         sum of the row's own group, and the smallest mean of another group
//         with its label.  far (the largest entry to a member of the own
//         group, exact in any order) is kept per wave and merged at the end.
//         Nothing of size n x g exists unless the caller asks for the sums.
// Widths: k_sil_widths: a, width per row.
// The O(n) folds per group (size, medoid, diameter, mean width) are host code
// on the downloaded per-row values.
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "ks_internal.h"
// after hip_runtime.h (ks_internal.h): the header's functions are __host__ __device__ here
#include "ks_dist_index.h"
#include "ks_finite_check.h"

namespace ks {
namespace {

constexpr int kSilRows = 64;      // rows of a strip: lane = row
constexpr int kSilWaves = 16;     // k_sil_sums: waves of a workgroup
constexpr int kSilThreads = kSilWaves * 64;
constexpr int kSilBatch = 64;     // chunks whose partials LDS holds at a time (32 KiB)
static_assert(kSilBatch % kSilWaves == 0, "every wave takes the same number of chunks of a full batch");

// The O(n) state of a call, one allocation (SilState::bytes).
struct SilState {
  double *sown, *bmin, *far, *a, *width;
  int32_t *perm, *grp, *neighbor, *cstart, *cgroup, *gsize;
  static size_t bytes(int64_t n, int64_t nchunks, int64_t g) {
    return (size_t)n * (5 * 8 + 3 * 4) + (size_t)(2 * nchunks + 1 + g + 1) * 4 + 64;
  }
  SilState(void *base, int64_t n, int64_t nchunks, int64_t g) {
    char *p = static_cast<char *>(base);
    sown = reinterpret_cast<double *>(p), p += n * 8;
    bmin = reinterpret_cast<double *>(p), p += n * 8;
    far = reinterpret_cast<double *>(p), p += n * 8;
    a = reinterpret_cast<double *>(p), p += n * 8;
    width = reinterpret_cast<double *>(p), p += n * 8;
    perm = reinterpret_cast<int32_t *>(p), p += n * 4;
    grp = reinterpret_cast<int32_t *>(p), p += n * 4;
    neighbor = reinterpret_cast<int32_t *>(p), p += n * 4;
    cstart = reinterpret_cast<int32_t *>(p), p += (nchunks + 1) * 4;
    cgroup = reinterpret_cast<int32_t *>(p), p += nchunks * 4;
    gsize = reinterpret_cast<int32_t *>(p);  // [g + 1], by label
  }
};

// Block s: rows 64 s .. 64 s + 63.  perm[cstart[q] .. cstart[q + 1]) are the
// members of chunk q, ascending; cgroup[q] is its label; the chunks of a group
// are consecutive.  sums: [n][g] or null.
__global__ void __launch_bounds__(kSilThreads) k_sil_sums(const double *__restrict__ d, int n, int g, int nchunks,
                                                          SilState st, double *__restrict__ sums) {
  __shared__ double part[kSilBatch][kSilRows];
  __shared__ double wfar[kSilWaves][kSilRows];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i = blockIdx.x * kSilRows + lane;
  const bool row = i < n;  // the last strip may be short: its idle lanes add zeros and store nothing
  const int o = row ? st.grp[i] : 0;
  const double *rowp = d + (dist_pair_offset(i, i + 1, n) - (i + 1));  // rowp[j] = D(i, j), j > i
  double far = 0.0;
  double S = 0.0, sown = 0.0, b = 0.0;  // wave 0: the fold
  int nb = 0;
  for (int q0 = 0; q0 < nchunks; q0 += kSilBatch) {
    const int qe = min(q0 + kSilBatch, nchunks);
    for (int q = q0 + wave; q < qe; q += kSilWaves) {
      const int t0 = st.cstart[q], t1 = st.cstart[q + 1];
      const bool own = st.cgroup[q] == o;
      double P = 0.0;
#pragma unroll 4
      for (int t = t0; t < t1; ++t) {
        const int j = st.perm[t];  // wave-uniform
        const double *colp = d + (dist_pair_offset(j, j + 1, n) - (j + 1));  // colp[i] = D(j, i), i > j
        const double *p = j < i ? colp + i : rowp + j;
        const double x = row && j != i ? *p : 0.0;  // D(i, i) = +0.0
        P = P + x;
        if (own && x > far) far = x;
      }
      part[q - q0][lane] = P;
    }
    __syncthreads();
    if (wave == 0) {
      for (int q = q0; q < qe; ++q) {
        const int c = st.cgroup[q];
        if (q == 0 || st.cgroup[q - 1] != c) S = 0.0;
        S = S + part[q - q0][lane];
        if (q == nchunks - 1 || st.cgroup[q + 1] != c) {  // S = S(i, c)
          if (sums && row) sums[(int64_t)i * g + (c - 1)] = S;
          if (c == o) {
            sown = S;
          } else {
            const double mean = S / (double)st.gsize[c];
            if (nb == 0 || mean < b) b = mean, nb = c;  // ascending c, strict <: the lowest label wins a tie
          }
        }
      }
    }
    __syncthreads();  // the next batch overwrites part
  }
  wfar[wave][lane] = far;
  __syncthreads();
  if (wave != 0 || !row) return;
  for (int w = 1; w < kSilWaves; ++w)
    if (wfar[w][lane] > far) far = wfar[w][lane];
  st.sown[i] = sown;
  st.bmin[i] = b;
  st.neighbor[i] = nb;
  st.far[i] = far;
}

__global__ void __launch_bounds__(256) k_sil_widths(int n, SilState st) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int no = st.gsize[st.grp[i]];
  const double b = st.bmin[i];
  double a = 0.0, w = 0.0;
  if (no > 1) {
    a = st.sown[i] / (double)(no - 1);
    if (a < b)
      w = (b - a) / b;
    else if (a > b)
      w = (b - a) / a;
  }
  st.a[i] = a;
  st.width[i] = w;
}

// ------------------------------------------------------------------- host

// Everything but the entries of diss, on the host.  size: [ngroups], filled.
ks_status check_sil_args(const void *diss, int64_t n, const int32_t *group, int32_t ngroups, int32_t flags,
                         const void *width, const void *a, const void *b, const void *neighbor, int32_t *size,
                         const void *medoid, const void *diameter, const void *avg_width, const void *avg_width_all) {
  if (n < 2) return fail(KS_ERR_ARG, "silhouette widths need at least 2 observations, n = %lld", (long long)n);
  if (n > 0x7ffffffeLL) return fail(KS_ERR_ARG, "n = %lld does not fit the int32 tables", (long long)n);
  if (flags) return fail(KS_ERR_ARG, "unknown silhouette flags 0x%x", (unsigned)flags);
  if (!diss) return fail(KS_ERR_ARG, "null dissimilarities");
  if (!group) return fail(KS_ERR_ARG, "null group");
  if (!width || !a || !b || !neighbor || !size || !medoid || !diameter || !avg_width || !avg_width_all)
    return fail(KS_ERR_ARG, "null output");
  if (ngroups < 1) return fail(KS_ERR_ARG, "ngroups = %d is not positive", (int)ngroups);
  for (int32_t c = 0; c < ngroups; ++c) size[c] = 0;
  for (int64_t i = 0; i < n; ++i) {
    const int32_t v = group[i];
    if (v < 1 || v > ngroups)
      return fail(KS_ERR_ARG, "group[%lld] = %d is not in 1 .. %d", (long long)i, (int)v, (int)ngroups);
    ++size[v - 1];
  }
  int64_t nonempty = 0;
  for (int32_t c = 0; c < ngroups; ++c) nonempty += size[c] > 0;
  if (nonempty < 2)
    return fail(KS_ERR_ARG, "silhouette widths need at least 2 non-empty groups, the labels name %lld", (long long)nonempty);
  return KS_OK;
}

// Everything validated, size filled; diss and sums are device pointers.
ks_status sil_impl(ks_ctx *ctx, const double *diss, int64_t n, const int32_t *group, int32_t g, double *width,
                   double *a, double *b, int32_t *neighbor, const int32_t *size, int32_t *medoid, double *diameter,
                   double *avg_width, double *avg_width_all, double *sums, ks_silhouette_stats *stats) {
  hipStream_t st = ctx->stream;
  const int64_t total = dist_pair_count(n);
  // members by (group, index): a stable counting sort; chunks of a group's members
  std::vector<int32_t> meta;  // perm | grp, then cstart | cgroup | gsize: the two uploads
  int64_t nchunks = 0;
  bool empty_group = false;
  for (int32_t c = 0; c < g; ++c) {
    nchunks += ((int64_t)size[c] + KS_SIL_CHUNK - 1) / KS_SIL_CHUNK;
    empty_group |= size[c] == 0;
  }
  meta.resize((size_t)(2 * n + 2 * nchunks + 1 + g + 1));
  int32_t *perm = meta.data(), *grp = perm + n, *cstart = grp + n, *cgroup = cstart + nchunks + 1,
          *gsize = cgroup + nchunks;
  {
    std::vector<int64_t> at((size_t)g + 1, 0);
    for (int32_t c = 0; c < g; ++c) at[c + 1] = at[c] + size[c];
    int64_t q = 0;
    for (int32_t c = 0; c < g; ++c)
      for (int64_t t = at[c]; t < at[c + 1]; t += KS_SIL_CHUNK) cstart[q] = (int32_t)t, cgroup[q] = c + 1, ++q;
    cstart[nchunks] = (int32_t)n;
    for (int64_t i = 0; i < n; ++i) perm[at[group[i] - 1]++] = (int32_t)i;
    memcpy(grp, group, (size_t)n * 4);
    gsize[0] = 0;
    memcpy(gsize + 1, size, (size_t)g * 4);
  }

  void *scal = nullptr, *state_mem = nullptr;
  const size_t state_bytes = SilState::bytes(n, nchunks, g);
  KS_TRY(ensure(ctx, SLOT_SCALARS, 4096, &scal));
  KS_TRY(ensure(ctx, SLOT_WORK_A, state_bytes, &state_mem));
  KS_TRY(check_all_finite(ctx, diss, total, static_cast<unsigned long long *>(scal) + kScSilBad));

  SilState ss(state_mem, n, nchunks, g);
  KS_HIP(hipMemcpyAsync(ss.perm, perm, (size_t)2 * n * 4, hipMemcpyHostToDevice, st));  // perm | grp
  KS_HIP(hipMemcpyAsync(ss.cstart, cstart, (size_t)(2 * nchunks + 1 + g + 1) * 4, hipMemcpyHostToDevice, st));
  // an empty group has no chunk: its column of sums is the empty sum
  if (sums && empty_group) KS_HIP(hipMemsetAsync(sums, 0, (size_t)n * g * 8, st));
  KS_HIP(hipEventRecord(ctx->ev[2], st));
  hipLaunchKernelGGL(k_sil_sums, dim3((unsigned)((n + kSilRows - 1) / kSilRows)), dim3(kSilThreads), 0, st, diss,
                     (int)n, (int)g, (int)nchunks, ss, sums);
  KS_HIP(hipGetLastError());
  KS_HIP(hipEventRecord(ctx->ev[3], st));
  hipLaunchKernelGGL(k_sil_widths, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (int)n, ss);
  KS_HIP(hipGetLastError());
  KS_HIP(hipEventRecord(ctx->ev[4], st));

  std::vector<double> sown((size_t)n), far((size_t)n);
  KS_HIP(hipMemcpyAsync(sown.data(), ss.sown, (size_t)n * 8, hipMemcpyDeviceToHost, st));
  KS_HIP(hipMemcpyAsync(far.data(), ss.far, (size_t)n * 8, hipMemcpyDeviceToHost, st));
  KS_HIP(hipMemcpyAsync(b, ss.bmin, (size_t)n * 8, hipMemcpyDeviceToHost, st));
  KS_HIP(hipMemcpyAsync(a, ss.a, (size_t)n * 8, hipMemcpyDeviceToHost, st));
  KS_HIP(hipMemcpyAsync(width, ss.width, (size_t)n * 8, hipMemcpyDeviceToHost, st));
  KS_HIP(hipMemcpyAsync(neighbor, ss.neighbor, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  KS_HIP(hipStreamSynchronize(st));

  // per group, members ascending: perm lists them so
  double all = 0.0;
  for (int64_t i = 0; i < n; ++i) all = all + width[i];
  *avg_width_all = all / (double)n;
  int64_t t = 0;
  for (int32_t c = 0; c < g; ++c) {
    if (size[c] == 0) {
      medoid[c] = -1;
      diameter[c] = avg_width[c] = std::numeric_limits<double>::quiet_NaN();
      continue;
    }
    int32_t med = perm[t];
    double best = sown[med], diam = 0.0, acc = 0.0;
    for (int64_t e = t + size[c]; t < e; ++t) {
      const int32_t i = perm[t];
      if (sown[i] < best) best = sown[i], med = i;
      if (far[i] > diam) diam = far[i];
      acc = acc + width[i];
    }
    medoid[c] = med;
    diameter[c] = diam;
    avg_width[c] = acc / (double)size[c];
  }
  if (stats) {
    KS_TRY(event_ms(ctx, 0, 4, &stats->ms_total));
    KS_TRY(event_ms(ctx, 0, 1, &stats->ms_check));
    KS_TRY(event_ms(ctx, 2, 3, &stats->ms_sums));
    KS_TRY(event_ms(ctx, 3, 4, &stats->ms_widths));
    stats->n = n;
    stats->ngroups = g;
    stats->n_chunks = nchunks;
    stats->work_bytes = (int64_t)state_bytes;
  }
  return KS_OK;
}

}  // namespace
}  // namespace ks

using namespace ks;

extern "C" ks_status ks_silhouette_dev(ks_ctx *ctx, const double *diss_dev, int64_t n, const int32_t *group,
                                       int32_t ngroups, int32_t flags, double *width, double *a, double *b,
                                       int32_t *neighbor, int32_t *size, int32_t *medoid, double *diameter,
                                       double *avg_width, double *avg_width_all, double *sums_dev,
                                       ks_silhouette_stats *stats) {
  if (stats) memset(stats, 0, sizeof(*stats));
  KS_TRY(check_sil_args(diss_dev, n, group, ngroups, flags, width, a, b, neighbor, size, medoid, diameter, avg_width,
                        avg_width_all));
  KS_TRY(default_ctx(&ctx));
  KS_ENTER(ctx);
  return sil_impl(ctx, diss_dev, n, group, ngroups, width, a, b, neighbor, size, medoid, diameter, avg_width,
                  avg_width_all, sums_dev, stats);
}

extern "C" ks_status ks_silhouette(ks_ctx *ctx, const double *diss, int64_t n, const int32_t *group, int32_t ngroups,
                                   int32_t flags, double *width, double *a, double *b, int32_t *neighbor,
                                   int32_t *size, int32_t *medoid, double *diameter, double *avg_width,
                                   double *avg_width_all, double *sums) {
  KS_TRY(check_sil_args(diss, n, group, ngroups, flags, width, a, b, neighbor, size, medoid, diameter, avg_width,
                        avg_width_all));
  const int64_t total = dist_pair_count(n);
  for (int64_t o = 0; o < total; ++o)
    if (!std::isfinite(diss[o])) return not_finite((unsigned long long)o);
  KS_TRY(default_ctx(&ctx));
  KS_ENTER(ctx);
  const HostEnd host_end{ctx};  // (ks_set_host_cache)
  void *d = nullptr;
  DevFree sums_dev;
  KS_TRY(ensure(ctx, SLOT_REG_TMP, (size_t)total * 8, &d));
  if (sums) KS_TRY(dev_alloc(&sums_dev, (size_t)n * ngroups * 8, "the group sums"));
  KS_HIP(hipMemcpyAsync(d, diss, (size_t)total * 8, hipMemcpyHostToDevice, ctx->stream));
  KS_TRY(sil_impl(ctx, static_cast<const double *>(d), n, group, ngroups, width, a, b, neighbor, size, medoid,
                  diameter, avg_width, avg_width_all, static_cast<double *>(sums_dev.p), nullptr));
  if (sums) {
    KS_HIP(hipMemcpyAsync(sums, sums_dev.p, (size_t)n * ngroups * 8, hipMemcpyDeviceToHost, ctx->stream));
    KS_HIP(hipStreamSynchronize(ctx->stream));
  }
  return KS_OK;
}
