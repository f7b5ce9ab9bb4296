// ks_kmeans_seed.hip -- starts for ks_spectra_kmeans: maximin (farthest-first)
// and k-means++ (D^2 sampling) seeding of row-normalised region spectra
// (ks_spectra_kmeans_seed and its _dev form); the contract is in
// include/kmer_spans.h.
//
// g dependent steps, each one pass "distance of every row to one centre" over
// the shared row-major FP64 profile panel (ks_panel.hip).  Memory is O(m ncol); nothing of size m x g exists.  Every
// value is a fixed order of separate FP64 operations (-ffp-contract=off,
// csrc/Makefile).
//
// Step:    k_seed_step, a workgroup per chunk of KS_KM_CHUNK = 256 rows, a
//          thread per row.  The centre is the panel row whose position the
//          previous select wrote to rows_out[j]: it is read from device memory,
//          so the host queues all steps without waiting for any.  Slices of 16
//          columns of the 256 rows go through LDS, transposed on the way in (the
//          panel is read in 128-byte row segments, a thread then walks its own
//          row), the centre's 16 columns beside them; the next slice is loaded
//          into registers while the current one is summed.  A thread runs its
//          row's column chain, updates mind / near and leaves the new mind in LDS.
//          Thread 0 then runs the chunk's 256-long left-to-right sum C[c]; the
//          chunk's largest mind and its lowest position were reduced by wave
//          shuffles before the barrier and thread 64 merges the four waves, so
//          only the chain's own wave waits for the chain.
// Select:  k_seed_select, one workgroup of 1024.  The chunk sums are staged in
//          LDS in pieces of 2048 and thread 0 runs the prefix chain P over
//          them (nchunks dependent additions).  Maximin: the lexicographic
//          maximum over (value, lowest position) of the chunk records, exact in
//          any order.  D^2: the prefix is kept (P, m / 256 doubles), the first
//          chunk whose prefix exceeds t = u[j] * pot is found by all threads
//          (an integer minimum), and thread 0 walks that chunk's 256 values.
//          Step 0 only records `first`; a last call after step g - 1 writes
//          the final potential, radius and far_row.
// The 2 g + 1 launches after the checks are queued back to back; one read-back
// at the end brings pick_dist, potential and the result.
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "ks_internal.h"
#include "ks_panel.h"

namespace ks {
namespace {

constexpr int kSK = 16;        // columns per LDS slice
constexpr int kSPad = 257;     // row stride of the transposed slice: conflict-free reads along the rows
constexpr int kSelThreads = 1024;
constexpr int kSelPiece = 2048;  // chunk sums per LDS piece of the prefix chain
constexpr int kNoPos = 0x7fffffff;

static_assert(KS_KM_CHUNK == 256, "k_seed_step: a thread per row of a chunk");

struct SeedHead {  // the result's device image, in front of pick_dist [g] and potential [g]
  double pot;
  double radius;
  long long far_row;
  long long pad;
};

__device__ __forceinline__ bool seed_better(double ov, int op, double v, int p) {  // (value desc, position asc)
  return ov > v || (ov == v && op < p);
}

__global__ void __launch_bounds__(256) k_seed_step(const double *__restrict__ panel, int64_t m, int ncol,
                                                   const int64_t *__restrict__ rows_out, int j,
                                                   double *__restrict__ mind, int *__restrict__ near,
                                                   double *__restrict__ csum, double *__restrict__ cmax,
                                                   int *__restrict__ cpos) {
  __shared__ double As[kSK][kSPad];  // [c][row]
  __shared__ double Bs[kSK];
  __shared__ double vals[KS_KM_CHUNK];
  __shared__ double wmax[4];
  __shared__ int wpos[4];
  const int tid = threadIdx.x;
  const int64_t i0 = (int64_t)blockIdx.x * KS_KM_CHUNK;
  const int cnt = (int)min((int64_t)KS_KM_CHUNK, m - i0);
  const double *cen = panel + (size_t)rows_out[j] * ncol;
  // a slice in registers: 16 consecutive columns of one row per 16 lanes
  double reg[kSK], breg = 0.0;
  auto fetch = [&](int k0) {
    if (tid < kSK) breg = k0 + tid < ncol ? cen[k0 + tid] : 0.0;
#pragma unroll
    for (int e = 0; e < kSK; ++e) {
      const int idx = tid + 256 * e;
      const int ra = idx / kSK, ka = idx % kSK;
      reg[e] = (k0 + ka < ncol && ra < cnt) ? panel[(size_t)(i0 + ra) * ncol + k0 + ka] : 0.0;
    }
  };
  double acc = 0.0;
  fetch(0);
  for (int k0 = 0; k0 < ncol; k0 += kSK) {
    if (tid < kSK) Bs[tid] = breg;
#pragma unroll
    for (int e = 0; e < kSK; ++e) {
      const int idx = tid + 256 * e;
      As[idx % kSK][idx / kSK] = reg[e];
    }
    __syncthreads();
    if (k0 + kSK < ncol) fetch(k0 + kSK);  // the next slice is on its way while this one is summed
    // columns past ncol are staged as zeros on both sides: acc + 0 * 0 leaves acc's bits
#pragma unroll
    for (int kk = 0; kk < kSK; ++kk) {
      const double d = As[kk][tid] - Bs[kk];
      acc = acc + d * d;
    }
    __syncthreads();
  }
  double v = -1.0;  // below every mind: a row past m never wins
  int p = kNoPos;
  if (tid < cnt) {
    const double old = j == 0 ? std::numeric_limits<double>::infinity() : mind[i0 + tid];
    v = old;
    if (acc < old) {
      v = acc;
      mind[i0 + tid] = acc;
      near[i0 + tid] = j + 1;
    }
    p = (int)(i0 + tid);
  }
  vals[tid] = v;
  for (int d = 1; d < 64; d <<= 1) {
    const double ov = __shfl_xor(v, d);
    const int op = __shfl_xor(p, d);
    if (seed_better(ov, op, v, p)) v = ov, p = op;
  }
  if ((tid & 63) == 0) wmax[tid >> 6] = v, wpos[tid >> 6] = p;
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
#pragma unroll 8
    for (int t = 0; t < cnt; ++t) s = s + vals[t];
    csum[blockIdx.x] = s;
  }
  if (tid == 64) {
    v = wmax[0], p = wpos[0];
    for (int w = 1; w < 4; ++w)
      if (seed_better(wmax[w], wpos[w], v, p)) v = wmax[w], p = wpos[w];
    cmax[blockIdx.x] = v;
    cpos[blockIdx.x] = p;
  }
}

// j == 0: rows_out[0] = first.  1 <= j < g: the pick of step j from the state
// steps 0 .. j - 1 left.  j == g: the head (potential, radius, far_row).
__global__ void __launch_bounds__(kSelThreads) k_seed_select(int dsq, int j, int g, int64_t m, int nch, int64_t first,
                                                             const double *__restrict__ mind,
                                                             const double *__restrict__ csum,
                                                             const double *__restrict__ cmax,
                                                             const int *__restrict__ cpos, double *__restrict__ P,
                                                             const double *__restrict__ ud,
                                                             int64_t *__restrict__ rows_out,
                                                             SeedHead *__restrict__ head, double *__restrict__ pd,
                                                             double *__restrict__ potv) {
  __shared__ double piece[kSelPiece];
  __shared__ double sh_pot;
  __shared__ double rv[kSelThreads / 64];
  __shared__ int rp[kSelThreads / 64];
  __shared__ int cstar;
  const int tid = threadIdx.x;
  if (j == 0) {
    if (tid == 0) {
      rows_out[0] = first;
      pd[0] = potv[0] = std::numeric_limits<double>::infinity();
    }
    return;
  }
  const bool keep = dsq && j < g;  // the prefix is searched below
  double run = 0.0;                // thread 0's
  if (tid == 0) {
    cstar = kNoPos;
    if (keep) P[0] = 0.0;
  }
  for (int c0 = 0; c0 < nch; c0 += kSelPiece) {
    const int len = min(kSelPiece, nch - c0);
    for (int i = tid; i < len; i += kSelThreads) piece[i] = csum[c0 + i];
    __syncthreads();
    if (tid == 0) {
#pragma unroll 8
      for (int i = 0; i < len; ++i) {
        run = run + piece[i];
        piece[i] = run;
      }
    }
    __syncthreads();
    if (keep)
      for (int i = tid; i < len; i += kSelThreads) P[c0 + 1 + i] = piece[i];
    __syncthreads();  // the piece is reused, and P is read by other threads below
  }
  if (tid == 0) sh_pot = run;
  __syncthreads();
  const double pot = sh_pot;

  if (!keep) {  // maximin, or the final radius of either method
    double v = -1.0;
    int p = kNoPos;
    for (int c = tid; c < nch; c += kSelThreads)
      if (seed_better(cmax[c], cpos[c], v, p)) v = cmax[c], p = cpos[c];
    for (int d = 1; d < 64; d <<= 1) {
      const double ov = __shfl_xor(v, d);
      const int op = __shfl_xor(p, d);
      if (seed_better(ov, op, v, p)) v = ov, p = op;
    }
    if ((tid & 63) == 0) rv[tid >> 6] = v, rp[tid >> 6] = p;
    __syncthreads();
    if (tid != 0) return;
    for (int w = 1; w < kSelThreads / 64; ++w)
      if (seed_better(rv[w], rp[w], v, p)) v = rv[w], p = rp[w];
    if (j == g) {
      head->pot = pot;
      head->radius = v;
      head->far_row = p;
    } else {
      rows_out[j] = p;
      pd[j] = v;
      potv[j] = pot;
    }
    return;
  }

  if (pot == 0.0) {  // every row coincides with a picked one
    if (tid == 0) {
      rows_out[j] = 0;
      pd[j] = 0.0;
      potv[j] = pot;
    }
    return;
  }
  const double t = ud[j] * pot;
  for (int c = tid; c < nch; c += kSelThreads)
    if (P[c + 1] > t) {
      atomicMin(&cstar, c);  // an integer minimum: the same in any order
      break;                 // this thread's later chunks are higher
    }
  __syncthreads();
  const int cs = cstar == kNoPos ? nch - 1 : cstar;  // u < 1 makes t < pot = P[nch]: a chunk is found
  const int64_t i0 = (int64_t)cs * KS_KM_CHUNK;
  const int cnt = (int)min((int64_t)KS_KM_CHUNK, m - i0);
  if (tid < cnt) piece[tid] = mind[i0 + tid];
  __syncthreads();
  if (tid != 0) return;
  const double base = P[cs];
  double acc = 0.0;
  int hit = cnt - 1;  // at the chunk's last row the test is P[cs + 1] > t
  for (int s = 0; s < cnt; ++s) {
    acc = acc + piece[s];
    if (base + acc > t) {
      hit = s;
      break;
    }
  }
  rows_out[j] = i0 + hit;
  pd[j] = piece[hit];
  potv[j] = pot;
}

// The work memory of a call, one allocation: the panel, then everything else.
struct SeedWork {
  double *panel, *csum, *cmax, *P, *ud, *pd, *potv;
  int *cpos;
  SeedHead *head;  // head, pd [g], potv [g] are contiguous: one copy brings them back
  unsigned long long *bad;  // the panel's two words: first bad row index, first empty row
  size_t panel_bytes = 0, bytes = 0;

  // base null: only the sizes
  void lay(char *base, int64_t m, int ncol, int g, int nch) {
    Arena a{base};
    panel = a.take<double>((size_t)m * ncol);
    panel_bytes = a.off;
    csum = a.take<double>((size_t)nch);
    cmax = a.take<double>((size_t)nch);
    cpos = a.take<int>((size_t)nch);
    P = a.take<double>((size_t)(nch + 1));
    ud = a.take<double>((size_t)g);
    head = reinterpret_cast<SeedHead *>(a.take<char>(sizeof(SeedHead) + (size_t)g * 16));
    pd = reinterpret_cast<double *>(reinterpret_cast<char *>(head) + sizeof(SeedHead));
    potv = pd + g;
    bad = a.take<unsigned long long>(2);
    bytes = a.off;
  }
};

// first: -1 is resolved by the caller of seed_impl.
ks_status check_seed_args(const void *spectra, int64_t n, int32_t ncol, const void *rows, int64_t m, int32_t g,
                          int32_t flags, int64_t first, const double *u, const void *rows_out, const void *near,
                          const void *mind, const void *pick_dist, const void *potential, const void *res) {
  KS_TRY(panel_check_common(n, ncol, rows, m, 0, "a seeding call"));
  if (g < 1 || g > KS_KM_MAX_GROUPS)
    return fail(KS_ERR_ARG, "the number of groups must be between 1 and %d (g = %d)", KS_KM_MAX_GROUPS, (int)g);
  if (flags != KS_SEED_MAXIMIN && flags != KS_SEED_DSQ)
    return fail(KS_ERR_ARG, "unknown flags 0x%x for a seeding call", (unsigned)flags);
  if (!spectra) return fail(KS_ERR_ARG, "null spectra");
  if (flags == KS_SEED_DSQ && !u) return fail(KS_ERR_ARG, "KS_SEED_DSQ needs the g uniform numbers u");
  if (flags == KS_SEED_MAXIMIN && u) return fail(KS_ERR_ARG, "u must be NULL with KS_SEED_MAXIMIN");
  if (u)
    for (int32_t j = 0; j < g; ++j)
      if (!(u[j] >= 0.0 && u[j] < 1.0)) return fail(KS_ERR_ARG, "u[%d] is not in [0, 1)", (int)j);
  if (first == -1 && flags != KS_SEED_DSQ)
    return fail(KS_ERR_ARG, "first = -1 (a drawn first row) needs KS_SEED_DSQ");
  if (first < -1 || first >= m)
    return fail(KS_ERR_ARG, "first = %lld is not in 0 .. %lld", (long long)first, (long long)(m - 1));
  if (!rows_out || !near || !mind || !pick_dist || !potential || !res) return fail(KS_ERR_ARG, "null output");
  return KS_OK;
}

// Everything but the device-side checks validated; u, pick_dist, potential, res are host pointers.
ks_status seed_impl(ks_ctx *ctx, const uint32_t *sp, int64_t n, int ncol, const int64_t *rows, int64_t m, int g,
                    int flags, int64_t first, const double *u, int64_t *rows_out, int *near, double *mind,
                    double *pick_dist, double *potential, ks_seed_result *res, ks_seed_stats *stats) {
  hipStream_t st = ctx->stream;
  const int dsq = flags == KS_SEED_DSQ;
  if (first == -1) first = (int64_t)(u[0] * (double)m);
  const int nch = (int)((m + KS_KM_CHUNK - 1) / KS_KM_CHUNK);
  SeedWork w;
  DevFree mem;
  w.lay(nullptr, m, ncol, g, nch);
  KS_TRY(dev_alloc(&mem, w.bytes, "the profile panel"));
  w.lay(static_cast<char *>(mem.p), m, ncol, g, nch);
  KS_HIP(hipEventRecord(ctx->ev[0], st));
  KS_HIP(hipMemsetAsync(w.bad, 0, 16, st));
  KS_TRY(panel_normalise(ctx, sp, n, ncol, rows, m, PanelRoot::kNone, w.panel, nullptr, &w.bad[0], &w.bad[1]));
  if (dsq) KS_HIP(hipMemcpyAsync(w.ud, u, (size_t)g * 8, hipMemcpyHostToDevice, st));
  unsigned long long hbad[2] = {0, 0};
  KS_HIP(hipMemcpyAsync(hbad, w.bad, sizeof(hbad), hipMemcpyDeviceToHost, st));
  KS_HIP(hipStreamSynchronize(st));
  KS_TRY(panel_report(hbad, 1, m, 0));
  // from here on the outputs are written
  KS_HIP(hipEventRecord(ctx->ev[1], st));
  for (int j = 0; j <= g; ++j) {
    hipLaunchKernelGGL(k_seed_select, dim3(1), dim3(kSelThreads), 0, st, dsq, j, g, m, nch, first, mind, w.csum,
                       w.cmax, w.cpos, w.P, w.ud, rows_out, w.head, w.pd, w.potv);
    if (j < g)
      hipLaunchKernelGGL(k_seed_step, dim3((unsigned)nch), dim3(256), 0, st, w.panel, m, ncol, rows_out, j, mind,
                         near, w.csum, w.cmax, w.cpos);
  }
  KS_HIP(hipGetLastError());
  KS_HIP(hipEventRecord(ctx->ev[2], st));
  std::vector<double> back(sizeof(SeedHead) / 8 + (size_t)2 * g);
  KS_HIP(hipMemcpyAsync(back.data(), w.head, back.size() * 8, hipMemcpyDeviceToHost, st));
  KS_HIP(hipStreamSynchronize(st));  // the work memory is freed on return
  SeedHead head;
  memcpy(&head, back.data(), sizeof(head));
  memcpy(pick_dist, back.data() + sizeof(SeedHead) / 8, (size_t)g * 8);
  memcpy(potential, back.data() + sizeof(SeedHead) / 8 + g, (size_t)g * 8);
  int nd = 1;
  for (int j = 1; j < g; ++j) nd += pick_dist[j] > 0.0;
  res->n_distinct = nd;
  res->reserved = 0;
  res->potential = head.pot;
  res->radius = head.radius;
  res->far_row = head.far_row;
  if (stats) {
    KS_TRY(event_ms(ctx, 0, 2, &stats->ms_total));
    KS_TRY(event_ms(ctx, 0, 1, &stats->ms_normalise));
    KS_TRY(event_ms(ctx, 1, 2, &stats->ms_steps));
    stats->n_launches = 2 + 2 * (int64_t)g;
    stats->panel_bytes = (int64_t)w.panel_bytes;
    stats->work_bytes = (int64_t)(w.bytes - w.panel_bytes);
  }
  return KS_OK;
}

}  // namespace
}  // namespace ks

using namespace ks;

extern "C" ks_status ks_spectra_kmeans_seed_dev(ks_ctx *ctx, const uint32_t *spectra_dev, int64_t n, int32_t ncol,
                                                const int64_t *rows_dev, int64_t m, int32_t g, int32_t flags,
                                                int64_t first, const double *u, int64_t *rows_out_dev,
                                                int32_t *near_dev, double *mind_dev, double *pick_dist,
                                                double *potential, ks_seed_result *res, ks_seed_stats *stats) {
  if (stats) memset(stats, 0, sizeof(*stats));
  KS_TRY(check_seed_args(spectra_dev, n, ncol, rows_dev, m, g, flags, first, u, rows_out_dev, near_dev, mind_dev,
                         pick_dist, potential, res));
  KS_TRY(default_ctx(&ctx));
  KS_ENTER(ctx);
  return seed_impl(ctx, spectra_dev, n, ncol, rows_dev, m, g, flags, first, u, rows_out_dev, near_dev, mind_dev,
                   pick_dist, potential, res, stats);
}

extern "C" ks_status ks_spectra_kmeans_seed(ks_ctx *ctx, const uint32_t *spectra, int64_t n, int32_t ncol,
                                            const int64_t *rows, int64_t m, int32_t g, int32_t flags, int64_t first,
                                            const double *u, int64_t *rows_out, int32_t *near, double *mind,
                                            double *pick_dist, double *potential, ks_seed_result *res) {
  KS_TRY(check_seed_args(spectra, n, ncol, rows, m, g, flags, first, u, rows_out, near, mind, pick_dist, potential,
                         res));
  KS_TRY(panel_check_rows_host(spectra, n, ncol, rows, m, nullptr, 0));
  KS_TRY(default_ctx(&ctx));
  KS_ENTER(ctx);
  const HostEnd host_end{ctx};  // (ks_set_host_cache)
  void *d_out = nullptr;
  KS_TRY(ensure(ctx, SLOT_REG_TMP, (size_t)m * 12, &d_out));
  SpectraUpload up;
  KS_TRY(upload_spectra(ctx, spectra, n, ncol, rows, m, nullptr, 0, g, &up));
  hipStream_t st = ctx->stream;
  int64_t *d_ro = up.extra;
  double *d_mind = static_cast<double *>(d_out);
  int *d_near = reinterpret_cast<int *>(d_mind + m);
  KS_TRY(seed_impl(ctx, up.sp, n, ncol, up.rows, m, g, flags, first, u, d_ro, d_near, d_mind, pick_dist, potential, res,
                   nullptr));
  KS_HIP(hipMemcpyAsync(rows_out, d_ro, (size_t)g * 8, hipMemcpyDeviceToHost, st));
  KS_HIP(hipMemcpyAsync(near, d_near, (size_t)m * 4, hipMemcpyDeviceToHost, st));
  KS_HIP(hipMemcpyAsync(mind, d_mind, (size_t)m * 8, hipMemcpyDeviceToHost, st));
  KS_HIP(hipStreamSynchronize(st));
  return KS_OK;
}
