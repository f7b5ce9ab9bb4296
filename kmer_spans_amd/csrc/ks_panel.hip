// ks_panel.hip -- the row-major FP64 profile panel of the spectra analyses and
// the scaffold of their calls (ks_panel.h).
//
// Normalise: k_panel_normalise, a wave per selected row: the index is checked,
//            the row summed in uint64 and p = cnt / T written to the ROW-MAJOR
//            panel [cnt][ncol].  A bad index or a row without counts is
//            recorded as cnt - s with integer atomicMax, so the first position
//            wins in any order; the caller reads the words back with whatever
//            else it checks and panel_report ends the call before any output is
//            written.  panel_check_rows_host is the same check on host buffers.
#include "ks_panel.h"

namespace ks {

// kRoot: the entry is sqrt(p) (PanelRoot::kSqrt); the instantiation without it is the kernel of every other caller.
template <bool kRoot>
__global__ void __launch_bounds__(256) k_panel_normalise(const uint32_t *__restrict__ sp, int64_t n, int ncol,
                                                         const int64_t *__restrict__ rows, int64_t cnt,
                                                         double *__restrict__ panel, int *__restrict__ iota,
                                                         unsigned long long *__restrict__ bad_index,
                                                         unsigned long long *__restrict__ bad_empty) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t s = (int64_t)blockIdx.x * 4 + wv;
  if (s >= cnt) return;  // wave-uniform
  if (iota && lane == 0) iota[s] = (int)s;
  const int64_t r = rows ? rows[s] : s;
  if (r < 0 || r >= n) {
    if (lane == 0) atomicMax(bad_index, (unsigned long long)(cnt - s));
    return;
  }
  const uint32_t *row = sp + (size_t)r * ncol;
  unsigned long long t = 0;
  for (int c = lane; c < ncol; c += 64) t += row[c];
  for (int d = 32; d > 0; d >>= 1) t += __shfl_xor(t, d);
  if (t == 0) {
    if (lane == 0) atomicMax(bad_empty, (unsigned long long)(cnt - s));
    // the two reports stay two paths: merged into one behind a select of the word, they cost two more VGPRs
    asm volatile("" ::: "memory");
    return;
  }
  const double tot = (double)t;  // below 2^44: exact
  double *dst = panel + (size_t)s * ncol;
  for (int c = lane; c < ncol; c += 64) {
    const double p = (double)row[c] / tot;
    dst[c] = kRoot ? sqrt(p) : p;
  }
}

namespace {
// [2 * what + side]: what 0 a bad index, 1 a row without counts
const char *const kBadText[4] = {"row index %lld out of range", "row index %lld of the second selection out of range",
                                 "row %lld has no counts", "row %lld of the second selection has no counts"};
}  // namespace

ks_status panel_check_count(int64_t m, int64_t least, const char *what, const char *unit, const char *name) {
  if (m < least)
    return fail(KS_ERR_ARG, "%s needs at least %lld %s%s (%s = %lld)", what, (long long)least, unit,
                least == 1 ? "" : "s", name, (long long)m);
  return KS_OK;
}

ks_status panel_check_most(int64_t m, int64_t most) {
  if (m > most) return fail(KS_ERR_ARG, "too many selected rows for one call");
  return KS_OK;
}

ks_status panel_check_ncol(int32_t ncol, int32_t most) {
  if (ncol < 1 || ncol > most) return fail(KS_ERR_ARG, "ncol must be between 1 and %d", (int)most);
  return KS_OK;
}

ks_status panel_check_n(int64_t n) {
  if (n < 0) return fail(KS_ERR_ARG, "the number of rows must not be negative");
  return KS_OK;
}

ks_status panel_check_null_rows(const void *rows, int64_t cnt, int64_t n, const char *rows_name,
                                const char *cnt_name) {
  if (!rows && cnt > n)
    return fail(KS_ERR_ARG, "%s is NULL (rows 0 .. %s - 1) but %s = %lld exceeds n = %lld", rows_name, cnt_name,
                cnt_name, (long long)cnt, (long long)n);
  return KS_OK;
}

ks_status panel_check_common(int64_t n, int32_t ncol, const void *rows, int64_t m, int32_t flags, const char *what) {
  KS_TRY(panel_check_count(m, 1, what, "row", "m"));
  KS_TRY(panel_check_most(m, 0x7ffffffeLL));
  KS_TRY(panel_check_ncol(ncol, KS_DIST_MAX_NCOL));
  if (flags) return fail(KS_ERR_ARG, "unknown flags 0x%x for %s", (unsigned)flags, what);
  KS_TRY(panel_check_n(n));
  return panel_check_null_rows(rows, m, n, "rows", "m");
}

ks_status dist_check_metric(int32_t flags) {
  static const char *const kName[] = {"euclidean", "manhattan", "maximum", "canberra", "hellinger"};
  const int metric = flags & KS_DIST_METRIC_MASK;
  if (metric > KS_DIST_HELLINGER) return fail(KS_ERR_ARG, "unknown distance metric %d", metric >> 8);
  if ((flags & KS_DIST_SQUARED) && metric != KS_DIST_EUCLIDEAN && metric != KS_DIST_HELLINGER)
    return fail(KS_ERR_ARG, "KS_DIST_SQUARED has no meaning for the %s metric: the flag needs euclidean or hellinger",
                kName[metric >> 8]);
  return KS_OK;
}

ks_status panel_normalise(ks_ctx *ctx, const uint32_t *sp, int64_t n, int ncol, const int64_t *rows, int64_t cnt,
                          PanelRoot root, double *panel, int *iota, unsigned long long *bad_index,
                          unsigned long long *bad_empty) {
  const dim3 grid((unsigned)((cnt + 3) / 4));
  if (root == PanelRoot::kSqrt)
    hipLaunchKernelGGL(k_panel_normalise<true>, grid, dim3(256), 0, ctx->stream, sp, n, ncol, rows, cnt, panel, iota,
                       bad_index, bad_empty);
  else
    hipLaunchKernelGGL(k_panel_normalise<false>, grid, dim3(256), 0, ctx->stream, sp, n, ncol, rows, cnt, panel, iota,
                       bad_index, bad_empty);
  KS_HIP(hipGetLastError());
  return KS_OK;
}

ks_status panel_report(const unsigned long long *bad, int sides, int64_t na, int64_t nb) {
  for (int what = 0; what < 2; ++what)
    for (int side = 0; side < sides; ++side)
      if (const unsigned long long b = bad[what * sides + side])
        return fail(KS_ERR_ARG, kBadText[2 * what + side], (long long)((side ? nb : na) - (int64_t)b));
  return KS_OK;
}

ks_status panel_check_index_host(const int64_t *rows, int64_t cnt, int64_t n, int side) {
  if (!rows) return KS_OK;
  for (int64_t s = 0; s < cnt; ++s)
    if (rows[s] < 0 || rows[s] >= n) return fail(KS_ERR_ARG, kBadText[side], (long long)s);
  return KS_OK;
}

ks_status panel_check_rows_host(const uint32_t *spectra, int64_t n, int ncol, const int64_t *rows, int64_t na,
                                const int64_t *rows_b, int64_t nb) {
  const int64_t *sel[2] = {rows, rows_b};
  const int64_t cnt[2] = {na, rows_b ? nb : 0};
  for (int side = 0; side < 2; ++side) KS_TRY(panel_check_index_host(sel[side], cnt[side], n, side));
  for (int side = 0; side < 2; ++side)
    for (int64_t s = 0; s < cnt[side]; ++s) {
      const uint32_t *row = spectra + (size_t)(sel[side] ? sel[side][s] : s) * ncol;
      uint64_t t = 0;
      for (int c = 0; c < ncol; ++c) t += row[c];
      if (t == 0) return fail(KS_ERR_ARG, kBadText[2 + side], (long long)s);
    }
  return KS_OK;
}

ks_status upload_spectra(ks_ctx *ctx, const uint32_t *spectra, int64_t n, int ncol, const int64_t *rows, int64_t na,
                         const int64_t *rows_b, int64_t nb, int64_t extra, SpectraUpload *up) {
  void *d_sp = nullptr, *d_rows = nullptr;
  KS_TRY(ensure(ctx, SLOT_COUNTS, (size_t)n * ncol * 4, &d_sp));
  KS_TRY(ensure(ctx, SLOT_REGIONS, (size_t)(na + nb + extra + 1) * 8, &d_rows));
  KS_HIP(hipMemcpyAsync(d_sp, spectra, (size_t)n * ncol * 4, hipMemcpyHostToDevice, ctx->stream));
  int64_t *r = static_cast<int64_t *>(d_rows);
  *up = SpectraUpload();
  up->sp = static_cast<const uint32_t *>(d_sp);
  up->extra = r + na + nb;
  if (rows) {
    up->rows = r;
    KS_HIP(hipMemcpyAsync(r, rows, (size_t)na * 8, hipMemcpyHostToDevice, ctx->stream));
  }
  if (rows_b) {
    up->rows_b = r + na;
    KS_HIP(hipMemcpyAsync(r + na, rows_b, (size_t)nb * 8, hipMemcpyHostToDevice, ctx->stream));
  }
  return KS_OK;
}

}  // namespace ks
