// ks_km_common.h -- what ks_kmeans.hip and ks_kmeans_seed.hip share: the
// row-major FP64 profile panel and its checks (k_km_normalise), the state block
// the checks report through, the host forms of the same checks and the guard of
// a call's one allocation.  Everything is in the unnamed namespace: each of the
// two files gets definitions of its own.
#pragma once
#include <cstdint>

#include "ks_internal.h"

namespace ks {
namespace {

struct KmState {
  // cnt - position of the first bad row index / empty row / non-finite centre entry / bad initial row (0: none)
  unsigned long long bad[4];
  int changed;
  int pad;
};

// A wave per selected row: the index is checked, the row summed in uint64 and
// p = cnt / T written to the row-major panel [cnt][ncol].  iota (may be null):
// iota[s] = s.
__global__ void __launch_bounds__(256) k_km_normalise(const uint32_t *__restrict__ sp, int64_t n, int ncol,
                                                      const int64_t *__restrict__ rows, int64_t cnt,
                                                      double *__restrict__ panel, int *__restrict__ iota,
                                                      KmState *__restrict__ state) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t s = (int64_t)blockIdx.x * 4 + wv;
  if (s >= cnt) return;  // wave-uniform
  if (iota && lane == 0) iota[s] = (int)s;
  const int64_t r = rows ? rows[s] : s;
  if (r < 0 || r >= n) {
    if (lane == 0) atomicMax(&state->bad[0], (unsigned long long)(cnt - s));
    return;
  }
  const uint32_t *row = sp + (size_t)r * ncol;
  unsigned long long t = 0;
  for (int c = lane; c < ncol; c += 64) t += row[c];
  for (int d = 32; d > 0; d >>= 1) t += __shfl_xor(t, d);
  if (t == 0) {
    if (lane == 0) atomicMax(&state->bad[1], (unsigned long long)(cnt - s));
    return;
  }
  const double tot = (double)t;  // below 2^44: exact
  double *dst = panel + (size_t)s * ncol;
  for (int c = lane; c < ncol; c += 64) dst[c] = (double)row[c] / tot;
}

struct DevFree {  // the work memory goes back before the call returns, whichever way it ends
  void *p = nullptr;
  ~DevFree() {
    if (p) (void)hipFree(p);
  }
};

ks_status check_km_common(int64_t n, int32_t ncol, const void *rows, int64_t m, int32_t flags, const char *what) {
  if (m < 1) return fail(KS_ERR_ARG, "%s needs at least 1 row (m = %lld)", what, (long long)m);
  if (m > 0x7ffffffeLL) return fail(KS_ERR_ARG, "too many selected rows for one call");
  if (ncol < 1 || ncol > KS_DIST_MAX_NCOL) return fail(KS_ERR_ARG, "ncol must be between 1 and %d", KS_DIST_MAX_NCOL);
  if (flags) return fail(KS_ERR_ARG, "unknown flags 0x%x for %s", (unsigned)flags, what);
  if (n < 0) return fail(KS_ERR_ARG, "the number of rows must not be negative");
  if (!rows && m > n) return fail(KS_ERR_ARG, "rows is NULL (rows 0 .. m - 1) but m = %lld exceeds n = %lld",
                                  (long long)m, (long long)n);
  return KS_OK;
}

// Indices and row sums of a host selection, as the device check reports them.
ks_status check_rows_and_sums_host(const uint32_t *spectra, int64_t n, int ncol, const int64_t *rows, int64_t m) {
  if (rows)
    for (int64_t s = 0; s < m; ++s)
      if (rows[s] < 0 || rows[s] >= n) return fail(KS_ERR_ARG, "row index %lld out of range", (long long)s);
  for (int64_t s = 0; s < m; ++s) {
    const uint32_t *row = spectra + (size_t)(rows ? rows[s] : s) * ncol;
    uint64_t t = 0;
    for (int c = 0; c < ncol; ++c) t += row[c];
    if (t == 0) return fail(KS_ERR_ARG, "row %lld has no counts", (long long)s);
  }
  return KS_OK;
}

}  // namespace
}  // namespace ks
