// ks_finite_check.h -- the finiteness pass over a condensed dissimilarity
// vector, shared by ks_hclust.hip, ks_nj.hip and ks_silhouette.hip: the matrix is read once
// (16-byte loads where the base allows, grid-stride) and the lowest offset of
// a non-finite entry is kept with atomicMin; one 8-byte read-back ends a call
// with a bad entry before anything is modified.  Include after ks_internal.h.
#pragma once
#include <cmath>

#include "ks_internal.h"

namespace ks {
namespace {

constexpr unsigned long long kNoBad = ~0ULL;

__global__ void __launch_bounds__(256) k_hclust_check(const double *__restrict__ d, int64_t total,
                                                      unsigned long long *__restrict__ bad) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x, t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t pairs2 = total >> 1;  // hipMalloc'd or offset by whole tensors: checked for 16-byte alignment by the caller
  unsigned long long first = kNoBad;
  const double2 *d2 = reinterpret_cast<const double2 *>(d);
  for (int64_t p = t0; p < pairs2; p += stride) {
    const double2 x = d2[p];
    // ascending p per thread: the first hit is this thread's lowest
    if (first == kNoBad && !(isfinite(x.x) && isfinite(x.y))) first = (unsigned long long)(2 * p + (isfinite(x.x) ? 1 : 0));
  }
  if (t0 == 0 && (total & 1) && !isfinite(d[total - 1]) && first == kNoBad) first = (unsigned long long)(total - 1);
  if (first != kNoBad) atomicMin(bad, first);
}

// the same for a base address that is only 8-byte aligned
__global__ void __launch_bounds__(256) k_hclust_check1(const double *__restrict__ d, int64_t total,
                                                       unsigned long long *__restrict__ bad) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  unsigned long long first = kNoBad;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += stride)
    if (first == kNoBad && !isfinite(d[p])) first = (unsigned long long)p;
  if (first != kNoBad) atomicMin(bad, first);
}

inline ks_status not_finite(unsigned long long off) {
  return fail(KS_ERR_ARG, "dissimilarity at offset %llu is not finite", off);
}

// Queues the pass on ctx->stream between ctx->ev[0] and ctx->ev[1], reads the
// result back and synchronises.  bad: a word of the context's SLOT_SCALARS.
// KS_ERR_ARG (not_finite) if an entry is NaN or an infinity.
inline ks_status check_all_finite(ks_ctx *ctx, const double *diss, int64_t total, unsigned long long *bad) {
  hipStream_t st = ctx->stream;
  KS_HIP(hipEventRecord(ctx->ev[0], st));
  unsigned long long hbad = kNoBad;
  KS_HIP(hipMemsetAsync(bad, 0xff, 8, st));
  {
    const bool al16 = (reinterpret_cast<uintptr_t>(diss) & 15) == 0;
    const int64_t items = al16 ? (total + 1) / 2 : total;
    const unsigned grid = (unsigned)std::min<int64_t>((items + 255) / 256, (int64_t)ctx->num_cus * 8);
    if (al16)
      hipLaunchKernelGGL(k_hclust_check, dim3(grid), dim3(256), 0, st, diss, total, bad);
    else
      hipLaunchKernelGGL(k_hclust_check1, dim3(grid), dim3(256), 0, st, diss, total, bad);
    KS_HIP(hipGetLastError());
  }
  KS_HIP(hipEventRecord(ctx->ev[1], st));
  KS_HIP(hipMemcpyAsync(&hbad, bad, 8, hipMemcpyDeviceToHost, st));
  KS_HIP(hipStreamSynchronize(st));
  if (hbad != kNoBad) return not_finite(hbad);
  return KS_OK;
}

}  // namespace
}  // namespace ks
