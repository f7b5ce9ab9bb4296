// ks_dist_metric.h -- the metric field of the distance flags (KS_DIST_METRIC_MASK,
// include/kmer_spans.h) as the distance and nearest-neighbour
// kernels use it: the kernels are templates on the metric M, a KS_DIST_*
// value, and take their per-column step and their last step from here, so the
// orders of operations the header fixes are written once.  Include after
// hip_runtime.h (ks_internal.h).
#pragma once
#include <type_traits>

#include "ks_internal.h"

namespace ks {

// hellinger is the Euclidean loop over a panel of roots (PanelRoot::kSqrt)
constexpr bool metric_is_l2(int m) { return m == KS_DIST_EUCLIDEAN || m == KS_DIST_HELLINGER; }
constexpr bool metric_has_squared(int m) { return metric_is_l2(m); }

// One column of one pair.  cnt is canberra's count of the columns it did not
// omit; the other metrics leave it alone (and their kernels keep no register
// for it).  A column staged as zero on both sides changes no bit in any
// metric: acc + 0 * 0, acc + |0|, max(acc, |0|) with acc >= +0, and canberra
// omits it without counting it.
template <int M>
__device__ __forceinline__ void metric_step(double &acc, int &cnt, double a, double b) {
  if constexpr (metric_is_l2(M)) {
    const double d = a - b;
    acc = acc + d * d;
  } else if constexpr (M == KS_DIST_MANHATTAN) {
    acc = acc + fabs(a - b);
  } else if constexpr (M == KS_DIST_MAXIMUM) {
    // t > acc ? t : acc for the numbers (both are >= +0, so the bits agree); the hardware maximum drops a NaN
    // t, which only a row without counts produces: the distance kernel's last step puts it back
    acc = fmax(acc, fabs(a - b));
  } else {
    static_assert(M == KS_DIST_CANBERRA, "unknown metric");
    const double s = a + b;
    const double q = fabs(a - b) / s;
    const bool omit = s == 0.0;  // false for a NaN s: the column counts and acc becomes NaN
    acc = acc + (omit ? 0.0 : q);  // acc + 0.0 keeps the bits of acc >= +0
    cnt += omit ? 0 : 1;
  }
}

// The value a pair is ranked by in ks_spectra_knn, and what the last step
// starts from: acc, for canberra scaled by the columns it kept.
template <int M>
__device__ __forceinline__ double metric_value(double acc, int cnt, int ncol) {
  if constexpr (M == KS_DIST_CANBERRA)
    return cnt == ncol ? acc : acc / ((double)cnt / (double)ncol);
  else
    return acc;
}

// The distance returned for a value.
template <int M>
__device__ __forceinline__ double metric_result(double v, int squared) {
  if constexpr (M == KS_DIST_EUCLIDEAN) {
    return squared ? v : sqrt(v);
  } else if constexpr (M == KS_DIST_HELLINGER) {
    const double h = 0.5 * v;
    return squared ? h : sqrt(h);
  } else {
    return v;
  }
}

// f(std::integral_constant<int, M>) for the metric of (checked) flags.
template <class F>
ks_status metric_dispatch(int flags, F &&f) {
  switch (flags & KS_DIST_METRIC_MASK) {
    case KS_DIST_MANHATTAN: return f(std::integral_constant<int, KS_DIST_MANHATTAN>{});
    case KS_DIST_MAXIMUM: return f(std::integral_constant<int, KS_DIST_MAXIMUM>{});
    case KS_DIST_CANBERRA: return f(std::integral_constant<int, KS_DIST_CANBERRA>{});
    case KS_DIST_HELLINGER: return f(std::integral_constant<int, KS_DIST_HELLINGER>{});
    default: return f(std::integral_constant<int, KS_DIST_EUCLIDEAN>{});
  }
}

}  // namespace ks
