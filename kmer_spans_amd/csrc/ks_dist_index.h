// ks_dist_index.h -- index arithmetic of the pairwise distance kernels
// (ks_spectra_dist.hip), all in 64-bit integers.
//
// Condensed order (R's `dist` object, scipy's pdist): the pairs i < j of m rows
// by ascending i, then ascending j; pair (i, j) sits at
//     i * m - i * (i + 1) / 2 + (j - i - 1),
// row i's m - 1 - i entries being contiguous in j.  m(m - 1)/2 passes 2^31 at
// m = 65,537, so nothing here is an int.
//
// Tile order: the condensed form launches only the tiles on or above the
// diagonal of the T x T tile grid, as a linear grid: tile row r holds the
// T - r tiles (r, r) .. (r, T - 1), and row r starts at linear id
//     S(r) = r * T - r * (r - 1) / 2.
// dist_tile_of inverts that: r is the largest row with S(r) <= t.  The FP64
// square root only proposes r ((2T + 1)^2 - 8t < 2^54 for every T a grid can
// have, and the estimate is off by at most one either way); integer
// comparisons against S settle it.
// Host and device (ks_dist_pair_offsets / ks_dist_tiles_of export it;
// tests/test_spectra_dist.py walks it on the host, where a GPU test would need
// terabytes of output to reach the same ids).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define KS_DIST_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define KS_DIST_FN static inline
#endif

namespace ks {

// entries of the condensed form of m rows
KS_DIST_FN int64_t dist_pair_count(int64_t m) { return m < 2 ? 0 : (m % 2 ? (m - 1) / 2 * m : m / 2 * (m - 1)); }

// offset of pair (i, j), 0 <= i < j < m
KS_DIST_FN int64_t dist_pair_offset(int64_t i, int64_t j, int64_t m) {
  return i * m - (i % 2 ? (i + 1) / 2 * i : i / 2 * (i + 1)) + (j - i - 1);
}

// tiles on or above the diagonal of a T x T tile grid
KS_DIST_FN int64_t dist_tile_count(int64_t T) { return T % 2 ? (T + 1) / 2 * T : T / 2 * (T + 1); }

// linear id of the first tile of tile row r (r = T: the tile count)
KS_DIST_FN int64_t dist_tile_row_start(int64_t r, int64_t T) {
  return r * T - (r % 2 ? (r - 1) / 2 * r : r / 2 * (r - 1));
}

// linear tile id t in [0, dist_tile_count(T)) -> (tile row, tile column), row <= column
KS_DIST_FN void dist_tile_of(int64_t t, int64_t T, int64_t *row, int64_t *col) {
  const double b = (double)(2 * T + 1);
  int64_t r = (int64_t)((b - sqrt(b * b - 8.0 * (double)t)) * 0.5);
  if (r < 0) r = 0;
  if (r > T - 1) r = T - 1;
  while (r > 0 && dist_tile_row_start(r, T) > t) --r;
  while (r < T - 1 && dist_tile_row_start(r + 1, T) <= t) ++r;
  *row = r;
  *col = r + (t - dist_tile_row_start(r, T));
}

}  // namespace ks
