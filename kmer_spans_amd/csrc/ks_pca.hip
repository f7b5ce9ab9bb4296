// ks_pca.hip -- principal components of row-normalised region spectra
// (ks_spectra_pca / ks_spectra_pca_dev, include/kmer_spans.h).
//
// What the reference's author does with the spectra besides dist() and hclust()
// (test.R:734-736, :811): prcomp() of the profile matrix, uncentred and centred.
// Here the spectra stay in HBM as ks_region_spectra_dev wrote them; the input is
// that n x ncol uint32 matrix and an optional row selection, as for
// ks_spectra_dist_dev.
//
// The centre, the cross-product G and the scores are fixed as orders of separate
// FP64 operations (the header comment; -ffp-contract=off, csrc/Makefile): one
// accumulator per entry, rows (or columns) ascending, so their bits do not
// depend on tile shape or grid and a host loop predicts them.  The eigen stage
// uses sqrt and division and is fixed as an algorithm, not as bits.
//
// Normalise: the shared row-major profile panel [m][ncol] (ks_panel.hip); one
//            16-byte read-back of its two words ends the call before any output
//            is written.
// Centre:    k_pca_center: a block per 16 columns stages 128 rows at a time in
//            LDS with all 256 threads (the loads are what is slow), then 16
//            threads run the 16 column chains over the staged rows: the chains
//            are not split, they overlap across columns and with the loads of
//            the other blocks.  k_pca_subtract rewrites the panel as xc.
// G:         k_pca_gram: 32 x 32 tiles on or above the diagonal (the linear tile
//            grid of ks_dist_index.h), 256 threads with 2 x 2 accumulators each,
//            chunks of 128 panel rows staged in LDS (the next chunk is fetched
//            into registers meanwhile), mirrored on store.  The tile is small
//            because the rows cannot be split: ncol = 256 gives 36 blocks, each
//            a chain over all m rows.
// Jacobi:    k_pca_jac_round, one launch per round of the round-robin order, no
//            kernel waits on another workgroup.  The matrix is double-buffered:
//            every thread recomputes the rotation of the one or two pairs it
//            needs from the round's read-only input (the same operations on the
//            same operands: the same bits in every thread), owns the 2 x 2 block
//            (pair k1 <= pair k2) and writes it and its mirror image, so the
//            matrix stays symmetric in bits; V is updated in place by threads
//            that own (row, pair).  Rotations are counted per sweep with integer
//            atomics; a launch whose previous sweep counted none returns at
//            once, so the decision to stop is taken on the device and the host
//            reads the counters once per few sweeps.
// Finish:    k_pca_finish: a thread per Jacobi column ranks its eigenvalue
//            (descending, ties by column), fixes the sign and writes sdev and
//            its column of rotation.
// Project:   k_pca_project: 64 x 64 tiles of panel x rotation, 4 x 4 accumulators
//            per thread, chunks of 16 columns staged in LDS, c ascending.
#include <cmath>
#include <cstring>

#include "ks_panel.h"
// after hip_runtime.h (ks_internal.h): the header's functions are __host__ __device__ here
#include "ks_dist_index.h"

namespace ks {
namespace {

constexpr int kCC = 16;    // k_pca_center: columns per block
constexpr int kCR = 128;   // rows per LDS chunk: 128 x 16 x 8 B = 16 KiB
constexpr int kGT = 32;    // k_pca_gram: tile edge (columns of the panel)
constexpr int kGR = 128;   // panel rows per LDS chunk: 2 x 128 x 32 x 8 B = 64 KiB
constexpr int kPT = 64;    // k_pca_project: tile edge (rows x components)
constexpr int kPK = 16;    // columns per LDS chunk
constexpr double kEps = 0x1p-52;

struct PcaState {
  unsigned long long bad[2];  // cnt - s of the first bad index / of the first empty row (0: none)
  double floor;               // 2^-52 * the largest |diagonal entry| of the input G
  int rot[KS_PCA_MAX_SWEEPS]; // rotations applied per sweep
};

// Slot i of round `round` of the round-robin order of P (even) indices, as (low, high).
__host__ __device__ inline void pca_slot_pair(int P, int round, int i, int *p, int *q) {
  const int n1 = P - 1;
  int a, b;
  if (i == 0) {
    a = P - 1;
    b = round;
  } else {
    a = (round + i) % n1;
    b = (round - i + n1) % n1;
  }
  *p = a < b ? a : b;
  *q = a < b ? b : a;
}

__global__ void __launch_bounds__(256) k_pca_center(const double *__restrict__ panel, int64_t m, int ncol,
                                                    double *__restrict__ center) {
  __shared__ double buf[kCR][kCC];
  const int tid = threadIdx.x, c0 = blockIdx.x * kCC;
  double acc = 0.0;
  for (int64_t r0 = 0; r0 < m; r0 += kCR) {
#pragma unroll
    for (int e = 0; e < kCR * kCC / 256; ++e) {
      const int idx = tid + 256 * e, rr = idx >> 4, cc = idx & 15;
      buf[rr][cc] = (r0 + rr < m && c0 + cc < ncol) ? panel[(size_t)(r0 + rr) * ncol + c0 + cc] : 0.0;
    }
    __syncthreads();
    if (tid < kCC) {
      const int rc = (int)min((int64_t)kCR, m - r0);
      for (int rr = 0; rr < rc; ++rr) acc = acc + buf[rr][tid];
    }
    __syncthreads();
  }
  if (tid < kCC && c0 + tid < ncol) center[c0 + tid] = acc / (double)m;
}

__global__ void __launch_bounds__(256) k_pca_subtract(double *__restrict__ panel, int64_t total, int ncol,
                                                      const double *__restrict__ center) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride)
    panel[i] = panel[i] - center[i % ncol];
}

// G[a][b] = sum over the panel rows ascending of xc[r][a] * xc[r][b], into the
// P x P work matrix (ld = P, the padding stays zero) and, if asked for, into the
// ncol x ncol output.
__global__ void __launch_bounds__(256) k_pca_gram(const double *__restrict__ panel, int64_t m, int ncol, int64_t tiles,
                                                  double *__restrict__ work, int ld, double *__restrict__ gout) {
  __shared__ __attribute__((aligned(16))) double As[kGR][kGT];
  __shared__ __attribute__((aligned(16))) double Bs[kGR][kGT];
  int64_t tr, tc;
  dist_tile_of((int64_t)blockIdx.x, tiles, &tr, &tc);
  const int a0 = (int)tr * kGT, b0 = (int)tc * kGT;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  double acc[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
  // the next chunk's rows are fetched into registers while this one is summed: a block runs
  // alone on its CU (ncol = 256 has 36 of them) and would otherwise wait out every load
  constexpr int kPer = kGR * kGT / 256;
  double pa[kPer], pb[kPer];
  auto fetch = [&](int64_t r0) {
#pragma unroll
    for (int e = 0; e < kPer; ++e) {
      const int idx = tid + 256 * e, rr = idx >> 5, cc = idx & 31;
      const bool in_r = r0 + rr < m;
      const size_t base = (size_t)(r0 + rr) * ncol;
      pa[e] = (in_r && a0 + cc < ncol) ? panel[base + a0 + cc] : 0.0;
      pb[e] = tr == tc ? pa[e] : ((in_r && b0 + cc < ncol) ? panel[base + b0 + cc] : 0.0);
    }
  };
  fetch(0);
  for (int64_t r0 = 0; r0 < m; r0 += kGR) {
#pragma unroll
    for (int e = 0; e < kPer; ++e) {
      const int idx = tid + 256 * e, rr = idx >> 5, cc = idx & 31;
      As[rr][cc] = pa[e];
      Bs[rr][cc] = pb[e];
    }
    __syncthreads();
    if (r0 + kGR < m) fetch(r0 + kGR);
    const int rc = (int)min((int64_t)kGR, m - r0);
#pragma unroll 8
    for (int rr = 0; rr < rc; ++rr) {
      const double a[2] = {As[rr][ty * 2], As[rr][ty * 2 + 1]};
      const double b[2] = {Bs[rr][tx], Bs[rr][tx + 16]};
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 2; ++e) acc[i][e] = acc[i][e] + a[i] * b[e];
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int a = a0 + ty * 2 + i;
    if (a >= ncol) continue;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int b = b0 + tx + 16 * e;
      if (b >= ncol) continue;
      work[(size_t)a * ld + b] = acc[i][e];
      if (gout) gout[(size_t)a * ncol + b] = acc[i][e];
      if (tr != tc) {  // the diagonal tiles compute both triangles themselves (a * b = b * a)
        work[(size_t)b * ld + a] = acc[i][e];
        if (gout) gout[(size_t)b * ncol + a] = acc[i][e];
      }
    }
  }
}

// One block: V = I (the caller zeroed it), the floor of the skip rule, the counters.
__global__ void __launch_bounds__(256) k_pca_jac_init(const double *__restrict__ a, double *__restrict__ v, int P,
                                                      int ncol, PcaState *__restrict__ state) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  double dmax = 0.0;
  for (int i = tid; i < P; i += 256) {
    v[(size_t)i * P + i] = 1.0;
    if (i < ncol) dmax = fmax(dmax, fabs(a[(size_t)i * P + i]));
  }
  red[tid] = dmax;
  __syncthreads();
  for (int d = 128; d > 0; d >>= 1) {
    if (tid < d) red[tid] = fmax(red[tid], red[tid + d]);  // a maximum: no order to keep
    __syncthreads();
  }
  if (tid == 0) state->floor = kEps * red[0];
  for (int i = tid; i < KS_PCA_MAX_SWEEPS; i += 256) state->rot[i] = 0;
}

struct Rot {
  double c, s, t;
  bool on;
};

// The rotation of pair (p < q) from the round's input matrix (the header's formulas).
__device__ __forceinline__ Rot pca_rot(const double *__restrict__ a, int P, int ncol, int p, int q, double floor) {
  Rot r{1.0, 0.0, 0.0, false};
  if (q >= ncol) return r;  // the dummy index's pair
  const double app = a[(size_t)p * P + p], aqq = a[(size_t)q * P + q], apq = a[(size_t)p * P + q];
  if (!(fabs(apq) > floor) || apq * apq <= (kEps * kEps) * fabs(app * aqq)) return r;
  const double theta = (aqq - app) / (2.0 * apq);
  double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
  if (theta < 0.0) t = -t;
  r.c = 1.0 / sqrt(t * t + 1.0);
  r.s = t * r.c;
  r.t = t;
  r.on = true;
  return r;
}

// Round `round` of sweep `sweep`: ain -> aout (both P x P, symmetric in bits), V in
// place.  Threads [0, H * H): the 2 x 2 block of pairs (k1, k2), k1 <= k2 only;
// threads [H * H, H * H + P * H): (row of V, pair).  H = P / 2.
__global__ void __launch_bounds__(256) k_pca_jac_round(const double *__restrict__ ain, double *__restrict__ aout,
                                                       double *__restrict__ v, int P, int ncol, int sweep, int round,
                                                       PcaState *__restrict__ state) {
  if (sweep > 0 && state->rot[sweep - 1] == 0) return;  // converged: nothing more is written
  const int H = P >> 1;
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x, na = (int64_t)H * H;
  const double floor = state->floor;
  if (gid < na) {
    const int k1 = (int)(gid / H), k2 = (int)(gid - (int64_t)k1 * H);
    if (k1 > k2) return;
    int p1, q1;
    pca_slot_pair(P, round, k1, &p1, &q1);
    const Rot r1 = pca_rot(ain, P, ncol, p1, q1, floor);
    if (k1 == k2) {
      const double app = ain[(size_t)p1 * P + p1], aqq = ain[(size_t)q1 * P + q1], apq = ain[(size_t)p1 * P + q1];
      if (r1.on) {
        atomicAdd(&state->rot[sweep], 1);
        aout[(size_t)p1 * P + p1] = app - r1.t * apq;
        aout[(size_t)q1 * P + q1] = aqq + r1.t * apq;
        aout[(size_t)p1 * P + q1] = 0.0;
        aout[(size_t)q1 * P + p1] = 0.0;
      } else {
        aout[(size_t)p1 * P + p1] = app;
        aout[(size_t)q1 * P + q1] = aqq;
        aout[(size_t)p1 * P + q1] = apq;
        aout[(size_t)q1 * P + p1] = apq;
      }
      return;
    }
    int p2, q2;
    pca_slot_pair(P, round, k2, &p2, &q2);
    const Rot r2 = pca_rot(ain, P, ncol, p2, q2, floor);
    const double x11 = ain[(size_t)p1 * P + p2], x12 = ain[(size_t)p1 * P + q2];
    const double x21 = ain[(size_t)q1 * P + p2], x22 = ain[(size_t)q1 * P + q2];
    double y11 = x11, y12 = x12, y21 = x21, y22 = x22;
    if (r1.on || r2.on) {
      // the column step of pair k2, then the row step of pair k1
      const double t11 = r2.c * x11 - r2.s * x12, t12 = r2.s * x11 + r2.c * x12;
      const double t21 = r2.c * x21 - r2.s * x22, t22 = r2.s * x21 + r2.c * x22;
      y11 = r1.c * t11 - r1.s * t21;
      y21 = r1.s * t11 + r1.c * t21;
      y12 = r1.c * t12 - r1.s * t22;
      y22 = r1.s * t12 + r1.c * t22;
    }
    aout[(size_t)p1 * P + p2] = y11;
    aout[(size_t)p2 * P + p1] = y11;
    aout[(size_t)p1 * P + q2] = y12;
    aout[(size_t)q2 * P + p1] = y12;
    aout[(size_t)q1 * P + p2] = y21;
    aout[(size_t)p2 * P + q1] = y21;
    aout[(size_t)q1 * P + q2] = y22;
    aout[(size_t)q2 * P + q1] = y22;
    return;
  }
  const int64_t g2 = gid - na;
  if (g2 >= (int64_t)P * H) return;
  const int i = (int)(g2 / H), k = (int)(g2 - (int64_t)i * H);
  int p, q;
  pca_slot_pair(P, round, k, &p, &q);
  const Rot r = pca_rot(ain, P, ncol, p, q, floor);
  if (!r.on) return;
  const double vp = v[(size_t)i * P + p], vq = v[(size_t)i * P + q];
  v[(size_t)i * P + p] = r.c * vp - r.s * vq;
  v[(size_t)i * P + q] = r.s * vp + r.c * vq;
}

// A thread per Jacobi column j: its place in the descending order, its sign, sdev
// and (place < ncomp) its column of rotation.
__global__ void __launch_bounds__(256) k_pca_finish(const double *__restrict__ a, const double *__restrict__ v, int P,
                                                    int ncol, int64_t m, int ncomp, double *__restrict__ sdev,
                                                    double *__restrict__ rotation) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= ncol) return;
  const double lam = a[(size_t)j * P + j];
  int place = 0;
  for (int i = 0; i < ncol; ++i) {
    const double li = a[(size_t)i * P + i];
    place += (li > lam || (li == lam && i < j)) ? 1 : 0;
  }
  sdev[place] = sqrt(fmax(lam, 0.0) / (double)(m - 1));
  if (place >= ncomp) return;
  double best = -1.0, at = 0.0;
  for (int c = 0; c < ncol; ++c) {
    const double x = v[(size_t)c * P + j];
    if (fabs(x) > best) best = fabs(x), at = x;  // strict: the lowest index among equals
  }
  const bool neg = at < 0.0;
  for (int c = 0; c < ncol; ++c) {
    const double x = v[(size_t)c * P + j];
    rotation[(size_t)c * ncomp + place] = neg ? -x : x;
  }
}

// x[r][j] = sum over c ascending of xc[r][c] * rotation[c][j].
__global__ void __launch_bounds__(256) k_pca_project(const double *__restrict__ panel, int64_t m, int ncol,
                                                     const double *__restrict__ rot, int ncomp, int tiles_j,
                                                     double *__restrict__ x) {
  __shared__ double As[kPK][kPT + 1];  // [c][row]: transposed on the way in
  __shared__ __attribute__((aligned(16))) double Bs[kPK][kPT];
  const int64_t ti = (int64_t)blockIdx.x / tiles_j;
  const int tj = (int)((int64_t)blockIdx.x - ti * tiles_j);
  const int64_t i0 = ti * kPT;
  const int j0 = tj * kPT;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  double acc[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[r][e] = 0.0;
  for (int k0 = 0; k0 < ncol; k0 += kPK) {
#pragma unroll
    for (int e = 0; e < kPK * kPT / 256; ++e) {
      const int idx = tid + 256 * e;
      const int ra = idx >> 4, ka = idx & 15;  // 16 consecutive columns of one panel row
      As[ka][ra] = (i0 + ra < m && k0 + ka < ncol) ? panel[(size_t)(i0 + ra) * ncol + k0 + ka] : 0.0;
      const int kb = idx >> 6, jb = idx & 63;
      Bs[kb][jb] = (k0 + kb < ncol && j0 + jb < ncomp) ? rot[(size_t)(k0 + kb) * ncomp + j0 + jb] : 0.0;
    }
    __syncthreads();
    // columns past ncol are staged as zeros: acc + 0 * 0 leaves acc's bits
#pragma unroll
    for (int kk = 0; kk < kPK; ++kk) {
      double a[4], b[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) a[r] = As[kk][ty * 4 + r];
#pragma unroll
      for (int e = 0; e < 4; ++e) b[e] = Bs[kk][tx + 16 * e];
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[r][e] = acc[r][e] + a[r] * b[e];
    }
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t i = i0 + ty * 4 + r;
    if (i >= m) continue;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int j = j0 + tx + 16 * e;
      if (j < ncomp) x[(size_t)i * ncomp + j] = acc[r][e];
    }
  }
}

ks_status check_pca_args(int64_t n, int32_t ncol, const void *rows, int64_t m, int32_t flags, int32_t ncomp) {
  KS_TRY(panel_check_count(m, 2, "a principal component analysis", "row", "m"));
  KS_TRY(panel_check_most(m, 0x7fffffffLL));
  KS_TRY(panel_check_ncol(ncol, KS_PCA_MAX_NCOL));
  if (ncomp < 1 || ncomp > ncol) return fail(KS_ERR_ARG, "ncomp must be between 1 and ncol = %d", (int)ncol);
  if (flags & ~KS_PCA_NO_CENTER) return fail(KS_ERR_ARG, "unknown pca flags 0x%x", (unsigned)flags);
  KS_TRY(panel_check_n(n));
  return panel_check_null_rows(rows, m, n, "rows", "m");
}

inline size_t pad16(size_t doubles) { return (doubles + 15) & ~(size_t)15; }

ks_status pca_impl(ks_ctx *ctx, const uint32_t *sp, int64_t n, int ncol, const int64_t *rows, int64_t m, int flags,
                   int ncomp, double *center, double *sdev, double *rotation, double *x, double *gram,
                   ks_pca_stats *stats) {
  hipStream_t st = ctx->stream;
  const int P = ncol + (ncol & 1), H = P / 2;
  const size_t panel_d = pad16((size_t)m * ncol), mat_d = pad16((size_t)P * P);
  const size_t work_bytes = (panel_d + 3 * mat_d) * 8 + sizeof(PcaState);
  DevFree mem;
  KS_TRY(dev_alloc(&mem, work_bytes, "the profile panel"));
  double *panel = static_cast<double *>(mem.p);
  double *a[2] = {panel + panel_d, panel + panel_d + mat_d};
  double *v = panel + panel_d + 2 * mat_d;
  PcaState *state = reinterpret_cast<PcaState *>(panel + panel_d + 3 * mat_d);

  // profiles; every index and every row sum is checked before any output is written
  KS_HIP(hipEventRecord(ctx->ev[0], st));
  KS_HIP(hipMemsetAsync(state, 0, sizeof(PcaState), st));
  KS_TRY(panel_normalise(ctx, sp, n, ncol, rows, m, PanelRoot::kNone, panel, nullptr, &state->bad[0], &state->bad[1]));
  unsigned long long hbad[2] = {0, 0};
  KS_HIP(hipMemcpyAsync(hbad, state->bad, 16, hipMemcpyDeviceToHost, st));
  KS_HIP(hipStreamSynchronize(st));
  KS_TRY(panel_report(hbad, 1, m, 0));

  if (flags & KS_PCA_NO_CENTER) {
    KS_HIP(hipMemsetAsync(center, 0, (size_t)ncol * 8, st));
  } else {
    hipLaunchKernelGGL(k_pca_center, dim3((unsigned)((ncol + kCC - 1) / kCC)), dim3(256), 0, st, panel, m, ncol,
                       center);
    KS_HIP(hipGetLastError());
    const int64_t total = m * ncol;
    const unsigned grid = (unsigned)std::min<int64_t>((total + 255) / 256, (int64_t)ctx->num_cus * 8);
    hipLaunchKernelGGL(k_pca_subtract, dim3(grid), dim3(256), 0, st, panel, total, ncol, center);
    KS_HIP(hipGetLastError());
  }
  KS_HIP(hipEventRecord(ctx->ev[1], st));

  // G into the first work matrix (P x P, zero padding) and the caller's, if any
  KS_HIP(hipMemsetAsync(a[0], 0, 3 * mat_d * 8, st));  // both work matrices and V
  {
    const int64_t tiles = (ncol + kGT - 1) / kGT;
    hipLaunchKernelGGL(k_pca_gram, dim3((unsigned)dist_tile_count(tiles)), dim3(256), 0, st, panel, m, ncol, tiles,
                       a[0], P, gram);
    KS_HIP(hipGetLastError());
  }
  KS_HIP(hipEventRecord(ctx->ev[2], st));

  // Jacobi: a launch per round; the counters come back once per few sweeps
  hipLaunchKernelGGL(k_pca_jac_init, dim3(1), dim3(256), 0, st, a[0], v, P, ncol, state);
  KS_HIP(hipGetLastError());
  const int64_t threads = (int64_t)H * H + (int64_t)P * H;
  const unsigned jgrid = (unsigned)((threads + 255) / 256);
  int queued = 0, n_sweeps = 0, cur = 0;
  int64_t n_rot = 0;
  int hrot[KS_PCA_MAX_SWEEPS];
  while (n_sweeps == 0) {
    if (queued == KS_PCA_MAX_SWEEPS)
      return fail(KS_ERR_INTERNAL, "the Jacobi iteration did not end within %d sweeps", KS_PCA_MAX_SWEEPS);
    // small matrices end in 5 to 8 sweeps, larger ones in 9 or more: the first batch stays below that
    const int batch = std::min(queued == 0 ? (P <= 32 ? 4 : 6) : 2, KS_PCA_MAX_SWEEPS - queued);
    for (int s = queued; s < queued + batch; ++s)
      for (int r = 0; r < P - 1; ++r) {
        hipLaunchKernelGGL(k_pca_jac_round, dim3(jgrid), dim3(256), 0, st, a[cur], a[cur ^ 1], v, P, ncol, s, r, state);
        cur ^= 1;
      }
    KS_HIP(hipGetLastError());
    queued += batch;
    KS_HIP(hipMemcpyAsync(hrot, state->rot, sizeof(hrot), hipMemcpyDeviceToHost, st));
    KS_HIP(hipStreamSynchronize(st));
    for (int s = 0; s < queued; ++s)
      if (hrot[s] == 0) {
        n_sweeps = s + 1;  // the sweep that rotated nothing ran too (and copied the matrix along)
        break;
      }
  }
  for (int s = 0; s < n_sweeps; ++s) n_rot += hrot[s];
  // n_sweeps * (P - 1) rounds ran, P - 1 is odd: the result is in buffer n_sweeps & 1
  const double *afin = a[n_sweeps & 1];
  hipLaunchKernelGGL(k_pca_finish, dim3((unsigned)((ncol + 255) / 256)), dim3(256), 0, st, afin, v, P, ncol, m, ncomp,
                     sdev, rotation);
  KS_HIP(hipGetLastError());
  KS_HIP(hipEventRecord(ctx->ev[3], st));

  if (x) {
    const int tiles_j = (ncomp + kPT - 1) / kPT;
    const int64_t grid = ((m + kPT - 1) / kPT) * tiles_j;
    hipLaunchKernelGGL(k_pca_project, dim3((unsigned)grid), dim3(256), 0, st, panel, m, ncol, rotation, ncomp, tiles_j,
                       x);
    KS_HIP(hipGetLastError());
  }
  KS_HIP(hipEventRecord(ctx->ev[4], st));
  KS_HIP(hipStreamSynchronize(st));  // the work memory is freed on return
  if (stats) {
    KS_TRY(event_ms(ctx, 0, 4, &stats->ms_total));
    KS_TRY(event_ms(ctx, 0, 1, &stats->ms_normalise));
    KS_TRY(event_ms(ctx, 1, 2, &stats->ms_gram));
    KS_TRY(event_ms(ctx, 2, 3, &stats->ms_eigen));
    KS_TRY(event_ms(ctx, 3, 4, &stats->ms_project));
    stats->n_sweeps = n_sweeps;
    stats->n_rotations = n_rot;
    stats->panel_bytes = (int64_t)work_bytes;
  }
  return KS_OK;
}

}  // namespace
}  // namespace ks

using namespace ks;

extern "C" ks_status ks_spectra_pca_dev(ks_ctx *ctx, const uint32_t *spectra_dev, int64_t n, int32_t ncol,
                                        const int64_t *rows_dev, int64_t m, int32_t flags, int32_t ncomp,
                                        double *center_dev, double *sdev_dev, double *rotation_dev, double *x_dev,
                                        double *gram_dev, ks_pca_stats *stats) {
  if (stats) memset(stats, 0, sizeof(*stats));
  KS_TRY(check_pca_args(n, ncol, rows_dev, m, flags, ncomp));
  if (!spectra_dev) return fail(KS_ERR_ARG, "null spectra");
  if (!center_dev || !sdev_dev || !rotation_dev) return fail(KS_ERR_ARG, "null output");
  KS_TRY(default_ctx(&ctx));
  KS_ENTER(ctx);
  return pca_impl(ctx, spectra_dev, n, ncol, rows_dev, m, flags, ncomp, center_dev, sdev_dev, rotation_dev, x_dev,
                  gram_dev, stats);
}

extern "C" ks_status ks_spectra_pca(ks_ctx *ctx, const uint32_t *spectra, int64_t n, int32_t ncol, const int64_t *rows,
                                    int64_t m, int32_t flags, int32_t ncomp, double *center, double *sdev,
                                    double *rotation, double *x, double *gram) {
  KS_TRY(check_pca_args(n, ncol, rows, m, flags, ncomp));
  if (!spectra) return fail(KS_ERR_ARG, "null spectra");
  if (!center || !sdev || !rotation) return fail(KS_ERR_ARG, "null output");
  KS_TRY(panel_check_rows_host(spectra, n, ncol, rows, m, nullptr, 0));
  KS_TRY(default_ctx(&ctx));
  KS_ENTER(ctx);
  const HostEnd host_end{ctx};  // (ks_set_host_cache)
  // outputs in one block: center | sdev | rotation | x | G
  const size_t o_sdev = (size_t)ncol, o_rot = 2 * (size_t)ncol, o_x = o_rot + (size_t)ncol * ncomp;
  const size_t o_g = o_x + (x ? (size_t)m * ncomp : 0), o_end = o_g + (gram ? (size_t)ncol * ncol : 0);
  void *d_out = nullptr;
  KS_TRY(ensure(ctx, SLOT_REG_TMP, o_end * 8, &d_out));
  SpectraUpload up;
  KS_TRY(upload_spectra(ctx, spectra, n, ncol, rows, m, nullptr, 0, 0, &up));
  hipStream_t st = ctx->stream;
  double *o = static_cast<double *>(d_out);
  KS_TRY(pca_impl(ctx, up.sp, n, ncol, up.rows, m, flags, ncomp, o, o + o_sdev, o + o_rot, x ? o + o_x : nullptr,
                  gram ? o + o_g : nullptr, nullptr));
  KS_HIP(hipMemcpyAsync(center, o, (size_t)ncol * 8, hipMemcpyDeviceToHost, st));
  KS_HIP(hipMemcpyAsync(sdev, o + o_sdev, (size_t)ncol * 8, hipMemcpyDeviceToHost, st));
  KS_HIP(hipMemcpyAsync(rotation, o + o_rot, (size_t)ncol * ncomp * 8, hipMemcpyDeviceToHost, st));
  if (x) KS_HIP(hipMemcpyAsync(x, o + o_x, (size_t)m * ncomp * 8, hipMemcpyDeviceToHost, st));
  if (gram) KS_HIP(hipMemcpyAsync(gram, o + o_g, (size_t)ncol * ncol * 8, hipMemcpyDeviceToHost, st));
  KS_HIP(hipStreamSynchronize(st));
  return KS_OK;
}

// The round-robin schedule on the host (tests walk it): the pairs of round
// `round` (0 .. P - 2) in slot order, the dummy index's pair left out.
extern "C" int32_t ks_pca_round_pairs(int32_t ncol, int32_t round, int32_t *p, int32_t *q) {
  if (ncol < 1 || ncol > KS_PCA_MAX_NCOL || !p || !q) return -1;
  const int P = ncol + (ncol & 1);
  if (round < 0 || round >= P - 1) return -1;
  int cnt = 0;
  for (int i = 0; i < P / 2; ++i) {
    int a, b;
    pca_slot_pair(P, round, i, &a, &b);
    if (b >= ncol) continue;
    p[cnt] = a;
    q[cnt] = b;
    ++cnt;
  }
  return cnt;
}
