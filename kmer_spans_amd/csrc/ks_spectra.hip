// ks_spectra.hip -- per-region q-mer spectra and Shannon entropy
// (ks_region_spectra / ks_region_spectra_dev, include/kmer_spans.h).
//
// What the reference's author does with the regions next (test.R:703-720):
// cut every region out with subseq(seq[pos[,1]+1], pos[,2], pos[,3]), count
// its tetramers on both strands, then -sum(p * log2(p)) per region.  Here the
// genome stays in HBM; the input is the region list (seq_id 0-based, beg..end
// 1-based inclusive, the numbers ks_scan_dev returns), the output one row of
// 4^q uint32 counts per region (internal A,C,T,G code order, first base most
// significant) and one FP64 entropy per region.
//
// Every window of q bytes wholly inside the interval and free of N/n counts
// once; there are no end-of-run quirks (Q1 and Q5 belong to the scan).
// Biostrings' oligonucleotideFrequency skips windows holding any non-ACGT
// letter; only N/n is skipped here, every other byte is coded (c >> 1) & 3.
//
// Plan:    k_spectra_plan validates the intervals and counts their tiles of
//          kTile word starts (at least one, so every row has a writer), an
//          exclusive scan gives the work list.  One scalar read-back (the
//          first bad interval, the tile total) ends a call with a bad interval
//          before anything touches the output, and sizes the count grid;
//          k_spectra_clear then zeroes the rows more than one tile adds to.
// Count:   a wave takes a contiguous block of the tile list and keeps one
//          histogram in its own LDS for as long as the interval stays the
//          same.  Lanes take contiguous stretches of a tile (q - 1 bytes of
//          look-ahead), read 16 bytes at a time where the aligned chunk lies
//          inside the sequence, and hold the last two distinct codes with run
//          lengths in registers, so a homopolymer or a dinucleotide repeat
//          costs two LDS adds per lane and tile instead of 64 lanes queueing
//          on one LDS address for every base.  At an interval change the row
//          leaves the LDS: plain coalesced stores (zeros included) where the
//          interval is a single tile, atomic adds of the non-zero bins where
//          several tiles share it.  The two-strand fold h[c] + h[rc(c)] is
//          applied here: it is linear, so it commutes with the cross-wave sum.
// Entropy: one wave per row sums T, then -sum p log2 p (device log2; a new
//          quantity with a tolerance, not reference bits).
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstring>

#include "ks_internal.h"

namespace ks {
namespace {

constexpr int kTile = 4096;       // word starts per work tile
constexpr int kSpThreads = 256;   // 4 waves, one LDS histogram each (64 KiB per block at q = 6)
constexpr int kSpWaves = kSpThreads / 64;
static_assert(kTile % 64 == 0, "lanes share a tile evenly");

// plan scalars (u64 words at the head of the work buffer)
constexpr int kSpBad = 0;    // n - (first bad interval), 0 = none
constexpr int kSpBases = 1;  // sum of widths
constexpr int kSpWords = 2;  // single-strand words counted
constexpr int kSpScalars = 8;

// LDS operations of one wave execute in order; this keeps the compiler from
// moving them across the point where lanes read what other lanes wrote.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

// Reverse complement of a q-digit code: the complement is digit ^ 2.
__device__ __forceinline__ uint32_t rc_code(uint32_t c, int q) {
  uint32_t r = __brev(c) >> (32 - 2 * q);  // digits reversed, and the two bits of each digit
  r = ((r & 0xAAAAAAAAu) >> 1) | ((r & 0x55555555u) << 1);  // the bits of each digit back in place
  return r ^ (0xAAAAAAAAu & ((1u << (2 * q)) - 1u));
}

__global__ void __launch_bounds__(256) k_spectra_plan(const int64_t *__restrict__ offs, int32_t nseq,
                                                      const int32_t *__restrict__ sid, const int32_t *__restrict__ beg,
                                                      const int32_t *__restrict__ end, int64_t n,
                                                      int64_t *__restrict__ ntile, unsigned long long *__restrict__ sc) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  long long width = 0;
  if (i < n) {
    const int32_t s = sid[i];
    const int64_t b = beg[i], e = end[i];
    bool ok = s >= 0 && s < nseq && b >= 1 && e >= b - 1;
    if (ok) ok = e <= offs[s + 1] - offs[s];
    if (!ok) atomicMax(&sc[kSpBad], (unsigned long long)(n - i));
    width = ok ? e - b + 1 : 0;
    ntile[i] = max((long long)1, (width + kTile - 1) / kTile);
  } else if (i == n) {
    ntile[n] = 0;
  }
  for (int d = 32; d > 0; d >>= 1) width += __shfl_down(width, d);
  if ((threadIdx.x & 63) == 0 && width) atomicAdd(&sc[kSpBases], (unsigned long long)width);
}

// Rows that several tiles add to start at zero (single-tile rows are written whole).
__global__ void __launch_bounds__(256) k_spectra_clear(const int64_t *__restrict__ tb, int64_t n, int nbins,
                                                       uint32_t *__restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t nw = (int64_t)gridDim.x * (blockDim.x >> 6);
  for (int64_t i = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); i < n; i += nw) {
    if (tb[i + 1] - tb[i] <= 1) continue;
    uint32_t *row = out + (size_t)i * nbins;
    for (int c = lane; c < nbins; c += 64) row[c] = 0;
  }
}

// One lane's stretch: the len bytes from absolute position p0 (all inside the
// interval); every N-free window of q of them is a word.  [slo, shi) is the
// sequence: an aligned 16-byte chunk is read whole only when it lies inside.
__device__ __forceinline__ void lane_count(const uint8_t *__restrict__ seq, int64_t p0, int len, int64_t slo,
                                           int64_t shi, int q, uint32_t mask, uint32_t *h, uint32_t &nw) {
  uint32_t code = 0, c0 = 0xffffffffu, c1 = 0xffffffffu, n0 = 0, n1 = 0;
  int run = 0;  // N-free bytes behind the current one, itself included (saturates at q)
  const int64_t pe = p0 + len;
  for (int64_t cb = p0 & ~(int64_t)15; cb < pe; cb += 16) {
    uint32_t w[4] = {0, 0, 0, 0};
    if (cb >= slo && cb + 16 <= shi) {
      const uint4 v = *reinterpret_cast<const uint4 *>(seq + cb);
      w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
    } else {
#pragma unroll
      for (int b = 0; b < 16; ++b) {
        const int64_t p = cb + b;
        if (p >= p0 && p < pe) w[b >> 2] |= (uint32_t)seq[p] << (8 * (b & 3));
      }
    }
    const int rel = (int)(cb - p0);  // -15 .. len - 1
#pragma unroll
    for (int b = 0; b < 16; ++b) {
      const uint8_t c = (uint8_t)(w[b >> 2] >> (8 * (b & 3)));
      if (rel + b >= 0 && rel + b < len) {
        run = is_n(c) ? 0 : min(run + 1, q);
        code = ((code << 2) | enc(c)) & mask;
        if (run >= q) {
          ++nw;
#ifdef KS_SPECTRA_NO_RLE  // comparison build (tools/spectra_bench.py --contended-only)
          atomicAdd(&h[code], 1u);
          continue;
#endif
          if (code == c0) {
            ++n0;
          } else if (code == c1) {
            ++n1;
          } else {
            if (n1) atomicAdd(&h[c1], n1);
            c1 = c0, n1 = n0;
            c0 = code, n0 = 1;
          }
        }
      }
    }
  }
  if (n0) atomicAdd(&h[c0], n0);
  if (n1) atomicAdd(&h[c1], n1);
}

__global__ void __launch_bounds__(kSpThreads) k_spectra_count(
    const uint8_t *__restrict__ seq, const int64_t *__restrict__ offs, const int32_t *__restrict__ sid,
    const int32_t *__restrict__ beg, const int32_t *__restrict__ end, const int64_t *__restrict__ tb, int64_t n,
    int64_t per_wave, int q, int both, uint32_t *__restrict__ out, unsigned long long *__restrict__ sc) {
  extern __shared__ __attribute__((aligned(16))) uint32_t sp_lds[];  // [kSpWaves][4^q]
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int nbins = 1 << (2 * q);
  const uint32_t mask = (uint32_t)nbins - 1u;
  uint32_t *h = sp_lds + wv * nbins;
  for (int c = lane; c < nbins; c += 64) h[c] = 0;
  wave_sync();
  const int64_t total = tb[n];
  int64_t t = ((int64_t)blockIdx.x * kSpWaves + wv) * per_wave;
  const int64_t t1 = min(t + per_wave, total);
  if (t >= t1) return;
  int64_t lo = 0, hi = n - 1;  // the interval of tile t: the last i with tb[i] <= t (every interval has a tile)
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (tb[mid] <= t) lo = mid; else hi = mid - 1;
  }
  uint32_t nw = 0;
  unsigned long long words = 0;
  for (int64_t i = lo; t < t1; ++i) {
    const int64_t tbi = tb[i], tbn = tb[i + 1];
    const int64_t tend = min(tbn, t1);
    const int32_t s = sid[i];
    const int64_t slo = offs[s], shi = offs[s + 1];
    const int64_t b = beg[i];
    const int64_t a0 = slo + b - 1;                           // the interval's first byte
    const int64_t nstart = (int64_t)end[i] - b + 1 - q + 1;   // word starts in the interval (<= 0: none)
    for (; t < tend; ++t) {
      const int64_t r0 = (t - tbi) * kTile;
      const int64_t r1 = min(r0 + kTile, nstart);
      if (r1 <= r0) continue;
      const int ns = (int)(r1 - r0);
      const int L = (ns + 63) >> 6;
      const int la = lane * L, lb = min(la + L, ns);
      if (la < lb) lane_count(seq, a0 + r0 + la, lb - la + q - 1, slo, shi, q, mask, h, nw);
      words += nw;
      nw = 0;
    }
    wave_sync();
    uint32_t *row = out + (size_t)i * nbins;
    const bool shared = tbn - tbi > 1;
    for (int c = lane; c < nbins; c += 64) {
      uint32_t v = h[c];
      if (both) v += h[rc_code((uint32_t)c, q)];
      if (!shared) row[c] = v;
      else if (v) atomicAdd(&row[c], v);
    }
    wave_sync();
    for (int c = lane; c < nbins; c += 64) h[c] = 0;
    wave_sync();
  }
  for (int d = 32; d > 0; d >>= 1) words += __shfl_down(words, d);
  if (lane == 0 && words) atomicAdd(&sc[kSpWords], words);
}

// H = -sum p log2 p over the non-zero bins of a row, p = row[c] / T; NaN when T = 0.
__global__ void __launch_bounds__(256) k_spectra_entropy(const uint32_t *__restrict__ sp, int64_t n, int nbins,
                                                         double *__restrict__ ent) {
  const int lane = threadIdx.x & 63;
  const int64_t nw = (int64_t)gridDim.x * (blockDim.x >> 6);
  for (int64_t i = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); i < n; i += nw) {
    const uint32_t *row = sp + (size_t)i * nbins;
    double tot = 0.0;  // integers below 2^44: exact in any order
    for (int c = lane; c < nbins; c += 64) tot += (double)row[c];
    for (int d = 32; d > 0; d >>= 1) tot += __shfl_xor(tot, d);
    double hsum = 0.0;
    for (int c = lane; c < nbins; c += 64) {
      const uint32_t v = row[c];
      if (v) {
        const double p = (double)v / tot;
        hsum += -(p * log2(p));
      }
    }
    for (int d = 32; d > 0; d >>= 1) hsum += __shfl_xor(hsum, d);
    if (lane == 0) ent[i] = tot > 0.0 ? hsum : __longlong_as_double(0x7ff8000000000000LL);
  }
}

ks_status check_spectra_args(int64_t n, int32_t q, int32_t flags) {
  if (q < 1 || q > KS_SPECTRA_MAX_Q) return fail(KS_ERR_ARG, "q must be between 1 and %d", KS_SPECTRA_MAX_Q);
  if (flags & ~KS_SPECTRA_BOTH_STRANDS) return fail(KS_ERR_ARG, "unknown spectra flags 0x%x", (unsigned)flags);
  if (n < 0) return fail(KS_ERR_ARG, "the number of intervals must not be negative");
  if (n >= INT32_MAX) return fail(KS_ERR_ARG, "too many intervals");
  return KS_OK;
}

ks_status spectra_impl(ks_ctx *ctx, const ks_dev_seqs *s, const int32_t *sid, const int32_t *beg, const int32_t *end,
                       int64_t n, int q, int flags, uint32_t *out, double *ent, ks_spectra_stats *stats) {
  hipStream_t st = ctx->stream;
  const int nbins = 1 << (2 * q);
  void *w = nullptr;
  KS_TRY(ensure(ctx, SLOT_WORK_A, (size_t)kSpScalars * 8 + 2 * ((size_t)n + 1) * 8, &w));
  unsigned long long *sc = static_cast<unsigned long long *>(w);
  int64_t *ntile = reinterpret_cast<int64_t *>(sc + kSpScalars);
  int64_t *tb = ntile + n + 1;
  size_t tmp_bytes = 0;
  KS_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, ntile, tb, (int)(n + 1), st));
  void *tmp = nullptr;
  KS_TRY(ensure(ctx, SLOT_SORT_TMP, tmp_bytes + 16, &tmp));

  KS_HIP(hipEventRecord(ctx->ev[0], st));
  KS_HIP(hipMemsetAsync(sc, 0, kSpScalars * 8, st));
  hipLaunchKernelGGL(k_spectra_plan, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, st, s->offsets_dev, s->nseq,
                     sid, beg, end, n, ntile, sc);
  KS_HIP(hipGetLastError());
  KS_HIP(hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, ntile, tb, (int)(n + 1), st));
  KS_HIP(hipEventRecord(ctx->ev[1], st));
  unsigned long long hsc[2] = {0, 0};
  int64_t tiles = 0;
  KS_HIP(hipMemcpyAsync(hsc, sc, sizeof(hsc), hipMemcpyDeviceToHost, st));
  KS_HIP(hipMemcpyAsync(&tiles, tb + n, 8, hipMemcpyDeviceToHost, st));
  KS_HIP(hipStreamSynchronize(st));
  if (hsc[kSpBad] != 0)  // nothing has touched the output, and no kernel sees an unchecked interval
    return fail(KS_ERR_ARG, "interval %lld out of range", (long long)(n - (int64_t)hsc[kSpBad]));
  const unsigned row_grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 3) / 4, (int64_t)ctx->num_cus * 32));
  hipLaunchKernelGGL(k_spectra_clear, dim3(row_grid), dim3(256), 0, st, tb, n, nbins, out);
  KS_HIP(hipGetLastError());

  // Waves take contiguous blocks of the tile list; enough waves to fill the
  // device (the LDS bounds the blocks per CU: 160 KiB / (4 x 4^q x 4 B)).
  const size_t lds = (size_t)kSpWaves * nbins * 4;
  const int64_t blocks_per_cu = std::max<int64_t>(1, std::min<int64_t>(8, (160 * 1024) / (int64_t)lds));
  const int64_t max_waves = (int64_t)ctx->num_cus * blocks_per_cu * kSpWaves;
  const int64_t per_wave = std::max<int64_t>(1, (tiles + max_waves - 1) / max_waves);
  const int64_t waves = (tiles + per_wave - 1) / per_wave;
  const unsigned grid = (unsigned)((waves + kSpWaves - 1) / kSpWaves);
  hipLaunchKernelGGL(k_spectra_count, dim3(grid), dim3(kSpThreads), lds, st, s->seq, s->offsets_dev, sid, beg, end, tb,
                     n, per_wave, q, (flags & KS_SPECTRA_BOTH_STRANDS) ? 1 : 0, out, sc);
  KS_HIP(hipGetLastError());
  KS_HIP(hipEventRecord(ctx->ev[2], st));
  if (ent) {
    hipLaunchKernelGGL(k_spectra_entropy, dim3(row_grid), dim3(256), 0, st, out, n, nbins, ent);
    KS_HIP(hipGetLastError());
  }
  KS_HIP(hipEventRecord(ctx->ev[3], st));
  unsigned long long words = 0;
  KS_HIP(hipMemcpyAsync(&words, sc + kSpWords, 8, hipMemcpyDeviceToHost, st));
  KS_HIP(hipStreamSynchronize(st));
  if (stats) {
    float ms = 0;
    KS_HIP(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[3]));
    stats->ms_total = ms;
    KS_HIP(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
    stats->ms_plan = ms;
    KS_HIP(hipEventElapsedTime(&ms, ctx->ev[1], ctx->ev[2]));
    stats->ms_count = ms;
    KS_HIP(hipEventElapsedTime(&ms, ctx->ev[2], ctx->ev[3]));
    stats->ms_entropy = ms;
    stats->n_regions = n;
    stats->n_bases = (int64_t)hsc[kSpBases];
    stats->n_words = (int64_t)words;
    stats->n_tiles = tiles;
  }
  return KS_OK;
}

}  // namespace
}  // namespace ks

using namespace ks;

extern "C" int32_t ks_spectra_tile_bases(void) { return kTile; }

extern "C" ks_status ks_region_spectra_dev(ks_ctx *ctx, const ks_dev_seqs *s, const int32_t *seq_id_dev,
                                           const int32_t *beg_dev, const int32_t *end_dev, int64_t n, int32_t q,
                                           int32_t flags, uint32_t *spectra_dev, double *entropy_dev,
                                           ks_spectra_stats *stats) {
  if (stats) memset(stats, 0, sizeof(*stats));
  KS_TRY(check_spectra_args(n, q, flags));
  if (n == 0) return KS_OK;
  KS_TRY(check_dev_seqs(s));
  if (!seq_id_dev || !beg_dev || !end_dev) return fail(KS_ERR_ARG, "null interval array");
  if (!spectra_dev) return fail(KS_ERR_ARG, "null output");
  KS_TRY(default_ctx(&ctx));
  KS_ENTER(ctx);
  return spectra_impl(ctx, s, seq_id_dev, beg_dev, end_dev, n, q, flags, spectra_dev, entropy_dev, stats);
}

extern "C" ks_status ks_region_spectra(ks_ctx *ctx, const char *const *seqs, const int64_t *lens, int32_t nseq,
                                       const int32_t *seq_id, const int32_t *beg, const int32_t *end, int64_t n,
                                       int32_t q, int32_t flags, uint32_t *spectra, double *entropy) {
  KS_TRY(check_spectra_args(n, q, flags));
  if (n == 0) return KS_OK;
  KS_TRY(check_seqs(seqs, lens, nseq));
  if (!seq_id || !beg || !end) return fail(KS_ERR_ARG, "null interval array");
  if (!spectra) return fail(KS_ERR_ARG, "null output");
  for (int64_t i = 0; i < n; ++i) {
    const int32_t sq = seq_id[i];
    if (sq < 0 || sq >= nseq || beg[i] < 1 || (int64_t)end[i] < (int64_t)beg[i] - 1 || end[i] > lens[sq])
      return fail(KS_ERR_ARG, "interval %lld out of range", (long long)i);
  }
  KS_TRY(default_ctx(&ctx));
  KS_ENTER(ctx);
  const HostEnd host_end{ctx};  // (ks_set_host_cache)
  Staged st;
  KS_TRY(stage(ctx, seqs, lens, nseq, &st));
  const size_t nbins = (size_t)1 << (2 * q);
  void *d_iv = nullptr, *d_sp = nullptr, *d_ent = nullptr;
  KS_TRY(ensure(ctx, SLOT_REGIONS, 3 * (size_t)n * 4, &d_iv));
  KS_TRY(ensure(ctx, SLOT_COUNTS, (size_t)n * nbins * 4, &d_sp));
  if (entropy) KS_TRY(ensure(ctx, SLOT_REG_TMP, (size_t)n * 8, &d_ent));
  int32_t *d_sid = static_cast<int32_t *>(d_iv), *d_beg = d_sid + n, *d_end = d_beg + n;
  KS_HIP(hipMemcpyAsync(d_sid, seq_id, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
  KS_HIP(hipMemcpyAsync(d_beg, beg, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
  KS_HIP(hipMemcpyAsync(d_end, end, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
  KS_TRY(spectra_impl(ctx, &st.dev, d_sid, d_beg, d_end, n, q, flags, static_cast<uint32_t *>(d_sp),
                      static_cast<double *>(d_ent), nullptr));
  KS_HIP(hipMemcpyAsync(spectra, d_sp, (size_t)n * nbins * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (entropy) KS_HIP(hipMemcpyAsync(entropy, d_ent, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
  KS_HIP(hipStreamSynchronize(ctx->stream));
  return KS_OK;
}
