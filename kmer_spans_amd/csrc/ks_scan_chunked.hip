// ks_scan_chunked.hip -- chunked carry scan (algo 1): the span scan with
// parallelism inside runs, bit-exact with the sequential reference.
//
// The sequential state machine of kmer_regions (kmer_spans.c:243-307) is
// decomposed (SURVEY 8(a) a5', verified by oracle/pyoracle.py):
//   T_i = max(fl(T_{i-1} + s_i), 0) over each run's scan indices [a+k, b-1];
//   excursions = maximal stretches with T > 0 (beg, first argmax, max, end);
//   an emitted excursion adds a region and a fresh rescan of (argmax, end].
// Every run is cut into chunks of CH = 256 scan indices, one lane each.
//
//  P1 (gather pass, the only random-access pass): codes -> table values;
//     clean-entry trajectory C_j (entry 0) of every chunk: exit value, the
//     open trailing excursion, closed emittable excursions ("candidates");
//     approximate aggregates (sum, min/max prefix); compressed tables also
//     store each index's uint16 table code so later passes stream 2 B/index.
//  P2 approximate max-plus scan of (sum, clean exit) per run -> predicted
//     entry x~_j; where x~_j puts the whole chunk inside one binade
//     [2^e, 2^(e+1)) far from 0, the chunk's binade-integer summary is built:
//     with S = m * 2^(e-52), fl(S + s) = S + RN(s / 2^(e-52)) exactly, ties to
//     even decided by the parity of m, so a chunk is an integer map
//     m -> m + D[parity(m)] with max/argmax/min per entry parity.
//  P3 exact carry per run (sequential over chunks, O(1) per chunk):
//     entry 0 -> exit C_j exactly;  summary valid for the exact entry ->
//     integer arithmetic;  x + minprefix < -margin -> the true trajectory
//     clamps in the chunk and then coincides with C_j (monotone rounding),
//     so the exit is C_j exactly;  otherwise exact replay of the chunk.
//  P4 heads: per chunk with positive exact entry, the part of the carried
//     excursion before its first clamp (replay, or the summary).
//  P5 stitch per run: excursions from heads, tails and candidates; emit
//     regions + rescan ranges; rescans run on the lane kernel.
#include <hip/hip_fp16.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstring>
#include <type_traits>
#include <vector>

#include "ks_scan_common.h"

namespace ks {

ks_status launch_scan_lane(ks_ctx *ctx, const uint8_t *seq, int64_t total, const int64_t *ra, const int64_t *rb,
                           const int32_t *rs, int64_t n, int k, const TableView &tv, uint64_t mw,
                           double min_score, uint32_t *visits, const RegionBuf &out,
                           const unsigned long long *d_cnt = nullptr, int64_t segcap = 0,
                           const ScanMode &mode = ScanMode(), int init_step = 1, const int64_t *offs = nullptr,
                           const uint32_t *packed = nullptr, hipStream_t strm = nullptr);

namespace {

constexpr int CH = 256;  // scan indices per chunk (one lane)
constexpr int NB = 16;   // indices per gather batch
constexpr int kModeClean = 0, kModeL = 1, kModeR = 2, kModeU = 3;

struct Chunks {
  int64_t *start;  // first scan index (global position)
  int32_t *n;      // indices in the chunk
  int32_t *run;    // run id
  int64_t nch;     // chunks [c0, nch) are this launch's (a half of the runs, see scan_chunked)
  const uint32_t *packed;  // 2-bit base codes (Runs::packed), nullptr: roll the bytes
  int64_t c0 = 0;
};

struct P1 {  // per-chunk results of the gather pass
  double *cexit, *asum, *pmin, *pmax, *sabs, *tmax;
  int32_t *tbeg, *targ;  // trailing open excursion (relative), tbeg = -1: none
  uint8_t *special;      // a non-finite value occurred
  int32_t *parg;         // first index of the prefix maximum pmax
  // epoch guard: pass 1 stamps every chunk it wrote with this call's epoch
  // (ks_ctx::scan_epoch); the stitch checks the stamp of every chunk whose
  // pass-1 results it reads (error bit 32: results of another call)
  uint32_t *ep = nullptr;
  uint32_t epoch = 0;
};

struct Summ {  // binade-integer summaries for the predicted binade (P2)
  int32_t *e;             // binade, INT32_MIN: none
  long long *D, *M, *N;   // [2 * nch] by entry parity
  int32_t *A;             // [2 * nch]
  // pass-1 summaries (p1summ): sel[c] < 2 = the chunk's summary is pass 1's
  // slot 2c + sel[c] of pD..pA for both entry parities (k_marks_select keeps
  // it in place instead of copying it into D..A); 2 = D..A.  sel null: D..A.
  uint8_t *sel = nullptr;
  const long long *pD = nullptr, *pM = nullptr, *pN = nullptr;
  const int32_t *pA = nullptr;
};

// Where chunk c's summary fields are: index i0 (entry parity 0) and i1
// (parity 1) into D / M / N / A.
struct SummAt {
  const long long *D, *M, *N;
  const int32_t *A;
  int64_t i0, i1;
};
__device__ __forceinline__ SummAt summ_at(const Summ &sm, int64_t c) {
  if (sm.sel) {
    const int s = sm.sel[c];
    if (s < 2) return SummAt{sm.pD, sm.pM, sm.pN, sm.pA, 2 * c + s, 2 * c + s};
  }
  return SummAt{sm.D, sm.M, sm.N, sm.A, 2 * c, 2 * c + 1};
}

struct SummP1 {  // binade summaries computed by pass 1 for the predicted binade (single trajectory)
  int32_t *e;             // [2 * nch] binade, INT32_MIN: none (no prediction, a tie, out of range)
  long long *D, *M, *N;   // [2 * nch] total, max, min (units 2^(e-52))
  int32_t *A;             // [2 * nch] first argmax
};

// A pass-1 summary of chunk c in binade e (slot t of the predicted binade and
// its neighbour): the binade-integer map of the chunk (D, M, N, A as
// chunk_summary_impl) from the steps r = (s + 1.5 * 2^e) - 1.5 * 2^e summed
// in FP64.  Valid if no step was a tie (bad), every |s| < 2^(e-1) (so the
// magic constant rounds s to the ulp 2^(e-52)) and every partial sum of the
// r inside (-2^e, 2^e) (so the sums are exact multiples of the ulp): then D,
// the maximum M and the minimum N are the integer trajectory's, exactly.
// (Until round 5 every partial sum of |s| had to stay below 2^(e-1) and N was
// a lower bound from the FP64 prefix minimum minus a 130-ulp margin; the
// exact form measured the same: metric step 14.59 vs 14.72 ms, weighted rank
// k = 15 61.9 vs 61.7 ms, profiles/r5/ab/ab_p1summ_exact*.txt)
__device__ __forceinline__ void summ_put(const SummP1 &sp, int64_t c, int t, int e, bool bad, double maxabs,
                                         double cur, double mx, double mn, int a) {
  const double lim = ldexp(1.0, e);
  // (a NaN step leaves cur NaN; fmin / fmax skip it in mn, mx, maxabs)
  const bool ok = e != INT32_MIN && !bad && cur == cur && maxabs < 0.5 * lim && mn <= mx && mx < lim && mn > -lim;
  sp.e[2 * c + t] = ok ? e : INT32_MIN;
  if (ok) {
    const double sc = ldexp(1.0, 52 - e);
    sp.D[2 * c + t] = (long long)(cur * sc);
    sp.M[2 * c + t] = (long long)(mx * sc);
    sp.N[2 * c + t] = (long long)(mn * sc);
    sp.A[2 * c + t] = a;
  }
}                        // slot 2c: the predicted binade, 2c + 1: its neighbour near an edge

struct Carry {  // P3/P4
  double *x;      // exact entry value
  uint8_t *mode;
  int32_t *hq;    // first clamp in the chunk (relative), -1 none
  double *hmax;   // max of the carried head (valid if the head is non-empty)
  int32_t *harg;
};

// Composites of the global 64-chunk tiles (chunks [64t, 64t + 64)) for the
// carry's tile batches: k_tile_comp writes, per tile whose chunks all have a
// summary in one binade e, the composed increment D_p of the tile and the
// interval [LO_p, HI_p] of entry mantissas (parity p) for which every
// chunk's trajectory stays inside the binade -- exactly the fast-tile test
// of carry_segment, reduced over the tile.  em / ee: the entry mantissa and
// binade of each tile the carry accepted in a batch (ee = INT32_MIN: not
// batched), expanded per chunk by k_tile_apply.
struct TileComp {
  int32_t *e;                // [tiles] binade, INT32_MIN: no composite
  long long *D, *LO, *HI;    // [2 * tiles] by entry parity
  long long *em;             // [tiles]
  int32_t *ee;               // [tiles]
};

// Values of the chunks the carry will likely replay (no summary, a predicted
// positive entry that does not clamp for certain), gathered ahead in
// parallel (k_summ_fixw): a replay then costs one coalesced 32-B load
// per lane instead of the dependent base / code / LUT loads of values4.
struct ReplayBuf {
  int32_t *slot;             // [nch] slot of chunk c, -1: none
  int64_t *chunk;            // [2 * cap] chunk of a slot
  double *v;                 // [2 * cap * 256] values, lane-major (4 per lane)
  unsigned long long *count; // [2] listed chunks per half (may exceed cap: those are not listed)
  int64_t cap;               // slots per half
};

struct Cand {  // closed emittable excursions of the clean trajectories (segmented append)
  long long *beg, *arg, *rst;
  double *best;
  unsigned long long *count;  // [kSegs]
  int64_t cap, segcap;
};

struct Rescan {
  int64_t *a, *b;  // virtual runs [a, b) for the lane kernel (segmented append)
  int32_t *seq;
  unsigned long long *count;  // [kSegs]
  int64_t cap, segcap;
};

// Emission rules of the scan (kmer_regions or tr_lr, see ScanMode).
struct EmitCfg {
  int trlr;
  uint64_t mw;          // kmer_regions: (size_t)min_width
  double min_score;     // kmer_regions
  int64_t min_len;      // tr_lr
  const double *ks;     // tr_lr: score of each run's first k-mer
  int k;
};

// tr_lr position of scan index j in a run whose first scan index is f: the
// first k-mer's step sits at f, the transition of the k-mer ending at p at
// index p + 1.  kmer_regions reports scan indices.
__device__ __forceinline__ int64_t pos_of(const EmitCfg &ec, int64_t j, int64_t f) {
  return (ec.trlr && j != f) ? j - 1 : j;
}

// What an excursion (beg, first argmax arg, max best, ending at scan index
// end; closed = it returned to 0 there, else open at the run end) produces:
// a region record and/or a rescan range (virtual run [res_a, res_b) for the
// lane kernel).  f = the run's first scan index.
struct Emission {
  bool reg, res;
  int64_t rbeg, rend;    // region record (positions)
  int64_t res_a, res_b;
};

__device__ __forceinline__ Emission decide(const EmitCfg &ec, int64_t f, int64_t beg, int64_t arg, double best,
                                           int64_t end, bool closed) {
  Emission e;
  if (!ec.trlr) {  // kmer_regions: emitted excursions rescan (arg, end], open ones included
    e.reg = (uint64_t)(arg - beg) >= ec.mw && best >= ec.min_score;
    e.res = e.reg && arg + 1 <= end;
    e.rbeg = beg;
    e.rend = arg;
    e.res_a = arg + 1 - ec.k;
    e.res_b = end + 1;
  } else {  // tr_lr: positions; every closed excursion rescans (pos(arg), pos(end)]
    const int64_t pb = pos_of(ec, beg, f), pa = pos_of(ec, arg, f), pe = pos_of(ec, end, f);
    e.reg = pa - pb >= ec.min_len;
    // ... but only a tail that can hold a region (>= min_len + 1 positions, and
    // >= 2: a one-position tail cannot even hold an excursion) changes the
    // output; the scan after the tail is the top-level one either way
    e.res = closed && pe - pa - 1 >= (ec.min_len > 1 ? ec.min_len : 1);
    e.rbeg = pb;
    e.rend = pa;
    e.res_a = pa + 1 - ec.k;  // lane kernel (tr_lr): positions [res_a + k, res_b)
    e.res_b = pe + 1;
  }
  (void)best;
  return e;
}

// Bits of a positive normal double in binade e: x = m * 2^(e-52), m in [2^52, 2^53).
__device__ __forceinline__ int binade_of(double x) {
  return (int)((__double_as_longlong(x) >> 52) & 0x7ff) - 1023;
}
__device__ __forceinline__ long long mant_of(double x) {
  return (__double_as_longlong(x) & ((1LL << 52) - 1)) | (1LL << 52);
}
__device__ __forceinline__ double from_mant(long long m, int e) {
  return __longlong_as_double(((long long)(e + 1023) << 52) | (m - (1LL << 52)));
}

__device__ __forceinline__ uint32_t roll(uint32_t c, uint8_t b, uint32_t mask) {
  return ((c << 2) | enc(b)) & mask;
}

// 16 bytes at an arbitrary position (two aligned 16-byte loads).
__device__ __forceinline__ void load16(const uint8_t *__restrict__ seq, int64_t p, int64_t total,
                                       uint8_t out[16]) {
  const int64_t a0 = p & ~(int64_t)15;
  const int sh = (int)(p - a0);
  uint32_t w[8];
  uint4 v0 = make_uint4(0x4e4e4e4eu, 0x4e4e4e4eu, 0x4e4e4e4eu, 0x4e4e4e4eu), v1 = v0;
  if (a0 < total) v0 = *reinterpret_cast<const uint4 *>(seq + a0);
  if (a0 + 16 < total) v1 = *reinterpret_cast<const uint4 *>(seq + a0 + 16);
  w[0] = v0.x; w[1] = v0.y; w[2] = v0.z; w[3] = v0.w; w[4] = v1.x; w[5] = v1.y; w[6] = v1.z; w[7] = v1.w;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int q = sh + j;
    out[j] = (uint8_t)(w[q >> 2] >> (8 * (q & 3)));
  }
}

__device__ __forceinline__ size_t code_slot(int64_t c, int i) {
  // [tile = c/64][i/4][lane = c%64][i%4]: a wave's lanes store 8 B each, contiguous
  return ((((size_t)(c >> 6) * (CH / 4) + (size_t)(i >> 2)) * 64 + (size_t)(c & 63)) << 2) + (size_t)(i & 3);
}

// Three dwords at a 4-byte-aligned address (one global_load_dwordx3).
typedef uint32_t u32x3a4 __attribute__((ext_vector_type(3), aligned(4)));
typedef uint32_t u32x4a4 __attribute__((ext_vector_type(4), aligned(4)));

// The 16 codes of indices b0 .. b0+15 (b0 % 4 == 0) as 8 words of 2 codes.
__device__ __forceinline__ void load_codes16(const uint16_t *__restrict__ codes, int64_t c, int b0, uint32_t w[8]) {
#pragma unroll
  for (int h = 0; h < 4; ++h) {
    const uint2 x = *reinterpret_cast<const uint2 *>(codes + code_slot(c, b0 + 4 * h));
    w[2 * h] = x.x;
    w[2 * h + 1] = x.y;
  }
}

// The kept codes (SLOT_CODE_KEEP, ChunkKeep::codes_ok): the uint16 LUT index
// of every scan index, in the steps of J indices the line pass that wrote them
// walks (k_pass1w / k_pass1l, kStore).  A step's J codes are one record of
// W = (J + 1) / 2 dwords, code t in halfword t, and the records lie
// [tile = c / 64][step][lane = c % 64]: a wave writes (and k_pass1c reads) one
// contiguous run of 64 W dwords per step.  J = 6: 43 steps x 12 B = 516 B per
// chunk, against 512 B for code_slot -- whose four-index groups a six-index
// step would fill with a varying number of stores per step, and the writer's
// counted waits need a fixed one.
__host__ __device__ constexpr int kc_words(int J) { return (J + 1) / 2; }
__host__ __device__ constexpr int kc_steps(int J) { return (CH + J - 1) / J; }
// dword offset of step s of chunk c
__host__ __device__ __forceinline__ size_t kc_slot(int64_t c, int s, int J) {
  return (((size_t)(c >> 6) * kc_steps(J) + (size_t)s) * 64 + (size_t)(c & 63)) * kc_words(J);
}
__host__ __device__ __forceinline__ size_t kc_bytes(int64_t nch, int J) {
  return (size_t)((nch + 63) >> 6) * kc_steps(J) * 64 * kc_words(J) * 4;
}
// One record (W dwords at a 4 W-byte-aligned address: one store / load).
template <int W>
__device__ __forceinline__ void kc_store(uint32_t *__restrict__ p, const uint32_t (&r)[W]) {
  if constexpr (W == 2) {
    *reinterpret_cast<uint2 *>(p) = make_uint2(r[0], r[1]);
  } else if constexpr (W == 3) {
    u32x3a4 v;
    v.x = r[0]; v.y = r[1]; v.z = r[2];
    *reinterpret_cast<u32x3a4 *>(p) = v;
  } else {
    static_assert(W == 4, "a record is 2 to 4 dwords");
    *reinterpret_cast<uint4 *>(p) = make_uint4(r[0], r[1], r[2], r[3]);
  }
}
template <int W>
__device__ __forceinline__ void kc_load(const uint32_t *__restrict__ p, uint32_t (&r)[W]) {
  if constexpr (W == 2) {
    const uint2 v = *reinterpret_cast<const uint2 *>(p);
    r[0] = v.x; r[1] = v.y;
  } else if constexpr (W == 3) {
    const u32x3a4 v = *reinterpret_cast<const u32x3a4 *>(p);
    r[0] = v.x; r[1] = v.y; r[2] = v.z;
  } else {
    static_assert(W == 4, "a record is 2 to 4 dwords");
    const uint4 v = *reinterpret_cast<const uint4 *>(p);
    r[0] = v.x; r[1] = v.y; r[2] = v.z; r[3] = v.w;
  }
}
// The record of J codes (each < 2^16).
template <int J>
__device__ __forceinline__ void kc_pack(const uint32_t (&cs)[J], uint32_t (&r)[(J + 1) / 2]) {
#pragma unroll
  for (int q = 0; q < (J + 1) / 2; ++q) r[q] = cs[2 * q] | (2 * q + 1 < J ? cs[2 * q + 1] << 16 : 0u);
}

// Values of NV consecutive scan indices from a line table (ks_table
// line_kind), OWN + 1 per line read: the line's own entries and the L1 entry
// chosen by the next base (its first 16-32 B; lane-wise reads, for the
// passes after pass 1).  x: 64 bits of packed bases from the first base of
// index b0's k-mer; indices past n read nothing and get 0.
template <int OWN, int NV>
__device__ __forceinline__ void line_values(const TableView &tv, uint64_t x, int k, int b0, int n, double v[NV],
                                            const double *s_lut) {
  constexpr int JL = OWN + 1;
  const int kx = k + OWN;  // the (m + 1)-mer: line index and the L1 base
  const uint64_t xmask = (1ull << (2 * kx)) - 1ull;
#pragma unroll
  for (int o = 0; o < NV; o += JL) {
    double lv[JL];
#pragma unroll
    for (int t = 0; t < JL; ++t) lv[t] = 0.0;
    if (b0 + o < n) line_entries<OWN>(tv, (x >> (64 - 2 * (o + kx))) & xmask, lv, s_lut);
#pragma unroll
    for (int t = 0; t < JL; ++t)
      if (o + t < NV) v[o + t] = (b0 + o + t < n) ? lv[t] : 0.0;
  }
}

template <int NV>
__device__ __forceinline__ void line_values_any(const TableView &tv, uint64_t x, int k, int b0, int n, double v[NV],
                                                const double *s_lut) {
  switch (tv.line_own) {
    case 1: line_values<1, NV>(tv, x, k, b0, n, v, s_lut); break;  // (wide lines at k = 15)
    case 2: line_values<2, NV>(tv, x, k, b0, n, v, s_lut); break;
    case 3: line_values<3, NV>(tv, x, k, b0, n, v, s_lut); break;
    case 4: line_values<4, NV>(tv, x, k, b0, n, v, s_lut); break;
    default: line_values<5, NV>(tv, x, k, b0, n, v, s_lut); break;
  }
}

// Values of scan indices b0 .. b0+15 of chunk c (0 past n) of a compressed
// table whose per-index codes were not stored (small-k pass 1): the 16
// k-mers from one 64-bit window of packed bases (bytes near the buffer end),
// each looked up in the base code table (L2-resident for small k) and the LUT.
template <int NV = 16>
__device__ __forceinline__ void values16_nostore(const Chunks &g, const uint8_t *__restrict__ seq, int64_t total,
                                                 int k, const TableView &tv, int64_t c, int b0, int n, double v[NV],
                                                 const double *s_lut) {
  const int64_t p = g.start[c] + b0 - k;  // first base of index b0's k-mer
  const uint32_t kmask = (1u << (2 * k)) - 1u;
  uint64_t x = 0;
  const bool pk = packed_bits(g.packed, total, p, x);
  if (pk && tv.line) {  // line table: OWN + 1 indices per read
    line_values_any<NV>(tv, x, k, b0, n, v, s_lut);
    return;
  }
  if (pk && tv.compressed && tv.ext && tv.ext_J >= 2 && k + tv.ext_J - 1 + 15 <= 32) {
    // one expanded-table read per J indices (the gathers of k_summ_fixw and
    // the heads: 4 random requests per 16 indices at J = 5 instead of 32;
    // uint16 / 12-bit code entries: FP64 tables take the base table below)
    const int J = tv.ext_J, kx = k + J - 1;
    const uint64_t xmask = (kx >= 32) ? ~0ull : ((1ull << (2 * kx)) - 1ull);
    const bool c12 = tv.ext_bits == 12;
    for (int o = 0; o < NV; o += J) {
      if (b0 + o >= n) {
        for (int t = o; t < NV; ++t) v[t] = 0.0;
        break;
      }
      const uint64_t gx = (x >> (64 - 2 * (o + kx))) & xmask;
      uint64_t e;
      if (J <= 2) e = reinterpret_cast<const uint32_t *>(tv.ext)[gx];
      else e = reinterpret_cast<const uint64_t *>(tv.ext)[gx];
      for (int t = 0; t < J && o + t < NV; ++t) {
        const int j = o + t;
        double val = 0.0;
        if (b0 + j < n) {
          uint32_t q;
          if (c12) {
            const uint32_t q12 = (uint32_t)(e >> (12 * t)) & 0xfffu;
            q = q12 != 0xfffu ? (uint32_t)tv.map12[q12]
                              : (uint32_t)tv.codes[(uint32_t)(x >> (64 - 2 * (j + k))) & kmask];
          } else {
            q = (uint32_t)(e >> (16 * t)) & 0xffffu;
          }
          val = s_lut ? s_lut[q] : tv.lut[q];
        }
        v[j] = val;
      }
    }
    return;
  }
  uint32_t code = pk ? 0u : prime_code(seq, p, k);
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    if (pk) code = (uint32_t)(x >> (64 - 2 * (j + k))) & kmask;
    else if (j > 0 && b0 + j < n) code = ((code << 2) | enc(seq[p + k - 1 + j])) & kmask;
    if (!tv.compressed) {  // FP64 base table (small k with the table in LDS for pass 1)
      v[j] = b0 + j < n ? tv.vals[code] : 0.0;
      continue;
    }
    const uint32_t q = b0 + j < n ? tv.codes[code] : 0u;
    v[j] = b0 + j < n ? (s_lut ? s_lut[q] : tv.lut[q]) : 0.0;
  }
}

// Values of scan indices b0 .. b0+15 of a chunk starting at start (0 past
// n) from an FP64 table: the line table (OWN + 1 indices per read) where the
// packed bases cover the window, else the base table by rolling codes.
// code: the k-mer of index b0 on entry, of b0 + 16 on exit.
__device__ __forceinline__ void values16_f64(const Chunks &g, const uint8_t *__restrict__ seq, int64_t total, int k,
                                             const TableView &tv, int64_t start, int b0, int n, uint32_t &code,
                                             uint32_t mask, double v[NB]) {
  uint64_t xb = 0;
  if (tv.line && packed_bits(g.packed, total, start + b0 - k, xb)) {
    line_values_any<NB>(tv, xb, k, b0, n, v, nullptr);
    code = (uint32_t)(xb >> (64 - 2 * (NB + k))) & mask;
    return;
  }
  uint8_t by[16];
  load16(seq, start + b0, total, by);
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    v[j] = (b0 + j < n) ? tv.vals[code] : 0.0;
    code = roll(code, by[j], mask);
  }
}

// The values4 of a replay from an FP64 64-B line table with own = 3 (weighted
// rank, k = 13: one line per lane, its three own entries and the L1 entry of
// the next base), fetched by the whole wave together: lanes 4m .. 4m + 3 load
// the four 16-B pieces of line 16 r + m (r = 0 .. 3), so each line costs one
// coalesced 64-B request instead of three divergent loads of one lane
// (round 6: half of the weighted-rank rescans' time was those loads,
// DESIGN.md section 10), by LDS-DMA into 4 KiB of LDS per wave.  Every lane of the
// wave calls it (uniform), each with its packed bases x of index i0's k-mer.
__device__ __forceinline__ void values4_coop_f64(const TableView &tv, uint64_t x, int k, int i0, int n,
                                                 double v[4], uint4 *__restrict__ s_piece,
                                                 unsigned long long *__restrict__ s_key) {
  const int lane = threadIdx.x & 63;
  const int kx = k + 3;
  const uint64_t key = (x >> (64 - 2 * kx)) & ((1ull << (2 * kx)) - 1ull);
  const bool valid = i0 < n;
  s_key[lane] = valid ? (unsigned long long)(key >> 2) : ~0ull;
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
  // LDS-DMA (global_load_lds_dwordx4): lane l's piece lands at s_piece[64 r + l] = piece l & 3 of
  // line 16 r + (l >> 2), no VGPRs on the way (the FP64 carry holds 168); a lane without a line
  // reads line 0 into a slot nobody reads
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const unsigned long long ln = s_key[16 * r + (lane >> 2)];
    const uint8_t *src = tv.line + (ln != ~0ull ? (size_t)ln * 64 : (size_t)0) + 16 * (lane & 3);
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                     (__attribute__((address_space(3))) void *)(s_piece + 64 * r), 16, 0, 0);
  }
  // the DMA writes must have landed before any lane reads them: an explicit
  // vmcnt(0) lgkmcnt(0) (hipcc placed its own wait only before the
  // conditional reads below, not before the hoisted L1 one)
  __builtin_amdgcn_s_waitcnt(0x0070);
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const double *L = reinterpret_cast<const double *>(s_piece + 4 * lane);
  const double l1 = L[3 + (int)(key & 3u)];
  v[0] = valid ? L[0] : 0.0;
  v[1] = i0 + 1 < n ? L[1] : 0.0;
  v[2] = i0 + 2 < n ? L[2] : 0.0;
  v[3] = i0 + 3 < n ? l1 : 0.0;
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");  // (the next call's writes after these reads)
}

// Values of scan indices i0 .. i0+3 of chunk c (0 past n): one 8-byte code
// load (compressed) or one k-mer prime plus three rolls.  start: the chunk's
// first scan index (g.start[c]), loaded by the caller ahead of time; xin
// (have_x): the 64 packed bits from base start + i0 - k, prefetched.
__device__ __forceinline__ void values4(const Chunks &g, const uint8_t *__restrict__ seq, int64_t total, int k,
                                        const TableView &tv, const uint16_t *__restrict__ codes, int64_t c,
                                        int64_t start, int i0, int n, double v[4], bool have_x = false,
                                        uint64_t xin = 0) {
#pragma unroll
  for (int q = 0; q < 4; ++q) v[q] = 0.0;
  if (i0 >= n) return;
  if (codes) {
    const uint2 w = *reinterpret_cast<const uint2 *>(codes + code_slot(c, i0));
    const uint32_t cw[2] = {w.x, w.y};
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (i0 + q < n) v[q] = tv.lut[(cw[q >> 1] >> (16 * (q & 1))) & 0xffffu];
    return;
  }
  const int64_t p = start + i0;
  if (tv.line) {  // line table: OWN + 1 indices per read
    uint64_t xp = xin;
    if (have_x || packed_bits(g.packed, total, p - k, xp)) {
      line_values_any<4>(tv, xp, k, i0, n, v, nullptr);
      return;
    }
  }
  if (!tv.compressed && tv.ext && tv.ext_J == 4) {  // FP64 expanded table: the 4 values in one 32-B entry
    uint64_t xp = xin;
    const uint64_t gcode = (have_x || packed_bits(g.packed, total, p - k, xp))
                               ? (xp >> (64 - 2 * (k + 3)))
                               : prime_code_guarded64(seq, p - k, k + 3, total);
    const double2 *E = reinterpret_cast<const double2 *>(tv.ext);
    const double2 e0 = E[2 * gcode], e1 = E[2 * gcode + 1];
    const double ev[4] = {e0.x, e0.y, e1.x, e1.y};
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (i0 + q < n) v[q] = ev[q];
    return;
  }
  if (!tv.compressed && !tv.line) {
    // FP64 J = 2 / 3 expanded tables (weighted rank, k = 14, 15) and FP64
    // base tables: the k-mers from the packed bases (prefetched by the carry),
    // not from k + 3 bytes
    uint64_t xp = xin;
    if (have_x || packed_bits(g.packed, total, p - k, xp)) {
      const uint64_t G = xp >> (64 - 2 * (k + 3));  // the (k + 3)-mer of indices i0 .. i0 + 3
      const uint64_t mk = ((uint64_t)1 << (2 * k)) - 1;
      double ev[4];
      if (tv.ext && tv.ext_J == 2) {  // entries (v_j, v_j+1) of (k + 1)-mers, 16 B
        const double2 *E = reinterpret_cast<const double2 *>(tv.ext);
        const uint64_t m1 = ((uint64_t)1 << (2 * (k + 1))) - 1;
        const double2 a = E[G >> 4], b = E[G & m1];
        ev[0] = a.x;
        ev[1] = a.y;
        ev[2] = b.x;
        ev[3] = b.y;
      } else if (tv.ext && tv.ext_J == 3) {  // entries (v_j .. v_j+2, 0) of (k + 2)-mers, 32 B
        const double2 *E = reinterpret_cast<const double2 *>(tv.ext);
        const uint64_t e = G >> 2;
        const double2 a = E[2 * e], b = E[2 * e + 1];
        ev[0] = a.x;
        ev[1] = a.y;
        ev[2] = b.x;
        ev[3] = tv.vals[G & mk];
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) ev[q] = tv.vals[(G >> (2 * (3 - q))) & mk];
      }
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (i0 + q < n) v[q] = ev[q];
      return;
    }
  }
  const uint32_t mask = (1u << (2 * k)) - 1u;
  uint32_t code = prime_code(seq, p - k, k);
  v[0] = tv_get(tv, code);
#pragma unroll
  for (int q = 1; q < 4; ++q) {
    if (i0 + q < n) {
      code = ((code << 2) | enc(seq[p + q - 1])) & mask;
      v[q] = tv_get(tv, code);
    }
  }
}

// Packed-code words staged in LDS per pass-1 lane: bases [q0, q0 + 320) of
// its chunk (q0 = start + J - 1), loaded once (5 x 16 B) instead of one 12-B
// load per batch, so the lane's two 128-B lines are fetched once even when
// the random table reads evict them from L2 between batches.
constexpr bool kP1Stage = true;
// Table reads per batch of the pipelined pass 1: 3 leaves registers for two
// binade summaries (G = 4 spilled: 17.10 vs 14.66 ms; G = 8 at 768-lane
// blocks: 17.7 vs 16.4 ms).  The buffer-end margins below are computed for
// kP1G = 4 (conservative for 3).
constexpr int kP1GSumm = 3;
constexpr int kP1G = 4;
constexpr int kP1Block = 1024;  // lanes per pass-1 block (512 / 256: 147 / 108 vs 163 Gbases/s)
// Pass-1 summaries start at predicted entries of 1024 (below, exact halves
// make most chunks' single-trajectory summaries void; k_summ_fixw does those).
constexpr double kP1SumMin = 1024.0;
// A predicted entry within this relative distance of a binade edge is
// summarised in the neighbouring binade too.
constexpr double kP1Margin = 0.125;
static_assert(kP1Block % 64 == 0 && kP1Block <= 1024, "pass-1 block is whole waves");
constexpr int kP1StageWords = 20;
// Bases past its chunk's first scan index a pass-1 lane may read: the
// pipelined kernel's windows reach two batches ahead (< 256 + 2 * 40 + 3 * 16)
// and the LDS staging reads kP1StageWords words from word (start + J - 1) / 16.
// Lanes closer than this to the buffer end are left to k_pass1 (tail_only),
// so every packed word they stage exists (the packed array has total / 16 + 1
// words, ks_runs.hip).
constexpr int kP1WinReach = 4 + 255 + 2 * 5 * kP1G + 16 * 3;  // J - 1 + last b0 + 2 PB + window
constexpr int kP1StageReach = 16 * kP1StageWords + 21;
constexpr int kP1TailMargin = kP1WinReach > kP1StageReach ? (kP1WinReach > 352 ? kP1WinReach : 352)
                                                          : (kP1StageReach > 352 ? kP1StageReach : 352);
static_assert(16 * kP1StageWords + 4 <= kP1TailMargin + 16 + 1, "staged packed words stay inside the buffer");
static_assert(kP1WinReach <= kP1TailMargin + 1, "pipelined windows stay inside the buffer");

// Wave-uniform broadcast of lane j's value (v_readlane: a VALU op, unlike a
// variable-lane __shfl which goes through ds_bpermute).
__device__ __forceinline__ int rl32(int v, int j) { return __builtin_amdgcn_readlane(v, j); }
__device__ __forceinline__ long long rl64(long long v, int j) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(v & 0xffffffff), j);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(v >> 32), j);
  return (long long)(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ double rld(double v, int j) { return __longlong_as_double(rl64(__double_as_longlong(v), j)); }

// Wave64 scans on DPP lane moves (GFX9 DPP, a VALU operand modifier: no LDS
// round trip, unlike the ds_bpermute behind a variable __shfl): lane i reads
// lane i - d of its 16-lane row (row_shr:d), lane 15 of the row before
// (row_bcast:15, rows 1 and 3), lane 31 (row_bcast:31, rows 2 and 3), or
// lane i - 1 across the wave (wave_shr:1).  Lanes without a source read 0,
// the identity of every scan below.  The whole wave must be active.
template <int CTRL, int RM>
__device__ __forceinline__ int dpp_i32(int v) {
  return __builtin_amdgcn_update_dpp(0, v, CTRL, RM, 0xf, true);
}
template <int CTRL, int RM>
__device__ __forceinline__ long long dpp_i64(long long v) {
  const int lo = dpp_i32<CTRL, RM>((int)(v & 0xffffffff)), hi = dpp_i32<CTRL, RM>((int)(v >> 32));
  return (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}
template <int CTRL, int RM>
__device__ __forceinline__ double dpp_f64(double v) {
  return __longlong_as_double(dpp_i64<CTRL, RM>(__double_as_longlong(v)));
}
constexpr int kDppShr1 = 0x111, kDppShr2 = 0x112, kDppShr4 = 0x114, kDppShr8 = 0x118, kDppBc15 = 0x142,
              kDppBc31 = 0x143, kDppWaveShr1 = 0x138;
// Inclusive wave scan of an associative op(left, right) whose identity is
// all-zero bits, on a value type V moved by Mov<CTRL, RM>(V).
#define KS_DPP_SCAN(V, x, MOV, OP)                     \
  do {                                                 \
    x = OP(MOV<kDppShr1, 0xf>(x), x);                  \
    x = OP(MOV<kDppShr2, 0xf>(x), x);                  \
    x = OP(MOV<kDppShr4, 0xf>(x), x);                  \
    x = OP(MOV<kDppShr8, 0xf>(x), x);                  \
    x = OP(MOV<kDppBc15, 0xa>(x), x);                  \
    x = OP(MOV<kDppBc31, 0xc>(x), x);                  \
  } while (0)

__device__ __forceinline__ double wave_sum_incl(double x) {
  auto add = [](double a, double b) { return a + b; };
  KS_DPP_SCAN(double, x, dpp_f64, add);
  return x;
}
// previous lane's value (0 in lane 0)
__device__ __forceinline__ long long wave_prev_i64(long long v) { return dpp_i64<kDppWaveShr1, 0xf>(v); }
__device__ __forceinline__ int wave_prev_i32(int v) { return dpp_i32<kDppWaveShr1, 0xf>(v); }

// Parity-pair integer maps (d0, d1): entry parity p -> increment d_p;
// (a then b)_p = a_p + b_{(p + a_p) & 1}.  Identity (0, 0).
struct PPair {
  long long d0, d1;
};
__device__ __forceinline__ PPair pp_compose(const PPair &a, const PPair &b) {
  return PPair{a.d0 + ((a.d0 & 1) ? b.d1 : b.d0), a.d1 + (((1 + a.d1) & 1) ? b.d1 : b.d0)};
}
template <int CTRL, int RM>
__device__ __forceinline__ PPair dpp_pp(const PPair &v) {
  return PPair{dpp_i64<CTRL, RM>(v.d0), dpp_i64<CTRL, RM>(v.d1)};
}
__device__ __forceinline__ PPair pp_scan_incl(PPair x) {
  KS_DPP_SCAN(PPair, x, dpp_pp, pp_compose);
  return x;
}
__device__ __forceinline__ PPair pp_prev(const PPair &v) { return PPair{wave_prev_i64(v.d0), wave_prev_i64(v.d1)}; }

// segmented parity-pair scan element (f: a segment starts in this lane's part)
struct SegPP {
  PPair s;
  int f;
};
template <int CTRL, int RM>
__device__ __forceinline__ SegPP dpp_seg(const SegPP &v) {
  return SegPP{dpp_pp<CTRL, RM>(v.s), dpp_i32<CTRL, RM>(v.f)};
}
__device__ __forceinline__ SegPP seg_op(const SegPP &l, const SegPP &r) {
  return SegPP{r.f ? r.s : pp_compose(l.s, r.s), l.f | r.f};
}
// forward fill of a flagged value
struct FillM {
  long long m;
  int f;
};
template <int CTRL, int RM>
__device__ __forceinline__ FillM dpp_fill(const FillM &v) {
  return FillM{dpp_i64<CTRL, RM>(v.m), dpp_i32<CTRL, RM>(v.f)};
}
__device__ __forceinline__ FillM fill_op(const FillM &l, const FillM &r) { return FillM{r.f ? r.m : l.m, l.f | r.f}; }

// DPP moves whose lanes without a source keep `old` (bound_ctrl off): scans
// whose identity is not all-zero bits.
template <int CTRL, int RM>
__device__ __forceinline__ double dpp_f64_or(double v, double old) {
  const long long x = __double_as_longlong(v), o = __double_as_longlong(old);
  const int lo = __builtin_amdgcn_update_dpp((int)(o & 0xffffffff), (int)(x & 0xffffffff), CTRL, RM, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp((int)(o >> 32), (int)(x >> 32), CTRL, RM, 0xf, false);
  return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}
// The predictor's max-plus pairs: (a1, b1) then (a2, b2) = (a1 + a2,
// max(b1 + a2, b2)); identity (0, -inf).
struct APair {
  double a, b;
};
template <int CTRL, int RM>
__device__ __forceinline__ APair dpp_ap(const APair &v) {
  return APair{dpp_f64_or<CTRL, RM>(v.a, 0.0), dpp_f64_or<CTRL, RM>(v.b, -INFINITY)};
}
__device__ __forceinline__ APair ap_op(const APair &l, const APair &r) { return APair{l.a + r.a, fmax(l.b + r.a, r.b)}; }
__device__ __forceinline__ APair ap_prev(const APair &v) { return dpp_ap<kDppWaveShr1, 0xf>(v); }

// ------------------------------------------------------------------- P0

// Chunk start, length and run, a wave per stitch tile (64 chunks of one run),
// the run from the tile map of k_tile_runs (in-process A/B against a binary
// search per chunk: 17.91-18.00 vs 18.01-18.13 ms).
__global__ void k_make_chunks(const int64_t *__restrict__ ra, const int64_t *__restrict__ cbase,
                              const int64_t *__restrict__ tbase, const int32_t *__restrict__ trun, int64_t ntiles,
                              int k, const int64_t *__restrict__ rbnd, int extra, Chunks g) {
  const int64_t t = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (t >= ntiles) return;
  const int64_t lo = trun[t];
  const int64_t c = cbase[lo] + (t - tbase[lo]) * 64 + (threadIdx.x & 63);
  if (c >= cbase[lo + 1]) return;
  const int64_t first = ra[lo] + k + (c - cbase[lo]) * CH;
  const int64_t last = rbnd[lo] - 1 + extra;  // tr_lr: one more index (the first k-mer's own step)
  g.start[c] = first;
  g.n[c] = (int32_t)min((int64_t)CH, last - first + 1);
  g.run[c] = (int32_t)lo;
}

// P0 binade predictor (pass-1 summaries): the approximate sum and clean
// exit of every chunk from the fp16 prefix means of the table (ks_table::
// d_approx, <= 128 KiB in LDS, one block per CU), rolled from the packed
// bases; a max-plus scan of them (k_approx_scan) predicts each chunk's entry,
// i.e. the binade pass 1 summarises in.  Only a prediction: a wrong binade
// costs one gathered summary (k_summ_fixw), never a result.
// The chunk's 18 packed words (bases q0 .. q0 + 287, q0 = start - k) in
// registers: five aligned 16-B loads (a quarter of the requests of 18 word
// loads: the lanes of a wave read 64 different lines per instruction), then
// the 18 words at offset w0 - wa selected in registers.
struct PredWords {
  uint32_t a[21];  // a[20]: the third word of the last 16 indices at o = 3 (past the loads: 0)
  int o;
  __device__ __forceinline__ void load(const uint32_t *__restrict__ packed, int64_t total, int64_t q0) {
    const int64_t w0 = q0 >> 4, last = total >> 4;
    const int64_t wa = w0 & ~(int64_t)3;
    if (wa + 20 <= last + 1) {
      const uint4 *P4 = reinterpret_cast<const uint4 *>(packed + wa);
#pragma unroll
      for (int t = 0; t < 5; ++t) {
        const uint4 v = P4[t];
        a[4 * t] = v.x;
        a[4 * t + 1] = v.y;
        a[4 * t + 2] = v.z;
        a[4 * t + 3] = v.w;
      }
      a[20] = 0;
      o = (int)(w0 - wa);
    } else {
#pragma unroll
      for (int t = 0; t < 18; ++t) a[t] = packed[min(w0 + t, last)];
      o = 0;
    }
  }
  __device__ __forceinline__ uint32_t w(int t) const {
    return o == 0 ? a[t] : (o == 1 ? a[t + 1] : (o == 2 ? a[t + 2] : a[t + 3]));
  }
};

// P0 binade predictor (pass-1 summaries): the approximate sum and clean
// exit of every chunk from the fp16 prefix means of the table (ks_table::
// d_approx, <= 128 KiB in LDS, one block per CU), rolled from the packed
// bases; a max-plus scan of them (k_approx_scan) predicts each chunk's entry,
// i.e. the binade pass 1 summarises in.  Only a prediction: a wrong binade
// costs one gathered summary (k_summ_fixw), never a result.  (A
// software-pipelined loop -- the next chunk's words in flight while one is
// summed -- measured the same: profiles/r4/ab/ab_log2.txt.)
template <int PS>
__global__ void __launch_bounds__(1024) k_predict(Chunks g, int64_t total, int k, const uint16_t *__restrict__ approx, int kp,
                                                  double *__restrict__ pa, double *__restrict__ pb) {
  extern __shared__ __half s_ap[];  // 4^kp entries (dynamic: 32 KiB at kp = 7 lets 4 blocks share a CU)
  const int np = 1 << (2 * kp);
  for (int i = threadIdx.x; i < np; i += blockDim.x) s_ap[i] = __ushort_as_half(approx[i]);
  __syncthreads();
  const uint32_t pmask = (uint32_t)np - 1u;
  const uint32_t *__restrict__ packed = g.packed;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  auto sum_chunk = [&](const PredWords &W, int64_t q0, int n, int64_t c) {
    const uint32_t bp = 2u * (uint32_t)(q0 & 15);
    float tsum = 0.f, tex = 0.f;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      if (16 * t < n) {
        const uint64_t x = ((((uint64_t)W.w(t) << 32) | W.w(t + 1)) << bp) | (((uint64_t)W.w(t + 2) << bp) >> 32);
        // every PS-th index, weighted PS (A/B: PS = 2 cut the predictor 1.11 -> 0.80 ms with the
        // same 16.2 K gathered summaries at the metric config; PS = 4 is the default since round 4)
        float a[16 / PS];
#pragma unroll
        for (int j = 0; j < 16; j += PS)
          a[j / PS] = __half2float(s_ap[(uint32_t)(x >> (64 - 2 * (j + kp))) & pmask]);
#pragma unroll
        for (int j = 0; j < 16; j += PS) {
          const float aj = (16 * t + j < n) ? a[j / PS] * (float)PS : 0.f;
          tsum += aj;
          tex = fmaxf(tex + aj, 0.f);
        }
      }
    }
    pa[c] = tsum;
    pb[c] = tex;
  };
  for (int64_t c = g.c0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < g.nch; c += stride) {
    PredWords W;
    const int64_t q0 = g.start[c] - k;  // index i's k-mer prefix: bases [q0 + i, q0 + i + kp)
    W.load(packed, total, q0);
    sum_chunk(W, q0, g.n[c], c);
  }
}

// ------------------------------------------------------------------- P1

// Every pass-1 kernel does the same work per scan index of a chunk and differs
// only in how it fetches the value s: that work is P1Lane below (init / step /
// finish), used by k_pass1l, k_pass1w, k_pass1r, k_pass1pf and k_pass1_lds.
// Four kernels keep a walk of their own.  k_pass1_lds_int walks on int32:
// 32-bit integer compares instead of FP64 ones are the point of that kernel.
// k_pass1p keeps a copy in locals, for its registers (see there).  k_pass1
// keeps its if / else-if form that asks decide(): on the walker its J = 1
// instantiations took 147-161 VGPRs instead of 181-191 and ran slower (see
// there).  k_pass1c without the visit histogram walks with code_index, the
// exact-entry step arranged for a wave of full chunks (see there; its visit
// flavour uses P1Lane).  All share the candidate append (cand_put) and the
// result store (p1_put / finish_exact).  So the emission rule (the candidate
// test) is written in five places: P1Lane::step, k_pass1p, code_index, for
// kmer_regions alone k_pass1_lds_int, and decide(), which k_pass1
// (cand_wanted), the stitch and k_candidates ask.

// A closed candidate excursion of the chunk starting at scan index start
// (chunk-relative beg, arg, end) joins the segmented list.
__device__ __forceinline__ void cand_put(const Cand &cand, int64_t start, int beg, int arg, int end, double best) {
  const int64_t slot = append_one(cand.count, cand.segcap);
  if (slot >= 0) {
    cand.beg[slot] = start + beg;
    cand.arg[slot] = start + arg;
    cand.rst[slot] = start + end;
    cand.best[slot] = best;
  }
}

// Chunk c's pass-1 results, stamped with the call's epoch: the aggregates,
// the clean exit prev and the trailing open excursion (beg, best, arg) if any.
__device__ __forceinline__ void p1_put(const P1 &o, int64_t c, double prev, double asum, double pmin, double pmax,
                                       int parg, double sabs, bool special, int beg, double best, int arg) {
  o.cexit[c] = prev;
  o.asum[c] = asum;
  o.pmin[c] = pmin;
  o.pmax[c] = pmax;
  o.parg[c] = parg;
  o.sabs[c] = sabs;
  o.special[c] = special ? 1 : 0;
  o.ep[c] = o.epoch;
  if (prev > 0) {
    o.tbeg[c] = beg; o.tmax[c] = best; o.targ[c] = arg;
  } else {
    o.tbeg[c] = -1; o.tmax[c] = 0.0; o.targ[c] = 0;
  }
}

// Per-lane state of pass 1 over one chunk: the clean-entry trajectory, its
// aggregates, closed candidates and (kSumm) the binade-integer summaries in
// the predicted binade and its neighbour.
//
// The summary of this chunk for the binade of its predicted entry xp
// (k_predict), single trajectory: s rounded to the binade's ulp u = 2^(e-52)
// as (s + C) - C with C = 1.5 * 2^e, exact partial sums while they stay within
// (-2^e, 2^e); an exact half (tie: the increment would depend on the parity of
// the entry) or |s| >= 2^(e-1) voids it (summ_put; k_summ_fixw then recomputes
// it).  Replaces the per-position code store and k_summaries.
//
// step() gives the same bits as fmin / fmax, an if / else-if chain and decide():
// asum starts at +0, so is never -0, and a NaN asum fails both compares, as fmin
// / fmax skip it; S > best is false at a close and while S stays 0 (best > 0
// inside, >= 0 outside), so open | (S > best) is the chain; want is decide()'s
// reg || res less start on both sides (pos_of: only a run's index 0 stays put).
//
// kExact (never with kSumm): the lane starts from the chunk's exact entry hx.T
// (the kept slot's, Keep::entry) instead of a prediction.  Beside the clean
// trajectory it walks the carried head with head_step -- the serial replay's
// and k_heads' arithmetic -- until its first clamp, writes the chunk's Carry
// fields itself and checks its exact exit against the kept entry of the next
// chunk (finish_exact).  No summaries and none of the aggregates that only
// P2-P4 read (asum, pmin, pmax, parg, sabs).

// The carried excursion of a chunk's head: its value T, its maximum hmax with
// the first argmax harg, and hq, the index of its first clamp (-1: none yet).
struct Head { double T, hmax; int harg, hq; };
// Scan index i with value v: nothing moves past the chunk's n indices or
// after the clamp.  (By value: passed by reference the heads kernels took 12 B
// of scratch per lane.)
__device__ __forceinline__ Head head_step(Head h, double v, int i, int n) {
  if (i < n && h.hq < 0) {
    const double t = h.T + v;
    h.T = t > 0 ? t : 0.0;
    if (h.T == 0.0) h.hq = i;
    else if (h.T > h.hmax) { h.hmax = h.T; h.harg = i; }
  }
  return h;
}

template <bool kSumm, bool kTrlr, bool kExact = false>
struct P1Lane {
  static_assert(!(kSumm && kExact), "the exact-entry pass writes no summaries");
  int64_t start;
  int n, f0;
  double prev = 0.0, best = 0.0;
  int beg = -1, arg = 0;
  double asum = 0.0, pmin = INFINITY, pmax = -INFINITY, sabs = 0.0;
  int parg = 0;
  bool special = false;
  int se = INT32_MIN, se2 = INT32_MIN;
  double sC = 0.0, sH = 0.0, scur = 0.0, smx = -INFINITY, smn = INFINITY;
  double sC2 = 0.0, sH2 = 0.0, scur2 = 0.0, smx2 = -INFINITY, smn2 = INFINITY;
  double smaxabs = 0.0;  // max |s| (the rounding of every step, both binades)
  int sarg = 0, sarg2 = 0;
  bool sbad = false, sbad2 = false;
  Head hx{0.0, -1.0, 0, 0};  // kExact: the carried head (hq = 0 while there is none to walk)
  bool hclean = true;        // kExact: entered at 0

  // first: the chunk starts its run; xp: the predicted entry (0: no summaries),
  // kExact: the exact entry (a run's first chunk enters at 0 whatever xp holds)
  __device__ __forceinline__ void init(int64_t st, int nn, bool first, bool live, double xp) {
    start = st;
    n = nn;
    f0 = first ? 0 : -1;
    if (kExact) {
      const double x = (first || !live) ? 0.0 : xp;
      hclean = x == 0.0;
      hx = Head{x, -1.0, 0, hclean ? 0 : -1};
    }
    if (kSumm && live && xp >= kP1SumMin && xp < 1.0e15) {
      se = binade_of(xp);
      sC = 1.5 * ldexp(1.0, se);
      sH = ldexp(1.0, se - 53);
      const double lo = ldexp(1.0, se);
      if (xp < lo * (1.0 + kP1Margin)) se2 = se - 1;
      else if (xp > 2.0 * lo * (1.0 - kP1Margin)) se2 = se + 1;
      if (se2 != INT32_MIN) {
        sC2 = 1.5 * ldexp(1.0, se2);
        sH2 = ldexp(1.0, se2 - 53);
      }
    }
  }

  // scan index i (< n) with value s
  __device__ __forceinline__ void step(double s, int i, const EmitCfg &ec, const Cand &cand) {
    if (kExact) {
      hx = head_step(hx, s, i, n);
    } else {
      asum += s;
      pmin = asum < pmin ? asum : pmin;
      parg = asum > pmax ? i : parg;
      pmax = asum > pmax ? asum : pmax;
      sabs += fabs(s);
    }
    special |= !isfinite(s);
    if (kSumm && se != INT32_MIN) {
      const double r = (s + sC) - sC;
      sbad |= fabs(r - s) == sH;
      smaxabs = fmax(smaxabs, fabs(s));
      scur += r;
      const bool su = scur > smx;
      smx = su ? scur : smx;
      sarg = su ? i : sarg;
      smn = fmin(smn, scur);
      if (se2 != INT32_MIN) {
        const double r2 = (s + sC2) - sC2;
        sbad2 |= fabs(r2 - s) == sH2;
        scur2 += r2;
        const bool su2 = scur2 > smx2;
        smx2 = su2 ? scur2 : smx2;
        sarg2 = su2 ? i : sarg2;
        smn2 = fmin(smn2, scur2);
      }
    }
    // clean trajectory, branch-free except for the rare candidate: open
    // (0 -> S > 0) starts an excursion, close (> 0 -> 0) ends it, the first
    // strict maximum is kept
    const double tt = prev + s;
    const double S = tt > 0 ? tt : 0.0;
    const bool open = (prev == 0) & (S > 0);
    const bool close = (prev > 0) & (S == 0);
    const long long ml = kTrlr ? ec.min_len : 0;
    const bool want =
        kTrlr ? (close & (((long long)((arg != f0 ? arg - 1 : arg) - (beg != f0 ? beg - 1 : beg)) >= ml) |
                          ((long long)((i != f0 ? i - 1 : i) - (arg != f0 ? arg - 1 : arg) - 1) >=
                           (ml > 1 ? ml : 1LL))))
              : (close & ((uint64_t)(int64_t)(arg - beg) >= ec.mw) & (best >= ec.min_score));
    if (want) cand_put(cand, start, beg, arg, i, best);
    const bool up = open | (S > best);
    best = up ? S : best;
    arg = up ? i : arg;
    beg = open ? i : (close ? -1 : beg);
    prev = S;
  }

  __device__ __forceinline__ void finish(int64_t c, const P1 &o, const SummP1 &sp) {
    if (kSumm) {
      summ_put(sp, c, 0, se, sbad, smaxabs, scur, smx, smn, sarg);
      summ_put(sp, c, 1, se2, sbad2, smaxabs, scur2, smx2, smn2, sarg2);
    }
    p1_put(o, c, prev, asum, pmin, pmax, parg, sabs, special, beg, best, arg);
  }

  // kExact: what the stitch, k_candidates and the epoch guard read of chunk c
  // (the clean exit, the trailing excursion, the epoch stamp; the carry's mode
  // -- they only tell clean from not clean -- and head), and the proof: the
  // chunk's exact exit, the head's value if it never clamped and else the clean
  // exit, must be the kept entry xh[c + 1] of the next chunk of the run, bit for
  // bit (error bit 64: scan_chunked reruns the call on the hint path).  g is
  // the part's view: parts are cut at run boundaries, so a chunk's successor in
  // its run is inside it.
  __device__ __forceinline__ void finish_exact(int64_t c, const Chunks &g, const P1 &o, const Carry &cr,
                                               const double *__restrict__ xh, unsigned int *__restrict__ err) {
    o.cexit[c] = prev;
    o.special[c] = special ? 1 : 0;
    o.ep[c] = o.epoch;
    if (prev > 0) {
      o.tbeg[c] = beg; o.tmax[c] = best; o.targ[c] = arg;
    } else {
      o.tbeg[c] = -1; o.tmax[c] = 0.0; o.targ[c] = 0;
    }
    cr.mode[c] = (uint8_t)(hclean ? kModeClean : kModeU);
    cr.hq[c] = hclean ? -1 : hx.hq;  // (clean: the values head_one writes)
    cr.hmax[c] = hx.hmax;
    cr.harg[c] = hx.harg;
    const double ex = (hclean || hx.hq >= 0) ? prev : hx.T;
    if (c + 1 < g.nch && g.run[c + 1] == g.run[c] &&
        __double_as_longlong(ex) != __double_as_longlong(xh[c + 1]))
      atomicOr(err, 64u);
  }
};

// The packed window of the small-k passes, 16 scan indices per batch: their
// k-mers (k <= 16) from one 64-bit window of packed bases, three words loaded
// one batch ahead (words past the last one, total >> 4, read it again).
struct Window16 {
  const uint32_t *__restrict__ packed;
  int64_t last;
  uint3 cur;

  __device__ __forceinline__ uint3 load3(int64_t q) const {
    const int64_t w = q >> 4;
    return make_uint3(packed[min(w, last)], packed[min(w + 1, last)], packed[min(w + 2, last)]);
  }
  __device__ __forceinline__ Window16(const uint32_t *__restrict__ pk, int64_t total, int64_t q0)
      : packed(pk), last(total >> 4) {
    cur = load3(q0);
  }
  // the 32 bases from q on, first base most significant; q + 16 comes next
  __device__ __forceinline__ uint64_t take(int64_t q) {
    const uint3 nxt = load3(q + 16);
    const uint32_t bp = 2u * (uint32_t)(q & 15);
    const uint64_t x = ((((uint64_t)cur.x << 32) | cur.y) << bp) | (((uint64_t)cur.z << bp) >> 32);
    cur = nxt;
    return x;
  }
};


// A closed excursion of a chunk's clean trajectory (chunk-relative beg, arg,
// end) is kept as a candidate if it could emit a region or (tr_lr) needs a
// rescan; first = the chunk starts its run.
__device__ __forceinline__ bool cand_wanted(const EmitCfg &ec, bool first, int64_t start, int beg, int arg, int end,
                                            double best) {
  const int64_t f = first ? start : -1;
  const Emission e = decide(ec, f, start + beg, start + arg, best, start + end, true);
  return e.reg || e.res;
}

// J = scan indices served by one table read: 1 reads the base table
// (uint16 code or FP64 value per index); J >= 2 reads the expanded table
// entry of the (k+J-1)-mer that spans J consecutive indices.
// kLds: the compressed LUT is copied to LDS once per 1024-lane block
// (random LUT reads hit LDS banks instead of the L1/L2 path).
// The per-index step is hand-written here, not P1Lane's (same bits, see the
// comment there): on the walker k_pass1<1, *> went from 181 / 191 VGPRs and 2
// waves per SIMD to 147-161 and 3, and the unexpanded k = 13 scan of 3.09 Gbp
// took 89.0 instead of 87.5 ms per step.
template <int J, bool kCompressed, bool kLds>
__global__ void __launch_bounds__(J == 1 ? 256 : 1024) k_pass1(Chunks g, const uint8_t *__restrict__ seq, int64_t total,
                                                int k, TableView tv, uint16_t *__restrict__ codes,
                                                EmitCfg ec, uint32_t *__restrict__ visits, P1 o, Cand cand,
                                                int64_t c0, int tail_only) {
  constexpr int G = (J == 1) ? 16 : (J >= 3 ? 4 : 8);  // table reads in flight per lane and batch
  constexpr int PB = G * J;             // scan indices per batch (16, 16, 12, 16, 20)
  constexpr bool k12 = (J == 5);        // 12-bit codes with escapes (kCompressed only)
  using GC = typename std::conditional<(J >= 3), uint64_t, uint32_t>::type;  // (k+J-1)-mer code
  __shared__ double s_lut[kLds ? kLdsLutMax : 1];
  __shared__ double s_lut12[k12 ? 4096 : 1];
  __shared__ uint16_t s_map12[k12 ? 4096 : 1];
  if (kLds) {
    for (int i = threadIdx.x; i < tv.nlut; i += blockDim.x) s_lut[i] = tv.lut[i];
  }
  if (k12) {
    for (int i = threadIdx.x; i < 4096; i += blockDim.x) {
      s_lut12[i] = tv.lut12[i];
      s_map12[i] = tv.map12[i];
    }
  }
  if (kLds || k12) __syncthreads();
  const int64_t c = c0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= g.nch) return;
  // tail_only: the chunks k_pass1p leaves (reads past the buffer end)
  if (tail_only && g.start[c] + g.n[c] + kP1TailMargin <= total) return;
  const int kx = k + J - 1;
  const GC xmask = (2 * kx >= 8 * (int)sizeof(GC)) ? ~(GC)0 : (((GC)1 << (2 * kx)) - 1);
  const uint32_t kmask = (1u << (2 * k)) - 1u;
  const int64_t start = g.start[c];
  const int n = g.n[c];
  const bool first = c == 0 || g.run[c - 1] != g.run[c];  // the chunk starts its run
  GC gcode = (GC)prime_code_guarded64(seq, start - k, kx, total);  // (k+J-1)-mer of group 0
  // tr_lr: the run's first scan index scores the first k-mer's own score
  const double first_val = (ec.trlr && first) ? ec.ks[(uint32_t)(gcode >> (2 * (J - 1))) & kmask] : 0.0;
  double prev = 0.0, best = 0.0;
  int beg = -1, arg = 0;
  double asum = 0.0, pmin = INFINITY, pmax = -INFINITY, sabs = 0.0;
  int parg = 0;
  bool special = false;
  for (int b0 = 0; b0 < n; b0 += PB) {
    uint8_t by[32];  // bytes rolled in by groups 1..G: start + b0 + J - 1 + [0, PB)
    load16(seq, start + b0 + J - 1, total, by);
    if (PB > 16) load16(seq, start + b0 + J - 1 + 16, total, by + 16);
    GC gc[G];
#pragma unroll
    for (int gi = 0; gi < G; ++gi) {
      gc[gi] = gcode;
#pragma unroll
      for (int t = 0; t < J; ++t) gcode = ((gcode << 2) | enc(by[gi * J + t])) & xmask;
    }
    double v[PB];
    uint16_t q[PB];
#pragma unroll
    for (int gi = 0; gi < G; ++gi) {
      const bool live = b0 + gi * J < n;
      if (J == 1) {
        if (kCompressed) q[gi] = live ? tv.codes[gc[gi]] : (uint16_t)0;
        else v[gi] = live ? tv.vals[gc[gi]] : 0.0;
      } else if (kCompressed && k12) {
        const uint64_t e = live ? reinterpret_cast<const uint64_t *>(tv.ext)[gc[gi]] : 0ull;
#pragma unroll
        for (int t = 0; t < J; ++t) {
          const uint32_t c12 = (uint32_t)(e >> (12 * t)) & 0xfffu;
          if (c12 != 0xfffu) {
            q[gi * J + t] = s_map12[c12];
            v[gi * J + t] = s_lut12[c12];
          } else {  // value outside the 12-bit set: base table
            const uint16_t qe = tv.codes[(uint32_t)(gc[gi] >> (2 * (J - 1 - t))) & kmask];
            q[gi * J + t] = qe;
            v[gi * J + t] = tv.lut[qe];
          }
        }
      } else if (kCompressed) {
        uint64_t e = 0;
        if (live) e = (J <= 2) ? (uint64_t)reinterpret_cast<const uint32_t *>(tv.ext)[gc[gi]]
                               : reinterpret_cast<const uint64_t *>(tv.ext)[gc[gi]];
#pragma unroll
        for (int t = 0; t < J; ++t) q[gi * J + t] = (uint16_t)(e >> (16 * t));
      } else {
        double2 e0 = make_double2(0.0, 0.0), e1 = e0;
        if (live) {
          const double2 *E = reinterpret_cast<const double2 *>(tv.ext);
          if (J <= 2) {
            e0 = E[gc[gi]];
          } else {
            e0 = E[2 * (size_t)gc[gi]];
            e1 = E[2 * (size_t)gc[gi] + 1];
          }
        }
        const double ev[4] = {e0.x, e0.y, e1.x, e1.y};
#pragma unroll
        for (int t = 0; t < J; ++t) v[gi * J + t] = ev[t];
      }
    }
    if (kCompressed) {
#pragma unroll
      for (int j = 0; j < PB; ++j)
        if (!k12) v[j] = kLds ? s_lut[q[j]] : tv.lut[q[j]];
#pragma unroll
      for (int r4 = 0; r4 < PB / 4; ++r4) {
        if (codes && b0 + 4 * r4 < CH) {
          uint2 w;
          w.x = q[4 * r4 + 0] | ((uint32_t)q[4 * r4 + 1] << 16);
          w.y = q[4 * r4 + 2] | ((uint32_t)q[4 * r4 + 3] << 16);
          *reinterpret_cast<uint2 *>(codes + code_slot(c, b0 + 4 * r4)) = w;
        }
      }
    }
    if (ec.trlr && first && b0 == 0) v[0] = first_val;
#pragma unroll
    for (int j = 0; j < PB; ++j) {
      const int i = b0 + j;
      if (i < n) {
        if (visits) atomicAdd(&visits[(uint32_t)(gc[j / J] >> (2 * (J - 1 - j % J))) & kmask], 1u);
        const double s = v[j];
        asum += s;
        pmin = fmin(pmin, asum);
        parg = asum > pmax ? i : parg;
        pmax = fmax(pmax, asum);
        sabs += fabs(s);
        special |= !isfinite(s);
        const double t = prev + s;
        const double S = t > 0 ? t : 0.0;
        if (prev == 0 && S > 0) {
          beg = i; arg = i; best = S;
        } else if (prev > 0 && S == 0) {
          if (cand_wanted(ec, first, start, beg, arg, i, best)) cand_put(cand, start, beg, arg, i, best);
          beg = -1;
        } else if (S > best) {
          best = S; arg = i;
        }
        prev = S;
      }
    }
  }
  p1_put(o, c, prev, asum, pmin, pmax, parg, sabs, special, beg, best, arg);
}

// Software-pipelined gather pass for expanded compressed tables (J >= 2):
// the reads of batch b+1 (and the sequence bytes of batch b+2) are issued
// before batch b is consumed, so every wave keeps its next table reads in
// flight while it runs the trajectory.  Loads are in-order on vmcnt, so the
// loop body must never wait on a load issued after those reads: the escape
// codes of batch b (J = 5: the first two escaped slots of the batch) are
// issued before them, all loads are unconditional (dead groups read entry 0)
// so the wait counts stay static, and the rare paths that do load (a third
// escape in one batch, the candidate append) drain explicitly inside the
// branch.  Results are identical to k_pass1.
template <int J, bool kLds, bool kTrlr>
__global__ void __launch_bounds__(kP1Block) k_pass1p(Chunks g, const uint8_t *__restrict__ seq, int64_t total, int k,
                                                 TableView tv, EmitCfg ec,
                                                 uint32_t *__restrict__ visits, P1 o, Cand cand,
                                                 const uint32_t *__restrict__ packed, const double *__restrict__ xh,
                                                 SummP1 sp) {
  constexpr int G = kP1GSumm;           // table reads per batch
  constexpr int BS = kP1Block;          // lanes per block (LDS staging stride)
  constexpr int PB = G * J;             // scan indices per batch (8, 12, 16, 20)
  constexpr bool k12 = (J == 5);        // 12-bit codes with escapes
  using GC = typename std::conditional<(J >= 3), uint64_t, uint32_t>::type;
  using EW = typename std::conditional<(J >= 3), uint64_t, uint32_t>::type;  // entry word
  // LDS: the value LUT (all distinct values, kLds), the 12-bit code maps
  // (J = 5; with kLds the 12-bit values are read through s_lut[s_map12[]] to
  // leave room for the staged packed bases) and the staged bases.
  constexpr bool kLut12 = k12 && !(kLds && kP1Stage);
  __shared__ double s_lut[kLds ? kLdsLutMax : 1];
  __shared__ double s_lut12[kLut12 ? 4096 : 1];
  __shared__ uint16_t s_map12[k12 ? 4096 : 1];
  __shared__ uint32_t s_pk[kP1Stage ? kP1StageWords * BS : 1];  // [word][lane]: conflict-free
  if (kLds)
    for (int i = threadIdx.x; i < tv.nlut; i += blockDim.x) s_lut[i] = tv.lut[i];
  if (k12)
    for (int i = threadIdx.x; i < 4096; i += blockDim.x) {
      if (kLut12) s_lut12[i] = tv.lut12[i];
      s_map12[i] = tv.map12[i];
    }
  if (kLds || k12) __syncthreads();
  const int64_t c = g.c0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= g.nch) return;
  const EW *__restrict__ ext = reinterpret_cast<const EW *>(tv.ext);
  const int kx = k + J - 1;
  const GC xmask = (2 * kx >= 8 * (int)sizeof(GC)) ? ~(GC)0 : (((GC)1 << (2 * kx)) - 1);
  const uint32_t kmask = (1u << (2 * k)) - 1u;
  const int64_t start = g.start[c];
  const int n = g.n[c];
  const bool first = c == 0 || g.run[c - 1] != g.run[c];  // the chunk starts its run
  GC gcode = (GC)prime_code_guarded64(seq, start - k, kx, total);  // (k+J-1)-mer of group 0
  // tr_lr: the run's first scan index scores the first k-mer's own score
  const double first_val = (kTrlr && first) ? ec.ks[(uint32_t)(gcode >> (2 * (J - 1))) & kmask] : 0.0;
  // tail lanes (reads could pass the end of the buffer) are left to k_pass1
  if (start + n + kP1TailMargin > total) {
    sp.e[2 * c] = sp.e[2 * c + 1] = INT32_MIN;  // no pass-1 summary (the workspace is reused)
    return;
  }
  // Batch m rolls the 2-bit codes of bases [q0 + m*PB, q0 + m*PB + PB) in:
  // three packed words from word (q0 + m*PB) >> 4 (one load, 96 bits >= the
  // 2*PB <= 40 bits at any offset), so a lane touches one or two 128-B lines
  // of packed codes over its whole chunk.
  const int64_t q0 = start + J - 1;
  const int64_t w0 = q0 >> 4;
  uint32_t *const pk = s_pk + threadIdx.x;
  if (kP1Stage) {  // (the tail margin keeps these 20 words inside the packed array)
#pragma unroll
    for (int i = 0; i < kP1StageWords / 4; ++i) {
      const u32x4a4 v4 = *reinterpret_cast<const u32x4a4 *>(packed + w0 + 4 * i);
      pk[(4 * i + 0) * BS] = v4.x;
      pk[(4 * i + 1) * BS] = v4.y;
      pk[(4 * i + 2) * BS] = v4.z;
      pk[(4 * i + 3) * BS] = v4.w;
    }
  }
  // window of 3 words at packed word wq (staged: clamped to the lane's slot;
  // only prefetches past the chunk's last batch are clamped, and unused)
  constexpr int WW = (2 * PB > 64) ? 5 : 3;  // window words: 2 x 64 bits of bases when PB > 32
  struct Win { uint32_t w[WW]; };
  auto window = [&](int64_t wq) -> Win {
    Win r;
    if (!kP1Stage) {
#pragma unroll
      for (int q = 0; q < WW; ++q) r.w[q] = packed[wq + q];
      return r;
    }
    const int i = min((int)(wq - w0), kP1StageWords - WW);
#pragma unroll
    for (int q = 0; q < WW; ++q) r.w[q] = pk[(i + q) * BS];
    return r;
  };
  // bases [qb, qb + 64) of window wn (qb & 15 = the offset in its first word)
  auto bits = [&](const Win &wn, int64_t qb, uint64_t &lo, uint64_t &hi) {
    const uint32_t bp = 2u * (uint32_t)(qb & 15);
    lo = ((((uint64_t)wn.w[0] << 32) | wn.w[1]) << bp) | (((uint64_t)wn.w[2] << bp) >> 32);
    hi = 0;
    if (WW == 5) hi = ((((uint64_t)wn.w[2] << 32) | wn.w[3]) << bp) | (((uint64_t)wn.w[4] << bp) >> 32);
  };
  // the 2J bits of group gi (bases gi*J .. gi*J + J - 1 of the batch)
  auto field = [&](uint64_t lo, uint64_t hi, int gi) -> uint64_t {
    const int e = 2 * J * (gi + 1);  // end bit of the group in the 128-bit lo:hi
    uint64_t f;
    if (e <= 64) f = lo >> (64 - e);
    else if (e - 2 * J >= 64) f = hi >> (128 - e);
    else f = (lo << (e - 64)) | (hi >> (128 - e));
    return f & ((1ull << (2 * J)) - 1ull);
  };
  Win win = window(q0 >> 4);
  GC gc[G];
  EW e[G];
  {
    uint64_t lo, hi;
    bits(win, q0, lo, hi);
#pragma unroll
    for (int gi = 0; gi < G; ++gi) {
      gc[gi] = gcode;
      gcode = ((gcode << (2 * J)) | (GC)field(lo, hi, gi)) & xmask;
    }
  }
  // prologue: reads of batch 0, window of batch 1
  win = window((q0 + PB) >> 4);
#pragma unroll
  for (int gi = 0; gi < G; ++gi) e[gi] = ext[(gi * J < n) ? gc[gi] : (GC)0];
  double prev = 0.0, best = 0.0;
  int beg = -1, arg = 0;
  double asum = 0.0, pmin = INFINITY, pmax = -INFINITY, sabs = 0.0;
  int parg = 0;
  bool special = false;
  // A deliberate copy of P1Lane (state, init, step, finish; keep them in
  // step): as locals the non-finite flag is a lane mask, as a member updated
  // in place it is a byte in a VGPR, and J = 5 sits at the 128-VGPR cap of a
  // 1024-lane block.  Scratch bytes per lane of k_pass1p<5, kLds, kTrlr> for
  // (kLds, kTrlr) = (0, 0) (0, 1) (1, 0) (1, 1): 20 28 20 28 on the walker,
  // 12 28 12 20 with this copy (-Rpass-analysis=kernel-resource-usage).
  int se = INT32_MIN, se2 = INT32_MIN;
  double sC = 0.0, sH = 0.0, scur = 0.0, smx = -INFINITY, smn = INFINITY;
  double sC2 = 0.0, sH2 = 0.0, scur2 = 0.0, smx2 = -INFINITY, smn2 = INFINITY;
  double smaxabs = 0.0;  // max |s| (the rounding of every step, both binades)
  int sarg = 0, sarg2 = 0;
  bool sbad = false, sbad2 = false;
  {
    const double x = xh ? xh[c] : 0.0;  // (no predictor: no summaries)
    if (x >= kP1SumMin && x < 1.0e15) {
      se = binade_of(x);
      sC = 1.5 * ldexp(1.0, se);
      sH = ldexp(1.0, se - 53);
      const double lo = ldexp(1.0, se);
      if (x < lo * (1.0 + kP1Margin)) se2 = se - 1;
      else if (x > 2.0 * lo * (1.0 - kP1Margin)) se2 = se + 1;
      if (se2 != INT32_MIN) {
        sC2 = 1.5 * ldexp(1.0, se2);
        sH2 = ldexp(1.0, se2 - 53);
      }
    }
  }
  for (int b0 = 0; b0 < n; b0 += PB) {
    // 1. escape reads of batch b first: the first two escaped slots of the
    //    batch (a third one, ~6e-5 of lane-batches, loads inline)
    int ja = PB, jb = PB;
    uint32_t qa = 0, qb = 0;
    if (k12) {
      uint64_t m = 0;
#pragma unroll
      for (int gi = 0; gi < G; ++gi)
#pragma unroll
        for (int t = 0; t < J; ++t)
          if (((uint32_t)(e[gi] >> (12 * t)) & 0xfffu) == 0xfffu) m |= 1ull << (gi * J + t);
      const uint64_t m2 = m & (m - 1ull);
      ja = m ? __builtin_ctzll(m) : PB;
      jb = m2 ? __builtin_ctzll(m2) : PB;
      // k-mer of slot jj (index 0 when absent): group jj / 5, offset jj % 5
      // k-mer of slot jj (index 0 when absent), selected among per-group
      // values (not array elements, so gc[] is never indexed dynamically)
      auto kmer_of = [&](int jj) -> uint32_t {
        uint32_t km = 0;
#pragma unroll
        for (int q = 0; q < G; ++q) {
          const uint32_t t = (uint32_t)(jj - q * J);  // < J iff slot jj is in group q
          const uint32_t kq = (uint32_t)(gc[q] >> (2 * (J - 1 - (t < J ? t : 0u)))) & kmask;
          km = t < (uint32_t)J ? kq : km;
        }
        return km;
      };
      qa = tv.codes[kmer_of(ja)];
      qb = tv.codes[kmer_of(jb)];
    }
    // 2. reads of batch b+1 (entry 0 where the group is past the chunk end)
    GC gn[G];
    EW en[G];
    {
      uint64_t lo, hi;
      bits(win, q0 + b0 + PB, lo, hi);
#pragma unroll
      for (int gi = 0; gi < G; ++gi) {
        gn[gi] = gcode;
        gcode = ((gcode << (2 * J)) | (GC)field(lo, hi, gi)) & xmask;
      }
    }
#pragma unroll
    for (int gi = 0; gi < G; ++gi) {
      en[gi] = ext[(b0 + PB + gi * J < n) ? gn[gi] : (GC)0];
    }
    // 3. window of batch b+2
    win = window((q0 + b0 + 2 * PB) >> 4);
    // 4. batch b group by group: values, trajectory
#pragma unroll
    for (int gi = 0; gi < G; ++gi) {
#pragma unroll
      for (int t = 0; t < J; ++t) {
        const int j = gi * J + t;
        uint32_t qq;
        double s;
        if (k12) {
          const uint32_t c12 = (uint32_t)(e[gi] >> (12 * t)) & 0xfffu;
          if (c12 != 0xfffu) {
            qq = s_map12[c12];
            s = kLut12 ? s_lut12[c12] : s_lut[qq];
          } else {
            qq = (j == ja) ? qa : qb;
            if (j != ja && j != jb) {  // third escape of the batch: load and drain here
              qq = tv.codes[(uint32_t)(gc[gi] >> (2 * (J - 1 - t))) & kmask];
              __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): never at the loop's shared waits
            }
            s = kLds ? s_lut[qq] : tv.lut[qq];
          }
        } else {
          qq = (uint32_t)(e[gi] >> (16 * t)) & 0xffffu;
          s = kLds ? s_lut[qq] : tv.lut[qq];
        }
        if (kTrlr && first && b0 == 0 && j == 0) s = first_val;
        const int i = b0 + j;
        if (i < n) {
          if (visits) atomicAdd(&visits[(uint32_t)(gc[gi] >> (2 * (J - 1 - t))) & kmask], 1u);
          asum += s;
          pmin = asum < pmin ? asum : pmin;
          parg = asum > pmax ? i : parg;
          pmax = asum > pmax ? asum : pmax;
          sabs += fabs(s);
          special |= !isfinite(s);
          if (se != INT32_MIN) {
            const double r = (s + sC) - sC;
            sbad |= fabs(r - s) == sH;
            smaxabs = fmax(smaxabs, fabs(s));
            scur += r;
            const bool su = scur > smx;
            smx = su ? scur : smx;
            sarg = su ? i : sarg;
            smn = fmin(smn, scur);
            if (se2 != INT32_MIN) {
              const double r2 = (s + sC2) - sC2;
              sbad2 |= fabs(r2 - s) == sH2;
              scur2 += r2;
              const bool su2 = scur2 > smx2;
              smx2 = su2 ? scur2 : smx2;
              sarg2 = su2 ? i : sarg2;
              smn2 = fmin(smn2, scur2);
            }
          }
          const double tt = prev + s;
          const double S = tt > 0 ? tt : 0.0;
          const bool open = (prev == 0) & (S > 0);
          const bool close = (prev > 0) & (S == 0);
          const int f0 = first ? 0 : -1;
          const long long ml = kTrlr ? ec.min_len : 0;
          const bool want =
              kTrlr ? (close & (((long long)((arg != f0 ? arg - 1 : arg) - (beg != f0 ? beg - 1 : beg)) >= ml) |
                                ((long long)((i != f0 ? i - 1 : i) - (arg != f0 ? arg - 1 : arg) - 1) >=
                                 (ml > 1 ? ml : 1LL))))
                    : (close & ((uint64_t)(int64_t)(arg - beg) >= ec.mw) & (best >= ec.min_score));
          if (want) {
            cand_put(cand, start, beg, arg, i, best);
            __builtin_amdgcn_s_waitcnt(0x0F70);
          }
          const bool up = open | (S > best);
          best = up ? S : best;
          arg = up ? i : arg;
          beg = open ? i : (close ? -1 : beg);
          prev = S;
        }
      }
    }
#pragma unroll
    for (int gi = 0; gi < G; ++gi) {
      gc[gi] = gn[gi];
      e[gi] = en[gi];
    }
  }
  summ_put(sp, c, 0, se, sbad, smaxabs, scur, smx, smn, sarg);
  summ_put(sp, c, 1, se2, sbad2, smaxabs, scur2, smx2, smn2, sarg2);
  p1_put(o, c, prev, asum, pmin, pmax, parg, sabs, special, beg, best, arg);
}

// ------------------------------------------------------------------- P1 (line tables)

// Pass 1 on a line table (ks_table line_kind; k_build_line_u16 / _f64 in
// ks_table.hip): a lane scans its chunk in steps of J = own + LV indices (LV
// = 2 continuation levels for uint16 codes, 1 for FP64 values).  Step s reads
// the line of the m-mer (m = k + own - 1) ending at base start - 1 + sJ +
// own - 1: its own entries are indices sJ .. sJ + own - 1, its continuation
// entries, selected by the next LV bases, the following LV indices.  So the
// step's key is the (k + J - 1)-mer ending at base start + sJ + J - 2, as
// for the expanded tables, and one random 64-B request serves J indices.
// Lines are fetched cooperatively: four lanes load the four 16-B pieces of
// one lane's line (global_load_lds_dwordx4: a wave instruction touches 16
// whole lines; random 64-B lines come at ~50 G/s from a 64-128 GiB table,
// against 25-38 G/s when each lane loads its own entry, tools/probes/line_bench*.hip,
// profiles/r3/line_bench*.txt), straight into a two-slot LDS ring per wave:
// the lines land in lane order (lane L's line at L x 64 B), and the next
// step's lines are in flight while a step is processed.  The loads are inline
// asm (the compiler would otherwise drain every LDS-DMA before each LDS
// read); the only ordinary memory accesses in the loop are the rare candidate
// appends, and the bases come from the packed 2-bit codes loaded into
// registers once per lane.  Same outputs as k_pass1p (kSumm: compressed
// tables also summarise in the predicted binades) / k_pass1pf (FP64).
constexpr int kLineLutMax = 7168;  // LDS LUT entries of the uint16 line pass (ring 96 KiB + 56 KiB)
constexpr int kLineWords = 20;     // packed words per lane: <= 15 + 17 + 255 + J bases

__device__ __forceinline__ uint32_t lds_addr(const void *p) {
  return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void *)p;
}

// One global_load_lds_dwordx4: 16 B from each lane's gsrc to LDS address
// lds + 16 x lane (lds wave-uniform).
__device__ __forceinline__ void glds16(const void *gsrc, uint32_t lds) {
  uint32_t keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(gsrc), "s"(lds)
               : "memory");
}

// The lane's packed 2-bit bases from the word holding base p0 on, kLineWords
// words in registers (guarded at the end of the packed array), and a rolling
// supply: acc holds na bases in its top 2 na bits; refill() appends the next
// word when 16 or fewer are left and shifts the word array down.
struct LaneBases {
  uint32_t a[kLineWords];
  uint64_t acc = 0;
  int na = 0;

  __device__ __forceinline__ void load(const uint32_t *__restrict__ packed, int64_t total, int64_t p0) {
    const int64_t w0 = p0 >> 4, wlast = total >> 4;  // words 0 .. total >> 4 exist
    const int64_t wa = w0 & ~(int64_t)3;
    if (wa + 24 <= wlast + 1) {
      uint32_t v[24];
      const uint4 *P4 = reinterpret_cast<const uint4 *>(packed + wa);
#pragma unroll
      for (int t = 0; t < 6; ++t) {
        const uint4 q = P4[t];
        v[4 * t] = q.x;
        v[4 * t + 1] = q.y;
        v[4 * t + 2] = q.z;
        v[4 * t + 3] = q.w;
      }
      const int off = (int)(w0 - wa);
#pragma unroll
      for (int t = 0; t < kLineWords; ++t)
        a[t] = off == 0 ? v[t] : (off == 1 ? v[t + 1] : (off == 2 ? v[t + 2] : v[t + 3]));
    } else {
#pragma unroll
      for (int t = 0; t < kLineWords; ++t) a[t] = packed[min(w0 + t, wlast)];
    }
    refill();
    refill();
    const int sk = (int)(p0 & 15);
    acc <<= 2 * sk;
    na -= sk;
  }
  __device__ __forceinline__ void refill() {
    const bool r = na <= 16;
    acc |= r ? ((uint64_t)a[0] << (32 - 2 * na)) : 0ull;
    na += r ? 16 : 0;
#pragma unroll
    for (int t = 0; t < kLineWords - 1; ++t) a[t] = r ? a[t + 1] : a[t];
  }
  // nb <= 16 bases (after a refill), first base most significant
  __device__ __forceinline__ uint64_t take(int nb) {
    const uint64_t v = acc >> (64 - 2 * nb);
    acc <<= 2 * nb;
    na -= nb;
    return v;
  }
  // the (kx)-mer of the next kx bases (kx <= 32), then steps of J bases
  __device__ __forceinline__ uint64_t first_key(int kx) {
    uint64_t x = 0;
    for (int left = kx; left > 0;) {
      refill();
      const int nb = left < 16 ? left : 16;
      x = (x << (2 * nb)) | take(nb);
      left -= nb;
    }
    return x;
  }
  __device__ __forceinline__ uint64_t next_key(uint64_t xp, int J, uint64_t xmask) {
    refill();
    return ((xp << (2 * J)) | take(J)) & xmask;
  }
};

// kExact (compressed lines): xh holds the kept exact entries, and the lane
// writes the chunk's Carry fields and verifies its exit (P1Lane::finish_exact).
// kStore (kExact): every step's J codes go to the kept codes kc (kc_slot), one
// store per step, issued after the step's lines of the step after next: the
// stores join the in-order VM counter of the ring's loads, so a step's wait
// lets pass the four loads of the next step and the two stores since (one or
// none in the first two steps, two and no loads in the last).
template <int OWN, bool kF64, bool kLdsLut, bool kTrlr, bool kExact = false, bool kStore = false>
__global__ void __launch_bounds__(kF64 ? 1024 : 768) k_pass1l(Chunks g, int64_t total, int k, TableView tv,
                                                              EmitCfg ec, uint32_t *__restrict__ visits, P1 o,
                                                              Cand cand, const double *__restrict__ xh, SummP1 sp,
                                                              Carry cr, unsigned int *__restrict__ err,
                                                              uint32_t *__restrict__ kc) {
  static_assert(!(kExact && kF64), "exact entries: compressed lines only");
  static_assert(!kStore || (kExact && kLdsLut), "the kept codes are written from exact entries");
  constexpr int BS = kF64 ? 1024 : 768;  // 16 / 12 waves: ring 128 / 96 KiB (+ the LUT)
  constexpr int LV = kF64 ? 1 : 2;
  constexpr int J = OWN + LV;
  constexpr int NS = (CH + J - 1) / J;  // steps per chunk (the same for the whole wave)
  constexpr bool kSumm = !kExact;  // (xh == nullptr: no predicted binades, no summaries)
  constexpr bool kLut = !kF64 && kLdsLut;
  static_assert(kF64 ? OWN + 4 <= 8 : OWN + 20 <= 32, "line layout");
  __shared__ __attribute__((aligned(16))) uint8_t s_ring[(BS / 64) * 2 * 4096];
  __shared__ double s_lut[kLut ? kLineLutMax : 1];
  if (kLut) {
    for (int i = threadIdx.x; i < tv.nlut; i += BS) s_lut[i] = tv.lut[i];
    __syncthreads();
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t c = g.c0 + (int64_t)blockIdx.x * BS + threadIdx.x;
  if (c - lane >= g.nch) return;  // the whole wave is past the end (the other lanes still fetch for theirs)
  const bool live = c < g.nch;
  const int64_t start = live ? g.start[c] : (int64_t)k;
  const int n = live ? g.n[c] : 0;
  const bool first = live && (c == 0 || g.run[c - 1] != g.run[c]);
  const uint32_t kmask = (1u << (2 * k)) - 1u;
  P1Lane<kSumm, kTrlr, kExact> L;
  L.init(start, n, first, live, (live && xh) ? xh[c] : 0.0);
  LaneBases B;
  B.load(g.packed, total, start - k);
  const int kx = k + J - 1;  // key length (<= 17)
  const uint64_t xmask = (1ull << (2 * kx)) - 1ull;
  uint64_t x = B.first_key(kx);  // key of step 0
  // tr_lr: the run's first scan index scores the first k-mer's own score
  const double first_val = (kTrlr && first) ? ec.ks[(uint32_t)(x >> (2 * (J - 1))) & kmask] : 0.0;

  // ---- the ring: lane L's line of slot q at ring + q x 4096 + L x 64
  uint8_t *const ring = s_ring + wv * 8192;
  const uint32_t ring_lds = __builtin_amdgcn_readfirstlane(lds_addr(ring));
  const uint8_t *__restrict__ lines = tv.line;
  auto issue = [&](uint32_t idx, int slot) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t li = (uint32_t)__shfl((int)idx, 16 * q + (lane >> 2));
      glds16(lines + (size_t)li * 64 + (lane & 3) * 16, ring_lds + (uint32_t)(slot * 4096 + q * 1024));
    }
  };
  // keys of the step being processed and of the two in flight
  uint64_t x1 = 0, x2 = 0;
  uint32_t *const kcl = kStore ? kc + kc_slot(live ? c : g.c0, 0, J) : nullptr;
  issue((uint32_t)(x >> (2 * LV)), 0);
  x1 = B.next_key(x, J, xmask);
  issue((uint32_t)(x1 >> (2 * LV)), 1);
  for (int st = 0; st < NS; ++st) {
    const uint64_t xs = x;  // key of this step
    // this step's lines complete (the next step's four loads may stay in flight)
    if constexpr (kStore) {
      if (st + 1 >= NS) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
      else if (st >= 2) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
      else if (st == 1) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    } else {
      if (st + 1 < NS) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    const uint8_t *ln = ring + (st & 1) * 4096 + lane * 64;
    double v[J];
    uint32_t rec[kc_words(J)] = {};
    if (!kF64) {
      uint32_t h[16];  // halfwords 0 .. 15 of the line (own + L1 <= 9 codes: 0 .. 8)
      const uint4 q0 = *reinterpret_cast<const uint4 *>(ln);
      h[0] = q0.x & 0xffffu; h[1] = q0.x >> 16; h[2] = q0.y & 0xffffu; h[3] = q0.y >> 16;
      h[4] = q0.z & 0xffffu; h[5] = q0.z >> 16; h[6] = q0.w & 0xffffu; h[7] = q0.w >> 16;
      if (OWN + 4 > 8) {
        const uint4 q1 = *reinterpret_cast<const uint4 *>(ln + 16);
        h[8] = q1.x & 0xffffu; h[9] = q1.x >> 16; h[10] = q1.y & 0xffffu; h[11] = q1.y >> 16;
        h[12] = q1.z & 0xffffu; h[13] = q1.z >> 16; h[14] = q1.w & 0xffffu; h[15] = q1.w >> 16;
      }
      const uint32_t c1 = (uint32_t)(xs >> 2) & 3u, c2 = (uint32_t)xs & 3u;
      uint32_t cs[J];
#pragma unroll
      for (int t = 0; t < OWN; ++t) cs[t] = h[t];
      cs[OWN] = c1 == 0 ? h[OWN] : (c1 == 1 ? h[OWN + 1] : (c1 == 2 ? h[OWN + 2] : h[OWN + 3]));
      cs[OWN + 1] = *reinterpret_cast<const uint16_t *>(ln + 2 * (OWN + 4 + 4 * c1 + c2));
#pragma unroll
      for (int t = 0; t < J; ++t) v[t] = kLut ? s_lut[cs[t]] : tv.lut[cs[t]];
      if constexpr (kStore) kc_pack<J>(cs, rec);
    } else {
      const double *lv = reinterpret_cast<const double *>(ln);
#pragma unroll
      for (int t = 0; t < OWN; ++t) v[t] = lv[t];
      v[OWN] = lv[OWN + ((int)xs & 3)];
    }
    // the step after next into the slot just read: two steps in flight
    // while this one is processed
    x = x1;
    if (st + 2 < NS) {
      x2 = B.next_key(x1, J, xmask);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the slot's reads are done before it is refilled
      issue((uint32_t)(x2 >> (2 * LV)), st & 1);
      x1 = x2;
    }
    if constexpr (kStore) {
      if (live) kc_store<kc_words(J)>(kcl + (size_t)st * 64 * kc_words(J), rec);
    }
#pragma unroll
    for (int t = 0; t < J; ++t) {
      const int i = st * J + t;
      if (i < n) {
        double sv = v[t];
        if (kTrlr && first && i == 0) sv = first_val;
        if (visits) atomicAdd(&visits[(uint32_t)(xs >> (2 * (J - 1 - t))) & kmask], 1u);
        L.step(sv, i, ec, cand);
      }
    }
  }
  if (!live) return;
  if constexpr (kExact) L.finish_exact(c, g, o, cr, xh, err);
  else L.finish(c, o, sp);
}

// Pass 1 on a wide line table (line_kind 3, 128-B lines, k_build_line_wide):
// own / L1 / L2 entries as 13-bit codes (the uint16 codes of a table with at
// most kLineLutMax distinct values: never an escape), the 64 L3 entries (the
// three-base continuations) as 11-bit codes, 2047 escaping to the base code
// table.  J = own + 3 indices per random request (6 at k = 13: 0.51 G
// requests per 3.06 G indices instead of 0.61 G), at 128 B per request: the
// size at which random lines still come at ~50 G/s (6.4 TB/s,
// profiles/r3/line_bench.txt).  Eight lanes load a line.  A step's L3 escape
// (one at most) is loaded right after its line is decoded
// (global_load_lds_dword of the code pair; a lane without one reads the
// table's first pair), and the step is processed one step later, when it
// has landed: every step then needs one counted wait, whatever the escapes.
// A step needs at most 7 of a line's 32 dwords (own + L1: 0 .. 2; the L2
// and L3 codes: two dwords each), so eight lanes gather exactly those
// dwords of a line (global_load_lds_dword; one line request either way):
// 2 KiB of ring per wave and step instead of 8, which leaves room for 12
// waves per CU beside the LUT (the whole 128-B lines fit 6).
constexpr int kWideBlock = 768;  // 12 waves: ring 48 KiB + LUT 56 KiB + escape slots 6 KiB

// One global_load_lds_dword: 4 B from each lane's gsrc to LDS lds + 4 x lane.
__device__ __forceinline__ void glds4(const void *gsrc, uint32_t lds) {
  uint32_t keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(gsrc), "s"(lds)
               : "memory");
}

// kExact: as k_pass1l's.  kStore (kExact): a step's J codes, the escaped L3
// code among them, go to the kept codes kc where the step is processed, one
// iteration late: one store per step after the eight loads of the step after
// next, so a step's wait lets pass those eight and the one store since (none in
// the first two steps; in the last step and after the loop the one store).
template <int OWN, bool kTrlr, bool kExact = false, bool kStore = false>
__global__ void __launch_bounds__(kWideBlock) k_pass1w(Chunks g, int64_t total, int k, TableView tv, EmitCfg ec,
                                                       uint32_t *__restrict__ visits, P1 o, Cand cand,
                                                       const double *__restrict__ xh, SummP1 sp, Carry cr,
                                                       unsigned int *__restrict__ err, uint32_t *__restrict__ kc) {
  static_assert(!kStore || kExact, "the kept codes are written from exact entries");
  constexpr int BS = kWideBlock;
  constexpr int J = OWN + 3;
  constexpr int NS = (CH + J - 1) / J;
  constexpr int N13 = OWN + 20;
  constexpr uint32_t B3 = 13 * N13;  // first L3 bit
  constexpr int NO = (13 * (OWN + 4) + 31) / 32;  // dwords of own + L1 (3 or 4)
  static_assert(NO + 4 <= 8, "own + L1, L2, L3 dwords in 8 lanes");
  __shared__ __attribute__((aligned(16))) uint8_t s_ring[(BS / 64) * 2 * 2048];
  __shared__ __attribute__((aligned(16))) uint32_t s_esc[(BS / 64) * 2 * 64];
  __shared__ double s_lut[kLineLutMax];
  for (int i = threadIdx.x; i < tv.nlut; i += BS) s_lut[i] = tv.lut[i];
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t c = g.c0 + (int64_t)blockIdx.x * BS + threadIdx.x;
  if (c - lane >= g.nch) return;
  const bool live = c < g.nch;
  const int64_t start = live ? g.start[c] : (int64_t)k;
  const int n = live ? g.n[c] : 0;
  const bool first = live && (c == 0 || g.run[c - 1] != g.run[c]);
  const uint32_t kmask = (1u << (2 * k)) - 1u;
  P1Lane<!kExact, kTrlr, kExact> L;
  L.init(start, n, first, live, (live && xh) ? xh[c] : 0.0);
  LaneBases B;
  B.load(g.packed, total, start - k);
  const int kx = k + J - 1;  // key length (<= 18)
  const uint64_t xmask = (1ull << (2 * kx)) - 1ull;
  uint64_t x = B.first_key(kx);
  const double first_val = (kTrlr && first) ? ec.ks[(uint32_t)(x >> (2 * (J - 1))) & kmask] : 0.0;

  uint8_t *const ring = s_ring + wv * 4096;
  uint32_t *const esc = s_esc + wv * 128;
  const uint32_t ring_lds = __builtin_amdgcn_readfirstlane(lds_addr(ring));
  const uint32_t esc_lds = __builtin_amdgcn_readfirstlane(lds_addr(esc));
  const uint8_t *__restrict__ lines = tv.line;
  // the dwords a step reads from its line (key xk): 0 .. NO - 1, the L2
  // code's two, the L3 code's two (a spare lane reloads dword 0)
  auto dwords = [&](uint64_t xk) -> uint32_t {
    const uint32_t c1 = (uint32_t)(xk >> 4) & 3u, c2 = (uint32_t)(xk >> 2) & 3u, c3 = (uint32_t)xk & 3u;
    const uint32_t d2 = (13u * (OWN + 4 + 4 * c1 + c2)) >> 5, d3 = (B3 + 11u * (16 * c1 + 4 * c2 + c3)) >> 5;
    return d2 | (d3 << 8);
  };
  auto issue = [&](uint64_t xk, int slot) {
    const uint32_t idx = (uint32_t)(xk >> 6), dd = dwords(xk);
    const int j = lane & 7;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int ow = 8 * q + (lane >> 3);
      const uint32_t li = (uint32_t)__shfl((int)idx, ow);
      const uint32_t od = (uint32_t)__shfl((int)dd, ow);
      const uint32_t d2 = od & 0xffu, d3 = od >> 8;
      const uint32_t dw = j < NO ? (uint32_t)j
                                 : (j < NO + 2 ? d2 + (uint32_t)(j - NO)
                                               : (j < NO + 4 ? min(d3 + (uint32_t)(j - NO - 2), 31u) : 0u));
      glds4(lines + (size_t)li * 128 + dw * 4, ring_lds + (uint32_t)(slot * 2048 + q * 256));
    }
  };
  // the step processed one iteration late: its values, key, escape
  double vp[J];
  uint64_t xp = 0;
  bool ep = false;
  constexpr int KW = kc_words(J);
  uint32_t *const kcl = kStore ? kc + kc_slot(live ? c : g.c0, 0, J) : nullptr;
  uint32_t recp[KW] = {};  // kStore: the late step's record (its L3 code 0 where it escaped)
  auto process = [&](int sp_, const double *vv, uint64_t xk, bool e) {
    double v5 = vv[J - 1];
    uint32_t c5 = 0;
    if (e) {  // the escaped L3 value: its code pair landed in the escape slot
      const uint32_t pr = esc[(sp_ & 1) * 64 + lane];
      const uint32_t km = (uint32_t)xk & kmask;
      c5 = (km & 1u) ? (pr >> 16) : (pr & 0xffffu);
      v5 = s_lut[c5];
    }
    if constexpr (kStore) {
      uint32_t rec[KW];
#pragma unroll
      for (int q = 0; q < KW; ++q) rec[q] = recp[q];
      rec[(J - 1) / 2] |= c5 << (16 * ((J - 1) & 1));
      if (live) kc_store<KW>(kcl + (size_t)sp_ * 64 * KW, rec);
    }
#pragma unroll
    for (int t = 0; t < J; ++t) {
      const int i = sp_ * J + t;
      if (i < n) {
        double sv = t == J - 1 ? v5 : vv[t];
        if (kTrlr && first && i == 0) sv = first_val;
        if (visits) atomicAdd(&visits[(uint32_t)(xk >> (2 * (J - 1 - t))) & kmask], 1u);
        L.step(sv, i, ec, cand);
      }
    }
  };
  uint64_t x1 = 0, x2 = 0;
  issue(x, 0);
  x1 = B.next_key(x, J, xmask);
  issue(x1, 1);
  for (int st = 0; st < NS; ++st) {
    const uint64_t xs = x;
    // this step's lines and the previous step's escape complete (the next
    // step's eight loads may stay in flight)
    if constexpr (kStore) {
      if (st + 1 >= NS) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
      else if (st >= 2) asm volatile("s_waitcnt vmcnt(9)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    } else {
      if (st + 1 < NS) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    const uint8_t *ln = ring + (st & 1) * 2048 + lane * 32;  // the step's 8 dwords (dwords())
    double v[J];
    uint32_t rec[KW] = {};
    bool e = false;
    {
      const uint4 q0 = *reinterpret_cast<const uint4 *>(ln);
      const uint4 q1 = *reinterpret_cast<const uint4 *>(ln + 16);
      const uint32_t D[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
      const uint64_t lo = (uint64_t)D[0] | ((uint64_t)D[1] << 32);
      const uint64_t hi = (uint64_t)D[2] | (NO > 3 ? ((uint64_t)D[3] << 32) : 0ull);
      auto f13 = [&](int b) -> uint32_t {  // static b < 128 - 13
        const uint64_t w = b < 64 ? ((lo >> b) | (b > 51 ? (hi << (64 - b)) : 0ull)) : (hi >> (b - 64));
        return (uint32_t)w & 0x1fffu;
      };
      const uint32_t c1 = (uint32_t)(xs >> 4) & 3u, c2 = (uint32_t)(xs >> 2) & 3u, c3 = (uint32_t)xs & 3u;
      uint32_t cs[J];
#pragma unroll
      for (int t = 0; t < OWN; ++t) cs[t] = f13(13 * t);
      const uint32_t l0 = f13(13 * OWN), l1 = f13(13 * (OWN + 1)), l2 = f13(13 * (OWN + 2)),
                     l3 = f13(13 * (OWN + 3));
      cs[OWN] = c1 == 0 ? l0 : (c1 == 1 ? l1 : (c1 == 2 ? l2 : l3));
      const uint32_t b2 = 13u * (OWN + 4 + 4 * c1 + c2), b3 = B3 + 11u * (16 * c1 + 4 * c2 + c3);
      cs[OWN + 1] = (uint32_t)(((uint64_t)D[NO] | ((uint64_t)D[NO + 1] << 32)) >> (b2 & 31)) & 0x1fffu;
      const uint32_t c11 = (uint32_t)(((uint64_t)D[NO + 2] | ((uint64_t)D[NO + 3] << 32)) >> (b3 & 31)) & 0x7ffu;
      e = c11 == 0x7ffu;
      cs[OWN + 2] = e ? 0u : c11;
#pragma unroll
      for (int t = 0; t < J; ++t) v[t] = s_lut[cs[t]];
      if constexpr (kStore) kc_pack<J>(cs, rec);
    }
    // this step's escape (every lane: a lane without one reads the first pair)
    {
      const uint32_t km = (uint32_t)xs & kmask;
      const uint16_t *src = e ? tv.codes + (km & ~1u) : tv.codes;
      glds4(src, esc_lds + (uint32_t)((st & 1) * 256));
    }
    x = x1;
    if (st + 2 < NS) {
      x2 = B.next_key(x1, J, xmask);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the slot's reads are done before it is refilled
      issue(x2, st & 1);
      x1 = x2;
    }
    if (st > 0) process(st - 1, vp, xp, ep);
#pragma unroll
    for (int t = 0; t < J; ++t) vp[t] = v[t];
    if constexpr (kStore) {
#pragma unroll
      for (int q = 0; q < KW; ++q) recp[q] = rec[q];
    }
    xp = xs;
    ep = e;
  }
  // the last escape (kStore: the store after it may stay in flight)
  if constexpr (kStore) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  process(NS - 1, vp, xp, ep);
  if (!live) return;
  if constexpr (kExact) L.finish_exact(c, g, o, cr, xh, err);
  else L.finish(c, o, sp);
}

// Pass 1 from the kept codes (ScanPlan::codes_read): a repeated scan of a
// genome / table pair whose exact entries and per-index codes an earlier scan
// left (k_pass1w / k_pass1l, kStore).  A lane streams its chunk's records
// (kc_slot; a wave reads 64 W contiguous dwords per step, kCodeDepth steps
// ahead), takes the values from the LUT in LDS and walks them as the exact
// flavours of the line passes do: no key, no ring, no table read.  Packed
// bases are read for the first k-mer of a run's first chunk (tr_lr), for the
// visit histogram (kVisits: the line passes' key walk) and for the tripwire:
// the first chunk of every 64 compares its first code with the base code
// table's at its own k-mer (error bit 128).  A tripwire for codes that are not
// the table's -- finish_exact still verifies every exact entry bit for bit
// (bit 64), which catches a wrong code wherever the carried sum does not clamp
// -- not a proof.
// Lanes per block.  The LUT copy (up to 56 KB of the CU's 160 KB of LDS) lets
// two blocks share a CU, whatever their size, so a CU holds 2 x kCodeBlock / 256
// waves per SIMD if the registers allow.  The walk without the visit histogram
// takes 64-82 VGPRs (7-6 waves per SIMD by registers): two 768-lane blocks are 6
// waves per SIMD up to 85 VGPRs, where 1024-lane blocks would leave one block
// (4 waves) on the CU from 65 VGPRs on.  The visit flavours take 78-88 VGPRs,
// one block per CU either way: 1024 lanes keep their 4 waves per SIMD.
constexpr int code_block(bool visits) { return visits ? 1024 : 768; }
// steps per batch; one batch is loaded while the one before is walked (2: 36 KB
// of records in flight per CU; 3 and 4 took 8-16 more VGPRs and gained nothing).
constexpr int kCodeDepth = 2;

// The k-mer (k <= 15) of bases [p0, p0 + k) from the packed words.
__device__ __forceinline__ uint32_t packed_kmer(const uint32_t *__restrict__ packed, int64_t total, int64_t p0, int k) {
  const int64_t w0 = p0 >> 4, wlast = total >> 4;
  const uint64_t x = ((uint64_t)packed[min(w0, wlast)] << 32) | packed[min(w0 + 1, wlast)];
  const int sk = (int)(p0 & 15);
  return (uint32_t)(x >> (64 - 2 * (sk + k))) & ((1u << (2 * k)) - 1u);
}

// One scan index of the reader's walk: P1Lane::step's exact-entry arithmetic on
// the lane's state L -- the same FP64 operations in the same order -- less the
// work whose outcome the wave already knows.  pos is prev > 0 carried from the
// index before (prev is never NaN and never below 0, so prev == 0 is !pos and
// S == 0 is !(S > 0)): open and close are two mask operations.  beg is not
// reset at a close: it is read only while prev > 0, where it is the last open's
// index, and finish_exact writes -1 for prev == 0 itself.  The candidate test
// is decide()'s, as in P1Lane::step, but evaluated only behind a condition it
// implies: kmer_regions needs best >= min_score; tr_lr needs pos(i) - pos(beg)
// >= min_len in both of its clauses, and pos(i) - pos(beg) <= i - beg + 1, so
// i - beg >= min_len - 1 (reach, clamped to int by the caller).  classify
// (uniform over the block): the LUT holds a non-finite value, so every value is
// classified; else special is known before the walk (see k_pass1c).
//
// The carried head is head_step as selects, with no branch (the caller has
// tested i < n): act is hq < 0 carried from the index before.  T moves on after
// the clamp, where nothing reads it (finish_exact takes T only from a head that
// never clamped).  The head is walked at every index, also after every head of
// the wave has clamped: skipping it then takes a second copy of the step per
// wave state, which cost registers and with them resident waves, and pays only
// where all 64 heads of a wave clamp early ("Kept-code
// reader", has the measurement).
template <bool kTrlr>
__device__ __forceinline__ void code_index(P1Lane<false, kTrlr, true> &L, bool &pos, bool &act, double s, int i,
                                           const EmitCfg &ec, int reach, const Cand &cand, bool classify) {
  {
    Head &h = L.hx;
    const double t = h.T + s;
    const bool tp = t > 0;
    const double T = tp ? t : 0.0;
    const bool hup = act & tp & (T > h.hmax);
    h.hq = (act & !tp) ? i : h.hq;
    h.hmax = hup ? T : h.hmax;
    h.harg = hup ? i : h.harg;
    h.T = T;
    act = act & tp;
  }
  if (classify) L.special |= !isfinite(s);
  const double tt = L.prev + s;
  const bool pn = tt > 0;
  const double S = pn ? tt : 0.0;
  const bool open = !pos & pn;
  const bool close = pos & !pn;
  if (kTrlr ? (close & (i - L.beg >= reach)) : (close & (L.best >= ec.min_score))) {
    const int f0 = L.f0, arg = L.arg, beg = L.beg;
    const long long ml = kTrlr ? ec.min_len : 0;
    const bool want =
        kTrlr ? ((((long long)((arg != f0 ? arg - 1 : arg) - (beg != f0 ? beg - 1 : beg)) >= ml) |
                  ((long long)((i != f0 ? i - 1 : i) - (arg != f0 ? arg - 1 : arg) - 1) >= (ml > 1 ? ml : 1LL))))
              : ((uint64_t)(int64_t)(arg - beg) >= ec.mw);
    if (want) cand_put(cand, L.start, beg, arg, i, L.best);
  }
  const bool up = open | (S > L.best);
  L.best = up ? S : L.best;
  L.arg = up ? i : L.arg;
  L.beg = open ? i : L.beg;
  L.prev = S;
  pos = pn;
}

// A wave picks the form of its steps (the choices are uniform over the wave,
// so no lane waits for another's branch):
//  full -- all 64 lanes are live chunks of CH indices (one ballot): no i < n
//    test, a step's J values are read from the LUT ahead of the step's walk
//    (counted LDS waits), and the last step's live count is a constant.  One
//    short chunk or a dead lane sends the wave, and only it, to the guarded
//    form.  Both forms sit in the one chunk loop: every further copy of the loop
//    (one per form, per phase of the head, per class flag) cost about ten
//    VGPRs and with them waves per SIMD;
//  classify, per block -- whether the LUT holds a non-finite value is found
//    while it is staged; a non-finite first value (tr_lr) is noted once.
#define KS_INLINE_LAMBDA __attribute__((always_inline))
template <int J, bool kTrlr, bool kVisits>
__global__ void __launch_bounds__(code_block(kVisits)) k_pass1c(Chunks g, int64_t total, int k, TableView tv, EmitCfg ec,
                                                       uint32_t *__restrict__ visits, P1 o, Cand cand,
                                                       const double *__restrict__ xh, Carry cr,
                                                       unsigned int *__restrict__ err,
                                                       const uint32_t *__restrict__ kc) {
  constexpr int NS = kc_steps(J), W = kc_words(J), D = kCodeDepth;
  constexpr int NG = (NS + D - 1) / D;
  constexpr int kCodeBlock = code_block(kVisits);
  constexpr int LAST = CH - (NS - 1) * J;  // indices of a full chunk's last step
  static_assert((NG - 1) * D < NS && LAST >= 1 && LAST <= J, "only the last batch is short, only the last step partial");
  extern __shared__ double s_clut[];
  int bad = 0;
  for (int i = threadIdx.x; i < tv.nlut; i += kCodeBlock) {
    const double v = tv.lut[i];
    s_clut[i] = v;
    if (!kVisits) bad |= !isfinite(v);
  }
  // (kVisits classifies every value itself: P1Lane::step)
  const bool lut_special = kVisits ? (__syncthreads(), false) : __syncthreads_or(bad) != 0;
  const int64_t c = g.c0 + (int64_t)blockIdx.x * kCodeBlock + threadIdx.x;
  if (c >= g.nch) return;
  const int64_t start = g.start[c];
  const int n = g.n[c];
  const bool first = c == 0 || g.run[c - 1] != g.run[c];
  const uint32_t *__restrict__ rp = kc + kc_slot(c, 0, J);
  uint32_t cur[D][W] = {}, nxt[D][W] = {};
  auto fetch = [&](int gi, uint32_t (&b)[D][W]) KS_INLINE_LAMBDA {
#pragma unroll
    for (int d = 0; d < D; ++d)
      if (gi * D + d < NS) kc_load<W>(rp + (size_t)(gi * D + d) * 64 * W, b[d]);
  };
  fetch(0, cur);
  P1Lane<false, kTrlr, true> L;
  L.init(start, n, first, true, xh[c]);
  // index i's k-mer: bases [start - k + i, start + i)
  double first_val = 0.0;
  if ((kTrlr && first) || (c & 63) == 0) {
    const uint32_t km0 = packed_kmer(g.packed, total, start - k, k);
    if (kTrlr && first) first_val = ec.ks[km0];
    if ((c & 63) == 0 && (cur[0][0] & 0xffffu) != (uint32_t)tv.codes[km0]) atomicOr(err, 128u);
  }
  // (the one value that is not the LUT's: index 0 of a run's first chunk)
  if (!kVisits && kTrlr && first && n > 0) L.special = !isfinite(first_val);
  const long long rl = kTrlr ? (long long)ec.min_len - 1 : 0;
  const int reach = (int)(rl < 0 ? 0 : (rl > CH ? CH + 1 : rl));
  using std::integral_constant;
  using std::true_type;
  using std::false_type;
  // step st (its record: r), LIVE indices of it
  auto step = [&](auto full, auto live, int st, const uint32_t (&r)[W]) KS_INLINE_LAMBDA {
    constexpr bool kFull = decltype(full)::value;
    constexpr int LIVE = decltype(live)::value;
    auto value = [&](int t) KS_INLINE_LAMBDA { return s_clut[(r[t >> 1] >> (16 * (t & 1))) & 0xffffu]; };
    double v[LIVE];
    if (kFull) {  // (guarded: a dead index's code is whatever the slot held, so it is read behind i < n)
#pragma unroll
      for (int t = 0; t < LIVE; ++t) v[t] = value(t);
      if (kTrlr) v[0] = (first && st == 0) ? first_val : v[0];
    }
    bool pos = L.prev > 0, act = L.hx.hq < 0;
#pragma unroll
    for (int t = 0; t < LIVE; ++t) {
      const int i = st * J + t;
      if (kFull || i < n) {
        double sv;
        if (kFull) {
          sv = v[t];
        } else {
          sv = value(t);
          if (kTrlr && first && i == 0) sv = first_val;
        }
        code_index<kTrlr>(L, pos, act, sv, i, ec, reach, cand, lut_special);
      }
    }
  };
  auto walk = [&](bool full) KS_INLINE_LAMBDA {
    auto either = [&](auto live, int st, const uint32_t (&r)[W]) KS_INLINE_LAMBDA {
      if (full) step(true_type{}, live, st, r);
      else step(false_type{}, live, st, r);
    };
    for (int gi = 0; gi < NG - 1; ++gi) {
      fetch(gi + 1, nxt);
      if (full || gi * D * J < n) {  // (a short chunk's later batches: nothing to walk)
#pragma unroll
        for (int d = 0; d < D; ++d) either(integral_constant<int, J>{}, gi * D + d, cur[d]);
      }
#pragma unroll
      for (int d = 0; d < D; ++d)
#pragma unroll
        for (int q = 0; q < W; ++q) cur[d][q] = nxt[d][q];
    }
    if (full || (NG - 1) * D * J < n) {  // the last batch: steps (NG - 1) D .. NS - 1
      auto rest = [&](auto self, auto dc) KS_INLINE_LAMBDA {
        constexpr int d = decltype(dc)::value, st = (NG - 1) * D + d;
        if constexpr (st < NS) {
          either(integral_constant<int, (st == NS - 1 ? LAST : J)>{}, st, cur[d]);
          self(self, integral_constant<int, d + 1>{});
        }
      };
      rest(rest, integral_constant<int, 0>{});
    }
  };
  if constexpr (kVisits) {
    // One global atomic per index bounds this flavour, and the key walk's
    // registers leave no room for the phases (they spilt): P1Lane's own step.
    LaneBases B;
    const uint32_t kmask = (1u << (2 * k)) - 1u;
    const uint64_t xmask = (1ull << (2 * (k + J - 1))) - 1ull;
    B.load(g.packed, total, start - k);
    uint64_t x = B.first_key(k + J - 1);
    for (int gi = 0; gi < NG; ++gi) {
      if (gi + 1 < NG) fetch(gi + 1, nxt);
      if (gi * D * J < n) {  // (a short chunk's later batches: nothing to walk)
#pragma unroll
        for (int d = 0; d < D; ++d) {
          const int st = gi * D + d;
          if (st < NS) {
#pragma unroll
            for (int t = 0; t < J; ++t) {
              const int i = st * J + t;
              if (i < n) {
                const uint32_t code = (cur[d][t >> 1] >> (16 * (t & 1))) & 0xffffu;
                double sv = s_clut[code];
                if (kTrlr && first && i == 0) sv = first_val;
                atomicAdd(&visits[(uint32_t)(x >> (2 * (J - 1 - t))) & kmask], 1u);
                L.step(sv, i, ec, cand);
              }
            }
            x = B.next_key(x, J, xmask);
          }
        }
      }
#pragma unroll
      for (int d = 0; d < D; ++d)
#pragma unroll
        for (int q = 0; q < W; ++q) cur[d][q] = nxt[d][q];
    }
  } else {
    walk(__ballot(n == CH) == ~0ull);
  }
  L.finish_exact(c, g, o, cr, xh, err);
}
#undef KS_INLINE_LAMBDA

// KS_TEST_KEPT_CODES (tests): the kept codes of a call that reads them, spoilt
// before its pass 1.  what 0 (sample): the first code of chunk 0, which the
// tripwire compares; 1 (all): every code; 2 (one): the code of index 1 of the
// first chunk that no tripwire samples, that has a successor in its run (so
// its exit is verified) and whose carried head the previous call -- its Carry
// fields are still in the workspace -- found never to clamp; none: nothing is
// spoilt and error bit 256 fails the call, so a test cannot pass on another
// code than the one it asked for.  A spoilt code is 0, or 1 where it was 0:
// another LUT entry, so another value.  One block.
__global__ void __launch_bounds__(256) k_test_codes(uint32_t *__restrict__ kc, Chunks g, Carry cr, int64_t nch,
                                                    int J, int what, unsigned int *__restrict__ err) {
  auto spoil = [&](int64_t c, int i) {
    uint32_t *p = kc + kc_slot(c, i / J, J) + (size_t)((i % J) >> 1);
    const int sh = 16 * ((i % J) & 1);
    const uint32_t code = (*p >> sh) & 0xffffu;
    *p = (*p & ~(0xffffu << sh)) | ((code ? 0u : 1u) << sh);
  };
  if (what == 1) {
    for (int64_t c = threadIdx.x; c < nch; c += blockDim.x)
      for (int i = 0; i < CH; ++i) spoil(c, i);
  } else if (what == 0) {
    if (threadIdx.x == 0) spoil(0, 0);
  } else {
    __shared__ unsigned long long s_first;
    if (threadIdx.x == 0) s_first = ~0ull;
    __syncthreads();
    for (int64_t c = threadIdx.x; c < nch; c += blockDim.x)
      if ((c & 63) != 0 && g.n[c] > 1 && c + 1 < nch && g.run[c + 1] == g.run[c] && cr.mode[c] != kModeClean &&
          cr.hq[c] < 0)
        atomicMin(&s_first, (unsigned long long)c);
    __syncthreads();
    if (threadIdx.x == 0) {
      if (s_first == ~0ull) atomicOr(err, 256u);
      else spoil((int64_t)s_first, 1);
    }
  }
}

// Pass 1 over weighted-rank code lines (ks_table::d_rlines, line kind 4):
// one 128-B line per 15-mer x holding the 32-bit rank codes of its OWN
// k-mers and of every one- and two-base continuation (L1: 4, L2: 16), so a
// line read serves J = OWN + 2 consecutive indices (5 at k = 13, against 4
// for the FP64 64-B lines of k_pass1l).  The 8 lanes that share a line fetch
// the 5 dwords a step needs with LDS-DMA (k_pass1w's ring and counted waits).
// A code is piece << kRankOffBits | offset, and the k-mer's weighted rank --
// R_j of the sorted position j, the closed-form prefix of rank_kmers_w
// (kmer_spans.c:196-200; RankPiece) -- is bits(R) = base + offset * inc of its
// piece; s = R - thr in FP64, as the FP64 table holds it (k_sub_thr).  The
// kRankPieceLds hottest pieces (weight order) are staged in LDS, the rest
// read from the L2-resident piece table.  Same outputs as k_pass1l<OWN, true>.
constexpr int kRankBlock = 768;

template <int OWN>
__global__ void __launch_bounds__(kRankBlock) k_pass1r(Chunks g, int64_t total, int k, TableView tv, EmitCfg ec,
                                                       uint32_t *__restrict__ visits, P1 o, Cand cand) {
  constexpr int BS = kRankBlock;
  constexpr int J = OWN + 2;
  constexpr int NS = (CH + J - 1) / J;
  static_assert(OWN + 2 <= 8, "own, L1, L2 dwords in 8 lanes");
  __shared__ __attribute__((aligned(16))) uint8_t s_ring[(BS / 64) * 2 * 2048];
  __shared__ unsigned long long s_pc[2 * kRankPieceLds];
  const int nl = min(tv.nrpc, kRankPieceLds);
  for (int i = threadIdx.x; i < 2 * nl; i += BS) s_pc[i] = tv.rpc[i];
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t c = g.c0 + (int64_t)blockIdx.x * BS + threadIdx.x;
  if (c - lane >= g.nch) return;
  const bool live = c < g.nch;
  const int64_t start = live ? g.start[c] : (int64_t)k;
  const int n = live ? g.n[c] : 0;
  const bool first = live && (c == 0 || g.run[c - 1] != g.run[c]);
  const uint32_t kmask = (1u << (2 * k)) - 1u;
  P1Lane<false, false> L;  // (FP64 tables take no chunk summaries)
  L.init(start, n, first, live, 0.0);
  LaneBases B;
  B.load(g.packed, total, start - k);
  const int kx = k + J - 1;  // key length: the 15-mer of the line and the two continuation bases
  const uint64_t xmask = (1ull << (2 * kx)) - 1ull;
  uint64_t x = B.first_key(kx);
  uint8_t *const ring = s_ring + wv * 4096;
  const uint32_t ring_lds = __builtin_amdgcn_readfirstlane(lds_addr(ring));
  const uint8_t *__restrict__ lines = tv.rline;
  const unsigned long long *__restrict__ gpc = tv.rpc;
  const double thr = tv.rthr;
  // the dwords a step reads (key xk): own 0 .. OWN - 1, L1 OWN + c1, L2 OWN + 4 + 4 c1 + c2
  auto issue = [&](uint64_t xk, int slot) {
    const uint32_t idx = (uint32_t)(xk >> 4);
    const uint32_t c1 = (uint32_t)(xk >> 2) & 3u, c2 = (uint32_t)xk & 3u;
    const uint32_t dd = (OWN + c1) | ((OWN + 4 + 4 * c1 + c2) << 8);
    const int j = lane & 7;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int ow = 8 * q + (lane >> 3);
      const uint32_t li = (uint32_t)__shfl((int)idx, ow);
      const uint32_t od = (uint32_t)__shfl((int)dd, ow);
      const uint32_t dw = j < OWN ? (uint32_t)j : (j == OWN ? (od & 0xffu) : (j == OWN + 1 ? (od >> 8) : 0u));
      glds4(lines + (size_t)li * 128 + dw * 4, ring_lds + (uint32_t)(slot * 2048 + q * 256));
    }
  };
  auto decode = [&](uint32_t code) -> double {
    const uint32_t p = code >> kRankOffBits;
    const unsigned long long off = code & ((1u << kRankOffBits) - 1u);
    unsigned long long base, inc;
    if ((int)p < nl) {
      base = s_pc[2 * p];
      inc = s_pc[2 * p + 1];
    } else {  // a cold piece: the L2-resident table
      base = gpc[2 * p];
      inc = gpc[2 * p + 1];
    }
    return __longlong_as_double((long long)(base + off * inc)) - thr;
  };
  double vp[J];
  uint64_t xp = 0;
  auto process = [&](int sp_, const double *vv, uint64_t xk) {
#pragma unroll
    for (int t = 0; t < J; ++t) {
      const int i = sp_ * J + t;
      if (i < n) {
        if (visits) atomicAdd(&visits[(uint32_t)(xk >> (2 * (J - 1 - t))) & kmask], 1u);
        L.step(vv[t], i, ec, cand);
      }
    }
  };
  uint64_t x1 = 0, x2 = 0;
  issue(x, 0);
  x1 = B.next_key(x, J, xmask);
  issue(x1, 1);
  for (int st = 0; st < NS; ++st) {
    const uint64_t xs = x;
    // this step's lines complete (the next step's eight loads may stay in flight)
    if (st + 1 < NS) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const uint8_t *ln = ring + (st & 1) * 2048 + lane * 32;
    uint32_t cs[J];
    {
      const uint4 q0 = *reinterpret_cast<const uint4 *>(ln);
      const uint4 q1 = *reinterpret_cast<const uint4 *>(ln + 16);
      const uint32_t D[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
#pragma unroll
      for (int t = 0; t < J; ++t) cs[t] = D[t];
    }
    x = x1;
    if (st + 2 < NS) {
      x2 = B.next_key(x1, J, xmask);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the slot's reads are done before it is refilled
      issue(x2, st & 1);
      x1 = x2;
    }
    if (st > 0) process(st - 1, vp, xp);
#pragma unroll
    for (int t = 0; t < J; ++t) vp[t] = decode(cs[t]);
    xp = xs;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  process(NS - 1, vp, xp);
  if (live) L.finish(c, o, SummP1{});
}

// Pass 1 for small k (north_star: "the frequency table LDS-staged for small
// k"): the 4^k FP64 values s[code] (k <= 7: <= 128 KiB) are staged in LDS
// once per persistent block, so every scanned index costs one LDS read and no
// random HBM request; bases are rolled from the packed 2-bit codes (one
// 4-B word per 16 bases).  No code store: later passes re-derive values from
// the packed bases and the base table (values16_nostore / values4).  Same
// outputs as k_pass1.
constexpr int kLdsTableK = 7;
// Pass 1 of small-k integer tables (k <= 7, ks_table::int_exact): the
// clean trajectory of a chunk starts at 0 and moves by at most 2^20 per
// index, so it and the chunk aggregates fit int32 (|S| <= 2^28) and equal the
// FP64 chain exactly; 32-bit integer compares and selects instead of FP64
// ones (half the VALU work of this ALU-bound pass), the table as int32 in
// LDS (64 KiB at k = 7: two blocks per CU).  Outputs as k_pass1_lds<false>
// without the |s| sum and the non-finite flag (FP64 aggregates).
__global__ void __launch_bounds__(1024) k_pass1_lds_int(Chunks g, int64_t total, int k, TableView tv, EmitCfg ec,
                                                        uint32_t *__restrict__ visits, P1 o, Cand cand) {
  __shared__ int32_t s_val[1 << (2 * kLdsTableK)];
  const int nk = 1 << (2 * k);
  for (int i = threadIdx.x; i < nk; i += blockDim.x) s_val[i] = (int32_t)tv_get(tv, (uint32_t)i);
  __syncthreads();
  const uint32_t kmask = (uint32_t)nk - 1u;
  for (int64_t c = g.c0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < g.nch;
       c += (int64_t)gridDim.x * blockDim.x) {
    const int64_t start = g.start[c];
    const int n = g.n[c];
    const int64_t q0 = start - k;
    Window16 win(g.packed, total, q0);
    // P1Lane::step on int32 (kmer_regions only, no |s| sum, no summaries)
    int32_t prev = 0, best = 0, asum = 0, pmin = INT32_MAX, pmax = INT32_MIN;
    int beg = -1, arg = 0, parg = 0;
    for (int b0 = 0; b0 < n; b0 += 16) {
      const uint64_t x = win.take(q0 + b0);
      for (int j = 0; j < 16; ++j) {
        const int i = b0 + j;
        if (i >= n) break;
        const uint32_t code = (uint32_t)(x >> (64 - 2 * (j + k))) & kmask;  // k-mer ending at start + i - 1
        const int32_t sv = s_val[code];
        if (visits) atomicAdd(&visits[code], 1u);
        asum += sv;
        pmin = asum < pmin ? asum : pmin;
        parg = asum > pmax ? i : parg;
        pmax = asum > pmax ? asum : pmax;
        const int32_t tt = prev + sv;
        const int32_t S = tt > 0 ? tt : 0;
        const bool open = (prev == 0) & (S > 0);
        const bool close = (prev > 0) & (S == 0);
        const bool want = close & ((uint64_t)(int64_t)(arg - beg) >= ec.mw) & ((double)best >= ec.min_score);
        if (want) cand_put(cand, start, beg, arg, i, (double)best);
        const bool up = open | (S > best);
        best = up ? S : best;
        arg = up ? i : arg;
        beg = open ? i : (close ? -1 : beg);
        prev = S;
      }
    }
    p1_put(o, c, (double)prev, (double)asum, n > 0 ? (double)pmin : INFINITY, n > 0 ? (double)pmax : -INFINITY, parg,
           0.0, false, beg, (double)best, arg);
  }
}

// Chunk c of the FP64 small-k pass from the LDS-staged table s_val; kSumm:
// with the summaries in the binades of the predicted entry xp.
template <bool kSumm, bool kTrlr>
__device__ __forceinline__ void lds_chunk(const Chunks &g, int64_t total, int k, const double *s_val,
                                          const EmitCfg &ec, uint32_t *__restrict__ visits, const P1 &o,
                                          const Cand &cand, const SummP1 &sp, int64_t c, double xp) {
  const uint32_t kmask = (1u << (2 * k)) - 1u;
  const int64_t start = g.start[c];
  const int n = g.n[c];
  const bool first = c == 0 || g.run[c - 1] != g.run[c];
  P1Lane<kSumm, kTrlr> L;
  L.init(start, n, first, true, xp);
  const int64_t q0 = start - k;
  Window16 win(g.packed, total, q0);
  for (int b0 = 0; b0 < n; b0 += 16) {
    const uint64_t x = win.take(q0 + b0);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int i = b0 + j;
      if (i < n) {
        const uint32_t code = (uint32_t)(x >> (64 - 2 * (j + k))) & kmask;  // k-mer ending at start + i - 1
        double s = s_val[code];
        if (kTrlr && first && i == 0) s = ec.ks[code];  // tr_lr: the run's first k-mer's own score
        if (visits) atomicAdd(&visits[code], 1u);
        L.step(s, i, ec, cand);
      }
    }
  }
  L.finish(c, o, sp);
}

// (integer tables on the exact carry take k_pass1_lds_int instead: neither the
// |s| sum nor the non-finite flag is read on that path)
template <bool kTrlr>
__global__ void __launch_bounds__(1024) k_pass1_lds(Chunks g, int64_t total, int k, TableView tv, EmitCfg ec,
                                                    uint32_t *__restrict__ visits, P1 o, Cand cand,
                                                    const double *__restrict__ xh, SummP1 sp) {
  __shared__ double s_val[1 << (2 * kLdsTableK)];
  const int nk = 1 << (2 * k);
  for (int i = threadIdx.x; i < nk; i += blockDim.x) s_val[i] = tv_get(tv, (uint32_t)i);
  __syncthreads();
  for (int64_t c = g.c0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < g.nch;
       c += (int64_t)gridDim.x * blockDim.x) {
    // xh: pass-1 summaries in the predicted binades (as k_pass1l)
    if (xh) lds_chunk<true, kTrlr>(g, total, k, s_val, ec, visits, o, cand, sp, c, xh[c]);
    else lds_chunk<false, kTrlr>(g, total, k, s_val, ec, visits, o, cand, sp, c, 0.0);
  }
}

// Software-pipelined gather pass for uncompressed FP64 expanded tables
// (weighted-rank tables: every k-mer has its own value, so no codes): one
// 16-B (J = 2) or 32-B (J = 3, 4) entry per J scan indices, the next batch's
// entries in flight while the current batch runs the clean trajectory, bases
// rolled from the packed codes.  Same outputs as k_pass1<J, false, false>
// (no code store: later passes re-read the table), plus (xh != nullptr) the
// binade-integer summaries in the predicted binades (P1Lane, as k_pass1l):
// at k = 15 a separate k_summaries pass re-read the 64 GiB table.
template <int J, bool kTrlr, int kBlock = 512>
__global__ void __launch_bounds__(kBlock) k_pass1pf(Chunks g, const uint8_t *__restrict__ seq, int64_t total, int k,
                                                  TableView tv, EmitCfg ec, uint32_t *__restrict__ visits, P1 o,
                                                  Cand cand, const uint32_t *__restrict__ packed,
                                                  const double *__restrict__ xh, SummP1 sp) {
  constexpr int G = (J == 2) ? 8 : 4;  // table reads per batch
  constexpr int PB = G * J;            // scan indices per batch (16, 12, 16)
  using GC = typename std::conditional<(J >= 3), uint64_t, uint32_t>::type;
  const int64_t c = g.c0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= g.nch) return;
  const double2 *__restrict__ E = reinterpret_cast<const double2 *>(tv.ext);
  const int kx = k + J - 1;
  const GC xmask = (2 * kx >= 8 * (int)sizeof(GC)) ? ~(GC)0 : (((GC)1 << (2 * kx)) - 1);
  const uint32_t kmask = (1u << (2 * k)) - 1u;
  const int64_t start = g.start[c];
  const int n = g.n[c];
  const bool first = c == 0 || g.run[c - 1] != g.run[c];
  // tail lanes (reads could pass the end of the buffer) are left to k_pass1
  if (start + n + kP1TailMargin > total) {
    sp.e[2 * c] = sp.e[2 * c + 1] = INT32_MIN;  // no pass-1 summary (the workspace is reused)
    return;
  }
  P1Lane<true, kTrlr> L;
  L.init(start, n, first, true, xh ? xh[c] : 0.0);
  GC gcode = (GC)prime_code_guarded64(seq, start - k, kx, total);
  const double first_val = (kTrlr && first) ? ec.ks[(uint32_t)(gcode >> (2 * (J - 1))) & kmask] : 0.0;
  const int64_t q0 = start + J - 1;
  constexpr uint64_t fmask = (1ull << (2 * J)) - 1ull;
  auto roll = [&](u32x3a4 w, int64_t qb, GC gout[G]) {
    const uint32_t bp = 2u * (uint32_t)(qb & 15);
    const uint64_t x = ((((uint64_t)w.x << 32) | w.y) << bp) | (((uint64_t)w.z << bp) >> 32);
#pragma unroll
    for (int gi = 0; gi < G; ++gi) {
      gout[gi] = gcode;
      gcode = ((gcode << (2 * J)) | (GC)((x >> (64 - 2 * J * (gi + 1))) & fmask)) & xmask;
    }
  };
  auto fetch = [&](const GC gg[G], int b0, double2 e0[G], double2 e1[G]) {
#pragma unroll
    for (int gi = 0; gi < G; ++gi) {
      const size_t ix = (b0 + gi * J < n) ? (size_t)gg[gi] : 0;
      if (J <= 2) {
        e0[gi] = E[ix];
      } else {
        e0[gi] = E[2 * ix];
        e1[gi] = E[2 * ix + 1];
      }
    }
  };
  GC gc[G];
  double2 e0[G], e1[G];
  u32x3a4 win = *reinterpret_cast<const u32x3a4 *>(packed + (q0 >> 4));
  roll(win, q0, gc);
  fetch(gc, 0, e0, e1);
  win = *reinterpret_cast<const u32x3a4 *>(packed + ((q0 + PB) >> 4));
  for (int b0 = 0; b0 < n; b0 += PB) {
    GC gn[G];
    double2 n0[G], n1[G];
    roll(win, q0 + b0 + PB, gn);
    fetch(gn, b0 + PB, n0, n1);
    win = *reinterpret_cast<const u32x3a4 *>(packed + ((q0 + b0 + 2 * PB) >> 4));
#pragma unroll
    for (int gi = 0; gi < G; ++gi) {
      const double ev[4] = {e0[gi].x, e0[gi].y, J > 2 ? e1[gi].x : 0.0, J > 3 ? e1[gi].y : 0.0};
#pragma unroll
      for (int t = 0; t < J; ++t) {
        const int j = gi * J + t;
        double s = ev[t];
        if (kTrlr && first && b0 == 0 && j == 0) s = first_val;
        const int i = b0 + j;
        if (i < n) {
          if (visits) atomicAdd(&visits[(uint32_t)(gc[gi] >> (2 * (J - 1 - t))) & kmask], 1u);
          L.step(s, i, ec, cand);
        }
      }
    }
#pragma unroll
    for (int gi = 0; gi < G; ++gi) {
      gc[gi] = gn[gi];
      e0[gi] = n0[gi];
      e1[gi] = n1[gi];
    }
  }
  L.finish(c, o, sp);
}

// ------------------------------------------------------------------- P3

// Binade-integer summary of chunk c for binade e: with S = m * 2^(e-52) and
// the whole trajectory inside [2^e, 2^(e+1)), fl(S + s) = S + RN(s * 2^(52-e))
// with ties to even decided by the parity of m.  For both entry parities t:
// total D, max M (first argmax A) and min N of the integer trajectory.
// Returns false if a value is not representable (overflow, NaN, Inf).
template <bool kCompressed, bool kDual>
__device__ int chunk_summary_impl(const Chunks &g, const uint8_t *__restrict__ seq, int64_t total, int k,
                                  const TableView &tv, const uint16_t *__restrict__ codes, int64_t c, int e,
                                  long long D[2], long long M[2], int A[2], long long N[2]) {
  // returns 1 ok, 0 not representable, -1 (single-trajectory mode only) a tie occurred
  const int n = g.n[c];
  const int64_t start = g.start[c];
  const uint32_t mask = (1u << (2 * k)) - 1u;
  const double scale = ldexp(1.0, 52 - e);
  uint32_t code = kCompressed ? 0u : prime_code(seq, start - k, k);
  long long cur[2] = {0, 0};
  M[0] = M[1] = LLONG_MIN;
  N[0] = N[1] = LLONG_MAX;
  A[0] = A[1] = 0;
  bool ok = true, tie_seen = false;
  for (int b0 = 0; b0 < n; b0 += NB) {
    double v[NB];
    if (kCompressed && !codes) {
      values16_nostore(g, seq, total, k, tv, c, b0, n, v, nullptr);
    } else if (kCompressed) {
      uint32_t w[8];
      load_codes16(codes, c, b0, w);
#pragma unroll
      for (int j = 0; j < NB; ++j) v[j] = tv.lut[(w[j >> 1] >> (16 * (j & 1))) & 0xffffu];
    } else {
      values16_f64(g, seq, total, k, tv, start, b0, n, code, mask, v);
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int i = b0 + j;
      if (i < n) {
        const double y = v[j] * scale;  // exact: power-of-two scaling
        ok &= fabs(y) < 4.0e18;         // also false for NaN / Inf
        const double fq = floor(y);
        const double f = y - fq;        // exact fractional part
        const bool up = f > 0.5, tie = f == 0.5;
        if (kDual) {
          const long long q = ok ? (long long)fq : 0;
#pragma unroll
          for (int t = 0; t < 2; ++t) {
            const long long par = (t + cur[t]) & 1;
            cur[t] += q + ((up || (tie && ((par + q) & 1))) ? 1 : 0);
            if (cur[t] > M[t]) { M[t] = cur[t]; A[t] = i; }
            N[t] = min(N[t], cur[t]);
          }
        } else {  // no tie: the increment does not depend on the parity
          tie_seen |= tie;
          const long long q = ok ? (long long)(up ? fq + 1.0 : fq) : 0;
          cur[0] += q;
          if (cur[0] > M[0]) { M[0] = cur[0]; A[0] = i; }
          N[0] = min(N[0], cur[0]);
        }
      }
    }
  }
  if (!ok) return 0;
  if (!kDual) {
    if (tie_seen) return -1;
    cur[1] = cur[0]; M[1] = M[0]; N[1] = N[0]; A[1] = A[0];
  }
  D[0] = cur[0];
  D[1] = cur[1];
  return 1;
}

// Binade-integer summary of chunk c for binade e: with S = m * 2^(e-52) and
// the whole trajectory inside [2^e, 2^(e+1)), fl(S + s) = S + RN(s * 2^(52-e))
// with ties to even decided by the parity of m.  For both entry parities t:
// total D, max M (first argmax A) and min N of the integer trajectory.  One
// trajectory is tracked unless an exact tie occurs (then both parities).
// Single-trajectory binade summary in FP64 integer arithmetic: with
// |y| < 2^51, (y + 1.5*2^52) - 1.5*2^52 is y rounded half-to-even, an exact
// integer; partial sums stay exact while |sum| < 2^53 (checked through the
// extremes).  Returns 1 ok, 0 not representable, -1 a tie occurred (the
// increment then depends on the parity: the dual-parity path is used).
template <bool kCompressed, bool kLds>
__device__ int chunk_summary_fast(const Chunks &g, const uint8_t *__restrict__ seq, int64_t total, int k,
                                  const TableView &tv, const uint16_t *__restrict__ codes, int64_t c, int e,
                                  long long D[2], long long M[2], int A[2], long long N[2],
                                  const double *s_lut) {
  const int n = g.n[c];
  const int64_t start = g.start[c];
  const uint32_t mask = (1u << (2 * k)) - 1u;
  const double scale = ldexp(1.0, 52 - e);
  constexpr double kMagic = 6755399441055744.0;  // 1.5 * 2^52
  uint64_t xp = 0;
  uint32_t code = kCompressed ? 0u
                  : packed_bits(g.packed, total, start - k, xp) ? (uint32_t)(xp >> (64 - 2 * k))
                                                                : prime_code(seq, start - k, k);
  double cur = 0.0, mx = -INFINITY, mn = INFINITY;
  int arg = 0;
  bool ok = true, tie_seen = false;
  for (int b0 = 0; b0 < n; b0 += NB) {
    double v[NB];
    if (kCompressed && !codes) {
      values16_nostore(g, seq, total, k, tv, c, b0, n, v, kLds ? s_lut : nullptr);
    } else if (kCompressed) {
      uint32_t w[8];
      load_codes16(codes, c, b0, w);
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        const uint32_t q = (w[j >> 1] >> (16 * (j & 1))) & 0xffffu;
        v[j] = kLds ? s_lut[q] : tv.lut[q];
      }
    } else if (tv.ext && tv.ext_J == 4) {  // FP64 expanded table: 4 values per 32-B read
      uint8_t by[16];
      uint64_t xb = 0;
      if (packed_bits(g.packed, total, start + b0, xb)) {  // bytes with the same enc() as the packed codes
#pragma unroll
        for (int j = 0; j < 16; ++j) by[j] = (uint8_t)(((xb >> (62 - 2 * j)) & 3u) << 1);
      } else {
        load16(seq, start + b0, total, by);
      }
      const double2 *E = reinterpret_cast<const double2 *>(tv.ext);
#pragma unroll
      for (int gq = 0; gq < NB / 4; ++gq) {
        // (k+3)-mer of indices b0+4gq .. +3: the k-mer of the first, then 3 bytes
        const uint64_t gx = ((uint64_t)code << 6) | ((uint64_t)enc(by[4 * gq]) << 4) |
                            ((uint64_t)enc(by[4 * gq + 1]) << 2) | (uint64_t)enc(by[4 * gq + 2]);
        double2 e0 = make_double2(0.0, 0.0), e1 = e0;
        if (b0 + 4 * gq < n) {
          e0 = E[2 * gx];
          e1 = E[2 * gx + 1];
        }
        v[4 * gq] = e0.x;
        v[4 * gq + 1] = e0.y;
        v[4 * gq + 2] = e1.x;
        v[4 * gq + 3] = e1.y;
#pragma unroll
        for (int t = 0; t < 4; ++t) code = roll(code, by[4 * gq + t], mask);
      }
    } else {
      values16_f64(g, seq, total, k, tv, start, b0, n, code, mask, v);
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      if (b0 + j < n) {
        const double y = v[j] * scale;  // exact: power-of-two scaling
        ok &= fabs(y) < 2251799813685248.0;  // 2^51; false for NaN / Inf
        const double r = (y + kMagic) - kMagic;
        tie_seen |= fabs(r - y) == 0.5;
        cur += r;
        if (cur > mx) { mx = cur; arg = b0 + j; }
        mn = fmin(mn, cur);
      }
    }
  }
  ok &= mx < 4503599627370496.0 && mn > -4503599627370496.0;  // |partial sums| < 2^52: all exact
  if (!ok) return 0;
  if (tie_seen) return -1;
  D[0] = D[1] = (long long)cur;
  M[0] = M[1] = (long long)mx;
  N[0] = N[1] = (long long)mn;
  A[0] = A[1] = arg;
  return 1;
}

template <bool kCompressed, bool kLds>
__device__ bool chunk_summary(const Chunks &g, const uint8_t *__restrict__ seq, int64_t total, int k,
                              const TableView &tv, const uint16_t *__restrict__ codes, int64_t c, int e,
                              long long D[2], long long M[2], int A[2], long long N[2], const double *s_lut) {
  const int rc = chunk_summary_fast<kCompressed, kLds>(g, seq, total, k, tv, codes, c, e, D, M, A, N, s_lut);
  if (rc >= 0) return rc == 1;
  return chunk_summary_impl<kCompressed, true>(g, seq, total, k, tv, codes, c, e, D, M, A, N) == 1;
}

// ------------------------------------------------------------------- P2

// Approximate max-plus scan, one wave per run: chunk j maps x -> max(x + a, b)
// (a = sum, b = clean exit); x~_j = composite of chunks < j applied to 0.  Only
// a prediction (which binade the exact carry will be in); never trusted.
__global__ void __launch_bounds__(64) k_approx_scan(const int64_t *__restrict__ cbase, int64_t nruns, P1 o,
                                                    double *__restrict__ xt, int64_t r_lo) {
  const int64_t r = r_lo + blockIdx.x;
  if (r >= nruns) return;
  const int lane = threadIdx.x;
  const int64_t c0 = cbase[r], c1 = cbase[r + 1];
  double carry = 0.0;
  for (int64_t cb = c0; cb < c1; cb += 64) {
    const int64_t c = cb + lane;
    APair p{0.0, -INFINITY};  // identity
    if (c < c1) {
      p.a = o.special[c] ? -INFINITY : o.asum[c];
      p.b = o.cexit[c];
    }
    KS_DPP_SCAN(APair, p, dpp_ap, ap_op);
    const APair ex = ap_prev(p);
    const double ea = ex.a, eb = ex.b;
    if (c < c1) xt[c] = fmax(carry + ea, eb);
    const double la = rld(p.a, 63), lb = rld(p.b, 63);
    carry = fmax(carry + la, lb);
    if (!(carry == carry)) carry = 0.0;
  }
}

// Per-tile run map: block r writes r for the stitch tiles of run r.
__global__ void k_tile_runs(const int64_t *__restrict__ tbase, int64_t nruns, int32_t *__restrict__ trun) {
  const int64_t r = blockIdx.x;
  if (r >= nruns) return;
  for (int64_t t = tbase[r] + threadIdx.x; t < tbase[r + 1]; t += blockDim.x) trun[t] = (int32_t)r;
}

// Run of stitch tile t from the per-tile run map (k_tile_runs): one load
// instead of a dependent binary search over the runs, which bounded the
// wave-per-tile kernels by its latency (12 loads at 2,790 runs).
__device__ __forceinline__ void tile_of(const int64_t *__restrict__ tbase, const int64_t *__restrict__ cbase,
                                        const int32_t *__restrict__ trun, int64_t t, int64_t &r, int64_t &c0,
                                        int64_t &c1, int64_t nruns) {
  int64_t lo;
  if (trun) {
    lo = trun[t];
  } else {  // (KS_TILE_SEARCH: the binary search, A/B)
    lo = 0;
    int64_t hi = nruns - 1;  // last run with tbase[r] <= t
    while (lo < hi) {
      const int64_t mid = (lo + hi + 1) >> 1;
      if (tbase[mid] <= t) lo = mid; else hi = mid - 1;
    }
  }
  r = lo;
  c0 = cbase[lo] + (t - tbase[lo]) * 64;
  c1 = min(c0 + 64, cbase[lo + 1]);
}

// The same prediction as k_approx_scan in three parallel steps over the
// 64-chunk tiles of the runs (the stitch tiles): (A) every tile's composite
// map, (B) per run a wave scan of its tiles' maps (64 tiles per step instead
// of 64 chunks), (C) every tile applies its entry to its chunks.  The
// composition order differs from k_approx_scan, so the FP64 results may
// differ in the last bits: only a prediction, never a result.
__device__ __forceinline__ void ascan_pair(double &a, double &b, int lane) {
  APair p{a, b};  // (a1,b1) then (a2,b2) = (a1+a2, max(b1+a2, b2))
  KS_DPP_SCAN(APair, p, dpp_ap, ap_op);
  a = p.a;
  b = p.b;
  (void)lane;
}
// the exclusive pair (the previous lane's inclusive one; identity in lane 0)
__device__ __forceinline__ void ascan_prev(double a, double b, double &ea, double &eb) {
  const APair ex = ap_prev(APair{a, b});
  ea = ex.a;
  eb = ex.b;
}
__global__ void __launch_bounds__(256) k_ascan_tiles(const int64_t *__restrict__ tbase, const int64_t *__restrict__ cbase,
                                                    int64_t nruns, const int32_t *__restrict__ trun, P1 o, double2 *__restrict__ tagg, int64_t t_lo,
                                                    int64_t t_hi) {
  const int64_t t = t_lo + (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);  // wave per tile
  if (t >= t_hi) return;
  const int lane = threadIdx.x & 63;
  int64_t r, c0, c1;
  tile_of(tbase, cbase, trun, t, r, c0, c1, nruns);
  const int64_t c = c0 + lane;
  double a = 0.0, b = -INFINITY;
  if (c < c1) {
    a = o.special[c] ? -INFINITY : o.asum[c];
    b = o.cexit[c];
  }
  ascan_pair(a, b, lane);
  if (lane == 63) tagg[t] = make_double2(a, b);
}
__global__ void __launch_bounds__(64) k_ascan_runs(const int64_t *__restrict__ tbase, int64_t nruns,
                                                   const double2 *__restrict__ tagg, double *__restrict__ tin,
                                                   int64_t r_lo) {
  const int64_t r = r_lo + blockIdx.x;
  if (r >= nruns) return;
  const int lane = threadIdx.x;
  const int64_t t0 = tbase[r], t1 = tbase[r + 1];
  double carry = 0.0;
  for (int64_t tb = t0; tb < t1; tb += 64) {
    const int64_t t = tb + lane;
    double a = 0.0, b = -INFINITY;
    if (t < t1) {
      const double2 v = tagg[t];
      a = v.x;
      b = v.y;
    }
    ascan_pair(a, b, lane);
    double ea, eb;
    ascan_prev(a, b, ea, eb);
    double xin = fmax(carry + ea, eb);
    if (!(xin == xin)) xin = 0.0;
    if (t < t1) tin[t] = xin;
    const double la = rld(a, 63), lb = rld(b, 63);
    carry = fmax(carry + la, lb);
    if (!(carry == carry)) carry = 0.0;
  }
}
__global__ void __launch_bounds__(256) k_ascan_apply(const int64_t *__restrict__ tbase, const int64_t *__restrict__ cbase,
                                                    int64_t nruns, const int32_t *__restrict__ trun, P1 o, const double *__restrict__ tin,
                                                    double *__restrict__ xt, int64_t t_lo, int64_t t_hi) {
  const int64_t t = t_lo + (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);  // wave per tile
  if (t >= t_hi) return;
  const int lane = threadIdx.x & 63;
  int64_t r, c0, c1;
  tile_of(tbase, cbase, trun, t, r, c0, c1, nruns);
  const int64_t c = c0 + lane;
  double a = 0.0, b = -INFINITY;
  if (c < c1) {
    a = o.special[c] ? -INFINITY : o.asum[c];
    b = o.cexit[c];
  }
  ascan_pair(a, b, lane);
  double ea, eb;
  ascan_prev(a, b, ea, eb);
  if (c < c1) xt[c] = fmax(tin[t] + ea, eb);
}

// Largest value of the predicted trajectory that keeps a binade summary
// meaningful; below kLMin the trajectory crosses binades every few steps.
constexpr double kLMin = 64.0;

// Summary of each chunk for the binade of its predicted trajectory (lane per
// chunk, full occupancy); chunks predicted to leave the binade or to approach
// 0 get none.
// kTab (small k, k_pass1_lds): the table staged in LDS too (dynamic, <= 128
// KiB): with a compressed table whose LUT is in LDS (kLds) its uint16 codes,
// else its 4^k FP64 values (lut[codes[i]] for a compressed one) read as an
// uncompressed base table (instantiated with kCompressed = false).  At k = 7
// (`profiles/r3/smallk/`): +-1 (2 values) codes 3.75 ms vs values 4.18;
// log2 (16 K values, LUT beyond LDS) values 6.4 ms vs codes 9.1.
// (KS_NO_SUMMARIES A/B: no chunk gets a summary; every carried chunk replays)
__global__ void __launch_bounds__(1024) k_summ_none(Chunks g, Summ sm) {
  const int64_t c = g.c0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c < g.nch) sm.e[c] = INT32_MIN;
}

template <bool kCompressed, bool kLds, bool kTab = false>
__global__ void __launch_bounds__(1024) k_summaries(Chunks g, const uint8_t *__restrict__ seq, int64_t total,
                                                    int k, TableView tv, const uint16_t *__restrict__ codes, P1 o,
                                                    const double *__restrict__ xt, Summ sm) {
  __shared__ double s_lut[kLds ? kLdsLutMax : 1];
  extern __shared__ __attribute__((aligned(16))) uint8_t s_tab[];
  if (kLds)
    for (int i = threadIdx.x; i < tv.nlut; i += blockDim.x) s_lut[i] = tv.lut[i];
  if (kTab) {
    const int nk = 1 << (2 * k);
    if (kCompressed) {
      uint16_t *sc = reinterpret_cast<uint16_t *>(s_tab);
      for (int i = threadIdx.x; i < nk; i += blockDim.x) sc[i] = tv.codes[i];
      tv.codes = sc;
    } else {
      double *sv = reinterpret_cast<double *>(s_tab);
      for (int i = threadIdx.x; i < nk; i += blockDim.x) sv[i] = tv.compressed ? tv.lut[tv.codes[i]] : tv.vals[i];
      tv.vals = sv;
      tv.compressed = 0;
      tv.codes = nullptr;
    }
    tv.ext = nullptr;  // (values from the staged base table)
    tv.line = nullptr;
  }
  if (kLds || kTab) __syncthreads();
  const int64_t c = g.c0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // (the part's chunks)
  if (c >= g.nch) return;
  sm.e[c] = INT32_MIN;
  if (o.special[c]) return;
  const double x = xt[c];
  if (!(x >= kLMin) || !(x < 1.0e18)) return;
  const int e = (int)((__double_as_longlong(x) >> 52) & 0x7ff) - 1023;
  const double lo = fmin(x, x + o.pmin[c]), hi = fmax(x, x + o.pmax[c]);
  const double slack = ldexp(1.0, e - 24) + o.sabs[c] * 1e-9;
  if (!(lo - slack >= ldexp(1.0, e)) || !(hi + slack < ldexp(1.0, e + 1))) return;
  long long D[2], M[2], N[2];
  int A[2];
  if (!chunk_summary<kCompressed, kLds>(g, seq, total, k, tv, codes, c, e, D, M, A, N, s_lut)) return;
  sm.e[c] = e;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    sm.D[2 * c + t] = D[t];
    sm.M[2 * c + t] = M[t];
    sm.N[2 * c + t] = N[t];
    sm.A[2 * c + t] = A[t];
  }
}

// Pass-1 summaries (kSumm): the summary of every chunk whose exact carry will
// want one (same test as k_summaries) is the pass-1 one when pass 1 predicted
// this binade; the others (no or another prediction, a tie, the tail chunks)
// are listed for k_summ_fixw.
// The per-chunk part of the selection: the selected summary (or none) of
// chunk c; want: list it for k_summ_fixw; rwant: list it for the replay
// prefetch.
__device__ __forceinline__ void select_one(const Chunks &g, const P1 &o, const double *__restrict__ xt,
                                           const SummP1 &sp, const Summ &sm, const double *__restrict__ xh,
                                           unsigned long long *__restrict__ why, const ReplayBuf &rp, int64_t c,
                                           bool &want, bool &rwant) {
  want = rwant = false;
  sm.e[c] = INT32_MIN;
  uint8_t sel = 2;
  const double x = xt[c];
  if (rp.slot) rp.slot[c] = -1;
  if (!o.special[c] && x >= kLMin && x < 1.0e18) {
    const int e = (int)((__double_as_longlong(x) >> 52) & 0x7ff) - 1023;
    const double lo = fmin(x, x + o.pmin[c]), hi = fmax(x, x + o.pmax[c]);
    const double slack = ldexp(1.0, e - 24) + o.sabs[c] * 1e-9;
    if (lo - slack >= ldexp(1.0, e) && hi + slack < ldexp(1.0, e + 1)) {
      const int t = sp.e[2 * c] == e ? 0 : (sp.e[2 * c + 1] == e ? 1 : -1);
      if (t >= 0) {
        sm.e[c] = e;
        if (sm.sel) {
          sel = (uint8_t)t;  // read in place (summ_at)
        } else {
          const long long D = sp.D[2 * c + t], M = sp.M[2 * c + t], N = sp.N[2 * c + t];
          const int A = sp.A[2 * c + t];
#pragma unroll
          for (int q = 0; q < 2; ++q) {
            sm.D[2 * c + q] = D;
            sm.M[2 * c + q] = M;
            sm.N[2 * c + q] = N;
            sm.A[2 * c + q] = A;
          }
        }
      } else {
        want = true;
        // diagnostics (KS_DEBUG_CARRY): no prediction / void summary / other binade
        if (why) atomicAdd(&why[sp.e[2 * c] != INT32_MIN ? 2 : (xh[c] >= kP1SumMin ? 1 : 0)], 1ull);
      }
    }
  }
  if (sm.sel) sm.sel[c] = sel;
  // no summary will serve it: a likely replay unless it enters at 0 or
  // clamps for certain (with a wide margin: a needless prefetch is cheap)
  rwant = rp.slot && !want && sel == 2 && sm.e[c] == INT32_MIN && !o.special[c] && x > 0.0 &&
          !(x + o.pmin[c] < -ldexp(fabs(x) + o.sabs[c], -8));
}

// Wave-aggregated appends of the wave's listed chunks (every lane calls it).
__device__ __forceinline__ void select_append(bool want, bool rwant, int64_t c, int64_t *__restrict__ fix,
                                              unsigned long long *__restrict__ nfix, const ReplayBuf &rp, int hi) {
  const int lane = threadIdx.x & 63;
  const unsigned long long b = __ballot(want);
  if (b) {
    const int leader = __ffsll((long long)b) - 1;
    unsigned long long base = 0;
    if (lane == leader) base = atomicAdd(nfix, (unsigned long long)__popcll(b));
    base = __shfl(base, leader, 64);
    if (want) fix[base + __popcll(b & ((1ull << lane) - 1ull))] = c;
  }
  const unsigned long long br = __ballot(rwant);
  if (br) {
    const int leader = __ffsll((long long)br) - 1;
    unsigned long long base = 0;
    if (lane == leader) base = atomicAdd(rp.count + hi, (unsigned long long)__popcll(br));
    base = __shfl(base, leader, 64);
    const unsigned long long q = base + __popcll(br & ((1ull << lane) - 1ull));
    if (rwant && (int64_t)q < rp.cap) {
      const int64_t sl = hi * rp.cap + (int64_t)q;
      rp.slot[c] = (int32_t)sl;
      rp.chunk[sl] = c;
    }
  }
}

// dst[0, n) = src[0, n), and *dst1 = src[n] (the word after the region counters: kScGuard)
__global__ void k_copy_u64(const unsigned long long *__restrict__ src, unsigned long long *__restrict__ dst, int n,
                           unsigned long long *__restrict__ dst1) {
  for (int i = threadIdx.x; i < n; i += blockDim.x) dst[i] = src[i];
  if (threadIdx.x == 0) *dst1 = src[n];
}

// k_seg_marks and the summary selection in one pass (a wave per 64-chunk window from
// the one holding c0 - 1): the window's segment marks, then the summaries.
__global__ void __launch_bounds__(256) k_marks_select(Chunks g, P1 o, const double *__restrict__ xt,
                                                      uint8_t *__restrict__ flag, int64_t nw, SummP1 sp, Summ sm,
                                                      int64_t *__restrict__ fix, unsigned long long *__restrict__ nfix,
                                                      const double *__restrict__ xh,
                                                      unsigned long long *__restrict__ why, ReplayBuf rp, int hi) {
  const int64_t wv = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (wv >= nw) return;
  const int lane = threadIdx.x & 63;
  const int64_t e = ((g.c0 > 0 ? g.c0 - 1 : 0) / 64 + wv) * 64 + lane;
  bool elig = false, next_run = false;
  if (e + 1 < g.nch && e + 1 >= g.c0) {
    next_run = g.run[e + 1] != g.run[e];
    if (!next_run && e >= g.c0 && !o.special[e]) {
      const double x = xt[e];
      elig = x + o.pmin[e] < -ldexp(fabs(x) + o.sabs[e], -20);  // false for NaN
    }
  }
  const unsigned long long b = __ballot(elig);
  const int f = b ? __ffsll((long long)b) - 1 : 64;
  if (e + 1 < g.nch && e + 1 >= g.c0) flag[e + 1] = (next_run || lane == f) ? 1 : 0;
  if (e == 0 && g.c0 == 0) flag[0] = 1;
  bool want = false, rwant = false;
  if (e >= g.c0 && e < g.nch) select_one(g, o, xt, sp, sm, xh, why, rp, e, want, rwant);
  select_append(want, rwant, e, fix, nfix, rp, hi);
}

// Parity map of a run of steps: entry parity p -> the increment d_p of the
// integer trajectory (exact halves round to even, so a step's increment
// depends on the accumulator's parity).  Composition is associative.
struct PMap {
  long long d0, d1;
};
__device__ __forceinline__ PMap pm_compose(const PMap &a, const PMap &b) {  // a then b
  return PMap{a.d0 + ((a.d0 & 1) ? b.d1 : b.d0), a.d1 + (((1 + a.d1) & 1) ? b.d1 : b.d0)};
}

// Summaries of the listed chunks, one wave per listed chunk (4 indices per lane): the values
// through the expanded table in one or two round trips, the binade-integer
// increments as parity maps, a wave scan of the maps, and wave reductions
// for the total, first maximum and minimum of both entry parities -- the
// same summary chunk_summary_impl computes serially.
template <bool kLds>
__global__ void __launch_bounds__(256) k_summ_fixw(Chunks g, const uint8_t *__restrict__ seq, int64_t total, int k,
                                                   TableView tv, const double *__restrict__ xt,
                                                   const int64_t *__restrict__ fix,
                                                   const unsigned long long *__restrict__ nfix, Summ sm,
                                                   ReplayBuf rp, int hi) {
  __shared__ double s_lut[kLds ? kLdsLutMax : 1];
  if (kLds) {
    for (int i = threadIdx.x; i < tv.nlut; i += blockDim.x) s_lut[i] = tv.lut[i];
    __syncthreads();
  }
  const int lane = threadIdx.x & 63;
  const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int64_t nf = (int64_t)*nfix;
  // the waves past the fix list gather the listed likely replays
  const int64_t nr = rp.slot ? min((int64_t)rp.count[hi], rp.cap) : 0;
  for (int64_t f = (((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6); f < nf + nr; f += nw) {
    if (f >= nf) {
      const int64_t sl = hi * rp.cap + (f - nf);
      const int64_t cr = rp.chunk[sl];
      double v[4];
      values16_nostore<4>(g, seq, total, k, tv, cr, 4 * lane, g.n[cr], v, kLds ? s_lut : nullptr);
      double2 *d = reinterpret_cast<double2 *>(rp.v + sl * 256 + 4 * lane);
      d[0] = make_double2(v[0], v[1]);
      d[1] = make_double2(v[2], v[3]);
      continue;
    }
    const int64_t c = fix[f];
    const int e = binade_of(xt[c]);
    const double scale = ldexp(1.0, 52 - e);
    const int n = g.n[c];
    double v[4];
    values16_nostore<4>(g, seq, total, k, tv, c, 4 * lane, n, v, kLds ? s_lut : nullptr);
    bool ok = true;
    PMap lm{0, 0}, pre[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (4 * lane + q < n) {
        const double y = v[q] * scale;  // exact: power-of-two scaling
        ok &= fabs(y) < 2251799813685248.0;  // 2^51; false for NaN / Inf
        const double fq = floor(y), fr = y - fq;
        const long long qi = ok ? (long long)fq : 0;
        const bool up = fr > 0.5, tie = fr == 0.5;
        const PMap el{qi + ((up || (tie && (qi & 1))) ? 1 : 0), qi + ((up || (tie && ((1 + qi) & 1))) ? 1 : 0)};
        lm = pm_compose(lm, el);
      }
      pre[q] = lm;
    }
    const PPair incp = pp_scan_incl(PPair{lm.d0, lm.d1});
    const PPair excp = pp_prev(incp);
    const PMap exc{excp.d0, excp.d1};
    const PMap tot{rl64(incp.d0, 63), rl64(incp.d1, 63)};
    ok = __all(ok);
    long long M[2], N[2];
    int A[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const long long et = t ? exc.d1 : exc.d0;
      const int pt = (int)((t + et) & 1);  // parity entering this lane's first step
      long long best = LLONG_MIN, mn = LLONG_MAX;
      int barg = 0x7fffffff;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (4 * lane + q < n) {
          const long long val = et + (pt ? pre[q].d1 : pre[q].d0);
          if (val > best) { best = val; barg = 4 * lane + q; }
          mn = min(mn, val);
        }
      }
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) {  // max with the first index, min
        const long long ob = __shfl_xor(best, d, 64);
        const int oa = __shfl_xor(barg, d, 64);
        if (ob > best || (ob == best && oa < barg)) { best = ob; barg = oa; }
        mn = min(mn, (long long)__shfl_xor(mn, d, 64));
      }
      M[t] = best;
      N[t] = mn;
      A[t] = barg;
    }
    const long long lim = 4503599627370496LL;  // 2^52: partial sums exact and far from overflow
    ok = ok && M[0] < lim && M[1] < lim && N[0] > -lim && N[1] > -lim;
    if (lane == 0 && ok) {
      sm.e[c] = e;
      sm.D[2 * c] = tot.d0;
      sm.D[2 * c + 1] = tot.d1;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        sm.M[2 * c + t] = M[t];
        sm.N[2 * c + t] = N[t];
        sm.A[2 * c + t] = A[t];
      }
    }
  }
}

// Segment starts: every run start, and after the first chunk of each
// 64-chunk window that is predicted to clamp by a wide margin (so that the
// exact entry, which differs from x~ by rounding only, clamps too).
__global__ void __launch_bounds__(256) k_seg_marks(Chunks g, P1 o, const double *__restrict__ xt,
                                                   uint8_t *__restrict__ flag, int64_t nw) {
  // windows of 64 chunks from the one holding c0 - 1 (a wave each, nw of
  // them); only this launch's chunks [c0, nch) are read and marked
  const int64_t wv = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (wv >= nw) return;
  const int lane = threadIdx.x & 63;
  const int64_t e = ((g.c0 > 0 ? g.c0 - 1 : 0) / 64 + wv) * 64 + lane;
  bool elig = false, next_run = false;
  if (e + 1 < g.nch && e + 1 >= g.c0) {
    next_run = g.run[e + 1] != g.run[e];
    if (!next_run && e >= g.c0 && !o.special[e]) {
      const double x = xt[e];
      elig = x + o.pmin[e] < -ldexp(fabs(x) + o.sabs[e], -20);  // false for NaN
    }
  }
  const unsigned long long b = __ballot(elig);
  const int f = b ? __ffsll((long long)b) - 1 : 64;
  if (e + 1 < g.nch && e + 1 >= g.c0) flag[e + 1] = (next_run || lane == f) ? 1 : 0;
  if (e == 0 && g.c0 == 0) flag[0] = 1;
}


// Exact carry, one wave per run, walking 64-chunk tiles (lane j <-> chunk
// cb + j).  Per chunk, in order: entry 0 -> clean exit (CLEAN); a binade
// summary valid for the exact entry -> integer step (L; the summaries of the
// tile's lanes are computed wave-parallel, once per binade); a certain clamp
// (x + minprefix < -margin) -> clean exit (R); else exact replay (U).  The
// chain is wave-uniform; L chunks also get their head (max/argmax) here.

// Exact carry, one wave per run, walking 64-chunk tiles (lane j <-> chunk
// cb + j, its inputs in registers, broadcast with v_readlane).  Per chunk, in
// order: entry 0 -> clean exit (CLEAN); the chunk's precomputed binade summary
// is for the exact entry's binade and its integer trajectory stays inside ->
// integer step (L, also yields the head); a certain clamp (x + minprefix <
// -margin) -> clean exit (R); else exact replay (U): the wave loads the 256
// values into registers (4 per lane) and walks them with readlane.
//
// Segments: a run's chain is cut after chunks predicted (x~ from P2, with a
// wide margin) to clamp: the chunk after one starts a segment whose entry is
// assumed to be that chunk's clean exit, and the segments run in parallel.
// The wave of the preceding segment checks the assumption against its exact
// exit (bit 16 of err on mismatch; the host then redoes the carry per run).
// Wave-parallel exact replay of one chunk (U) from its exact entry x > 0, for
// a trajectory that stays positive (no clamp): speculate, then verify.
//  1. approximate prefix sums y_p (wave scan) give each position the binade
//     e_p its exact value S_p should have; every y_p must be farther than
//     the summation error bound from a binade edge and from 0;
//  2. inside a stretch of equal binades, fl(S + s) = S + RN(s / ulp) exactly
//     (lemma 2 of the summaries) once S and the result are known to share
//     binade e: integer increments d_p, an exact segmented prefix scan;
//  3. the first position of each stretch (a binade crossing) is the
//     reference's FP64 add on the exact previous value, walked in order
//     (a few per chunk);
//  4. every integer result is checked to lie strictly inside its binade
//     (m in [2^52 + 1, 2^53 - 2]), every crossing value to have the predicted
//     binade.  Half-ulp ties round to even, i.e. depend on the parity of m:
//     steps are parity pairs composed associatively (as in the summaries).
// Returns false (wave-uniform) if anything cannot be verified: the caller
// replays serially.  On success T = exit, hmax / harg = max and first argmax.
// Positions are lane-major: p = 4 * lane + q.
__device__ bool replay_par(const double v[4], int n, double x, double &T, double &hmax, int &harg) {
  const int lane = threadIdx.x & 63;
  bool live[4];
  double a[4];
  double loc = 0.0, labs = 0.0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    live[q] = 4 * lane + q < n;
    const double vq = live[q] ? v[q] : 0.0;
    loc += vq;
    labs += fabs(vq);
    a[q] = loc;
  }
  const double incl = wave_sum_incl(loc);
  const double sab = rld(wave_sum_incl(labs), 63);
  if (!(sab < 1.0e300)) return false;  // non-finite values: serial
  const double excl = incl - loc;
  const double err = ldexp(x + sab, -42);  // >> 2 * 256 * 2^-53 * (x + sum |s|)
  int e[4];
  bool ok = true;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const double y = x + excl + a[q];
    const double lo = y - err, hi = y + err;
    e[q] = binade_of(y);
    if (live[q]) ok &= lo > 0x1p-1000 && hi < 1.0e300 && binade_of(lo) == binade_of(hi);
  }
  if (!__all(ok)) return false;
  // crossings and integer increments: a step inside binade e adds
  // RN(s / ulp) to the mantissa m; at an exact half the even result wins, so
  // the increment depends on the parity of m: each step is the pair
  // (d0, d1) = increment for an even / odd m, and pairs compose
  // associatively: (f then g)_b = f_b + g_{(b + f_b) & 1}.
  const int ex = binade_of(x);
  const int eprev_lane = wave_prev_i32(e[3]);
  bool cr[4];
  long long d0[4], d1[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int ep = q ? e[q - 1] : (lane ? eprev_lane : ex);
    cr[q] = live[q] && e[q] != ep;
    d0[q] = 0;
    d1[q] = 0;
    if (live[q] && !cr[q]) {
      const double yv = ldexp(v[q], 52 - e[q]);
      const double fl = floor(yv), fr = yv - fl;
      ok &= fabs(yv) < 0x1p60;
      const long long f = (long long)fl;
      if (fr == 0.5) {
        d0[q] = f + (f & 1);
        d1[q] = f + ((1 + f) & 1);
      } else {
        d0[q] = d1[q] = f + (fr > 0.5 ? 1 : 0);
      }
    }
  }
  if (!__all(ok)) return false;
  auto comp = [](long long f0, long long f1, long long g0, long long g1, long long &r0, long long &r1) {
    r0 = f0 + (((f0 & 1) == 0) ? g0 : g1);
    r1 = f1 + ((((1 + f1) & 1) == 0) ? g0 : g1);
  };
  // segmented inclusive scan: (Q0, Q1)[q] = composed increments since the
  // last crossing (a crossing position is a segment head with the identity)
  long long Q0[4], Q1[4];
  long long r0 = 0, r1 = 0;
  bool lflag = false;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (cr[q]) { r0 = 0; r1 = 0; lflag = true; }
    long long n0, n1;
    comp(r0, r1, d0[q], d1[q], n0, n1);
    r0 = n0; r1 = n1;
    Q0[q] = r0;
    Q1[q] = r1;
  }
  // segmented scan of the lane aggregates after their last crossing:
  // (L, R) -> R.f ? R : (L.s then R.s, L.f | R.f); identity ((0, 0), 0)
  SegPP sg{PPair{r0, r1}, lflag ? 1 : 0};
  KS_DPP_SCAN(SegPP, sg, dpp_seg, seg_op);
  const PPair cin = pp_prev(sg.s);  // exclusive carry-in (lane 0: identity)
  long long c0 = cin.d0, c1 = cin.d1;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (cr[q]) break;
    long long n0, n1;
    comp(c0, c1, Q0[q], Q1[q], n0, n1);
    Q0[q] = n0;
    Q1[q] = n1;
  }
  // walk the crossings in order: S_c = fl(S_{c-1} + v_c) on the exact previous value
  long long Mc[4] = {0, 0, 0, 0};
  long long Mcur = mant_of(x);
  unsigned long long lm = __ballot(cr[0] || cr[1] || cr[2] || cr[3]);
  bool good = true;
  while (lm) {
    const int L = __ffsll((long long)lm) - 1;
    lm &= lm - 1;
    const int crm = __builtin_amdgcn_readlane((cr[0] ? 1 : 0) | (cr[1] ? 2 : 0) | (cr[2] ? 4 : 0) | (cr[3] ? 8 : 0), L);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (!(crm & (1 << q))) continue;
      const int p = 4 * L + q;
      double sprev;
      if (p == 0) {
        sprev = x;
      } else {
        const int pl = (p - 1) >> 2, pq = (p - 1) & 3;
        const bool odd = Mcur & 1;
        const long long qsel = pq == 0 ? (odd ? Q1[0] : Q0[0]) : pq == 1 ? (odd ? Q1[1] : Q0[1])
                             : pq == 2 ? (odd ? Q1[2] : Q0[2]) : (odd ? Q1[3] : Q0[3]);
        const int esel = pq == 0 ? e[0] : pq == 1 ? e[1] : pq == 2 ? e[2] : e[3];
        const long long mp = Mcur + rl64(qsel, pl);
        const int ep = rl32(esel, pl);
        good &= mp >= (1LL << 52) + 1 && mp <= (1LL << 53) - 2;
        sprev = from_mant(mp, ep);
      }
      const double vc = rld(v[q], L);
      const double t = sprev + vc;  // the reference's add (kmer_spans.c:269)
      const int ec = rl32(e[q], L);
      good &= t > 0 && binade_of(t) == ec;
      Mcur = mant_of(t);
      if (lane == L) Mc[q] = Mcur;
    }
  }
  if (!good) return false;  // wave-uniform (built from broadcast values)
  // stretch-start mantissa per position (forward fill of the crossings) and
  // the exact values, verified strictly inside their binades
  long long lastm = 0;
  bool has = false;
#pragma unroll
  for (int q = 0; q < 4; ++q)
    if (cr[q]) { lastm = Mc[q]; has = true; }
  // forward fill: (L, R) -> (R.f ? R.m : L.m, L.f | R.f); identity (0, 0)
  FillM fw{lastm, has ? 1 : 0};
  KS_DPP_SCAN(FillM, fw, dpp_fill, fill_op);
  long long start_m = wave_prev_i64(fw.m);
  const int start_f = wave_prev_i32(fw.f);
  if (lane == 0 || !start_f) start_m = mant_of(x);
  double S[4];
  bool inb = true;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (cr[q]) start_m = Mc[q];
    const long long m = cr[q] ? start_m : start_m + ((start_m & 1) ? Q1[q] : Q0[q]);
    if (live[q] && !cr[q]) inb &= m >= (1LL << 52) + 1 && m <= (1LL << 53) - 2;
    S[q] = from_mant(m, e[q]);
  }
  if (!__all(inb)) return false;
  // exit, max and first argmax
  const int pl = (n - 1) >> 2, pq = (n - 1) & 3;
  const double slast = pq == 0 ? S[0] : pq == 1 ? S[1] : pq == 2 ? S[2] : S[3];
  T = rld(slast, pl);
  double bm = -1.0;
  int bi = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q)
    if (live[q] && S[q] > bm) { bm = S[q]; bi = 4 * lane + q; }
  // wave max (the DPP identity 0.0 is below no result: every S is >= 0)
  double wm = bm;
  auto dmax = [](double a, double b) { return fmax(a, b); };
  KS_DPP_SCAN(double, wm, dpp_f64, dmax);
  wm = rld(wm, 63);
  const unsigned long long bl = __ballot(bm == wm && bm >= 0.0);
  const int fl = __ffsll((long long)bl) - 1;
  hmax = wm;
  harg = __builtin_amdgcn_readlane(bi, fl);
  return true;
}

template <bool kCompressed>
__device__ __forceinline__ void carry_segment(const Chunks &g, int64_t c0, int64_t c1, const uint8_t *__restrict__ seq,
                                              int64_t total, int k, const TableView &tv,
                                              const uint16_t *__restrict__ codes, const P1 &o, const Summ &sm,
                                              const Carry &cr, const TileComp &tc, const ReplayBuf &rp,
                                              unsigned long long *__restrict__ nreplay,
                                              unsigned int *__restrict__ err, long long *__restrict__ dbg,
                                              int64_t r) {
  const int lane = threadIdx.x & 63;
  // (the cooperative FP64 line fetch of the replays, values4_coop_f64: a wave's slice)
  __shared__ uint4 s_coop[4][256];
  __shared__ unsigned long long s_ckey[4][64];
  double x = (c0 > 0 && g.run[c0] == g.run[c0 - 1]) ? o.cexit[c0 - 1] : 0.0;
  unsigned long long replays = 0;
  const long long t_start = dbg ? (long long)__builtin_amdgcn_s_memtime() : 0;
  long long n_l = 0, n_r = 0, n_par = 0;  // diagnostics: replays that clamp, replayed indices
  // per-lane inputs of one 64-chunk tile; the next tile's are loaded before
  // the current one is processed (all loads independent: hides their latency
  // behind the tile's scan)
  // (start: a replay's first memory round trip -- chunk start, then its
  // packed bases, then the table -- is taken here, with the tile's loads)
  struct TileIn {
    double exit, pmin, sabs;
    int64_t start;
    int spec, n, se, rs;
    long long D[2], M[2], N[2];
    int A[2];
  };
  auto load_tile = [&](int64_t cb, int64_t ce, TileIn &t) {
    const int64_t c = cb + lane;
    const bool live = c < ce;
    const int64_t cc = live ? c : c0;  // dead lanes read a valid chunk, values unused
    t.exit = o.cexit[cc];
    t.pmin = o.pmin[cc];
    t.sabs = o.sabs[cc];
    t.spec = live ? o.special[cc] : 1;
    t.n = live ? g.n[cc] : 0;
    t.start = g.start[cc];
    t.rs = (live && rp.slot) ? rp.slot[cc] : -1;
    const int se = sm.e[cc];
    t.se = live ? se : INT32_MIN;
    const SummAt r = summ_at(sm, cc);
    t.D[0] = r.D[r.i0];
    t.D[1] = r.D[r.i1];
    t.M[0] = r.M[r.i0];
    t.M[1] = r.M[r.i1];
    t.N[0] = r.N[r.i0];
    t.N[1] = r.N[r.i1];
    t.A[0] = r.A[r.i0];
    t.A[1] = r.A[r.i1];
  };
  // tiles are the global 64-chunk tiles (partial at the segment's ends)
  auto tile_end = [&](int64_t cb) { return min(c1, (cb & ~(int64_t)63) + 64); };
  TileIn cur;
  load_tile(c0, tile_end(c0), cur);
  long long t_fast = 0, t_rep = 0;  // diagnostics: cycles in fast tiles, in replays
  bool try_batch = true;
  // the packed bases of the chunk after a replayed one, loaded under that
  // replay's table reads (replays come in runs where the carry crosses
  // binades): pf_c = the chunk they belong to, pf_ok = packed_bits' result
  int64_t pf_c = -1;
  bool pf_ok = false;
  uint64_t pf_x = 0;
  for (int64_t cb = c0; cb < c1;) {
    const long long tt0 = dbg ? (long long)__builtin_amdgcn_s_memtime() : 0;
    // Tile batch: up to 64 whole tiles at once from their composites (the
    // serial fast path's test per tile, with the entries of all of them from
    // one wave scan of the composed increments); accepted tiles are expanded
    // per chunk by k_tile_apply.  The first rejected tile takes the per-tile
    // path below.
    if (tc.e && try_batch && (cb & 63) == 0 && x >= kLMin && x < 1.0e18) {
      const int e = binade_of(x);
      const int64_t ntl = min((int64_t)64, (c1 - cb) >> 6);
      if (e >= 6 && e <= 58 && ntl >= 2) {
        const int64_t t = (cb >> 6) + lane;
        const bool in = lane < ntl;
        const int te = in ? tc.e[t] : INT32_MIN;
        long long d0 = 0, d1 = 0, lo0 = 0, lo1 = 0, hi0 = -1, hi1 = -1;
        if (in) {
          d0 = tc.D[2 * t];
          d1 = tc.D[2 * t + 1];
          lo0 = tc.LO[2 * t];
          lo1 = tc.LO[2 * t + 1];
          hi0 = tc.HI[2 * t];
          hi1 = tc.HI[2 * t + 1];
        }
        if (!in || te != e) d0 = d1 = 0;  // identity beyond the first rejected tile (never used)
        const PPair ip = pp_scan_incl(PPair{d0, d1});  // inclusive composed increments
        const PPair xp = pp_prev(ip);
        const long long i0 = ip.d0, i1 = ip.d1, x0 = xp.d0, x1 = xp.d1;
        const long long m0 = mant_of(x);
        const long long mt = m0 + ((m0 & 1) ? x1 : x0);  // entry mantissa of tile t
        const int pt = (int)(mt & 1);
        const bool ok = in && te == e && mt >= (pt ? lo1 : lo0) && mt <= (pt ? hi1 : hi0);
        const unsigned long long bad = __ballot(!ok);
        const int f = bad ? __ffsll((long long)bad) - 1 : 64;
        if (f > 0) {
          if (lane < f) {
            tc.em[t] = mt;
            tc.ee[t] = e;
          }
          const long long mi = m0 + ((m0 & 1) ? i1 : i0);  // exit of tile t
          x = from_mant(rl64(mi, f - 1), e);
          n_l += 64 * f;
          cb += 64 * f;
          if (dbg) t_fast += (long long)__builtin_amdgcn_s_memtime() - tt0;
          if (cb >= c1) break;
          load_tile(cb, tile_end(cb), cur);
          try_batch = f == 64;  // a rejected tile goes through the per-tile path first
          continue;
        }
      }
    }
    try_batch = true;
    const int64_t ce = tile_end(cb);
    if (lane == 0 && tc.ee) tc.ee[cb >> 6] = INT32_MIN;  // not batched (the fallback pass reruns segments)
    TileIn nxt = cur;
    if (ce < c1) load_tile(ce, tile_end(ce), nxt);
    const int64_t c = cb + lane;
    const bool live = c < ce;
    const double l_exit = live ? cur.exit : 0.0;
    const double l_pmin = live ? cur.pmin : 0.0;
    const double l_sabs = live ? cur.sabs : 0.0;
    const int l_spec = cur.spec;
    const int l_n = cur.n;
    const int se = cur.se;
    long long D[2] = {0, 0}, M[2] = {0, 0}, N[2] = {0, 0};
    int A[2] = {0, 0};
    if (se != INT32_MIN) {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        D[t] = cur.D[t];
        M[t] = cur.M[t];
        N[t] = cur.N[t];
        A[t] = cur.A[t];
      }
    }
    const int nb = (int)(ce - cb);
    double my_x = 0.0, my_hmax = -1.0;
    int my_mode = kModeClean, my_harg = 0, my_hq = -1;
    // Runs of summary chunks: from chunk j on, the chunks that have a summary
    // for the binade of the exact carry and stay inside it are taken at once:
    // their integer maps m -> m + D[m & 1] composed by a wave scan (chunks
    // before j and past the tile: identity), each checked at its exact entry.
    // The first other chunk takes the serial step.  (A fast tile is one run
    // from j = 0; a replay in mid-tile no longer walks the rest serially.)
    bool tile_done = true;  // diagnostics: no serial step in this tile
    for (int j = 0; j < nb; ++j) {
      if (x >= kLMin && x < 1.0e18 && rl32(se, j) == binade_of(x)) {
        const int e = binade_of(x);
        const bool in = live && lane >= j;
        const PPair ip = pp_scan_incl(PPair{in ? D[0] : 0, in ? D[1] : 0});  // inclusive composed map
        const PPair xp = pp_prev(ip);
        const long long x0 = xp.d0, x1 = xp.d1;
        const long long m0 = mant_of(x);
        const long long mj = m0 + ((m0 & 1) ? x1 : x0);  // exact entry of this lane's chunk
        const int pj = (int)(mj & 1);
        const bool ok = lane < j || (in && se == e && mj + (pj ? N[1] : N[0]) >= (1LL << 52) + 1 &&
                                     mj + (pj ? M[1] : M[0]) <= (1LL << 53) - 2);
        const unsigned long long bad = __ballot(!ok);
        const int f = bad ? __ffsll((long long)bad) - 1 : 64;  // <= nb
        if (f > j) {
          if (lane >= j && lane < f) {
            my_x = from_mant(mj, e);
            my_mode = kModeL;
            my_hmax = from_mant(mj + (pj ? M[1] : M[0]), e);
            my_harg = pj ? A[1] : A[0];
          }
          x = from_mant(rl64(mj + (pj ? D[1] : D[0]), f - 1), e);
          n_l += f - j;
          j = f - 1;
          continue;
        }
      }
      // Runs of clean and certain-clamp chunks at once: both leave the
      // chunk's clean exit, so from chunk j on, a chunk entered by its
      // predecessor's clean exit (x for chunk j) that enters at 0 or clamps
      // for certain -- and has no summary for its entry's binade, which the
      // serial order tries first -- takes its mode here; the first other
      // chunk takes the serial step.  (Weighted rank at config 3: 11 M of
      // 12 M chunks are clean or clamp; in-process k = 15 44.2 vs 44.9 ms,
      // k = 13 30.1 vs 30.6, metric unchanged: profiles/r5/ab/ab_bulk_clean_*.txt)
      {
        const double pe = __longlong_as_double(wave_prev_i64(__double_as_longlong(l_exit)));
        const double ent = lane == j ? x : pe;
        const bool in = live && lane >= j;
        const bool cl = ent == 0.0;
        const bool sm_ok = se != INT32_MIN && ent >= kLMin && ent < 1.0e18 && se == binade_of(ent);
        const bool rc = !cl && !sm_ok && !l_spec && ent + l_pmin < -ldexp(fabs(ent) + l_sabs, -40);
        const bool ok = lane < j || (in && (cl || rc));
        const unsigned long long bad = __ballot(!ok);
        const int f = bad ? __ffsll((long long)bad) - 1 : 64;
        if (f > j) {
          if (lane >= j && lane < f) {
            my_x = ent;
            my_mode = cl ? kModeClean : kModeR;
          }
          if (dbg) n_r += __popcll(__ballot(lane >= j && lane < f && rc));
          x = rld(l_exit, f - 1);
          j = f - 1;
          continue;
        }
      }
      tile_done = false;
      const double cj_exit = rld(l_exit, j);
      if (lane == j) my_x = x;
      int mode = kModeU;
      bool done = false;
      if (x == 0.0) {
        mode = kModeClean;
        x = cj_exit;
        done = true;
      } else if (x >= kLMin && x < 1.0e18 && rl32(se, j) == binade_of(x)) {
        const int e = binade_of(x);
        const long long m0 = mant_of(x);
        const int par = (int)(m0 & 1);
        const long long Nj = rl64(par ? N[1] : N[0], j), Mj = rl64(par ? M[1] : M[0], j);
        if (m0 + Nj >= (1LL << 52) + 1 && m0 + Mj <= (1LL << 53) - 2) {
          const long long Dj = rl64(par ? D[1] : D[0], j);
          mode = kModeL;
          if (lane == j) {
            my_hmax = from_mant(m0 + Mj, e);
            my_harg = par ? A[1] : A[0];
          }
          x = from_mant(m0 + Dj, e);
          done = true;
        }
      }
      if (!done && !rl32(l_spec, j) && x + rld(l_pmin, j) < -ldexp(fabs(x) + rld(l_sabs, j), -40)) {
        mode = kModeR;  // certain clamp -> coincides with the clean trajectory
        x = cj_exit;
        done = true;
      }
      const long long tr0 = dbg ? (long long)__builtin_amdgcn_s_memtime() : 0;
      if (!done) {  // exact replay of chunk cb + j from x; also yields its head
        mode = kModeU;
        ++replays;
        const int64_t cj = cb + j;
        const int n = rl32(l_n, j);
        double v[4];
        const int rsj = rl32(cur.rs, j);
        if (rsj >= 0) {  // gathered ahead (k_summ_fixw)
          const double2 *d = reinterpret_cast<const double2 *>(rp.v + (int64_t)rsj * 256 + 4 * lane);
          const double2 a = d[0], b = d[1];
          v[0] = a.x;
          v[1] = a.y;
          v[2] = b.x;
          v[3] = b.y;
        } else {
          const bool hx = !kCompressed && pf_c == cj && pf_ok;
          if (dbg && hx) n_par += 1LL << 32;  // (diagnostics: replays with their bases prefetched)
          uint64_t xq = pf_x;
          // (in-process at config 3: 24.63 vs 25.00 ms min, carry 4.83 vs 5.18 ms,
          // profiles/r6/rank/ab_carry_coop.txt)
          const bool coop = !kCompressed && tv.line && tv.line_kind == 2 && tv.line_own == 3 &&
                            __ballot(!(hx || packed_bits(g.packed, total, rl64(cur.start, j) + 4 * lane - k, xq))) == 0;
          if (coop) {
            values4_coop_f64(tv, xq, k, 4 * lane, n, v, s_coop[threadIdx.x >> 6], s_ckey[threadIdx.x >> 6]);
          } else {
            values4(g, seq, total, k, tv, kCompressed ? codes : nullptr, cj, rl64(cur.start, j), 4 * lane, n, v, hx,
                    pf_x);
          }
        }
        if (!kCompressed && cj + 1 < c1) {  // the next chunk's packed bases, under this replay's reads
          const int64_t stn = (j + 1 < nb) ? rl64(cur.start, j + 1) : rl64(nxt.start, 0);
          pf_ok = packed_bits(g.packed, total, stn + 4 * lane - k, pf_x);
          pf_c = cj + 1;
        }
        double T = x, hmax = -1.0;
        int hq = -1, harg = 0;
        const bool par = replay_par(v, n, x, T, hmax, harg);
        if (par) n_par += 1;
        for (int i = 0; i < 64 && hq < 0 && !par; ++i) {
          if (4 * i >= n) break;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int idx = 4 * i + q;
            if (idx < n && hq < 0) {
              const double t = T + rld(v[q], i);
              T = t > 0 ? t : 0.0;
              if (T == 0.0) hq = idx;
              else if (T > hmax) { hmax = T; harg = idx; }
            }
          }
        }
        if (lane == j) {
          my_hq = hq;
          my_hmax = hmax;
          my_harg = harg;
        }
        x = hq >= 0 ? cj_exit : T;
        if (dbg) t_rep += (long long)__builtin_amdgcn_s_memtime() - tr0;
      }
      if (lane == j) my_mode = mode;
      n_l += mode == kModeL;
      n_r += mode == kModeR;
    }
    if (live) {
      cr.x[c] = my_x;
      cr.mode[c] = (uint8_t)my_mode;
      if (my_mode == kModeL || my_mode == kModeU) {
        cr.hq[c] = my_hq;
        cr.hmax[c] = my_hmax;
        cr.harg[c] = my_harg;
      }
    }
    if (dbg && tile_done) t_fast += (long long)__builtin_amdgcn_s_memtime() - tt0;
    cur = nxt;
    cb = ce;
  }
  if (lane == 0 && replays) atomicAdd(nreplay, replays);
  if (lane == 0 && c1 < g.nch && g.run[c1] == g.run[c1 - 1] &&
      __double_as_longlong(x) != __double_as_longlong(o.cexit[c1 - 1]))
    atomicOr(err, 16u);  // the next segment assumed a different entry
  if (dbg && lane == 0) {  // accumulated per block (several segments per window)
    dbg[9 * r + 0] += (long long)__builtin_amdgcn_s_memtime() - t_start;
    dbg[9 * r + 1] += c1 - c0;
    dbg[9 * r + 2] += (long long)replays;
    dbg[9 * r + 3] += 1;
    dbg[9 * r + 4] += n_l;
    dbg[9 * r + 5] += n_r;
    dbg[9 * r + 6] += t_fast;
    dbg[9 * r + 7] += t_rep;
    dbg[9 * r + 8] += n_par;
  }
}

// Exact carry (tables of small integers, ks_table::int_exact): every partial
// sum is exact in FP64, so the max-plus prescan xt (k_ascan_*) is the exact
// entry of every chunk -- max(x + sum, clean exit) composes exactly -- and a
// chunk's carried head follows from its pass-1 aggregates: entered at 0, the
// clean trajectory; no clamp (x + prefix min > 0), the trajectory x + prefix
// with its maximum x + pmax first reached at parg (mode L); else mode R (the
// head up to the clamp: k_heads).  Replaces the predictor, the binade
// summaries and the replays.
__global__ void __launch_bounds__(256) k_carry_exact(Chunks g, P1 o, const double *__restrict__ xt, Carry cr) {
  const int64_t c = g.c0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= g.nch) return;
  const double x = xt[c];
  cr.x[c] = x;
  if (x == 0.0) {
    cr.mode[c] = (uint8_t)kModeClean;
  } else if (x + o.pmin[c] > 0.0) {
    cr.mode[c] = (uint8_t)kModeL;
    cr.hq[c] = -1;
    cr.hmax[c] = x + o.pmax[c];
    cr.harg[c] = o.parg[c];
  } else {
    cr.mode[c] = (uint8_t)kModeR;
  }
}

// Tile composites (TileComp) of the global tiles of chunks [g.c0, g.nch):
// one wave per tile, from the final summaries (after k_summ_fixw).  Also
// clears the batch marks (ee) of the range.
__global__ void __launch_bounds__(256) k_tile_comp(Chunks g, Summ sm, TileComp tc) {
  const int lane = threadIdx.x & 63;
  const int64_t t = (g.c0 >> 6) + (((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  if (g.nch <= g.c0 || t > ((g.nch - 1) >> 6)) return;  // whole waves
  const int64_t c = 64 * t + lane;
  const bool live = c >= g.c0 && c < g.nch;
  const int se = live ? sm.e[c] : INT32_MIN;
  const int e = __builtin_amdgcn_readfirstlane(se);
  if (lane == 0) tc.ee[t] = INT32_MIN;
  if (e == INT32_MIN || !__all(live && se == e)) {
    if (lane == 0) tc.e[t] = INT32_MIN;
    return;
  }
  const SummAt r = summ_at(sm, c);
  const long long D0 = r.D[r.i0], D1 = r.D[r.i1];
  const long long M0 = r.M[r.i0], M1 = r.M[r.i1];
  const long long N0 = r.N[r.i0], N1 = r.N[r.i1];
  const PPair ip = pp_scan_incl(PPair{D0, D1});
  const PPair xp = pp_prev(ip);
  const long long i0 = ip.d0, i1 = ip.d1, x0 = xp.d0, x1 = xp.d1;
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    // entry mantissa m (parity p): chunk lane enters at m + inc with parity pj
    // and stays in the binade iff m + inc + N_pj >= 2^52 + 1 and
    // m + inc + M_pj <= 2^53 - 2 (carry_segment's fast-tile test)
    const long long inc = p ? x1 : x0;
    const int pj = (int)((p + inc) & 1);
    long long lo = (1LL << 52) + 1 - inc - (pj ? N1 : N0);
    long long hi = (1LL << 53) - 2 - inc - (pj ? M1 : M0);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      lo = max(lo, (long long)__shfl_xor(lo, d, 64));
      hi = min(hi, (long long)__shfl_xor(hi, d, 64));
    }
    const long long tot = __shfl(p ? i1 : i0, 63, 64);
    if (lane == 0) {
      tc.D[2 * t + p] = tot;
      tc.LO[2 * t + p] = lo;
      tc.HI[2 * t + p] = hi;
    }
  }
  if (lane == 0) tc.e[t] = e;
}

// Per-chunk carry of the tiles accepted in batches (ee != INT32_MIN): the
// fast-tile path of carry_segment from the tile's exact entry.  gated: only
// after a fallback (bit 16 of err), for the tiles k_carry_run batched.
__global__ void __launch_bounds__(256) k_tile_apply(Chunks g, Summ sm, TileComp tc, Carry cr,
                                                    const unsigned int *__restrict__ err, int gated) {
  const int lane = threadIdx.x & 63;
  const int64_t t = (g.c0 >> 6) + (((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  if (g.nch <= g.c0 || t > ((g.nch - 1) >> 6)) return;
  if (gated && !(*(volatile const unsigned int *)err & 16u)) return;
  const int e = tc.ee[t];
  if (e == INT32_MIN) return;
  const long long m = tc.em[t];
  const int64_t c = 64 * t + lane;
  const bool live = c < g.nch;
  const int64_t cc = live ? c : 64 * t;
  const SummAt r = summ_at(sm, cc);
  const long long D0 = r.D[r.i0], D1 = r.D[r.i1];
  const PPair xp = pp_prev(pp_scan_incl(PPair{live ? D0 : 0, live ? D1 : 0}));
  const long long x0 = xp.d0, x1 = xp.d1;
  if (!live) return;
  const long long mj = m + ((m & 1) ? x1 : x0);
  const int pj = (int)(mj & 1);
  cr.x[c] = from_mant(mj, e);
  cr.mode[c] = (uint8_t)kModeL;
  cr.hq[c] = -1;
  cr.hmax[c] = from_mant(mj + r.M[pj ? r.i1 : r.i0], e);
  cr.harg[c] = r.A[pj ? r.i1 : r.i0];
}

// Carry by window: block w runs the segments that start in chunks
// [64w, 64w + 64) (segment starts flagged by k_seg_marks; a segment ends at
// the next flagged chunk, possibly windows later).
// kW: waves per SIMD the register allocation must allow (3: the FP64 form
// fits 168 VGPRs without spills instead of taking 170 at 2 waves; weighted
// rank in-process k = 13 30.4 vs 31.6 ms, k = 15 53.6 vs 55.1, metric
// unchanged: profiles/r5/ab/ab_carry_occ*.txt; 4 waves spill 64-87 VGPRs)
template <bool kCompressed, int kW = 3>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(kW, 8))) k_carry_win(Chunks g, const uint8_t *__restrict__ flag,
                                                  const uint8_t *__restrict__ seq, int64_t total, int k, TableView tv,
                                                  const uint16_t *__restrict__ codes, P1 o, Summ sm, Carry cr,
                                                  TileComp tc, ReplayBuf rp, unsigned long long *__restrict__ nreplay,
                                                  unsigned int *__restrict__ err, long long *__restrict__ dbg) {
  // a wave per window: segment starts in [c0, nch); segments end by nch
  const int64_t w = g.c0 / 64 + (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (g.nch <= 0 || w > (g.nch - 1) / 64) return;
  const int lane = threadIdx.x & 63;
  const int64_t base = w * 64;
  unsigned long long m = __ballot(base + lane >= g.c0 && base + lane < g.nch && flag[base + lane]);
  while (m) {
    const int b = __ffsll((long long)m) - 1;
    m &= m - 1;
    const int64_t c0 = base + b;
    int64_t c1 = g.nch;
    if (m) {
      c1 = base + __ffsll((long long)m) - 1;
    } else {
      for (int64_t nb = base + 64; nb < g.nch; nb += 64) {
        const unsigned long long mm = __ballot(nb + lane < g.nch && flag[nb + lane]);
        if (mm) {
          c1 = nb + __ffsll((long long)mm) - 1;
          break;
        }
      }
    }
    carry_segment<kCompressed>(g, c0, c1, seq, total, k, tv, codes, o, sm, cr, tc, rp, nreplay, err, dbg, w);
  }
}

// Carry by run (the fallback when a segment assumption failed): gated on
// bit 16 of err, so it can be queued unconditionally.
template <bool kCompressed>
__global__ void __launch_bounds__(64) k_carry_run(Chunks g, const int64_t *__restrict__ cbase, int64_t nruns,
                                                  const uint8_t *__restrict__ seq, int64_t total, int k, TableView tv,
                                                  const uint16_t *__restrict__ codes, P1 o, Summ sm, Carry cr,
                                                  TileComp tc, ReplayBuf rp, unsigned long long *__restrict__ nreplay,
                                                  unsigned int *__restrict__ err, long long *__restrict__ dbg,
                                                  int64_t r_lo) {
  const int64_t r = r_lo + blockIdx.x;
  if (r >= nruns || !(*(volatile unsigned int *)err & 16u)) return;
  const int64_t c0 = cbase[r], c1 = cbase[r + 1];
  if (c0 < c1) carry_segment<kCompressed>(g, c0, c1, seq, total, k, tv, codes, o, sm, cr, tc, rp, nreplay, err, nullptr, r);
}

// Fallback preparation: after a failed segment check, the first heads pass
// may have flagged clamps against the wrong carry; clear everything but 16.
__global__ void k_fallback_prep(unsigned int *__restrict__ err, unsigned long long *__restrict__ nreplay,
                                int force) {
  if (force) *err |= 16u;
  if (*err & 16u) {
    *err = 16u;
    *nreplay = 0;
  }
}


// ------------------------------------------------------------------- P4

// (Head and head_step: before P1Lane, whose exact-entry flavour walks the head too.)

// Heads of the R chunks (the carried excursion up to its certain clamp):
// lane per chunk, from the exact entry.  Uncompressed tables read the
// expanded table (J indices per read) like P1.
template <int J, bool kCompressed, bool kWide = false>
__device__ __forceinline__ void head_walk(const Chunks &g, const uint8_t *__restrict__ seq, int64_t total, int k,
                                          const TableView &tv, const uint16_t *__restrict__ codes, const Carry &cr,
                                          unsigned int *__restrict__ err, int64_t c) {
  const uint32_t *__restrict__ packed = g.packed;
  const double x = cr.x[c];
  const int n = g.n[c];
  const int64_t start = g.start[c];
  Head h{x, -1.0, 0, -1};
  if (kCompressed) {
    for (int b0 = 0; b0 < n && h.hq < 0; b0 += NB) {
      double v[NB];
      if (!codes) {
        values16_nostore(g, seq, total, k, tv, c, b0, n, v, nullptr);
      } else {
        uint32_t w[8];
        load_codes16(codes, c, b0, w);
#pragma unroll
        for (int j = 0; j < NB; ++j) v[j] = tv.lut[(w[j >> 1] >> (16 * (j & 1))) & 0xffffu];
      }
#pragma unroll
      for (int j = 0; j < NB; ++j) h = head_step(h, v[j], b0 + j, n);
    }
  } else if (tv.line) {  // FP64 line table: OWN + 1 indices per read
    const uint32_t mask = (1u << (2 * k)) - 1u;
    uint64_t xp = 0;
    uint32_t code = packed_bits(packed, total, start - k, xp) ? (uint32_t)(xp >> (64 - 2 * k))
                                                              : prime_code_guarded(seq, start - k, k, total);
    // (kWide: two batches' reads in flight per round trip; FP64 line tables)
    constexpr int NW = kWide ? 2 * NB : NB;
    for (int b0 = 0; b0 < n && h.hq < 0; b0 += NW) {
      double v[NW];
      values16_f64(g, seq, total, k, tv, start, b0, n, code, mask, v);
      if (kWide) values16_f64(g, seq, total, k, tv, start, b0 + NB, n, code, mask, v + NB);
#pragma unroll
      for (int j = 0; j < NW; ++j) h = head_step(h, v[j], b0 + j, n);
    }
  } else {
    constexpr int G = (J == 1) ? 16 : (J == 4 ? 4 : 8);
    constexpr int PB = G * J;
    const int kx = k + J - 1;
    const uint32_t xmask = (kx >= 16) ? 0xffffffffu : ((1u << (2 * kx)) - 1u);
    // prime and the first batch's bases from the packed codes: one round trip
    uint64_t xp = 0;
    uint32_t gcode = packed_bits(packed, total, start - k, xp) ? (uint32_t)(xp >> (64 - 2 * kx))
                                                               : prime_code_guarded(seq, start - k, kx, total);
    for (int b0 = 0; b0 < n && h.hq < 0; b0 += PB) {
      uint32_t gc[G];
      uint64_t xb = 0;
      if (2 * PB <= 64 && packed_bits(packed, total, start + b0 + J - 1, xb)) {
#pragma unroll
        for (int gi = 0; gi < G; ++gi) {
          gc[gi] = gcode;
          gcode = ((gcode << (2 * J)) | (uint32_t)((xb >> (64 - 2 * J * (gi + 1))) & ((1u << (2 * J)) - 1u))) & xmask;
        }
      } else {
        uint8_t by[32];
        load16(seq, start + b0 + J - 1, total, by);
        if (PB > 16) load16(seq, start + b0 + J - 1 + 16, total, by + 16);
#pragma unroll
        for (int gi = 0; gi < G; ++gi) {
          gc[gi] = gcode;
#pragma unroll
          for (int t = 0; t < J; ++t) gcode = ((gcode << 2) | enc(by[gi * J + t])) & xmask;
        }
      }
      double v[PB];
#pragma unroll
      for (int gi = 0; gi < G; ++gi) {
        const bool live = b0 + gi * J < n;
        if (J == 1) {
          v[gi] = live ? tv.vals[gc[gi]] : 0.0;
        } else {
          double2 e0 = make_double2(0.0, 0.0), e1 = e0;
          if (live) {
            const double2 *E = reinterpret_cast<const double2 *>(tv.ext);
            if (J <= 2) {
              e0 = E[gc[gi]];
            } else {
              e0 = E[2 * (size_t)gc[gi]];
              e1 = E[2 * (size_t)gc[gi] + 1];
            }
          }
          const double ev[4] = {e0.x, e0.y, e1.x, e1.y};
#pragma unroll
          for (int t = 0; t < J; ++t) v[gi * J + t] = ev[t];
        }
      }
#pragma unroll
      for (int j = 0; j < PB; ++j) h = head_step(h, v[j], b0 + j, n);
    }
  }
  if (h.hq < 0) atomicOr(err, 2u);  // predicted clamp did not happen
  cr.hq[c] = h.hq;
  cr.hmax[c] = h.hmax;
  cr.harg[c] = h.harg;
}

template <int J, bool kCompressed, bool kWide = false>
__device__ __forceinline__ void head_one(const Chunks &g, const uint8_t *__restrict__ seq, int64_t total, int k,
                                         const TableView &tv, const uint16_t *__restrict__ codes, const Carry &cr,
                                         unsigned int *__restrict__ err, int64_t c) {
  const int mode = cr.mode[c];
  if (mode == kModeL || mode == kModeU) return;  // head written by the carry (summary / replay)
  cr.hq[c] = -1;
  cr.hmax[c] = -1.0;
  cr.harg[c] = 0;
  if (mode == kModeClean) return;
  head_walk<J, kCompressed, kWide>(g, seq, total, k, tv, codes, cr, err, c);
}

// gated: the second pass, after a fallback only (bit 16 of err); queued
// unconditionally on a small grid (a grid-stride loop), so that the common
// case costs one short launch instead of a block per 256 chunks (80 us of
// empty blocks at the metric genome's second part)
template <int J, bool kCompressed, bool kWide = false>
__global__ void __launch_bounds__(256) k_heads(Chunks g, const uint8_t *__restrict__ seq, int64_t total,
                                               int k, TableView tv, const uint16_t *__restrict__ codes,
                                               Carry cr, unsigned int *__restrict__ err, int gated) {
  if (gated && !(*(volatile unsigned int *)err & 16u)) return;  // second pass only after a fallback
  for (int64_t c = g.c0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < g.nch;
       c += (int64_t)gridDim.x * blockDim.x)
    head_one<J, kCompressed, kWide>(g, seq, total, k, tv, codes, cr, err, c);
}

// k_heads with the R chunks packed densely: a wave takes 256 chunks, lists
// its R chunks in LDS (ballot order) and walks them 64 at a time, so every
// lane of a walking wave has a head to walk (weighted rank: ~28% of the
// chunks are R, scattered; config 3 in-process 29.18 vs 29.90 ms, k = 15
// 43.7 vs 43.8: profiles/r5/ab/ab_heads_dense_lane_pf_*.txt, where the next
// rescan batch's bases loaded one batch ahead measured slower, 29.18 vs 28.51).
constexpr int kHeadSpan = 256;
template <int J, bool kCompressed, bool kWide = false>
__global__ void __launch_bounds__(256) k_heads_dense(Chunks g, const uint8_t *__restrict__ seq, int64_t total,
                                                     int k, TableView tv, const uint16_t *__restrict__ codes,
                                                     Carry cr, unsigned int *__restrict__ err, int gated) {
  if (gated && !(*(volatile unsigned int *)err & 16u)) return;
  __shared__ int32_t s_list[4][kHeadSpan];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t sp = g.c0 + (((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6) * kHeadSpan; sp < g.nch;
       sp += nw * kHeadSpan) {
    int cnt = 0;
#pragma unroll
    for (int q = 0; q < kHeadSpan / 64; ++q) {
      const int64_t c = sp + q * 64 + lane;
      bool isr = false;
      if (c < g.nch) {
        const int mode = cr.mode[c];
        if (mode == kModeClean || mode == kModeR) {
          cr.hq[c] = -1;
          cr.hmax[c] = -1.0;
          cr.harg[c] = 0;
        }
        isr = mode == kModeR;
      }
      const unsigned long long b = __ballot(isr);
      if (isr) s_list[w][cnt + __popcll(b & ((1ull << lane) - 1ull))] = q * 64 + lane;
      cnt += __popcll(b);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (int t = lane; t < cnt; t += 64)
      head_walk<J, kCompressed, kWide>(g, seq, total, k, tv, codes, cr, err, sp + s_list[w][t]);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
}

// ------------------------------------------------------------------- P5

// One lane's emission (sporadic callers).
__device__ __forceinline__ void emit(const Emission &e, const RegionBuf &rb, const Rescan &rs, int32_t sid,
                                     double best) {
  if (e.reg) push_region(rb, sid, e.rbeg, e.rend, best);
  if (e.res) {
    const int64_t slot = append_one(rs.count, rs.segcap);
    if (slot >= 0) {
      rs.a[slot] = e.res_a;
      rs.b[slot] = e.res_b;
      rs.seq[slot] = sid;
    }
  }
}

// emit() for a whole wave (every lane calls it): one atomic per wave and
// buffer segment instead of one per record.
__device__ __forceinline__ void emit_wave(const Emission &e, const RegionBuf &rb, const Rescan &rs, int32_t sid,
                                          double best) {
  const unsigned long long m = __ballot(e.reg);
  const unsigned long long mr = __ballot(e.res);
  if ((m | mr) == 0) return;
  const int lane = (int)(threadIdx.x & 63);
  const int leader = __ffsll((long long)(m | mr)) - 1;
  const int sg = append_seg();
  unsigned long long base = 0, rbase = 0;
  if (lane == leader) {
    if (m) base = atomicAdd(&rb.count[sg], (unsigned long long)__popcll(m));
    if (mr) rbase = atomicAdd(&rs.count[sg], (unsigned long long)__popcll(mr));
  }
  base = __shfl(base, leader, 64);
  rbase = __shfl(rbase, leader, 64);
  const unsigned long long below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  if (e.reg) {
    const unsigned long long i = base + (unsigned long long)__popcll(m & below);
    if ((int64_t)i < rb.segcap) {
      const int64_t slot = (int64_t)sg * rb.segcap + (int64_t)i;
      rb.seq[slot] = sid;
      rb.beg[slot] = e.rbeg;
      rb.end[slot] = e.rend;
      rb.score[slot] = best;
    }
  }
  if (e.res) {
    const unsigned long long i = rbase + (unsigned long long)__popcll(mr & below);
    if ((int64_t)i < rs.segcap) {
      const int64_t slot = (int64_t)sg * rs.segcap + (int64_t)i;
      rs.a[slot] = e.res_a;
      rs.b[slot] = e.res_b;
      rs.seq[slot] = sid;
    }
  }
}

// Stitch as a segmented scan, one wave per run.  Chunk c acts on the open
// excursion state by one of: RESET(tail or none) -- an excursion closes in the
// chunk and/or its clean tail opens a new one -- or EXTEND(head) -- the carried
// excursion takes the chunk's head maximum (first argmax: a later head wins
// only when strictly greater).  The operator is associative, so 64 chunks are
// combined per step with shuffles; the chunk that closes an excursion emits it.
struct XState {
  int reset;  // 1: RESET to (open, xb, xm, xa); 0: EXTEND by (xm, xa)
  int open;
  long long xb, xa;
  double xm;
};

__device__ __forceinline__ XState x_compose(const XState &f1, const XState &f2) {  // f1 then f2
  if (f2.reset) return f2;
  XState r = f1;
  if (f2.xm > f1.xm) { r.xm = f2.xm; r.xa = f2.xa; }
  return r;
}

__device__ __forceinline__ XState x_shfl(const XState &a, int l) {
  XState r;
  r.reset = __shfl(a.reset, l, 64);
  r.open = __shfl(a.open, l, 64);
  r.xb = __shfl(a.xb, l, 64);
  r.xa = __shfl(a.xa, l, 64);
  r.xm = __shfl(a.xm, l, 64);
  return r;
}

// First scan index at which a candidate or tail of the chunk is valid: after
// the carried head's clamp, or nowhere when the carried excursion spans it.
__device__ __forceinline__ int64_t valid_from(int mode, int hq, int64_t st, int64_t en) {
  if (mode == kModeClean) return st;
  return hq >= 0 ? st + hq + 1 : en;
}

// The operator of chunk c on the open-excursion state, plus what the chunk
// needs to emit a closing excursion.
struct ChunkOp {
  XState f;
  bool closes;
  int64_t close_pos;
  double hmax;
  int64_t harg;
  int mode;
};

__device__ __forceinline__ ChunkOp chunk_op(const Chunks &g, const P1 &o, const Carry &cr, int64_t c) {
  ChunkOp r;
  r.f = XState{0, 0, 0, 0, -INFINITY};  // identity
  r.closes = false;
  r.close_pos = 0;
  r.hmax = -INFINITY;
  r.harg = 0;
  const int64_t st = g.start[c];
  const int64_t en = st + g.n[c];
  const int mode = cr.mode[c];
  const int hq = cr.hq[c];
  const int tb = o.tbeg[c];
  r.mode = mode;
  const int64_t vf = valid_from(mode, hq, st, en);
  if (mode != kModeClean && hq != 0) { r.hmax = cr.hmax[c]; r.harg = st + cr.harg[c]; }
  r.closes = mode != kModeClean && hq >= 0;
  r.close_pos = st + hq;
  const bool opens = tb >= 0 && st + tb >= vf && !(mode != kModeClean && hq < 0);
  if (opens) {
    r.f = XState{1, 1, st + tb, st + o.targ[c], o.tmax[c]};
  } else if (r.closes) {
    r.f = XState{1, 0, 0, 0, -1.0};
  } else if (mode != kModeClean) {
    r.f = XState{0, 0, 0, r.harg, r.hmax};
  }
  return r;
}

// DPP move of a state; lanes without a source read the identity (EXTEND by
// nothing: xm = -inf)
template <int CTRL, int RM>
__device__ __forceinline__ XState dpp_x(const XState &a) {
  return XState{dpp_i32<CTRL, RM>(a.reset), dpp_i32<CTRL, RM>(a.open), dpp_i64<CTRL, RM>(a.xb),
                dpp_i64<CTRL, RM>(a.xa), dpp_f64_or<CTRL, RM>(a.xm, -INFINITY)};
}

__device__ __forceinline__ XState wave_inclusive(XState inc, int lane) {
  KS_DPP_SCAN(XState, inc, dpp_x, x_compose);
  (void)lane;
  return inc;
}

// Tile t (64 chunks of one run, aligned to the run's first chunk) -> run id
// and first chunk.

// Stitch as a three-phase segmented scan (tile aggregates in parallel, a
// short per-run scan of the aggregates, then every tile again with its
// carry-in).  Chunk c acts on the open excursion state by one of:
// RESET(tail or none) -- an excursion closes in the chunk and/or its clean
// tail opens a new one -- or EXTEND(head) -- the carried excursion takes the
// chunk's head maximum (first argmax: a later head wins only when strictly
// greater).  The operator is associative; the chunk that closes an excursion
// emits it.
struct XTiles {
  int32_t *reset, *open;
  long long *xb, *xa;
  double *xm;
};

__device__ __forceinline__ void xt_store(const XTiles &a, int64_t t, const XState &v) {
  a.reset[t] = v.reset; a.open[t] = v.open; a.xb[t] = v.xb; a.xa[t] = v.xa; a.xm[t] = v.xm;
}
__device__ __forceinline__ XState xt_load(const XTiles &a, int64_t t) {
  return XState{a.reset[t], a.open[t], a.xb[t], a.xa[t], a.xm[t]};
}

__global__ void __launch_bounds__(256) k_stitch_tiles(Chunks g, const int64_t *__restrict__ tbase,
                                                     const int64_t *__restrict__ cbase, int64_t nruns, const int32_t *__restrict__ trun, P1 o,
                                                     Carry cr, XTiles agg, int64_t t_lo, int64_t t_hi) {
  const int64_t t = t_lo + (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);  // wave per tile
  if (t >= t_hi) return;
  const int lane = threadIdx.x & 63;
  int64_t r, c0, c1;
  tile_of(tbase, cbase, trun, t, r, c0, c1, nruns);
  const int64_t c = c0 + lane;
  XState f{0, 0, 0, 0, -INFINITY};
  if (c < c1) f = chunk_op(g, o, cr, c).f;
  const XState inc = wave_inclusive(f, lane);
  if (lane == 63) xt_store(agg, t, inc);
}

// Per run: exclusive scan of its tile aggregates (64 tiles per step) -> the
// state entering each tile; the excursion still open at the run end is
// emitted here.
__global__ void __launch_bounds__(64) k_stitch_runs(const int64_t *__restrict__ tbase, int64_t nruns,
                                                    const int64_t *__restrict__ ra, const int64_t *__restrict__ rb_end,
                                                    const int32_t *__restrict__ rseq, EmitCfg ec, XTiles agg,
                                                    XTiles tin, RegionBuf out, Rescan rs, int64_t r_lo) {
  const int64_t r = r_lo + blockIdx.x;  // runs [r_lo, nruns)
  if (r >= nruns) return;
  const int lane = threadIdx.x;
  const int64_t t0 = tbase[r], t1 = tbase[r + 1];
  if (t0 == t1) return;
  XState carry{1, 0, 0, 0, -1.0};  // closed
  for (int64_t tb = t0; tb < t1; tb += 64) {
    const int64_t t = tb + lane;
    XState f{0, 0, 0, 0, -INFINITY};
    if (t < t1) f = xt_load(agg, t);
    const XState inc = wave_inclusive(f, lane);
    const XState exc = dpp_x<kDppWaveShr1, 0xf>(inc);  // (lane 0: the identity)
    if (t < t1) xt_store(tin, t, x_compose(carry, exc));
    carry = x_compose(carry, x_shfl(inc, 63));
  }
  if (lane == 0 && carry.open) {  // excursion open at the run end
    const int64_t last = rb_end[r] - 1 + ec.trlr;  // last scan index of the run
    emit(decide(ec, ra[r] + ec.k, carry.xb, carry.xa, carry.xm, last, false), out, rs, rseq[r], carry.xm);
  }
}

__global__ void __launch_bounds__(256) k_stitch_emit(Chunks g, const int64_t *__restrict__ tbase,
                                                    const int64_t *__restrict__ cbase, int64_t nruns, const int32_t *__restrict__ trun,
                                                    const int64_t *__restrict__ ra, const int32_t *__restrict__ rseq,
                                                    P1 o, Carry cr, EmitCfg ec, XTiles tin, RegionBuf out,
                                                    Rescan rs, unsigned int *__restrict__ err, int64_t t_lo,
                                                    int64_t t_hi) {
  const int64_t t = t_lo + (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);  // wave per tile
  if (t >= t_hi) return;
  const int lane = threadIdx.x & 63;
  int64_t r, c0, c1;
  tile_of(tbase, cbase, trun, t, r, c0, c1, nruns);
  const int64_t c = c0 + lane;
  const bool live = c < c1;
  ChunkOp op;
  op.f = XState{0, 0, 0, 0, -INFINITY};
  op.closes = false;
  if (live) {
    op = chunk_op(g, o, cr, c);
    if (o.ep[c] != o.epoch) atomicOr(err, 32u);  // pass-1 results of another call
  }
  const XState inc = wave_inclusive(op.f, lane);
  const XState exc = dpp_x<kDppWaveShr1, 0xf>(inc);  // (lane 0: the identity)
  const XState in = x_compose(xt_load(tin, t), exc);  // state entering chunk c
  double xm = in.xm;
  long long xa = in.xa;
  Emission e{false, false, 0, 0, 0, 0};
  if (live && op.closes) {
    if (!in.open) {
      atomicOr(err, 4u);
    } else {
      if (op.hmax > xm) { xm = op.hmax; xa = op.harg; }
      e = decide(ec, ra[r] + ec.k, in.xb, xa, xm, op.close_pos, true);
    }
  }
  emit_wave(e, out, rs, rseq[r], xm);
  if (live && !op.closes && op.f.reset == 0 && op.mode != kModeClean && !in.open) atomicOr(err, 8u);
}

// Candidates (closed emittable excursions of the clean trajectories) are
// valid when they begin at or after their chunk's valid_from.
__global__ void k_candidates(Chunks g, const int64_t *__restrict__ ra, const int64_t *__restrict__ cbase,
                             int64_t nruns, const int32_t *__restrict__ rseq, EmitCfg ec, Cand cand,
                             Carry cr, RegionBuf out, Rescan rs) {
  const int k = ec.k;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool want = false;
  int64_t b = 0, arg = 0, rst = 0, f = 0;
  double best = 0.0;
  int32_t sid = 0;
  if (i < cand.cap && (i % cand.segcap) < (int64_t)cand.count[i / cand.segcap]) {
    b = cand.beg[i];
    int64_t lo = 0, hi = nruns - 1;  // last run with ra <= b
    while (lo < hi) {
      const int64_t mid = (lo + hi + 1) >> 1;
      if (ra[mid] <= b) lo = mid; else hi = mid - 1;
    }
    const int64_t c = cbase[lo] + (b - (ra[lo] + k)) / CH;
    const int64_t st = g.start[c];
    want = b >= valid_from(cr.mode[c], cr.hq[c], st, st + g.n[c]);
    sid = rseq[lo];
    arg = cand.arg[i];
    best = cand.best[i];
    rst = cand.rst[i];
    f = ra[lo] + k;
  }
  Emission e{false, false, 0, 0, 0, 0};
  if (want) e = decide(ec, f, b, arg, best, rst, true);
  emit_wave(e, out, rs, sid, best);
}

// KS_TEST_ENTRY_HINT (tests): the entry hint of a call that reuses one,
// overwritten before its pass 1.  what 0: zero, 1: 1e14, 2: NaN, 3: chunk c
// gets chunk c + 1's value from src, a copy of the hint taken beforehand.
__global__ void __launch_bounds__(256) k_test_hint(double *__restrict__ xh, const double *__restrict__ src,
                                                   int64_t nch, int what) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nch) return;
  double v = 0.0;
  if (what == 1) v = 1.0e14;
  if (what == 2) v = __longlong_as_double(0x7ff8000000000000LL);
  if (what == 3) v = src[c + 1 < nch ? c + 1 : c];
  xh[c] = v;
}

}  // namespace

// ------------------------------------------------------------ host driver
//
// scan_chunked reads top to bottom: kept slot (carve_keep: what the previous
// scan left) -> plan (plan_scan: which path the call takes, and what it takes
// from the kept slot) -> workspace (carve) -> layout kernels -> predictor
// (either only without it) -> pass 1 -> post-processing and rescans per half
// -> counter read-back -> retry decisions.  The helpers before it launch; none
// of them decides a path.
namespace {

// Slots of ks_ctx::ev this file records (chunked_phase_times reads the phase marks).
enum : int {
  kEvBegin = 7,         // phase mark: layout kernels begin
  kEvP1Begin = 8,       // phase mark: layout and predictor issued, pass 1 begins
  kEvP1End = 9,         // phase mark: end of pass 1 (the later of the halves)
  kEvCandEnd = 10,      // phase mark: the last half's candidates emitted
  kEvEnd = 11,          // phase mark: rescans issued
  kEvP1Half0 = 12,      // two parts: half 0's pass 1 done (hi); one part: the tail launch's fork (main)
  kEvSideDone = 13,     // side stream's work done: one part the tail launch, two parts half 1's post-processing
  kEvP2End = 14,        // phase mark: the last half's prediction and summaries
  kEvP34End = 15,       // phase mark: the last half's carry and heads
  kEvPredictFork = 16,  // side forked off main for half 1's predictor
  kEvP1Fork = 17,       // hi (and side, unless forked already) forked off main for pass 1
  kEvP1Side = 18,       // side stream's pass 1 done
};

// One kernel launch, checked.
template <class... KA, class... A>
ks_status launch(void (*kern)(KA...), dim3 grid, dim3 block, size_t lds, hipStream_t strm, const A &...a) {
  hipLaunchKernelGGL(kern, grid, block, lds, strm, a...);
  KS_HIP(hipGetLastError());
  return KS_OK;
}

// Run-time value -> template argument: f(std::integral_constant<int, v>) for
// v in [Lo, Hi], every other value as Def; f(std::true_type / false_type).
template <int Lo, int Hi, int Def, class F>
ks_status pick_int(int v, F &&f) {
  if constexpr (Lo > Hi) {
    return f(std::integral_constant<int, Def>{});
  } else {
    if (v == Lo) return f(std::integral_constant<int, Lo>{});
    return pick_int<Lo + 1, Hi, Def>(v, f);
  }
}
template <class F>
ks_status pick_bool(bool v, F &&f) {
  return v ? f(std::true_type{}) : f(std::false_type{});
}

// A part of the runs: chunks [c0, c1), runs [r0, r1), stitch tiles [t0, t1).
struct Half {
  int64_t c0, c1, r0, r1, t0, t1;
};

enum class P1Family {
  Lds,           // small k: the whole table in LDS, persistent blocks, no code store (k_pass1_lds / _int)
  Line,          // line tables: every chunk, a lane's bases from guarded loads (k_pass1l / k_pass1w / k_pass1r<3>)
  F64Expanded,   // FP64 expanded table, weighted rank (k_pass1pf + tail launch, or k_pass1r<1|2> alone)
  CompExpanded,  // expanded table on the pipelined pass (k_pass1p + tail launch)
  Plain,         // unexpanded table (k_pass1<1, ...>; a compressed one with the code store)
};

// Everything a call's path depends on, decided once (plan_scan).
struct ScanPlan {
  P1Family family;
  bool comp;       // compressed table
  bool lds_table;  // k <= kLdsTableK on packed bases (KS_NO_LDS_TABLE: off)
  // Integer tables: the exact carry (k_carry_exact) needs no predictor and no
  // summaries (KS_NO_EXACT: the general path, for A/B runs and tests).  Only
  // on the table forms of the pipelined passes -- LDS, line, expanded; an
  // unexpanded table of another size takes the code-store pass and
  // k_summaries.  Exact while every partial sum of a run is: |s| <= 2^20 over
  // fewer than 2^32 indices stays below 2^52.  KS_TEST_SEG_FALLBACK, which
  // forces the general carry's per-run fallback, takes the general path.
  bool exact;
  // Pass 1 writes the binade summaries itself (no per-position code store):
  // small k from the LDS-staged table (k_summaries after the prescan took 13.3
  // vs 8.8 ms at k = 7 log2); compressed expanded and line tables; FP64 tables
  // only with KS_F64_P1SUMM=1 (lines, expanded J 2..4).  Needs packed bases
  // and the binade predictor (a table without one is scanned unexpanded).
  bool p1summ;
  // No chunk summaries at all: KS_NO_SUMMARIES, and FP64 tables unless
  // KS_F64_P1SUMM is set (=0: k_summaries).  A summary serves a chunk only
  // while its carry-in stays >= 64 in one binade; weighted rank values in
  // [-0.5, 0.5] keep the carry far below that: 5,598 of 11.96 M chunks at
  // config 3 were summary-served, 1.0 M replayed.  At k = 15 50.6 vs 53.7 ms
  // with k_pass1pf's pass-1 summaries and 59.4 with k_summaries, at k = 13
  // 29.8 vs 30.2 with k_summaries (profiles/r5/ab/ab_nosumm_*.txt).
  bool no_summ;
  bool lds_lut;     // compressed: the LUT fits the LDS copy of the streaming passes
  bool need_codes;  // per-index code store (uint16 per scan index): written by the compressed
                    // unexpanded pass 1 for k_summaries
  int J;            // expansion of the table as pass 1 and the heads read it (compressed tables are
                    // scanned expanded only on the summarising or exact pass)
  int force_fb;     // KS_TEST_SEG_FALLBACK (tests): force the carry's per-run fallback
  bool epoch_stale; // KS_TEST_EPOCH_STALE (tests): the post-processing expects another epoch than pass
                    // 1 stamped -- what it would see reading an earlier call's pass-1 results -- so
                    // the epoch guard must fail the call
  bool rank_alone;  // F64Expanded: the weighted-rank code lines in one launch (k = 14 / 15: J = 4 / 3
                    // per 128-B line read against 3 / 2 per FP64 expanded entry); every chunk
  bool tail;        // the family launches the last chunks apart: k_pass1p / k_pass1pf leave the chunks
                    // whose reads could pass the end of the buffer (chunk starts increase with the
                    // chunk index, so they are among the last kP1TailMargin + CH chunks) to k_pass1
  int64_t ctail;    // first chunk of the tail launch
  // Two halves of the runs (pass-1-summary path): the second half's pass 1
  // (side stream) runs while the first half's latency-bound later passes
  // (carry, stitch) run on the main stream; halves split at a run boundary, so
  // no carry or stitch crosses it.  One part where it measured no slower:
  //  - without pass-1 summaries.  FP64 line tables (weighted rank): the two
  //    pass-1 launches ran side by side and ended together (15.2 ms each,
  //    profiles/r5/rank/step_timeline_rank_k13_twopart.txt), so the first
  //    part's post-processing never ran under the second's pass 1: 27.75 vs
  //    28.56 ms in one part (profiles/r5/ab/ab_nosplit_k13.txt).  FP64 expanded
  //    tables: two parts 52.1 vs 51.6 ms at k = 15, 46.0 vs 44.8 at k = 14
  //    (profiles/r5/ab/ab_nosumm_split_k15.txt, ab_nosumm_k14.txt).  The exact
  //    carry's post-processing is short: two parts measured the same at lower
  //    run-to-run spread, 6.44 vs 6.55 ms median at k = 7
  //    (profiles/r4/ab3/ab_k7pm1_exact_split.txt).
  //  - below ~2 M chunks, ~500 Mbp: at the 8-way shard, 1.5 M chunks, 2.38 vs
  //    2.42 ms in-process; 4-way, 3 M chunks, two parts 4.24 vs 4.37
  //    (profiles/r5/ab/ab_one_part_*.txt).  KS_SPLIT_MIN_CHUNKS: the threshold
  //    -- tests set 0 to run the two-part path on small genomes.
  bool split;
  int nhalf;
  Half half[2];
  bool debug_carry, debug_verify;  // KS_DEBUG_CARRY, KS_DEBUG_VERIFY (diagnostics; read once per process)
  // What the call takes from the kept slot (kept: the previous chunked scan on
  // the context was of the same sequence index, k, scan kind and layout, and
  // the slot's buffer is still the one it wrote):
  //  chunk_reuse: the chunk table and tile map (KS_NO_CHUNK_REUSE: off);
  //  hint_reuse: with the same table(s), that scan's P2 prediction as the
  //    entry hint, no predictor (KS_NO_ENTRY_HINT: off, and entry_reuse too);
  //  entry_reuse: its exact entries (ChunkKeep::entry_ok).  Pass 1 starts from
  //    them, writes the Carry fields and verifies every entry, and P2-P4 are
  //    not run at all (KS_NO_EXACT_ENTRY: off, for A/B runs and tests).  On
  //    the compressed line families' kernels (k_pass1w, k_pass1l); not with
  //    the diagnostics that read P2-P4 results, nor with the forced fallback.
  bool chunk_reuse, hint_reuse, entry_reuse;
  // The kept codes (SLOT_CODE_KEEP; plan_codes, once the slot is there): a
  // sub-mode of entry_reuse.  codes_J: the steps the form's line pass walks, 0:
  // the form keeps no codes.  codes_write: the exact flavour of the line pass
  // stores them (the first entry_reuse call that finds none: scan #2 of a genome
  // / table pair); codes_read: k_pass1c streams them instead of reading lines.
  int codes_J;
  bool codes_write, codes_read;
};

// The OWN template argument of the compressed line passes for a table's
// line_own (own 1..4 of the wide lines, 2..5 of the uint16 lines): the one
// place pass1_half's dispatch and kept_codes_J take it from.
template <class F>
ks_status pick_wide_own(int own, F &&f) {
  return pick_int<1, 3, 4>(own, f);
}
template <class F>
ks_status pick_u16_own(int own, F &&f) {
  return pick_int<3, 5, 2>(own, f);
}

// The steps of the line pass whose codes an indexed scan of this plan keeps,
// 0: none (FP64 and rank tables, a LUT past the LDS copy, plain calls;
// KS_NO_KEPT_CODES: off, for A/B runs and tests).
int kept_codes_J(const ScanPlan &p, const TableView &tv, const ScanMode &mode) {
  if (!mode.index || !p.p1summ || p.family != P1Family::Line || !p.comp || tv.nlut > kLineLutMax ||
      getenv("KS_NO_KEPT_CODES") != nullptr)
    return 0;
  int J = 0;  // (k_pass1w: J = OWN + 3, k_pass1l on uint16 lines: J = OWN + 2)
  if (tv.line_kind == 3)
    (void)pick_wide_own(tv.line_own, [&](auto o) { J = decltype(o)::value + 3; return KS_OK; });
  else
    (void)pick_u16_own(tv.line_own, [&](auto o) { J = decltype(o)::value + 2; return KS_OK; });
  return J;
}

// What the call does with the kept codes kc (null: the slot could not be had).
void plan_codes(ScanPlan &p, const ChunkKeep &prev, const uint32_t *kc) {
  // (the records lie by the kept chunk table's chunk index: not with KS_NO_CHUNK_REUSE)
  const bool have = p.entry_reuse && p.chunk_reuse && kc != nullptr && p.codes_J != 0;
  p.codes_read = have && prev.codes_ok && prev.codes_base == kc && prev.codes_J == p.codes_J;
  p.codes_write = have && !p.codes_read;
}

// The plan of one call.  Reads every KS_* switch of this file (per call: tests
// set them in-process between calls); makes no HIP call.  prev, kept: the kept
// slot's tag and whether it matches this call (scan_chunked).
ScanPlan plan_scan(const TableView &tv, int k, const ScanMode &mode, const Runs &runs, const RunLayout &lay,
                   const ChunkKeep &prev, bool kept) {
  static const bool debug_carry = getenv("KS_DEBUG_CARRY") != nullptr;
  static const bool debug_verify = getenv("KS_DEBUG_VERIFY") != nullptr;
  const char *f64e = getenv("KS_F64_P1SUMM");
  const char *smin = getenv("KS_SPLIT_MIN_CHUNKS");
  const int64_t split_min = smin ? atoll(smin) : ((int64_t)2 << 20);
  const bool packed = runs.packed != nullptr;
  const int Jt = tv.ext != nullptr ? tv.ext_J : 1;
  const int64_t nch = lay.nch;

  ScanPlan p{};
  p.debug_carry = debug_carry;
  p.debug_verify = debug_verify;
  p.comp = tv.compressed != 0;
  p.lds_table = k <= kLdsTableK && packed && getenv("KS_NO_LDS_TABLE") == nullptr;
  const bool line = tv.line != nullptr && !p.lds_table && packed;
  const bool f64_summ = !p.comp && !p.lds_table && f64e && atoi(f64e) != 0 && (line || (Jt >= 2 && Jt <= 4));
  p.force_fb = getenv("KS_TEST_SEG_FALLBACK") != nullptr ? 1 : 0;
  p.epoch_stale = getenv("KS_TEST_EPOCH_STALE") != nullptr;
  p.exact = tv.exact && !mode.trlr && packed && (p.lds_table || line || Jt >= 2) &&
            lay.longest < ((int64_t)1 << 32) && !p.force_fb && getenv("KS_NO_EXACT") == nullptr;
  p.no_summ = getenv("KS_NO_SUMMARIES") != nullptr || (!p.comp && !p.lds_table && !f64e);
  p.p1summ = !p.exact && (p.lds_table || (p.comp ? (Jt >= 2 || line) : f64_summ)) && packed && tv.approx != nullptr;
  p.need_codes = p.comp && !p.p1summ && !p.exact && !p.lds_table;
  p.lds_lut = p.comp && tv.nlut <= kLdsLutMax;
  p.J = (tv.ext != nullptr && (p.p1summ || p.exact || !p.comp)) ? tv.ext_J : 1;

  p.ctail = nch > 1024 ? nch - 1024 : 0;
  p.split = p.p1summ && nch > split_min && lay.split_r > 0 && lay.split_r < runs.n && lay.split_c >= 1024 &&
            lay.split_c + 1024 <= p.ctail;
  p.nhalf = p.split ? 2 : 1;
  p.half[0] = Half{0, nch, 0, runs.n, 0, lay.ntiles};
  if (p.split) {
    p.half[0] = Half{0, lay.split_c, 0, lay.split_r, 0, lay.split_t};
    p.half[1] = Half{lay.split_c, nch, lay.split_r, runs.n, lay.split_t, lay.ntiles};
  }

  if (p.lds_table)
    p.family = P1Family::Lds;
  else if (line && (p.p1summ || p.exact || !p.comp))
    p.family = P1Family::Line;
  else if (!p.comp && p.J >= 2 && p.J <= 4 && packed)
    p.family = P1Family::F64Expanded;
  else if (p.p1summ || p.exact)
    p.family = P1Family::CompExpanded;
  else
    p.family = P1Family::Plain;
  p.rank_alone = p.family == P1Family::F64Expanded && tv.rline && !mode.trlr && !p.p1summ && !p.split &&
                 (k == 14 || k == 15);
  p.tail = (p.family == P1Family::F64Expanded && !p.rank_alone) || p.family == P1Family::CompExpanded;

  p.chunk_reuse = kept && getenv("KS_NO_CHUNK_REUSE") == nullptr;
  p.hint_reuse = kept && p.p1summ && prev.hint >= 0 && prev.table_id == mode.table_id &&
                 prev.init_id == mode.init_id && getenv("KS_NO_ENTRY_HINT") == nullptr;
  p.entry_reuse = p.hint_reuse && prev.entry_ok && p.family == P1Family::Line && p.comp && !p.force_fb &&
                  !p.debug_carry && !p.debug_verify && getenv("KS_NO_EXACT_ENTRY") == nullptr;
  return p;
}

// Bump carver over one allocation: take<T>(n) hands out n elements of T on a
// 256-byte boundary.  Without a base it only sizes (and returns null).
struct Carver {
  char *base;
  size_t off = 0;
  template <class T>
  T *take(size_t n) {
    T *p = base ? reinterpret_cast<T *>(base + off) : nullptr;
    off += (n * sizeof(T) + 255) & ~(size_t)255;
    return p;
  }
};

// SLOT_CHUNK_KEEP carved (carve_keep): what a later scan of the same
// sequence index may take as it is (ChunkKeep, ks_internal.h).  No kernel
// writes start / n / run / trun after P0 (k_make_chunks, k_tile_runs), and
// none writes a hint array after the scan that filled it (P0's or P2's ascan).
struct Keep {
  int64_t *start;
  int32_t *n, *run;
  int32_t *trun;  // stitch tile -> run (k_tile_runs)
  // the two hint arrays: one is the call's Work::xh (read by pass 1), the
  // other its Work::xt (written by P2); a call that takes xh from the previous
  // call's xt writes the other array, so the roles swap from call to call and
  // P2 of the first part never overwrites what the second part's pass 1 reads
  double *hint[2];
  // every chunk's exact entry: Work::cr.x of a scan with a sequence index, so
  // the general path's carry (carry_segment, k_tile_apply, k_carry_exact: each
  // writes cr.x of every live chunk it covers) leaves them here with no copy;
  // a pass 1 from exact entries (ScanPlan::entry_reuse) reads and verifies
  // them and writes none
  double *entry;
};

Keep carve_keep(char *base, int64_t nch, int64_t ntiles, size_t *bytes) {
  Carver cv{base};
  Keep kp{};
  kp.start = cv.take<int64_t>(nch);
  kp.n = cv.take<int32_t>(nch);
  kp.run = cv.take<int32_t>(nch);
  kp.trun = cv.take<int32_t>(ntiles + 1);
  kp.hint[0] = cv.take<double>(nch);
  kp.hint[1] = cv.take<double>(nch);
  kp.entry = cv.take<double>(nch);
  *bytes = cv.off;
  return kp;
}

// The call's buffers: SLOT_CHUNK_A carved (carve), the kept slot's arrays,
// the code store, the candidate and rescan lists of each half, the
// diagnostics' counters.
struct Work {
  Chunks g;
  P1 p1;
  double *xt;  // predicted entries (P2 prescan): one of Keep::hint
  Summ sm;
  Carry cr;
  // cnts: [0, kSegs) candidate counters, [kSegs, 2 kSegs) rescan counters,
  // [2 kSegs + 2h] replays, [2 kSegs + 2h + 1] error bits (u32) of half h,
  // [2 kSegs + 4] the copy of the sequence index guard's flag,
  // [2 kSegs + 8, 3 kSegs + 8) the region counters' copy, [3 kSegs + 8,
  // 5 kSegs + 8) the second half's candidate and rescan counters
  unsigned long long *cnts;
  uint8_t *flag;
  XTiles xagg, xtin;
  // pass-1 summaries: predictor sums / exits / zero flags, predicted entries,
  // the summaries, the fix list (nfix[2]: one counter per half)
  double *pa, *pb;
  uint8_t *pz;
  double *xh;  // the other of Keep::hint: P0's prediction, or the previous call's xt
  SummP1 sp1;
  unsigned long long *nfix;
  int64_t *fix;
  double2 *tagg;  // parallel approximate scan: tile maps, tile entries
  double *tin;
  int32_t *trun;  // stitch tile -> run (k_tile_runs)
  TileComp tcomp;
  ReplayBuf rpb;  // likely-replay prefetch (k_marks_select lists, k_summ_fixw fills)
  uint16_t *codes = nullptr;  // ScanPlan::need_codes
  uint32_t *kc = nullptr;     // the kept codes (SLOT_CODE_KEEP), null: none
  // Candidates and rescans in one list per half: the first half's are
  // emitted and rescanned while the second half is post-processed (a list
  // cannot be read while the other half's pass 1 still appends to it).
  Cand cands[2];
  Rescan rss[2];
  long long *dbg = nullptr;  // KS_DEBUG_CARRY: 9 counters per 64-chunk window + 4
  int64_t nwin = 0;
};

// SLOT_CHUNK_A's layout.  base null: the size alone.  xt and xh are the
// caller's choice among kp.hint.
Work carve(char *base, const ScanPlan &plan, int64_t nch, int64_t ntiles, const uint32_t *packed, const Keep &kp,
           size_t *bytes) {
  Carver cv{base};
  double *p1d = cv.take<double>(nch * 6);
  int32_t *p1i = cv.take<int32_t>(nch * 3);
  uint8_t *spec = cv.take<uint8_t>(nch);
  uint32_t *ep = cv.take<uint32_t>(nch);
  int32_t *se = cv.take<int32_t>(nch);
  long long *sD = cv.take<long long>(nch * 6);
  int32_t *sA = cv.take<int32_t>(nch * 2);
  double *x = cv.take<double>(nch);
  uint8_t *cmode = cv.take<uint8_t>(nch);
  int32_t *hq = cv.take<int32_t>(nch * 2);
  double *hmax = cv.take<double>(nch);
  unsigned long long *cnts = cv.take<unsigned long long>(5 * kSegs + 8);  // + the region counters' copy, half 1's lists
  uint8_t *flag = cv.take<uint8_t>(nch + 64);
  char *xa0 = cv.take<char>(ntiles * 32), *xa1 = cv.take<char>(ntiles * 32);
  double *pa = cv.take<double>(nch);
  double *pb = cv.take<double>(nch);
  uint8_t *pz = cv.take<uint8_t>(nch);
  int32_t *spe = cv.take<int32_t>(nch * 2);
  long long *spd = cv.take<long long>(nch * 6);
  int32_t *spa = cv.take<int32_t>(nch * 2);
  unsigned long long *nfix = cv.take<unsigned long long>(nch + 2);  // [2] counters, then the list
  uint8_t *ssel = cv.take<uint8_t>(nch);  // Summ::sel
  double2 *tagg = cv.take<double2>(ntiles);
  double *tin = cv.take<double>(ntiles);
  const int64_t ngt = nch / 64 + 2;  // global 64-chunk tiles (carry tile batches)
  int32_t *gte = cv.take<int32_t>(ngt);
  long long *gtd = cv.take<long long>(ngt * 6);
  long long *gtm = cv.take<long long>(ngt);
  int32_t *gtee = cv.take<int32_t>(ngt);
  const int64_t rcap_h = std::max<int64_t>(65536, nch / 128);  // replay slots per half
  int32_t *rslot = cv.take<int32_t>(nch);
  int64_t *rchunk = cv.take<int64_t>(2 * rcap_h);
  unsigned long long *rcnt = cv.take<unsigned long long>(8);
  double *rval = cv.take<double>(2 * rcap_h * 256);
  *bytes = cv.off;

  Work w{};
  if (!base) return w;
  w.g = Chunks{kp.start, kp.n, kp.run, nch, packed};
  w.p1 = P1{p1d, p1d + nch, p1d + 2 * nch, p1d + 3 * nch, p1d + 4 * nch, p1d + 5 * nch, p1i, p1i + nch, spec,
            p1i + 2 * nch};
  w.p1.ep = ep;
  w.sm = Summ{se, sD, sD + 2 * nch, sD + 4 * nch, sA};
  w.cr = Carry{x, cmode, hq, hmax, hq + nch};
  w.cnts = cnts;
  w.flag = flag;
  auto xtiles = [&](char *p) {
    return XTiles{reinterpret_cast<int32_t *>(p), reinterpret_cast<int32_t *>(p) + ntiles,
                  reinterpret_cast<long long *>(p + ntiles * 8), reinterpret_cast<long long *>(p + ntiles * 16),
                  reinterpret_cast<double *>(p + ntiles * 24)};
  };
  w.xagg = xtiles(xa0);
  w.xtin = xtiles(xa1);
  w.pa = pa;
  w.pb = pb;
  w.pz = pz;
  w.sp1 = SummP1{spe, spd, spd + 2 * nch, spd + 4 * nch, spa};
  w.nfix = nfix;
  w.fix = reinterpret_cast<int64_t *>(nfix + 2);
  w.tagg = tagg;
  w.tin = tin;
  w.trun = kp.trun;
  w.tcomp = TileComp{gte, gtd, gtd + 2 * ngt, gtd + 4 * ngt, gtm, gtee};
  // (the carry reads no replay slots unless k_marks_select wrote them)
  w.rpb = ReplayBuf{plan.p1summ ? rslot : nullptr, rchunk, rval, rcnt, rcap_h};
  // pass-1 summaries are read where pass 1 wrote them (summ_at): the selection
  // writes a byte per chunk instead of copying 56 (metric step 14.47 vs 14.61 ms
  // median in-process, profiles/r4/ab4/ab_copy_log2.txt)
  if (plan.p1summ) {
    w.sm.sel = ssel;
    w.sm.pD = w.sp1.D;
    w.sm.pM = w.sp1.M;
    w.sm.pN = w.sp1.N;
    w.sm.pA = w.sp1.A;
  }
  w.nwin = (nch + 63) / 64;
  return w;
}

// One call's inputs, as the launches take them.
struct ScanCall {
  ks_ctx *ctx;
  const ks_dev_seqs *s;
  int64_t total;
  int k;
  const TableView &tv;
  const EmitCfg ec;
  const Runs &runs;
  const RunLayout &lay;
  const RegionBuf &rb;
  uint32_t *visits, *visits_rescan;
  const ScanMode &mode;
};

Chunks view(const Chunks &g, const Half &h) {
  Chunks v = g;
  v.c0 = h.c0;
  v.nch = h.c1;
  return v;
}

// waves per block of the wave-per-tile / wave-per-window kernels (A/B: 2 of 1-4)
constexpr int kWpb = 2;

// Approximate max-plus scan of (sum, clean exit) over the runs of h: three
// parallel kernels (the one-wave-per-run k_approx_scan when h has no tile).
ks_status ascan(const ScanCall &c, const Work &w, const P1 &o, double *out, const Half &h, hipStream_t strm) {
  const int64_t nruns = c.runs.n;
  if (h.r1 <= h.r0) return KS_OK;
  const dim3 gr((unsigned)(h.r1 - h.r0));
  if (h.t1 <= h.t0) return launch(k_approx_scan, gr, dim3(64), 0, strm, c.lay.cbase, h.r1, o, out, h.r0);
  const dim3 g4((unsigned)((h.t1 - h.t0 + kWpb - 1) / kWpb)), b4(64 * kWpb);  // a wave per tile, kWpb per block
  KS_TRY(launch(k_ascan_tiles, g4, b4, 0, strm, c.lay.tbase, c.lay.cbase, nruns, w.trun, o, w.tagg, h.t0, h.t1));
  KS_TRY(launch(k_ascan_runs, gr, dim3(64), 0, strm, c.lay.tbase, h.r1, w.tagg, w.tin, h.r0));
  return launch(k_ascan_apply, g4, b4, 0, strm, c.lay.tbase, c.lay.cbase, nruns, w.trun, o, w.tin, out, h.t0, h.t1);
}

// P0: the predicted entries (Work::xh) of the chunks of h.
ks_status predict(const ScanCall &c, const Work &w, const Half &h, hipStream_t strm) {
  P1 pp = w.p1;
  pp.asum = w.pa;
  pp.cexit = w.pb;
  pp.special = w.pz;
  KS_HIP(hipMemsetAsync(w.pz + h.c0, 0, (size_t)(h.c1 - h.c0), strm));
  const size_t lds = (size_t)2 << (2 * c.tv.approx_k);  // the fp16 prefix table
  const int per_cu = lds <= ((size_t)32 << 10) ? 4 : 1;
  const unsigned gl = (unsigned)std::max<int64_t>(
      1, std::min<int64_t>((h.c1 - h.c0 + 1023) / 1024, (int64_t)c.ctx->num_cus * per_cu));
  // every fourth index sampled, weighted 4 (at four 32-KiB blocks per CU:
  // metric step 14.48 vs 14.62 ms median with every second, predictor 0.56 vs
  // 0.64 ms; every eighth: predictor 0.21 ms but more mispredicted binades,
  // carry + stitch 1.18 vs 0.85 ms; profiles/r4/ab4/ab_pred_log2.txt).
  KS_HIP(hipFuncSetAttribute((const void *)k_predict<4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  KS_TRY(launch(k_predict<4>, dim3(gl), dim3(1024), lds, strm, view(w.g, h), c.total, c.k, c.tv.approx,
                c.tv.approx_k, pp.asum, pp.cexit));
  return ascan(c, w, pp, w.xh, h, strm);
}

// Pass 1 of the chunks of h on strm, appending to cand (every family but Plain).
ks_status pass1_half(const ScanCall &c, const ScanPlan &plan, const Work &w, const Half &h, hipStream_t strm,
                     const Cand &cand) {
  const Chunks gv = view(w.g, h);
  const int64_t n = h.c1 - h.c0;
  const TableView &tv = c.tv;
  const EmitCfg &ec = c.ec;
  const P1 &p1 = w.p1;
  const SummP1 &sp1 = w.sp1;
  // (entry_reuse: the kept exact entries, Work::cr.x = Keep::entry, and the part's error bits)
  const double *xh = plan.entry_reuse ? w.cr.x : (plan.p1summ ? w.xh : nullptr);
  const Carry &cr = w.cr;
  unsigned int *err = reinterpret_cast<unsigned int *>(w.cnts + 2 * kSegs + 2 * (&h - plan.half) + 1);
  const bool trlr = ec.trlr != 0;
  auto blocks = [&](int64_t per) { return dim3((unsigned)((n + per - 1) / per)); };
  auto persistent = [&](int per_cu) {
    return dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 1023) / 1024, (int64_t)per_cu * c.ctx->num_cus)));
  };
  switch (plan.family) {
    case P1Family::Lds:
      if (trlr)
        return launch(k_pass1_lds<true>, persistent(1), dim3(1024), 0, strm, gv, c.total, c.k, tv, ec, c.visits, p1,
                      cand, xh, sp1);
      // integer small-k tables: the int32 pass, two blocks per CU (4.72 vs 5.57 ms
      // at k = 7, profiles/r4/ab3/ab_k7pm1_int.txt; KS_NO_EXACT: the FP64 pass)
      if (plan.exact)
        return launch(k_pass1_lds_int, persistent(2), dim3(1024), 0, strm, gv, c.total, c.k, tv, ec, c.visits, p1,
                      cand);
      return launch(k_pass1_lds<false>, persistent(1), dim3(1024), 0, strm, gv, c.total, c.k, tv, ec, c.visits, p1,
                    cand, xh, sp1);
    case P1Family::Line: {
      const int own = tv.line_own;
      if (plan.codes_read)  // the kept codes instead of the lines
        return pick_int<5, 7, 4>(plan.codes_J, [&](auto j) {
          return pick_bool(trlr, [&](auto t) {
            return pick_bool(c.visits != nullptr, [&](auto v) {
              constexpr int kBlock = code_block(decltype(v)::value);
              return launch(k_pass1c<decltype(j)::value, decltype(t)::value, decltype(v)::value>, blocks(kBlock),
                            dim3(kBlock), (size_t)tv.nlut * 8, strm, gv, c.total, c.k, tv, ec, c.visits, p1, cand,
                            xh, cr, err, w.kc);
            });
          });
        });
      if (tv.rline && !trlr && !plan.p1summ && own == 3)  // weighted-rank code lines (k = 13)
        return launch(k_pass1r<3>, blocks(kRankBlock), dim3(kRankBlock), 0, strm, gv, c.total, c.k, tv, ec, c.visits,
                      p1, cand);
      if (tv.line_kind == 3)  // wide lines: own 1..4 at k = 15..12 (J = 4..7)
        return pick_wide_own(own, [&](auto o) {
          return pick_bool(trlr, [&](auto t) {
            return pick_int<1, 2, 0>(plan.entry_reuse ? (plan.codes_write ? 2 : 1) : 0, [&](auto x) {
              return launch(k_pass1w<decltype(o)::value, decltype(t)::value, (decltype(x)::value > 0),
                                     (decltype(x)::value > 1)>,
                            blocks(kWideBlock), dim3(kWideBlock), 0, strm, gv, c.total, c.k, tv, ec, c.visits, p1, cand,
                            xh, sp1, cr, err, w.kc);
            });
          });
        });
      if (!plan.comp)
        return pick_int<3, 4, 2>(own, [&](auto o) {
          return pick_bool(trlr, [&](auto t) {
            return launch(k_pass1l<decltype(o)::value, true, false, decltype(t)::value>, blocks(1024), dim3(1024), 0,
                          strm, gv, c.total, c.k, tv, ec, c.visits, p1, cand, xh, sp1, cr, err, w.kc);
          });
        });
      return pick_u16_own(own, [&](auto o) {
        return pick_bool(tv.nlut <= kLineLutMax, [&](auto l) {
          return pick_bool(trlr, [&](auto t) {
            // (codes_write implies the LDS LUT, kept_codes_J)
            return pick_int<1, 2, 0>(plan.entry_reuse ? (plan.codes_write ? 2 : 1) : 0, [&](auto x) {
              return launch(k_pass1l<decltype(o)::value, false, decltype(l)::value, decltype(t)::value,
                                     (decltype(x)::value > 0), (decltype(x)::value > 1 && decltype(l)::value)>,
                            blocks(768), dim3(768), 0, strm, gv, c.total, c.k, tv, ec, c.visits, p1, cand, xh, sp1, cr,
                            err, w.kc);
            });
          });
        });
      });
    }
    case P1Family::F64Expanded:
      // 512-lane blocks: up to 256 VGPRs, 152 used, no spills, 3 waves per SIMD
      // (1024-lane blocks capped it at 128 with 17-29 VGPRs spilled to scratch:
      // weighted rank k = 15 in-process 55.3 vs 61.4 ms, profiles/r5/ab/ab_p1pf_block.txt)
      return pick_int<3, 4, 2>(plan.J, [&](auto j) {
        return pick_bool(trlr, [&](auto t) {
          return launch(k_pass1pf<decltype(j)::value, decltype(t)::value, 512>, blocks(512), dim3(512), 0, strm, gv,
                        c.s->seq, c.total, c.k, tv, ec, c.visits, p1, cand, c.runs.packed, xh, sp1);
        });
      });
    case P1Family::CompExpanded:
      return pick_int<3, 5, 2>(plan.J, [&](auto j) {
        return pick_bool(plan.lds_lut, [&](auto l) {
          return pick_bool(trlr, [&](auto t) {
            return launch(k_pass1p<decltype(j)::value, decltype(l)::value, decltype(t)::value>, blocks(kP1Block),
                          dim3(kP1Block), 0, strm, gv, c.s->seq, c.total, c.k, tv, ec, c.visits, p1, cand,
                          c.runs.packed, xh, sp1);
          });
        });
      });
    case P1Family::Plain:
      break;
  }
  return fail(KS_ERR_INTERNAL, "chunked scan: no pass-1 launch per half for this table form");
}

// The tail chunks [plan.ctail, nch) of the expanded families (a latency-bound
// serial walk each; no code store on these paths).
ks_status pass1_tail(const ScanCall &c, const ScanPlan &plan, const Work &w, hipStream_t strm, const Cand &cand) {
  const dim3 grid((unsigned)((w.g.nch - plan.ctail + 1023) / 1024));
  auto go = [&](auto j, auto comp, auto l) {
    return launch(k_pass1<decltype(j)::value, decltype(comp)::value, decltype(l)::value>, grid, dim3(1024), 0, strm,
                  w.g, c.s->seq, c.total, c.k, c.tv, nullptr, c.ec, c.visits, w.p1, cand, plan.ctail, 1);
  };
  if (plan.family == P1Family::F64Expanded)
    return pick_int<3, 4, 2>(plan.J, [&](auto j) { return go(j, std::false_type{}, std::false_type{}); });
  if (plan.J == 5) return go(std::integral_constant<int, 5>{}, std::true_type{}, std::false_type{});
  return pick_int<3, 4, 2>(plan.J, [&](auto j) {
    return pick_bool(plan.lds_lut, [&](auto l) { return go(j, std::true_type{}, l); });
  });
}

// P2-P5 (without the candidates) of half hi on stream strm, with its own
// replay counter, error bits and fix list; kEvP2End / kEvP34End mark the
// last half's phases.
ks_status post_half(const ScanCall &c, const ScanPlan &plan, const Work &w, int hi, hipStream_t strm) {
  const Half &h = plan.half[hi];
  const bool last = hi == plan.nhalf - 1;
  const Chunks gv = view(w.g, h);
  const Chunks &g = w.g;
  const TableView &tv = c.tv;
  const P1 &p1 = w.p1;
  const Summ &sm = w.sm;
  const Carry &cr = w.cr;
  const TileComp &tch = w.tcomp;
  const ReplayBuf &rpb = w.rpb;
  const uint8_t *seq = c.s->seq;
  const int64_t total = c.total, nruns = c.runs.n;
  const int k = c.k;
  const int64_t nh = h.c1 - h.c0, nr = h.r1 - h.r0, nt = h.t1 - h.t0;
  if (nh <= 0) return KS_OK;
  unsigned long long *rep_h = w.cnts + 2 * kSegs + 2 * hi;
  unsigned int *err_h = reinterpret_cast<unsigned int *>(rep_h + 1);
  const dim3 gch_h((unsigned)((nh + 255) / 256)), gsum_h((unsigned)((nh + 1023) / 1024));
  const dim3 bw(64 * kWpb);
  const dim3 gst((unsigned)((nt + kWpb - 1) / kWpb));
  // P5 stitch
  auto stitch = [&]() -> ks_status {
    if (nt > 0)
      KS_TRY(launch(k_stitch_tiles, gst, bw, 0, strm, g, c.lay.tbase, c.lay.cbase, nruns, w.trun, p1, cr, w.xagg, h.t0,
                    h.t1));
    if (nr > 0)
      KS_TRY(launch(k_stitch_runs, dim3((unsigned)nr), dim3(64), 0, strm, c.lay.tbase, h.r1, c.runs.a, c.runs.b,
                    c.runs.seq, c.ec, w.xagg, w.xtin, c.rb, w.rss[hi], h.r0));
    if (nt > 0)
      KS_TRY(launch(k_stitch_emit, gst, bw, 0, strm, g, c.lay.tbase, c.lay.cbase, nruns, w.trun, c.runs.a, c.runs.seq,
                    p1, cr, c.ec, w.xtin, c.rb, w.rss[hi], err_h, h.t0, h.t1));
    return KS_OK;
  };
  if (plan.entry_reuse) {
    // pass 1 started from the exact entries and wrote the Carry fields: no
    // P2-P4 (the phase marks stay, for chunked_phase_times)
    if (last) {
      KS_HIP(hipEventRecord(c.ctx->ev[kEvP2End], strm));
      KS_HIP(hipEventRecord(c.ctx->ev[kEvP34End], strm));
    }
    return stitch();
  }
  // ---- P2 prediction, segment starts, summaries
  KS_TRY(ascan(c, w, p1, w.xt, h, strm));
  const int64_t wl = (h.c0 > 0 ? h.c0 - 1 : 0) / 64;
  const int64_t nwm = (h.c1 + 63) / 64 - wl;
  if (plan.exact) {  // the prescan is the carry (k_carry_exact)
    KS_TRY(launch(k_carry_exact, gch_h, dim3(256), 0, strm, gv, p1, w.xt, cr));
  } else if (plan.p1summ) {
    // segment marks and summary selection in one pass over the chunks
    KS_HIP(hipMemsetAsync(w.nfix + hi, 0, 8, strm));
    KS_HIP(hipMemsetAsync(rpb.count + hi, 0, 8, strm));
    KS_TRY(launch(k_marks_select, dim3((unsigned)((nwm + 3) / 4)), dim3(256), 0, strm, gv, p1, w.xt, w.flag, nwm,
                  w.sp1, sm, w.fix + h.c0, w.nfix + hi, w.xh,
                  w.dbg ? reinterpret_cast<unsigned long long *>(w.dbg + w.nwin * 9) : nullptr, rpb, hi));
    // summaries of the listed chunks, a wave each; the LUT read through L2,
    // not staged in LDS: a 54 KB LDS copy per block (2048 blocks, most
    // without a listed chunk) cost more than the ~4 M lookups of the ~16 K
    // listed chunks
    const unsigned gw = (unsigned)std::max<int64_t>(1, (int64_t)c.ctx->num_cus * 8);
    KS_TRY(launch(k_summ_fixw<false>, dim3(gw), dim3(256), 0, strm, g, seq, total, k, tv, w.xt, w.fix + h.c0,
                  w.nfix + hi, sm, rpb, hi));
  } else {
    KS_TRY(launch(k_seg_marks, dim3((unsigned)((nwm + kWpb - 1) / kWpb)), bw, 0, strm, gv, p1, w.xt, w.flag, nwm));
    if (plan.no_summ) {
      KS_TRY(launch(k_summ_none, gsum_h, dim3(1024), 0, strm, gv, sm));
    } else if (plan.lds_table) {
      // small k: the table staged in LDS as for k_pass1_lds (from HBM / L2: 12.8 / 18.7 vs 3.8 / 6.4 ms)
      if (plan.comp && plan.lds_lut) {
        const size_t tb = (size_t)2 << (2 * k);
        KS_HIP(hipFuncSetAttribute((const void *)k_summaries<true, true, true>,
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)tb));
        KS_TRY(launch(k_summaries<true, true, true>, gsum_h, dim3(1024), tb, strm, gv, seq, total, k, tv, nullptr, p1,
                      w.xt, sm));
      } else {
        const size_t tb = (size_t)8 << (2 * k);
        KS_HIP(hipFuncSetAttribute((const void *)k_summaries<false, false, true>,
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)tb));
        KS_TRY(launch(k_summaries<false, false, true>, gsum_h, dim3(1024), tb, strm, gv, seq, total, k, tv, nullptr,
                      p1, w.xt, sm));
      }
    } else if (plan.lds_lut) {
      KS_TRY(launch(k_summaries<true, true>, gsum_h, dim3(1024), 0, strm, gv, seq, total, k, tv, w.codes, p1, w.xt,
                    sm));
    } else if (plan.comp) {
      KS_TRY(launch(k_summaries<true, false>, gsum_h, dim3(1024), 0, strm, gv, seq, total, k, tv, w.codes, p1, w.xt,
                    sm));
    } else {
      KS_TRY(launch(k_summaries<false, false>, gsum_h, dim3(1024), 0, strm, gv, seq, total, k, tv, w.codes, p1, w.xt,
                    sm));
    }
  }
  if (last) KS_HIP(hipEventRecord(c.ctx->ev[kEvP2End], strm));

  // ---- P3 carry by segments + P4 heads; then the gated per-run fallback
  const int64_t wc = h.c0 / 64;
  const unsigned nwc = (unsigned)((h.c1 - 1) / 64 - wc + 1);
  const dim3 gtc((unsigned)(((h.c1 - 1) / 64 - wc + 1 + 3) / 4));  // 4 tiles per block
  // FP64 tables: the R chunks' heads packed densely (k_heads_dense; lane per
  // chunk, k_heads, measured slower at config 3: 29.9 vs 29.2 ms,
  // profiles/r5/ab/ab_heads_dense_lane_pf_*.txt); compressed tables: k_heads
  auto heads = [&](int gated) -> ks_status {
    // (gated: a small grid-stride grid; it exits at once unless the carry fell back)
    const unsigned full = plan.comp ? gch_h.x : (unsigned)((nh + 4 * kHeadSpan - 1) / (4 * kHeadSpan));
    const dim3 gh(gated ? std::min<unsigned>(full, (unsigned)c.ctx->num_cus * 2) : full);
    if (plan.comp)
      return launch(k_heads<1, true>, gh, dim3(256), 0, strm, gv, seq, total, k, tv, w.codes, cr, err_h, gated);
    if (plan.J == 4 && tv.line)
      return launch(k_heads_dense<4, false, true>, gh, dim3(256), 0, strm, gv, seq, total, k, tv, w.codes, cr, err_h,
                    gated);
    return pick_int<2, 4, 1>(plan.J, [&](auto j) {
      return launch(k_heads_dense<decltype(j)::value, false, false>, gh, dim3(256), 0, strm, gv, seq, total, k, tv,
                    w.codes, cr, err_h, gated);
    });
  };
  if (plan.exact) {
    KS_TRY(heads(0));
  } else {
    const dim3 gcw((nwc + kWpb - 1) / kWpb);
    KS_TRY(launch(k_tile_comp, gtc, dim3(256), 0, strm, gv, sm, tch));
    KS_TRY(pick_bool(plan.comp, [&](auto cp) {
      return launch(k_carry_win<decltype(cp)::value>, gcw, bw, 0, strm, gv, w.flag, seq, total, k, tv, w.codes, p1, sm,
                    cr, tch, rpb, rep_h, err_h, w.dbg);
    }));
    KS_TRY(launch(k_tile_apply, gtc, dim3(256), 0, strm, gv, sm, tch, cr, err_h, 0));
    KS_TRY(heads(0));
    KS_TRY(launch(k_fallback_prep, dim3(1), dim3(1), 0, strm, err_h, rep_h, plan.force_fb));
    if (nr > 0) {
      KS_TRY(pick_bool(plan.comp, [&](auto cp) {
        return launch(k_carry_run<decltype(cp)::value>, dim3((unsigned)nr), dim3(64), 0, strm, gv, c.lay.cbase, h.r1,
                      seq, total, k, tv, w.codes, p1, sm, cr, tch, rpb, rep_h, err_h, nullptr, h.r0);
      }));
      KS_TRY(launch(k_tile_apply, gtc, dim3(256), 0, strm, gv, sm, tch, cr, err_h, 1));
    }
    KS_TRY(heads(1));
  }
  if (last) KS_HIP(hipEventRecord(c.ctx->ev[kEvP34End], strm));

  // ---- P5 stitch
  return stitch();
}

// Candidates (count read on the device) and rescans of half h's lists on rst
// (the rescan slots in list order: sorted longest first they took 5.23 vs
// 3.56 ms at config 3, profiles/r4/ab2/ab_rank.txt).
ks_status emit_rescan(const ScanCall &c, const ScanPlan &plan, const Work &w, int h, hipStream_t rst) {
  const Rescan &rs = w.rss[h];
  KS_TRY(launch(k_candidates, dim3((unsigned)((w.cands[h].cap + 255) / 256)), dim3(256), 0, rst, w.g, c.runs.a,
                c.lay.cbase, c.runs.n, c.runs.seq, c.ec, w.cands[h], w.cr, c.rb, rs));
  if (h == plan.nhalf - 1) KS_HIP(hipEventRecord(c.ctx->ev[kEvCandEnd], rst));
  return launch_scan_lane(c.ctx, c.s->seq, c.total, rs.a, rs.b, rs.seq, rs.cap, c.k, c.tv, c.ec.mw, c.ec.min_score,
                          c.visits_rescan, c.rb, rs.count, rs.segcap, c.mode, 0, nullptr, c.runs.packed, rst);
}

// Diagnostics (at the end of the file), called under their flags.
void debug_verify(const ScanCall &c, const Work &w);
ks_status debug_carry_report(const ScanPlan &plan, Work &w, int64_t nruns);
ks_status debug_rescan_hist(const Rescan &rs, const unsigned long long *counts, int k, int64_t nres);

}  // namespace

ks_status scan_chunked(ks_ctx *ctx, const ks_dev_seqs *s, const Runs &runs, const RunLayout &lay, int k,
                       const TableView &tv, uint64_t mw, double min_score, uint32_t *visits,
                       uint32_t *visits_rescan, const RegionBuf &rb, ks_scan_stats *stats, const ScanMode &mode) {
  hipStream_t st = ctx->stream, side = ctx->side, hi = ctx->hi;
  const int64_t nruns = runs.n, nch = lay.nch, ntiles = lay.ntiles;
  ctx->chunked_events = false;
  // The kept slot's tag (what the previous chunked scan on this context left
  // for this one) is taken and cleared here and set again where the call
  // returns KS_OK, so a failed call or a retry leaves none behind.
  const ChunkKeep prev = ctx->chunk_keep;
  chunk_keep_clear(ctx);
  if (nruns == 0 || nch == 0) return KS_OK;
  const EmitCfg ec{mode.trlr, mw, min_score, mode.min_len, mode.ks, k};
  const ScanCall c{ctx, s, s->offsets_host[s->nseq], k, tv, ec, runs, lay, rb, visits, visits_rescan, mode};
  auto record = [&](int e, hipStream_t strm) -> ks_status {
    KS_HIP(hipEventRecord(ctx->ev[e], strm));
    return KS_OK;
  };
  auto wait = [&](hipStream_t strm, int e) -> ks_status {
    KS_HIP(hipStreamWaitEvent(strm, ctx->ev[e], 0));
    return KS_OK;
  };

  // ---- the kept slot.  A matching tag implies a sequence index hit with the
  // cached layout: a build or a new layout clears it (find_runs, run_layout).
  size_t kbytes = 0;
  carve_keep(nullptr, nch, ntiles, &kbytes);
  void *ksp = nullptr;
  KS_TRY(ensure(ctx, SLOT_CHUNK_KEEP, kbytes, &ksp));
  const Keep kp = carve_keep(static_cast<char *>(ksp), nch, ntiles, &kbytes);
  const uint64_t ixid = mode.index ? mode.index->id : 0;
  const bool kept = ixid != 0 && prev.id == ixid && prev.k == k && prev.trlr == mode.trlr && prev.nch == nch &&
                    prev.ntiles == ntiles && prev.base == ksp;
  ScanPlan plan = plan_scan(tv, k, mode, runs, lay, prev, kept);
  const bool chunk_reuse = plan.chunk_reuse, hint_reuse = plan.hint_reuse, entry_reuse = plan.entry_reuse;
  // ---- the kept codes: a slot of their own, sized by every indexed scan whose
  // form keeps codes (so a fresh buffer is a first call's cost, never a
  // repeated step's); without the memory the call goes on without the path
  plan.codes_J = kept_codes_J(plan, tv, mode);
  uint32_t *kcodes = nullptr;
  if (plan.codes_J != 0) {
    // a request the driver refused is not made again until the context's
    // workspace went back (free_workspace): no hipMalloc of the whole slot per step
    const size_t want = kc_bytes(nch, plan.codes_J);
    void *p = nullptr;
    const bool refused = ctx->code_keep_refused != 0 && want >= ctx->code_keep_refused &&
                         ctx->slots[SLOT_CODE_KEEP].bytes < want;
    if (!refused && getenv("KS_TEST_KEPT_CODES_NOMEM") == nullptr &&
        ensure(ctx, SLOT_CODE_KEEP, want, &p) == KS_OK) {
      kcodes = static_cast<uint32_t *>(p);
    } else {
      if (!refused && getenv("KS_TEST_KEPT_CODES_NOMEM") == nullptr) {
        ctx->code_keep_refused = want;
        (void)hipGetLastError();  // (a failed hipMalloc is not this call's error,
        clear_last_error();       //  nor its message this call's)
      }
      ++mode.index->code_alloc_failures;
    }
  }
  plan_codes(plan, prev, kcodes);

  // ---- workspace
  size_t bytes = 0;
  carve(nullptr, plan, nch, ntiles, runs.packed, kp, &bytes);
  void *wsp = nullptr;
  KS_TRY(ensure(ctx, SLOT_CHUNK_A, bytes, &wsp));
  Work w = carve(static_cast<char *>(wsp), plan, nch, ntiles, runs.packed, kp, &bytes);
  const int hx = hint_reuse ? prev.hint : 0;  // the array pass 1 reads; P2 writes the other
  w.xh = kp.hint[hx];
  w.xt = kp.hint[1 - hx];
  // with a sequence index the exact entries live in the kept slot: the carry
  // leaves them there for the next scan (entry_reuse: pass 1 reads them there)
  if (ixid != 0) w.cr.x = kp.entry;
  w.kc = kcodes;
  w.p1.epoch = ++ctx->scan_epoch;
  unsigned long long *cnts = w.cnts;
  KS_HIP(hipMemsetAsync(cnts, 0, 8 * (2 * kSegs + 8), st));
  KS_HIP(hipMemsetAsync(cnts + 3 * kSegs + 8, 0, 8 * (2 * kSegs), st));
  if (plan.need_codes) {
    void *cp = nullptr;
    const int64_t ctiles = (nch + 63) / 64;  // code store tiles (global chunk index / 64): 2 B x 256 per chunk
    KS_TRY(ensure(ctx, SLOT_CHUNK_B, (size_t)ctiles * 64 * CH * 2, &cp));
    w.codes = static_cast<uint16_t *>(cp);
  }
  int64_t ccap = std::max<int64_t>(1 << 16, nch / 4);  // per candidate list
  const size_t cand_bytes = ctx->slots[SLOT_CHUNK_C].bytes;  // use what the grow-only slot holds
  if (cand_bytes > 2048 && (cand_bytes - 2048) / 80 > (size_t)ccap) ccap = (int64_t)((cand_bytes - 2048) / 80);
  const int64_t csegcap = ccap / kSegs;
  ccap = csegcap * kSegs;
  void *cbuf = nullptr;
  KS_TRY(ensure(ctx, SLOT_CHUNK_C, (size_t)ccap * 80 + 2048, &cbuf));
  // kmer_regions: a rescan accompanies a region in the same segment; tr_lr
  // rescans every closed excursion, so its capacity grows on its own
  const int64_t rsegcap = std::max<int64_t>(rb.segcap, ctx->rescan_segcap);
  const int64_t rcap = rsegcap * kSegs;  // per rescan list
  void *rsb = nullptr;
  KS_TRY(ensure(ctx, SLOT_WORK_A, (size_t)rcap * 40 + 2048, &rsb));
  for (int h = 0; h < 2; ++h) {
    long long *cb = reinterpret_cast<long long *>(cbuf) + (size_t)h * 5 * ccap;
    w.cands[h] = Cand{cb, cb + ccap, cb + 2 * ccap, reinterpret_cast<double *>(cb + 3 * ccap),
                      h ? cnts + 3 * kSegs + 8 : cnts, ccap, csegcap};
    int64_t *b = reinterpret_cast<int64_t *>(static_cast<char *>(rsb) + (size_t)h * ((size_t)rcap * 20 + 256));
    w.rss[h] = Rescan{b, b + rcap, reinterpret_cast<int32_t *>(b + 2 * rcap), h ? cnts + 4 * kSegs + 8 : cnts + kSegs,
                      rcap, rsegcap};
  }
  if (plan.debug_carry) {  // per-window carry statistics to stderr
    KS_HIP(hipMalloc(&w.dbg, (w.nwin * 9 + 4) * sizeof(long long)));
    KS_HIP(hipMemsetAsync(w.dbg, 0, (w.nwin * 9 + 4) * sizeof(long long), st));
  }

  // ---- P0 chunk layout, predictor
  KS_TRY(record(kEvBegin, st));
  if (!chunk_reuse) {
    KS_TRY(launch(k_tile_runs, dim3((unsigned)nruns), dim3(256), 0, st, lay.tbase, nruns, w.trun));
    if (ntiles > 0)
      KS_TRY(launch(k_make_chunks, dim3((unsigned)((ntiles + 3) / 4)), dim3(256), 0, st, runs.a, lay.cbase,
                    lay.tbase, w.trun, ntiles, k, runs.b, mode.trlr, w.g));
  }
  bool side_forked = false;  // the side stream already waits for the chunks
  if (hint_reuse) {
    // no predictor: w.xh is the previous call's P2 prediction (from pass 1's
    // exact clean exits and sums, closer than P0's); both parts' pass 1 read it
    // (entry_reuse: they read the kept exact entries, w.cr.x, instead -- the
    // array the test hook then spoils; the general path of the rerun rewrites
    // every entry, so the slot is whole again afterwards)
    if (const char *th = getenv("KS_TEST_ENTRY_HINT")) {
      const int what = !strcmp(th, "zero") ? 0 : !strcmp(th, "huge") ? 1 : !strcmp(th, "nan") ? 2 :
                       !strcmp(th, "shift") ? 3 : -1;
      if (what < 0) return fail(KS_ERR_ARG, "KS_TEST_ENTRY_HINT must be zero, huge, nan or shift");
      double *spoilt = entry_reuse ? w.cr.x : w.xh;
      // (w.pa, the predictor's sums, is free on this path: the copy the shift reads)
      if (what == 3) KS_HIP(hipMemcpyAsync(w.pa, spoilt, (size_t)nch * 8, hipMemcpyDeviceToDevice, st));
      KS_TRY(launch(k_test_hint, dim3((unsigned)((nch + 255) / 256)), dim3(256), 0, st, spoilt, w.pa, nch, what));
    }
    if (const char *tc = plan.codes_read ? getenv("KS_TEST_KEPT_CODES") : nullptr) {
      const int what = !strcmp(tc, "sample") ? 0 : !strcmp(tc, "all") ? 1 : !strcmp(tc, "one") ? 2 : -1;
      if (what < 0) return fail(KS_ERR_ARG, "KS_TEST_KEPT_CODES must be sample, all or one");
      KS_TRY(launch(k_test_codes, dim3(1), dim3(256), 0, st, w.kc, w.g, w.cr, nch, plan.codes_J, what,
                    reinterpret_cast<unsigned int *>(cnts + 2 * kSegs + 1)));
    }
  } else if (plan.p1summ) {
    // the first half's predictor and prescan first (they gate its pass 1;
    // the predictor holds whole CUs: 128 KiB of LDS per block), then the
    // second half's on the side stream, under the first half's pass 1 (also
    // at shard sizes: both first on the main stream measured 2.48 vs 2.38 ms
    // at the 8-way shard, profiles/r4/ab/ab_shard8.txt)
    KS_TRY(predict(c, w, plan.half[0], st));
    if (plan.split) {
      side_forked = true;
      KS_TRY(record(kEvPredictFork, st));
      KS_TRY(wait(side, kEvPredictFork));
      KS_TRY(predict(c, w, plan.half[1], side));
    }
  }
  KS_TRY(record(kEvP1Begin, st));

  // ---- P1 gather pass
  if (plan.family == P1Family::Plain) {
    KS_TRY(pick_bool(plan.comp, [&](auto cp) {
      return launch(k_pass1<1, decltype(cp)::value, false>, dim3((unsigned)((nch + 255) / 256)), dim3(256), 0, st, w.g,
                    s->seq, c.total, k, tv, w.codes, c.ec, visits, w.p1, w.cands[0], (int64_t)0, 0);
    }));
  } else if (plan.rank_alone) {  // every chunk (guarded base loads)
    const dim3 grid((unsigned)((nch + kRankBlock - 1) / kRankBlock));
    KS_TRY(pick_bool(k == 15, [&](auto k15) {
      return launch(k_pass1r<decltype(k15)::value ? 1 : 2>, grid, dim3(kRankBlock), 0, st, w.g, c.total, k, tv, c.ec,
                    visits, w.p1, w.cands[0]);
    }));
  } else if (plan.split) {
    // first half on the highest-priority stream, the tail chunks and the
    // second half on the (lowest-priority) side stream at once: the second
    // half's blocks fill the CUs the first half leaves, its drain included,
    // and the first half ends first (its carry and stitch then run under
    // the rest of the second half; serial halves cost 0.6 ms in-process).
    KS_TRY(record(kEvP1Fork, st));
    KS_TRY(wait(hi, kEvP1Fork));
    if (!side_forked) KS_TRY(wait(side, kEvP1Fork));
    KS_TRY(pass1_half(c, plan, w, plan.half[0], hi, w.cands[0]));
    KS_TRY(record(kEvP1Half0, hi));
    KS_TRY(wait(st, kEvP1Half0));
    if (plan.tail) KS_TRY(pass1_tail(c, plan, w, side, w.cands[1]));  // (the tail chunks are the second half's)
    KS_TRY(pass1_half(c, plan, w, plan.half[1], side, w.cands[1]));
  } else {
    // the tail chunks on the side stream, overlapped with the pipelined pass
    if (plan.tail) {
      KS_TRY(record(kEvP1Half0, st));
      KS_TRY(wait(side, kEvP1Half0));
      KS_TRY(pass1_tail(c, plan, w, side, w.cands[0]));
      KS_TRY(record(kEvSideDone, side));
    }
    KS_TRY(pass1_half(c, plan, w, plan.half[0], st, w.cands[0]));
    if (plan.tail) KS_TRY(wait(st, kEvSideDone));
  }
  // (the first half's post-processing on the high-priority stream, ahead of
  // the second half's pass-1 blocks, measured the same: 14.15 vs 14.15 ms,
  // profiles/r5/ab/ab_post0.txt)
  if (plan.split) {
    // end of pass 1 = the later of the halves: the hi stream (idle now) joins the side stream's
    KS_TRY(record(kEvP1Side, side));
    KS_TRY(wait(hi, kEvP1Side));
    KS_TRY(record(kEvP1End, hi));
  } else {
    KS_TRY(record(kEvP1End, st));
  }
  if (plan.epoch_stale) ++w.p1.epoch;

  // ---- P2-P5 per half, then its candidates and rescans on the main stream
  KS_TRY(post_half(c, plan, w, 0, st));  // two parts: under the second half's pass 1
  KS_TRY(emit_rescan(c, plan, w, 0, st));
  if (plan.split) {
    // (the first half's rescans under the second half's post-processing: config 3
    // 32.1 vs 32.9 ms with both after the join, profiles/r4/ab3/; the second
    // half's rescans after the join, not on the side stream beside the first
    // half's: 28.46 vs 28.53 ms at config 3, metric 14.65 vs 14.71,
    // profiles/r5/ab/ab_rescan_side_*.txt)
    KS_TRY(post_half(c, plan, w, 1, side));
    KS_TRY(record(kEvSideDone, side));
    KS_TRY(wait(st, kEvSideDone));
    KS_TRY(emit_rescan(c, plan, w, 1, st));
  }
  KS_TRY(record(kEvEnd, st));

  // ---- read-back: the scan's counters and the region counters (final: the
  // rescans above append the last regions) in one copy, so scan_impl needs no
  // round trip of its own
  // (with them the sequence index guard's flag, the word after the region counters: kScGuard)
  static_assert(kScGuard == kScRegions + kSegs, "the guard's flag follows the region counters");
  KS_TRY(launch(k_copy_u64, dim3(1), dim3(64), 0, st, rb.count, cnts + 2 * kSegs + 8, kSegs, cnts + 2 * kSegs + 4));
  std::vector<unsigned long long> hcv(5 * kSegs + 8);
  KS_HIP(hipMemcpyAsync(hcv.data(), cnts, 8 * (5 * kSegs + 8), hipMemcpyDeviceToHost, st));
  KS_HIP(hipStreamSynchronize(st));
  std::copy(hcv.begin() + 2 * kSegs + 8, hcv.begin() + 3 * kSegs + 8, ctx->hreg);
  ctx->hguard = hcv[2 * kSegs + 4];
  ctx->hreg_ok = true;
  if (plan.debug_verify) debug_verify(c, w);
  unsigned long long cand_max = 0, res_max = 0, res_tot = 0;
  for (int q = 0; q < kSegs; ++q) {
    const unsigned long long c0 = hcv[q], c1 = hcv[3 * kSegs + 8 + q];
    const unsigned long long r0 = hcv[kSegs + q], r1 = hcv[4 * kSegs + 8 + q];
    cand_max = std::max(cand_max, std::max(c0, c1));
    res_max = std::max(res_max, std::max(r0, r1));
    res_tot += std::min<unsigned long long>(r0, (unsigned long long)rsegcap) +
               std::min<unsigned long long>(r1, (unsigned long long)rsegcap);
  }
  const unsigned long long replays = hcv[2 * kSegs] + hcv[2 * kSegs + 2];
  const unsigned int errbits = (unsigned int)((hcv[2 * kSegs + 1] | hcv[2 * kSegs + 3]) & 0xffffffffull);
  if ((errbits & 16u) && !plan.force_fb)
    fprintf(stderr, "kmer_spans_amd: carry segment check failed; the carry was redone per run\n");
  if (plan.debug_carry) KS_TRY(debug_carry_report(plan, w, nruns));

  // ---- failures and retries
  if (errbits & 32u)
    return fail(KS_ERR_DEVICE, "chunked scan epoch check failed: the stitch read pass-1 results not written by this "
                                 "call (epoch %u)", w.p1.epoch);
  if (entry_reuse && (errbits & (64u | 128u))) {
    // a kept entry was not the exact exit of the chunk before it: nothing of
    // this attempt counts (scan_core resets the region counters and the
    // scratch visit histogram per attempt).  The slot's chunk table and P2 hint
    // were not written, so the tag goes back without entry_ok and the rerun
    // takes the hint path, whose carry rewrites every entry.
    // Bit 128: a sampled kept code was not the table's (k_pass1c).  Either bit
    // on a call that read the codes takes them away too: the next call from
    // exact entries writes them again.
    ctx->chunk_keep = prev;
    ctx->chunk_keep.entry_ok = false;
    if (plan.codes_read || plan.codes_write) ctx->chunk_keep.codes_ok = false;
    if (mode.index) ++mode.index->entry_fallbacks;
    if (mode.index && plan.codes_read) ++mode.index->code_fallbacks;
    return KS_INTERNAL_RETRY;
  }
  if (errbits & ~16u) return fail(KS_ERR_INTERNAL, "chunked scan consistency check failed (bits %u)", errbits);
  if ((int64_t)cand_max > csegcap) {  // grow the candidate buffers and rerun the pass
    void *grown = nullptr;
    const size_t seg = (size_t)(cand_max + cand_max / 4 + 64);
    KS_TRY(ensure(ctx, SLOT_CHUNK_C, seg * kSegs * 80 + 2048, &grown));
    return KS_INTERNAL_RETRY;
  }
  if ((int64_t)res_max > rsegcap) {  // grow the rescan buffer (regions may have overflowed too) and rerun
    ctx->rescan_segcap = (int64_t)(res_max + res_max / 4 + 64);
    return KS_INTERNAL_RETRY;
  }
  const int64_t nres = (int64_t)res_tot;
  if (plan.debug_carry && nres > 0) KS_TRY(debug_rescan_hist(w.rss[0], hcv.data() + kSegs, k, nres));
  if (stats) {  // (phase times: chunked_phase_times, after the call's last sync)
    stats->n_rescan = nres;
    stats->n_replay = (int64_t)replays;
  }
  ctx->chunked_events = true;
  if (ixid != 0) {
    // what this call leaves for the next one: the chunk table, and w.xt, which
    // P2 wrote for every chunk (ascan covers every run and tile of both parts);
    // entry_reuse wrote neither, so the kept hint and its index pass on
    // unchanged.  entry_ok: Work::cr.x is Keep::entry here, and the carry wrote
    // every chunk's entry (general path) or pass 1 verified every one.
    ctx->chunk_keep = ChunkKeep{ixid, k, mode.trlr, nch, ntiles, ksp, mode.table_id, mode.init_id,
                                entry_reuse ? prev.hint : 1 - hx, true};
    // the kept codes: written or read and verified by this call, or left as they
    // were by a call from exact entries that went without them; any other call
    // (another table, the general path) leaves none
    if (entry_reuse) {
      const bool used = plan.codes_read || plan.codes_write;
      ctx->chunk_keep.codes_ok = used || prev.codes_ok;
      ctx->chunk_keep.codes_base = used ? kcodes : prev.codes_base;
      ctx->chunk_keep.codes_J = used ? plan.codes_J : prev.codes_J;
    }
    ks_seq_index *ix = mode.index;
    if (plan.codes_write) ++ix->code_builds;
    if (plan.codes_read) ++ix->code_reuses;
    if (chunk_reuse) ++ix->chunk_reuses;
    if (hint_reuse) ++ix->hint_reuses;
    if (entry_reuse) ++ix->entry_reuses;
    if (plan.p1summ && !hint_reuse) ++ix->predictor_builds;
  }
  return KS_OK;
}

}  // namespace ks

// Where the kept codes keep scan index i of chunk c of nch, in steps of J:
// the slot's bytes and the index's halfword offset (host arithmetic only).
extern "C" ks_status ks_kept_codes_layout(int32_t J, int64_t nch, int64_t c, int32_t i, int64_t *bytes,
                                          int64_t *halfword) {
  using namespace ks;
  if (J < 2 || J > 8 || nch < 0 || c < 0 || c >= std::max<int64_t>(nch, 1) || i < 0 || i >= CH || !bytes || !halfword)
    return fail(KS_ERR_ARG, "ks_kept_codes_layout: bad argument");
  *bytes = (int64_t)kc_bytes(nch, J);
  *halfword = (int64_t)(kc_slot(c, i / J, J) * 2 + (size_t)(i % J));
  return KS_OK;
}

// Test-only read window (as ks_table_debug_read): the kept codes of chunks
// [c0, c0 + nchunks) of the context's last chunked scan, in index order, 256
// per chunk -- a copy to the host and a host reorder, no kernel and no device
// write.  KS_ERR_ARG when the context keeps no codes.
extern "C" ks_status ks_kept_codes_debug_read(ks_ctx *ctx, int64_t c0, int64_t nchunks, uint16_t *dst_host,
                                              int32_t *steps_J) {
  using namespace ks;
  if (!ctx) ctx = ks_default_ctx();
  if (!ctx || !dst_host) return fail(KS_ERR_ARG, "ks_kept_codes_debug_read: null argument");
  const ChunkKeep &kk = ctx->chunk_keep;
  if (kk.id == 0 || !kk.codes_ok || kk.codes_base != ctx->slots[SLOT_CODE_KEEP].ptr || kk.codes_J == 0)
    return fail(KS_ERR_ARG, "ks_kept_codes_debug_read: the context keeps no codes");
  if (c0 < 0 || nchunks < 0 || c0 > kk.nch || nchunks > kk.nch - c0)
    return fail(KS_ERR_ARG, "ks_kept_codes_debug_read: chunks [%lld, %lld + %lld) outside the scan's %lld",
                (long long)c0, (long long)c0, (long long)nchunks, (long long)kk.nch);
  if (steps_J) *steps_J = kk.codes_J;
  if (nchunks == 0) return KS_OK;
  const int J = kk.codes_J;
  const int64_t t0 = c0 >> 6, t1 = (c0 + nchunks + 63) >> 6;
  const size_t tile_dw = (size_t)kc_steps(J) * 64 * kc_words(J);
  std::vector<uint32_t> h((size_t)(t1 - t0) * tile_dw);
  int cur = -1;
  KS_HIP(hipGetDevice(&cur));
  KS_HIP(hipSetDevice(ctx->device));
  const hipError_t e = hipMemcpy(h.data(), static_cast<const uint32_t *>(kk.codes_base) + (size_t)t0 * tile_dw,
                                 h.size() * 4, hipMemcpyDeviceToHost);
  if (cur >= 0) (void)hipSetDevice(cur);
  KS_HIP(e);
  const uint16_t *hh = reinterpret_cast<const uint16_t *>(h.data());
  for (int64_t c = c0; c < c0 + nchunks; ++c)
    for (int i = 0; i < CH; ++i)
      dst_host[(size_t)(c - c0) * CH + i] = hh[(kc_slot(c, i / J, J) - (size_t)t0 * tile_dw) * 2 + (size_t)(i % J)];
  return KS_OK;
}

namespace ks {

// Phase times of the last chunked scan on ctx (its events are complete once
// the caller has synchronised after the region readback).
ks_status chunked_phase_times(ks_ctx *ctx, ks_scan_stats *stats) {
  if (!ctx->chunked_events) {  // nothing to scan (no run longer than k): no phase was recorded
    stats->ms_layout = stats->ms_scan = stats->ms_predict = stats->ms_carry = stats->ms_stitch = stats->ms_rescan = 0;
    return KS_OK;
  }
  float ms_lay = 0, ms_p1 = 0, ms_p2 = 0, ms_p34 = 0, ms_p5 = 0, ms_res = 0;
  KS_HIP(hipEventElapsedTime(&ms_lay, ctx->ev[kEvBegin], ctx->ev[kEvP1Begin]));
  KS_HIP(hipEventElapsedTime(&ms_p1, ctx->ev[kEvP1Begin], ctx->ev[kEvP1End]));
  KS_HIP(hipEventElapsedTime(&ms_p2, ctx->ev[kEvP1End], ctx->ev[kEvP2End]));
  KS_HIP(hipEventElapsedTime(&ms_p34, ctx->ev[kEvP2End], ctx->ev[kEvP34End]));
  KS_HIP(hipEventElapsedTime(&ms_p5, ctx->ev[kEvP34End], ctx->ev[kEvCandEnd]));
  KS_HIP(hipEventElapsedTime(&ms_res, ctx->ev[kEvCandEnd], ctx->ev[kEvEnd]));
  // (the second part's P2-P5 events can precede the end of the union of the
  // pass-1 launches when it finished first: such a phase counts 0)
  stats->ms_layout = ms_lay;
  stats->ms_scan = ms_p1;
  stats->ms_predict = std::max(0.0f, ms_p2);
  stats->ms_carry = std::max(0.0f, ms_p34);
  stats->ms_stitch = std::max(0.0f, ms_p5);
  stats->ms_rescan = ms_res;
  return KS_OK;
}

// ------------------------------------------------------------ diagnostics
namespace {

// KS_DEBUG_VERIFY=1: after a chunked scan of a small input (<= 64 Mi bases,
// k <= 11, kmer_regions mode), the device's packed codes, chunk layout,
// pass-1 results and carry modes are copied back and checked against a host
// recomputation from the sequence bytes and the base table; every mismatch
// goes to stderr with its chunk and both values.  Reads the buffers after the
// call's last kernel, so a value that is right here but was wrong when a
// kernel read it points at an ordering edge, one that is wrong here at the
// kernel that wrote it.
void debug_verify(const ScanCall &c, const Work &w) {
  const Chunks &g = w.g;
  const P1 &p1 = w.p1;
  const Carry &cr = w.cr;
  const TableView &tv = c.tv;
  const int64_t total = c.total, nch = g.nch;
  const int k = c.k;
  if (c.mode.trlr || k > 11 || total > ((int64_t)64 << 20) || nch <= 0) return;
  (void)hipDeviceSynchronize();
  auto get = [&](auto *dst, const void *src, size_t n) {
    if (n) (void)hipMemcpy(dst, src, n * sizeof(*dst), hipMemcpyDeviceToHost);
  };
  std::vector<uint8_t> seq((size_t)total);
  get(seq.data(), c.s->seq, (size_t)total);
  const int64_t nk = (int64_t)1 << (2 * k);
  std::vector<double> val((size_t)nk);
  if (tv.compressed) {
    std::vector<uint16_t> codes((size_t)nk);
    get(codes.data(), tv.codes, (size_t)nk);
    std::vector<double> lut((size_t)std::max(tv.nlut, 1));
    get(lut.data(), tv.lut, (size_t)tv.nlut);
    for (int64_t i = 0; i < nk; ++i) val[i] = lut[codes[i]];
  } else {
    get(val.data(), tv.vals, (size_t)nk);
  }
  long long bad = 0;
  auto report = [&](const char *what, int64_t ch, double got, double want) {
    if (++bad <= 12)
      fprintf(stderr, "[verify] chunk %lld of %lld: %s = %.17g, host %.17g\n", (long long)ch, (long long)nch, what, got,
              want);
  };
  std::vector<int64_t> start((size_t)nch);
  std::vector<int32_t> n((size_t)nch), run((size_t)nch), tbeg((size_t)nch), targ((size_t)nch);
  std::vector<double> cexit((size_t)nch), tmax((size_t)nch), cx((size_t)nch);
  std::vector<uint8_t> mode((size_t)nch);
  get(start.data(), g.start, (size_t)nch);
  get(n.data(), g.n, (size_t)nch);
  if (g.packed) {  // the words the chunks read (a part's run pass packs its own range only)
    const int64_t nw = total / 16 + 1;
    std::vector<uint32_t> pk((size_t)nw);
    std::vector<uint8_t> used((size_t)nw, 0);
    for (int64_t ch = 0; ch < nch; ++ch)
      for (int64_t q = std::max<int64_t>(0, (start[ch] - k) / 16); q <= (start[ch] + n[ch]) / 16 && q < nw; ++q)
        used[q] = 1;
    get(pk.data(), g.packed, (size_t)nw);
    for (int64_t q = 0; q < nw; ++q) {
      uint32_t want = 0;
      for (int b = 0; b < 16; ++b) want |= enc(16 * q + b < total ? seq[16 * q + b] : (uint8_t)'N') << (30 - 2 * b);
      if (used[q] && pk[q] != want && 16 * q + 16 <= total) report("packed word", q, (double)pk[q], (double)want);
    }
  }
  get(run.data(), g.run, (size_t)nch);
  get(tbeg.data(), p1.tbeg, (size_t)nch);
  get(targ.data(), p1.targ, (size_t)nch);
  get(cexit.data(), p1.cexit, (size_t)nch);
  get(tmax.data(), p1.tmax, (size_t)nch);
  get(cx.data(), cr.x, (size_t)nch);
  get(mode.data(), cr.mode, (size_t)nch);
  const uint64_t kmask = (uint64_t)nk - 1;
  for (int64_t ch = 0; ch < nch; ++ch) {
    // clean trajectory from 0 over indices start .. start + n - 1 (k-mer
    // ending at index - 1), as P1Lane::step
    double prev = 0.0, best = 0.0;
    int beg = -1, arg = 0;
    for (int i = 0; i < n[ch]; ++i) {
      const int64_t p = start[ch] + i;
      uint64_t code = 0;
      for (int64_t q = p - k; q < p; ++q) code = ((code << 2) | enc(seq[q])) & kmask;
      const double sv = val[code];
      const double tt = prev + sv;
      const double S = tt > 0 ? tt : 0.0;
      const bool open = (prev == 0) & (S > 0), close = (prev > 0) & (S == 0);
      const bool up = open | (S > best);
      best = up ? S : best;
      arg = up ? i : arg;
      beg = open ? i : (close ? -1 : beg);
      prev = S;
    }
    auto ne = [](double a, double b) { return memcmp(&a, &b, 8) != 0; };
    if (ne(cexit[ch], prev)) report("clean exit", ch, cexit[ch], prev);
    if (prev > 0) {
      if (tbeg[ch] != beg) report("tail begin", ch, tbeg[ch], beg);
      if (targ[ch] != arg) report("tail argmax", ch, targ[ch], arg);
      if (ne(tmax[ch], best)) report("tail max", ch, tmax[ch], best);
    } else if (tbeg[ch] != -1) {
      report("tail begin (none)", ch, tbeg[ch], -1);
    }
    const bool first = ch == 0 || run[ch - 1] != run[ch];
    if (first && (mode[ch] != kModeClean || cx[ch] != 0.0)) report("run-first chunk carry mode", ch, mode[ch], kModeClean);
  }
  if (bad) fprintf(stderr, "[verify] %lld mismatches in %lld chunks (k %d, %lld bases)\n", bad, (long long)nch, k,
                   (long long)total);
}

// KS_DEBUG_CARRY=1: what the summary selection and the carry counted (Work::dbg,
// freed here), per call and for the eight costliest 64-chunk windows.
ks_status debug_carry_report(const ScanPlan &plan, Work &w, int64_t nruns) {
  const int64_t nwin = w.nwin, nch = w.g.nch;
  if (plan.p1summ) {
    unsigned long long nf2[2] = {0, 0};
    KS_HIP(hipMemcpy(nf2, w.nfix, 16, hipMemcpyDeviceToHost));
    unsigned long long why[3] = {0, 0, 0};
    KS_HIP(hipMemcpy(why, w.dbg + nwin * 9, 24, hipMemcpyDeviceToHost));
    fprintf(stderr, "[p1summ] chunks %lld gathered summaries %llu (no prediction %llu, void %llu, other binade %llu)\n",
            (long long)nch, nf2[0] + nf2[1], why[0], why[1], why[2]);
    if (w.rpb.slot) {
      unsigned long long rc[2] = {0, 0};
      KS_HIP(hipMemcpy(rc, w.rpb.count, 16, hipMemcpyDeviceToHost));
      fprintf(stderr, "[replay prefetch] listed %llu + %llu chunks (cap %lld per half)\n", rc[0], rc[1],
              (long long)w.rpb.cap);
    }
  }
  std::vector<long long> h(nwin * 9);
  KS_HIP(hipMemcpy(h.data(), w.dbg, nwin * 9 * sizeof(long long), hipMemcpyDeviceToHost));
  KS_HIP(hipFree(w.dbg));
  w.dbg = nullptr;
  std::vector<int64_t> idx(nwin);
  for (int64_t i = 0; i < nwin; ++i) idx[i] = i;
  std::sort(idx.begin(), idx.end(), [&](int64_t a, int64_t b) { return h[9 * a] > h[9 * b]; });
  long long tot[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int64_t i = 0; i < nwin; ++i)
    for (int q = 0; q < 9; ++q) tot[q] += h[9 * i + q];
  fprintf(stderr, "[carry] windows %lld (runs %lld) chunks %lld replays %lld (wave-parallel %lld, bases prefetched "
          "%lld; cycles %lld, in fast tiles %lld, in replays %lld) segments %lld L %lld R %lld\n", (long long)nwin,
          (long long)nruns, tot[1], tot[2], tot[8] & 0xffffffffLL, tot[8] >> 32, tot[0], tot[6], tot[7], tot[3],
          tot[4], tot[5]);
  for (int64_t i = 0; i < std::min<int64_t>(nwin, 8); ++i) {
    const long long *d = &h[9 * idx[i]];
    fprintf(stderr, "[carry] window %lld cycles %lld (fast tiles %lld, replays %lld) chunks %lld replays %lld "
            "segments %lld L %lld R %lld\n", (long long)idx[i], d[0], d[6], d[7], d[1], d[2], d[3], d[4], d[5]);
  }
  return KS_OK;
}

// KS_DEBUG_CARRY=1: length histogram (log2 buckets) of the first list's rescans.
ks_status debug_rescan_hist(const Rescan &rs, const unsigned long long *counts, int k, int64_t nres) {
  std::vector<int64_t> a(rs.cap), b(rs.cap);
  KS_HIP(hipMemcpy(a.data(), rs.a, rs.cap * 8, hipMemcpyDeviceToHost));
  KS_HIP(hipMemcpy(b.data(), rs.b, rs.cap * 8, hipMemcpyDeviceToHost));
  long long hist[40] = {0}, tot = 0, mx = 0;
  for (int64_t i = 0; i < rs.cap; ++i) {
    if ((i % rs.segcap) >= (int64_t)counts[i / rs.segcap]) continue;
    const long long L = b[i] - a[i] - k;
    tot += L;
    mx = std::max(mx, L);
    int e = 0;
    while (e < 39 && (1LL << (e + 1)) <= L) ++e;
    ++hist[L > 0 ? e : 0];
  }
  fprintf(stderr, "[rescan] n %lld indices %lld max %lld |", (long long)nres, tot, mx);
  for (int e = 0; e < 40; ++e)
    if (hist[e]) fprintf(stderr, " 2^%d:%lld", e, hist[e]);
  fprintf(stderr, "\n");
  return KS_OK;
}

static_assert(CH == kChunk, "the scan's chunk is the layout's chunk (ks_runs.hip cuts the runs by kChunk)");

}  // namespace

}  // namespace ks

extern "C" int32_t ks_scan_chunk_indices(void) { return ks::CH; }
extern "C" int32_t ks_scan_tile_chunks(void) { return ks::kTileChunks; }
