// k_score.hip -- scores of predictions against held-out targets on gfx950 (gpar_score_samples,
// gpar_score_gaussian): a per-entry pass that writes one small record per entry, and a reduction
// of the records to per-output aggregates in a fixed order.
//
// Sample scorer.  Entry (i, c) of F[s * ld_s + i * ld_r + c * ld_c] (s < S) owns a list of S
// doubles and a target y = Y[i * ldy_r + c * ldy_c].  With x the ascending sort and d_k = x_k - y:
//   below = #{s : F_s < y}, equal = #{s : F_s == y}                               (exact)
//   bin   = min(B - 1, ((2 below + equal) B) / (2 S))      (integer mid-rank PIT bin, exact)
//   crps  = (1/S) sum_k |d_k| - (1/S^2) sum_k (2k - S + 1) d_k      (the energy form about y)
//   inside_l = Q(q_lo) <= y <= Q(q_hi), Q = k_quantile.hip's quantile: the same (lo, g) from the
//              host, the same quant_lerp
// Both sums are taken by a binary tree over the positions 0 .. 2^m - 1 (terms past S are zero):
// level 0 adds positions (2j, 2j + 1), level 1 the results of (4j, 4j + 2), ...  Zero padding
// changes no value, so the order is a function of S alone and the register and LDS paths give an
// entry the same bits.  FMA contraction is off in the terms and the sums.
// status: 0 scored, 1 missing (y is NaN), 2 bad (y present, a sample NaN); a missing or bad
// entry's record is crps = NaN, below = equal = -1.
//
// Register path (S <= kScoreRegMax): one lane per entry, the list in NP = 16 / 32 / 64
// registers (NP = 128 needs scratch beside the two trees: DESIGN 4.10); below / equal / the NaN
// test are counted as the list is loaded, then the network sorts, the quantiles are picked by a chain of selects on the uniform lo, and the two trees run
// depth-first (log2 NP partial sums live).
// LDS path (S <= 4096): a 256-thread workgroup over G lists of NP2 doubles, sorted by the bitonic
// network; thread l takes list l's rank (two binary searches of the sorted list: the same counts)
// and its quantiles, then all threads turn the lists into the level-0 sums in place (|d| sums at
// even positions, weighted sums at odd ones) and walk up the tree.  No atomics.
//
// Gaussian scorer: one lane per entry, z = (y - mu) / sigma, record crps, log density, squared
// error; status 2 for a NaN mu or sigma or sigma <= 0.
//
// Reduction (both scorers): records are indexed e = i p + c.  Stage 1: workgroup (chunk, c) takes
// the kScoreChunk = 256 points i = 256 chunk + t of output c: a fixed tree over the 256 lanes for
// the fp64 sums (zeros for lanes that are not scored), integer LDS counters for the counts.
// Stage 2: one thread per (c, field) adds the chunk partials in index order.  The order depends
// on (n, p) alone; counts are integers; no floating-point atomics anywhere.
#include <cstdlib>
#include <cstring>

#include "device_common.hpp"
#include "launch.hpp"
#include "nm_dev.hpp"
#include "sort_net.hpp"

namespace gpar {

std::atomic<int64_t> g_score_reg_launches{0}, g_score_lds_launches{0};

struct ScoreSel {
  int nl, bins;
  int lo[2 * kScoreMaxL];      // [2l] the lower quantile of level l, [2l + 1] the upper
  double g[2 * kScoreMaxL];
};

struct GaussSel {
  int nl, bins;
  double z[kScoreMaxL];
};

constexpr unsigned kStScored = 0, kStMissing = 1, kStBad = 2, kStNone = 3;

__device__ __forceinline__ unsigned score_flags(unsigned inside, int bin, unsigned status) {
  return inside | ((unsigned)bin << 8) | (status << 16);
}

// the record of a sample-scored entry from its sums, counts and inside mask
__device__ __forceinline__ void score_write(const ScoreRec& rec, int64_t r, int S, int bins,
                                            double y, bool nan_sample, double s1, double s2,
                                            int below, int equal, unsigned inside) {
  GPAR_NO_FMA
  const unsigned status = y != y ? kStMissing : (nan_sample ? kStBad : kStScored);
  const double fs = (double)S;
  const double crps = s1 / fs - s2 / (fs * fs);
  int bin = ((2 * below + equal) * bins) / (2 * S);
  if (bin > bins - 1) bin = bins - 1;
  const bool ok = status == kStScored;
  rec.crps[r] = ok ? crps : __builtin_nan("");
  rec.below[r] = ok ? below : -1;
  rec.equal[r] = ok ? equal : -1;
  rec.flags[r] = score_flags(ok ? inside : 0u, ok ? bin : 0, status);
}

// ---------------------------------------------------------------------------- register path
// the tree over positions [LO, LO + LEN) of sum |d_k| (W = false) or sum (2k - S + 1) d_k
template <int NP, int LO, int LEN, bool W>
__device__ __forceinline__ double score_tree(const double (&x)[NP], double y, int S) {
  GPAR_NO_FMA
  if constexpr (LEN == 1) {
    const double d = x[LO] - y;
    const double t = W ? (double)(2 * LO - S + 1) * d : fabs(d);
    return LO < S ? t : 0.0;
  } else {
    const double a = score_tree<NP, LO, LEN / 2, W>(x, y, S);
    const double b = score_tree<NP, LO + LEN / 2, LEN / 2, W>(x, y, S);
    return a + b;
  }
}

// lane = entry e0 + blockIdx.x * 64 + threadIdx.x; its record at rec_off + e
template <int NP>
__global__ __launch_bounds__(64) void score_reg(const double* __restrict__ F, int S, int64_t p,
                                                int64_t ld_s, int64_t ld_r, int64_t ld_c,
                                                const double* __restrict__ Y, int64_t ldy_r,
                                                int64_t ldy_c, int64_t e0, int64_t e1,
                                                ScoreSel sel, ScoreRec rec, int64_t rec_off) {
  const int64_t e = e0 + blockIdx.x * (int64_t)64 + threadIdx.x;
  if (e >= e1) return;
  const int64_t i = e / p, c = e - i * p;
  const double* f = F + i * ld_r + c * ld_c;
  const double y = Y[i * ldy_r + c * ldy_c];
  double x[NP];
#pragma unroll
  for (int k = 0; k < NP; ++k) x[k] = k < S ? f[(int64_t)k * ld_s] : INFINITY;
  bool bad = false;
  int below = 0, equal = 0;
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    bad |= x[k] != x[k];
    if (k < S) {
      below += x[k] < y ? 1 : 0;
      equal += x[k] == y ? 1 : 0;
    }
  }
  oem_sort<NP>(x);
  unsigned inside = 0;
  for (int l = 0; l < sel.nl; ++l) {
    // chains of selects on the uniform lo, as quantile_reg picks (a runtime index would put x
    // into scratch)
    const int lo0 = sel.lo[2 * l], hi0 = lo0 + 1 < S ? lo0 + 1 : S - 1;
    const int lo1 = sel.lo[2 * l + 1], hi1 = lo1 + 1 < S ? lo1 + 1 : S - 1;
    double a0 = x[0], b0 = x[0], a1 = x[0], b1 = x[0];
#pragma unroll
    for (int k = 1; k < NP; ++k) {
      a0 = k == lo0 ? x[k] : a0;
      b0 = k == hi0 ? x[k] : b0;
      a1 = k == lo1 ? x[k] : a1;
      b1 = k == hi1 ? x[k] : b1;
    }
    const double ql = quant_lerp(a0, b0, sel.g[2 * l]);
    const double qh = quant_lerp(a1, b1, sel.g[2 * l + 1]);
    inside |= (ql <= y && y <= qh) ? 1u << l : 0u;
  }
  const double s1 = score_tree<NP, 0, NP, false>(x, y, S);
  const double s2 = score_tree<NP, 0, NP, true>(x, y, S);
  score_write(rec, rec_off + e, S, sel.bins, y, bad, s1, s2, below, equal, inside);
}

// ---------------------------------------------------------------------------- LDS path
// workgroup = G consecutive entries from e0 + blockIdx.x * G; lists at sh[l * NP2 ...]
__global__ __launch_bounds__(256) void score_lds(const double* __restrict__ F, int S, int NP2,
                                                 int G, int64_t p, int64_t ld_s, int64_t ld_r,
                                                 int64_t ld_c, const double* __restrict__ Y,
                                                 int64_t ldy_r, int64_t ldy_c, int64_t e0,
                                                 int64_t e1, ScoreSel sel, ScoreRec rec,
                                                 int64_t rec_off) {
  extern __shared__ double sh[];
  __shared__ int bad[kQuantLdsMaxG];
  __shared__ double yv[kQuantLdsMaxG];
  const int tid = threadIdx.x;
  const int64_t eb = e0 + blockIdx.x * (int64_t)G;
  if (tid < G) {
    bad[tid] = 0;
    const int64_t e = eb + tid;
    double y = 0.0;
    if (e < e1) {
      const int64_t i = e / p, c = e - i * p;
      y = Y[i * ldy_r + c * ldy_c];
    }
    yv[tid] = y;
  }
  __syncthreads();
  // list l's sample s: l fastest, so a step's G loads are consecutive entries
  for (int idx = tid; idx < G * NP2; idx += 256) {
    const int l = idx % G, s = idx / G;
    const int64_t e = eb + l;
    double v = INFINITY;
    if (s < S && e < e1) {
      const int64_t i = e / p, c = e - i * p;
      v = F[(int64_t)s * ld_s + i * ld_r + c * ld_c];
      if (v != v) bad[l] = 1;
    }
    sh[l * NP2 + s] = v;
  }
  __syncthreads();
  bitonic_sort_lists(sh, NP2, G, tid);
  // thread l: list l's rank and quantiles from the sorted list, kept in registers over the tree
  int below = 0, equal = 0;
  unsigned inside = 0;
  if (tid < G) {
    const double* x = sh + tid * NP2;
    const double y = yv[tid];
    int a = 0, b = S;
    while (a < b) {   // the first position that is not below y
      const int m = (a + b) >> 1;
      if (x[m] < y) a = m + 1;
      else b = m;
    }
    below = a;
    b = S;
    while (a < b) {   // the first position above y
      const int m = (a + b) >> 1;
      if (x[m] <= y) a = m + 1;
      else b = m;
    }
    equal = a - below;
    for (int l = 0; l < sel.nl; ++l) {
      const int lo0 = sel.lo[2 * l], hi0 = lo0 + 1 < S ? lo0 + 1 : S - 1;
      const int lo1 = sel.lo[2 * l + 1], hi1 = lo1 + 1 < S ? lo1 + 1 : S - 1;
      const double ql = quant_lerp(x[lo0], x[hi0], sel.g[2 * l]);
      const double qh = quant_lerp(x[lo1], x[hi1], sel.g[2 * l + 1]);
      inside |= (ql <= y && y <= qh) ? 1u << l : 0u;
    }
  }
  __syncthreads();
  // level 0 of both trees, in place: positions (2j, 2j + 1) become (sum |d|, weighted sum)
  const int half = G * NP2 / 2;
  for (int t = tid; t < half; t += 256) {
    GPAR_NO_FMA
    const int u = 2 * t;
    const int w = u & (NP2 - 1);
    const double y = yv[u / NP2];
    const double d0 = sh[u] - y, d1 = sh[u + 1] - y;
    const double m0 = w < S ? fabs(d0) : 0.0, m1 = w + 1 < S ? fabs(d1) : 0.0;
    const double w0 = w < S ? (double)(2 * w - S + 1) * d0 : 0.0;
    const double w1 = w + 1 < S ? (double)(2 * w + 2 - S + 1) * d1 : 0.0;
    sh[u] = m0 + m1;
    sh[u + 1] = w0 + w1;
  }
  __syncthreads();
  for (int st = 2; st < NP2; st <<= 1) {
    const int cnt = G * NP2 / (2 * st);
    for (int t = tid; t < cnt; t += 256) {
      GPAR_NO_FMA
      const int base = t * 2 * st;   // 2 st divides NP2: a pair never straddles two lists
      sh[base] = sh[base] + sh[base + st];
      sh[base + 1] = sh[base + 1] + sh[base + st + 1];
    }
    __syncthreads();
  }
  if (tid < G && eb + tid < e1)
    score_write(rec, rec_off + eb + tid, S, sel.bins, yv[tid], bad[tid] != 0, sh[tid * NP2],
                sh[tid * NP2 + 1], below, equal, inside);
}

// ---------------------------------------------------------------------------- Gaussian scorer
__global__ __launch_bounds__(256) void score_gauss(
    const double* __restrict__ M, int64_t ldm_r, int64_t ldm_c, const double* __restrict__ Sd,
    int64_t lds_r, int64_t lds_c, const double* __restrict__ Y, int64_t ldy_r, int64_t ldy_c,
    int64_t p, int64_t e0, int64_t e1, GaussSel sel, ScoreRec rec, int64_t rec_off) {
  GPAR_NO_FMA
  const int64_t e = e0 + blockIdx.x * (int64_t)256 + threadIdx.x;
  if (e >= e1) return;
  const int64_t i = e / p, c = e - i * p;
  const double mu = M[i * ldm_r + c * ldm_c], sg = Sd[i * lds_r + c * lds_c];
  const double y = Y[i * ldy_r + c * ldy_c];
  const unsigned status =
      y != y ? kStMissing : ((mu != mu || sg != sg || !(sg > 0.0)) ? kStBad : kStScored);
  const double z = (y - mu) / sg;
  const double kInvSqrt2 = 0.70710678118654752440, kInvSqrt2Pi = 0.39894228040143267794;
  const double kInvSqrtPi = 0.56418958354775628695, kLog2Pi = 1.8378770664093454836;
  const double Phi = 0.5 * erfc(-z * kInvSqrt2);
  const double phi = kInvSqrt2Pi * exp(-0.5 * z * z);
  const double crps = sg * (z * erf(z * kInvSqrt2) + 2.0 * phi - kInvSqrtPi);
  const double ld = -0.5 * (kLog2Pi + 2.0 * log(sg)) - 0.5 * z * z;
  const double err = y - mu;
  int bin = (int)floor(Phi * (double)sel.bins);
  if (bin > sel.bins - 1) bin = sel.bins - 1;
  if (bin < 0) bin = 0;
  unsigned inside = 0;
  const double az = fabs(z);
  for (int l = 0; l < sel.nl; ++l) inside |= az <= sel.z[l] ? 1u << l : 0u;
  const bool ok = status == kStScored;
  const int64_t r = rec_off + e;
  const double nan = __builtin_nan("");
  rec.crps[r] = ok ? crps : nan;
  rec.x1[r] = ok ? ld : nan;
  rec.x2[r] = ok ? err * err : nan;
  rec.flags[r] = score_flags(ok ? inside : 0u, ok ? bin : 0, status);
}

// ---------------------------------------------------------------------------- reduction
// stage 1: workgroup b = chunk * p + c (from b0); pd[b * 3 + k], pi[b * ni + f],
// f = scored, missing, bad, inside[nl], hist[bins]
__global__ __launch_bounds__(kScoreChunk) void score_chunks(ScoreRec rec, int64_t n, int64_t p,
                                                            int nl, int bins, int64_t b0,
                                                            double* __restrict__ pd,
                                                            int32_t* __restrict__ pi) {
  __shared__ double sd[3][kScoreChunk];
  __shared__ int si[3 + kScoreMaxL + kScoreMaxBins];
  const int tid = threadIdx.x;
  const int64_t b = b0 + blockIdx.x;
  const int64_t chunk = b / p, c = b - chunk * p;
  const int64_t i = chunk * kScoreChunk + tid;
  const int ni = 3 + nl + bins;
  if (tid < ni) si[tid] = 0;
  unsigned flags = kStNone << 16;
  double v0 = 0.0, v1 = 0.0, v2 = 0.0;
  if (i < n) {
    const int64_t e = i * p + c;
    flags = rec.flags[e];
    if ((flags >> 16) == kStScored) {
      v0 = rec.crps[e];
      if (rec.x1) {
        v1 = rec.x1[e];
        v2 = rec.x2[e];
      }
    }
  }
  sd[0][tid] = v0;
  sd[1][tid] = v1;
  sd[2][tid] = v2;
  __syncthreads();
  const unsigned status = flags >> 16;
  if (status < kStNone) atomicAdd(&si[status], 1);   // integer LDS counters: order-free
  if (status == kStScored) {
    for (int l = 0; l < nl; ++l)
      if (flags >> l & 1u) atomicAdd(&si[3 + l], 1);
    atomicAdd(&si[3 + nl + (int)(flags >> 8 & 0xFFu)], 1);
  }
  for (int st = kScoreChunk / 2; st > 0; st >>= 1) {
    if (tid < st) {
      GPAR_NO_FMA
      sd[0][tid] = sd[0][tid] + sd[0][tid + st];
      sd[1][tid] = sd[1][tid] + sd[1][tid + st];
      sd[2][tid] = sd[2][tid] + sd[2][tid + st];
    }
    __syncthreads();
  }
  if (tid < 3) pd[b * 3 + tid] = sd[tid][0];
  if (tid < ni) pi[b * ni + tid] = si[tid];
}

// stage 2: thread g = c * (3 + ni) + f adds field f of output c over the chunks in index order;
// od[c * 3 + f] (f < 3), oi[c * ni + f - 3]
__global__ __launch_bounds__(256) void score_finish(const double* __restrict__ pd,
                                                    const int32_t* __restrict__ pi,
                                                    int64_t nchunks, int64_t p, int ni,
                                                    double* __restrict__ od,
                                                    int64_t* __restrict__ oi) {
  GPAR_NO_FMA
  const int64_t gid = blockIdx.x * (int64_t)256 + threadIdx.x;
  const int nf = 3 + ni;
  if (gid >= p * nf) return;
  const int64_t c = gid / nf;
  const int f = (int)(gid - c * nf);
  if (f < 3) {
    double s = 0.0;
    for (int64_t k = 0; k < nchunks; ++k) s = s + pd[(k * p + c) * 3 + f];
    od[c * 3 + f] = s;
  } else {
    int64_t s = 0;
    for (int64_t k = 0; k < nchunks; ++k) s += pi[(k * p + c) * ni + (f - 3)];
    oi[c * ni + (f - 3)] = s;
  }
}

// per-entry records to the caller's strided device arrays (each optional)
__global__ __launch_bounds__(256) void score_export(ScoreRec rec, int64_t p, int64_t e0,
                                                    int64_t e1, ScoreOut out) {
  const int64_t e = e0 + blockIdx.x * (int64_t)256 + threadIdx.x;
  if (e >= e1) return;
  const int64_t i = e / p, c = e - i * p;
  if (out.crps) out.crps[i * out.ldc_r + c * out.ldc_c] = rec.crps[e];
  if (out.below) out.below[i * out.ldb_r + c * out.ldb_c] = rec.below[e];
  if (out.equal) out.equal[i * out.lde_r + c * out.lde_c] = rec.equal[e];
  if (out.x1) out.x1[i * out.ld1_r + c * out.ld1_c] = rec.x1[e];
  if (out.x2) out.x2[i * out.ld2_r + c * out.ld2_c] = rec.x2[e];
}

// ---------------------------------------------------------------------------- launchers
// GPAR_SCORE_PATH=reg / lds (tests): the register path at every S it can hold / the LDS path at
// every S
static_assert(kScoreRegMax == 64, "the register path's widest instantiation");
static int score_forced_path() {
  const char* e = std::getenv("GPAR_SCORE_PATH");
  if (!e) return 0;
  if (std::strcmp(e, "reg") == 0) return 1;
  if (std::strcmp(e, "lds") == 0) return 2;
  return 0;
}

void launch_score_samples(hipStream_t st, const double* F, int S, int64_t n, int64_t p,
                          int64_t ld_s, int64_t ld_r, int64_t ld_c, const double* Y,
                          int64_t ldy_r, int64_t ldy_c, int nl, const int* lo, const double* g,
                          int bins, const ScoreRec& rec, int64_t rec_off) {
  ScoreSel sel;
  sel.nl = nl;
  sel.bins = bins;
  for (int j = 0; j < 2 * kScoreMaxL; ++j) {
    sel.lo[j] = j < 2 * nl ? lo[j] : 0;
    sel.g[j] = j < 2 * nl ? g[j] : 0.0;
  }
  const int forced = score_forced_path();
  const bool reg = forced == 2 ? false : S <= kScoreRegMax;
  const int64_t ne = n * p;
  if (reg) {
    const int64_t per = (int64_t)64 << 24;   // entries per launch (2^24 blocks)
    for (int64_t e0 = 0; e0 < ne; e0 += per) {
      const int64_t e1 = e0 + per < ne ? e0 + per : ne;
      const unsigned nb = (unsigned)((e1 - e0 + 63) / 64);
#define GPAR_SREG(NP)                                                                           \
  score_reg<NP><<<nb, 64, 0, st>>>(F, S, p, ld_s, ld_r, ld_c, Y, ldy_r, ldy_c, e0, e1, sel, rec, \
                                   rec_off)
      if (S <= 16) GPAR_SREG(16);
      else if (S <= 32) GPAR_SREG(32);
      else GPAR_SREG(64);
#undef GPAR_SREG
      g_score_reg_launches.fetch_add(1, std::memory_order_relaxed);
    }
    return;
  }
  int NP2 = 1;
  while (NP2 < S) NP2 <<= 1;
  if (NP2 < 2) NP2 = 2;
  int G = kQuantLdsDoubles / NP2;
  if (G > kQuantLdsMaxG) G = kQuantLdsMaxG;
  const int64_t per = (int64_t)G << 24;
  for (int64_t e0 = 0; e0 < ne; e0 += per) {
    const int64_t e1 = e0 + per < ne ? e0 + per : ne;
    const unsigned nb = (unsigned)((e1 - e0 + G - 1) / G);
    score_lds<<<nb, 256, (size_t)G * NP2 * sizeof(double), st>>>(
        F, S, NP2, G, p, ld_s, ld_r, ld_c, Y, ldy_r, ldy_c, e0, e1, sel, rec, rec_off);
    g_score_lds_launches.fetch_add(1, std::memory_order_relaxed);
  }
}

void launch_score_gaussian(hipStream_t st, const double* M, int64_t ldm_r, int64_t ldm_c,
                           const double* Sd, int64_t lds_r, int64_t lds_c, const double* Y,
                           int64_t ldy_r, int64_t ldy_c, int64_t n, int64_t p, int nl,
                           const double* z, int bins, const ScoreRec& rec, int64_t rec_off) {
  GaussSel sel;
  sel.nl = nl;
  sel.bins = bins;
  for (int l = 0; l < kScoreMaxL; ++l) sel.z[l] = l < nl ? z[l] : 0.0;
  const int64_t ne = n * p, per = (int64_t)256 << 22;
  for (int64_t e0 = 0; e0 < ne; e0 += per) {
    const int64_t e1 = e0 + per < ne ? e0 + per : ne;
    score_gauss<<<(unsigned)((e1 - e0 + 255) / 256), 256, 0, st>>>(
        M, ldm_r, ldm_c, Sd, lds_r, lds_c, Y, ldy_r, ldy_c, p, e0, e1, sel, rec, rec_off);
  }
}

int64_t score_chunks_of(int64_t n) { return (n + kScoreChunk - 1) / kScoreChunk; }

void launch_score_reduce(hipStream_t st, const ScoreRec& rec, int64_t n, int64_t p, int nl,
                         int bins, double* pd, int32_t* pi, double* od, int64_t* oi) {
  const int64_t nchunks = score_chunks_of(n), nb = nchunks * p, per = (int64_t)1 << 30;
  const int ni = 3 + nl + bins;
  for (int64_t b0 = 0; b0 < nb; b0 += per) {
    const int64_t cnt = b0 + per < nb ? per : nb - b0;
    score_chunks<<<(unsigned)cnt, kScoreChunk, 0, st>>>(rec, n, p, nl, bins, b0, pd, pi);
  }
  const int64_t nt = p * (3 + ni);
  score_finish<<<(unsigned)((nt + 255) / 256), 256, 0, st>>>(pd, pi, nchunks, p, ni, od, oi);
}

void launch_score_export(hipStream_t st, const ScoreRec& rec, int64_t n, int64_t p,
                         const ScoreOut& out) {
  const int64_t ne = n * p, per = (int64_t)256 << 22;
  for (int64_t e0 = 0; e0 < ne; e0 += per) {
    const int64_t e1 = e0 + per < ne ? e0 + per : ne;
    score_export<<<(unsigned)((e1 - e0 + 255) / 256), 256, 0, st>>>(rec, p, e0, e1, out);
  }
}

}  // namespace gpar
