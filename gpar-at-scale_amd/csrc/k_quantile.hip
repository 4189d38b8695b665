// k_quantile.hip -- per-entry quantiles over the sample axis of a strided sample tensor on gfx950
// (gpar_sample_quantiles): the credible bands of a sample chain, computed where the chain lives.
//
// Entry (i, c) of F[s * ld_s + i * ld_r + c * ld_c] (s < S, i < n, c < p) owns a list of S doubles.
// With x its ascending sort, quantile q is numpy's default ("linear", Hyndman-Fan type 7):
//   h = q (S - 1), lo = floor(h), g = h - lo, hi = min(lo + 1, S - 1), a = x[lo], b = x[hi],
//   a if g = 0 or a = b, else a + (b - a) g for g < 1/2 and b - (b - a) (1 - g) for g >= 1/2
// (numpy's _lerp; lo and g come from the host, FMA contraction is off in the interpolation).  A list
// that holds a NaN gives NaN for every q (the min / max exchanges drop NaNs, so the loads look for
// them); +-inf sort as values.
//
// Register path (S <= kQuantRegMax): one lane per entry, entries dealt to lanes in order, so with
// ld_c = 1 the 64 loads of a wave at one s are consecutive addresses.  The lane loads its list into
// NP registers (NP = 16, 32, 64, 128; +inf beyond S), every load independent of the others, so the
// whole list is in flight at once, sorts it with Batcher's odd-even mergesort as a fully unrolled
// compare-exchange network (v_min_f64 / v_max_f64; 63 / 191 / 543 / 1471 exchanges), and picks
// x[lo], x[hi] by an unrolled chain of selects on the uniform lo (a runtime index into the array
// would put it into scratch).  F is read once, 8 S n p bytes; nothing of that size is written.
//
// LDS path (S <= 4096): a 256-thread workgroup sorts G consecutive entries' lists, each padded with
// +inf to NP2 = the power of two >= S, G * NP2 <= 4096 doubles (32 KB), G <= 16, by a bitonic network in
// LDS; no atomics (the NaN flag of a list is a plain store of 1 by whoever meets one).
//
// An entry's result is a function of its S values and (lo, g) alone: both paths sort the same
// multiset with the same min / max and interpolate with the same function, so grids, strides and
// paths do not change a bit of it.
#include <cstdlib>
#include <cstring>
#include <utility>

#include "device_common.hpp"
#include "launch.hpp"
#include "nm_dev.hpp"
#include "sort_net.hpp"

namespace gpar {

std::atomic<int64_t> g_quantile_reg_launches{0}, g_quantile_lds_launches{0};

struct QuantSel {
  int nq;
  int lo[kQuantMaxQ];
  double g[kQuantMaxQ];
};

// ---------------------------------------------------------------------------- register path
// lane = entry e0 + blockIdx.x * 64 + threadIdx.x of the ne entries of this launch
template <int NP>
__global__ __launch_bounds__(64) void quantile_reg(const double* __restrict__ F, int S, int64_t p,
                                                   int64_t ld_s, int64_t ld_r, int64_t ld_c,
                                                   int64_t e0, int64_t e1, QuantSel sel,
                                                   double* __restrict__ out, int64_t ldo_q,
                                                   int64_t ldo_r, int64_t ldo_c) {
  const int64_t e = e0 + blockIdx.x * (int64_t)64 + threadIdx.x;
  if (e >= e1) return;
  const int64_t i = e / p, c = e - i * p;
  const double* f = F + i * ld_r + c * ld_c;
  double x[NP];
#pragma unroll
  for (int k = 0; k < NP; ++k) x[k] = k < S ? f[(int64_t)k * ld_s] : INFINITY;
  bool bad = false;
#pragma unroll
  for (int k = 0; k < NP; ++k) bad |= x[k] != x[k];
  oem_sort<NP>(x);
  double* o = out + i * ldo_r + c * ldo_c;
  for (int j = 0; j < sel.nq; ++j) {
    // a chain of selects on the uniform lo: a runtime index would put x into scratch, and so did
    // a search by scalar branches with a leaf per position
    const int lo = sel.lo[j], hi = lo + 1 < S ? lo + 1 : S - 1;
    double a = x[0], b = x[0];
#pragma unroll
    for (int k = 1; k < NP; ++k) {
      a = k == lo ? x[k] : a;
      b = k == hi ? x[k] : b;
    }
    const double v = quant_lerp(a, b, sel.g[j]);
    o[(int64_t)j * ldo_q] = bad ? __builtin_nan("") : v;
  }
}

// ---------------------------------------------------------------------------- LDS path
// workgroup = G consecutive entries from e0 + blockIdx.x * G; lists at sh[l * NP2 ...]
__global__ __launch_bounds__(256) void quantile_lds(const double* __restrict__ F, int S, int NP2,
                                                    int G, int64_t p, int64_t ld_s, int64_t ld_r,
                                                    int64_t ld_c, int64_t e0, int64_t e1,
                                                    QuantSel sel, double* __restrict__ out,
                                                    int64_t ldo_q, int64_t ldo_r, int64_t ldo_c) {
  extern __shared__ double sh[];
  __shared__ int bad[kQuantLdsMaxG];
  const int tid = threadIdx.x;
  const int64_t eb = e0 + blockIdx.x * (int64_t)G;
  if (tid < G) bad[tid] = 0;
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
  for (int idx = tid; idx < G * sel.nq; idx += 256) {
    const int l = idx % G, j = idx / G;
    const int64_t e = eb + l;
    if (e >= e1) continue;
    const int64_t i = e / p, c = e - i * p;
    const int lo = sel.lo[j], hi = lo + 1 < S ? lo + 1 : S - 1;
    const double v = quant_lerp(sh[l * NP2 + lo], sh[l * NP2 + hi], sel.g[j]);
    out[(int64_t)j * ldo_q + i * ldo_r + c * ldo_c] = bad[l] ? __builtin_nan("") : v;
  }
}

// ---------------------------------------------------------------------------- launcher
// GPAR_QUANTILE_PATH=reg / lds (tests): the register path at every S it can hold / the LDS path
// at every S
static int quantile_forced_path() {
  const char* e = std::getenv("GPAR_QUANTILE_PATH");
  if (!e) return 0;
  if (std::strcmp(e, "reg") == 0) return 1;
  if (std::strcmp(e, "lds") == 0) return 2;
  return 0;
}

void launch_quantiles(hipStream_t st, const double* F, int S, int64_t n, int64_t p, int64_t ld_s,
                      int64_t ld_r, int64_t ld_c, int nq, const int* lo, const double* g,
                      double* out, int64_t ldo_q, int64_t ldo_r, int64_t ldo_c) {
  QuantSel sel;
  sel.nq = nq;
  for (int j = 0; j < kQuantMaxQ; ++j) {
    sel.lo[j] = j < nq ? lo[j] : 0;
    sel.g[j] = j < nq ? g[j] : 0.0;
  }
  const int forced = quantile_forced_path();
  const bool reg = forced == 2 ? false : S <= kQuantRegMax;
  const int64_t ne = n * p;
  if (reg) {
    const int64_t per = (int64_t)64 << 24;   // entries per launch (2^24 blocks)
    for (int64_t e0 = 0; e0 < ne; e0 += per) {
      const int64_t e1 = e0 + per < ne ? e0 + per : ne;
      const unsigned nb = (unsigned)((e1 - e0 + 63) / 64);
#define GPAR_QREG(NP)                                                                          \
  quantile_reg<NP><<<nb, 64, 0, st>>>(F, S, p, ld_s, ld_r, ld_c, e0, e1, sel, out, ldo_q, ldo_r, \
                                      ldo_c)
      if (S <= 16) GPAR_QREG(16);
      else if (S <= 32) GPAR_QREG(32);
      else if (S <= 64) GPAR_QREG(64);
      else GPAR_QREG(128);
#undef GPAR_QREG
      g_quantile_reg_launches.fetch_add(1, std::memory_order_relaxed);
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
    quantile_lds<<<nb, 256, (size_t)G * NP2 * sizeof(double), st>>>(
        F, S, NP2, G, p, ld_s, ld_r, ld_c, e0, e1, sel, out, ldo_q, ldo_r, ldo_c);
    g_quantile_lds_launches.fetch_add(1, std::memory_order_relaxed);
  }
}

}  // namespace gpar
