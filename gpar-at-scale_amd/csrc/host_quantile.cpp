// host_quantile.cpp -- gpar_sample_quantiles: quantiles over the sample axis of a strided sample
// tensor (k_quantile.hip).  Device tensors are read in place with no workspace; host tensors are
// staged through the context's workspace in blocks of entries of at most 256 MB.
#include "host.hpp"

#include <algorithm>
#include <cmath>

using namespace gpar;

// No two elements of a tensor of the given sizes and (positive) strides share an address: taken
// in order of their strides, every dimension of more than one element steps past the extent of
// the narrower ones (the check gpar_predict_samples makes of ld_s against (n_star - 1) ld_r + d)
bool gpar::strides_disjoint(const int64_t (&size)[3], const int64_t (&ld)[3]) {
  int ord[3] = {0, 1, 2};
  std::sort(ord, ord + 3, [&](int a, int b) { return ld[a] < ld[b]; });
  __int128 extent = 1;   // 1 + the largest offset over the dimensions seen so far
  for (int k : ord) {
    if (size[k] == 1) continue;
    if ((__int128)ld[k] < extent) return false;
    extent += (__int128)(size[k] - 1) * ld[k];
  }
  return extent <= ((__int128)1 << 60);
}

namespace {

constexpr int64_t kQuantStageBytes = (int64_t)256 << 20;   // most staged bytes of F per host block

// the launches of one tensor already on the device: kQuantMaxQ quantiles per launch
void run_quantiles(gpar_ctx* c, const double* f, int S, int64_t n, int64_t p, int64_t ld_s,
                   int64_t ld_r, int64_t ld_c, int nq, const int* lo, const double* g, double* out,
                   int64_t ldo_q, int64_t ldo_r, int64_t ldo_c) {
  for (int j0 = 0; j0 < nq; j0 += kQuantMaxQ) {
    const int cnt = std::min(kQuantMaxQ, nq - j0);
    Timed tm_(c, "quantile", 8.0 * (double)S * (double)n * (double)p);
    launch_quantiles(c->stream, f, S, n, p, ld_s, ld_r, ld_c, cnt, lo + j0, g + j0,
                     out + (int64_t)j0 * ldo_q, ldo_q, ldo_r, ldo_c);
    check_launch("sample quantiles");
  }
}

}  // namespace

extern "C" int32_t gpar_sample_quantiles(gpar_ctx* ctx, int32_t samples, int64_t n, int64_t p,
                                         const double* f, int64_t ld_s, int64_t ld_r, int64_t ld_c,
                                         int32_t nq, const double* q, int32_t mem, double* out,
                                         int64_t ldo_q, int64_t ldo_r, int64_t ldo_c) {
  API_BEGIN(ctx)
  ARGCHECK(f && q && out, "gpar_sample_quantiles: f, q and out must not be NULL");
  ARGCHECK(mem == GPAR_MEM_HOST || mem == GPAR_MEM_DEVICE,
           "gpar_sample_quantiles: mem must be GPAR_MEM_HOST or GPAR_MEM_DEVICE");
  ARGCHECK(samples >= 1 && n >= 1 && p >= 1 && nq >= 1,
           "gpar_sample_quantiles: samples, n, p and nq must be >= 1");
  ARGCHECK(n <= ((int64_t)1 << 40) && p <= ((int64_t)1 << 40) && n * p <= ((int64_t)1 << 40),
           "gpar_sample_quantiles: n p too large");
  for (int j = 0; j < nq; ++j)
    ARGCHECK(q[j] >= 0.0 && q[j] <= 1.0, "gpar_sample_quantiles: every q must be in [0, 1]");
  ARGCHECK(ld_s >= 1 && ld_r >= 1 && ld_c >= 1 && ldo_q >= 1 && ldo_r >= 1 && ldo_c >= 1,
           "gpar_sample_quantiles: strides must be positive");
  {
    const int64_t fs[3] = {samples, n, p}, fl[3] = {ld_s, ld_r, ld_c};
    const int64_t os[3] = {nq, n, p}, ol[3] = {ldo_q, ldo_r, ldo_c};
    ARGCHECK(strides_disjoint(fs, fl), "gpar_sample_quantiles: two entries of f share an address "
                                       "under these strides");
    ARGCHECK(strides_disjoint(os, ol), "gpar_sample_quantiles: two entries of out share an address "
                                       "under these strides");
  }
  if (samples > kQuantMaxS)
    throw Error(GPAR_ERR_UNSUPPORTED, "gpar_sample_quantiles: more than 4096 samples");
  const int S = samples;
  // h = q (S - 1), lo = floor(h), g = h - lo (numpy's virtual index and gamma)
  std::vector<int> lo(nq);
  std::vector<double> g(nq);
  for (int j = 0; j < nq; ++j) {
    const double h = q[j] * (double)(S - 1);
    double fl = std::floor(h);
    if (fl > (double)(S - 1)) fl = (double)(S - 1);
    lo[j] = (int)fl;
    g[j] = h - fl;
  }
  if (mem == GPAR_MEM_DEVICE) {
    run_quantiles(ctx, f, S, n, p, ld_s, ld_r, ld_c, nq, lo.data(), g.data(), out, ldo_q, ldo_r,
                  ldo_c);
    sync(ctx);
  } else {
    // blocks of consecutive entries e = i p + c, packed [s][k] on the host, results [j][k]
    const int64_t ne = n * p;
    const int64_t blk = std::min(ne, std::max<int64_t>(1, kQuantStageBytes / (8 * (int64_t)S)));
    double* df = ws<double>(ctx, "quant_f", (size_t)S * blk);
    double* dout = ws<double>(ctx, "quant_out", (size_t)nq * blk);
    std::vector<double> hf((size_t)S * blk), ho((size_t)nq * blk);
    for (int64_t e0 = 0; e0 < ne; e0 += blk) {
      const int64_t cnt = std::min(blk, ne - e0);
      for (int s = 0; s < S; ++s)
        for (int64_t k = 0; k < cnt; ++k) {
          const int64_t i = (e0 + k) / p, c = (e0 + k) % p;
          hf[(size_t)s * cnt + k] = f[s * ld_s + i * ld_r + c * ld_c];
        }
      h2d(ctx, df, hf.data(), (size_t)S * cnt);
      run_quantiles(ctx, df, S, cnt, 1, cnt, 1, 1, nq, lo.data(), g.data(), dout, cnt, 1, 1);
      d2h(ctx, ho.data(), dout, (size_t)nq * cnt);
      sync(ctx);
      for (int j = 0; j < nq; ++j)
        for (int64_t k = 0; k < cnt; ++k) {
          const int64_t i = (e0 + k) / p, c = (e0 + k) % p;
          out[j * ldo_q + i * ldo_r + c * ldo_c] = ho[(size_t)j * cnt + k];
        }
    }
  }
  API_END(ctx)
}
