// host_score.cpp -- gpar_score_samples / gpar_score_gaussian: scores of predictions against
// held-out targets (k_score.hip).  A per-entry pass writes packed records (entry (i, c) at i p + c)
// into the workspace, one reduction over all records gives the per-output aggregates, which are
// finished (means, coverage) on the host.  Device tensors are read in place; host tensors are
// staged in blocks of entries of at most 256 MB whose records land at the same indices, so the
// reduction -- and with it every bit of the result -- is the device call's.
#include "host.hpp"

#include <algorithm>
#include <cmath>
#include <limits>

using namespace gpar;

namespace {

constexpr int64_t kScoreStageBytes = (int64_t)256 << 20;   // most staged bytes per host block

bool plane_disjoint(int64_t n, int64_t p, int64_t ld_r, int64_t ld_c) {
  const int64_t size[3] = {1, n, p}, ld[3] = {1, ld_r, ld_c};
  return strides_disjoint(size, ld);
}

// z with P(|Z| <= z) = level for a standard normal Z: erfc(z / sqrt 2) = 1 - level, by bisection
// (erfc is monotone; 200 halvings of [0, 40] end at neighbouring doubles)
double normal_central_quantile(double level) {
  const double tail = 1.0 - level;
  double a = 0.0, b = 40.0;
  for (int it = 0; it < 200; ++it) {
    const double m = 0.5 * (a + b);
    if (std::erfc(m * 0.70710678118654752440) > tail) a = m;
    else b = m;
  }
  return 0.5 * (a + b);
}

struct ScoreArgs {
  int64_t n, p;
  int nl, bins;
  const double* levels;
  int mem;
};

void check_common(const char* who, const ScoreArgs& a, bool required_ptrs) {
  const std::string w(who);
  ARGCHECK(required_ptrs, w + ": a required pointer is NULL");
  ARGCHECK(a.mem == GPAR_MEM_HOST || a.mem == GPAR_MEM_DEVICE,
           w + ": mem must be GPAR_MEM_HOST or GPAR_MEM_DEVICE");
  ARGCHECK(a.n >= 1 && a.p >= 1, w + ": n and p must be >= 1");
  ARGCHECK(a.n <= ((int64_t)1 << 40) && a.p <= ((int64_t)1 << 28) &&
               a.n * a.p <= ((int64_t)1 << 40),
           w + ": n p too large");
  ARGCHECK(a.nl >= 1 && a.nl <= kScoreMaxL, w + ": nlevels must be in 1..8");
  ARGCHECK(a.bins >= 1 && a.bins <= kScoreMaxBins, w + ": bins must be in 1..64");
  for (int l = 0; l < a.nl; ++l)
    ARGCHECK(a.levels[l] > 0.0 && a.levels[l] < 1.0, w + ": every level must be in (0, 1)");
}

void check_plane(const char* who, const char* what, const void* ptr, bool optional, int64_t n,
                 int64_t p, int64_t ld_r, int64_t ld_c) {
  if (optional && !ptr) return;
  ARGCHECK(ld_r >= 1 && ld_c >= 1, std::string(who) + ": strides must be positive");
  ARGCHECK(plane_disjoint(n, p, ld_r, ld_c), std::string(who) + ": two entries of " + what +
                                                 " share an address under these strides");
}

struct ScoreBufs {
  ScoreRec rec;
  double *pd, *od;
  int32_t* pi;
  int64_t* oi;
  int ni;
};

// records and partials: gauss = the Gaussian scorer's (x1, x2 instead of below, equal)
ScoreBufs score_bufs(gpar_ctx* c, int64_t n, int64_t p, int nl, int bins, bool gauss) {
  ScoreBufs b{};
  const size_t ne = (size_t)n * p, nb = (size_t)score_chunks_of(n) * p;
  b.ni = 3 + nl + bins;
  b.rec.crps = ws<double>(c, "score_crps", ne);
  b.rec.flags = ws<uint32_t>(c, "score_flags", ne);
  if (gauss) {
    b.rec.x1 = ws<double>(c, "score_x1", ne);
    b.rec.x2 = ws<double>(c, "score_x2", ne);
  } else {
    b.rec.below = ws<int32_t>(c, "score_below", ne);
    b.rec.equal = ws<int32_t>(c, "score_equal", ne);
  }
  b.pd = ws<double>(c, "score_pd", nb * 3);
  b.pi = ws<int32_t>(c, "score_pi", nb * b.ni);
  b.od = ws<double>(c, "score_od", (size_t)p * 3);
  b.oi = ws<int64_t>(c, "score_oi", (size_t)p * b.ni);
  return b;
}

template <class T>
void scatter_host(gpar_ctx* c, const T* dev, int64_t n, int64_t p, T* out, int64_t ld_r,
                  int64_t ld_c) {
  if (!out) return;
  std::vector<T> h((size_t)n * p);
  d2h(c, h.data(), dev, h.size());
  sync(c);
  for (int64_t i = 0; i < n; ++i)
    for (int64_t k = 0; k < p; ++k) out[i * ld_r + k * ld_c] = h[(size_t)(i * p + k)];
}

// the reduction, the per-entry outputs and the aggregates of records already written
void finish_scores(gpar_ctx* c, const ScoreBufs& b, int64_t n, int64_t p, int nl, int bins,
                   int mem, const ScoreOut& out, double* crps, double* m1, double* m2,
                   double* coverage, int64_t* pit_hist, int64_t* scored, int64_t* missing,
                   int64_t* bad) {
  std::vector<double> hd((size_t)p * 3);
  std::vector<int64_t> hi((size_t)p * b.ni);
  {
    Timed tm_(c, "score_reduce", 20.0 * (double)n * (double)p);
    launch_score_reduce(c->stream, b.rec, n, p, nl, bins, b.pd, b.pi, b.od, b.oi);
    if (mem == GPAR_MEM_DEVICE && (out.crps || out.below || out.equal || out.x1 || out.x2))
      launch_score_export(c->stream, b.rec, n, p, out);
    check_launch("score reduction");
  }
  d2h(c, hd.data(), b.od, hd.size());
  d2h(c, hi.data(), b.oi, hi.size());
  sync(c);
  if (mem == GPAR_MEM_HOST) {
    scatter_host(c, b.rec.crps, n, p, out.crps, out.ldc_r, out.ldc_c);
    scatter_host(c, b.rec.below, n, p, out.below, out.ldb_r, out.ldb_c);
    scatter_host(c, b.rec.equal, n, p, out.equal, out.lde_r, out.lde_c);
    scatter_host(c, b.rec.x1, n, p, out.x1, out.ld1_r, out.ld1_c);
    scatter_host(c, b.rec.x2, n, p, out.x2, out.ld2_r, out.ld2_c);
  }
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (int64_t k = 0; k < p; ++k) {
    const int64_t* oi = hi.data() + k * b.ni;
    const double cnt = (double)oi[0];
    scored[k] = oi[0];
    missing[k] = oi[1];
    bad[k] = oi[2];
    crps[k] = oi[0] ? hd[k * 3] / cnt : nan;
    if (m1) m1[k] = oi[0] ? hd[k * 3 + 1] / cnt : nan;
    if (m2) m2[k] = oi[0] ? hd[k * 3 + 2] / cnt : nan;
    for (int l = 0; l < nl; ++l) coverage[l * p + k] = oi[0] ? (double)oi[3 + l] / cnt : nan;
    for (int j = 0; j < bins; ++j) pit_hist[j * p + k] = oi[3 + nl + j];
  }
}

}  // namespace

extern "C" int32_t gpar_score_samples(gpar_ctx* ctx, int32_t samples, int64_t n, int64_t p,
                                      const double* f, int64_t ld_s, int64_t ld_r, int64_t ld_c,
                                      const double* y, int64_t ldy_r, int64_t ldy_c,
                                      int32_t nlevels, const double* levels, int32_t bins,
                                      int32_t mem, double* crps_e, int64_t ldc_r, int64_t ldc_c,
                                      int32_t* below_e, int64_t ldb_r, int64_t ldb_c,
                                      int32_t* equal_e, int64_t lde_r, int64_t lde_c, double* crps,
                                      double* coverage, int64_t* pit_hist, int64_t* scored,
                                      int64_t* missing, int64_t* bad) {
  API_BEGIN(ctx)
  const char* who = "gpar_score_samples";
  check_common(who, {n, p, nlevels, bins, levels, mem},
               f && y && levels && crps && coverage && pit_hist && scored && missing && bad);
  ARGCHECK(samples >= 1, "gpar_score_samples: samples must be >= 1");
  ARGCHECK(ld_s >= 1 && ld_r >= 1 && ld_c >= 1, "gpar_score_samples: strides must be positive");
  {
    const int64_t fs[3] = {samples, n, p}, fl[3] = {ld_s, ld_r, ld_c};
    ARGCHECK(strides_disjoint(fs, fl), "gpar_score_samples: two entries of f share an address "
                                       "under these strides");
  }
  check_plane(who, "y", y, false, n, p, ldy_r, ldy_c);
  check_plane(who, "crps_e", crps_e, true, n, p, ldc_r, ldc_c);
  check_plane(who, "below_e", below_e, true, n, p, ldb_r, ldb_c);
  check_plane(who, "equal_e", equal_e, true, n, p, lde_r, lde_c);
  if (samples > kQuantMaxS)
    throw Error(GPAR_ERR_UNSUPPORTED, "gpar_score_samples: more than 4096 samples");
  const int S = samples;
  // the two quantiles of each level as gpar_sample_quantiles takes them: h = q (S - 1),
  // lo = floor(h), g = h - lo
  int lo[2 * kScoreMaxL];
  double g[2 * kScoreMaxL];
  for (int l = 0; l < nlevels; ++l)
    for (int side = 0; side < 2; ++side) {
      const double q = side ? (1.0 + levels[l]) / 2.0 : (1.0 - levels[l]) / 2.0;
      const double h = q * (double)(S - 1);
      double fl = std::floor(h);
      if (fl > (double)(S - 1)) fl = (double)(S - 1);
      lo[2 * l + side] = (int)fl;
      g[2 * l + side] = h - fl;
    }
  const ScoreBufs b = score_bufs(ctx, n, p, nlevels, bins, false);
  if (mem == GPAR_MEM_DEVICE) {
    Timed tm_(ctx, "score", 8.0 * (double)S * (double)n * (double)p);
    launch_score_samples(ctx->stream, f, S, n, p, ld_s, ld_r, ld_c, y, ldy_r, ldy_c, nlevels, lo,
                         g, bins, b.rec, 0);
    check_launch("sample scores");
  } else {
    // blocks of consecutive entries e = i p + c, packed [s][k] with their targets [k]
    const int64_t ne = n * p;
    const int64_t blk = std::min(ne, std::max<int64_t>(1, kScoreStageBytes / (8 * (int64_t)S)));
    double* df = ws<double>(ctx, "score_f", (size_t)S * blk);
    double* dy = ws<double>(ctx, "score_y", (size_t)blk);
    std::vector<double> hf((size_t)S * blk), hy((size_t)blk);
    for (int64_t e0 = 0; e0 < ne; e0 += blk) {
      const int64_t cnt = std::min(blk, ne - e0);
      for (int64_t k = 0; k < cnt; ++k) {
        const int64_t i = (e0 + k) / p, c = (e0 + k) % p;
        hy[(size_t)k] = y[i * ldy_r + c * ldy_c];
        for (int s = 0; s < S; ++s) hf[(size_t)s * cnt + k] = f[s * ld_s + i * ld_r + c * ld_c];
      }
      h2d(ctx, df, hf.data(), (size_t)S * cnt);
      h2d(ctx, dy, hy.data(), (size_t)cnt);
      {
        Timed tm_(ctx, "score", 8.0 * (double)S * (double)cnt);
        launch_score_samples(ctx->stream, df, S, cnt, 1, cnt, 1, 1, dy, 1, 1, nlevels, lo, g, bins,
                             b.rec, e0);
        check_launch("sample scores");
      }
      sync(ctx);   // the staging vectors are refilled
    }
  }
  ScoreOut out{};
  out.crps = crps_e, out.ldc_r = ldc_r, out.ldc_c = ldc_c;
  out.below = below_e, out.ldb_r = ldb_r, out.ldb_c = ldb_c;
  out.equal = equal_e, out.lde_r = lde_r, out.lde_c = lde_c;
  finish_scores(ctx, b, n, p, nlevels, bins, mem, out, crps, nullptr, nullptr, coverage, pit_hist,
                scored, missing, bad);
  API_END(ctx)
}

extern "C" int32_t gpar_score_gaussian(gpar_ctx* ctx, int64_t n, int64_t p, const double* mean,
                                       int64_t ldm_r, int64_t ldm_c, const double* std_,
                                       int64_t lds_r, int64_t lds_c, const double* y, int64_t ldy_r,
                                       int64_t ldy_c, int32_t nlevels, const double* levels,
                                       int32_t bins, int32_t mem, double* crps_e, int64_t ldc_r,
                                       int64_t ldc_c, double* logdens_e, int64_t ldl_r,
                                       int64_t ldl_c, double* sqerr_e, int64_t ldq_r, int64_t ldq_c,
                                       double* crps, double* log_density, double* mse,
                                       double* coverage, int64_t* pit_hist, int64_t* scored,
                                       int64_t* missing, int64_t* bad) {
  API_BEGIN(ctx)
  const char* who = "gpar_score_gaussian";
  check_common(who, {n, p, nlevels, bins, levels, mem},
               mean && std_ && y && levels && crps && log_density && mse && coverage && pit_hist &&
                   scored && missing && bad);
  check_plane(who, "mean", mean, false, n, p, ldm_r, ldm_c);
  check_plane(who, "std", std_, false, n, p, lds_r, lds_c);
  check_plane(who, "y", y, false, n, p, ldy_r, ldy_c);
  check_plane(who, "crps_e", crps_e, true, n, p, ldc_r, ldc_c);
  check_plane(who, "logdens_e", logdens_e, true, n, p, ldl_r, ldl_c);
  check_plane(who, "sqerr_e", sqerr_e, true, n, p, ldq_r, ldq_c);
  double z[kScoreMaxL];
  for (int l = 0; l < nlevels; ++l) z[l] = normal_central_quantile(levels[l]);
  const ScoreBufs b = score_bufs(ctx, n, p, nlevels, bins, true);
  const int64_t ne = n * p;
  if (mem == GPAR_MEM_DEVICE) {
    Timed tm_(ctx, "score_gauss", 24.0 * (double)ne);
    launch_score_gaussian(ctx->stream, mean, ldm_r, ldm_c, std_, lds_r, lds_c, y, ldy_r, ldy_c, n,
                          p, nlevels, z, bins, b.rec, 0);
    check_launch("gaussian scores");
  } else {
    const int64_t blk = std::min(ne, std::max<int64_t>(1, kScoreStageBytes / 24));
    double* d3 = ws<double>(ctx, "score_f", (size_t)3 * blk);
    std::vector<double> h3((size_t)3 * blk);
    for (int64_t e0 = 0; e0 < ne; e0 += blk) {
      const int64_t cnt = std::min(blk, ne - e0);
      for (int64_t k = 0; k < cnt; ++k) {
        const int64_t i = (e0 + k) / p, c = (e0 + k) % p;
        h3[(size_t)k] = mean[i * ldm_r + c * ldm_c];
        h3[(size_t)(cnt + k)] = std_[i * lds_r + c * lds_c];
        h3[(size_t)(2 * cnt + k)] = y[i * ldy_r + c * ldy_c];
      }
      h2d(ctx, d3, h3.data(), (size_t)3 * cnt);
      {
        Timed tm_(ctx, "score_gauss", 24.0 * (double)cnt);
        launch_score_gaussian(ctx->stream, d3, 1, 1, d3 + cnt, 1, 1, d3 + 2 * cnt, 1, 1, cnt, 1,
                              nlevels, z, bins, b.rec, e0);
        check_launch("gaussian scores");
      }
      sync(ctx);
    }
  }
  ScoreOut out{};
  out.crps = crps_e, out.ldc_r = ldc_r, out.ldc_c = ldc_c;
  out.x1 = logdens_e, out.ld1_r = ldl_r, out.ld1_c = ldl_c;
  out.x2 = sqerr_e, out.ld2_r = ldq_r, out.ld2_c = ldq_c;
  finish_scores(ctx, b, n, p, nlevels, bins, mem, out, crps, log_density, mse, coverage, pit_hist,
                scored, missing, bad);
  API_END(ctx)
}
