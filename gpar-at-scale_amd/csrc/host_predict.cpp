// host_predict.cpp -- the prediction stages (test inputs, merged grid, gains, the Sigma^{-1} solve,
// delivery), the prediction modes built from them (analytic, MC, posterior paths, paths with
// per-sample test inputs, mean only), their workspace estimates and the single-output C-ABI entries.
#include "host.hpp"

namespace gpar {

// --------------------------------------------------------------------------- stages
std::vector<int64_t> ascending_perm(const double* t, int64_t n) {
  std::vector<int64_t> perm;
  if (std::is_sorted(t, t + n)) return perm;
  perm.resize(n);
  for (int64_t i = 0; i < n; ++i) perm[i] = i;
  std::stable_sort(perm.begin(), perm.end(), [&](int64_t a, int64_t b) { return t[a] < t[b]; });
  return perm;
}

void deliver(gpar_ctx* c, int mem, const std::vector<int64_t>& perm, bool defer, int64_t n,
             std::initializer_list<Delivery> vecs, int64_t rows) {
  const size_t len = (size_t)rows * n;
  if (mem == GPAR_MEM_DEVICE) {
    for (const Delivery& v : vecs)
      HIPCHECK(hipMemcpyAsync(v.dst, v.src, len * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    if (!defer) sync(c);
  } else if (perm.empty()) {   // t* was ascending: straight into the caller's buffers
    for (const Delivery& v : vecs) d2h(c, v.dst, v.src, len);
    if (!defer) sync(c);
  } else {
    std::vector<double> h(vecs.size() * len);
    size_t k = 0;
    for (const Delivery& v : vecs) d2h(c, h.data() + k++ * len, v.src, len);
    sync(c);
    k = 0;
    for (const Delivery& v : vecs) {
      const double* src = h.data() + k++ * len;
      for (int64_t b = 0; b < rows; ++b)
        for (int64_t i = 0; i < n; ++i) v.dst[b * n + perm[i]] = src[b * n + i];
    }
  }
}

// A prediction's test inputs on the device, ascending: host inputs are stably sorted here (perm:
// ascending_perm; the caller un-permutes its outputs); device inputs must already be ascending
// and pass through.
struct TestInputs {
  const double *ts, *vs;
  int64_t ldv;
  std::vector<int64_t> perm;
};
static TestInputs stage_test_inputs(gpar_ctx* c, int mem, int64_t n_star, int64_t d,
                                    const double* t_star_in, const double* v_star_in,
                                    int64_t ldvs) {
  TestInputs ti{t_star_in, v_star_in, ldvs, {}};
  if (mem != GPAR_MEM_HOST) return ti;
  std::vector<int64_t>& perm = ti.perm;
  double* dts = ws<double>(c, "pr_ts", n_star);
  double* dvs = ws<double>(c, "pr_vs", (size_t)n_star * d);
  perm = ascending_perm(t_star_in, n_star);
  if (perm.empty()) {
    h2d(c, dts, t_star_in, n_star);
    if (d > 0) h2d_rows(c, dvs, v_star_in, ldvs, d, n_star);   // (0: no column every sample shares)
  } else {
    std::vector<double> tsh(n_star), vsh((size_t)n_star * d);
    for (int64_t i = 0; i < n_star; ++i) {
      tsh[i] = t_star_in[perm[i]];
      for (int64_t q = 0; q < d; ++q) vsh[i * d + q] = v_star_in[perm[i] * ldvs + q];
    }
    h2d(c, dts, tsh.data(), n_star);
    h2d(c, dvs, vsh.data(), (size_t)n_star * d);
  }
  sync(c);
  ti.ts = dts;
  ti.vs = dvs;
  ti.ldv = d;
  return ti;
}

MergedGrid merge_grid(gpar_ctx* c, const std::string& tag, const DevProblem& P, double s2,
                      const double* ts, int64_t n_star, const double* ycol, const double* vs,
                      int64_t ldvs, bool want_inputs, bool want_pos, const char* yname,
                      bool want_tpos) {
  MergedGrid g{};
  const int64_t n = P.n, d = want_inputs ? P.d : 0;
  g.nt = n + n_star;
  g.nch = (g.nt + kChunk - 1) / kChunk;
  g.tm = ws<double>(c, tag + "_tm", g.nt);
  g.ym = ws<double>(c, tag + yname, g.nt);
  g.rm = ws<double>(c, tag + "_rm", g.nt);
  if (want_inputs) g.vm = ws<double>(c, tag + "_vm", (size_t)g.nt * d);
  if (want_pos) g.pos = ws<int64_t>(c, tag + "_pos", n_star);
  if (want_tpos) g.tpos = ws<int64_t>(c, tag + "_tpos", n);
  launch_merge_side(c->stream, P.t, n, ts, n_star, 0, ycol, s2, want_inputs ? P.v : nullptr,
                    want_inputs ? P.ldv : 0, (int)d, g.tm, g.ym, g.rm, g.vm, d, g.tpos);
  launch_merge_side(c->stream, ts, n_star, P.t, n, 1, nullptr, 1e10, want_inputs ? vs : nullptr,
                    want_inputs ? ldvs : 0, (int)d, g.tm, g.ym, g.rm, g.vm, d, g.pos);
  return g;
}

GridGains grid_gains(gpar_ctx* c, int sdim, const ChainParamsHost& cp, const MergedGrid& grid,
                     const PredPrep* prep, const std::string& tag) {
  if (prep) {   // computed ahead on the side stream (gpar_posterior_prepare)
    HIPCHECK(hipStreamWaitEvent(c->stream, c->ev_prep_ready[prep - c->prep.data()], 0));
    return prep->gg;
  }
  GridGains gg;
  gg.g = run_gains(c, sdim, grid.tm, grid.nt, {cp}, grid.rm, false, tag);
  return gg;
}

double* fixup_rows(gpar_ctx* c, int sdim, GridGains& gg, int64_t n, int64_t nch,
                   const std::string& name) {
  if (!gg.h) {
    gg.h = ws<double>(c, name, (size_t)n * 4);   // kGStride
    launch_gains_adjoint(c->stream, sdim, gg.g.rec, n, kChunk, nch, 1, gg.h);
  }
  return gg.h;
}

void release_prep(gpar_ctx* c, const PredPrep* prep) {
  if (prep) HIPCHECK(hipEventRecord(c->ev_prep_free[prep - c->prep.data()], c->stream));
}

SigmaCols sigma_cols(gpar_ctx* c, const std::string& tag, double* X, int64_t ldx, int64_t mc,
                     int64_t n, bool wide, const double* wmask) {
  SigmaCols s{X, ldx, mc, n, (n + kChunk - 1) / kChunk, wide, wmask, nullptr, nullptr, nullptr, nullptr};
  const size_t cs = (size_t)s.nch * mc * kSStride;
  s.send = ws<double>(c, tag + "_send", cs);
  s.cin = ws<double>(c, tag + "_cin", cs);
  s.bend = ws<double>(c, tag + "_bend", cs);
  s.chat = ws<double>(c, tag + "_chat", cs);
  return s;
}

double* sigma_inv_columns(gpar_ctx* c, int sdim, GridGains gg, const SigmaCols& s,
                          const std::string& ws_tag, const std::string& run_tag, const char* span,
                          double work) {
  const GainsOut& g = gg.g;
  run_carry(c, sdim, g.phi, 0, s.send, s.cin, 0, s.nch, s.mc, s.mc, 1, run_tag + "f");
  double* h = fixup_rows(c, sdim, gg, s.n, s.nch, ws_tag + "_h");
  {
    std::optional<Timed> tm_;
    if (span) tm_.emplace(c, span, work);
    if (s.wide)
      launch_adjoint_local_wide(c->stream, sdim, s.X, s.ldx, s.mc, g.rec, g.g, s.cin, s.mc, s.n,
                                kChunk, s.nch, s.bend, s.wmask);
    else
      launch_adjoint_local(c->stream, sdim, s.X, s.ldx, s.mc, g.rec, g.g, s.cin, s.mc, s.n, kChunk,
                           s.nch, s.bend);
  }
  run_carry(c, sdim, g.phi, 0, s.bend, s.chat, 0, s.nch, s.mc, s.mc, 1, run_tag + "b", /*rev=*/true);
  return h;
}

// --------------------------------------------------------------------------- posterior paths
// S joint posterior samples of the latent f along one LGSSM chain (TemporalGPs posterior_rand,
// tmp.jl:161-167) with the simulation smoother (k_path.hip): gains g of the chain over the n steps
// of the grid t (params cp, observation noise `noise` per step or cp.r), data v_{k,s} = ym[k] - fx[k * ldfx + s]
// (fx null: ym[k] for every sample).  Samples -> F[k * S + s].
void path_samples(gpar_ctx* c, int sdim, const GainsOut& g, const ChainParamsHost& cp,
                  const double* t, const double* noise, int64_t n, const double* ym,
                  const double* fx, int64_t ldfx, int S, uint64_t seed, double* F) {
  const int64_t nch = (n + kChunk - 1) / kChunk;
  const size_t cs = (size_t)nch * S * kSStride;
  double* lq = ws<double>(c, "path_lq", (size_t)n * sdim * sdim);
  double* phia = ws<double>(c, "path_phia", (size_t)nch * sdim * sdim);
  double* z = ws<double>(c, "path_z", (size_t)S * n);
  double* X = ws<double>(c, "path_X", (size_t)n * S);
  double* sp_ = ws<double>(c, "path_sp", cs);
  double* cp_ = ws<double>(c, "path_cp", cs);
  const SigmaCols cols = sigma_cols(c, "path", X, S, S, n, /*wide=*/true, nullptr);
  const uint64_t ps = path_seed(seed);
  Timed tm_(c, "path");
  // prior paths: local pass, carry with the chunk transfers prod A_k, final pass (x~[0] -> F,
  // the data columns v - y~ -> z)
  launch_dk_consts(c->stream, sdim, t, n, cp.inv_l, cp.s, lq);
  launch_dk_phi(c->stream, sdim, g.rec, n, kChunk, nch, phia);
  launch_dk_prior(c->stream, sdim, g.rec, lq, noise, cp.r, n, kChunk, nch, S, ps, ym, fx, ldfx,
                  nullptr, sp_, nullptr, nullptr);
  run_carry(c, sdim, phia, 0, sp_, cp_, 0, nch, S, S, 1, "pathp");
  launch_dk_prior(c->stream, sdim, g.rec, lq, noise, cp.r, n, kChunk, nch, S, ps, ym, fx, ldfx,
                  cp_, nullptr, F, z);
  // smoother mean of the S columns (shared gains): whitening into X (column s), then the
  // prediction's Sigma^{-1} solve, then F += v - R Sigma^{-1} v
  launch_whiten_vec(c->stream, sdim, g.rec, 0, z, n, n, kChunk, nch, S, X, 1, cols.send, kSStride,
                    S, 0, /*astride=*/S);
  GridGains gg;   // the fix-up rows are the path's own, whoever computed the gains
  gg.g = g;
  const double* h = sigma_inv_columns(c, sdim, gg, cols, "path", "path");
  launch_dk_finish(c->stream, sdim, X, S, h, cols.chat, z, noise, cp.r, n, kChunk, nch, S, F);
  check_launch("path samples");
}

// --------------------------------------------------------------------------- prediction
struct MeanStd {   // the device vectors a mode's tail left the mean and the std in
  const double *mean, *std;
};
// q(u) draws as Distributions samples q_u = MvNormal(m_e, Symmetric(inv(D)))
// (gpar_scaled_inference.jl:103,185): m_e + Lc xi with Lc = chol(inv(D)) lower, so a given xi
// (gpar_mc_normals) gives the reference's sample; W = Lc^T L_u^{-1} carries it through U_u^{-1}.
struct McFactor {
  double* W;
  int* status;   // the Cholesky's flag, read by check() once the mode's launches are queued
  void check(gpar_ctx* c) const {
    int st = 0;
    d2h(c, &st, status, 1);
    sync(c);
    if (st) throw Error(GPAR_ERR_NOT_PD, "PosDefException: cholesky(Symmetric(inv(D))) failed (MvNormal, gpar_scaled_inference.jl:185)");
  }
};

// One prediction: what its stages share (the problem, q(u)'s factors, the merged grid and its
// gains, the result vectors) and the stages after the gains, mode by mode.
struct Pred {
  gpar_ctx* c;
  const DevProblem& P;
  const Theta& th;
  int64_t n_star;
  int samples;
  uint64_t seed;
  QuPre q;
  MergedGrid grid;
  ChainParamsHost cp;
  GridGains gg;
  double *mean, *std;   // n* each
  // ANALYTIC / MC: the whitened columns' Sigma^{-1} solve (solve_kfu_columns)
  SigmaCols cols;
  const double* h;

  McFactor mc_factor() const {
    const int64_t ld = q.ld;
    double* Lc = ws<double>(c, "pr_Lc", (size_t)ld * ld);
    double* Tdc = ws<double>(c, "pr_Tdc", (size_t)q.nb * kDenseNB * kDenseNB);
    int* stc = ws<int>(c, "pr_stc", 1);
    HIPCHECK(hipMemsetAsync(stc, 0, sizeof(int), c->stream));
    launch_pad_identity_copy(c->stream, q.cov, ld, (int)P.m, Lc);
    CholJob2Host cj{Lc, nullptr, Tdc, stc};
    auto* dcj = ws<CholJob2Host>(c, "pr_cholc", 1);
    h2d(c, dcj, &cj, 1);
    launch_chol_blocked(c->stream, dcj, 1, ld, q.nb, /*want_t=*/false);
    double* W = ws<double>(c, "pr_W", (size_t)ld * ld);
    launch_mc_factor(c->stream, Lc, q.X1, ld, (int)P.m, W);
    check_launch("predict: MC factor");
    return {W, stc};
  }

  // PATH (tmp.jl:119-167): per sample, fx_s = Cf*u U_u^{-1} e_s (e_s ~ q(u)) on the merged grid, then a
  // posterior path of the time GP given y* - fx_s (simulation smoother, path_samples), f*_s = fx_s + f_t,s
  MeanStd path_tail() const {
    const McFactor f = mc_factor();
    const double* Bm = sample_loadings(f);
    double* FX = ws<double>(c, "pr_FX", (size_t)grid.nt * samples);
    shared_input_fx(grid.vm, P.d, grid.nt, Bm, FX);
    check_launch("predict: path fx");
    path_draws(FX);
    f.check(c);
    return {mean, std};
  }

  // the pseudo-point samples' loadings Bm (samples x mp): U_u^{-1} (m_e + Lc xi_s), xi = gpar_mc_normals
  const double* sample_loadings(const McFactor& f) const {
    const int64_t m = P.m, mp = P.mp;
    double* xi = ws<double>(c, "pr_xi", (size_t)samples * mp);
    launch_normal(c->stream, xi, mp, samples, m, samples, seed);
    double* Bm = ws<double>(c, "pr_Bm", (size_t)samples * mp);
    launch_path_bmat(c->stream, f.W, q.ld, q.w, xi, mp, samples, (int)m, mp, Bm, mp);
    return Bm;
  }

  // fx (rows x samples, packed) = Cf*u Bm^T at `rows` inputs every sample shares: Cf*u stored
  void shared_input_fx(const double* v, int64_t ldv, int64_t rows, const double* Bm,
                       double* fx) const {
    const int64_t m = P.m, d = P.d, mp = P.mp;
    double* Ks = ws<double>(c, "pr_Ks", (size_t)rows * mp);   // Cf*u (gpar_scaled_inference.jl:89)
    launch_dist2(c->stream, P.ok, v, ldv, rows, P.z, P.ldz, m, mp, (int)d, P.zc, Ks, mp,
                 /*take_sqrt=*/P.ok != GPAR_EQ);
    launch_kfu_from_dist(c->stream, P.ok, Ks, rows, m, mp, 1.0 / th.l_o, th.sv_o * th.sv_o);
    // fx only: no row sums (mode 0 writes them per 128-column block when asked)
    launch_gemm_nt(c->stream, Ks, mp, Bm, mp, rows, samples, m, 0, fx, samples, nullptr, 0, nullptr,
                   nullptr, nullptr, 0);
  }

  // the posterior paths given y* - FX and their statistics at the test rows; returns F
  const double* path_draws(const double* FX) const {
    double* F = ws<double>(c, "pr_F", (size_t)grid.nt * samples);
    path_samples(c, P.sdim, gg.g, cp, grid.tm, grid.rm, grid.nt, grid.ym, FX, samples, samples, seed,
                 F);
    launch_path_stats(c->stream, FX, samples, F, samples, grid.pos, n_star, mean, std);
    check_launch("predict: path stats");
    return F;
  }

  // SAMPLES: FX when every sample has its own test inputs.  The training rows use the shared
  // training inputs (shared_input_fx over the n training rows alone, scattered to their merged
  // rows); the test rows come from launch_kfu_samples, which stores no kernel matrix.
  double* per_sample_fx(const TestInputs& ti, int64_t d_sh, const double* vsa, int64_t ld_s,
                        int64_t ld_r, const int64_t* dperm, const double* Bm) const {
    const int64_t d_sa = P.d - d_sh;
    double* FX = ws<double>(c, "pr_FX", (size_t)grid.nt * samples);
    double* fxtr = ws<double>(c, "ps_fxtr", (size_t)P.n * samples);
    shared_input_fx(P.v, P.ldv, P.n, Bm, fxtr);
    launch_scatter_rows(c->stream, fxtr, P.n, samples, grid.tpos, FX, samples);
    {   // flops of the distance contractions; the samples * n* * m kernel evaluations come on top
      Timed tm_(c, "pred_sfx", 2.0 * (double)samples * (double)n_star * (double)P.m * (double)P.d);
      launch_kfu_samples(c->stream, P.ok, ti.vs, ti.ldv, (int)d_sh, vsa, ld_s, ld_r, (int)d_sa, dperm,
                         n_star, samples, P.z, P.ldz, P.m, P.zc, Bm, P.mp, 1.0 / th.l_o,
                         th.sv_o * th.sv_o, grid.pos, FX, samples);
    }
    check_launch("predict samples: fx");
    return FX;
  }

  // ANALYTIC / MC, first half: the Cf*u columns (on the fly) and y* whitened into X, and
  // Sigma^{-1} of them; u is read back only at the test rows, where rm = 1e10.
  void solve_kfu_columns() {
    const int64_t m = P.m, d = P.d, mp = P.mp, mc = P.mc, nt = grid.nt;
    const int64_t ldx = mp + 64;
    double* X = ws<double>(c, "pr_X", (size_t)nt * ldx);
    cols = sigma_cols(c, "pr", X, ldx, mc, nt, /*wide=*/true, grid.rm);
    {   // algorithmic HBM bytes: merged inputs V* (d) read, gains records + fix-up rows (20), the
        // m whitened Cf*u columns written, per merged row
      Timed tm_(c, "pred_whiten", 8.0 * (double)nt * ((double)d + (double)m + 20.0));
      whiten_kfu_any(c, P, gg.g, grid.vm, d, nt, grid.nch, th, X, ldx, cols.send, nullptr);
      launch_whiten_vec(c->stream, P.sdim, gg.g.rec, 0, grid.ym, 0, nt, kChunk, grid.nch, 1, X + mp, 0,
                        cols.send, 0, mc, mp, ldx);
    }
    check_launch("predict: whiten");
    // pred_adjoint bytes: the mc whitened columns read per merged row, records + fix-up rows + R
    // (21), u written at the test rows
    h = sigma_inv_columns(c, P.sdim, gg, cols, "pr", "pred", "pred_adjoint",
                          8.0 * ((double)nt * ((double)mc + 21.0) + (double)n_star * (double)mc));
    check_launch("predict: adjoint");
  }

  // ANALYTIC with m <= 512 (predict_var_tiles): rows, mean and |Q_i V^T| in one pass, Q never stored
  MeanStd fused_var_tail() const {
    {   // flops of |Q_i V^T|^2 with V lower triangular, as pred_gemm
      Timed tm_(c, "pred_var", (double)n_star * (double)P.m * (double)(P.m + 1));
      launch_predict_var(c->stream, P.sdim, cols.X, cols.ldx, h, cols.chat, P.mc, P.mp, P.m, kChunk,
                         grid.pos, n_star, grid.rm, grid.ym, q.w, q.Vm, q.ld, mean, std);
    }
    check_launch("predict: rows + variance");
    return {mean, std};
  }

  // per test row: Q = R Sigma^{-1} Cf*u (n* x mp), and the mean
  double* rows() const {
    double* Q = ws<double>(c, "pr_Q", (size_t)n_star * P.mp);
    {   // bytes: u rows at the test points read, Q rows written (mp each)
      Timed tm_(c, "pred_rows", 16.0 * (double)n_star * (double)P.mp);
      launch_predict_rows(c->stream, P.sdim, cols.X, cols.ldx, h, cols.chat, P.mc, P.mp, P.m, kChunk,
                          grid.pos, n_star, grid.rm, grid.ym, q.w, Q, P.mp, mean);
    }
    check_launch("predict: rows");
    return Q;
  }

  // ANALYTIC, unfused: Z = Q V^T, std = |Z_i|
  MeanStd gemm_var_tail(const double* Q) const {
    const int64_t m = P.m;
    const int ncb = (int)((m + 127) / 128);
    double* rowsq = ws<double>(c, "pr_rowsq", (size_t)ncb * n_star);
    {   // flops of |Q_i V^T|^2 with V lower triangular: 2 n* sum_c (c + 1) = n* m (m + 1)
      Timed tm_(c, "pred_gemm", (double)n_star * (double)m * (double)(m + 1));
      launch_gemm_nt(c->stream, Q, P.mp, q.Vm, q.ld, n_star, m, m, 0, nullptr, 0, rowsq, 0, nullptr,
                     nullptr, nullptr, /*tri=*/1);
    }
    launch_rowsq_finish(c->stream, rowsq, n_star, ncb, std);
    check_launch("predict: gemm");
    return {mean, std};
  }

  // MC: f_s = mean + (I - S) K* U_u^{-1} Lc xi_s = mean + Z xi_s, mean / std over the samples
  MeanStd mc_tail(const double* Q) const {
    const int64_t m = P.m, mp = P.mp;
    const int ncb = (int)((m + 127) / 128);
    const McFactor f = mc_factor();
    double* Z = ws<double>(c, "pr_Z", (size_t)n_star * mp);
    double* rowsq = ws<double>(c, "pr_rowsq", (size_t)ncb * n_star);
    double* xi = ws<double>(c, "pr_xi", (size_t)samples * mp);
    double* mmc = ws<double>(c, "pr_mmc", n_star);
    launch_gemm_nt(c->stream, Q, mp, f.W, q.ld, n_star, m, m, 0, Z, mp, rowsq, 0, nullptr, nullptr,
                   nullptr, /*tri=*/0);
    launch_normal(c->stream, xi, mp, samples, m, samples, seed);
    if (samples <= 128) {   // one column tile: statistics in the GEMM epilogue
      launch_gemm_nt(c->stream, Z, mp, xi, mp, n_star, samples, m, 1, nullptr, 0, nullptr, samples,
                     mean, mmc, std);
    } else {
      const int nsb = (int)((samples + 127) / 128);
      double* part = ws<double>(c, "pr_mcpart", (size_t)nsb * n_star * 2);
      launch_gemm_nt(c->stream, Z, mp, xi, mp, n_star, samples, m, 2, nullptr, 0, part, 0, nullptr,
                     nullptr, nullptr);
      launch_mc_stats_finish(c->stream, part, n_star, nsb, samples, mean, mmc, std);
    }
    f.check(c);
    check_launch("predict: gemm");
    return {mmc, std};
  }
};

// Prediction half of get_gpar_scaled_predictions (gpar_scaled_inference.jl:63-135); see the
// header of k_predict.hip for the algebra.
void predict_impl(gpar_ctx* c, const DevProblem& P, const Theta& th, int mem, int64_t n_star,
                  const double* t_star_in, const double* v_star_in, int64_t ldvs, int mode,
                  int samples, uint64_t seed, double* mean_out, double* std_out,
                  const GramCache* gc, bool defer, const QuPre* pre, const PredPrep* prep) {
  if (mode == GPAR_PREDICT_PATH)   // path draw (s, k, i): counter index k (sdim + 1) + i, 32 bits
    ARGCHECK((P.n + n_star) * (P.sdim + 1) <= ((int64_t)1 << 32),
             "path mode: (n + n_star) * (state dimension + 1) must be <= 2^32");
  const TestInputs ti = stage_test_inputs(c, mem, n_star, P.d, t_star_in, v_star_in, ldvs);
  Pred s{c, P, th, n_star, samples, seed};
  s.q = qu_factors(c, P, th, gc, pre, /*want_cov=*/mode != GPAR_PREDICT_ANALYTIC);
  check_launch("predict: q(u) tail");
  const double s2 = th.sigma * th.sigma;
  s.grid = merge_grid(c, "pr", P, s2, ti.ts, n_star, P.y, ti.vs, ti.ldv, /*want_inputs=*/true,
                      /*want_pos=*/true);
  check_launch("predict: merge");
  s.cp = chain_params_of(th, s2);   // noise sigma^2 train / 1e10 test
  s.gg = grid_gains(c, P.sdim, s.cp, s.grid, prep, "pred");
  s.mean = ws<double>(c, "pr_mean", n_star);
  s.std = ws<double>(c, "pr_std", n_star);
  MeanStd out;
  if (mode == GPAR_PREDICT_PATH) {
    out = s.path_tail();
  } else {
    s.solve_kfu_columns();
    if (mode == GPAR_PREDICT_MC)
      out = s.mc_tail(s.rows());
    else if (c->predict_fused && s.q.ld == P.mp && predict_var_tiles(P.mp) > 0)
      out = s.fused_var_tail();
    else
      out = s.gemm_var_tail(s.rows());
  }
  release_prep(c, prep);
  deliver(c, mem, ti.perm, defer, n_star, {{out.mean, mean_out}, {out.std, std_out}});
}

// Device bytes of predict_impl's workspace (merged grid of n + n_star).
int64_t predict_ws_estimate(int64_t n, int64_t n_star, int64_t mp, int64_t d, int mode,
                            int samples, bool fused) {
  const int64_t nt = n + n_star, nch = (nt + kChunk - 1) / kChunk;
  int64_t doubles = nt * (mp + 64)                 // whitened Cf*u + y*
                    + n_star * ((fused ? 0 : mp) + 8 + d)   // Q rows (not with predict_var), mean / std, sorted test inputs
                    + nt * (20 + 8 + d)            // gains records, grid, merged inputs
                    + 4 * nch * (mp + 1) * 4       // carries
                    + 8 * mp * mp;                 // q(u) dense
  if (mode == GPAR_PREDICT_MC) doubles += n_star * mp + (int64_t)samples * mp + 2 * n_star * ((samples + 127) / 128);
  if (mode == GPAR_PREDICT_PATH)   // Cf*u, fx, the data columns, their whitening and the samples
    doubles += nt * mp + (int64_t)samples * (4 * nt + 2 * mp) + 6 * nch * samples * kSStride;
  return doubles * (int64_t)sizeof(double);
}

// --------------------------------------------------------------------------- sample-chained prediction
// Path mode with per-sample test inputs, its samples delivered (host_predict.hpp): predict_impl's
// stages with per_sample_fx in place of the shared-input Cf*u product.
void predict_samples_impl(gpar_ctx* c, const DevProblem& P, const Theta& th, int mem,
                          int64_t n_star, const double* t_star_in, const double* v_sh_in,
                          int64_t ldvs, int64_t d_sh, const double* v_sa_in, int64_t ld_s,
                          int64_t ld_r, int samples, uint64_t seed, double* f_out, int64_t ldf_s,
                          int64_t ldf_r, double* mean_out, double* std_out, const QuPre* pre,
                          const PredPrep* prep) {
  // path draw (s, k, i): counter index k (sdim + 1) + i, 32 bits
  ARGCHECK((P.n + n_star) * (P.sdim + 1) <= ((int64_t)1 << 32),
           "sample prediction: (n + n_star) * (state dimension + 1) must be <= 2^32");
  const int64_t d_sa = P.d - d_sh;
  const TestInputs ti = stage_test_inputs(c, mem, n_star, d_sh, t_star_in, v_sh_in, ldvs);
  // the sample inputs: device tensors are read in place; host ones are uploaded packed, in the
  // caller's row order -- the kernel gathers rows through the sort permutation either way
  const double* vsa = v_sa_in;
  const int64_t* dperm = nullptr;
  if (mem == GPAR_MEM_HOST && d_sa > 0) {
    double* dv = ws<double>(c, "ps_vsa", (size_t)samples * n_star * d_sa);
    if (ld_r == d_sa && ld_s == n_star * d_sa)
      h2d(c, dv, v_sa_in, (size_t)samples * n_star * d_sa);
    else
      for (int s = 0; s < samples; ++s)
        h2d_rows(c, dv + (size_t)s * n_star * d_sa, v_sa_in + (size_t)s * ld_s, ld_r, d_sa, n_star);
    vsa = dv;
    ld_r = d_sa;
    ld_s = n_star * d_sa;
    if (!ti.perm.empty()) {
      int64_t* dp = ws<int64_t>(c, "ps_perm", n_star);
      h2d(c, dp, ti.perm.data(), n_star);
      dperm = dp;
    }
  }
  Pred s{c, P, th, n_star, samples, seed};
  s.q = qu_factors(c, P, th, nullptr, pre, /*want_cov=*/true);
  check_launch("predict samples: q(u) tail");
  const double s2 = th.sigma * th.sigma;
  s.grid = merge_grid(c, "pr", P, s2, ti.ts, n_star, P.y, nullptr, 0, /*want_inputs=*/false,
                      /*want_pos=*/true, "_ym", /*want_tpos=*/true);
  check_launch("predict samples: merge");
  s.cp = chain_params_of(th, s2);   // noise sigma^2 train / 1e10 test
  s.gg = grid_gains(c, P.sdim, s.cp, s.grid, prep, "pred");
  s.mean = ws<double>(c, "pr_mean", n_star);
  s.std = ws<double>(c, "pr_std", n_star);
  const McFactor f = s.mc_factor();
  const double* Bm = s.sample_loadings(f);
  const double* FX = s.per_sample_fx(ti, d_sh, vsa, ld_s, ld_r, dperm, Bm);
  const double* F = s.path_draws(FX);
  release_prep(c, prep);
  // ---- delivery: the samples (strided destination, caller's row order), then mean and std
  if (mem == GPAR_MEM_DEVICE) {
    launch_sample_values(c->stream, FX, samples, F, samples, s.grid.pos, n_star, f_out, ldf_s, ldf_r);
    check_launch("predict samples: values");
  } else {
    double* dout = ws<double>(c, "ps_out", (size_t)samples * n_star);
    launch_sample_values(c->stream, FX, samples, F, samples, s.grid.pos, n_star, dout, n_star, 1);
    check_launch("predict samples: values");
    std::vector<double> h((size_t)samples * n_star);
    d2h(c, h.data(), dout, h.size());
    sync(c);   // every input is uploaded and read: f_out may now overwrite a column of v_sa's tensor
    for (int b = 0; b < samples; ++b)
      for (int64_t i = 0; i < n_star; ++i)
        f_out[b * ldf_s + (ti.perm.empty() ? i : ti.perm[i]) * ldf_r] = h[(size_t)b * n_star + i];
  }
  f.check(c);
  if (mean_out) deliver(c, mem, ti.perm, false, n_star, {{s.mean, mean_out}});
  if (std_out) deliver(c, mem, ti.perm, false, n_star, {{s.std, std_out}});
  if (!mean_out && !std_out && mem == GPAR_MEM_DEVICE) sync(c);
}

// Device bytes of predict_samples_impl's workspace: path mode's without the merged inputs and with
// Cf*u over the training rows only, plus the training rows' fx and the positions.
int64_t predict_samples_ws_estimate(int64_t n, int64_t n_star, int64_t mp, int64_t d_sh,
                                    int64_t d_sa, int samples, bool host) {
  const int64_t nt = n + n_star, nch = (nt + kChunk - 1) / kChunk;
  int64_t doubles = nt * (20 + 8)                       // gains records, fix-up rows, grid
                    + n + n_star * (4 + d_sh)           // positions, mean / std, sorted shared inputs
                    + 8 * mp * mp                       // q(u) dense, Lc, W
                    + n * mp + (int64_t)samples * (n + 4 * nt + 2 * mp)   // Cf*u (train), fx, z, X, F, xi, Bm
                    + 6 * nch * samples * kSStride + 4 * nch * 4;         // carries
  if (host) doubles += (int64_t)samples * n_star * (d_sa + 1) + n_star;   // staged inputs, outputs, perm
  return doubles * (int64_t)sizeof(double);
}

// --------------------------------------------------------------------------- mean-only prediction
// The ANALYTIC mean alone (gpar_scaled_inference.jl:91-97 with e = m_e): with w = U_u^{-1} m_e,
//   f = Cf*u w on the merged grid,  mean_i = f_k + (S (y* - f))_k,  k = pos[i],
// one Kfu-vector product (launch_kfu_gemv, Kfu never stored) and the smoother on ONE column --
// predict_impl whitens and adjoints all m columns of Cf*u to get the same number.  The training
// rows of y* - f depend on the posterior only (xtr).
void kfu_train_residual(gpar_ctx* c, const DevProblem& P, const Theta& th, const double* w,
                        double* xtr) {
  launch_kfu_gemv(c->stream, P.ok, P.v, P.ldv, P.n, P.z, P.ldz, P.m, (int)P.d, P.zc, w,
                  1.0 / th.l_o, th.sv_o * th.sv_o, P.y, 1.0, nullptr, xtr, nullptr);
  check_launch("predict mean: train f");
}

int64_t predict_mean_ws_estimate(int64_t n, int64_t n_star, int64_t mp, int64_t d) {
  const int64_t nt = n + n_star, nch = (nt + kChunk - 1) / kChunk;
  const int64_t doubles = nt * (20 + 8 + 5)      // gains records, fix-up rows, grid, x and u
                          + n + n_star * (4 + d)   // train residual, f*, mean, positions, sorted inputs
                          + 4 * nch * 4            // carries
                          + 8 * mp * mp;           // q(u) dense (no precomputed q(u))
  return doubles * (int64_t)sizeof(double);
}

void predict_mean_impl(gpar_ctx* c, const DevProblem& P, const Theta& th, int mem, int64_t n_star,
                       const double* t_star_in, const double* v_star_in, int64_t ldvs,
                       double* mean_out, const GramCache* gc, bool defer, const QuPre* pre,
                       const PredPrep* prep, const double* xtr) {
  const int64_t m = P.m, d = P.d;
  Timed tm_all(c, "pred_mean");
  const TestInputs ti = stage_test_inputs(c, mem, n_star, d, t_star_in, v_star_in, ldvs);
  const double* w = qu_factors(c, P, th, gc, pre, /*want_cov=*/false).w;
  // ---- the training rows of x = y* - f
  if (!xtr) {
    double* xv = ws<double>(c, "pm_xtr", P.n);
    kfu_train_residual(c, P, th, w, xv);
    xtr = xv;
  }
  // ---- merged grid: times, noise, and x (train rows placed by the merge, test rows by the
  //      test side's product below); no merged inputs
  const double s2 = th.sigma * th.sigma;
  const MergedGrid grid = merge_grid(c, "pm", P, s2, ti.ts, n_star, xtr, nullptr, 0,
                                     /*want_inputs=*/false, /*want_pos=*/true, "_x");
  double* x = grid.ym;
  double* fstar = ws<double>(c, "pm_fstar", n_star);
  check_launch("predict mean: merge");
  {   // flops of the test side's distances and product; its n* m kernel evaluations come on top
    Timed tm_(c, "pred_mean_kfu", 2.0 * (double)n_star * (double)m * (double)(d + 1));
    launch_kfu_gemv(c->stream, P.ok, ti.vs, ti.ldv, n_star, P.z, P.ldz, m, (int)d, P.zc, w,
                    1.0 / th.l_o, th.sv_o * th.sv_o, nullptr, 0.0, grid.pos, x, fstar);
  }
  check_launch("predict mean: test f");
  const GridGains gg = grid_gains(c, P.sdim, chain_params_of(th, s2), grid, prep, "pmean");
  // ---- S x at the test rows: whitening and the Sigma^{-1} solve, all on one column
  double* u = ws<double>(c, "pm_u", grid.nt);
  const SigmaCols cols = sigma_cols(c, "pm", u, 1, 1, grid.nt, /*wide=*/false, nullptr);
  double* dmean = ws<double>(c, "pm_mean", n_star);
  launch_whiten_vec(c->stream, P.sdim, gg.g.rec, 0, x, 0, grid.nt, kChunk, grid.nch, 1, u, 0,
                    cols.send, 0, 1, 0);
  const double* h = sigma_inv_columns(c, P.sdim, gg, cols, "pm", "pmean");
  launch_mean_finish(c->stream, P.sdim, u, h, cols.chat, x, grid.rm, fstar, grid.pos, n_star, kChunk,
                     dmean);
  check_launch("predict mean: smoother");
  release_prep(c, prep);
  deliver(c, mem, ti.perm, defer, n_star, {{dmean, mean_out}});
}

}  // namespace gpar
using namespace gpar;
extern "C" {

int32_t gpar_predict(gpar_ctx* ctx, const gpar_problem* prob, const double* theta,
                     int64_t n_star, const double* t_star, const double* v_star, int64_t ldvs,
                     int32_t mode, int32_t samples, uint64_t seed, double* mean, double* std) {
  API_BEGIN(ctx)
  ARGCHECK(prob && theta && t_star && v_star && mean && std, "null argument");
  ARGCHECK(n_star >= 1, "n_star must be >= 1");
  ARGCHECK(ldvs >= prob->d, "ldvs must be >= d");
  check_predict_mode(mode, samples);
  const DevProblem P = prepare_problem(ctx, *prob, 0);
  predict_impl(ctx, P, thetas_from(theta, 1)[0], prob->mem, n_star, t_star, v_star, ldvs, mode,
               samples, seed, mean, std);
  API_END(ctx)
}

int32_t gpar_predict_mean(gpar_ctx* ctx, const gpar_problem* prob, const double* theta,
                          int64_t n_star, const double* t_star, const double* v_star,
                          int64_t ldvs, double* mean) {
  API_BEGIN(ctx)
  ARGCHECK(prob && theta && t_star && v_star && mean, "null argument");
  ARGCHECK(n_star >= 1, "n_star must be >= 1");
  ARGCHECK(ldvs >= prob->d, "ldvs must be >= d");
  const DevProblem P = prepare_problem(ctx, *prob, 0);
  predict_mean_impl(ctx, P, thetas_from(theta, 1)[0], prob->mem, n_star, t_star, v_star, ldvs, mean);
  API_END(ctx)
}

int32_t gpar_predict_samples(gpar_ctx* ctx, const gpar_problem* prob, const double* theta,
                             int64_t n_star, const double* t_star, const double* v_shared,
                             int64_t ldvs, int64_t d_shared, const double* v_samp, int64_t ld_s,
                             int64_t ld_r, int32_t samples, uint64_t seed, double* f_out,
                             int64_t ldf_s, int64_t ldf_r, double* mean, double* std) {
  API_BEGIN(ctx)
  ARGCHECK(prob && theta, "null argument");
  check_sample_args(prob->d, n_star, t_star, v_shared, ldvs, d_shared, v_samp, ld_s, ld_r, samples,
                    f_out, ldf_s, ldf_r);
  const DevProblem P = prepare_problem(ctx, *prob, 0);
  predict_samples_impl(ctx, P, thetas_from(theta, 1)[0], prob->mem, n_star, t_star, v_shared, ldvs,
                       d_shared, v_samp, ld_s, ld_r, samples, seed, f_out, ldf_s, ldf_r, mean, std);
  API_END(ctx)
}

int32_t gpar_mc_normals(gpar_ctx* ctx, int32_t samples, int64_t m, uint64_t seed, double* xi_out) {
  API_BEGIN(ctx)
  ARGCHECK(xi_out, "null argument");
  ARGCHECK(samples >= 1 && samples <= kMaxSamples, "samples must be in 1..65536");
  ARGCHECK(m >= 1 && m <= (int64_t)1 << 20, "m out of range");
  double* xi = ws<double>(ctx, "mc_xi_export", (size_t)samples * m);
  launch_normal(ctx->stream, xi, m, samples, m, samples, seed);
  check_launch("normal draws");
  d2h(ctx, xi_out, xi, (size_t)samples * m);
  sync(ctx);
  API_END(ctx)
}

int32_t gpar_path_normals(gpar_ctx* ctx, int32_t samples, int64_t n, int32_t d, uint64_t seed,
                          double* xi_out) {
  API_BEGIN(ctx)
  ARGCHECK(xi_out, "null argument");
  ARGCHECK(samples >= 1 && samples <= kMaxSamples, "samples must be in 1..65536");
  ARGCHECK(d >= 1 && d <= 4 && n >= 1 && n * d <= ((int64_t)1 << 32) - 1, "n, d out of range");
  double* xi = ws<double>(ctx, "path_xi_export", (size_t)samples * n * d);
  launch_normal(ctx->stream, xi, n * d, samples, n * d, samples, path_seed(seed));
  check_launch("path normal draws");
  d2h(ctx, xi_out, xi, (size_t)samples * n * d);
  sync(ctx);
  API_END(ctx)
}

int32_t gpar_lgssm_posterior_rand(gpar_ctx* ctx, int64_t n, const double* t, const double* y,
                                  const double* noise, int32_t kernel, const double* theta,
                                  int32_t samples, uint64_t seed, int32_t mem, double* f_out) {
  API_BEGIN(ctx)
  ARGCHECK(n >= 1 && t && y && theta && f_out, "bad argument");
  ARGCHECK(samples >= 1 && samples <= kMaxSamples, "samples must be in 1..65536");
  ARGCHECK(mem == GPAR_MEM_HOST || mem == GPAR_MEM_DEVICE, "bad mem");
  const int sdim = sde_dim(kernel);
  // draw (s, k, i) is counter_normal(seed, s, k (sdim + 1) + i): the index must fit 32 bits
  ARGCHECK(n * (sdim + 1) <= ((int64_t)1 << 32), "n * (state dimension + 1) must be <= 2^32");
  std::vector<ChainParamsHost> cps = chain_params(theta, 1);
  const double *dt = t, *dy = y, *dn = noise;
  if (mem == GPAR_MEM_HOST) {
    check_sorted_host(t, n);
    double* tt = ws<double>(ctx, "lpr_t", n);
    double* yy = ws<double>(ctx, "lpr_y", n);
    h2d(ctx, tt, t, n);
    h2d(ctx, yy, y, n);
    if (noise) {
      double* nn = ws<double>(ctx, "lpr_noise", n);
      h2d(ctx, nn, noise, n);
      dn = nn;
    }
    dt = tt;
    dy = yy;
  }
  GainsOut g = run_gains(ctx, sdim, dt, n, cps, dn, false, "lpr");
  double* F = ws<double>(ctx, "lpr_F", (size_t)n * samples);
  path_samples(ctx, sdim, g, cps[0], dt, dn, n, dy, nullptr, 0, samples, seed, F);
  double* out = mem == GPAR_MEM_DEVICE ? f_out : ws<double>(ctx, "lpr_out", (size_t)n * samples);
  launch_path_transpose(ctx->stream, F, n, samples, out);
  check_launch("posterior_rand");
  if (mem == GPAR_MEM_HOST) d2h(ctx, f_out, out, (size_t)n * samples);
  sync(ctx);
  API_END(ctx)
}

}  // extern "C"
