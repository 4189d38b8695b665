// host_fit_predict.cpp -- the batched fit + predict driver (gpar_fit_predict[_chain]): one fit, then
// every output's prediction at its fitted theta over the prediction lanes.
#include "host.hpp"

namespace gpar {

// Host-memory batches without a chain: the test inputs go up once after the fit (t* sorted once;
// every distinct v* base -- GPAR's outputs read column prefixes of one N* x P matrix -- in one
// linear copy), the predictions run on device buffers (with lanes), and the means / stds come
// down at the end.  (With a chain, later outputs read host columns the earlier predictions
// write: those predictions keep the per-output host path.)
struct StagedInputs {
  std::vector<int64_t> perm;        // ascending_perm of t*
  const double* ts = nullptr;       // t*, ascending, on the device
  std::vector<const double*> vs;    // per output: its inputs on the device, rows in ts's order
  std::vector<int64_t> ldv;
  double* res = nullptr;            // the outputs' results: [nprob][mean, std][n_star]
};
static StagedInputs stage_batch_inputs(gpar_ctx* ctx, const gpar_problem* probs, int32_t nprob,
                                       int64_t n_star, const double* t_star,
                                       const double* const* v_star, const int64_t* ldvs) {
  StagedInputs st;
  st.vs.assign(nprob, nullptr);
  st.ldv.assign(nprob, 0);
  const std::vector<int64_t>& perm = st.perm = ascending_perm(t_star, n_star);
  std::vector<double> tmp;
  double* tsd = ws<double>(ctx, "fph_ts", n_star);
  if (perm.empty()) {
    h2d(ctx, tsd, t_star, n_star);
  } else {
    tmp.resize(n_star);
    for (int64_t k = 0; k < n_star; ++k) tmp[k] = t_star[perm[k]];
    h2d(ctx, tsd, tmp.data(), n_star);
    sync(ctx);
  }
  st.ts = tsd;
  std::vector<int> grp(nprob, -1);
  int ng = 0;
  for (int i = 0; i < nprob; ++i) {
    for (int j = 0; j < i && grp[i] < 0; ++j)
      if (v_star[j] == v_star[i] && ldvs[j] == ldvs[i]) grp[i] = grp[j];
    if (grp[i] < 0) grp[i] = ng++;
  }
  for (int g = 0; g < ng; ++g) {
    int64_t wmax = 0;
    int first = -1;
    for (int i = 0; i < nprob; ++i)
      if (grp[i] == g) {
        wmax = std::max(wmax, probs[i].d);
        if (first < 0) first = i;
      }
    std::pair<const double*, int64_t> b;
    if (perm.empty()) {
      b = upload_shared_block(ctx, "fph_vs" + std::to_string(g), v_star[first], ldvs[first], wmax,
                              n_star);
    } else {   // the rows in t*'s ascending order, gathered on the host
      tmp.assign((size_t)n_star * wmax, 0.0);
      for (int64_t k = 0; k < n_star; ++k)
        for (int64_t q = 0; q < wmax; ++q) tmp[k * wmax + q] = v_star[first][perm[k] * ldvs[first] + q];
      b = upload_shared_block(ctx, "fph_vs" + std::to_string(g), tmp.data(), wmax, wmax, n_star);
      sync(ctx);
    }
    for (int i = 0; i < nprob; ++i)
      if (grp[i] == g) {
        st.vs[i] = b.first;
        st.ldv[i] = b.second;
      }
  }
  st.res = ws<double>(ctx, "fph_res", (size_t)nprob * 2 * n_star);
  return st;
}
// the staged means / stds into the caller's host buffers, in t*'s input order
static void unstage_results(gpar_ctx* ctx, const StagedInputs& st, int32_t nprob, int64_t n_star,
                            double* const* mean_out, double* const* std_out) {
  for (int i = 0; i < nprob; ++i) {
    const double* src = st.res + (size_t)(2 * i) * n_star;
    deliver(ctx, GPAR_MEM_HOST, st.perm, /*defer=*/true, n_star,
            {{src, mean_out[i]}, {src + n_star, std_out[i]}});
  }
  sync(ctx);
}

// a lane's stream and workspace names; restored on any exit
struct LaneScope {
  gpar_ctx* c;
  hipStream_t saved;
  LaneScope(gpar_ctx* c_, int lane) : c(c_), saved(c_->stream) {
    c->stream = lane ? c->side : c->main;
    c->ws_suffix = lane ? "~1" : "";
  }
  ~LaneScope() {
    c->stream = saved;
    c->ws_suffix.clear();
  }
};

// get_gpar_scaled_predictions for a batch: batched fit, then each output's prediction at its
// fitted theta (in output order).  chain (optional): after output i's prediction its mean is also
// written to column chain_col[i] of chain (point k at chain[k * ld_chain + col]), so later outputs'
// v_star may point into chain and read earlier outputs' predicted means as inference inputs.
static void fit_predict_impl(gpar_ctx* ctx, const gpar_problem* probs, int32_t nprob,
                             const double* log_theta0, const gpar_fit_options* opts, int64_t n_star,
                             const double* t_star, const double* const* v_star, const int64_t* ldvs,
                             int32_t mode, int32_t samples, uint64_t seed, double* chain,
                             int64_t ld_chain, const int32_t* chain_col, double* theta_out,
                             double* nlml_out, int32_t* evals_out, double* const* mean_out,
                             double* const* std_out) {
  ARGCHECK(probs && nprob >= 1 && log_theta0 && theta_out && t_star && v_star && ldvs &&
               mean_out && std_out, "null argument");
  ARGCHECK(n_star >= 1, "n_star must be >= 1");
  check_predict_mode(mode, samples);
  for (int i = 0; i < nprob; ++i) {
    ARGCHECK(v_star[i] && mean_out[i] && std_out[i], "null per-output pointer");
    ARGCHECK(ldvs[i] >= probs[i].d, "ldvs must be >= d");
    if (chain) ARGCHECK(chain_col[i] < ld_chain, "chain_col must be < ld_chain");
  }
  check_batch(probs, nprob);
  gpar_fit_options o{0, 1000, 1e-8, 0.0};
  if (opts) o = *opts;
  const std::vector<DevProblem> P = prepare_batch(ctx, probs, nprob);
  FitKeep keep;
  const int mem = probs[0].mem;
  // Prediction lanes: with device-memory outputs and no chain between the predictions, outputs
  // alternate over the context's two streams, each lane with its own workspace (name suffix), so
  // one output's memory-bound passes (merge, adjoint, rows) run beside the other's DP / MFMA work
  // (whitening, variance GEMM).  A lane's host syncs (q(u)'s Cholesky status) wait for that lane
  // only.
  // Host-memory batches without a chain run staged (StagedInputs), with lanes.
  const bool stage = mem == GPAR_MEM_HOST && !chain;
  const bool lanes = (mem == GPAR_MEM_DEVICE || stage) && !chain && nprob > 1 &&
                     ctx->predict_lanes > 1;
  // the predictions' workspace (named buffers, reused across the outputs: the largest counts)
  int64_t pred_bytes = 0;
  for (const auto& p : P)
    pred_bytes = std::max(pred_bytes, predict_ws_estimate(p.n, n_star, p.mp, p.d, mode, samples,
                                                          mode == GPAR_PREDICT_ANALYTIC &&
                                                              ctx->predict_fused &&
                                                              predict_var_tiles(p.mp) > 0));
  int64_t stage_bytes = stage ? 8 * n_star * (1 + 2 * (int64_t)nprob) : 0;
  for (int i = 0; i < nprob && stage; ++i) stage_bytes += 8 * n_star * ldvs[i];   // upper bound
  // "chain_mean_first": the chain carries means only (GPAR_scaled_examples.jl:172), so the
  // context stream runs each output's mean-only prediction in chain order and the full
  // prediction of output i, which supplies its std, follows on the side stream's lane
  const bool mean_first = ctx->chain_mean_first && chain && mem == GPAR_MEM_DEVICE &&
                          mode == GPAR_PREDICT_ANALYTIC;
  int64_t mean_bytes = 0;
  if (mean_first)
    for (const auto& p : P)
      mean_bytes = std::max(mean_bytes, predict_mean_ws_estimate(p.n, n_star, p.mp, p.d));
  fit_impl(ctx, P, log_theta0, o, theta_out, nlml_out, evals_out, &keep,
           (lanes ? 2 : 1) * pred_bytes + stage_bytes + mean_bytes);
  StagedInputs st;
  if (stage) st = stage_batch_inputs(ctx, probs, nprob, n_star, t_star, v_star, ldvs);
  const std::vector<Theta> T = thetas_from(theta_out, nprob);
  // wall time of the predictions (both lanes): from here on the context stream to the join
  std::optional<Timed> tm_pred(std::in_place, ctx, "predictions");
  // q(u) and its substitutions for every output at once (one sync), when the outputs share the
  // q(u) convention
  bool same_qu = true;
  for (const auto& p : P) same_qu = same_qu && p.qu_noise == P[0].qu_noise;
  std::vector<QuPre> pre;
  if (ctx->qu_batch && nprob > 1 && same_qu)
    pre = run_q_u_batch(ctx, P, T, keep, mode != GPAR_PREDICT_ANALYTIC);
  // output i's kept Gram and precomputed q(u), where there is one
  auto gc = [&](int i) { return keep.valid[i] ? &keep.gram[i] : nullptr; };
  auto pq = [&](int i) { return pre.empty() ? nullptr : &pre[i]; };
  if (lanes) {   // the side lane follows the fit (kept Grams, inputs) on the context stream
    HIPCHECK(hipEventRecord(ctx->ev_fork, ctx->main));
    HIPCHECK(hipStreamWaitEvent(ctx->side, ctx->ev_fork, 0));
  }
  for (int i = 0; i < nprob && mean_first; ++i) {
    {   // ordered part: the mean, its chain column, the event the full prediction follows
      LaneScope lane_(ctx, 0);
      predict_mean_impl(ctx, P[i], T[i], mem, n_star, t_star, v_star[i], ldvs[i], mean_out[i],
                        gc(i), /*defer=*/true, pq(i));
      if (chain_col[i] >= 0)
        HIPCHECK(hipMemcpy2DAsync(chain + chain_col[i], ld_chain * sizeof(double), mean_out[i],
                                  sizeof(double), sizeof(double), n_star, hipMemcpyDeviceToDevice,
                                  ctx->stream));
      HIPCHECK(hipEventRecord(ctx->ev_fork, ctx->main));
    }
    {   // output i's std, beside the later outputs' means; its mean goes to a scratch vector
      LaneScope lane_(ctx, 1);
      HIPCHECK(hipStreamWaitEvent(ctx->side, ctx->ev_fork, 0));
      double* mean_full = ws<double>(ctx, "fp_mean_full", n_star);
      predict_impl(ctx, P[i], T[i], mem, n_star, t_star, v_star[i], ldvs[i], mode, samples,
                   seed + (uint64_t)i, mean_full, std_out[i], gc(i), /*defer=*/true, pq(i));
    }
  }
  if (mean_first) {
    HIPCHECK(hipEventRecord(ctx->ev_join, ctx->side));
    HIPCHECK(hipStreamWaitEvent(ctx->main, ctx->ev_join, 0));
  }
  for (int i = 0; i < nprob && !mean_first; ++i) {
    LaneScope lane_(ctx, lanes ? (i & 1) : 0);
    if (stage)
      predict_impl(ctx, P[i], T[i], GPAR_MEM_DEVICE, n_star, st.ts, st.vs[i], st.ldv[i], mode,
                   samples, seed + (uint64_t)i, st.res + (size_t)(2 * i) * n_star,
                   st.res + (size_t)(2 * i + 1) * n_star, gc(i), /*defer=*/true, pq(i));
    else
      predict_impl(ctx, P[i], T[i], mem, n_star, t_star, v_star[i], ldvs[i], mode, samples,
                   seed + (uint64_t)i, mean_out[i], std_out[i], gc(i), /*defer=*/lanes, pq(i));
    if (chain && chain_col[i] >= 0) {
      double* dst = chain + chain_col[i];
      if (mem == GPAR_MEM_DEVICE) {   // stream-ordered before the next output's merge reads it
        HIPCHECK(hipMemcpy2DAsync(dst, ld_chain * sizeof(double), mean_out[i], sizeof(double),
                                  sizeof(double), n_star, hipMemcpyDeviceToDevice, ctx->stream));
      } else {
        for (int64_t k = 0; k < n_star; ++k) dst[k * ld_chain] = mean_out[i][k];
      }
    }
  }
  if (lanes) {
    HIPCHECK(hipEventRecord(ctx->ev_join, ctx->side));
    HIPCHECK(hipStreamWaitEvent(ctx->main, ctx->ev_join, 0));
  }
  tm_pred.reset();
  if (lanes || stage || (chain && mem == GPAR_MEM_DEVICE)) sync(ctx);
  if (stage) unstage_results(ctx, st, nprob, n_star, mean_out, std_out);
}
}  // namespace gpar
using namespace gpar;
extern "C" {

int32_t gpar_fit_predict(gpar_ctx* ctx, const gpar_problem* probs, int32_t nprob,
                         const double* log_theta0, const gpar_fit_options* opts, int64_t n_star,
                         const double* t_star, const double* const* v_star, const int64_t* ldvs,
                         int32_t mode, int32_t samples, uint64_t seed, double* theta_out,
                         double* nlml_out, int32_t* evals_out, double* const* mean_out,
                         double* const* std_out) {
  API_BEGIN(ctx)
  fit_predict_impl(ctx, probs, nprob, log_theta0, opts, n_star, t_star, v_star, ldvs, mode, samples,
                   seed, nullptr, 0, nullptr, theta_out, nlml_out, evals_out, mean_out, std_out);
  API_END(ctx)
}

int32_t gpar_fit_predict_chain(gpar_ctx* ctx, const gpar_problem* probs, int32_t nprob,
                               const double* log_theta0, const gpar_fit_options* opts,
                               int64_t n_star, const double* t_star, const double* const* v_star,
                               const int64_t* ldvs, int32_t mode, int32_t samples, uint64_t seed,
                               double* chain, int64_t ld_chain, const int32_t* chain_col,
                               double* theta_out, double* nlml_out, int32_t* evals_out,
                               double* const* mean_out, double* const* std_out) {
  API_BEGIN(ctx)
  ARGCHECK(chain && chain_col && ld_chain >= 1, "null chain argument");
  fit_predict_impl(ctx, probs, nprob, log_theta0, opts, n_star, t_star, v_star, ldvs, mode, samples,
                   seed, chain, ld_chain, chain_col, theta_out, nlml_out, evals_out, mean_out,
                   std_out);
  API_END(ctx)
}

}  // extern "C"
