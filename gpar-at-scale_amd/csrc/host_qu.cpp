// host_qu.cpp -- q(u) and the substitutions the predictions read, for a batch of outputs or one.
#include "host.hpp"

namespace gpar {

// one: the single-output route -- the kept Gram is read in place (mpmax == mp: nothing to pack)
// and the Cholesky failures are reported without an output index.
//
// G = beta^T beta and r = beta^T alpha do not depend on Cuu's jitter (only L_u does,
// gpar_scaled_inference.jl:157-187), but their rounding matters for the noise-free Cuu: it takes
// the extra beta fix-up pass (a plain beta^T beta of the true beta carries ~10x less rounding
// than the objective's correction form, and cond(Cuu) up to ~1e10 amplifies it -- reusing the
// fit's correction-form Gram there measured 1.5e-7 relative off the oracle's std, r04a).  With
// qu_kuu_noise the factor is the objective's regularised Kuu + s2 I and the correction-form Grams
// the fit computed at these thetas are reused when the caller hands them over (keep).
static std::vector<QuPre> q_u_batch(gpar_ctx* c, const std::vector<DevProblem>& P,
                                    const std::vector<Theta>& T, const FitKeep& keep,
                                    bool want_cov, bool one) {
  const int np = (int)P.size();
  const int64_t mpmax = max_mp(P);
  int64_t mmax = 0;
  for (const auto& p : P) mmax = std::max(mmax, p.m);
  const bool qn = P[0].qu_noise;
  bool kept = qn;   // the fit's Grams serve the regularised convention only
  for (int i = 0; i < np; ++i)
    kept = kept && i < (int)keep.valid.size() && keep.valid[i] && keep.gram[i].G;
  GramOut go;
  const size_t sq = (size_t)mpmax * mpmax;
  if (kept) {   // the fit's Grams at the fitted theta, packed at the batch's ld
    go.ldg = mpmax;
    go.npart = 1;
    go.a2part = ws<double>(c, "qub_zero_a2", (size_t)np);   // dtc terms: unused in q(u) mode
    go.logs = ws<double>(c, "qub_zero_logs", (size_t)np * P[0].nch);
    HIPCHECK(hipMemsetAsync(go.a2part, 0, (size_t)np * sizeof(double), c->stream));
    HIPCHECK(hipMemsetAsync(go.logs, 0, (size_t)np * P[0].nch * sizeof(double), c->stream));
    if (one) {
      go.G = const_cast<double*>(keep.gram[0].G);
      go.r = const_cast<double*>(keep.gram[0].r);
    } else {
      go.G = ws<double>(c, "qub_G", (size_t)np * sq);
      go.r = ws<double>(c, "qub_r", (size_t)np * mpmax);
      HIPCHECK(hipMemsetAsync(go.G, 0, (size_t)np * sq * sizeof(double), c->stream));
      HIPCHECK(hipMemsetAsync(go.r, 0, (size_t)np * mpmax * sizeof(double), c->stream));
      for (int i = 0; i < np; ++i) {
        const GramCache& g = keep.gram[i];
        HIPCHECK(hipMemcpy2DAsync(go.G + i * sq, mpmax * sizeof(double), g.G, P[i].mp * sizeof(double),
                                  P[i].mp * sizeof(double), P[i].mp, hipMemcpyDeviceToDevice, c->stream));
        HIPCHECK(hipMemcpyAsync(go.r + (size_t)i * mpmax, g.r, P[i].mp * sizeof(double),
                                hipMemcpyDeviceToDevice, c->stream));
      }
    }
  } else {
    go = run_gram_stage(c, P, T, /*fix_beta=*/!qn);
  }
  DenseOut dn = run_dense(c, P, T, go, /*qu_mode=*/true);
  const int64_t ld = dn.ld;
  double* me = ws<double>(c, "qub_me", (size_t)np * ld);
  double* dout = ws<double>(c, "qub_out", (size_t)np);
  std::vector<Finish2JobHost> fj(np);
  for (int i = 0; i < np; ++i) fj[i] = finish_job(dn, go, P[i], i, P[0].nch, dout + i, me + i * ld);
  auto* dfj = ws<Finish2JobHost>(c, "qub_finish", np);
  h2d(c, dfj, fj.data(), np);
  launch_finish2(c->stream, dfj, np, ld, dn.nb);
  check_launch("finish(q_u batch)");
  std::vector<int> st(2 * np);
  d2h(c, st.data(), dn.status, 2 * np);
  sync(c);
  for (int i = 0; i < np; ++i) {
    const std::string which = one ? "" : ", output " + std::to_string(i);
    if (st[2 * i]) throw Error(GPAR_ERR_NOT_PD, "PosDefException: cholesky(Symmetric(Cuu)) failed (gpar_scaled_inference.jl:159)" + which);
    if (st[2 * i + 1]) throw Error(GPAR_ERR_NOT_PD, "PosDefException: cholesky(Symmetric(D)) failed (gpar_scaled_inference.jl:188)" + which);
  }
  // w, X1, Vm (and X, cov) by substitution, one launch each for all outputs.  q(u) factors the
  // noise-free Cuu (gpar_scaled_inference.jl:157; cond up to ~1e10), where products of explicit
  // inverses lose accuracy that triangular substitution keeps -- the objective's
  // T_u = chol(Kuu + s2 I)^-1 is regularised by the noise and stays on the blocked-inverse path.
  double* I = ws<double>(c, "qub_eye", (size_t)ld * ld);
  double* w = ws<double>(c, "qub_w", (size_t)np * ld);
  double* X1 = ws<double>(c, "qub_X1", (size_t)np * ld * ld);
  double* Vm = ws<double>(c, "qub_V", (size_t)np * ld * ld);
  // V = 0 outside its m x m block (predict_var reads the whole ld x ld buffer)
  HIPCHECK(hipMemsetAsync(Vm, 0, (size_t)np * ld * ld * sizeof(double), c->stream));
  launch_eye(c->stream, I, ld, (int)mmax);
  std::vector<TrsvJobHost> tv(np);
  std::vector<TrsmJobHost> t1(np), t2(np), t3(np);
  double* Xc = want_cov ? ws<double>(c, "qub_Xc", (size_t)np * ld * ld) : nullptr;
  double* cov = want_cov ? ws<double>(c, "qub_cov", (size_t)np * ld * ld) : nullptr;
  for (int i = 0; i < np; ++i) {
    const double* Lu = dn.Lu + i * (size_t)ld * ld;
    const double* LD = dn.Llam + i * (size_t)ld * ld;
    const int m = (int)P[i].m;
    tv[i] = {Lu, ld, m, me + i * ld, w + i * ld, 1};
    t1[i] = {Lu, ld, I, ld, X1 + i * (size_t)ld * ld, ld, m, P[i].m, 0, 0};
    t2[i] = {LD, ld, X1 + i * (size_t)ld * ld, ld, Vm + i * (size_t)ld * ld, ld, m, P[i].m, 0, 0};
    if (want_cov) t3[i] = {LD, ld, I, ld, Xc + i * (size_t)ld * ld, ld, m, P[i].m, 0, 0};
  }
  auto* dtv = ws<TrsvJobHost>(c, "qub_trsv", np);
  auto* dt1 = ws<TrsmJobHost>(c, "qub_trsm1", np);
  auto* dt2 = ws<TrsmJobHost>(c, "qub_trsm2", np);
  h2d(c, dtv, tv.data(), np);
  h2d(c, dt1, t1.data(), np);
  h2d(c, dt2, t2.data(), np);
  launch_trsv(c->stream, dtv, np);
  launch_trsm(c->stream, dt1, np, mmax);
  launch_trsm(c->stream, dt2, np, mmax);
  if (want_cov) {
    auto* dt3 = ws<TrsmJobHost>(c, "qub_trsm3", np);
    h2d(c, dt3, t3.data(), np);
    launch_trsm(c->stream, dt3, np, mmax);
    for (int i = 0; i < np; ++i)
      launch_gram_small(c->stream, Xc + i * (size_t)ld * ld, ld, (int)P[i].m, cov + i * (size_t)ld * ld, ld);
  }
  check_launch("q_u batch substitutions");
  std::vector<QuPre> out(np);
  for (int i = 0; i < np; ++i)
    out[i] = {dn.Lu + i * (size_t)ld * ld, dn.Llam + i * (size_t)ld * ld, me + i * ld, w + i * ld,
              X1 + i * (size_t)ld * ld, Vm + i * (size_t)ld * ld,
              want_cov ? cov + i * (size_t)ld * ld : nullptr, ld, dn.nb};
  return out;
}

std::vector<QuPre> run_q_u_batch(gpar_ctx* c, const std::vector<DevProblem>& P,
                                 const std::vector<Theta>& T, const FitKeep& keep, bool want_cov) {
  return q_u_batch(c, P, T, keep, want_cov, /*one=*/false);
}

QuPre run_q_u_one(gpar_ctx* c, const DevProblem& p, const Theta& th, const GramCache* gc,
                  bool want_cov) {
  FitKeep keep;
  if (gc) {
    keep.gram.push_back(*gc);
    keep.valid.push_back(1);
  }
  return q_u_batch(c, {p}, {th}, keep, want_cov, /*one=*/true)[0];
}

}  // namespace gpar
using namespace gpar;
extern "C" {

int32_t gpar_q_u(gpar_ctx* ctx, const gpar_problem* prob, const double* theta, double* m_e,
                 double* cov, double* U_u) {
  API_BEGIN(ctx)
  ARGCHECK(prob && theta && m_e && cov && U_u, "null argument");
  const DevProblem P = prepare_problem(ctx, *prob, 0);
  const QuPre q = run_q_u_one(ctx, P, thetas_from(theta, 1)[0], nullptr, /*want_cov=*/true);
  const int64_t m = P.m;
  double* Ucol = ws<double>(ctx, "qu_U", (size_t)m * m);   // U_u = L_u^T, column-major
  launch_lower_to_upper_colmajor(ctx->stream, q.Lu, q.ld, (int)m, Ucol);
  check_launch("q_u tail");
  const hipMemcpyKind kind = prob->mem == GPAR_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  HIPCHECK(hipMemcpyAsync(m_e, q.me, m * sizeof(double), kind, ctx->stream));
  HIPCHECK(hipMemcpy2DAsync(cov, m * sizeof(double), q.cov, q.ld * sizeof(double), m * sizeof(double), m, kind, ctx->stream));
  HIPCHECK(hipMemcpyAsync(U_u, Ucol, m * m * sizeof(double), kind, ctx->stream));
  sync(ctx);
  API_END(ctx)
}

}  // extern "C"
