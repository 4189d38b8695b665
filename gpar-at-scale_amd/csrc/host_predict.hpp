// host_predict.hpp -- the prediction side's shared declarations (included by host.hpp): q(u), the
// named stages every prediction mode is a sequence of (host_predict.cpp), and what the batched
// driver (host_fit_predict.cpp) and the posterior objects (host_posterior.cpp) call.
#pragma once

#include <initializer_list>

namespace gpar {

// --------------------------------------------------------------------------- q(u)  (host_qu.cpp)
// compute_q_u (gpar_scaled_inference.jl:141-196): Cuu without noise, D = L_u^-1 G L_u^-T + I,
// m_e = D^-1 L_u^-1 r, cov = inv(D) = L_D^-T L_D^-1, U_u = chol(Cuu).U.
// q(u) and the substitutions every prediction mode needs, for all outputs of a gpar_fit_predict
// call at once (a batched prediction used to run them per output: the blocked Cholesky, the
// finish, three trsm and a trsv, each a latency-bound launch of one small job, ~4 ms per output
// and a host sync each).  Per output i: Lu, LD (chol(Cuu), chol(D)), me = m_e, w = U_u^{-1} m_e
// = L_u^{-T} m_e, X1 = L_u^{-1}, Vm = L_D^{-1} L_u^{-1} (zero outside m x m), and for the MC / path
// modes cov = inv(D) = X^T X, X = L_D^{-1}.  DenseOut and QuPre are the only way a factor pointer
// leaves run_dense.
struct QuPre {
  const double *Lu, *LD, *me, *w, *X1, *Vm, *cov;
  int64_t ld;
  int nb;
};
std::vector<QuPre> run_q_u_batch(gpar_ctx* c, const std::vector<DevProblem>& P,
                                 const std::vector<Theta>& T, const FitKeep& keep, bool want_cov);
// One output's q(u): the batch of one.  gc (optional): the fit's Gram at th, read in place.
QuPre run_q_u_one(gpar_ctx* c, const DevProblem& p, const Theta& th, const GramCache* gc,
                  bool want_cov);
// A prediction's q(u) factors: the precomputed ones (pre), or computed here.
inline QuPre qu_factors(gpar_ctx* c, const DevProblem& P, const Theta& th, const GramCache* gc,
                        const QuPre* pre, bool want_cov) {
  return pre ? *pre : run_q_u_one(c, P, th, gc, want_cov);
}

// --------------------------------------------------------------------------- stages  (host_predict.cpp)
// The stable sort permutation of t (sorted position -> input position); empty when t is ascending
// already, which every reader takes for the identity.
std::vector<int64_t> ascending_perm(const double* t, int64_t n);

// Result vectors (rows x n each, ascending test order on the device) into the caller's buffers:
// device memory by a device copy; host memory straight down when perm is empty, else through a
// scratch vector, each row un-permuted.  defer: leave out the closing sync where nothing on the
// host waits for the copies (the caller synchronises); the un-permutation always waits.
struct Delivery {
  const double* src;
  double* dst;
};
void deliver(gpar_ctx* c, int mem, const std::vector<int64_t>& perm, bool defer, int64_t n,
             std::initializer_list<Delivery> vecs, int64_t rows = 1);

// Train and test points merged in time order: times tm, the data column ym (ycol on the train
// rows, 0 on the test rows), noise rm (s2 train / 1e10 test), with want_inputs the inputs vm
// (ld d), with want_pos the test points' merged rows pos, with want_tpos the training points'
// tpos.  Workspace names tag + "_tm", ...
struct MergedGrid {
  double *tm, *ym, *rm, *vm;
  int64_t* pos;
  int64_t nt, nch;
  int64_t* tpos;
};
MergedGrid merge_grid(gpar_ctx* c, const std::string& tag, const DevProblem& P, double s2,
                      const double* ts, int64_t n_star, const double* ycol, const double* vs,
                      int64_t ldvs, bool want_inputs, bool want_pos, const char* yname = "_ym",
                      bool want_tpos = false);

// The merged grid's gains, and the adjoint's fix-up rows h once something has computed them
// (fixup_rows).  gpar_posterior_prepare fills one ahead of the prediction (PredPrep).
struct GridGains {
  GainsOut g{};
  double* h = nullptr;
};
// The part of one output's prediction that does not read the inference inputs, queued ahead on
// the side stream (gpar_posterior_prepare): the merged grid's gains and the adjoint's fix-up
// vectors h for given test times.  A slot is consumed by the matching gpar_posterior_predict.
// A slot is matched by the posterior's unique id (never by its address, which a later
// gpar_fit_posterior may reuse after gpar_posterior_destroy), the output index and the test times.
struct PredPrep {
  uint64_t post_id = 0;
  int out = -1;
  const double* ts = nullptr;
  int64_t n_star = 0;
  GridGains gg{};
  bool valid = false;
};
// prep: the slot computed ahead (the stream waits for it); else run_gains under `tag`
GridGains grid_gains(gpar_ctx* c, int sdim, const ChainParamsHost& cp, const MergedGrid& grid,
                     const PredPrep* prep, const std::string& tag);
// gg.h, computed into workspace `name` (n x 4) if gg has none yet
double* fixup_rows(gpar_ctx* c, int sdim, GridGains& gg, int64_t n, int64_t nch,
                   const std::string& name);
// the prepared slot may be refilled once the prediction on c->stream has read it
void release_prep(gpar_ctx* c, const PredPrep* prep);

// mc whitened columns X (ld ldx) over the n steps of a grid and the four chunk-carry buffers of
// their Sigma^{-1} solve (workspace tag + "_send", ...): the caller's whitening fills X and send.
// wide: the many-column adjoint (wmask optional: u written at rows with wmask >= 1e10 only).
struct SigmaCols {
  double* X;
  int64_t ldx, mc, n, nch;
  bool wide;
  const double* wmask;
  double *send, *cin, *bend, *chat;
};
SigmaCols sigma_cols(gpar_ctx* c, const std::string& tag, double* X, int64_t ldx, int64_t mc,
                     int64_t n, bool wide, const double* wmask);
// Sigma^{-1} x = W^T (W x) on the whitened columns: forward carry, fix-up rows, local adjoint (u in
// place of X), reverse carry into s.chat.  ws_tag: the fix-up rows' workspace, run_tag: the
// carries'.  span (optional): a Timed span of `work` around exactly the adjoint launch.
// Returns the fix-up rows h.
double* sigma_inv_columns(gpar_ctx* c, int sdim, GridGains gg, const SigmaCols& s,
                          const std::string& ws_tag, const std::string& run_tag,
                          const char* span = nullptr, double work = 0.0);

// --------------------------------------------------------------------------- posterior paths
// The path draws of a seed are decorrelated from its q(u) draws (gpar_path_normals exports them).
constexpr uint64_t kPathSeedXor = 0x5851F42D4C957F2Dull;
inline uint64_t path_seed(uint64_t seed) { return seed ^ kPathSeedXor; }
void path_samples(gpar_ctx* c, int sdim, const GainsOut& g, const ChainParamsHost& cp,
                  const double* t, const double* noise, int64_t n, const double* ym,
                  const double* fx, int64_t ldfx, int S, uint64_t seed, double* F);

// --------------------------------------------------------------------------- predictions
inline void check_predict_mode(int mode, int samples) {
  ARGCHECK(mode == GPAR_PREDICT_ANALYTIC || mode == GPAR_PREDICT_MC || mode == GPAR_PREDICT_PATH,
           "bad mode");
  if (mode != GPAR_PREDICT_ANALYTIC)
    ARGCHECK(samples >= 2 && samples <= kMaxSamples, "MC / path modes take 2..65536 samples");
}
// defer (device memory only): the outputs are queued on c->stream but not waited for -- the caller
// synchronises (gpar_fit_predict's prediction lanes).
void predict_impl(gpar_ctx* c, const DevProblem& P, const Theta& th, int mem, int64_t n_star,
                  const double* t_star_in, const double* v_star_in, int64_t ldvs, int mode,
                  int samples, uint64_t seed, double* mean_out, double* std_out,
                  const GramCache* gc = nullptr, bool defer = false, const QuPre* pre = nullptr,
                  const PredPrep* prep = nullptr);
// The ANALYTIC mean of predict_impl without its variance: f = Cf*u w by launch_kfu_gemv and a
// one-column smoother of y* - f on the merged grid, O((n + n*) m d) work and O(n + n*) workspace.
// xtr (optional): the training rows' y - Kfu w (kfu_train_residual), which depends only on the
// posterior; null: computed here.  pre / prep / defer as predict_impl's.
void kfu_train_residual(gpar_ctx* c, const DevProblem& P, const Theta& th, const double* w,
                        double* xtr);
void predict_mean_impl(gpar_ctx* c, const DevProblem& P, const Theta& th, int mem, int64_t n_star,
                       const double* t_star_in, const double* v_star_in, int64_t ldvs,
                       double* mean_out, const GramCache* gc = nullptr, bool defer = false,
                       const QuPre* pre = nullptr, const PredPrep* prep = nullptr,
                       const double* xtr = nullptr);
// Sample-chained prediction: path mode (GPAR_PREDICT_PATH) with per-sample test inputs and the
// samples delivered.  Test row i of sample s sits at [v_sh_i (d_sh columns, ld ldvs) , v_sa_{s,i}
// (d_sa = P.d - d_sh columns at v_sa[s * ld_s + i * ld_r + .])]; the draws are path mode's for
// (samples, seed), so with d_sa = 0 this is predict_impl's path mode with its samples exposed.
// f_out[s * ldf_s + i * ldf_r] = sample s at test point i (the caller's row order); mean_out /
// std_out (either may be null): the sample mean and Bessel std, as path mode reduces them
// (samples = 1: the std is 0 / 0).  f_out may lie in the tensor v_sa points into, at a column this
// call does not read: everything is read before anything is delivered.  pre / prep as predict_impl's.
void predict_samples_impl(gpar_ctx* c, const DevProblem& P, const Theta& th, int mem,
                          int64_t n_star, const double* t_star_in, const double* v_sh_in,
                          int64_t ldvs, int64_t d_sh, const double* v_sa_in, int64_t ld_s,
                          int64_t ld_r, int samples, uint64_t seed, double* f_out, int64_t ldf_s,
                          int64_t ldf_r, double* mean_out, double* std_out,
                          const QuPre* pre = nullptr, const PredPrep* prep = nullptr);
// The argument checks gpar_predict_samples and gpar_posterior_predict_samples share (d: the
// problem's input dimension).
inline void check_sample_args(int64_t d, int64_t n_star, const double* t_star, const double* v_sh,
                              int64_t ldvs, int64_t d_sh, const double* v_sa, int64_t ld_s,
                              int64_t ld_r, int samples, const double* f_out, int64_t ldf_s,
                              int64_t ldf_r) {
  ARGCHECK(t_star && f_out, "null argument");
  ARGCHECK(n_star >= 1, "n_star must be >= 1");
  ARGCHECK(d_sh >= 0 && d_sh <= d, "d_shared must be in 0..d");
  const int64_t d_sa = d - d_sh;
  ARGCHECK(d_sh == 0 || v_sh, "null v_shared with d_shared > 0");
  ARGCHECK(d_sa == 0 || v_sa, "null v_samp with d - d_shared > 0");
  ARGCHECK(d_sh == 0 || ldvs >= d_sh, "ldvs must be >= d_shared");
  ARGCHECK(d_sa == 0 || (ld_r >= d_sa && ld_s >= (n_star - 1) * ld_r + d_sa),
           "sample strides: ld_r must be >= d - d_shared and ld_s >= (n_star - 1) ld_r + d - d_shared");
  ARGCHECK(ldf_r >= 1 && ldf_s >= (n_star - 1) * ldf_r + 1,
           "output strides: ldf_r must be >= 1 and ldf_s >= (n_star - 1) ldf_r + 1");
  ARGCHECK(samples >= 1 && samples <= kMaxSamples, "samples must be in 1..65536");
}
// Device bytes of a prediction's workspace (what gpar_fit_predict reserves beside the fit's cache)
int64_t predict_ws_estimate(int64_t n, int64_t n_star, int64_t mp, int64_t d, int mode,
                            int samples, bool fused);
int64_t predict_mean_ws_estimate(int64_t n, int64_t n_star, int64_t mp, int64_t d);
// host: the sample inputs and the delivered samples are staged on the device too
int64_t predict_samples_ws_estimate(int64_t n, int64_t n_star, int64_t mp, int64_t d_sh,
                                    int64_t d_sa, int samples, bool host);

}  // namespace gpar
