// host_posterior.cpp -- posterior objects: the fit and q(u) of a batch kept for later predictions,
// the part of a prediction that can be queued ahead of its inference inputs, and their entries.
#include "host.hpp"

#include <atomic>

// gpar_fit_posterior keeps, per output, everything get_gpar_scaled_predictions computes before it
// reads the inference inputs (gpar_scaled_inference.jl:20-73: the fit and q(u), :141-196), so a
// caller whose inference inputs arrive later -- the chained sweep of GPAR_scaled_examples.jl:172,
// eeg.jl:249,274, one owner per output across ranks -- runs only the V*-dependent prediction per
// output (gpar_posterior_predict).
struct gpar_posterior {
  // unique over the process's lifetime: gpar_posterior_prepare's slots match on it, so a slot left
  // by a destroyed posterior can never be taken for a new one at the same address
  uint64_t id = 0;
  int device = 0;
  int mem = GPAR_MEM_DEVICE;   // memory space of the problems (and of every predict call's I/O)
  struct Out {
    gpar::DevProblem p;        // t, v, z, y: borrowed (device problems) or owned (host problems)
    gpar::Theta th;
    gpar::QuPre q;             // me, w, X1, Vm, cov in owned device memory
    // the mean-only prediction's training rows y - Kfu w (n doubles, owned), filled on first use
    // (post_xtr); xtr_ev: recorded behind the fill when it ran on the side stream
    // (gpar_posterior_prepare_mean), and waited for by every reader on the context stream
    mutable const double* xtr = nullptr;
    mutable hipEvent_t xtr_ev = nullptr;
  };
  std::vector<Out> outs;
  mutable std::vector<void*> owned;   // hipMalloc'd blocks, freed by gpar_posterior_destroy
  ~gpar_posterior() {
    (void)hipSetDevice(device);
    for (const Out& o : outs)
      if (o.xtr_ev) (void)hipEventDestroy(o.xtr_ev);
    for (void* b : owned) (void)hipFree(b);
  }
};

namespace gpar {

static double* post_alloc(const gpar_posterior* post, size_t doubles) {
  void* b = nullptr;
  const hipError_t e = hipMalloc(&b, std::max<size_t>(doubles, 1) * sizeof(double));
  if (e != hipSuccess) {
    (void)hipGetLastError();
    throw Error(e == hipErrorOutOfMemory ? GPAR_ERR_OOM : GPAR_ERR_HIP,
                std::string("gpar_fit_posterior: hipMalloc: ") + hipGetErrorString(e));
  }
  post->owned.push_back(b);
  return reinterpret_cast<double*>(b);
}

// device copy of `doubles` doubles on the context stream into posterior-owned memory
static const double* post_keep(gpar_ctx* c, gpar_posterior* post, const double* src, size_t doubles) {
  double* dst = post_alloc(post, doubles);
  HIPCHECK(hipMemcpyAsync(dst, src, doubles * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  return dst;
}

// Output i's training rows y - Kfu w of the mean-only prediction, computed on c->stream on first
// use and kept by the posterior (the same kernel either way: a later call finds the bits it would
// have computed).  on_side: c->stream is the side stream, so an event orders the readers.
static const double* post_xtr(gpar_ctx* c, const gpar_posterior* post, int i, bool on_side) {
  const gpar_posterior::Out& o = post->outs[i];
  if (o.xtr) return o.xtr;
  double* x = post_alloc(post, o.p.n);
  kfu_train_residual(c, o.p, o.th, o.q.w, x);
  if (on_side) {
    if (!o.xtr_ev) HIPCHECK(hipEventCreateWithFlags(&o.xtr_ev, hipEventDisableTiming));
    HIPCHECK(hipEventRecord(o.xtr_ev, c->stream));
  }
  o.xtr = x;
  return x;
}

// What gpar_posterior_prepare queues on the side stream for output i and test times t_star (the
// merged grid's gains and fix-up rows into the next of the context's two slots); with_f: also
// the output's training rows of the mean-only prediction, if the posterior has none yet.
static void posterior_prepare(gpar_ctx* ctx, const gpar_posterior* post, int32_t i, int64_t n_star,
                              const double* t_star, bool with_f) {
  const gpar_posterior::Out& o = post->outs[i];
  const DevProblem& P = o.p;
  if (ctx->prep.empty()) ctx->prep.resize(2);
  for (int k = 0; k < 2; ++k)
    for (hipEvent_t* ev : {&ctx->ev_prep_ready[k], &ctx->ev_prep_free[k]})
      if (!*ev) HIPCHECK(hipEventCreateWithFlags(ev, hipEventDisableTiming));
  const int slot = ctx->prep_next;
  ctx->prep_next ^= 1;
  PredPrep& s = ctx->prep[slot];
  s.valid = false;
  // the side stream follows the context stream (inputs, earlier calls) and the slot's last reader
  HIPCHECK(hipEventRecord(ctx->ev_fork, ctx->main));
  HIPCHECK(hipStreamWaitEvent(ctx->side, ctx->ev_fork, 0));
  HIPCHECK(hipStreamWaitEvent(ctx->side, ctx->ev_prep_free[slot], 0));
  const std::string tag = "prep" + std::to_string(slot);
  {
    OnStream on_(ctx, ctx->side);
    if (with_f) post_xtr(ctx, post, i, /*on_side=*/true);
    // the merged grid's times and noise (predict_impl merges the inputs again, identically)
    const double s2 = o.th.sigma * o.th.sigma;
    const MergedGrid grid = merge_grid(ctx, tag, P, s2, t_star, n_star, P.y, nullptr, 0,
                                       /*want_inputs=*/false, /*want_pos=*/false);
    check_launch("prepare: merge");
    s.gg = grid_gains(ctx, P.sdim, chain_params_of(o.th, s2), grid, nullptr, tag);
    fixup_rows(ctx, P.sdim, s.gg, grid.nt, grid.nch, tag + "_h");
    check_launch("prepare: gains");
    HIPCHECK(hipEventRecord(ctx->ev_prep_ready[slot], ctx->side));
  }
  s.post_id = post->id;
  s.out = i;
  s.ts = t_star;
  s.n_star = n_star;
  s.valid = true;
}

// the slot gpar_posterior_prepare[_mean] filled for this output and these test times, taken
static const PredPrep* take_prep(gpar_ctx* ctx, const gpar_posterior* post, int32_t i,
                                 int64_t n_star, const double* t_star) {
  const PredPrep* prep = nullptr;
  for (PredPrep& s : ctx->prep)
    if (s.valid && s.post_id == post->id && s.out == i && s.ts == t_star && s.n_star == n_star) {
      s.valid = false;
      prep = &s;
    }
  return prep;
}

// Output i of a posterior for a call on ctx with n_star test points, checked.  prepare_entry (the
// prepare entries, by name): device-memory posteriors only.
static const gpar_posterior::Out& posterior_output(gpar_ctx* ctx, const gpar_posterior* post,
                                                   int32_t i, int64_t n_star,
                                                   const char* prepare_entry = nullptr) {
  ARGCHECK(post->device == ctx->device, "the posterior belongs to another device's context");
  if (prepare_entry)
    ARGCHECK(post->mem == GPAR_MEM_DEVICE, std::string(prepare_entry) + ": device-memory posteriors only");
  ARGCHECK(i >= 0 && i < (int32_t)post->outs.size(), "output index out of range");
  ARGCHECK(n_star >= 1, "n_star must be >= 1");
  return post->outs[i];
}

}  // namespace gpar

using namespace gpar;
extern "C" {

int32_t gpar_fit_posterior(gpar_ctx* ctx, const gpar_problem* probs, int32_t nprob,
                           const double* log_theta0, const gpar_fit_options* opts,
                           double* theta_out, double* nlml_out, int32_t* evals_out,
                           gpar_posterior** out) {
  if (out) *out = nullptr;
  std::unique_ptr<gpar_posterior> post;
  API_BEGIN(ctx)
  ARGCHECK(probs && nprob >= 1 && log_theta0 && theta_out && out, "null argument");
  check_batch(probs, nprob);
  gpar_fit_options o{0, 1000, 1e-8, 0.0};
  if (opts) o = *opts;
  const std::vector<DevProblem> P = prepare_batch(ctx, probs, nprob);
  FitKeep keep;
  fit_impl(ctx, P, log_theta0, o, theta_out, nlml_out, evals_out, &keep);
  post.reset(new gpar_posterior());
  static std::atomic<uint64_t> next_id{1};
  post->id = next_id.fetch_add(1);
  post->device = ctx->device;
  post->mem = probs[0].mem;
  post->outs.resize(nprob);
  const std::vector<Theta> T = thetas_from(theta_out, nprob);
  for (int i = 0; i < nprob; ++i) post->outs[i].th = T[i];
  // q(u) batched per convention (run_q_u_batch takes one), each batch copied out of the workspace
  // before the next overwrites it
  for (int qn : {0, 1}) {
    std::vector<int> idx;
    for (int i = 0; i < nprob; ++i)
      if (P[i].qu_noise == qn) idx.push_back(i);
    if (idx.empty()) continue;
    std::vector<DevProblem> Pq;
    std::vector<Theta> Tq;
    FitKeep kq;
    for (int i : idx) {
      Pq.push_back(P[i]);
      Tq.push_back(post->outs[i].th);
      kq.gram.push_back(keep.gram[i]);
      kq.valid.push_back(keep.valid[i]);
    }
    std::vector<QuPre> pre = run_q_u_batch(ctx, Pq, Tq, kq, /*want_cov=*/true);
    for (size_t a = 0; a < idx.size(); ++a) {
      const QuPre& s = pre[a];
      const size_t sq = (size_t)s.ld * s.ld;
      QuPre& d = post->outs[idx[a]].q;
      d = s;
      d.Lu = d.LD = nullptr;   // prediction reads w, X1, Vm (and me, cov: MC / path) only
      d.me = post_keep(ctx, post.get(), s.me, s.ld);
      d.w = post_keep(ctx, post.get(), s.w, s.ld);
      d.X1 = post_keep(ctx, post.get(), s.X1, sq);
      d.Vm = post_keep(ctx, post.get(), s.Vm, sq);
      d.cov = post_keep(ctx, post.get(), s.cov, sq);
    }
    sync(ctx);
  }
  // the problems: device inputs stay the caller's (borrowed until gpar_posterior_destroy); host
  // inputs were uploaded into workspace that later calls reuse, so they are copied (a time grid or
  // input base several outputs share, once)
  std::unordered_map<const double*, const double*> shared;
  auto keep_once = [&](const double* src, size_t doubles) {
    auto it = shared.find(src);
    if (it != shared.end()) return it->second;
    const double* dst = post_keep(ctx, post.get(), src, doubles);
    shared[src] = dst;
    return dst;
  };
  for (int i = 0; i < nprob; ++i) {
    DevProblem d = P[i];
    d.d2 = nullptr;   // the fit's distance cache is not the posterior's
    d.cache_slot = -1;
    d.zc = post_keep(ctx, post.get(), P[i].zc, (size_t)((d.mp + 255) / 256) * zc_stride((int)d.d));
    if (probs[0].mem == GPAR_MEM_HOST) {
      d.t = keep_once(P[i].t, d.n);
      d.y = post_keep(ctx, post.get(), P[i].y, d.n);
      d.v = keep_once(P[i].v, (size_t)d.n * d.ldv);
      d.z = post_keep(ctx, post.get(), P[i].z, (size_t)d.m * d.ldz);
    }
    post->outs[i].p = d;
  }
  sync(ctx);
  *out = post.release();
  API_END(ctx)
}

// gpar_posterior_prepare and gpar_posterior_prepare_mean (entry: the name the error text carries)
static int32_t prepare_entry(gpar_ctx* ctx, const gpar_posterior* post, int32_t i, int64_t n_star,
                             const double* t_star, bool with_f, const char* entry) {
  API_BEGIN(ctx)
  ARGCHECK(post && t_star, "null argument");
  posterior_output(ctx, post, i, n_star, entry);
  posterior_prepare(ctx, post, i, n_star, t_star, with_f);
  API_END(ctx)
}

int32_t gpar_posterior_prepare(gpar_ctx* ctx, const gpar_posterior* post, int32_t i,
                               int64_t n_star, const double* t_star) {
  return prepare_entry(ctx, post, i, n_star, t_star, /*with_f=*/false, "gpar_posterior_prepare");
}

int32_t gpar_posterior_prepare_mean(gpar_ctx* ctx, const gpar_posterior* post, int32_t i,
                                    int64_t n_star, const double* t_star) {
  return prepare_entry(ctx, post, i, n_star, t_star, /*with_f=*/true, "gpar_posterior_prepare_mean");
}

int32_t gpar_posterior_predict_mean(gpar_ctx* ctx, const gpar_posterior* post, int32_t i,
                                    int64_t n_star, const double* t_star, const double* v_star,
                                    int64_t ldvs, double* mean) {
  API_BEGIN(ctx)
  ARGCHECK(post && t_star && v_star && mean, "null argument");
  const gpar_posterior::Out& o = posterior_output(ctx, post, i, n_star);
  ARGCHECK(ldvs >= o.p.d, "ldvs must be >= d");
  const PredPrep* prep = take_prep(ctx, post, i, n_star, t_star);
  const double* xtr = post_xtr(ctx, post, i, /*on_side=*/false);
  if (o.xtr_ev) HIPCHECK(hipStreamWaitEvent(ctx->stream, o.xtr_ev, 0));
  predict_mean_impl(ctx, o.p, o.th, post->mem, n_star, t_star, v_star, ldvs, mean, nullptr, false,
                    &o.q, prep, xtr);
  API_END(ctx)
}

int32_t gpar_posterior_predict(gpar_ctx* ctx, const gpar_posterior* post, int32_t i,
                               int64_t n_star, const double* t_star, const double* v_star,
                               int64_t ldvs, int32_t mode, int32_t samples, uint64_t seed,
                               double* mean, double* std) {
  API_BEGIN(ctx)
  ARGCHECK(post && t_star && v_star && mean && std, "null argument");
  const gpar_posterior::Out& o = posterior_output(ctx, post, i, n_star);
  ARGCHECK(ldvs >= o.p.d, "ldvs must be >= d");
  check_predict_mode(mode, samples);
  const PredPrep* prep = take_prep(ctx, post, i, n_star, t_star);
  predict_impl(ctx, o.p, o.th, post->mem, n_star, t_star, v_star, ldvs, mode, samples, seed, mean,
               std, nullptr, false, &o.q, prep);
  API_END(ctx)
}

int32_t gpar_posterior_predict_samples(gpar_ctx* ctx, const gpar_posterior* post, int32_t i,
                                       int64_t n_star, const double* t_star,
                                       const double* v_shared, int64_t ldvs, int64_t d_shared,
                                       const double* v_samp, int64_t ld_s, int64_t ld_r,
                                       int32_t samples, uint64_t seed, double* f_out,
                                       int64_t ldf_s, int64_t ldf_r, double* mean, double* std) {
  API_BEGIN(ctx)
  ARGCHECK(post, "null argument");
  const gpar_posterior::Out& o = posterior_output(ctx, post, i, n_star);
  check_sample_args(o.p.d, n_star, t_star, v_shared, ldvs, d_shared, v_samp, ld_s, ld_r, samples,
                    f_out, ldf_s, ldf_r);
  const PredPrep* prep = take_prep(ctx, post, i, n_star, t_star);
  predict_samples_impl(ctx, o.p, o.th, post->mem, n_star, t_star, v_shared, ldvs, d_shared, v_samp,
                       ld_s, ld_r, samples, seed, f_out, ldf_s, ldf_r, mean, std, &o.q, prep);
  API_END(ctx)
}

int32_t gpar_posterior_destroy(gpar_posterior* post) {
  delete post;
  return GPAR_OK;
}

}  // extern "C"
