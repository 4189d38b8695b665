// span.hpp -- the "corr_span" plan (include/gpar_hip.h): S consecutive 256-step chunks filtered
// from one zero state by the fit's cached whitening.  The small host / device arithmetic that the
// whitening, the span kernels (k_span.hip) and the host plan share, so that they cannot disagree:
// span counts, the closed-loop transitions composed over a span, the default rule.
#pragma once
#include <cstdint>

#ifndef GPAR_HD   // (nm_dev.hpp defines the same)
#if defined(__HIPCC__)
#define GPAR_HD __host__ __device__
#else
#define GPAR_HD
#endif
#endif

namespace gpar {

constexpr int kMaxCorrSpan = 8;
// the span a split fit takes on its own (corr_span = -1): profiles/ab_corr_span.txt
constexpr int kCorrSpanAuto = 2;

GPAR_HD inline bool corr_span_valid(int s) { return s == 1 || s == 2 || s == 4 || s == 8; }

// spans of S chunks covering nch chunks (the last may be partial)
GPAR_HD inline int64_t span_count(int64_t nch, int s) { return (nch + s - 1) / s; }

// The knob resolved for one batch: a set value as it is; auto takes kCorrSpanAuto where the
// default CU split applies by its own size gate in a fit call too large for the round overlap
// (big: n mp^2 >= kSplitMinWork and at least kCorrSpanAutoMinOutputs outputs, host.hpp), else 1.
GPAR_HD inline int corr_span_resolve(int knob, bool split, bool big) {
  if (knob >= 1) return knob;
  return split && big ? kCorrSpanAuto : 1;
}

// P <- F P (row-major d x d): the transition over the chunks so far, extended by chunk
// transition F.  cin[j + 1] = Phi_j cin[j] + send[j] (carry kernels), so the state at the start of
// the span's chunk i is Psi_i c + (span-local state), Psi_0 = I, Psi_{i + 1} = Phi_i Psi_i.
template <int D>
GPAR_HD inline void span_compose(const double* f, double (&p)[D][D]) {
  double x[D][D];
  for (int i = 0; i < D; ++i)
    for (int q = 0; q < D; ++q) {
      double acc = 0.0;
      for (int r = 0; r < D; ++r) acc += f[i * D + r] * p[r][q];
      x[i][q] = acc;
    }
  for (int i = 0; i < D; ++i)
    for (int q = 0; q < D; ++q) p[i][q] = x[i][q];
}

// One span of a chain: pre[i] = Psi_i for its cnt chunks (phi: their transitions, d x d each),
// tot = Psi_cnt, the span's own transition.
template <int D>
GPAR_HD inline void span_psi(const double* phi, int cnt, double* pre, double* tot) {
  double p[D][D];
  for (int i = 0; i < D; ++i)
    for (int q = 0; q < D; ++q) p[i][q] = i == q ? 1.0 : 0.0;
  for (int c = 0; c < cnt; ++c) {
    for (int i = 0; i < D; ++i)
      for (int q = 0; q < D; ++q) pre[c * D * D + i * D + q] = p[i][q];
    span_compose<D>(phi + c * D * D, p);
  }
  for (int i = 0; i < D; ++i)
    for (int q = 0; q < D; ++q) tot[i * D + q] = p[i][q];
}

}  // namespace gpar
