// k_span.hip -- the span-granular short chain of the "corr_span" plan (span.hpp; gfx950).
//
// With corr_span = S > 1 the fit's cached whitening (whiten_kfu_d2x2<.., SPAN = true>, k_dist.hip)
// filters S consecutive chunks from one zero state, so beta_loc is local to the SPAN: the true
// beta_k = beta_loc,k + g'_k C_J^T with C_J the filter states at the start of span J and
// g'_k = g_k Psi_i for a step of the span's chunk i (g_k counts its transition from the chunk start,
// k_lgssm.hip; Psi_i carries it back to the span start).  The Gram's correction (k_gram.hip) then
// runs over ceil(nch / S) spans with
//   W_J = sum_{k in J} g'_k^T g'_k,  q_J = sum_{k in J} g'_k alpha_k,  E_J = H_J + W_J C_J / 2,
// H_J summed by the whitening itself.  alpha keeps its 256-step chunks and a carry of its own: it
// is fixed in place here, chunk by chunk, before it enters q_J.
#include "device_common.hpp"
#include "span.hpp"

namespace gpar {

// pre[j] = Psi_i of chunk j = J S + i, tot[J] = the span's transition; one thread per span.
template <int D>
__global__ __launch_bounds__(256) void span_psi_kernel(const double* __restrict__ phi, int64_t nch,
                                                       int span, double* __restrict__ pre,
                                                       double* __restrict__ tot) {
  const int64_t J = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t j0 = J * span;
  if (j0 >= nch) return;
  const int cnt = (int)(j0 + span <= nch ? span : nch - j0);
  span_psi<D>(phi + j0 * D * D, cnt, pre + j0 * D * D, tot + J * D * D);
}

// vec_fix (k_lgssm.hip) for a span: one 256-thread block per span walks its chunks.  Per chunk j:
// alpha[k] += g_k . acin[j] (alpha's own chunk carry) and the chunk's sum of alpha^2 -> part[j],
// summed as vec_fix sums it.  Over the span: W_J, q_J -> qout[J], E_J in place of H_J (hsum), for
// the ncols beta columns, from the span states cin[J].
template <int D>
__global__ __launch_bounds__(256) void vec_fix_span(
    double* __restrict__ alpha, const double* __restrict__ g, const double* __restrict__ acin,
    const double* __restrict__ pre, const double* __restrict__ cin, int64_t mc, int64_t n,
    int span, int64_t nch, double* __restrict__ part, double* __restrict__ hsum, int64_t ncols,
    double* __restrict__ qout) {
  constexpr int NW = D * (D + 1) / 2;   // packed upper triangle of W
  constexpr int NV = NW + D;            // W | q
  __shared__ double a2[4];
  __shared__ double red[4][NV];
  __shared__ double wq[NV];
  const int64_t J = blockIdx.x;
  double vals[NV];
#pragma unroll
  for (int e = 0; e < NV; ++e) vals[e] = 0.0;
  for (int i = 0; i < span; ++i) {
    const int64_t j = J * span + i;
    if (j >= nch) break;
    const int64_t k = j * 256 + threadIdx.x;
    double a2v = 0.0;
    if (k < n) {
      const double* gp = g + k * kGStride;
      const double* cp = acin + j * kSStride;
      const double* ps = pre + j * D * D;
      double a = alpha[k];
      double gk[D], gq[D];
#pragma unroll
      for (int q = 0; q < D; ++q) {
        gk[q] = gp[q];
        a = fma(gk[q], cp[q], a);
      }
      alpha[k] = a;
      a2v = a * a;
#pragma unroll
      for (int q = 0; q < D; ++q) {
        double acc = 0.0;
#pragma unroll
        for (int r = 0; r < D; ++r) acc = fma(gk[r], ps[r * D + q], acc);
        gq[q] = acc;
      }
      int e = 0;
#pragma unroll
      for (int q = 0; q < D; ++q)
#pragma unroll
        for (int r = q; r < D; ++r) {
          vals[e] = fma(gq[q], gq[r], vals[e]);
          ++e;
        }
#pragma unroll
      for (int q = 0; q < D; ++q) vals[NW + q] = fma(gq[q], a, vals[NW + q]);
    }
    const double v = wave_sum(a2v);
    if ((threadIdx.x & 63) == 0) a2[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) part[j] = ((a2[0] + a2[1]) + a2[2]) + a2[3];
    __syncthreads();
  }
  for (int e = 0; e < NV; ++e) {
    const double v = wave_sum(vals[e]);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][e] = v;
  }
  __syncthreads();
  if (threadIdx.x < NV)
    wq[threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) +
                      red[3][threadIdx.x];
  __syncthreads();
  if (threadIdx.x < 4) qout[J * 4 + threadIdx.x] = threadIdx.x < D ? wq[NW + threadIdx.x] : 0.0;
  double W[D][D];
  {
    int e = 0;
#pragma unroll
    for (int q = 0; q < D; ++q)
#pragma unroll
      for (int r = q; r < D; ++r) {
        W[q][r] = wq[e];
        W[r][q] = wq[e];
        ++e;
      }
  }
  for (int64_t c = threadIdx.x; c < ncols; c += 256) {
    const double* cp = cin + (J * mc + c) * kSStride;
    double* hp = hsum + (J * mc + c) * kSStride;
    double cv[D], ev[D];
#pragma unroll
    for (int q = 0; q < D; ++q) cv[q] = cp[q];
#pragma unroll
    for (int q = 0; q < D; ++q) {
      double acc = 0.0;
#pragma unroll
      for (int r = 0; r < D; ++r) acc = fma(W[q][r], cv[r], acc);
      ev[q] = fma(0.5, acc, hp[q]);
    }
#pragma unroll
    for (int q = 0; q < kSStride; ++q) hp[q] = q < D ? ev[q] : 0.0;
  }
}

}  // namespace gpar

// ============================================================================ launch wrappers
#include "launch.hpp"

namespace gpar {

#define GPAR_SPAN_D(D, ...)                                       \
  switch (D) {                                                    \
    case 1: { constexpr int DD = 1; __VA_ARGS__; } break;         \
    case 2: { constexpr int DD = 2; __VA_ARGS__; } break;         \
    default: { constexpr int DD = 3; __VA_ARGS__; } break;        \
  }

void launch_span_psi(hipStream_t st, int sdim, const double* phi, int64_t nch, int span,
                     double* pre, double* tot) {
  const int64_t nsp = span_count(nch, span);
  if (nsp <= 0) return;
  GPAR_SPAN_D(sdim, span_psi_kernel<DD><<<(unsigned)((nsp + 255) / 256), 256, 0, st>>>(
                        phi, nch, span, pre, tot));
}

void launch_vec_fix_span(hipStream_t st, int sdim, double* alpha, const double* g,
                         const double* acin, const double* pre, const double* cin, int64_t mc,
                         int64_t n, int span, int64_t nch, double* part, double* hsum,
                         int64_t ncols, double* qout) {
  const int64_t nsp = span_count(nch, span);
  if (nsp <= 0) return;
  GPAR_SPAN_D(sdim, vec_fix_span<DD><<<(unsigned)nsp, 256, 0, st>>>(
                        alpha, g, acin, pre, cin, mc, n, span, nch, part, hsum, ncols, qout));
}
#undef GPAR_SPAN_D

}  // namespace gpar
