// k_kfu_gemv.hip -- f = Kfu w with the kernel matrix evaluated on the fly (gfx950), and the
// finish of the mean-only prediction.
//
// The mean of a scaled-GPAR prediction needs Cf*u only through the vector f = Cf*u U_u^{-1} m_e
// (gpar_scaled_inference.jl:89-97): with w = U_u^{-1} m_e,
//
//   f_k = sum_c s_o kappa(|v_k - z_c| / l_o) w_c
//
// is one kernel-matrix--vector product, O(n M D), and no n x Mp matrix is ever written.  A
// workgroup owns its rows across ALL column tiles and adds their contributions in tile order, the
// columns of a tile in a fixed lane order: no atomics, the result of a row does not depend on the
// grid.  Smooth output kernels take their distances in the Gram form of dist2_mfma_kernel
// (k_dist.hip: fp64 MFMA, centred per 256-column group, D streamed through LDS in 16-wide K-steps,
// so any D) and the s_o kappa . w epilogue runs on the accumulator tiles; Matern-1/2 takes direct
// differences (dist2_direct_kernel's reason).
//
// Outputs per row k < n: fout[k] = f_k (optional) and xout[dst(k)] = a y_k - f_k (optional; y
// null: 0), dst(k) = k or pos[k] -- the merged grid's positions (merge_side), so the test side
// writes y* - f straight into the merged data vector.
#include "device_common.hpp"

namespace gpar {

typedef double d4 __attribute__((ext_vector_type(4)));

// the tile of dist2_mfma_kernel: 128 rows x 128 columns per 256-thread workgroup, 2 x 2 waves of
// 4 x 4 v_mfma_f64_16x16x4_f64 tiles, K-step 16 double-buffered through LDS (k-major rows padded
// to kGvLds: the 16 lanes of a fragment read 16 consecutive doubles)
constexpr int kGvT = 128, kGvBK = 16, kGvLds = 136;

template <int OK>
__global__ __launch_bounds__(256, 2) void kfu_gemv_mfma(
    const double* __restrict__ v, int64_t ldv, int64_t n, const double* __restrict__ z,
    int64_t ldz, int64_t m, int d, const double* __restrict__ zc, int64_t zld,
    const double* __restrict__ w, double inv_lo, double s_o, const double* __restrict__ y,
    double a_y, const int64_t* __restrict__ pos, double* __restrict__ xout,
    double* __restrict__ fout, ExpNegConsts ek) {
  __shared__ __attribute__((aligned(16))) double smem[2 * 2 * kGvBK * kGvLds];
  __shared__ double vn_s[kGvT], zn_s[kGvT], w_s[kGvT];
  __shared__ double red[2 * kGvT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int64_t r0 = (int64_t)blockIdx.x * kGvT;
  const int srow = tid >> 1, sk = (tid & 1) * 8;
  const int64_t arow = r0 + srow;
  const bool av = arow < n;
  const int64_t arc = av ? arow : n - 1;
  const int frow = lane >> 4, fcol = lane & 15;
  const int nsteps = (d + kGvBK - 1) / kGvBK;
  // this lane's partial sums of its 16 rows over the columns it has seen (fcol, all tiles)
  double racc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int r = 0; r < 4; ++r) racc[a][r] = 0.0;
  for (int64_t c0 = 0; c0 < m; c0 += kGvT) {
    const double* cg = zc + (c0 >> 8) * zld;   // 128-column tiles never straddle a 256-group
    const int64_t brow = c0 + srow;
    const bool bv = brow < m;
    const int64_t brc = bv ? brow : m - 1;
    double ra[8], rb[8];
    double an = 0.0, bn = 0.0;
    auto load = [&](int k0) {
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int kk = k0 + sk + q;
        const int kc = kk < d ? kk : d - 1;
        const double g = cg[kc];
        const double a = v[arc * ldv + kc] - g;
        const double b = z[brc * ldz + kc] - g;
        ra[q] = (av && kk < d) ? a : 0.0;
        rb[q] = (bv && kk < d) ? b : 0.0;
        an = fma(ra[q], ra[q], an);
        bn = fma(rb[q], rb[q], bn);
      }
    };
    auto store = [&](int buf) {
      double* la = smem + (buf * 2 + 0) * kGvBK * kGvLds;
      double* lb = smem + (buf * 2 + 1) * kGvBK * kGvLds;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        la[(sk + q) * kGvLds + srow] = ra[q];
        lb[(sk + q) * kGvLds + srow] = rb[q];
      }
    };
    d4 acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[a][c] = d4{0.0, 0.0, 0.0, 0.0};
    load(0);
    store(0);
    __syncthreads();
    for (int s = 0; s < nsteps; ++s) {
      const int buf = s & 1;
      const bool more = s + 1 < nsteps;
      if (more) load((s + 1) * kGvBK);
      const double* la = smem + (buf * 2 + 0) * kGvBK * kGvLds;
      const double* lb = smem + (buf * 2 + 1) * kGvBK * kGvLds;
#pragma unroll
      for (int ks = 0; ks < kGvBK / 4; ++ks) {
        double fa[4], fb[4];
        const int kr = ks * 4 + frow;
#pragma unroll
        for (int a = 0; a < 4; ++a) fa[a] = la[kr * kGvLds + wr * 64 + a * 16 + fcol];
#pragma unroll
        for (int c = 0; c < 4; ++c) fb[c] = lb[kr * kGvLds + wc * 64 + c * 16 + fcol];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int c = 0; c < 4; ++c)
            acc[a][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[a], fb[c], acc[a][c], 0, 0, 0);
      }
      if (more) store(buf ^ 1);
      __syncthreads();
    }
    // row norms (the two staging threads of a row hold complementary halves of every K-step) and
    // the tile's w: zero past m, so the padding columns add nothing
    an += __shfl_xor(an, 1, 64);
    bn += __shfl_xor(bn, 1, 64);
    if ((tid & 1) == 0) {
      vn_s[srow] = an;
      zn_s[srow] = bn;
    }
    if (tid < kGvT) w_s[tid] = (c0 + tid < m) ? w[c0 + tid] : 0.0;
    __syncthreads();
    // epilogue on the accumulator tiles (C layout: lane holds rows frow + 4 r, column fcol of each
    // 16 x 16 tile): s_o kappa(d / l_o) w_c, summed over this lane's columns in tile order.
    // Evaluated for every column and selected after (padding columns: finite values, dropped)
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double vn = vn_s[wr * 64 + a * 16 + frow + 4 * r];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int cl = wc * 64 + c * 16 + fcol;
          double d2 = vn + zn_s[cl] - 2.0 * acc[a][c][r];
          if constexpr (OK == KEQ) d2 = d2 > 0.0 ? d2 : 0.0;
          const double kv = skappa_sq_k<OK>(d2, inv_lo, s_o, ek);
          racc[a][r] = fma((c0 + cl < m) ? kv : 0.0, w_s[cl], racc[a][r]);
        }
      }
    // (the next tile's first writes to vn_s / zn_s / w_s come after its K-loop's barriers)
  }
  // the 16 lanes sharing a row (fcol), then the two column halves (wc), in a fixed order
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) racc[a][r] += __shfl_xor(racc[a][r], off, 64);
      if (fcol == 0) red[wc * kGvT + wr * 64 + a * 16 + frow + 4 * r] = racc[a][r];
    }
  __syncthreads();
  if (tid < kGvT) {
    const int64_t row = r0 + tid;
    if (row < n) {
      const double f = red[tid] + red[kGvT + tid];
      if (fout) fout[row] = f;
      if (xout) xout[pos ? pos[row] : row] = (y ? a_y * y[row] : 0.0) - f;
    }
  }
}

// Matern-1/2: d2 = sum_i (v_k,i - z_c,i)^2 by direct differences (dist2_direct_kernel's layout:
// one column per thread, the tile's V rows staged through LDS 16 dimensions at a time and read
// back as broadcasts).  A workgroup owns kGdRows rows over all 256-column tiles; a thread adds
// its columns' terms per row in tile order, then the threads' sums are added in a fixed order.
constexpr int kGdRows = 32, kGdDim = 16;

__global__ __launch_bounds__(256) void kfu_gemv_direct(
    const double* __restrict__ v, int64_t ldv, int64_t n, const double* __restrict__ z,
    int64_t ldz, int64_t m, int d, const double* __restrict__ w, double inv_lo, double s_o,
    const double* __restrict__ y, double a_y, const int64_t* __restrict__ pos,
    double* __restrict__ xout, double* __restrict__ fout, ExpNegConsts ek) {
  __shared__ double vs[kGdRows][kGdDim + 1];
  __shared__ double red[4][kGdRows];
  const int tid = threadIdx.x;
  const int64_t k0 = (int64_t)blockIdx.x * kGdRows;
  double racc[kGdRows];
#pragma unroll
  for (int r = 0; r < kGdRows; ++r) racc[r] = 0.0;
  for (int64_t c0 = 0; c0 < m; c0 += 256) {
    const int64_t c = c0 + tid;
    const bool cv = c < m;
    const int64_t cc = cv ? c : 0;
    double acc[kGdRows];
#pragma unroll
    for (int r = 0; r < kGdRows; ++r) acc[r] = 0.0;
    for (int i0 = 0; i0 < d; i0 += kGdDim) {
      __syncthreads();
      for (int e = tid; e < kGdRows * kGdDim; e += 256) {
        const int r = e / kGdDim, i = e % kGdDim;
        const int64_t k = k0 + r;
        vs[r][i] = (k < n && i0 + i < d) ? v[k * ldv + i0 + i] : 0.0;
      }
      double zr[kGdDim];
#pragma unroll
      for (int i = 0; i < kGdDim; ++i) zr[i] = (i0 + i < d) ? z[cc * ldz + i0 + i] : 0.0;
      __syncthreads();
#pragma unroll
      for (int r = 0; r < kGdRows; ++r)
#pragma unroll
        for (int i = 0; i < kGdDim; ++i) {
          const double a = vs[r][i] - zr[i];   // dimensions past d: 0 - 0
          acc[r] = fma(a, a, acc[r]);
        }
    }
    const double wc = cv ? w[c] : 0.0;
#pragma unroll
    for (int r = 0; r < kGdRows; ++r) {
      const double kv = skappa_sq_k<KM12>(acc[r], inv_lo, s_o, ek);
      racc[r] = fma(cv ? kv : 0.0, wc, racc[r]);
    }
  }
#pragma unroll
  for (int r = 0; r < kGdRows; ++r) {
    const double s = wave_sum(racc[r]);
    if ((tid & 63) == 0) red[tid >> 6][r] = s;
  }
  __syncthreads();
  if (tid < kGdRows) {
    const int64_t row = k0 + tid;
    if (row < n) {
      const double f = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
      if (fout) fout[row] = f;
      if (xout) xout[pos ? pos[row] : row] = (y ? a_y * y[row] : 0.0) - f;
    }
  }
}

// ---------------------------------------------------------------------------- mean-only finish
// mean_i = f_k + x_k - R_k (Sigma^{-1} x)_k at the test rows k = pos[i] only, x = y* - f the
// smoothed column, (Sigma^{-1} x)_k = u_k + h_k . chat_{chunk(k)} (u: the one-column adjoint's
// output): the last-lane arithmetic of predict_rows on the single column.  f_k + x_k first: at a
// test row x_k = 0 - f_k, so the sum is exact.
template <int D>
__global__ __launch_bounds__(256) void mean_finish(const double* __restrict__ u,
                                                   const double* __restrict__ h,
                                                   const double* __restrict__ chat,
                                                   const double* __restrict__ x,
                                                   const double* __restrict__ rm,
                                                   const double* __restrict__ fstar,
                                                   const int64_t* __restrict__ pos, int64_t nstar,
                                                   int L, double* __restrict__ mean) {
  const int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x;
  if (i >= nstar) return;
  const int64_t k = pos[i];
  const int64_t j = k >> __builtin_ctz(L);   // L is a power of two (kChunk)
  double uu = u[k];
#pragma unroll
  for (int q = 0; q < D; ++q) uu = fma(h[k * kGStride + q], chat[j * kSStride + q], uu);
  mean[i] = fma(-rm[k], uu, fstar[i] + x[k]);
}

}  // namespace gpar

// ============================================================================ launch wrappers
#include "launch.hpp"

namespace gpar {

void launch_kfu_gemv(hipStream_t st, int out_kind, const double* v, int64_t ldv, int64_t n,
                     const double* z, int64_t ldz, int64_t m, int d, const double* zc,
                     const double* w, double inv_lo, double s_o, const double* y, double a_y,
                     const int64_t* pos, double* xout, double* fout) {
  if (n <= 0) return;
  if (out_kind == KM12) {
    kfu_gemv_direct<<<(unsigned)((n + kGdRows - 1) / kGdRows), 256, 0, st>>>(
        v, ldv, n, z, ldz, m, d, w, inv_lo, s_o, y, a_y, pos, xout, fout, exp_neg_consts());
    return;
  }
  const unsigned grid = (unsigned)((n + kGvT - 1) / kGvT);
#define GV_ARGS v, ldv, n, z, ldz, m, d, zc, zc_stride(d), w, inv_lo, s_o, y, a_y, pos, xout, fout, exp_neg_consts()
  switch (out_kind) {
    case KM32: kfu_gemv_mfma<KM32><<<grid, 256, 0, st>>>(GV_ARGS); break;
    case KEQ: kfu_gemv_mfma<KEQ><<<grid, 256, 0, st>>>(GV_ARGS); break;
    default: kfu_gemv_mfma<KM52><<<grid, 256, 0, st>>>(GV_ARGS); break;
  }
#undef GV_ARGS
}

void launch_mean_finish(hipStream_t st, int sdim, const double* u, const double* h,
                        const double* chat, const double* x, const double* rm,
                        const double* fstar, const int64_t* pos, int64_t nstar, int L,
                        double* mean) {
  const unsigned grid = (unsigned)((nstar + 255) / 256);
  switch (sdim) {
    case 1: mean_finish<1><<<grid, 256, 0, st>>>(u, h, chat, x, rm, fstar, pos, nstar, L, mean); break;
    case 2: mean_finish<2><<<grid, 256, 0, st>>>(u, h, chat, x, rm, fstar, pos, nstar, L, mean); break;
    default: mean_finish<3><<<grid, 256, 0, st>>>(u, h, chat, x, rm, fstar, pos, nstar, L, mean); break;
  }
}

}  // namespace gpar
