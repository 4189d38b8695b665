// k_kfu_samples.hip -- FX = Cf*u applied to S pseudo-point samples when every sample has its own
// test inputs (gfx950): the new stage of the sample-chained prediction (predict_samples_impl).
//
// A joint draw of GPAR's outputs feeds sample s of the earlier outputs into sample s of the later
// ones, so test row i of sample s sits at the input [vsh_i , vsa_{s,i}] (d_sh columns shared by all
// samples, d_sa columns of its own) and
//
//   FX[pos[i] * ldfx + s] = sum_c s_o kappa(|[vsh_i , vsa_{s,i}] - z_c| / l_o) Bm[s * ldb + c]
//
// with Bm the u-sample loadings of path_bmat.  That is S kernel matrices of N* x M, none of which
// is ever written: a workgroup owns kSfR test rows over ALL column tiles and ALL samples, a z
// column tile staged in LDS serves every sample of the row tile, and
//
//   d2 = (|a_sh|^2 + |b_sh|^2 - 2 a_sh.b_sh) + (|a_sa|^2 + |b_sa|^2 - 2 a_sa.b_sa)
//
// (a, b: the row's and the column's inputs less the 256-column group's centre, dist2_mfma_kernel's
// Gram form) splits into the shared columns' part, computed ONCE per (row tile, column tile) and
// kept folded in registers, and the sample columns' part, one fp64 MFMA contraction per sample.
// The sum over c runs in a fixed order -- the lane's four columns of a tile, the 16 lanes of a row,
// the two column halves, the tiles in order, each tile's partial added to FX by the one thread that
// owns the row -- with no atomics: the value of (i, s) depends neither on the grid, nor on S, nor
// on another sample's inputs.  Matern-1/2 takes direct differences (dist2_direct_kernel's reason).
// Sample element (s, i, q) is read at vsa[s * ld_s + perm[i] * ld_r + q] (perm: the test-time sort
// permutation, null = identity), so the caller's tensor is gathered in place, never copied.
#include "device_common.hpp"

namespace gpar {

typedef double d4 __attribute__((ext_vector_type(4)));

// 64 rows x 128 columns per 256-thread workgroup: 2 x 2 waves of 2 x 4 v_mfma_f64_16x16x4_f64
// tiles.  The accumulators are held twice (the folded shared part and the running sample): 2 x 32
// doubles = 128 VGPRs, which is what fixes the row tile at 64 under two workgroups per CU.  Inputs
// are staged k-major, 32 dimensions at a time; the leading dimensions are = 16 (mod 32) doubles, so
// the two 16-lane fragments a 32-lane half reads (k-rows kr, kr + 1) fall on opposite halves of
// the 64 LDS banks, and the staging writes go to consecutive rows: both conflict-free.
constexpr int kSfR = 64, kSfC = 128, kSfK = 32, kSfLa = 80, kSfLb = 144;

template <int OK>
__global__ __launch_bounds__(256, 2) void kfu_samples_mfma(
    const double* __restrict__ vsh, int64_t ldvs, int d_sh, const double* __restrict__ vsa,
    int64_t ld_s, int64_t ld_r, int d_sa, const int64_t* __restrict__ perm, int64_t nstar, int S,
    const double* __restrict__ z, int64_t ldz, int64_t m, const double* __restrict__ zc,
    int64_t zld, const double* __restrict__ Bm, int64_t ldb, double inv_lo, double s_o,
    const int64_t* __restrict__ pos, double* __restrict__ FX, int64_t ldfx, ExpNegConsts ek) {
  __shared__ __attribute__((aligned(16))) double la[kSfK * kSfLa];
  __shared__ __attribute__((aligned(16))) double lb[kSfK * kSfLb];
  // partial squared norms of the staged operands (per staging thread: 8 / 16 dimensions of every
  // chunk): the row's of the running part, the columns' of the shared and of the sample part
  __shared__ double vnp[4][kSfR], znp[2][kSfC], zsp[2][kSfC];
  __shared__ double bm_s[kSfC];
  __shared__ double red[2][kSfR];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int frow = lane >> 4, fcol = lane & 15;
  const int64_t r0 = (int64_t)blockIdx.x * kSfR;
  // staging roles: a wave per 8 dimensions of the row tile, a half block per 16 of the column tile
  const int arow = tid & (kSfR - 1), akg = tid >> 6;
  const int bcol = tid & (kSfC - 1), bkg = tid >> 7;
  const bool av = r0 + arow < nstar;
  const int64_t irc = av ? r0 + arow : nstar - 1;
  const double* ash = d_sh > 0 ? vsh + irc * ldvs : nullptr;
  const double* asa = d_sa > 0 ? vsa + (perm ? perm[irc] : irc) * ld_r : nullptr;
  const int nch_sa = d_sa > 0 ? (d_sa + kSfK - 1) / kSfK : 1;
  for (int64_t c0 = 0; c0 < m; c0 += kSfC) {
    const double* cg = zc + (c0 >> 8) * zld;   // 128-column tiles never straddle a 256-group
    const bool bv = c0 + bcol < m;
    const double* bz = z + (bv ? c0 + bcol : m - 1) * ldz;
    // one chunk of `dims` input dimensions from k0 (columns zoff + . of z and of the centres) into
    // la, and into lb when the column tile's copy is not there yet; padding rows, columns and
    // dimensions are zeros
    auto stage = [&](const double* ap, int zoff, int dims, int k0, bool with_b, double& an,
                     double& bn) __attribute__((always_inline)) {
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int kk = k0 + akg * 8 + q;
        const int kc = kk < dims ? kk : dims - 1;
        const double a = ap[kc] - cg[zoff + kc];
        const double x = (av && kk < dims) ? a : 0.0;
        an = fma(x, x, an);
        la[(akg * 8 + q) * kSfLa + arow] = x;
      }
      if (with_b) {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int kk = k0 + bkg * 16 + q;
          const int kc = kk < dims ? kk : dims - 1;
          const double b = bz[zoff + kc] - cg[zoff + kc];
          const double x = (bv && kk < dims) ? b : 0.0;
          bn = fma(x, x, bn);
          lb[(bkg * 16 + q) * kSfLb + bcol] = x;
        }
      }
    };
    auto contract = [&](d4 (&acc)[2][4], int dims_left) __attribute__((always_inline)) {
      const int nk4 = ((dims_left < kSfK ? dims_left : kSfK) + 3) >> 2;
      for (int ks = 0; ks < nk4; ++ks) {
        const int kr = ks * 4 + frow;
        double fa[2], fb[4];
#pragma unroll
        for (int a = 0; a < 2; ++a) fa[a] = la[kr * kSfLa + wr * 32 + a * 16 + fcol];
#pragma unroll
        for (int c = 0; c < 4; ++c) fb[c] = lb[kr * kSfLb + wc * 64 + c * 16 + fcol];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int c = 0; c < 4; ++c)
            acc[a][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[a], fb[c], acc[a][c], 0, 0, 0);
      }
    };
    // ---- the shared columns' part of d2, once for all samples of this (row tile, column tile)
    d4 sh[2][4];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) sh[a][c] = d4{0.0, 0.0, 0.0, 0.0};
    if (d_sh > 0) {
      double an = 0.0, bn = 0.0;
      for (int k0 = 0; k0 < d_sh; k0 += kSfK) {
        __syncthreads();   // the previous readers of la / lb / the norms are done
        stage(ash, 0, d_sh, k0, true, an, bn);
        if (k0 + kSfK >= d_sh) {
          vnp[akg][arow] = an;
          znp[bkg][bcol] = bn;
        }
        __syncthreads();
        contract(sh, d_sh - k0);
      }
      // C layout: lane holds rows frow + 4 r, column fcol of each 16 x 16 tile
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int rl = wr * 32 + a * 16 + frow + 4 * r;
          const double vn = (vnp[0][rl] + vnp[1][rl]) + (vnp[2][rl] + vnp[3][rl]);
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const int cl = wc * 64 + c * 16 + fcol;
            sh[a][c][r] = vn + (znp[0][cl] + znp[1][cl]) - 2.0 * sh[a][c][r];
          }
        }
    }
    // ---- per sample: its columns' part on the staged z tile, the kernel, the product with Bm
    for (int s = 0; s < S; ++s) {
      // the z tile's sample columns stay in lb for every sample when one chunk holds them
      const bool with_b = s == 0 || nch_sa > 1;
      const double* ap = d_sa > 0 ? asa + (int64_t)s * ld_s : nullptr;
      d4 acc[2][4];
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[a][c] = d4{0.0, 0.0, 0.0, 0.0};
      double an = 0.0, bn = 0.0;
      for (int ch = 0; ch < nch_sa; ++ch) {
        const int k0 = ch * kSfK;
        __syncthreads();   // the previous sample's (or the shared part's) readers are done
        if (d_sa > 0) stage(ap, d_sh, d_sa, k0, with_b, an, bn);
        if (ch == nch_sa - 1) {
          vnp[akg][arow] = an;
          if (with_b) zsp[bkg][bcol] = bn;
          // the sample's loadings of this tile: zero past m, so the padding columns add nothing
          if (tid < kSfC) bm_s[tid] = (c0 + tid < m) ? Bm[(int64_t)s * ldb + c0 + tid] : 0.0;
        }
        __syncthreads();
        contract(acc, d_sa - k0);
      }
      // epilogue on the accumulator tiles: s_o kappa(d / l_o) Bm_c over this lane's columns in tile
      // order.  Evaluated for every column and selected after (padding: finite values, dropped)
      double racc[2][4];
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int rl = wr * 32 + a * 16 + frow + 4 * r;
          const double vn = (vnp[0][rl] + vnp[1][rl]) + (vnp[2][rl] + vnp[3][rl]);
          double sum = 0.0;
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const int cl = wc * 64 + c * 16 + fcol;
            double d2 = sh[a][c][r] + (vn + (zsp[0][cl] + zsp[1][cl]) - 2.0 * acc[a][c][r]);
            if constexpr (OK == KEQ) d2 = d2 > 0.0 ? d2 : 0.0;
            const double kv = skappa_sq_k<OK>(d2, inv_lo, s_o, ek);
            sum = fma((c0 + cl < m) ? kv : 0.0, bm_s[cl], sum);
          }
          racc[a][r] = sum;
        }
      // the 16 lanes sharing a row (fcol), then the two column halves (wc), in a fixed order
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
          for (int off = 1; off < 16; off <<= 1) racc[a][r] += __shfl_xor(racc[a][r], off, 64);
          if (fcol == 0) red[wc][wr * 32 + a * 16 + frow + 4 * r] = racc[a][r];
        }
      __syncthreads();
      // the tiles' partials are added in tile order by the one thread that owns the row
      if (tid < kSfR && r0 + tid < nstar) {
        const double f = red[0][tid] + red[1][tid];
        double* dst = FX + pos[r0 + tid] * ldfx + s;
        *dst = c0 == 0 ? f : *dst + f;
      }
      // (red, vnp, zsp and bm_s are next written behind the next chunk loop's first barrier)
    }
  }
}

// Matern-1/2: d2 by direct differences (kfu_gemv_direct's layout: one column per thread, the row
// tile's inputs staged through LDS 16 dimensions at a time and read back as broadcasts).  The
// shared columns' sum of squares is kept per (row, column) in registers and every sample starts
// from it; per sample a thread's term per row is summed over the wave and the four waves in a
// fixed order, and the 256-column tiles' partials are added to FX in tile order by the row's thread.
constexpr int kSdRows = 32, kSdDim = 16;

__global__ __launch_bounds__(256) void kfu_samples_direct(
    const double* __restrict__ vsh, int64_t ldvs, int d_sh, const double* __restrict__ vsa,
    int64_t ld_s, int64_t ld_r, int d_sa, const int64_t* __restrict__ perm, int64_t nstar, int S,
    const double* __restrict__ z, int64_t ldz, int64_t m, const double* __restrict__ Bm,
    int64_t ldb, double inv_lo, double s_o, const int64_t* __restrict__ pos,
    double* __restrict__ FX, int64_t ldfx, ExpNegConsts ek) {
  __shared__ double vs[kSdRows][kSdDim + 1];
  __shared__ double red[4][kSdRows];
  const int tid = threadIdx.x;
  const int64_t k0 = (int64_t)blockIdx.x * kSdRows;
  // the staging element of this thread: row sr, dimension si of a 16-wide slice (two per thread)
  auto stage = [&](const double* base, int64_t ldrow, bool gather, int dims, int i0)
                   __attribute__((always_inline)) {
    for (int e = tid; e < kSdRows * kSdDim; e += 256) {
      const int r = e / kSdDim, i = e % kSdDim;
      const int64_t k = k0 + r;
      double x = 0.0;
      if (k < nstar && i0 + i < dims) x = base[((gather && perm) ? perm[k] : k) * ldrow + i0 + i];
      vs[r][i] = x;
    }
  };
  for (int64_t c0 = 0; c0 < m; c0 += 256) {
    const int64_t c = c0 + tid;
    const bool cv = c < m;
    const double* zr_p = z + (cv ? c : 0) * ldz;
    auto accumulate = [&](double (&acc)[kSdRows], int zoff, int dims, int i0)
                          __attribute__((always_inline)) {
      double zr[kSdDim];
#pragma unroll
      for (int i = 0; i < kSdDim; ++i) zr[i] = (i0 + i < dims) ? zr_p[zoff + i0 + i] : 0.0;
#pragma unroll
      for (int r = 0; r < kSdRows; ++r)
#pragma unroll
        for (int i = 0; i < kSdDim; ++i) {
          const double a = vs[r][i] - zr[i];   // dimensions past dims: 0 - 0
          acc[r] = fma(a, a, acc[r]);
        }
    };
    double sh[kSdRows];
#pragma unroll
    for (int r = 0; r < kSdRows; ++r) sh[r] = 0.0;
    for (int i0 = 0; i0 < d_sh; i0 += kSdDim) {
      __syncthreads();
      stage(vsh, ldvs, false, d_sh, i0);
      __syncthreads();
      accumulate(sh, 0, d_sh, i0);
    }
    for (int s = 0; s < S; ++s) {
      double acc[kSdRows];
#pragma unroll
      for (int r = 0; r < kSdRows; ++r) acc[r] = sh[r];
      for (int i0 = 0; i0 < d_sa; i0 += kSdDim) {
        __syncthreads();
        stage(vsa + (int64_t)s * ld_s, ld_r, true, d_sa, i0);
        __syncthreads();
        accumulate(acc, d_sh, d_sa, i0);
      }
      const double bw = cv ? Bm[(int64_t)s * ldb + c] : 0.0;
      __syncthreads();   // the previous sample's readers of red are done
#pragma unroll
      for (int r = 0; r < kSdRows; ++r) {
        const double kv = skappa_sq_k<KM12>(acc[r], inv_lo, s_o, ek);
        const double t = wave_sum(cv ? kv * bw : 0.0);
        if ((tid & 63) == 0) red[tid >> 6][r] = t;
      }
      __syncthreads();
      if (tid < kSdRows && k0 + tid < nstar) {
        const double f = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
        double* dst = FX + pos[k0 + tid] * ldfx + s;
        *dst = c0 == 0 ? f : *dst + f;
      }
    }
  }
}

// dst[pos[k] * ldd + s] = src[k * S + s]: the training rows' FX (computed over the n training rows
// alone) into their rows of the merged grid
__global__ __launch_bounds__(256) void scatter_rows(const double* __restrict__ src, int64_t n, int S,
                                                    const int64_t* __restrict__ pos,
                                                    double* __restrict__ dst, int64_t ldd) {
  const int64_t e = blockIdx.x * (int64_t)256 + threadIdx.x;
  if (e >= n * S) return;
  const int64_t k = e / S, s = e - k * S;
  dst[pos[k] * ldd + s] = src[e];
}

// out[s * ld_s + i * ld_r] = fx[k * ldfx + s] + F[k * S + s], k = pos[i]: sample s's value at test
// point i (what path_stats reduces), sample-major into a strided destination
__global__ __launch_bounds__(256) void sample_values(const double* __restrict__ fx, int64_t ldfx,
                                                     const double* __restrict__ F, int S,
                                                     const int64_t* __restrict__ pos,
                                                     int64_t nstar, double* __restrict__ out,
                                                     int64_t ld_s, int64_t ld_r) {
  const int64_t e = blockIdx.x * (int64_t)256 + threadIdx.x;
  if (e >= nstar * S) return;
  const int64_t i = e % nstar, s = e / nstar;
  const int64_t k = pos[i];
  out[s * ld_s + i * ld_r] = fx[k * ldfx + s] + F[k * S + s];
}

}  // namespace gpar

// ============================================================================ launch wrappers
#include "launch.hpp"

namespace gpar {

void launch_kfu_samples(hipStream_t st, int out_kind, const double* vsh, int64_t ldvs, int d_sh,
                        const double* vsa, int64_t ld_s, int64_t ld_r, int d_sa,
                        const int64_t* perm, int64_t nstar, int S, const double* z, int64_t ldz,
                        int64_t m, const double* zc, const double* Bm, int64_t ldb, double inv_lo,
                        double s_o, const int64_t* pos, double* FX, int64_t ldfx) {
  if (nstar <= 0 || S <= 0) return;
  if (out_kind == KM12) {
    kfu_samples_direct<<<(unsigned)((nstar + kSdRows - 1) / kSdRows), 256, 0, st>>>(
        vsh, ldvs, d_sh, vsa, ld_s, ld_r, d_sa, perm, nstar, S, z, ldz, m, Bm, ldb, inv_lo, s_o, pos,
        FX, ldfx, exp_neg_consts());
    return;
  }
  const unsigned grid = (unsigned)((nstar + kSfR - 1) / kSfR);
#define SF_ARGS vsh, ldvs, d_sh, vsa, ld_s, ld_r, d_sa, perm, nstar, S, z, ldz, m, zc, zc_stride(d_sh + d_sa), Bm, ldb, inv_lo, s_o, pos, FX, ldfx, exp_neg_consts()
  switch (out_kind) {
    case KM32: kfu_samples_mfma<KM32><<<grid, 256, 0, st>>>(SF_ARGS); break;
    case KEQ: kfu_samples_mfma<KEQ><<<grid, 256, 0, st>>>(SF_ARGS); break;
    default: kfu_samples_mfma<KM52><<<grid, 256, 0, st>>>(SF_ARGS); break;
  }
#undef SF_ARGS
}

void launch_scatter_rows(hipStream_t st, const double* src, int64_t n, int S, const int64_t* pos,
                         double* dst, int64_t ldd) {
  if (n <= 0) return;
  scatter_rows<<<(unsigned)((n * S + 255) / 256), 256, 0, st>>>(src, n, S, pos, dst, ldd);
}

void launch_sample_values(hipStream_t st, const double* fx, int64_t ldfx, const double* F, int S,
                          const int64_t* pos, int64_t nstar, double* out, int64_t ld_s,
                          int64_t ld_r) {
  sample_values<<<(unsigned)((nstar * S + 255) / 256), 256, 0, st>>>(fx, ldfx, F, S, pos, nstar, out,
                                                                    ld_s, ld_r);
}

}  // namespace gpar
