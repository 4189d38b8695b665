// k_gram.hip -- the dominant contraction of the DTC objective on fp64 MFMA.
//
// G = beta^T beta (M x M) and r = beta^T alpha over N time steps.  The whitening writes the
// chunk-local beta_loc (k_lgssm.hip); the true beta is beta_loc + g_k C_j^T in chunk j, with C_j
// (M x d) the carried-in filter states.  Expanding the product per chunk,
//   G = sum_k beta_loc,k^T beta_loc,k + sum_j (E_j C_j^T + C_j E_j^T),
//   E_j = H_j + C_j W_j / 2,  H_j = sum_{k in j} beta_loc,k^T g_k,  W_j = sum_{k in j} g_k^T g_k,
//   r = sum_k beta_loc,k^T alpha_k + sum_j C_j q_j,  q_j = sum_{k in j} g_k alpha_k,
// so the streamed loop is a plain Gram of beta_loc and the fix-up collapses to a rank-2d term per
// chunk (K = 2 d N / 256, ~2 % of the loop), computed in each split's tail from E_j (whitening +
// vec_fix) and C_j (carry).  In the reference this is the M x M x N trsm + gemm of dtc.jl:119-120
// (A = L_u^{-1} beta^T; Lambda = A A^T + I), which the build reassociates as
// Lambda = L_u^{-1} (beta^T beta) L_u^{-T} + I.
//
// Tiling: split-K over the time axis on v_mfma_f64_16x16x4_f64 (C/D: col = lane & 15, row =
// (lane >> 4) + 4 * reg).  K-step = 16 time rows staged global -> LDS by LDS-DMA (no VGPRs),
// double buffered.  v3 (gram3_*, the default): fat two-wave workgroups, one wave per SIMD with 32
// accumulator tiles; v2 (gram2_kernel, the two-lane mode's one-workgroup-per-CU plan): 4 waves of
// 16 / 18 tiles.
#include <type_traits>

#include "gram_common.hpp"

namespace gpar {

// ============================================================================ v2 decomposition
// The v1 groups compute every diagonal 64 x 64 sub-tile whole although 6 of its 16 tiles lie
// above G's diagonal (12 % of the MFMAs at M = 512), and every workgroup's critical path is a
// full sub-tile, so the waste sets the kernel time.  v2 re-packs the work into two workgroup
// types of equal per-wave work, each with its own number of time splits:
//   * OFF(a, b), a > b (unchanged): the 2 x 2 sub-tiles of the off-diagonal 128 x 128 block
//     (diagonal-block indices a, b; panels 2a, 2a+1 | 2b, 2b+1), 16 tiles of 16 x 16 per wave;
//   * DG(q): the lower triangles of the diagonal 128-blocks a0 = 2q, a1 = 2q + 1 (panels
//     2a0, 2a0+1, 2a1, 2a1+1 in slots 0..3), 36 tiles each, split 18 + 18 over two waves:
//     half 0 owns local tile rows {0, 1, 2, 3, 7}, half 1 rows {4, 5, 6} (local row r in 0..7:
//     slot base + r / 4, tile r % 4 of that panel).  Nothing above the diagonal is computed
//     except the upper halves of the 8 diagonal 16 x 16 tiles themselves.
// gram2_plan picks the split counts so the per-wave work (tiles x rows) of the two types
// matches and the workgroups fill the 512 co-resident slots.  DG also owns r = beta^T alpha
// (every panel is staged by exactly one DG workgroup per split).
// (kD2T and the d2_* tile maps: gram_common.hpp)

// PF: operand fragments of k-substep ks + 1 are read from LDS while substep ks's MFMAs issue
// (two fragment sets in registers).  Used by the one-workgroup-per-CU mode, where each SIMD has a
// single Gram wave and nothing else of the Gram to hide LDS latency behind; the two-per-CU kernel
// (PF = false) keeps reading each substep's fragments just before its MFMAs.
template <int D, bool PF>
__global__ __launch_bounds__(256, 2) void gram2_kernel(
    const double* __restrict__ beta, int64_t ldb, int64_t n, const double* __restrict__ ecor,
    const double* __restrict__ cin, const double* __restrict__ qv, int64_t mc, int L,
    const double* __restrict__ alpha, int npan, int noff, int ndg, int soff, int sdg,
    int64_t rows_off, int64_t rows_dg, double* __restrict__ part, double* __restrict__ rpart) {
  __shared__ __attribute__((aligned(16))) double smem[8 * kPanelD + 2 * 4 * kBK];
  double* ringa = smem + 8 * kPanelD;
  const int nbk = npan >> 1;   // diagonal 128-blocks

  // Work items in order: all OFF workgroups (group fastest), then all DG workgroups.  Blocks
  // are dealt to the 8 XCDs round-robin (blockIdx % 8), so item i runs as block
  // 8 (i % per) + i / per: every XCD gets a run of consecutive items, and the 6 OFF groups of
  // a split -- 24 panel reads of 8 distinct panels -- share one L2.
  const int nwg = noff * soff + ndg * sdg;
  const int per = (nwg + 7) >> 3;
  const int b = ((int)blockIdx.x & 7) * per + ((int)blockIdx.x >> 3);
  if (b >= nwg) return;
  bool dg;
  int split, gid, nsplit;
  int64_t rows;
  if (b < noff * soff) {
    dg = false; gid = b % noff; split = b / noff; nsplit = soff; rows = rows_off;
  } else {
    const int bb = b - noff * soff;
    dg = true; gid = bb % ndg; split = bb / ndg; nsplit = sdg; rows = rows_dg;
  }
  if (split >= nsplit) return;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // this wave's staged panel, operand slots, and role
  int spanel, sa = 0, sb = 0, pa = 0, pb = 0, half = 0, blk = 0;
  bool mf = true, owns_r = false;
  if (!dg) {
    int a = 1;
    while (a * (a + 1) / 2 <= gid) ++a;
    const int bo = gid - a * (a - 1) / 2;
    sa = wave >> 1;
    sb = 2 + (wave & 1);
    pa = 2 * a + (wave >> 1);
    pb = 2 * bo + (wave & 1);
    spanel = (wave < 2) ? 2 * a + wave : 2 * bo + (wave - 2);
  } else {
    const int a0 = 2 * gid, a1 = 2 * gid + 1;
    blk = (wave < 2) ? a0 : a1;
    half = wave & 1;
    mf = blk < nbk;
    const int pblk = mf ? blk : a0;                       // a missing second block: duplicate
    spanel = 2 * pblk + (wave & 1);                        // slot w holds panel 2 blk + (w & 1)
    sa = (wave < 2) ? 0 : 2;                               // slot base of this wave's block
    owns_r = mf;
  }

  const int64_t kb = (int64_t)split * rows;
  int64_t ke = kb + rows;
  if (ke > n) ke = n;
  const int nsteps = (int)(ke > kb ? (ke - kb + kBK - 1) / kBK : 0);

  double racc4[4] = {0.0, 0.0, 0.0, 0.0};
  const int lq = lane >> 4, lc = lane & 15;
  const int hl = lane >> 5, cl2 = (lane & 31) * 2;
  const uint32_t boff =
      (uint32_t)(((int64_t)hl * ldb + (int64_t)spanel * kPW + (cl2 ^ (hl << 4))) * 8);
  const char* bbase = reinterpret_cast<const char*>(beta);
  const double* zrow = beta + n * ldb;
  auto issue = [&](int s) __attribute__((always_inline)) {
    const int64_t k0 = kb + (int64_t)s * kBK;
    double* img = smem + ((s & 1) * 4 + wave) * kPanelD;
#pragma unroll
    for (int i = 0; i < kBK / 2; ++i) {
      const char* rowp = bbase + (k0 + 2 * i) * ldb * 8;
      __builtin_amdgcn_global_load_lds(rowp + boff, img + 2 * i * kPW, 16, 0, 0);
    }
    if (lane < 32) {
      const int64_t kr = k0 + (lane >> 1);
      const unsigned* as = kr < n ? reinterpret_cast<const unsigned*>(alpha + kr) + (lane & 1)
                                  : reinterpret_cast<const unsigned*>(zrow);
      __builtin_amdgcn_global_load_lds(as, ringa + ((s & 1) * 4 + wave) * kBK, 4, 0, 0);
    }
  };
  const int frow = lane >> 4, fcol = lane & 15;
  const int par = frow & 1;
  // fragment offset of tile t (0..3) of slot sl at k-substep 0
  auto foff = [&](int sl, int t) __attribute__((always_inline)) {
    return sl * kPanelD + frow * kPW + ((t ^ par) << 4) + fcol;
  };
  const int roff = wave * kPanelD + lq * kPW + lc;
  auto r_update = [&](int s, const double* base) __attribute__((always_inline)) {
    const double* ar = ringa + ((s & 1) * 4 + wave) * kBK;
    const double* im = base + roff;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const double av = ar[lq + 4 * i];
      const int rsw = (i * 4 + lq) & 1;
#pragma unroll
      for (int c = 0; c < 4; ++c) racc4[c] = fma(av, im[4 * i * kPW + ((c ^ rsw) << 4)], racc4[c]);
    }
  };

  if (nsteps > 0) issue(0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  const int64_t nch = (n + L - 1) / L;
  const int64_t j0 = (int64_t)split * nch / nsplit, j1 = (int64_t)(split + 1) * nch / nsplit;
  const bool cv = lq < D;
  const int64_t cstride = mc * kSStride;
  double* ptile = part + (((int64_t)b * 4 + wave) * kD2T) * 256;   // this wave's tile slots

  // store tile t of acc: C layout (col = lane & 15, row = (lane >> 4) + 4 r)
  auto store_tile = [&](int t, const d4& v) __attribute__((always_inline)) {
#pragma unroll
    for (int r = 0; r < 4; ++r) ptile[t * 256 + (frow + 4 * r) * 16 + fcol] = v[r];
  };

  if (!dg) {
    // ---------------- OFF: 4 x 4 tiles, A tiles 0..3 of slot sa, B tiles 0..3 of slot sb
    d4 acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[a][c] = d4{0.0, 0.0, 0.0, 0.0};
    int offa[4], offb[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) { offa[a] = foff(sa, a); offb[a] = foff(sb, a); }
    for (int s = 0; s < nsteps; ++s) {
      if (s + 1 < nsteps) issue(s + 1);
      const double* base = smem + (s & 1) * 4 * kPanelD;
      if constexpr (PF) {
        double fa[2][4], fb[2][4];
#pragma unroll
        for (int a = 0; a < 4; ++a) { fa[0][a] = base[offa[a]]; fb[0][a] = base[offb[a]]; }
#pragma unroll
        for (int ks = 0; ks < kBK / 4; ++ks) {
          const int cur = ks & 1;
          if (ks + 1 < kBK / 4) {
#pragma unroll
            for (int a = 0; a < 4; ++a) {
              fa[cur ^ 1][a] = base[offa[a] + (ks + 1) * 4 * kPW];
              fb[cur ^ 1][a] = base[offb[a] + (ks + 1) * 4 * kPW];
            }
          }
          __builtin_amdgcn_s_setprio(1);
#pragma unroll
          for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int c = 0; c < 4; ++c)
              acc[a][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[cur][a], fb[cur][c], acc[a][c], 0, 0, 0);
          __builtin_amdgcn_s_setprio(0);
        }
      } else {
#pragma unroll
      for (int ks = 0; ks < kBK / 4; ++ks) {
        double fa[4], fb[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) fa[a] = base[offa[a] + ks * 4 * kPW];
#pragma unroll
        for (int c = 0; c < 4; ++c) fb[c] = base[offb[c] + ks * 4 * kPW];
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int c = 0; c < 4; ++c)
            acc[a][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[a], fb[c], acc[a][c], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
      }
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }
    if (ecor) {
      const int64_t oa = ((int64_t)pa * kPW + lc) * kSStride + lq;
      const int64_t ob = ((int64_t)pb * kPW + lc) * kSStride + lq;
      // chunk jj + 1's E / C rows are loaded while chunk jj's 32 MFMAs run
      double ea[4], ca[4], eb[4], cb[4];
      auto ld = [&](int64_t jj) __attribute__((always_inline)) {
        const double* ej = ecor + jj * cstride;
        const double* cj = cin + jj * cstride;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          ea[t] = ej[oa + t * 16 * kSStride];
          eb[t] = ej[ob + t * 16 * kSStride];
          ca[t] = cv ? cj[oa + t * 16 * kSStride] : 0.0;
          cb[t] = cv ? cj[ob + t * 16 * kSStride] : 0.0;
        }
      };
      if (j0 < j1) ld(j0);
      for (int64_t jj = j0; jj < j1; ++jj) {
        double xa[4], ya[4], xb[4], yb[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) { xa[t] = ea[t]; ya[t] = ca[t]; xb[t] = eb[t]; yb[t] = cb[t]; }
        if (jj + 1 < j1) ld(jj + 1);
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            acc[a][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[a], yb[c], acc[a][c], 0, 0, 0);
            acc[a][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(ya[a], xb[c], acc[a][c], 0, 0, 0);
          }
      }
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) store_tile(a * 4 + c, acc[a][c]);
    return;
  }

  // ---------------- DG: 18 tiles of the diagonal block blk (local rows per half)
  auto dg_body = [&](auto htag) __attribute__((always_inline)) {
    constexpr int H = decltype(htag)::value;
    constexpr int NA = d2_na<H>(), NB = d2_nb<H>();
    d4 acc[kD2T];
#pragma unroll
    for (int t = 0; t < kD2T; ++t) acc[t] = d4{0.0, 0.0, 0.0, 0.0};
    int offa[NA], offb[NB];
#pragma unroll
    for (int ia = 0; ia < NA; ++ia) {
      const int r = d2_row<H>(ia);
      offa[ia] = foff(sa + (r >> 2), r & 3);
    }
#pragma unroll
    for (int c = 0; c < NB; ++c) offb[c] = foff(sa + (c >> 2), c & 3);
    for (int s = 0; s < nsteps; ++s) {
      if (s + 1 < nsteps) issue(s + 1);
      const double* base = smem + (s & 1) * 4 * kPanelD;
      if constexpr (PF) {
        double fa[2][NA], fb[2][NB];
#pragma unroll
        for (int ia = 0; ia < NA; ++ia) fa[0][ia] = base[offa[ia]];
#pragma unroll
        for (int c = 0; c < NB; ++c) fb[0][c] = base[offb[c]];
#pragma unroll
        for (int ks = 0; ks < kBK / 4; ++ks) {
          const int cur = ks & 1;
          if (ks + 1 < kBK / 4) {
#pragma unroll
            for (int ia = 0; ia < NA; ++ia) fa[cur ^ 1][ia] = base[offa[ia] + (ks + 1) * 4 * kPW];
#pragma unroll
            for (int c = 0; c < NB; ++c) fb[cur ^ 1][c] = base[offb[c] + (ks + 1) * 4 * kPW];
          }
          __builtin_amdgcn_s_setprio(1);
#pragma unroll
          for (int ia = 0; ia < NA; ++ia)
#pragma unroll
            for (int c = 0; c <= d2_row<H>(ia); ++c)
              acc[d2_tile<H>(ia, c)] = __builtin_amdgcn_mfma_f64_16x16x4f64(
                  fa[cur][ia], fb[cur][c], acc[d2_tile<H>(ia, c)], 0, 0, 0);
          __builtin_amdgcn_s_setprio(0);
        }
      } else {
#pragma unroll
      for (int ks = 0; ks < kBK / 4; ++ks) {
        double fa[NA], fb[NB];
#pragma unroll
        for (int ia = 0; ia < NA; ++ia) fa[ia] = base[offa[ia] + ks * 4 * kPW];
#pragma unroll
        for (int c = 0; c < NB; ++c) fb[c] = base[offb[c] + ks * 4 * kPW];
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int ia = 0; ia < NA; ++ia)
#pragma unroll
          for (int c = 0; c <= d2_row<H>(ia); ++c)
            acc[d2_tile<H>(ia, c)] =
                __builtin_amdgcn_mfma_f64_16x16x4f64(fa[ia], fb[c], acc[d2_tile<H>(ia, c)], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
      }
      }
      if (owns_r) r_update(s, base);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }
    if (ecor && mf) {
      const int64_t pbase = (int64_t)2 * blk * kPW;   // first column of the diagonal block
      // E / C rows of the block, indexed by local tile column 0..7 (rows and columns share
      // them); chunk jj + 1's are loaded while chunk jj's MFMAs run
      double e8[8], c8[8];   // 8: the r update reads columns 4 H .. 4 H + 3
      auto ld = [&](int64_t jj) __attribute__((always_inline)) {
        const double* ej = ecor + jj * cstride;
        const double* cj = cin + jj * cstride;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          const int64_t o = (pbase + c * 16 + lc) * kSStride + lq;
          e8[c] = ej[o];
          c8[c] = cv ? cj[o] : 0.0;
        }
      };
      if (j0 < j1) ld(j0);
      for (int64_t jj = j0; jj < j1; ++jj) {
        double xe[8], xc[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) { xe[c] = e8[c]; xc[c] = c8[c]; }
        if (jj + 1 < j1) ld(jj + 1);
#pragma unroll
        for (int ia = 0; ia < NA; ++ia)
#pragma unroll
          for (int c = 0; c <= d2_row<H>(ia); ++c) {
            const int r = d2_row<H>(ia);
            acc[d2_tile<H>(ia, c)] = __builtin_amdgcn_mfma_f64_16x16x4f64(xe[r], xc[c], acc[d2_tile<H>(ia, c)], 0, 0, 0);
            acc[d2_tile<H>(ia, c)] = __builtin_amdgcn_mfma_f64_16x16x4f64(xc[r], xe[c], acc[d2_tile<H>(ia, c)], 0, 0, 0);
          }
        if (owns_r) {   // this wave's staged panel is tile columns 4 H .. 4 H + 3 of the block
          const double qq = cv ? qv[jj * 4 + lq] : 0.0;
#pragma unroll
          for (int c = 0; c < 4; ++c) racc4[c] = fma(xc[4 * H + c], qq, racc4[c]);
        }
      }
    }
#pragma unroll
    for (int t = 0; t < kD2T; ++t) store_tile(t, acc[t]);
  };
  if (half == 0)
    dg_body(std::integral_constant<int, 0>{});
  else
    dg_body(std::integral_constant<int, 1>{});
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    double v = racc4[c];
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    if (owns_r && lq == 0) rpart[(int64_t)split * npan * kPW + (int64_t)spanel * kPW + c * 16 + lc] = v;
  }
}

// ============================================================================ v3: fat waves
// One wave per SIMD with twice the tiles.  A workgroup is 2 waves (128 threads), two workgroups
// per CU, in three launches:
//   * OFF(a, b), a > b (gram3_off_kernel, here): the whole off-diagonal 128 x 128 block; wave w
//     takes row panel 2a + w against both column panels 2b, 2b + 1: 4 x 8 = 32 tiles, whose
//     accumulators fill the 256 AGPRs.  Four panels per K-step, two staged by each wave (slots w
//     and 2 + w);
//   * DG(q) (gram3_dg_kernel, k_gram3v.hip): ONE diagonal 128-block q, its lower triangle's 36
//     tiles split 18 + 18 over the two waves as in v2 (local tile rows {0, 1, 2, 3, 7} |
//     {4, 5, 6}); wave h stages panel 2q + h.  DG also owns r = beta^T alpha (each panel is
//     staged by exactly one DG workgroup per split);
//   * the chunk correction sum_j (E_j C_j^T + C_j E_j^T) and r's sum_j C_j q_j
//     (gram3_corr_kernel, k_gram3v.hip) as extra "splits" of the same partial-tile layout.
// Per K-step an OFF wave issues 128 MFMAs between barriers, twice v2's, from 12 fragment reads
// per 32 MFMAs (v2: 8 per 16), and the next k-substep's fragments are read under the current
// substep's MFMAs.  A pure 4 x 8-tile wave loop measured 67 TF/s on MI355X (0.85 of the fp64
// peak) with one wave per SIMD, against v2's ~60 TF/s in the job.  The three kernels are
// separate because the register allocator keeps loop-carried accumulators in place only in a
// kernel with one accumulation loop: with the correction tail (or the DG path) in the same
// function it parks tiles in VGPRs and copies all of them every K-step.  The DG and correction
// kernels fit their accumulators in VGPRs and are compiled with VGPR-form MFMAs (Makefile).
//
// Partial-tile layout (part): workgroup slot w, wave h, tile t at ((w * 2 + h) * kF3T + t) * 256
// (16 x 16 row-major).  OFF slots: gid + s * noff for s < soff + ncs (ncs correction splits
// after the soff time splits); DG slots from noff * (soff + ncs): gid + s * ndg, s < sdg + ncs.
// rpart: (sdg + ncs) x Mp.
__global__ __launch_bounds__(128) void gram3_off_kernel(const double* __restrict__ beta,
                                                        int64_t ldb, int64_t n, int noff,
                                                        int soff, int64_t rows,
                                                        double* __restrict__ part,
                                                        const GramGroupPtrs* __restrict__ grp) {
  if (grp) {
    const GramGroupPtrs& q = grp[blockIdx.y];
    beta = q.beta; part = q.part;
  }
  __shared__ __attribute__((aligned(16))) double smem[8 * kPanelD];

  const int nty = noff * soff;
  const int per = (nty + 7) >> 3;
  const int b = ((int)blockIdx.x & 7) * per + ((int)blockIdx.x >> 3);   // XCD-major deal
  if (b >= nty) return;
  const int gid = b % noff, split = b / noff;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int a = 1;
  while (a * (a + 1) / 2 <= gid) ++a;
  const int bo = gid - a * (a - 1) / 2;
  const int pA = 2 * a + wave, pB = 2 * bo + wave;   // panels this wave stages

  const int64_t kb = (int64_t)split * rows;
  int64_t ke = kb + rows;
  if (ke > n) ke = n;
  const int nsteps = (int)(ke > kb ? (ke - kb + kBK - 1) / kBK : 0);

  const int hl = lane >> 5, cl2 = (lane & 31) * 2;
  const int64_t lrow = (int64_t)hl * ldb;
  const uint32_t boffA = (uint32_t)((lrow + (int64_t)pA * kPW + (cl2 ^ (hl << 4))) * 8);
  const uint32_t boffB = (uint32_t)((lrow + (int64_t)pB * kPW + (cl2 ^ (hl << 4))) * 8);
  const char* bbase = reinterpret_cast<const char*>(beta);
  // wave w stages its A panel into slot w and its B panel into slot 2 + w
  auto issue = [&](int s) __attribute__((always_inline)) {
    const int64_t k0 = kb + (int64_t)s * kBK;
    double* imgA = smem + ((s & 1) * 4 + wave) * kPanelD;
    double* imgB = smem + ((s & 1) * 4 + 2 + wave) * kPanelD;
#pragma unroll
    for (int i = 0; i < kBK / 2; ++i) {
      const char* rowp = bbase + (k0 + 2 * i) * ldb * 8;
      __builtin_amdgcn_global_load_lds(rowp + boffA, imgA + 2 * i * kPW, 16, 0, 0);
      __builtin_amdgcn_global_load_lds(rowp + boffB, imgB + 2 * i * kPW, 16, 0, 0);
    }
  };
  const int frow = lane >> 4, fcol = lane & 15;
  const int par = frow & 1;
  auto foff = [&](int sl, int t) __attribute__((always_inline)) {
    return sl * kPanelD + frow * kPW + ((t ^ par) << 4) + fcol;
  };

  if (nsteps > 0) issue(0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  // rows = tiles 0..3 of slot `wave`, columns = tiles 0..3 of slots 2, 3
  d4 acc[4][8];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[i][c] = d4{0.0, 0.0, 0.0, 0.0};
  int offa[4], offb[8];
#pragma unroll
  for (int i = 0; i < 4; ++i) offa[i] = foff(wave, i);
#pragma unroll
  for (int c = 0; c < 8; ++c) offb[c] = foff(2 + (c >> 2), c & 3);
  for (int s = 0; s < nsteps; ++s) {
    if (s + 1 < nsteps) issue(s + 1);
    const double* base = smem + (s & 1) * 4 * kPanelD;
    double fa[2][4], fb[2][8];
#pragma unroll
    for (int i = 0; i < 4; ++i) fa[0][i] = base[offa[i]];
#pragma unroll
    for (int c = 0; c < 8; ++c) fb[0][c] = base[offb[c]];
#pragma unroll
    for (int ks = 0; ks < kBK / 4; ++ks) {
      const int cur = ks & 1;
      if (ks + 1 < kBK / 4) {
#pragma unroll
        for (int i = 0; i < 4; ++i) fa[cur ^ 1][i] = base[offa[i] + (ks + 1) * 4 * kPW];
#pragma unroll
        for (int c = 0; c < 8; ++c) fb[cur ^ 1][c] = base[offb[c] + (ks + 1) * 4 * kPW];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int c = 0; c < 8; ++c)
          acc[i][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[cur][i], fb[cur][c], acc[i][c], 0, 0, 0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  double* ptile = part + (((int64_t)b * 2 + wave) * kF3T) * 256;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int c = 0; c < 8; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        ptile[(i * 8 + c) * 256 + (frow + 4 * r) * 16 + fcol] = acc[i][c][r];
}

// v3 reduction: one grid row per (workgroup of the first split, wave, tile), summed over the
// type's time splits then its ncs correction splits, in order (deterministic); writes G and its
// mirror.  The last row sums r.
__global__ __launch_bounds__(256) void gram3_reduce(const double* __restrict__ part,
                                                    const double* __restrict__ rpart, int npan,
                                                    int noff, int ndg, int soff, int sdg, int ncs,
                                                    double* __restrict__ G, int64_t ldg,
                                                    double* __restrict__ r,
                                                    const GramGroupPtrs* __restrict__ grp) {
  if (grp) {
    const GramGroupPtrs& q = grp[blockIdx.y];
    part = q.part; rpart = q.rpart; G = q.G; r = q.r;
  }
  const int e = threadIdx.x;
  const int y = blockIdx.x;
  const int nrow_off = noff * 2 * kF3T, nrow_dg = ndg * 2 * kD2T;
  if (y == nrow_off + nrow_dg) {
    const int mp = npan * kPW;
    for (int c = e; c < mp; c += 256) {
      double s = 0.0;
#pragma unroll 8
      for (int sp = 0; sp < sdg + ncs; ++sp) s += rpart[(int64_t)sp * mp + c];
      r[c] = s;
    }
    return;
  }
  int64_t grow, gcol, wb;
  int w, t, nsp, stride;
  bool diag_tile = false;
  if (y < nrow_off) {
    const int gid = y / (2 * kF3T), rem = y % (2 * kF3T);
    w = rem / kF3T; t = rem % kF3T;
    int a = 1;
    while (a * (a + 1) / 2 <= gid) ++a;
    const int bo = gid - a * (a - 1) / 2;
    const int i = t / 8, c = t % 8;
    grow = (int64_t)(2 * a + w) * kPW + i * 16;
    gcol = (int64_t)(2 * bo + (c >> 2)) * kPW + (c & 3) * 16;
    wb = gid; nsp = soff + ncs; stride = noff;
  } else {
    const int yy = y - nrow_off;
    const int gid = yy / (2 * kD2T), rem = yy % (2 * kD2T);
    w = rem / kD2T; t = rem % kD2T;
    const int H = w;
    int ia = 0, tt = t, rr = 0;
    for (;;) {
      rr = (H == 0) ? (ia < 4 ? ia : 7) : 4 + ia;
      if (tt <= rr) break;
      tt -= rr + 1;
      ++ia;
    }
    grow = (int64_t)2 * gid * kPW + rr * 16;
    gcol = (int64_t)2 * gid * kPW + tt * 16;
    diag_tile = rr == tt;
    wb = (int64_t)noff * (soff + ncs) + gid; nsp = sdg + ncs; stride = ndg;
  }
  const int er = e / 16, ec = e % 16;
  if (diag_tile && er < ec) return;
  const double* pp = part + ((wb * 2 + w) * kF3T + t) * 256 + e;
  const int64_t pstride = (int64_t)stride * 2 * kF3T * 256;
  double s = 0.0;
#pragma unroll 8
  for (int sp = 0; sp < nsp; ++sp) s += pp[sp * pstride];
  const int64_t gr = grow + er, gc = gcol + ec;
  G[gr * ldg + gc] = s;
  G[gc * ldg + gr] = s;
}

// v2 reduction: one grid row per (workgroup of the first split, wave, tile); sums that tile's
// partials over the type's splits in split order and writes G (and its mirror).  The last grid
// row sums r over the DG splits.
__global__ __launch_bounds__(256) void gram2_reduce(const double* __restrict__ part,
                                                    const double* __restrict__ rpart, int npan,
                                                    int noff, int ndg, int soff, int sdg,
                                                    double* __restrict__ G, int64_t ldg,
                                                    double* __restrict__ r,
                                                    const GramGroupPtrs* __restrict__ grp) {
  if (grp) {
    const GramGroupPtrs& q = grp[blockIdx.y];
    part = q.part; rpart = q.rpart; G = q.G; r = q.r;
  }
  const int e = threadIdx.x;   // element of the 16 x 16 tile (C layout row-major 16 x 16)
  const int y = blockIdx.x;
  const int nbk = npan >> 1;
  const int nrow_off = noff * 4 * 16, nrow_dg = ndg * 4 * kD2T;
  if (y == nrow_off + nrow_dg) {
    const int mp = npan * kPW;
    for (int c = e; c < mp; c += 256) {
      double s = 0.0;
#pragma unroll 8
      for (int sp = 0; sp < sdg; ++sp) s += rpart[(int64_t)sp * mp + c];
      r[c] = s;
    }
    return;
  }
  int64_t grow, gcol;
  int64_t wb;        // workgroup index (first split) and wave
  int w, t, nsp, stride;
  bool diag_tile = false;
  if (y < nrow_off) {
    const int gid = y / 64, rem = y % 64;
    w = rem / 16; t = rem % 16;
    int a = 1;
    while (a * (a + 1) / 2 <= gid) ++a;
    const int bo = gid - a * (a - 1) / 2;
    const int pa = 2 * a + (w >> 1), pb = 2 * bo + (w & 1);
    grow = (int64_t)pa * kPW + (t >> 2) * 16;
    gcol = (int64_t)pb * kPW + (t & 3) * 16;
    wb = gid; nsp = soff; stride = noff;
  } else {
    const int yy = y - nrow_off;
    const int gid = yy / (4 * kD2T), rem = yy % (4 * kD2T);
    w = rem / kD2T; t = rem % kD2T;
    const int blk = (w < 2) ? 2 * gid : 2 * gid + 1;
    if (blk >= nbk) return;
    // invert d2_tile: walk the half's rows
    const int H = w & 1;
    int ia = 0, tt = t, rr = 0;
    for (;;) {
      rr = (H == 0) ? (ia < 4 ? ia : 7) : 4 + ia;
      if (tt <= rr) break;
      tt -= rr + 1;
      ++ia;
    }
    grow = (int64_t)2 * blk * kPW + rr * 16;
    gcol = (int64_t)2 * blk * kPW + tt * 16;
    diag_tile = rr == tt;
    wb = (int64_t)noff * soff + gid; nsp = sdg; stride = ndg;
  }
  const int er = e / 16, ec = e % 16;
  if (diag_tile && er < ec) return;
  // split order kept (deterministic); unrolled so the loads are in flight together
  const double* pp = part + ((wb * 4 + w) * kD2T + t) * 256 + e;
  const int64_t pstride = (int64_t)stride * 4 * kD2T * 256;
  double s = 0.0;
#pragma unroll 8
  for (int sp = 0; sp < nsp; ++sp) s += pp[sp * pstride];
  const int64_t gr = grow + er, gc = gcol + ec;
  G[gr * ldg + gc] = s;
  G[gc * ldg + gr] = s;
}

// The Gram-stage results of an evaluation that differs from a kept one only in the output
// kernel's variance s_o = sv_o^2 (GramScaleJob): Kfu, beta and the correction's H_j, C_j are linear
// in s_o and the filter does not see it, so G and r scale by c^2 and c = s_o' / s_o, and the
// alpha^2 / log S partials are the kept ones.  Grid (rows, jobs): block x takes row x of G; block 0
// also r and the partials.
__global__ __launch_bounds__(256) void gram_scale_kernel(const GramScaleJob* __restrict__ jobs) {
  const GramScaleJob j = jobs[blockIdx.y];
  const int64_t row = blockIdx.x;
  if (row >= j.mp) return;
  const double c2 = j.c * j.c;
  for (int64_t q = threadIdx.x; q < j.mp; q += 256) j.Gd[row * j.ldd + q] = c2 * j.G[row * j.lds + q];
  if (row != 0) return;
  for (int64_t q = threadIdx.x; q < j.mp; q += 256) j.rd[q] = j.c * j.r[q];
  for (int64_t q = threadIdx.x; q < j.npart; q += 256) j.a2d[q] = j.a2part[q];
  for (int64_t q = threadIdx.x; q < j.nch; q += 256) j.logsd[q] = j.logs[q];
}

// Materialise the corrected beta (only for the (dtc, A) parity entry point).
template <int D>
__global__ __launch_bounds__(256) void beta_fix_kernel(double* __restrict__ beta, int64_t ldb,
                                                       int64_t n, const double* __restrict__ g,
                                                       const double* __restrict__ cin, int64_t mc,
                                                       int L) {
  const int64_t e = blockIdx.x * (int64_t)256 + threadIdx.x;
  if (e >= n * ldb) return;
  const int64_t k = e / ldb, c = e % ldb;
  const int64_t ch = k >> __builtin_ctz(L);  // L is a power of two (kChunk)
  double v = beta[e];
#pragma unroll
  for (int i = 0; i < D; ++i) v = fma(g[k * kGStride + i], cin[(ch * mc + c) * kSStride + i], v);
  beta[e] = v;
}

}  // namespace gpar

// ============================================================================ launch wrappers
#include "launch.hpp"

namespace gpar {


// v2: split counts for the OFF and DG workgroups minimising the per-CU work
// ceil(workgroups / 256) x max(16 x rows_off, 18 x rows_dg), at most 512 workgroups (2 per CU);
// at M = 512, N = 1e6: 6 x 62 OFF + 2 x 70 DG = 512 workgroups, 16 x 16144 vs 18 x 14288
// tile-rows per wave (v1: 16 x 17872).
static void gram2_plan(int64_t n, int64_t mp, GramPlan& p, bool one_per_cu) {
  const int slots = one_per_cu ? 256 : 512;   // co-resident workgroups the splits should fill
  p.one_per_cu = one_per_cu ? 1 : 0;
  const int nbk = (int)(mp / 128);
  p.v2 = 1;
  p.npan = 2 * nbk;
  p.noff = nbk * (nbk - 1) / 2;
  p.ndg = (nbk + 1) / 2;
  // >= 256 rows per split, but at least 8 splits: shorter sequential sums per accumulator (the
  // noise-free q(u) factors a Cuu with cond ~1e7 and sees the Gram's rounding)
  const int64_t maxs = (n + 255) / 256 > 8 ? (n + 255) / 256 : 8;
  auto rows_of = [&](int64_t s) { return (((n + s - 1) / s + kBK - 1) / kBK) * kBK; };
  double best = 1e300;
  int bo = 1, bd = 1, bw = 0;
  for (int so = (p.noff ? 1 : 0); so <= (p.noff ? slots : 0); ++so) {
    if (so > maxs) break;
    const int left = slots - p.noff * so;
    if (left < p.ndg) break;
    for (int sd = 1; sd <= left / p.ndg && sd <= maxs; ++sd) {
      const int wgs = p.noff * so + p.ndg * sd;
      const double wo = so ? 16.0 * (double)rows_of(so) : 0.0;
      const double wd = 18.0 * (double)rows_of(sd);
      // one workgroup per CU leaves one wave per SIMD, with nothing to hide its barrier and LDS
      // waits behind: priced 15 % worse than the same work spread two per CU
      const double cost = (double)((wgs + 255) / 256) * (wo > wd ? wo : wd) *
                          (one_per_cu ? 1.0 : (wgs > 384 ? 1.0 : 1.15));
      if (cost < best * (1.0 - 1e-9) || (cost <= best * (1.0 + 1e-9) && wgs > bw)) {
        best = cost; bo = so; bd = sd; bw = wgs;
      }
    }
  }
  p.soff = p.noff ? bo : 0;
  p.sdg = bd;
  p.rows_off = p.noff ? rows_of(p.soff) : 0;
  p.rows_dg = rows_of(p.sdg);
  p.nsplit = p.sdg;
  p.part_doubles = (int64_t)(p.noff * p.soff + p.ndg * p.sdg) * 4 * kD2T * 256;
  p.rpart_doubles = (int64_t)p.sdg * mp;
}

#define HIPCHECK_G(x) do { if ((x) != hipSuccess) throw std::runtime_error("launch_gram: " #x); } while (0)
// DG workgroup slots of the whole chip: 238 VGPRs, so two waves per SIMD (512 slots: 2.18 ms per
// launch, 1024: 1.16 ms, 2048: 1.27 ms at the north config)
constexpr int kGram3DgSlots = 1024;

// v3: split counts for OFF (32 tiles per wave) and DG (18 tiles per wave, one diagonal block per
// workgroup), two launches of up to 512 workgroups each (two per CU, one wave per SIMD).
static void gram3_plan(int64_t n, int64_t mp, GramPlan& p, int cus, int dg_cus) {
  const int nbk = (int)(mp / 128);
  p.v2 = 1;
  p.v3 = 1;
  p.npan = 2 * nbk;
  p.noff = nbk * (nbk - 1) / 2;
  p.ndg = nbk;
  const int64_t maxs = (n + 255) / 256 > 8 ? (n + 255) / 256 : 8;
  auto rows_of = [&](int64_t sp) { return (((n + sp - 1) / sp + kBK - 1) / kBK) * kBK; };
  // OFF and DG run as two launches, each filling the 512 slots (two workgroups per CU) alone:
  // the most splits <= 512 / groups, and >= 8
  auto splits = [&](int groups, int slots) {
    int sp = slots / groups;
    if (sp < 1) sp = 1;
    if (sp > maxs) sp = (int)maxs;
    return sp;
  };
  p.soff = p.noff ? splits(p.noff, 2 * cus) : 0;
  // DG (238 VGPRs, 33 KB LDS) runs two waves per SIMD: 1024 slots
  p.sdg = splits(p.ndg, kGram3DgSlots * dg_cus / 256);
  p.rows_off = p.noff ? rows_of(p.soff) : 0;
  p.rows_dg = rows_of(p.sdg);
  p.nsplit = p.sdg;
  // chunk-correction splits: (noff + ndg) x ncs four-wave workgroups, two per CU
  const int64_t nch = (n + 255) / 256;
  int ncs = 2 * cus / (p.noff + p.ndg);
  if (ncs < 1) ncs = 1;
  if (ncs > nch) ncs = (int)(nch > 0 ? nch : 1);
  p.ncs = ncs;
  // co-run: the slim correction's 8 waves per (group, split), at most one per SIMD beside OFF
  int ncs2 = 4 * cus / (8 * (p.noff + p.ndg));
  if (ncs2 < 1) ncs2 = 1;
  if (ncs2 > nch) ncs2 = (int)(nch > 0 ? nch : 1);
  p.ncs_slim = ncs2;
  const int nc = ncs > ncs2 ? ncs : ncs2;
  p.part_doubles = (int64_t)(p.noff * (p.soff + nc) + p.ndg * (p.sdg + nc)) * 2 * kF3T * 256;
  p.rpart_doubles = (int64_t)(p.sdg + nc) * mp;
}

GramPlan gram_plan(int64_t n, int64_t mp, bool one_per_cu, int cus, int dg_cus) {
  GramPlan p;
  if (!one_per_cu)
    gram3_plan(n, mp, p, cus, dg_cus > 0 ? dg_cus : cus);
  else
    gram2_plan(n, mp, p, one_per_cu);
  return p;
}

void launch_gram(hipStream_t st, int sdim, const GramPlan& plan, const double* beta,
                 int64_t ldb, int64_t n, const double* ecor, const double* cin, const double* qv,
                 int64_t mc, int L, const double* alpha, double* part, double* rpart, double* G,
                 int64_t ldg, double* r, hipStream_t side, hipEvent_t ev_a, hipEvent_t ev_b,
                 hipStream_t st_w, hipEvent_t ev_w, int w_items) {
  if (plan.v3) {
    const bool corun = ecor && side && plan.noff > 0;
    const int ncs = ecor ? (corun ? plan.ncs_slim : plan.ncs) : 0;
    const int noffw = ((plan.noff * plan.soff + 7) / 8) * 8;   // XCD deal
    const int ndgw = ((plan.ndg * plan.sdg + 7) / 8) * 8;
    const int64_t nchk = (n + L - 1) / L;
    if (corun) {   // the slim correction beside the OFF kernel, on the second stream
      HIPCHECK_G(hipEventRecord(ev_a, st));
      HIPCHECK_G(hipStreamWaitEvent(side, ev_a, 0));
    }
    if (noffw > 0)
      gram3_off_kernel<<<noffw, 128, 0, st>>>(beta, ldb, n, plan.noff, plan.soff, plan.rows_off, part,
                                              nullptr);
    if (corun)
      launch_gram3_corr_slim(side, sdim, ecor, cin, qv, mc, nchk, plan.npan, plan.noff, plan.ndg,
                             plan.soff, plan.sdg, ncs, part, rpart);
    const int64_t dslot0 = (int64_t)plan.noff * (plan.soff + ncs);
    if (st_w && w_items > 0) {   // the first w_items DG items on another stream (other CUs)
      launch_gram3_dg(st_w, 0, beta, ldb, n, alpha, plan.npan, plan.ndg, plan.sdg, plan.rows_dg,
                      dslot0, part, rpart, 0, w_items, plan.dg_sw, plan.dg_rows_w);
      HIPCHECK_G(hipEventRecord(ev_w, st_w));
      launch_gram3_dg(st, 0, beta, ldb, n, alpha, plan.npan, plan.ndg, plan.sdg, plan.rows_dg,
                      dslot0, part, rpart, w_items, -1, plan.dg_sw, plan.dg_rows_w);
      HIPCHECK_G(hipStreamWaitEvent(st, ev_w, 0));
    } else {
      launch_gram3_dg(st, ndgw, beta, ldb, n, alpha, plan.npan, plan.ndg, plan.sdg, plan.rows_dg,
                      dslot0, part, rpart);
    }
    if (corun) {
      HIPCHECK_G(hipEventRecord(ev_b, side));
      HIPCHECK_G(hipStreamWaitEvent(st, ev_b, 0));
    } else if (ncs) {
      launch_gram3_corr(st, sdim, ecor, cin, qv, mc, nchk, plan.npan, plan.noff, plan.ndg,
                        plan.soff, plan.sdg, ncs, part, rpart);
    }
    const int nrows = plan.noff * 2 * kF3T + plan.ndg * 2 * kD2T + 1;
    gram3_reduce<<<nrows, 256, 0, st>>>(part, rpart, plan.npan, plan.noff, plan.ndg, plan.soff,
                                        plan.sdg, ncs, G, ldg, r, nullptr);
    return;
  }
  if (plan.v2) {
    const int nwg = ((plan.noff * plan.soff + plan.ndg * plan.sdg + 7) / 8) * 8;   // XCD deal
#define GRAM2_ARGS beta, ldb, n, ecor, cin, qv, mc, L, alpha, plan.npan, plan.noff, plan.ndg, \
                   plan.soff, plan.sdg, plan.rows_off, plan.rows_dg, part, rpart
    if (plan.one_per_cu) {
      // 65 KB static + 24 KB padding: a second Gram workgroup no longer fits a CU (160 KB), the
      // other lane's whitening (40 KB, 216 VGPRs beside the Gram's 239) does
      const size_t pad = 24 * 1024;
      switch (sdim) {
        case 1: gram2_kernel<1, true><<<nwg, 256, pad, st>>>(GRAM2_ARGS); break;
        case 2: gram2_kernel<2, true><<<nwg, 256, pad, st>>>(GRAM2_ARGS); break;
        default: gram2_kernel<3, true><<<nwg, 256, pad, st>>>(GRAM2_ARGS); break;
      }
    } else {
      switch (sdim) {
        case 1: gram2_kernel<1, false><<<nwg, 256, 0, st>>>(GRAM2_ARGS); break;
        case 2: gram2_kernel<2, false><<<nwg, 256, 0, st>>>(GRAM2_ARGS); break;
        default: gram2_kernel<3, false><<<nwg, 256, 0, st>>>(GRAM2_ARGS); break;
      }
    }
#undef GRAM2_ARGS
    const int nrows = plan.noff * 4 * 16 + plan.ndg * 4 * kD2T + 1;
    gram2_reduce<<<nrows, 256, 0, st>>>(part, rpart, plan.npan, plan.noff, plan.ndg, plan.soff, plan.sdg, G, ldg, r,
                                        nullptr);
  }
}

// v3 over ngrp outputs of one size in one set of launches (grid y = output; per-output pointers
// from the device table grp: GramGroupPtrs), with the chunk correction (the objective's form)
void launch_gram_grouped(hipStream_t st, int sdim, const GramPlan& plan, const GramGroupPtrs* grp,
                         int ngrp, int64_t ldb, int64_t n, int64_t mc, int L, int64_t ldg,
                         hipStream_t side, hipEvent_t ev_a, hipEvent_t ev_b) {
  const bool corun = side && plan.noff > 0;
  const int ncs = corun ? plan.ncs_slim : plan.ncs;
  const int noffw = ((plan.noff * plan.soff + 7) / 8) * 8;   // XCD deal (per grid row)
  const int ndgw = ((plan.ndg * plan.sdg + 7) / 8) * 8;
  const int64_t nchk = (n + L - 1) / L;
  if (corun) {
    HIPCHECK_G(hipEventRecord(ev_a, st));
    HIPCHECK_G(hipStreamWaitEvent(side, ev_a, 0));
  }
  if (noffw > 0)
    gram3_off_kernel<<<dim3((unsigned)noffw, (unsigned)ngrp), 128, 0, st>>>(
        nullptr, ldb, n, plan.noff, plan.soff, plan.rows_off, nullptr, grp);
  if (corun)
    launch_gram3_corr_slim(side, sdim, nullptr, nullptr, nullptr, mc, nchk, plan.npan, plan.noff,
                           plan.ndg, plan.soff, plan.sdg, ncs, nullptr, nullptr, grp, ngrp);
  const int64_t dslot0 = (int64_t)plan.noff * (plan.soff + ncs);
  launch_gram3_dg(st, ndgw, nullptr, ldb, n, nullptr, plan.npan, plan.ndg, plan.sdg, plan.rows_dg,
                  dslot0, nullptr, nullptr, 0, -1, 0, 0, grp, ngrp);
  if (corun) {
    HIPCHECK_G(hipEventRecord(ev_b, side));
    HIPCHECK_G(hipStreamWaitEvent(st, ev_b, 0));
  } else {
    launch_gram3_corr(st, sdim, nullptr, nullptr, nullptr, mc, nchk, plan.npan, plan.noff, plan.ndg,
                      plan.soff, plan.sdg, ncs, nullptr, nullptr, grp, ngrp);
  }
  const int nrows = plan.noff * 2 * kF3T + plan.ndg * 2 * kD2T + 1;
  gram3_reduce<<<dim3((unsigned)nrows, (unsigned)ngrp), 256, 0, st>>>(
      nullptr, nullptr, plan.npan, plan.noff, plan.ndg, plan.soff, plan.sdg, ncs, nullptr, ldg,
      nullptr, grp);
}

void launch_gram_scale(hipStream_t st, const GramScaleJob* jobs_dev, int njobs, int64_t mpmax) {
  if (njobs <= 0 || mpmax <= 0) return;
  gram_scale_kernel<<<dim3((unsigned)mpmax, (unsigned)njobs), 256, 0, st>>>(jobs_dev);
}

void launch_beta_fix(hipStream_t st, int sdim, double* beta, int64_t ldb, int64_t n,
                     const double* g, const double* cin, int64_t mc, int L) {
  const unsigned nb = (unsigned)((n * ldb + 255) / 256);
  switch (sdim) {
    case 1: beta_fix_kernel<1><<<nb, 256, 0, st>>>(beta, ldb, n, g, cin, mc, L); break;
    case 2: beta_fix_kernel<2><<<nb, 256, 0, st>>>(beta, ldb, n, g, cin, mc, L); break;
    default: beta_fix_kernel<3><<<nb, 256, 0, st>>>(beta, ldb, n, g, cin, mc, L); break;
  }
}

}  // namespace gpar
