// k_kmeans.hip -- pseudo-input selection: Lloyd's k-means over one output's inputs (gfx950).
//
// The library's entry points take the pseudo-inputs Z as given; gpar_select_pseudo_inputs places
// them.  One Lloyd iteration is {assign every input v_k to its nearest centre; move every centre
// to the mean of its members}.
//
// Assignment (the hot path, 2 n m d flop): the contraction of k_dist.hip's dist2_mfma_kernel,
//
//   d2[k][c] = |v_k - g|^2 + |z_c - g|^2 - 2 (v_k - g).(z_c - g),   g = mean of the centres,
//
// on v_mfma_f64_16x16x4_f64 with D streamed through LDS in 16-wide K-steps, but the n x m matrix
// is never stored: a workgroup owns 128 rows, loops over the 128-centre tiles and keeps each row's
// running (min, argmin) in registers.  Ties go to the lowest centre index: equal rows of Z see the
// same operations in the same order whatever tile they sit in, so their distances are equal bit
// for bit.  Outputs label / dmin per row, integer-atomic counts per cluster (one atomic per
// distinct label of a row tile) and one inertia partial per row tile, summed in fixed order.
//
// Update: the sums of the members are per-split partial sums in a fixed layout
// (part[split][c][i]), each accumulated in row order by the one thread that owns (c mod 16, i),
// then summed over the splits in order (compensated sums): no floating-point atomics, the same
// bits every run.  The
// one-hot contraction L^T V on MFMA would cost the assignment's 2 n m d flop again plus the same
// split partials (its output is only m x d); the owner-thread form reads V once and costs
// O(n d) adds.
//
// Snap: each non-empty cluster's centre becomes its member row nearest to it -- a 64-bit integer
// atomic-min over the bit pattern of the (non-negative) dmin per cluster, then an atomic-min of
// the row index among the rows attaining it.
#include "device_common.hpp"

namespace gpar {

typedef double d4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------- centre of the centres
// g[i] = mean_c z[c][i]: 16 dimensions per workgroup, 16 row lanes each summing the centres
// c = j (mod 16) in order, the lanes then summed in order.
__global__ __launch_bounds__(256) void kmeans_center_kernel(const double* __restrict__ z,
                                                            int64_t ldz, int64_t m, int d,
                                                            double* __restrict__ g) {
  __shared__ double ps[16][17];
  const int i = threadIdx.x & 15, j = threadIdx.x >> 4;
  const int dim = blockIdx.x * 16 + i;
  double s = 0.0;
  if (dim < d)
    for (int64_t c = j; c < m; c += 16) s += z[c * ldz + dim];
  ps[j][i] = s;
  __syncthreads();
  if (j == 0 && dim < d) {
    double t = 0.0;
    for (int q = 0; q < 16; ++q) t += ps[q][i];
    g[dim] = t / (double)m;
  }
}

// ---------------------------------------------------------------------------- assignment
// 128 rows per 256-thread workgroup, 2 x 2 waves of 4 x 4 MFMA tiles against each 128-centre
// tile in turn (the tile, K-step and LDS padding of dist2_mfma_kernel).  C layout: a lane holds
// rows frow + 4 r, column fcol of each 16 x 16 tile, so a row's candidates sit in the 16 lanes of
// one frow (shuffle reduction) of both column waves (LDS).
constexpr int kKT = 128, kKBK = 16, kKLds = 136;

__device__ __forceinline__ void kmeans_take_lower(double& x, int& ix, double ox, int oi) {
  if (ox < x || (ox == x && oi < ix)) {
    x = ox;
    ix = oi;
  }
}

__global__ __launch_bounds__(256, 2) void kmeans_assign_kernel(
    const double* __restrict__ v, int64_t ldv, int64_t n, const double* __restrict__ z,
    int64_t ldz, int64_t m, int d, const double* __restrict__ cg, int32_t* __restrict__ label,
    double* __restrict__ dmin, unsigned long long* __restrict__ count,
    double* __restrict__ ipart) {
  __shared__ __attribute__((aligned(16))) double smem[2 * 2 * kKBK * kKLds];
  __shared__ double vn_s[kKT], zn_s[kKT];
  __shared__ double red_d[2][kKT];
  __shared__ int red_i[2][kKT];
  __shared__ int lab_s[kKT];
  __shared__ double sum_s[kKT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int64_t r0 = (int64_t)blockIdx.x * kKT;
  const int srow = tid >> 1, sk = (tid & 1) * 8;
  const int64_t arow = r0 + srow;
  const bool av = arow < n;
  const int64_t arc = av ? arow : n - 1;
  const int frow = lane >> 4, fcol = lane & 15;
  const int nsteps = (d + kKBK - 1) / kKBK;
  double bd[4][4];
  int bi[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      bd[a][r] = __builtin_huge_val();
      bi[a][r] = 0;
    }
  const int64_t ntile = (m + kKT - 1) / kKT;
  for (int64_t ct = 0; ct < ntile; ++ct) {
    const int64_t c0 = ct * kKT;
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
      double* la = smem + (buf * 2 + 0) * kKBK * kKLds;
      double* lb = smem + (buf * 2 + 1) * kKBK * kKLds;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        la[(sk + q) * kKLds + srow] = ra[q];
        lb[(sk + q) * kKLds + srow] = rb[q];
      }
    };
    d4 acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[a][c] = d4{0.0, 0.0, 0.0, 0.0};
    // (every wave left the previous tile's K-loop and norms behind the barriers that end them)
    load(0);
    store(0);
    __syncthreads();
    for (int s = 0; s < nsteps; ++s) {
      const int buf = s & 1;
      const bool more = s + 1 < nsteps;
      if (more) load((s + 1) * kKBK);
      const double* la = smem + (buf * 2 + 0) * kKBK * kKLds;
      const double* lb = smem + (buf * 2 + 1) * kKBK * kKLds;
#pragma unroll
      for (int ks = 0; ks < kKBK / 4; ++ks) {
        double fa[4], fb[4];
        const int kr = ks * 4 + frow;
#pragma unroll
        for (int a = 0; a < 4; ++a) fa[a] = la[kr * kKLds + wr * 64 + a * 16 + fcol];
#pragma unroll
        for (int c = 0; c < 4; ++c) fb[c] = lb[kr * kKLds + wc * 64 + c * 16 + fcol];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int c = 0; c < 4; ++c)
            acc[a][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[a], fb[c], acc[a][c], 0, 0, 0);
      }
      if (more) store(buf ^ 1);
      __syncthreads();
    }
    // row norms: the two staging threads of a row hold complementary halves of every K-step
    an += __shfl_xor(an, 1, 64);
    bn += __shfl_xor(bn, 1, 64);
    if ((tid & 1) == 0) {
      vn_s[srow] = an;
      zn_s[srow] = bn;
    }
    __syncthreads();
    // the tile's candidates in rising column order: a strict < keeps the lowest index
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double vn = vn_s[wr * 64 + a * 16 + frow + 4 * r];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int cl = wc * 64 + c * 16 + fcol;
          const int64_t col = c0 + cl;
          double d2 = vn + zn_s[cl] - 2.0 * acc[a][c][r];
          d2 = d2 > 0.0 ? d2 : 0.0;
          if (col < m && d2 < bd[a][r]) {
            bd[a][r] = d2;
            bi[a][r] = (int)col;
          }
        }
      }
    // vn_s / zn_s are next written behind the next tile's K-loop barriers
  }
  // a row's 16 lanes, then its two column waves
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      double x = bd[a][r];
      int ix = bi[a][r];
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) {
        const double ox = __shfl_xor(x, off, 64);
        const int oi = __shfl_xor(ix, off, 64);
        kmeans_take_lower(x, ix, ox, oi);
      }
      if (fcol == 0) {
        const int rl = wr * 64 + a * 16 + frow + 4 * r;
        red_d[wc][rl] = x;
        red_i[wc][rl] = ix;
      }
    }
  __syncthreads();
  int mine = -1;
  if (tid < kKT) {
    double x = red_d[0][tid];
    int ix = red_i[0][tid];
    kmeans_take_lower(x, ix, red_d[1][tid], red_i[1][tid]);
    const int64_t row = r0 + tid;
    const bool valid = row < n;
    if (valid) {
      label[row] = ix;
      dmin[row] = x;
      mine = ix;
    }
    lab_s[tid] = mine;
    sum_s[tid] = valid ? x : 0.0;
  }
  __syncthreads();
  // counts: one integer atomic per distinct label of the tile (its first row adds the tally)
  if (mine >= 0) {
    bool first = true;
    unsigned long long cnt = 0;
    for (int r = 0; r < kKT; ++r)
      if (lab_s[r] == mine) {
        if (r < tid) first = false;
        ++cnt;
      }
    if (first) atomicAdd(&count[mine], cnt);
  }
  // the tile's inertia: a fixed tree
  for (int s = kKT / 2; s > 0; s >>= 1) {
    if (tid < s) sum_s[tid] += sum_s[tid + s];
    __syncthreads();
  }
  if (tid == 0) ipart[blockIdx.x] = sum_s[0];
}

// *out = sum of the row tiles' partials: each thread its tiles in order, then a fixed tree.
__global__ __launch_bounds__(256) void kmeans_inertia_kernel(const double* __restrict__ ipart,
                                                             int64_t nb, double* __restrict__ out) {
  __shared__ double sh[256];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int64_t b = tid; b < nb; b += 256) s += ipart[b];
  sh[tid] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) sh[tid] += sh[tid + w];
    __syncthreads();
  }
  if (tid == 0) out[0] = sh[0];
}

// ---------------------------------------------------------------------------- update
// part[s][c][i] = sum of v[k][i] over the rows k of split s labelled c, in row order.  grid
// (splits, ceil(d / 16), ceil(m / 256)): a workgroup scans its split's labels, 64 rows at a time
// staged through LDS with their 16-dimension slice of V, and thread (q, i) adds the rows whose
// cluster c = q (mod 16) lies in the workgroup's 256-cluster tile into its own LDS accumulator
// [c][i]: every accumulator has one owner and sees its rows in order (the rows of a thread's
// clusters come from wave ballots over the staged labels, so a wave steps only through rows that
// one of its four q owns; scanning every row per wave took 1.25 ms at N = 1e6, M = 512, D = 32,
// as long as the assignment).  The sums are compensated
// (each addition's rounding error is kept in a second accumulator, part[...][1]), so a mean that
// comes out near zero from members of size one keeps its relative accuracy.
constexpr int kKUC = 256, kKUR = 64, kKUD = 16;

// s + x exactly: the rounded sum in s, its rounding error added to e
__device__ __forceinline__ void kmeans_two_sum(double& s, double& e, double x) {
  const double t = s + x;
  const double bp = t - s;
  e += (s - (t - bp)) + (x - bp);
  s = t;
}

__global__ __launch_bounds__(256, 2) void kmeans_sums_kernel(
    const double* __restrict__ v, int64_t ldv, int64_t n, const int32_t* __restrict__ label,
    int64_t m, int d, int64_t rows_per_split, double* __restrict__ part) {
  __shared__ double acc[kKUC * kKUD], err[kKUC * kKUD];
  __shared__ double vs[kKUR * kKUD];
  __shared__ int lab[kKUR];
  static_assert(kKUR == 64, "one lane tests one staged row");
  const int tid = threadIdx.x, i = tid & 15, lane = tid & 63;   // q = tid >> 4
  const int64_t s = blockIdx.x;
  const int i0 = blockIdx.y * kKUD;
  const int64_t c0 = (int64_t)blockIdx.z * kKUC;
  for (int e = tid; e < kKUC * kKUD; e += 256) acc[e] = err[e] = 0.0;
  const int64_t k_lo = s * rows_per_split;
  const int64_t k_hi = (k_lo + rows_per_split < n) ? k_lo + rows_per_split : n;
  // a tile's labels and V slice are fetched into registers one tile ahead (a thread's four
  // elements e = tid + 256 j sit in rows (tid >> 4) + 16 j, dimension i)
  int plab = -1;
  double pv[4];
  auto fetch = [&](int64_t kb) {
    plab = (tid < kKUR && kb + tid < k_hi) ? (int)((int64_t)label[kb + tid] - c0) : -1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t k = kb + (tid >> 4) + 16 * j;
      pv[j] = (k < k_hi && i0 + i < d) ? v[k * ldv + i0 + i] : 0.0;
    }
  };
  if (k_lo < k_hi) fetch(k_lo);
  for (int64_t kb = k_lo; kb < k_hi; kb += kKUR) {
    __syncthreads();
    if (tid < kKUR) lab[tid] = plab;
#pragma unroll
    for (int j = 0; j < 4; ++j) vs[tid + 256 * j] = pv[j];
    __syncthreads();
    if (kb + kKUR < k_hi) fetch(kb + kKUR);
    // the staged rows of the thread's clusters as a bit mask (lane r tests row r, one ballot per q
    // of the wave), then walked in row order
    const int mylab = lab[lane];
    unsigned long long rows = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned long long hit =
          __ballot((unsigned)mylab < (unsigned)kKUC && (mylab & 15) == ((tid >> 6) << 2) + j);
      if (j == (lane >> 4)) rows = hit;
    }
    while (rows) {
      const int r = __ffsll(rows) - 1;
      rows &= rows - 1;
      const int l = lab[r];
      double a = acc[l * kKUD + i], b = err[l * kKUD + i];
      kmeans_two_sum(a, b, vs[r * kKUD + i]);
      acc[l * kKUD + i] = a;
      err[l * kKUD + i] = b;
    }
  }
  __syncthreads();
  for (int e = tid; e < kKUC * kKUD; e += 256) {
    const int64_t c = c0 + (e >> 4);
    const int dim = i0 + (e & 15);
    if (c < m && dim < d) {
      double* o = part + 2 * ((s * m + c) * d + dim);
      o[0] = acc[e];
      o[1] = err[e];
    }
  }
}

// z[c][i] = (compensated sum over the splits, in order) / count[c] for the non-empty clusters; an
// empty cluster's centre is not touched.
__global__ __launch_bounds__(256) void kmeans_mean_kernel(const double* __restrict__ part,
                                                          int nsplit,
                                                          const unsigned long long* __restrict__ count,
                                                          int64_t m, int d, double* __restrict__ z,
                                                          int64_t ldz) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= m * d) return;
  const int64_t c = e / d;
  const int dim = (int)(e - c * d);
  const unsigned long long cnt = count[c];
  if (cnt == 0) return;
  double s = 0.0, r = 0.0;
  for (int q = 0; q < nsplit; ++q) {
    const double* p = part + 2 * (((int64_t)q * m + c) * d + dim);
    kmeans_two_sum(s, r, p[0]);
    r += p[1];
  }
  z[c * ldz + dim] = (s + r) / (double)cnt;
}

// ---------------------------------------------------------------------------- snap
// best[c] = min over the members of cluster c of dmin's bit pattern (dmin >= 0: the patterns
// order as the values do)
__global__ __launch_bounds__(256) void kmeans_snap_min_kernel(const int32_t* __restrict__ label,
                                                              const double* __restrict__ dmin,
                                                              int64_t n,
                                                              unsigned long long* __restrict__ best) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k < n) atomicMin(&best[label[k]], (unsigned long long)__double_as_longlong(dmin[k]));
}

// idx[c] = the lowest member row attaining best[c]
__global__ __launch_bounds__(256) void kmeans_snap_row_kernel(
    const int32_t* __restrict__ label, const double* __restrict__ dmin, int64_t n,
    const unsigned long long* __restrict__ best, unsigned long long* __restrict__ idx) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const int32_t c = label[k];
  if ((unsigned long long)__double_as_longlong(dmin[k]) == best[c])
    atomicMin(&idx[c], (unsigned long long)k);
}

// z[c] = v[idx[c]] for the non-empty clusters (idx[c] = all ones: empty, untouched)
__global__ __launch_bounds__(256) void kmeans_snap_copy_kernel(
    const double* __restrict__ v, int64_t ldv, const unsigned long long* __restrict__ idx,
    int64_t m, int d, double* __restrict__ z, int64_t ldz) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= m * d) return;
  const int64_t c = e / d;
  const int dim = (int)(e - c * d);
  const unsigned long long k = idx[c];
  if (k == ~0ull) return;
  z[c * ldz + dim] = v[(int64_t)k * ldv + dim];
}

}  // namespace gpar

// ============================================================================ launch wrappers
#include "launch.hpp"

namespace gpar {

void launch_kmeans_center(hipStream_t st, const double* z, int64_t ldz, int64_t m, int d,
                          double* g) {
  kmeans_center_kernel<<<(unsigned)((d + 15) / 16), 256, 0, st>>>(z, ldz, m, d, g);
}

int64_t kmeans_assign_blocks(int64_t n) { return (n + kKT - 1) / kKT; }

void launch_kmeans_assign(hipStream_t st, const double* v, int64_t ldv, int64_t n, const double* z,
                          int64_t ldz, int64_t m, int d, const double* g, int32_t* label,
                          double* dmin, unsigned long long* count, double* ipart) {
  kmeans_assign_kernel<<<(unsigned)kmeans_assign_blocks(n), 256, 0, st>>>(
      v, ldv, n, z, ldz, m, d, g, label, dmin, count, ipart);
}

void launch_kmeans_inertia(hipStream_t st, const double* ipart, int64_t nb, double* out) {
  kmeans_inertia_kernel<<<1, 256, 0, st>>>(ipart, nb, out);
}

// 2048 rows per split, at most 256 splits, and at most 256 MB of partials (two doubles per sum)
int kmeans_sum_splits(int64_t n, int64_t m, int d) {
  int64_t s = (n + 2047) / 2048;
  if (s > 256) s = 256;
  while (s > 1 && (double)s * (double)m * (double)d * 16.0 > 268435456.0) s /= 2;
  return (int)s;
}

void launch_kmeans_update(hipStream_t st, const double* v, int64_t ldv, int64_t n,
                          const int32_t* label, const unsigned long long* count, int64_t m, int d,
                          double* part, double* z, int64_t ldz) {
  const int ns = kmeans_sum_splits(n, m, d);
  const int64_t rps = ((n + ns - 1) / ns + kKUR - 1) / kKUR * kKUR;
  dim3 grid((unsigned)ns, (unsigned)((d + kKUD - 1) / kKUD), (unsigned)((m + kKUC - 1) / kKUC));
  kmeans_sums_kernel<<<grid, 256, 0, st>>>(v, ldv, n, label, m, d, rps, part);
  kmeans_mean_kernel<<<(unsigned)((m * d + 255) / 256), 256, 0, st>>>(part, ns, count, m, d, z,
                                                                      ldz);
}

void launch_kmeans_snap(hipStream_t st, const double* v, int64_t ldv, int64_t n,
                        const int32_t* label, const double* dmin, int64_t m, int d,
                        unsigned long long* best, unsigned long long* idx, double* z,
                        int64_t ldz) {
  const unsigned nb = (unsigned)((n + 255) / 256);
  kmeans_snap_min_kernel<<<nb, 256, 0, st>>>(label, dmin, n, best);
  kmeans_snap_row_kernel<<<nb, 256, 0, st>>>(label, dmin, n, best, idx);
  kmeans_snap_copy_kernel<<<(unsigned)((m * d + 255) / 256), 256, 0, st>>>(v, ldv, idx, m, d, z,
                                                                           ldz);
}

}  // namespace gpar
