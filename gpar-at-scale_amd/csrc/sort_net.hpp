// sort_net.hpp -- the sorting pieces k_quantile.hip and k_score.hip share: Batcher's odd-even
// mergesort as a fully unrolled compare-exchange network over a register array, one step of the
// bitonic network over lists in LDS, and the quantile interpolation (numpy's _lerp).
#pragma once
#include <cstddef>
#include <utility>

#include "nm_dev.hpp"

namespace gpar {

__device__ __forceinline__ double quant_lerp(double a, double b, double g) {
  GPAR_NO_FMA
  if (g == 0.0 || a == b) return a;
  const double d = b - a;
  if (g < 0.5) return a + d * g;
  return b - d * (1.0 - g);
}

// ---------------------------------------------------------------------------- the network
// Batcher's odd-even mergesort on N = 2^k wires as a list of exchanges (lo wire, hi wire)
constexpr int oem_count(int N) {
  int cnt = 0;
  for (int p = 1; p < N; p *= 2)
    for (int k = p; k >= 1; k /= 2)
      for (int j = k % p; j + k < N; j += 2 * k)
        for (int i = 0; i < k && i + j + k < N; ++i)
          if ((i + j) / (2 * p) == (i + j + k) / (2 * p)) ++cnt;
  return cnt;
}

template <int N>
struct OemNet {
  static constexpr int count = oem_count(N);
  unsigned char a[count], b[count];
  constexpr OemNet() : a{}, b{} {
    int cnt = 0;
    for (int p = 1; p < N; p *= 2)
      for (int k = p; k >= 1; k /= 2)
        for (int j = k % p; j + k < N; j += 2 * k)
          for (int i = 0; i < k && i + j + k < N; ++i)
            if ((i + j) / (2 * p) == (i + j + k) / (2 * p)) {
              a[cnt] = (unsigned char)(i + j);
              b[cnt] = (unsigned char)(i + j + k);
              ++cnt;
            }
  }
};
static_assert(oem_count(16) == 63 && oem_count(32) == 191 && oem_count(64) == 543 &&
                  oem_count(128) == 1471,
              "Batcher odd-even mergesort exchange counts");

template <int N>
struct OemTable {
  static constexpr OemNet<N> net{};
};

template <int N, size_t I>
__device__ __forceinline__ int quant_cx(double (&x)[N]) {
  constexpr int ia = OemTable<N>::net.a[I], ib = OemTable<N>::net.b[I];
  const double lo = fmin(x[ia], x[ib]), hi = fmax(x[ia], x[ib]);
  x[ia] = lo;
  x[ib] = hi;
  return 0;
}

template <int N, size_t... I>
__device__ __forceinline__ void oem_apply(double (&x)[N], std::index_sequence<I...>) {
  const int done[] = {quant_cx<N, I>(x)...};
  (void)done;
}

template <int N>
__device__ __forceinline__ void oem_sort(double (&x)[N]) {
  oem_apply<N>(x, std::make_index_sequence<(size_t)OemNet<N>::count>{});
}

// ---------------------------------------------------------------------------- LDS lists
// Bitonic sort, ascending, of the G lists of NP2 = 2^k doubles at sh[l * NP2 ...] by a 256-thread
// workgroup (every thread calls it; the lists are written and a barrier passed before the call,
// and a barrier follows the last step)
__device__ __forceinline__ void bitonic_sort_lists(double* sh, int NP2, int G, int tid) {
  const int half = G * NP2 / 2;
  for (int k = 2; k <= NP2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < half; t += 256) {
        // the t-th pair (u, u + j) over all lists: u's bit j is clear
        const int u = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const int w = u & (NP2 - 1);   // position within its list (NP2 divides the list stride)
        const double a = sh[u], b = sh[u + j];
        const double mn = fmin(a, b), mx = fmax(a, b);
        const bool up = (w & k) == 0;
        sh[u] = up ? mn : mx;
        sh[u + j] = up ? mx : mn;
      }
      __syncthreads();
    }
}

}  // namespace gpar
