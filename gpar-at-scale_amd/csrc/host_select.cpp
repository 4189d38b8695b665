// host_select.cpp -- gpar_select_pseudo_inputs: Lloyd's k-means over one output's inputs
// (k_kmeans.hip).  Workspaces are O(n + m d + the update's split partials), never n x m.
#include "host.hpp"

#include <climits>

using namespace gpar;

extern "C" int32_t gpar_select_pseudo_inputs(gpar_ctx* ctx, int64_t n, int64_t d, const double* v,
                                             int64_t ldv, int64_t m, const double* z0,
                                             int64_t ldz0, int32_t iters, int32_t snap, int32_t mem,
                                             double* z_out, int64_t ldz_out, int64_t* index_out,
                                             int32_t* label_out, int64_t* count_out,
                                             double* inertia_out) {
  API_BEGIN(ctx)
  ARGCHECK(v && z0 && z_out, "gpar_select_pseudo_inputs: v, z0 and z_out must not be NULL");
  ARGCHECK(mem == GPAR_MEM_HOST || mem == GPAR_MEM_DEVICE,
           "gpar_select_pseudo_inputs: mem must be GPAR_MEM_HOST or GPAR_MEM_DEVICE");
  ARGCHECK(n >= 1 && d >= 1 && m >= 1, "gpar_select_pseudo_inputs: n, d and m must be >= 1");
  ARGCHECK(m <= n, "gpar_select_pseudo_inputs: more centres than inputs (m > n)");
  ARGCHECK(m <= INT32_MAX && d <= INT32_MAX, "gpar_select_pseudo_inputs: m or d too large");
  ARGCHECK(ldv >= d && ldz0 >= d && ldz_out >= d,
           "gpar_select_pseudo_inputs: a leading dimension is below d");
  ARGCHECK(iters >= 0, "gpar_select_pseudo_inputs: iters must be >= 0");
  const bool dev = mem == GPAR_MEM_DEVICE;
  const hipMemcpyKind in_kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  const hipMemcpyKind out_kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  hipStream_t st = ctx->stream;
  const int di = (int)d;
  // inputs: device V is read in place; the centres always work in a copy (z_out may alias z0)
  const double* dv = v;
  int64_t dldv = ldv;
  if (!dev) {
    double* vb = ws<double>(ctx, "km_v", (size_t)n * d);
    h2d_rows(ctx, vb, v, ldv, d, n);
    dv = vb;
    dldv = d;
  }
  double* zc = ws<double>(ctx, "km_z", (size_t)m * d);
  HIPCHECK(hipMemcpy2DAsync(zc, d * sizeof(double), z0, ldz0 * sizeof(double), d * sizeof(double),
                            m, in_kind, st));
  double* g = ws<double>(ctx, "km_g", (size_t)d);
  int32_t* label = ws<int32_t>(ctx, "km_label", (size_t)n);
  double* dmin = ws<double>(ctx, "km_dmin", (size_t)n);
  auto* count = ws<unsigned long long>(ctx, "km_count", (size_t)m);
  const int64_t nb = kmeans_assign_blocks(n);
  double* ipart = ws<double>(ctx, "km_ipart", (size_t)nb);
  double* iner = ws<double>(ctx, "km_inertia", (size_t)iters + 1);
  double* part = nullptr;
  if (iters > 0)
    part = ws<double>(ctx, "km_part", (size_t)kmeans_sum_splits(n, m, di) * m * d * 2);
  const double flops = 2.0 * (double)n * (double)m * (double)d;
  for (int it = 0; it <= iters; ++it) {
    Timed tk_(ctx, "kmeans", flops);
    {
      Timed ta_(ctx, "kmeans_assign", flops);
      launch_kmeans_center(st, zc, d, m, di, g);
      HIPCHECK(hipMemsetAsync(count, 0, (size_t)m * sizeof(unsigned long long), st));
      launch_kmeans_assign(st, dv, dldv, n, zc, d, m, di, g, label, dmin, count, ipart);
      launch_kmeans_inertia(st, ipart, nb, iner + it);
      check_launch("kmeans assign");
    }
    if (it < iters) {
      Timed tu_(ctx, "kmeans_update", 8.0 * (double)n * (double)d);
      launch_kmeans_update(st, dv, dldv, n, label, count, m, di, part, zc, d);
      check_launch("kmeans update");
    }
  }
  // index: all ones (-1) unless snapped
  auto* idx = ws<unsigned long long>(ctx, "km_index", (size_t)m);
  HIPCHECK(hipMemsetAsync(idx, 0xFF, (size_t)m * sizeof(unsigned long long), st));
  if (snap) {
    auto* best = ws<unsigned long long>(ctx, "km_best", (size_t)m);
    HIPCHECK(hipMemsetAsync(best, 0xFF, (size_t)m * sizeof(unsigned long long), st));
    launch_kmeans_snap(st, dv, dldv, n, label, dmin, m, di, best, idx, zc, d);
    check_launch("kmeans snap");
  }
  HIPCHECK(hipMemcpy2DAsync(z_out, ldz_out * sizeof(double), zc, d * sizeof(double),
                            d * sizeof(double), m, out_kind, st));
  if (index_out)
    HIPCHECK(hipMemcpyAsync(index_out, idx, (size_t)m * sizeof(int64_t), out_kind, st));
  if (label_out)
    HIPCHECK(hipMemcpyAsync(label_out, label, (size_t)n * sizeof(int32_t), out_kind, st));
  if (count_out)
    HIPCHECK(hipMemcpyAsync(count_out, count, (size_t)m * sizeof(int64_t), out_kind, st));
  if (inertia_out) d2h(ctx, inertia_out, iner, (size_t)iters + 1);
  sync(ctx);
  API_END(ctx)
}
