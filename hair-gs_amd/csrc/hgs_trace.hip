// hgs_trace.hip -- strands traced from the scalp through the lifted hair directions (utils/trace.py states the contract, its numpy
// paths and the loop restatement in tests/trace_reference.py state the same thing; trace_strands.py is the scene driver):
// hgs_field_splat, hgs_field_solve, hgs_strand_trace.  gfx950, wave64.  Built with -ffp-contract=off: all arithmetic is float64,
// rounded once per operation, in the order written.  dot(u, v) = (u0*v0 + u1*v1) + u2*v2.
//
// field_splat_kernel: one lane per point of the directed cloud, 256 per block.  A point that is not finite, or whose dot(dir, dir)
//   is not finite or not > 0, adds one to `skipped` and nothing else.  The others walk a box of span^3 nodes (span is the host's:
//   wavefront-uniform) that holds every node closer than r, test d2 < r2 on each node of it that lies on the grid, and add
//   rint(k * 2^32) and the six rint((k * m) * 2^32) to the node's seven int64 sums with 64-bit integer atomics.  Integer addition
//   is associative: the sums are the same bits whatever the arrival order, the launch shape or the split of the cloud, and equal to
//   the numpy path's.  (The gather form -- one lane per node over all points -- needs a spatial index to be anything but nodes x
//   points pair tests; float atomics would make the sums depend on the order.  DESIGN.md 8 has the sizing.)  A node's seven sums lie
//   in 56 contiguous bytes, so the seven atomics of a lane go to one or two 64-byte lines.
// field_solve_kernel: one lane per node; cyclic Jacobi on T = Tq * 2^-32 in registers (hgs_jacobi3.h).
// strand_trace_kernel: one lane per root; the bounded loop of the contract, the range test in front of every load.
#include "hgs_common.h"
#include "hgs_jacobi3.h"

#include <math.h>

#define HGS_TRACE_MAX_NODES (1ll << 26)
#define HGS_TRACE_MAX_POINTS (1 << 24)
#define HGS_TRACE_MAX_STEPS 4096
#define HGS_TRACE_MAX_REACH 8.0      // r <= 8 h: the box a lane walks has at most 18^3 nodes

namespace {

#define TRACE_BLOCK 256
#define FIXED_ONE 4294967296.0       // 2^32

__device__ __forceinline__ bool finite3(double x, double y, double z) {
  const double big = __builtin_inf();
  return fabs(x) < big && fabs(y) < big && fabs(z) < big;
}

__device__ __forceinline__ void add64(long long* p, long long v) {
  atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);   // (two's complement: the wrap is the signed sum)
}

// First node of the box along one axis, or a value that leaves the box empty.  t - reach is taken in float64 and clamped to
// [-span, n] before the conversion, so no value of t (huge, infinite) overflows the integer.
__device__ __forceinline__ int box_start(double x, double o, double k, double reach, int span, int n) {
  double lo = floor((x - o) * k - reach);
  if (!(lo > (double)(-span))) lo = (double)(-span);                            // (also a NaN: an empty box)
  if (!(lo < (double)n)) lo = (double)n;
  return (int)lo;
}

__global__ __launch_bounds__(TRACE_BLOCK) void field_splat_kernel(int N, const double* __restrict__ points, const double* __restrict__ dirs,
                                                                  double ox, double oy, double oz, double h, double k, int nx, int ny,
                                                                  int nz, double r2, double reach, int span,
                                                                  long long* __restrict__ acc, int* __restrict__ skipped) {
  const int i = blockIdx.x * TRACE_BLOCK + threadIdx.x;
  if (i >= N) return;
  const double x = points[3 * (size_t)i], y = points[3 * (size_t)i + 1], z = points[3 * (size_t)i + 2];
  double d0 = dirs[3 * (size_t)i], d1 = dirs[3 * (size_t)i + 1], d2v = dirs[3 * (size_t)i + 2];
  const double dd = dot3(d0, d1, d2v, d0, d1, d2v);
  if (!finite3(x, y, z) || !(dd > 0.0 && dd < __builtin_inf())) {
    atomicAdd(skipped, 1);
    return;
  }
  const double len = sqrt(dd);
  d0 = d0 / len; d1 = d1 / len; d2v = d2v / len;
  const double mxx = d0 * d0, mxy = d0 * d1, mxz = d0 * d2v, myy = d1 * d1, myz = d1 * d2v, mzz = d2v * d2v;
  const int bx = box_start(x, ox, k, reach, span, nx), by = box_start(y, oy, k, reach, span, ny), bz = box_start(z, oz, k, reach, span, nz);
  for (int cz = 0; cz < span; cz++) {
    const int iz = bz + cz;
    if (iz < 0 || iz >= nz) continue;
    const double ez = (oz + (double)iz * h) - z;
    for (int cy = 0; cy < span; cy++) {
      const int iy = by + cy;
      if (iy < 0 || iy >= ny) continue;
      const double ey = (oy + (double)iy * h) - y;
      for (int cx = 0; cx < span; cx++) {
        const int ix = bx + cx;
        if (ix < 0 || ix >= nx) continue;
        const double ex = (ox + (double)ix * h) - x;
        const double dist2 = dot3(ex, ey, ez, ex, ey, ez);
        if (!(dist2 < r2)) continue;
        const double w = 1.0 - dist2 / r2;
        long long* a = acc + 7 * (((size_t)iz * ny + iy) * nx + ix);
        add64(a + 0, (long long)rint(w * FIXED_ONE));
        add64(a + 1, (long long)rint((w * mxx) * FIXED_ONE));
        add64(a + 2, (long long)rint((w * mxy) * FIXED_ONE));
        add64(a + 3, (long long)rint((w * mxz) * FIXED_ONE));
        add64(a + 4, (long long)rint((w * myy) * FIXED_ONE));
        add64(a + 5, (long long)rint((w * myz) * FIXED_ONE));
        add64(a + 6, (long long)rint((w * mzz) * FIXED_ONE));
      }
    }
  }
}

__global__ __launch_bounds__(TRACE_BLOCK) void field_solve_kernel(long long nodes, const long long* __restrict__ acc,
                                                                  double* __restrict__ dir, double* __restrict__ conf) {
  const long long i = (long long)blockIdx.x * TRACE_BLOCK + threadIdx.x;
  if (i >= nodes) return;
  const long long* __restrict__ a = acc + 7 * (size_t)i;
  const double scale = 1.0 / FIXED_ONE;                                           // 2^-32, exact
  double a00 = (double)a[1] * scale, a01 = (double)a[2] * scale, a02 = (double)a[3] * scale;
  double a11 = (double)a[4] * scale, a12 = (double)a[5] * scale, a22 = (double)a[6] * scale;
  double dx = 0.0, dy = 0.0, dz = 0.0, c = 0.0;
  const double big = __builtin_inf();
  const bool finite = fabs(a00) < big && fabs(a01) < big && fabs(a02) < big && fabs(a11) < big && fabs(a12) < big && fabs(a22) < big;
  if (finite && a[0] != 0) {
    double v00, v01, v02, v10, v11, v12, v20, v21, v22;
    jacobi3_sweeps(a00, a01, a02, a11, a12, a22, v00, v01, v02, v10, v11, v12, v20, v21, v22);
    // column of the largest eigenvalue (highest index on a tie: numpy.linalg.eigh's last column), and the middle eigenvalue
    const int hi = a22 >= a11 ? (a22 >= a00 ? 2 : 0) : (a11 >= a00 ? 1 : 0);
    const double l2 = hi == 0 ? a00 : (hi == 1 ? a11 : a22);
    const double e1 = hi == 0 ? a11 : a00, e2 = hi == 2 ? a11 : a22;              // the other two
    const double l1 = e1 >= e2 ? e1 : e2;
    double ux = hi == 0 ? v00 : (hi == 1 ? v01 : v02), uy = hi == 0 ? v10 : (hi == 1 ? v11 : v12), uz = hi == 0 ? v20 : (hi == 1 ? v21 : v22);
    const double len = sqrt((ux * ux + uy * uy) + uz * uz);
    if (len > 0.5 && len < 2.0) {
      ux = ux / len; uy = uy / len; uz = uz / len;
      const double ax = fabs(ux), ay = fabs(uy), az = fabs(uz);
      const double top = ax >= ay ? (ax >= az ? ux : uz) : (ay >= az ? uy : uz);
      const double sg = top < 0.0 ? -1.0 : 1.0;
      dx = sg * ux; dy = sg * uy; dz = sg * uz;
      c = l2 - l1;
    }
  }
  dir[3 * (size_t)i] = dx; dir[3 * (size_t)i + 1] = dy; dir[3 * (size_t)i + 2] = dz;
  conf[i] = c;
}

enum { STOP_STEPS = 0, STOP_BOUNDS = 1, STOP_TURN = 2, STOP_GAP = 3 };

__global__ __launch_bounds__(TRACE_BLOCK) void strand_trace_kernel(int S, const double* __restrict__ roots, const double* __restrict__ p0,
                                                                   const double* __restrict__ dir, const double* __restrict__ conf,
                                                                   double ox, double oy, double oz, double k, int nx, int ny, int nz,
                                                                   double step, int max_steps, double cos_max, double min_conf,
                                                                   int max_gap, double* __restrict__ joints, int* __restrict__ count,
                                                                   int* __restrict__ reason) {
  const int s = blockIdx.x * TRACE_BLOCK + threadIdx.x;
  if (s >= S) return;
  double x = roots[3 * (size_t)s], y = roots[3 * (size_t)s + 1], z = roots[3 * (size_t)s + 2];
  double px = p0[3 * (size_t)s], py = p0[3 * (size_t)s + 1], pz = p0[3 * (size_t)s + 2];
  double* __restrict__ J = joints + 3 * (size_t)s * (size_t)(max_steps + 1);
  J[0] = x; J[1] = y; J[2] = z;
  const double tx_top = (double)(nx - 1), ty_top = (double)(ny - 1), tz_top = (double)(nz - 1);
  const size_t sy = (size_t)nx, sz = (size_t)nx * ny;
  int gap = 0, n = 1, last = 0, why = STOP_STEPS;
  bool entered = false;
  for (int it = 0; it < max_steps; it++) {
    const double tx = (x - ox) * k, ty = (y - oy) * k, tz = (z - oz) * k;
    // (finite and 0 <= t < n - 1: a NaN fails every comparison, +inf the second)
    if (!(tx >= 0.0 && tx < tx_top && ty >= 0.0 && ty < ty_top && tz >= 0.0 && tz < tz_top)) { why = STOP_BOUNDS; break; }
    const double flx = floor(tx), fly = floor(ty), flz = floor(tz);
    const int ix = (int)flx, iy = (int)fly, iz = (int)flz;                        // 0 <= i <= n - 2
    const double fx = tx - flx, fy = ty - fly, fz = tz - flz;
    const double gx0 = 1.0 - fx, gy0 = 1.0 - fy, gz0 = 1.0 - fz;
    const size_t base = ((size_t)iz * ny + iy) * nx + ix;
    double w = 0.0, v0 = 0.0, v1 = 0.0, v2 = 0.0;
#pragma unroll
    for (int c = 0; c < 8; c++) {                                                 // z outermost, then y, then x, each 0 then 1
      const int cx = c & 1, cy = (c >> 1) & 1, cz = c >> 2;
      const size_t at = base + (cz ? sz : 0) + (cy ? sy : 0) + (size_t)cx;
      const double tw = ((cx ? fx : gx0) * (cy ? fy : gy0)) * (cz ? fz : gz0);
      double a = tw * conf[at];
      w = w + a;
      const double e0 = dir[3 * at], e1 = dir[3 * at + 1], e2 = dir[3 * at + 2];
      if (dot3(e0, e1, e2, px, py, pz) < 0.0) a = -a;
      v0 = v0 + a * e0; v1 = v1 + a * e1; v2 = v2 + a * e2;
    }
    const double nn = dot3(v0, v1, v2, v0, v1, v2);
    double d0, d1, d2;
    if (w >= min_conf && nn > 0.0 && nn < __builtin_inf()) {
      const double len = sqrt(nn);
      d0 = v0 / len; d1 = v1 / len; d2 = v2 / len;
      if (entered && dot3(d0, d1, d2, px, py, pz) < cos_max) { why = STOP_TURN; break; }
      entered = true;
      gap = 0;
    } else {
      gap = gap + 1;
      if (gap > max_gap) { why = STOP_GAP; break; }
      d0 = px; d1 = py; d2 = pz;
    }
    x = x + step * d0; y = y + step * d1; z = z + step * d2;
    px = d0; py = d1; pz = d2;
    J[3 * n] = x; J[3 * n + 1] = y; J[3 * n + 2] = z;
    n = n + 1;
    if (gap == 0) last = n - 1;
  }
  count[s] = last + 1;
  reason[s] = why;
}

int grid_check(const char* who, int nx, int ny, int nz, double ox, double oy, double oz, double h) {
  if (nx < 2 || ny < 2 || nz < 2 || nx > 1024 || ny > 1024 || nz > 1024 || (long long)nx * ny * nz > HGS_TRACE_MAX_NODES) {
    hgs_set_error("%s: a grid of %d x %d x %d nodes (2 to 1024 an axis, at most 2^26 in all)", who, nx, ny, nz);
    return 1;
  }
  if (!(h > 0.0) || !isfinite(h) || !isfinite(ox) || !isfinite(oy) || !isfinite(oz) || !isfinite(1.0 / h) || !(1.0 / h > 0.0)) {
    hgs_set_error("%s: origin (%g, %g, %g) and spacing %g must be finite, the spacing and 1/spacing > 0", who, ox, oy, oz, h);
    return 1;
  }
  return 0;
}

}  // namespace

extern "C" int hgs_field_splat(void* stream, int N, const double* points, const double* dirs, double ox, double oy, double oz, double h,
                               int nx, int ny, int nz, double r2, long long* acc, int* skipped) {
  if (N < 0 || N > HGS_TRACE_MAX_POINTS) { hgs_set_error("hgs_field_splat: %d points (0 to 2^24)", N); return 1; }
  if (grid_check("hgs_field_splat", nx, ny, nz, ox, oy, oz, h)) return 1;
  if (!(r2 > 0.0) || !isfinite(r2) || !(sqrt(r2) / h <= HGS_TRACE_MAX_REACH)) {
    hgs_set_error("hgs_field_splat: r2 = %g with spacing %g (finite and > 0, the radius at most %g spacings)", r2, h, HGS_TRACE_MAX_REACH);
    return 1;
  }
  if (!acc || !skipped) { hgs_set_error("hgs_field_splat: acc and skipped are required"); return 1; }
  if (N == 0) return 0;
  if (!points || !dirs) { hgs_set_error("hgs_field_splat: points and dirs are required"); return 1; }
  // the box: nodes floor(t - reach) .. + span - 1 per axis hold every node with |index - t| < r/h, with 1/64 of a spacing to spare for
  // the roundings of t and of the node positions
  const double reach = sqrt(r2) / h + 0.015625;
  const int span = (int)floor(2.0 * reach) + 2;
  hipLaunchKernelGGL(field_splat_kernel, dim3((N + TRACE_BLOCK - 1) / TRACE_BLOCK), dim3(TRACE_BLOCK), 0, (hipStream_t)stream, N, points,
                     dirs, ox, oy, oz, h, 1.0 / h, nx, ny, nz, r2, reach, span, acc, skipped);
  HGS_CHECK_LAUNCH();
  return 0;
}

extern "C" int hgs_field_solve(void* stream, int nx, int ny, int nz, const long long* acc, double* dir, double* conf) {
  if (nx < 2 || ny < 2 || nz < 2 || nx > 1024 || ny > 1024 || nz > 1024 || (long long)nx * ny * nz > HGS_TRACE_MAX_NODES) {
    hgs_set_error("hgs_field_solve: a grid of %d x %d x %d nodes (2 to 1024 an axis, at most 2^26 in all)", nx, ny, nz);
    return 1;
  }
  if (!acc || !dir || !conf) { hgs_set_error("hgs_field_solve: acc, dir and conf are required"); return 1; }
  const long long nodes = (long long)nx * ny * nz;
  hipLaunchKernelGGL(field_solve_kernel, dim3((unsigned)((nodes + TRACE_BLOCK - 1) / TRACE_BLOCK)), dim3(TRACE_BLOCK), 0,
                     (hipStream_t)stream, nodes, acc, dir, conf);
  HGS_CHECK_LAUNCH();
  return 0;
}

extern "C" int hgs_strand_trace(void* stream, int S, const double* roots, const double* p0, const double* dir, const double* conf,
                                double ox, double oy, double oz, double h, int nx, int ny, int nz, double step, int max_steps,
                                double cos_max, double min_conf, int max_gap, double* joints, int* count, int* reason) {
  if (S < 0 || S > (1 << 24)) { hgs_set_error("hgs_strand_trace: %d roots (0 to 2^24)", S); return 1; }
  if (grid_check("hgs_strand_trace", nx, ny, nz, ox, oy, oz, h)) return 1;
  if (max_steps < 1 || max_steps > HGS_TRACE_MAX_STEPS) {
    hgs_set_error("hgs_strand_trace: max_steps = %d (1 to %d)", max_steps, HGS_TRACE_MAX_STEPS); return 1;
  }
  if (!(step > 0.0) || !isfinite(step) || !isfinite(cos_max) || cos_max < -1.0 || cos_max > 1.0 || !isfinite(min_conf) || max_gap < 0) {
    hgs_set_error("hgs_strand_trace: step = %g (finite and > 0), cos_max = %g (-1 to 1), min_conf = %g (finite), max_gap = %d (>= 0)", step,
                  cos_max, min_conf, max_gap);
    return 1;
  }
  if (!dir || !conf) { hgs_set_error("hgs_strand_trace: dir and conf are required"); return 1; }
  if (S == 0) return 0;
  if (!roots || !p0 || !joints || !count || !reason) {
    hgs_set_error("hgs_strand_trace: roots, p0, joints, count and reason are required"); return 1;
  }
  hipLaunchKernelGGL(strand_trace_kernel, dim3((S + TRACE_BLOCK - 1) / TRACE_BLOCK), dim3(TRACE_BLOCK), 0, (hipStream_t)stream, S, roots, p0,
                     dir, conf, ox, oy, oz, 1.0 / h, nx, ny, nz, step, max_steps, cos_max, min_conf, max_gap, joints, count, reason);
  HGS_CHECK_LAUNCH();
  return 0;
}
