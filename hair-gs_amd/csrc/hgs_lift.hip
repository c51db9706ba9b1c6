// hgs_lift.hip -- 3-D hair directions lifted from a capture's 2-D orientation maps (utils/lift.py states the contract, init_cloud.py
// --directions is the scene driver): hgs_lift_moments, hgs_lift_moments_gated, hgs_lift_solve.  gfx950, wave64.
//
// The contract (one definition for the numpy path, these kernels and the tests' loop restatement).  A view k is a pinhole camera
// with three uint8 planes [H][W] at the record's mask_offset of three buffers: mask, orient and conf.  TAB[256][2] =
// (sin, cos)(o*pi/255), float64, built on the host: no transcendental is evaluated here.  Term of the point (x, y, z) in view k, all
// float64, one rounding per operation in the order written (this file is built with -ffp-contract=off):
//   xc, yc, zc, u, v, seen, px, py as in hgs_pinhole.h
//   used iff seen and mask[py][px] != 0 and conf[py][px] >= min_conf
//     (hgs_lift_moments_gated: and bit k % 32 of visible[i][k / 32] is set -- utils/visibility.py's words)
//   lu = TAB[orient[py][px]][0], lv = TAB[..][1];  a = lu/fx, b = lv/fy
//   ncx = -(zc*b), ncy = zc*a, ncz = xc*b - yc*a;  n_i = (R0i*ncx + R1i*ncy) + R2i*ncz;  nn = (n0*n0 + n1*n1) + n2*n2
//   not used unless nn > 0 and nn is finite
//   w = conf[py][px]/255.0;  with prev p != (0, 0, 0):  r2 = ((n0*p0 + n1*p1) + n2*p2)^2 / nn,  w = w*(s2/(s2 + r2))
//   g = w/nn;  M += g*(n0n0, n0n1, n0n2, n1n1, n1n2, n2n2) (product, times g, added);  wsum += w;  count += 1
// over the views in index order.  Solve: the eigenvalues l0 <= l1 <= l2 of M; d = the unit eigenvector of l0, its component of largest
// magnitude positive (lowest index on a tie); coherence = (l1 - l0)/(l1 + l0), 0 where the denominator is not > 0; d = 0 and
// coherence = 0 where count < min_views, l1 <= 0 or an entry of M is not finite.
//
// Work split.  One lane per point in both kernels.  hgs_lift_moments runs the view loop inside the lane, so a point's sums have the
// contract's order whatever the launch looks like: bitwise repeatable, and equal to the numpy path.  The view record is indexed by
// the loop counter alone (wavefront-uniform: scalar loads); TAB is indexed by the sampled byte, which differs from lane to lane, so
// the workgroup copies its 4 KiB into LDS once.  hgs_lift_solve is cyclic Jacobi on the 3 x 3 matrix in registers (hgs_jacobi3.h,
// shared with csrc/hgs_normals.hip).  No atomics.
#include "hgs_common.h"
#include "hgs_jacobi3.h"
#include "hgs_pinhole.h"

#define HGS_LIFT_MAX_VIEWS 4096

namespace {

// GATED: a view is used only where its bit of the point's visibility words is set (hgs_hull_visibility's layout); the word of the
// current 32 views is kept in a register, and a view whose bit is clear is left before its projection.  One body for both entry
// points: the sums of the two instances have the same order.
template <bool GATED>
__global__ __launch_bounds__(256) void lift_moments_kernel(long long N, const double* __restrict__ points, int V,
                                                           const HgsCarveView* __restrict__ views, const unsigned char* __restrict__ masks,
                                                           const unsigned char* __restrict__ orients, const unsigned char* __restrict__ confs,
                                                           const double* __restrict__ tab, const double* __restrict__ prev, double s2,
                                                           int min_conf, const int* __restrict__ visible, int words,
                                                           double* __restrict__ M, double* __restrict__ wsum_out,
                                                           int* __restrict__ count_out) {
  __shared__ double stab[512];
  stab[threadIdx.x] = tab[threadIdx.x];
  stab[256 + threadIdx.x] = tab[256 + threadIdx.x];
  __syncthreads();
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const double x = points[3 * (size_t)i], y = points[3 * (size_t)i + 1], z = points[3 * (size_t)i + 2];
  double p0 = 0.0, p1 = 0.0, p2 = 0.0;
  if (prev) { p0 = prev[3 * (size_t)i]; p1 = prev[3 * (size_t)i + 1]; p2 = prev[3 * (size_t)i + 2]; }
  const bool robust = prev && !(p0 == 0.0 && p1 == 0.0 && p2 == 0.0);
  double m00 = 0.0, m01 = 0.0, m02 = 0.0, m11 = 0.0, m12 = 0.0, m22 = 0.0, wsum = 0.0;
  int count = 0;
  unsigned gate = 0u;
  for (int k = 0; k < V; k++) {
    if (GATED) {
      if ((k & 31) == 0) gate = (unsigned)visible[(size_t)i * words + (k >> 5)];
      if (!((gate >> (k & 31)) & 1u)) continue;
    }
    const HgsCarveView& c = views[k];
    const Pinhole q = pinhole_project(c, x, y, z);
    if (!pinhole_seen(&c, q)) continue;
    const size_t at = (size_t)c.mask_offset + pinhole_pixel(c, q);
    if (masks[at] == 0) continue;
    const int cf = confs[at];
    if (cf < min_conf) continue;
    const int o = orients[at];
    const double a = stab[2 * o] / c.fx, b = stab[2 * o + 1] / c.fy;
    const double ncx = -(q.zc * b), ncy = q.zc * a, ncz = q.xc * b - q.yc * a;
    const double n0 = (c.R[0] * ncx + c.R[3] * ncy) + c.R[6] * ncz;
    const double n1 = (c.R[1] * ncx + c.R[4] * ncy) + c.R[7] * ncz;
    const double n2 = (c.R[2] * ncx + c.R[5] * ncy) + c.R[8] * ncz;
    const double nn = (n0 * n0 + n1 * n1) + n2 * n2;
    if (!(nn > 0.0 && nn < __builtin_inf())) continue;
    double w = (double)cf / 255.0;
    if (robust) {
      const double dot = (n0 * p0 + n1 * p1) + n2 * p2;
      const double r2 = (dot * dot) / nn;
      w = w * (s2 / (s2 + r2));
    }
    const double g = w / nn;
    m00 = m00 + g * (n0 * n0); m01 = m01 + g * (n0 * n1); m02 = m02 + g * (n0 * n2);
    m11 = m11 + g * (n1 * n1); m12 = m12 + g * (n1 * n2); m22 = m22 + g * (n2 * n2);
    wsum = wsum + w;
    count++;
  }
  double* __restrict__ m = M + 6 * (size_t)i;
  m[0] = m00; m[1] = m01; m[2] = m02; m[3] = m11; m[4] = m12; m[5] = m22;
  wsum_out[i] = wsum;
  count_out[i] = count;
}

__global__ __launch_bounds__(256) void lift_solve_kernel(long long N, const double* __restrict__ M, const int* __restrict__ count,
                                                         int min_views, double* __restrict__ d, double* __restrict__ coherence) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const double* __restrict__ m = M + 6 * (size_t)i;
  double a00 = m[0], a01 = m[1], a02 = m[2], a11 = m[3], a12 = m[4], a22 = m[5];
  double dx = 0.0, dy = 0.0, dz = 0.0, coh = 0.0;
  const double big = __builtin_inf();
  const bool finite = fabs(a00) < big && fabs(a01) < big && fabs(a02) < big && fabs(a11) < big && fabs(a12) < big && fabs(a22) < big;
  if (finite && count[i] >= min_views) {
    double v00, v01, v02, v10, v11, v12, v20, v21, v22;
    jacobi3_sweeps(a00, a01, a02, a11, a12, a22, v00, v01, v02, v10, v11, v12, v20, v21, v22);
    // column of the smallest eigenvalue (lowest index on a tie), and the middle eigenvalue
    const int lo = a00 <= a11 ? (a22 < a00 ? 2 : 0) : (a22 < a11 ? 2 : 1);
    const double l0 = lo == 0 ? a00 : (lo == 1 ? a11 : a22);
    const double e1 = lo == 0 ? a11 : a00, e2 = lo == 2 ? a11 : a22;          // the other two
    const double l1 = e1 <= e2 ? e1 : e2;
    double nx = lo == 0 ? v00 : (lo == 1 ? v01 : v02), ny = lo == 0 ? v10 : (lo == 1 ? v11 : v12), nz = lo == 0 ? v20 : (lo == 1 ? v21 : v22);
    const double len = sqrt((nx * nx + ny * ny) + nz * nz);
    if (l1 > 0.0 && len > 0.5 && len < 2.0) {
      nx = nx / len; ny = ny / len; nz = nz / len;
      const double ax = fabs(nx), ay = fabs(ny), az = fabs(nz);
      const double top = ax >= ay ? (ax >= az ? nx : nz) : (ay >= az ? ny : nz);
      const double sg = top < 0.0 ? -1.0 : 1.0;
      dx = sg * nx; dy = sg * ny; dz = sg * nz;
      const double den = l1 + l0;
      coh = den > 0.0 ? (l1 - l0) / den : 0.0;
    }
  }
  d[3 * (size_t)i] = dx; d[3 * (size_t)i + 1] = dy; d[3 * (size_t)i + 2] = dz;
  coherence[i] = coh;
}

}  // namespace

// the checks and the launch of both entry points: `who` names the one that was called, `gated` says that it takes the words
static int lift_moments_launch(const char* who, void* stream, long long N, const double* points, int V, const HgsCarveView* views_dev,
                               const unsigned char* masks, const unsigned char* orients, const unsigned char* confs, const double* tab_dev,
                               const double* prev, double s2, int min_conf, bool gated, const int* visible, int words, double* M,
                               double* wsum, int* count) {
  if (N < 0 || N > 0x7FFFFFFFll * 256) { hgs_set_error("%s: N = %lld points", who, N); return 1; }
  if (V < 1 || V > HGS_LIFT_MAX_VIEWS) { hgs_set_error("%s: V = %d views (1 to %d)", who, V, HGS_LIFT_MAX_VIEWS); return 1; }
  if (min_conf < 0 || min_conf > 255) { hgs_set_error("%s: min_conf = %d (0 to 255)", who, min_conf); return 1; }
  if (prev && !(s2 > 0.0 && s2 < __builtin_inf())) {
    hgs_set_error("%s: s2 = %g with a previous direction (finite and positive)", who, s2); return 1;
  }
  if (gated && words != (V + 31) / 32) { hgs_set_error("%s: words = %d, %d views take %d", who, words, V, (V + 31) / 32); return 1; }
  if (N == 0) return 0;
  if (!points || !views_dev || !masks || !orients || !confs || !tab_dev || !M || !wsum || !count || (gated && !visible)) {
    hgs_set_error("%s: null argument", who); return 1;
  }
  const dim3 grid((unsigned)((N + 255) / 256)), block(256);
  if (gated)
    hipLaunchKernelGGL(lift_moments_kernel<true>, grid, block, 0, (hipStream_t)stream, N, points, V, views_dev, masks, orients, confs,
                       tab_dev, prev, s2, min_conf, visible, words, M, wsum, count);
  else
    hipLaunchKernelGGL(lift_moments_kernel<false>, grid, block, 0, (hipStream_t)stream, N, points, V, views_dev, masks, orients, confs,
                       tab_dev, prev, s2, min_conf, (const int*)nullptr, 0, M, wsum, count);
  HGS_CHECK_LAUNCH();
  return 0;
}

extern "C" int hgs_lift_moments(void* stream, long long N, const double* points, int V, const HgsCarveView* views_dev,
                                const unsigned char* masks, const unsigned char* orients, const unsigned char* confs, const double* tab_dev,
                                const double* prev, double s2, int min_conf, double* M, double* wsum, int* count) {
  return lift_moments_launch("hgs_lift_moments", stream, N, points, V, views_dev, masks, orients, confs, tab_dev, prev, s2, min_conf, false,
                             nullptr, 0, M, wsum, count);
}

extern "C" int hgs_lift_moments_gated(void* stream, long long N, const double* points, int V, const HgsCarveView* views_dev,
                                      const unsigned char* masks, const unsigned char* orients, const unsigned char* confs,
                                      const double* tab_dev, const double* prev, double s2, int min_conf, const int* visible, int words,
                                      double* M, double* wsum, int* count) {
  return lift_moments_launch("hgs_lift_moments_gated", stream, N, points, V, views_dev, masks, orients, confs, tab_dev, prev, s2, min_conf,
                             true, visible, words, M, wsum, count);
}

extern "C" int hgs_lift_solve(void* stream, long long N, const double* M, const int* count, int min_views, double* d,
                              double* coherence) {
  if (N < 0 || N > 0x7FFFFFFFll * 256) { hgs_set_error("hgs_lift_solve: N = %lld points", N); return 1; }
  if (min_views < 2) { hgs_set_error("hgs_lift_solve: min_views = %d (>= 2)", min_views); return 1; }
  if (N == 0) return 0;
  if (!M || !count || !d || !coherence) { hgs_set_error("hgs_lift_solve: null argument"); return 1; }
  const dim3 grid((unsigned)((N + 255) / 256)), block(256);
  hipLaunchKernelGGL(lift_solve_kernel, grid, block, 0, (hipStream_t)stream, N, M, count, min_views, d, coherence);
  HGS_CHECK_LAUNCH();
  return 0;
}
