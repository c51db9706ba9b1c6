// hgs_visibility.hip -- which views can see a point of the carved hull (utils/visibility.py states the contract, init_cloud.py
// --directions --visibility is the scene driver): hgs_hull_visibility.  gfx950, wave64.
//
// The contract (one definition for the numpy path, this kernel and the tests' loop restatement).  occ[nz][ny][nx] is the carve's
// grid: voxel i spans origin + i*h .. origin + (i + 1)*h per axis.  For the point p and the camera centre C of view k, all float64,
// one rounding per operation in the order written (this file is built with -ffp-contract=off):
//   t_a = (p_a - origin_a)/h;  the start is inside iff 0 <= t_a < n_a on every axis (a NaN fails; the test precedes the conversion);
//   a point that does not start inside has every bit below V set.  Otherwise i0_a = (int)floor(t_a), D = C - p and per axis
//     D_a > 0:  step = +1, tmax = ((origin_a + (i0_a + 1)*h) - p_a)/D_a, td = h/D_a
//     D_a < 0:  step = -1, tmax = ((origin_a + i0_a*h) - p_a)/D_a,       td = h/(-D_a)
//     D_a == 0: step = 0,  tmax = +inf
//   walk from i = i0, blocked = 0:  a = the axis of the smallest tmax (strict <: the lowest axis wins a tie);  VISIBLE unless
//   tmax_a < 1.0;  i_a += step_a, VISIBLE if i_a has left the grid;  tmax_a = tmax_a + td_a;  if max_a |i_a - i0_a| > skip and
//   occ[i] != 0: blocked += 1, BLOCKED if blocked > max_blocked;  at most nx + ny + nz steps (the indices move monotonically and stay
//   inside the grid between steps: the cap cannot be reached), then VISIBLE.
//   visible[i][k / 32] bit k % 32 = view k is not blocked; the bits at and above V are 0.
//
// Work split.  One lane per (point, word): 256 points a workgroup in x, blockIdx.y the word.  The lane computes its start voxel once,
// walks the word's up to 32 rays one after the other with the word in a register, and writes one 4-byte store.  The view index
// depends on blockIdx.y and the loop counter alone (wavefront-uniform: the centre arrives by scalar loads, as the view records do in
// hgs_carve.hip and hgs_lift.hip).  occ is the carve's own uint8 buffer; every load of it follows the range test of its index.  No
// atomics, no LDS.
#include "hgs_common.h"

#define HGS_VIS_MAX_DIM 1024
#define HGS_VIS_MAX_VIEWS 4096
#define HGS_VIS_MAX_SKIP 1024
#define HGS_VIS_MAX_BLOCKED 3072

namespace {

struct VisGrid { double ox, oy, oz, h; int nx, ny, nz, skip, max_blocked; };

// one axis of the ray setup
__device__ __forceinline__ void vis_axis(double o, double h, int i0, double p, double D, int& step, double& tmax, double& td) {
  step = 0; tmax = __builtin_inf(); td = 0.0;
  if (D > 0.0) { step = 1; tmax = ((o + (double)(i0 + 1) * h) - p) / D; td = h / D; }
  else if (D < 0.0) { step = -1; tmax = ((o + (double)i0 * h) - p) / D; td = h / (-D); }
}

__device__ __forceinline__ bool vis_ray(const VisGrid& g, const unsigned char* __restrict__ occ, double px, double py, double pz, int i0x,
                                        int i0y, int i0z, double cx, double cy, double cz) {
  int sx, sy, sz;
  double tmx, tmy, tmz, tdx, tdy, tdz;
  vis_axis(g.ox, g.h, i0x, px, cx - px, sx, tmx, tdx);
  vis_axis(g.oy, g.h, i0y, py, cy - py, sy, tmy, tdy);
  vis_axis(g.oz, g.h, i0z, pz, cz - pz, sz, tmz, tdz);
  int ix = i0x, iy = i0y, iz = i0z, blocked = 0;
  const int cap = g.nx + g.ny + g.nz;
  for (int s = 0; s < cap; s++) {
    int a = 0;
    double ta = tmx;
    if (tmy < ta) { a = 1; ta = tmy; }
    if (tmz < ta) { a = 2; ta = tmz; }
    if (!(ta < 1.0)) return true;
    if (a == 0) { ix += sx; if (ix < 0 || ix >= g.nx) return true; tmx = tmx + tdx; }
    else if (a == 1) { iy += sy; if (iy < 0 || iy >= g.ny) return true; tmy = tmy + tdy; }
    else { iz += sz; if (iz < 0 || iz >= g.nz) return true; tmz = tmz + tdz; }
    const int dx = abs(ix - i0x), dy = abs(iy - i0y), dz = abs(iz - i0z);
    const int cheb = dx > dy ? (dx > dz ? dx : dz) : (dy > dz ? dy : dz);
    if (cheb > g.skip && occ[((size_t)iz * g.ny + iy) * g.nx + ix] != 0) {
      blocked++;
      if (blocked > g.max_blocked) return false;
    }
  }
  return true;
}

__global__ __launch_bounds__(256) void hull_visibility_kernel(long long N, const double* __restrict__ points, int V,
                                                              const double* __restrict__ centres, const unsigned char* __restrict__ occ,
                                                              VisGrid g, int words, int* __restrict__ visible) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const int word = blockIdx.y, k0 = word * 32;
  const int kn = V - k0 < 32 ? V - k0 : 32;                      // (1 to 32: the host launches ceil(V/32) words)
  const double px = points[3 * (size_t)i], py = points[3 * (size_t)i + 1], pz = points[3 * (size_t)i + 2];
  const double tx = (px - g.ox) / g.h, ty = (py - g.oy) / g.h, tz = (pz - g.oz) / g.h;
  unsigned bits = kn == 32 ? 0xFFFFFFFFu : ((1u << kn) - 1u);
  if (tx >= 0.0 && tx < (double)g.nx && ty >= 0.0 && ty < (double)g.ny && tz >= 0.0 && tz < (double)g.nz) {
    const int i0x = (int)floor(tx), i0y = (int)floor(ty), i0z = (int)floor(tz);
    bits = 0u;
    for (int b = 0; b < kn; b++) {
      const double* __restrict__ c = centres + 3 * (size_t)(k0 + b);
      if (vis_ray(g, occ, px, py, pz, i0x, i0y, i0z, c[0], c[1], c[2])) bits |= 1u << b;
    }
  }
  visible[(size_t)i * words + word] = (int)bits;
}

}  // namespace

extern "C" int hgs_hull_visibility(void* stream, long long N, const double* points, int V, const double* centres_dev,
                                   const unsigned char* occ, const double* origin_host, double h, int nx, int ny, int nz, int skip,
                                   int max_blocked, int* visible) {
  const double big = __builtin_inf();
  if (N < 0 || N > 0x7FFFFFFFll * 256) { hgs_set_error("hgs_hull_visibility: N = %lld points", N); return 1; }
  if (V < 1 || V > HGS_VIS_MAX_VIEWS) { hgs_set_error("hgs_hull_visibility: V = %d views (1 to %d)", V, HGS_VIS_MAX_VIEWS); return 1; }
  if (nx < 1 || ny < 1 || nz < 1 || nx > HGS_VIS_MAX_DIM || ny > HGS_VIS_MAX_DIM || nz > HGS_VIS_MAX_DIM) {
    hgs_set_error("hgs_hull_visibility: a grid of %d x %d x %d voxels (1 to %d per axis)", nx, ny, nz, HGS_VIS_MAX_DIM); return 1;
  }
  if (skip < 0 || skip > HGS_VIS_MAX_SKIP || max_blocked < 0 || max_blocked > HGS_VIS_MAX_BLOCKED) {
    hgs_set_error("hgs_hull_visibility: skip = %d (0 to %d), max_blocked = %d (0 to %d)", skip, HGS_VIS_MAX_SKIP, max_blocked,
                  HGS_VIS_MAX_BLOCKED);
    return 1;
  }
  if (!(h > 0.0 && h < big && 1.0 / h > 0.0 && 1.0 / h < big)) {
    hgs_set_error("hgs_hull_visibility: voxel size h = %g (h and 1/h finite and positive)", h); return 1;
  }
  if (!origin_host) { hgs_set_error("hgs_hull_visibility: null argument"); return 1; }
  if (!(fabs(origin_host[0]) < big && fabs(origin_host[1]) < big && fabs(origin_host[2]) < big)) {
    hgs_set_error("hgs_hull_visibility: the origin is not finite"); return 1;
  }
  if (N == 0) return 0;
  if (!points || !centres_dev || !occ || !visible) { hgs_set_error("hgs_hull_visibility: null argument"); return 1; }
  const int words = (V + 31) / 32;
  const VisGrid g = {origin_host[0], origin_host[1], origin_host[2], h, nx, ny, nz, skip, max_blocked};
  const dim3 grid((unsigned)((N + 255) / 256), (unsigned)words), block(256);
  hipLaunchKernelGGL(hull_visibility_kernel, grid, block, 0, (hipStream_t)stream, N, points, V, centres_dev, occ, g, words, visible);
  HGS_CHECK_LAUNCH();
  return 0;
}
