// hgs_carve.hip -- a point cloud carved from a capture's hair masks (utils/carve.py states the contract, init_cloud.py is the scene
// driver): hgs_carve_votes, hgs_carve_grid, hgs_carve_shell.  gfx950, wave64.
//
// The contract (one definition for the numpy path, these kernels and the tests' loop restatement).  A view k is a pinhole camera with
// a uint8 mask [H][W].  Vote of the point (x, y, z) in view k (this file is built with -ffp-contract=off):
//   xc, yc, zc, u, v, seen, px, py as in hgs_pinhole.h
//   hit  iff seen and mask[py][px] != 0
// seen[i], hits[i] are the counts over the views, rgb_sum[i][c] the sum of image[py][px][c] over the views that hit: integer sums,
// exact and independent of order.  Keep rule, integers min_views >= 1 and 0 <= min_percent <= 100:
//   kept iff seen >= min_views and 100*hits >= min_percent*seen
// Grid: occ[z][y][x] = kept(origin + (i + 0.5)*h per axis).  Shell: occ and a face neighbour that is 0 or outside the grid.
//
// Work split.  One lane per voxel (or point), x fastest: a wavefront is 64 consecutive x of one row, a workgroup a 64 x 4 brick of
// one z slice, so what a brick touches of a mask is a small patch of it.  The view loop runs inside the lane; the view record is
// indexed by the loop counter alone (wavefront-uniform: scalar loads).  hgs_carve_grid leaves a voxel's loop as soon as the rule is
// decided either way -- with s seen, t hits and r views left: seen can no longer reach min_views; 100*(s - t) > (100 - min_percent)*
// (s + r), the misses can never be outvoted; or s >= min_views and 100*t >= min_percent*(s + r), the hits can never be.  Each is a
// bound on the final integers, so occ is what the full counts give (tests/test_carve_gpu.py holds it to hgs_carve_votes' counts).
// hgs_carve_votes has no early exit: its counts are the contract.  No atomics, no LDS.
#include "hgs_common.h"
#include "hgs_pinhole.h"

#define HGS_CARVE_BX 64
#define HGS_CARVE_BY 4
#define HGS_CARVE_MAX_DIM 1024
#define HGS_CARVE_MAX_VIEWS 4096

namespace {

__global__ __launch_bounds__(256) void carve_votes_kernel(long long N, const double* __restrict__ points, int V,
                                                          const HgsCarveView* __restrict__ views, const unsigned char* __restrict__ masks,
                                                          const unsigned char* __restrict__ images, int* __restrict__ seen_out,
                                                          int* __restrict__ hits_out, int* __restrict__ rgb_sum) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const double x = points[3 * (size_t)i], y = points[3 * (size_t)i + 1], z = points[3 * (size_t)i + 2];
  int seen = 0, hits = 0, r = 0, g = 0, b = 0;
  for (int k = 0; k < V; k++) {
    const HgsCarveView& c = views[k];
    const Pinhole q = pinhole_project(c, x, y, z);
    if (!pinhole_seen(&c, q)) continue;
    seen++;
    const size_t pixel = pinhole_pixel(c, q);
    if (masks[(size_t)c.mask_offset + pixel] == 0) continue;
    hits++;
    if (images && c.image_offset >= 0) {
      const unsigned char* __restrict__ p = images + (size_t)c.image_offset + 3 * pixel;
      r += p[0]; g += p[1]; b += p[2];
    }
  }
  seen_out[i] = seen;
  hits_out[i] = hits;
  if (rgb_sum) { rgb_sum[3 * (size_t)i] = r; rgb_sum[3 * (size_t)i + 1] = g; rgb_sum[3 * (size_t)i + 2] = b; }
}

__global__ __launch_bounds__(HGS_CARVE_BX * HGS_CARVE_BY) void carve_grid_kernel(double ox, double oy, double oz, double h, int nx,
                                                                                 int ny, int nz, int V,
                                                                                 const HgsCarveView* __restrict__ views,
                                                                                 const unsigned char* __restrict__ masks, int min_views,
                                                                                 int min_percent, unsigned char* __restrict__ occ) {
  const int ix = blockIdx.x * HGS_CARVE_BX + threadIdx.x, iy = blockIdx.y * HGS_CARVE_BY + threadIdx.y, iz = blockIdx.z;
  if (ix >= nx || iy >= ny || iz >= nz) return;
  const double x = ox + ((double)ix + 0.5) * h, y = oy + ((double)iy + 0.5) * h, z = oz + ((double)iz + 0.5) * h;
  const int slack = 100 - min_percent;
  int seen = 0, hits = 0;
  bool decided = false, kept = false;
  for (int k = 0; k < V; k++) {
    const HgsCarveView& c = views[k];
    const Pinhole q = pinhole_project(c, x, y, z);
    if (pinhole_seen(&c, q)) {
      seen++;
      if (masks[(size_t)c.mask_offset + pinhole_pixel(c, q)] != 0) hits++;
    }
    const int left = V - 1 - k, most = seen + left;                 // most: the largest `seen` the voxel can still end with
    if (most < min_views || 100 * (seen - hits) > slack * most) { decided = true; kept = false; break; }
    if (seen >= min_views && 100 * hits >= min_percent * most) { decided = true; kept = true; break; }
  }
  if (!decided) kept = seen >= min_views && 100 * hits >= min_percent * seen;   // (V == 0 cannot happen: the host refuses it)
  occ[((size_t)iz * ny + iy) * nx + ix] = kept ? 1 : 0;
}

__global__ __launch_bounds__(HGS_CARVE_BX * HGS_CARVE_BY) void carve_shell_kernel(int nx, int ny, int nz,
                                                                                  const unsigned char* __restrict__ occ,
                                                                                  unsigned char* __restrict__ out) {
  const int ix = blockIdx.x * HGS_CARVE_BX + threadIdx.x, iy = blockIdx.y * HGS_CARVE_BY + threadIdx.y, iz = blockIdx.z;
  if (ix >= nx || iy >= ny || iz >= nz) return;
  const size_t sy = (size_t)nx, sz = (size_t)nx * ny, i = (size_t)iz * sz + (size_t)iy * sy + ix;
  bool open = ix == 0 || ix == nx - 1 || iy == 0 || iy == ny - 1 || iz == 0 || iz == nz - 1;
  if (!open) open = !(occ[i - 1] && occ[i + 1] && occ[i - sy] && occ[i + sy] && occ[i - sz] && occ[i + sz]);
  out[i] = occ[i] && open ? 1 : 0;
}

bool carve_dims_ok(const char* who, int nx, int ny, int nz) {
  if (nx < 1 || ny < 1 || nz < 1 || nx > HGS_CARVE_MAX_DIM || ny > HGS_CARVE_MAX_DIM || nz > HGS_CARVE_MAX_DIM) {
    hgs_set_error("%s: a grid of %d x %d x %d voxels (1 to %d per axis)", who, nx, ny, nz, HGS_CARVE_MAX_DIM);
    return false;
  }
  return true;
}

dim3 carve_bricks(int nx, int ny, int nz) {
  return dim3((unsigned)((nx + HGS_CARVE_BX - 1) / HGS_CARVE_BX), (unsigned)((ny + HGS_CARVE_BY - 1) / HGS_CARVE_BY), (unsigned)nz);
}

}  // namespace

extern "C" size_t hgs_carve_view_bytes(void) { return sizeof(HgsCarveView); }

extern "C" int hgs_carve_votes(void* stream, long long N, const double* points, int V, const HgsCarveView* views_dev,
                               const unsigned char* masks, const unsigned char* images, int* seen, int* hits, int* rgb_sum) {
  if (N < 0 || N > 0x7FFFFFFFll * 256) { hgs_set_error("hgs_carve_votes: N = %lld points", N); return 1; }
  if (V < 1 || V > HGS_CARVE_MAX_VIEWS) { hgs_set_error("hgs_carve_votes: V = %d views (1 to %d)", V, HGS_CARVE_MAX_VIEWS); return 1; }
  if (rgb_sum && !images) { hgs_set_error("hgs_carve_votes: rgb_sum without images"); return 1; }
  if (N == 0) return 0;
  if (!points || !views_dev || !masks || !seen || !hits) { hgs_set_error("hgs_carve_votes: null argument"); return 1; }
  const dim3 grid((unsigned)((N + 255) / 256)), block(256);
  hipLaunchKernelGGL(carve_votes_kernel, grid, block, 0, (hipStream_t)stream, N, points, V, views_dev, masks, images, seen, hits, rgb_sum);
  HGS_CHECK_LAUNCH();
  return 0;
}

extern "C" int hgs_carve_grid(void* stream, const double* origin_host, double h, int nx, int ny, int nz, int V,
                              const HgsCarveView* views_dev, const unsigned char* masks, int min_views, int min_percent,
                              unsigned char* occ) {
  if (!carve_dims_ok("hgs_carve_grid", nx, ny, nz)) return 1;
  if (V < 1 || V > HGS_CARVE_MAX_VIEWS) { hgs_set_error("hgs_carve_grid: V = %d views (1 to %d)", V, HGS_CARVE_MAX_VIEWS); return 1; }
  if (min_views < 1 || min_percent < 0 || min_percent > 100) {
    hgs_set_error("hgs_carve_grid: min_views = %d (>= 1), min_percent = %d (0 to 100)", min_views, min_percent); return 1;
  }
  if (!origin_host || !views_dev || !masks || !occ) { hgs_set_error("hgs_carve_grid: null argument"); return 1; }
  const dim3 block(HGS_CARVE_BX, HGS_CARVE_BY);
  hipLaunchKernelGGL(carve_grid_kernel, carve_bricks(nx, ny, nz), block, 0, (hipStream_t)stream, origin_host[0], origin_host[1],
                     origin_host[2], h, nx, ny, nz, V, views_dev, masks, min_views, min_percent, occ);
  HGS_CHECK_LAUNCH();
  return 0;
}

extern "C" int hgs_carve_shell(void* stream, int nx, int ny, int nz, const unsigned char* occ, unsigned char* out) {
  if (!carve_dims_ok("hgs_carve_shell", nx, ny, nz)) return 1;
  if (!occ || !out) { hgs_set_error("hgs_carve_shell: null argument"); return 1; }
  const dim3 block(HGS_CARVE_BX, HGS_CARVE_BY);
  hipLaunchKernelGGL(carve_shell_kernel, carve_bricks(nx, ny, nz), block, 0, (hipStream_t)stream, nx, ny, nz, occ, out);
  HGS_CHECK_LAUNCH();
  return 0;
}
