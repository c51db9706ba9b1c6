// hgs_scalp.hip -- the scalp of a capture labelled on its head mesh from the hair masks (utils/scalp.py states the contract,
// init_scalp.py is the scene driver): hgs_scalp_depth, hgs_scalp_votes.  gfx950, wave64.
//
// The contract (one definition for the numpy path, these kernels and the tests' loop restatement).  Views are HgsCarveView records;
// xc, yc, zc, u, v, seen, px, py of a point as in hgs_pinhole.h.  All float64, one rounding per operation in the order written (this
// file is built with -ffp-contract=off).
// Depth map of view k, Z[H][W], +inf to begin with.  For a face with (xc_i, yc_i, zc_i), (u_i, v_i) of its vertices i = 0, 1, 2:
//   dropped (and counted) when a zc_i is not > 0 or a u_i, v_i is not finite
//   candidates: max(0, ceil(min u - 0.5)) <= px <= min(W - 1, floor(max u - 0.5)), likewise py; centre (cx, cy) = (px + 0.5, py + 0.5)
//   E0 = (u2 - u1)*(cy - v1) - (v2 - v1)*(cx - u1),  E1 = (u0 - u2)*(cy - v2) - (v0 - v2)*(cx - u2),
//   E2 = (u1 - u0)*(cy - v0) - (v1 - v0)*(cx - u0),  S = (E0 + E1) + E2
//   covered iff S != 0 and (every E >= 0 or every E <= 0)
//   iz = (E0*(1/zc0) + E1*(1/zc1)) + E2*(1/zc2),  z = S/iz;   Z[py][px] = min(Z[py][px], z) where covered and 0 < z < inf
// Vote of the sample (p, n) in view k:
//   nc_r = (R_r0*n0 + R_r1*n1) + R_r2*n2;  d = -((nc0*xc + nc1*yc) + nc2*zc);  nn = (nc0*nc0 + nc1*nc1) + nc2*nc2;
//   pp = (xc*xc + yc*yc) + zc*zc;  facing iff d > 0 and d*d >= (min_cos*min_cos)*(nn*pp)
//   visible iff seen and facing and zc <= Z[py][px] + depth_tol;   vis += visible, hits += visible and mask[py][px] != 0
//
// Work split of the depth kernel.  A face's footprint is anything from no pixel to the whole frame, so a lane per face with a pixel
// loop of its own would leave 63 lanes waiting for the largest face.  Instead a workgroup is ONE wavefront that owns 64 consecutive
// faces of one view (grid: face chunks x views).  Each lane sets up one face -- projection, drop test, clipped box -- and parks it in
// LDS; the wavefront then takes the faces that have candidates one after another (a ballot names them: a wavefront-uniform loop) and
// its lanes stride over that face's box.  The map is lowered by a 64-bit unsigned atomic minimum on the bit pattern of z: the bits of
// positive doubles order like the doubles, +inf above every finite one, and an integer minimum is exact and order-free, so the maps
// are bitwise reproducible whatever the schedule.  A lane first reads the cell and skips the atomic where the cell is already as
// low: a cell only ever falls, so a stale read can cost an atomic and never lose one.  The maps are set to +inf by a launch of this
// file (fill kernel) in front, on the same stream.  The vote kernel is hgs_carve_votes' shape: one lane per sample, the view loop
// inside it, the view record indexed by the loop counter alone.
#include <stdint.h>

#include "hgs_common.h"
#include "hgs_pinhole.h"

#define HGS_SCALP_MAX_VIEWS 4096
#define HGS_SCALP_MAX_VERTS (1 << 24)
#define HGS_SCALP_MAX_FACES (1 << 24)
#define HGS_SCALP_INF_BITS 0x7FF0000000000000ull

namespace {

__device__ __forceinline__ bool scalp_finite(double a) { return a - a == 0.0; }   // (false for NaN and both infinities)

// grid (blocks, V): the blocks of row k stride over view k's W*H cells; block (0, 0) also clears the drop counter
__global__ __launch_bounds__(256) void scalp_fill_kernel(const HgsCarveView* __restrict__ views, unsigned long long* __restrict__ depth,
                                                         unsigned long long* __restrict__ dropped) {
  const HgsCarveView& c = views[blockIdx.y];
  const size_t n = (size_t)c.W * (size_t)c.H;
  unsigned long long* __restrict__ z = depth + (size_t)c.mask_offset;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) z[i] = HGS_SCALP_INF_BITS;
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *dropped = 0;
}

__global__ __launch_bounds__(64) void scalp_depth_kernel(const double* __restrict__ verts, int F, const int* __restrict__ faces,
                                                         const HgsCarveView* __restrict__ views, unsigned long long* __restrict__ depth,
                                                         unsigned long long* __restrict__ dropped) {
  __shared__ double s_u[3][64], s_v[3][64], s_iz[3][64];
  __shared__ int s_x0[64], s_y0[64], s_bw[64], s_bh[64];
  const int lane = threadIdx.x;
  const int f = blockIdx.x * 64 + lane;
  const HgsCarveView& c = views[blockIdx.y];
  const int W = c.W, H = c.H;
  bool drop = false;
  int bw = 0, bh = 0;
  if (f < F) {
    double u[3], v[3], iz[3];
    bool ok = true;
    for (int i = 0; i < 3; i++) {
      const double* __restrict__ p = verts + 3 * (size_t)faces[3 * (size_t)f + i];   // (the caller guarantees 0 <= index < NV)
      const Pinhole q = pinhole_project(c, p[0], p[1], p[2]);
      u[i] = q.u;
      v[i] = q.v;
      iz[i] = 1.0 / q.zc;
      ok = ok && q.zc > 0.0 && scalp_finite(u[i]) && scalp_finite(v[i]);
    }
    drop = !ok;
    if (ok) {
      const double x0 = fmax(0.0, ceil(fmin(fmin(u[0], u[1]), u[2]) - 0.5)), x1 = fmin((double)W - 1.0, floor(fmax(fmax(u[0], u[1]), u[2]) - 0.5));
      const double y0 = fmax(0.0, ceil(fmin(fmin(v[0], v[1]), v[2]) - 0.5)), y1 = fmin((double)H - 1.0, floor(fmax(fmax(v[0], v[1]), v[2]) - 0.5));
      if (x0 <= x1 && y0 <= y1) {                                 // both ends lie in [0, W - 1] x [0, H - 1]: the casts are exact
        s_x0[lane] = (int)x0;
        s_y0[lane] = (int)y0;
        bw = (int)x1 - (int)x0 + 1;
        bh = (int)y1 - (int)y0 + 1;
        for (int i = 0; i < 3; i++) { s_u[i][lane] = u[i]; s_v[i][lane] = v[i]; s_iz[i][lane] = iz[i]; }
      }
    }
  }
  s_bw[lane] = bw;
  s_bh[lane] = bh;
  const unsigned long long drops = __ballot(drop);
  if (lane == 0 && drops) atomicAdd(dropped, (unsigned long long)__popcll(drops));
  unsigned long long live = __ballot(bw > 0);
  __syncthreads();
  unsigned long long* Z = depth + (size_t)c.mask_offset;
  while (live) {                                                    // wavefront-uniform: the faces of this chunk that have candidates
    const int j = __ffsll((long long)live) - 1;
    live &= live - 1;
    const double u0 = s_u[0][j], u1 = s_u[1][j], u2 = s_u[2][j], v0 = s_v[0][j], v1 = s_v[1][j], v2 = s_v[2][j];
    const double iz0 = s_iz[0][j], iz1 = s_iz[1][j], iz2 = s_iz[2][j];
    const double a0 = u2 - u1, b0 = v2 - v1, a1 = u0 - u2, b1 = v0 - v2, a2 = u1 - u0, b2 = v1 - v0;
    const int x0 = s_x0[j], y0 = s_y0[j], w = s_bw[j];
    const unsigned n = (unsigned)w * (unsigned)s_bh[j];           // (at most W*H, which the caller keeps below 2^31)
    for (unsigned i = (unsigned)lane; i < n; i += 64) {
      const int py = y0 + (int)(i / (unsigned)w), px = x0 + (int)(i % (unsigned)w);   // 0 <= px < W, 0 <= py < H by the clipped box
      const double cx = (double)px + 0.5, cy = (double)py + 0.5;
      const double E0 = a0 * (cy - v1) - b0 * (cx - u1);
      const double E1 = a1 * (cy - v2) - b1 * (cx - u2);
      const double E2 = a2 * (cy - v0) - b2 * (cx - u0);
      const double S = (E0 + E1) + E2;
      const bool covered = S != 0.0 && ((E0 >= 0.0 && E1 >= 0.0 && E2 >= 0.0) || (E0 <= 0.0 && E1 <= 0.0 && E2 <= 0.0));
      if (!covered) continue;
      const double z = S / ((E0 * iz0 + E1 * iz1) + E2 * iz2);
      if (!(z > 0.0 && z < __longlong_as_double((long long)HGS_SCALP_INF_BITS))) continue;
      unsigned long long* cell = Z + ((size_t)py * (size_t)W + (size_t)px);
      const unsigned long long bits = (unsigned long long)__double_as_longlong(z);
      if (*cell > bits) atomicMin(cell, bits);
    }
  }
}

__global__ __launch_bounds__(256) void scalp_votes_kernel(long long N, const double* __restrict__ points, const double* __restrict__ normals,
                                                          int V, const HgsCarveView* __restrict__ views,
                                                          const unsigned char* __restrict__ masks, const double* __restrict__ depth,
                                                          double cos2, double depth_tol, int* __restrict__ vis_out, int* __restrict__ hits_out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const double x = points[3 * (size_t)i], y = points[3 * (size_t)i + 1], z = points[3 * (size_t)i + 2];
  const double n0 = normals[3 * (size_t)i], n1 = normals[3 * (size_t)i + 1], n2 = normals[3 * (size_t)i + 2];
  int vis = 0, hits = 0;
  for (int k = 0; k < V; k++) {
    const HgsCarveView& c = views[k];
    const Pinhole q = pinhole_project(c, x, y, z);
    if (!pinhole_seen(&c, q)) continue;
    const double nc0 = (c.R[0] * n0 + c.R[1] * n1) + c.R[2] * n2;
    const double nc1 = (c.R[3] * n0 + c.R[4] * n1) + c.R[5] * n2;
    const double nc2 = (c.R[6] * n0 + c.R[7] * n1) + c.R[8] * n2;
    const double d = -((nc0 * q.xc + nc1 * q.yc) + nc2 * q.zc);
    const double nn = (nc0 * nc0 + nc1 * nc1) + nc2 * nc2, pp = (q.xc * q.xc + q.yc * q.yc) + q.zc * q.zc;
    if (!(d > 0.0 && d * d >= cos2 * (nn * pp))) continue;          // not facing
    const size_t pixel = pinhole_pixel(c, q);
    if (!(q.zc <= depth[(size_t)c.mask_offset + pixel] + depth_tol)) continue;          // hidden
    vis++;
    if (masks[(size_t)c.mask_offset + pixel] != 0) hits++;
  }
  vis_out[i] = vis;
  hits_out[i] = hits;
}

}  // namespace

extern "C" int hgs_scalp_depth(void* stream, int NV, const double* verts, int F, const int* faces, int V, const HgsCarveView* views_dev,
                               double* depth, unsigned long long* dropped) {
  if (V < 1 || V > HGS_SCALP_MAX_VIEWS) { hgs_set_error("hgs_scalp_depth: V = %d views (1 to %d)", V, HGS_SCALP_MAX_VIEWS); return 1; }
  if (NV < 0 || NV > HGS_SCALP_MAX_VERTS) { hgs_set_error("hgs_scalp_depth: NV = %d vertices (0 to %d)", NV, HGS_SCALP_MAX_VERTS); return 1; }
  if (F < 0 || F > HGS_SCALP_MAX_FACES) { hgs_set_error("hgs_scalp_depth: F = %d faces (0 to %d)", F, HGS_SCALP_MAX_FACES); return 1; }
  if (F > 0 && NV == 0) { hgs_set_error("hgs_scalp_depth: F = %d faces of no vertex", F); return 1; }
  if (!views_dev || !depth || !dropped || (F > 0 && (!verts || !faces))) { hgs_set_error("hgs_scalp_depth: null argument"); return 1; }
  hipLaunchKernelGGL(scalp_fill_kernel, dim3(64, (unsigned)V), dim3(256), 0, (hipStream_t)stream, views_dev, (unsigned long long*)depth,
                     dropped);
  HGS_CHECK_LAUNCH();
  if (F == 0) return 0;
  hipLaunchKernelGGL(scalp_depth_kernel, dim3((unsigned)((F + 63) / 64), (unsigned)V), dim3(64), 0, (hipStream_t)stream, verts, F, faces,
                     views_dev, (unsigned long long*)depth, dropped);
  HGS_CHECK_LAUNCH();
  return 0;
}

extern "C" int hgs_scalp_votes(void* stream, long long N, const double* points, const double* normals, int V, const HgsCarveView* views_dev,
                               const unsigned char* masks, const double* depth, double min_cos, double depth_tol, int* vis, int* hits) {
  if (N < 0 || N > 0x7FFFFFFFll * 256) { hgs_set_error("hgs_scalp_votes: N = %lld samples", N); return 1; }
  if (V < 1 || V > HGS_SCALP_MAX_VIEWS) { hgs_set_error("hgs_scalp_votes: V = %d views (1 to %d)", V, HGS_SCALP_MAX_VIEWS); return 1; }
  if (!(min_cos >= 0.0 && min_cos <= 1.0)) { hgs_set_error("hgs_scalp_votes: min_cos = %g (0 to 1)", min_cos); return 1; }
  if (!(depth_tol >= 0.0 && depth_tol - depth_tol == 0.0)) {
    hgs_set_error("hgs_scalp_votes: depth_tol = %g (finite and >= 0)", depth_tol); return 1;
  }
  if (N == 0) return 0;
  if (!points || !normals || !views_dev || !masks || !depth || !vis || !hits) { hgs_set_error("hgs_scalp_votes: null argument"); return 1; }
  hipLaunchKernelGGL(scalp_votes_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, N, points, normals, V,
                     views_dev, masks, depth, min_cos * min_cos, depth_tol, vis, hits);
  HGS_CHECK_LAUNCH();
  return 0;
}
