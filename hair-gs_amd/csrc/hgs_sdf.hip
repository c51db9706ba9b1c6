// hgs_sdf.hip -- the head mesh as a signed distance field, and the penetration term that samples it at the strand joints
// (hgs_mesh_sdf, hgs_head_penalty_forward / _backward; utils/head_sdf.py states the contract, its numpy path and the loop
// restatement in tests/head_sdf_reference.py state the same thing).  Built with -ffp-contract=off: every operation below is
// rounded once, in the order written.
//
// mesh_sdf_kernel: one lane per node of the [nz][ny][nx] grid, 256 lanes (4 waves) per block.  The F triangles (9 float64 each:
//   v0, v1, v2) pass through LDS in tiles of SDF_TILE faces; every lane walks the tile in face order, so a node sees the faces in
//   the order 0 .. F-1 whatever the grid.  Per (node, face) the differences a = v0 - p, b = v1 - p, c = v2 - p are formed once and
//   feed both the closest-point region form (squared distance, minimised: independent of the order) and the solid angle (summed in
//   face order).  Nothing is shared between lanes beyond the staged tile: no atomics, no reduction.
// head_penalty_kernel: one lane per point, 256 per block; float32, operation by operation.  Eight gathers of the field, value and
//   analytic gradient of the trilinear interpolant, pen = r r and g = (-2 r) grad d for r = margin - d > 0 in range.  pen is summed in
//   float64: a fixed butterfly within the wave, the 4 waves in wave order through LDS, one partial per block.
// head_penalty_reduce_kernel: one wave adds the partials, lane l taking rows l, l + 64, ... in order, then the same butterfly;
//   out[0] = float(sum / E), 0 for E = 0.  Bitwise reproducible.
// head_penalty_bwd_kernel: d_points = g * (upstream / E), upstream read from device memory: no host synchronisation anywhere.
#include "hgs_common.h"
#include "hgs_sdf_sample.h"

#include <math.h>

namespace {

#define SDF_BLOCK 256
#define SDF_WAVES (SDF_BLOCK / HGS_WAVE)
#define SDF_TILE 256                 // faces per LDS tile: 256 * 9 * 8 = 18 KiB

__global__ __launch_bounds__(SDF_BLOCK) void mesh_sdf_kernel(int F, const double* __restrict__ tris, double ox, double oy, double oz,
                                                             double h, int nx, int ny, long long N, float* __restrict__ phi,
                                                             double* __restrict__ winding) {
  __shared__ double s_tri[SDF_TILE * 9];
  const long long node = (long long)blockIdx.x * SDF_BLOCK + threadIdx.x;
  const bool live = node < N;
  const long long safe = live ? node : 0;
  const int ix = (int)(safe % nx), iy = (int)((safe / nx) % ny), iz = (int)(safe / ((long long)nx * ny));
  const double px = ox + (double)ix * h, py = oy + (double)iy * h, pz = oz + (double)iz * h;
  double best = INFINITY, S = 0.0;
  for (int base = 0; base < F; base += SDF_TILE) {
    const int nt = min(SDF_TILE, F - base);
    __syncthreads();                 // (the previous tile is read out)
    for (int i = threadIdx.x; i < nt * 9; i += SDF_BLOCK) s_tri[i] = tris[(size_t)base * 9 + i];
    __syncthreads();
    if (!live) continue;
    for (int f = 0; f < nt; f++) {
      const double* t = s_tri + f * 9;
      const double v0x = t[0], v0y = t[1], v0z = t[2], v1x = t[3], v1y = t[4], v1z = t[5], v2x = t[6], v2y = t[7], v2z = t[8];
      const double ax = v0x - px, ay = v0y - py, az = v0z - pz;
      const double bx = v1x - px, by = v1y - py, bz = v1z - pz;
      const double cx = v2x - px, cy = v2y - py, cz = v2z - pz;
      // ---- closest point, region form; ap = -a, bp = -b, cp = -c (exact)
      const double e1x = v1x - v0x, e1y = v1y - v0y, e1z = v1z - v0z;      // ab
      const double e2x = v2x - v0x, e2y = v2y - v0y, e2z = v2z - v0z;      // ac
      const double d1 = dot3(e1x, e1y, e1z, -ax, -ay, -az), d2 = dot3(e2x, e2y, e2z, -ax, -ay, -az);
      const double d3 = dot3(e1x, e1y, e1z, -bx, -by, -bz), d4 = dot3(e2x, e2y, e2z, -bx, -by, -bz);
      const double d5 = dot3(e1x, e1y, e1z, -cx, -cy, -cz), d6 = dot3(e2x, e2y, e2z, -cx, -cy, -cz);
      const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
      double qx, qy, qz;
      if (d1 <= 0.0 && d2 <= 0.0) {                                        // vertex v0
        qx = -ax; qy = -ay; qz = -az;
      } else if (d3 >= 0.0 && d4 <= d3) {                                  // vertex v1
        qx = -bx; qy = -by; qz = -bz;
      } else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {                    // edge v0 v1
        const double v = d1 / (d1 - d3);
        qx = -ax - v * e1x; qy = -ay - v * e1y; qz = -az - v * e1z;
      } else if (d6 >= 0.0 && d5 <= d6) {                                  // vertex v2
        qx = -cx; qy = -cy; qz = -cz;
      } else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {                    // edge v0 v2
        const double w = d2 / (d2 - d6);
        qx = -ax - w * e2x; qy = -ay - w * e2y; qz = -az - w * e2z;
      } else if (va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0) {      // edge v1 v2
        const double w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        qx = -bx - w * (v2x - v1x); qy = -by - w * (v2y - v1y); qz = -bz - w * (v2z - v1z);
      } else {                                                             // interior
        const double den = 1.0 / ((va + vb) + vc);
        const double v = vb * den, w = vc * den;
        qx = -ax - (e1x * v + e2x * w); qy = -ay - (e1y * v + e2y * w); qz = -az - (e1z * v + e2z * w);
      }
      const double dist2 = dot3(qx, qy, qz, qx, qy, qz);
      if (dist2 < best) best = dist2;                                      // (a NaN or +inf never passes: the face is skipped)
      // ---- solid angle
      const double la = sqrt(dot3(ax, ay, az, ax, ay, az)), lb = sqrt(dot3(bx, by, bz, bx, by, bz)), lc = sqrt(dot3(cx, cy, cz, cx, cy, cz));
      const double det = (ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz)) + az * (bx * cy - by * cx);
      const double ab = dot3(ax, ay, az, bx, by, bz), bc = dot3(bx, by, bz, cx, cy, cz), ca = dot3(cx, cy, cz, ax, ay, az);
      const double den = (((la * lb) * lc + ab * lc) + bc * la) + ca * lb;
      S += 2.0 * atan2(det, den);
    }
  }
  if (!live) return;
  const double w = S / 12.566370614359172;                                 // 4 pi
  const double d = sqrt(best);
  float v = (float)d;
  if (w > 0.5 && v != 0.f) v = -v;                                         // (a zero is stored as +0)
  phi[node] = v;
  if (winding) winding[node] = w;
}

__global__ __launch_bounds__(SDF_BLOCK) void head_penalty_kernel(int E, const float* __restrict__ points, const float* __restrict__ phi,
                                                                 int nx, int ny, int nz, float ox, float oy, float oz, float inv_h,
                                                                 float margin, float* __restrict__ g, float* __restrict__ pen_out,
                                                                 float* __restrict__ dist_out, double* __restrict__ partials) {
  __shared__ double s_part[SDF_WAVES];
  const int e = blockIdx.x * SDF_BLOCK + threadIdx.x;
  double mine = 0.0;
  if (e < E) {
    const float x = points[3 * (size_t)e], y = points[3 * (size_t)e + 1], z = points[3 * (size_t)e + 2];
    // (the sampling statement: hgs_sdf_sample.h, shared with hgs_collide.hip)
    float tx, ty, tz;
    const bool in = sdf_grid_coords(x, y, z, ox, oy, oz, inv_h, nx, ny, nz, tx, ty, tz);
    float pen = 0.f, gx = 0.f, gy = 0.f, gz = 0.f, d = INFINITY;
    if (in) {
      const SdfCell cell = sdf_cell(phi, nx, ny, tx, ty, tz);
      d = sdf_value(cell);
      const float r = margin - d;
      if (r > 0.f) {
        float dx, dy, dz;
        sdf_gradient(cell, inv_h, dx, dy, dz);
        const float s = -2.f * r;
        pen = r * r;
        gx = s * dx; gy = s * dy; gz = s * dz;
      }
    }
    g[3 * (size_t)e] = gx; g[3 * (size_t)e + 1] = gy; g[3 * (size_t)e + 2] = gz;
    if (pen_out) pen_out[e] = pen;
    if (dist_out) dist_out[e] = d;
    mine = (double)pen;
  }
  const int lane = threadIdx.x & (HGS_WAVE - 1), wv = threadIdx.x / HGS_WAVE;
  mine = wave_sum(mine);
  if (lane == 0) s_part[wv] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    double acc = s_part[0];
    for (int w = 1; w < SDF_WAVES; w++) acc += s_part[w];
    partials[blockIdx.x] = acc;
  }
}

__global__ __launch_bounds__(HGS_WAVE) void head_penalty_reduce_kernel(int E, int nb, const double* __restrict__ partials,
                                                                       float* __restrict__ out) {
  const int lane = threadIdx.x;
  double acc = 0.0;
  for (int r = lane; r < nb; r += HGS_WAVE) acc += partials[r];
  acc = wave_sum(acc);
  if (lane == 0) out[0] = E > 0 ? (float)(acc / (double)E) : 0.f;
}

__global__ __launch_bounds__(SDF_BLOCK) void head_penalty_bwd_kernel(int n, int E, const float* __restrict__ g,
                                                                     const float* __restrict__ upstream, float* __restrict__ d_points) {
  const int i = blockIdx.x * SDF_BLOCK + threadIdx.x;
  if (i >= n) return;
  const float s = upstream[0] / (float)E;
  d_points[i] = g[i] * s;
}

}  // namespace

extern "C" int hgs_mesh_sdf(void* stream, int F, const double* tris, double ox, double oy, double oz, double h, int nx, int ny, int nz,
                            float* phi, double* winding) {
  if (F < 1 || F > (1 << 24)) { hgs_set_error("hgs_mesh_sdf: %d faces (1 to 2^24)", F); return 1; }
  if (nx < 1 || ny < 1 || nz < 1 || nx > 1024 || ny > 1024 || nz > 1024 || (long long)nx * ny * nz >= (1ll << 31)) {
    hgs_set_error("hgs_mesh_sdf: a grid of %d x %d x %d nodes (1 to 1024 an axis, fewer than 2^31 in all)", nx, ny, nz);
    return 1;
  }
  if (!(h > 0.0) || !isfinite(h) || !isfinite(ox) || !isfinite(oy) || !isfinite(oz)) {
    hgs_set_error("hgs_mesh_sdf: origin (%g, %g, %g) and spacing %g must be finite, the spacing > 0", ox, oy, oz, h);
    return 1;
  }
  if (!tris || !phi) { hgs_set_error("hgs_mesh_sdf: tris and phi are required"); return 1; }
  const long long N = (long long)nx * ny * nz;
  const unsigned nb = (unsigned)((N + SDF_BLOCK - 1) / SDF_BLOCK);
  hipLaunchKernelGGL(mesh_sdf_kernel, dim3(nb), dim3(SDF_BLOCK), 0, (hipStream_t)stream, F, tris, ox, oy, oz, h, nx, ny, N, phi, winding);
  HGS_CHECK_LAUNCH();
  return 0;
}

extern "C" int hgs_head_penalty_num_blocks(int E) { return E < 0 ? 0 : (E + SDF_BLOCK - 1) / SDF_BLOCK; }

static int head_grid_check(const char* who, int E, int nx, int ny, int nz) {
  if (E < 0 || E > (1 << 28)) { hgs_set_error("%s: %d points (0 to 2^28)", who, E); return 1; }
  if (nx < 1 || ny < 1 || nz < 1 || nx > 1024 || ny > 1024 || nz > 1024 || (long long)nx * ny * nz >= (1ll << 31)) {
    hgs_set_error("%s: a grid of %d x %d x %d nodes (1 to 1024 an axis, fewer than 2^31 in all)", who, nx, ny, nz);
    return 1;
  }
  return 0;
}

extern "C" int hgs_head_penalty_forward(void* stream, int E, const float* points, const float* phi, int nx, int ny, int nz, float ox,
                                        float oy, float oz, float inv_h, float margin, float* g, float* pen, float* dist,
                                        double* partials, float* out) {
  if (head_grid_check("hgs_head_penalty_forward", E, nx, ny, nz)) return 1;
  if (!(inv_h > 0.f) || !isfinite(inv_h) || !isfinite(ox) || !isfinite(oy) || !isfinite(oz) || !isfinite(margin)) {
    hgs_set_error("hgs_head_penalty_forward: origin (%g, %g, %g), 1/h = %g and margin %g must be finite, 1/h > 0", ox, oy, oz, inv_h, margin);
    return 1;
  }
  if (!phi || !out) { hgs_set_error("hgs_head_penalty_forward: phi and out are required"); return 1; }
  if (E > 0 && (!points || !g || !partials)) { hgs_set_error("hgs_head_penalty_forward: points, g and partials are required"); return 1; }
  hipStream_t st = (hipStream_t)stream;
  const int nb = hgs_head_penalty_num_blocks(E);
  if (nb > 0) {
    hipLaunchKernelGGL(head_penalty_kernel, dim3(nb), dim3(SDF_BLOCK), 0, st, E, points, phi, nx, ny, nz, ox, oy, oz, inv_h, margin, g,
                       pen, dist, partials);
    HGS_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(head_penalty_reduce_kernel, dim3(1), dim3(HGS_WAVE), 0, st, E, nb, partials, out);
  HGS_CHECK_LAUNCH();
  return 0;
}

extern "C" int hgs_head_penalty_backward(void* stream, int E, const float* g, const float* upstream, float* d_points) {
  if (E < 0 || E > (1 << 28)) { hgs_set_error("hgs_head_penalty_backward: %d points (0 to 2^28)", E); return 1; }
  if (E == 0) return 0;
  if (!g || !upstream || !d_points) { hgs_set_error("hgs_head_penalty_backward: g, upstream and d_points are required"); return 1; }
  const int n = 3 * E;
  hipLaunchKernelGGL(head_penalty_bwd_kernel, dim3((n + SDF_BLOCK - 1) / SDF_BLOCK), dim3(SDF_BLOCK), 0, (hipStream_t)stream, n, E, g,
                     upstream, d_points);
  HGS_CHECK_LAUNCH();
  return 0;
}
