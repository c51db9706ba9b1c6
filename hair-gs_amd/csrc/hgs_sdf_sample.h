// hgs_sdf_sample.h -- the float32 trilinear value and gradient of the head's distance field: the Term statement of
// utils/head_sdf.py, operation by operation (every file that includes this is built with -ffp-contract=off).  One definition for
// head_penalty_kernel (hgs_sdf.hip) and strand_collide_kernel (hgs_collide.hip): the two cannot drift apart.
//   t = (p - o) * k per axis; in range iff every t is finite and 0 <= t < n_axis - 1; i = floor(t), f = t - i
//   d  = lerp(lerp(lerp(c000, c100, fx), lerp(c010, c110, fx), fy), lerp(lerp(c001, c101, fx), lerp(c011, c111, fx), fy), fz)
//   gx = lerp(lerp(c100 - c000, c110 - c010, fy), lerp(c101 - c001, c111 - c011, fy), fz) * k, gy and gz likewise
#pragma once

#include <hip/hip_runtime.h>

struct SdfCell {
  float c000, c100, c010, c110, c001, c101, c011, c111;   // c_xyz = phi[iz + z][iy + y][ix + x]
  float fx, fy, fz;
};

__device__ __forceinline__ float sdf_lerp(float a, float b, float f) { return a + f * (b - a); }

// the grid coordinates of p, and whether they are in range (a NaN fails every comparison, +inf the second)
__device__ __forceinline__ bool sdf_grid_coords(float x, float y, float z, float ox, float oy, float oz, float inv_h, int nx, int ny, int nz,
                                                float& tx, float& ty, float& tz) {
  tx = (x - ox) * inv_h; ty = (y - oy) * inv_h; tz = (z - oz) * inv_h;
  return tx >= 0.f && tx < (float)(nx - 1) && ty >= 0.f && ty < (float)(ny - 1) && tz >= 0.f && tz < (float)(nz - 1);
}

// the eight corners and the fractions of the cell of in-range coordinates: 0 <= i <= n - 2 on every axis
__device__ __forceinline__ SdfCell sdf_cell(const float* __restrict__ phi, int nx, int ny, float tx, float ty, float tz) {
  const float flx = floorf(tx), fly = floorf(ty), flz = floorf(tz);
  const int ix = (int)flx, iy = (int)fly, iz = (int)flz;
  const float* c = phi + ((size_t)iz * ny + iy) * nx + ix;
  const size_t sy = (size_t)nx, szz = (size_t)nx * ny;
  SdfCell k;
  k.fx = tx - flx; k.fy = ty - fly; k.fz = tz - flz;
  k.c000 = c[0]; k.c100 = c[1]; k.c010 = c[sy]; k.c110 = c[sy + 1];
  k.c001 = c[szz]; k.c101 = c[szz + 1]; k.c011 = c[szz + sy]; k.c111 = c[szz + sy + 1];
  return k;
}

__device__ __forceinline__ float sdf_value(const SdfCell& k) {
  const float c00 = sdf_lerp(k.c000, k.c100, k.fx), c10 = sdf_lerp(k.c010, k.c110, k.fx);
  const float c01 = sdf_lerp(k.c001, k.c101, k.fx), c11 = sdf_lerp(k.c011, k.c111, k.fx);
  const float c0 = sdf_lerp(c00, c10, k.fy), c1 = sdf_lerp(c01, c11, k.fy);
  return sdf_lerp(c0, c1, k.fz);
}

__device__ __forceinline__ void sdf_gradient(const SdfCell& k, float inv_h, float& dx, float& dy, float& dz) {
  dx = sdf_lerp(sdf_lerp(k.c100 - k.c000, k.c110 - k.c010, k.fy), sdf_lerp(k.c101 - k.c001, k.c111 - k.c011, k.fy), k.fz) * inv_h;
  dy = sdf_lerp(sdf_lerp(k.c010 - k.c000, k.c110 - k.c100, k.fx), sdf_lerp(k.c011 - k.c001, k.c111 - k.c101, k.fx), k.fz) * inv_h;
  dz = sdf_lerp(sdf_lerp(k.c001 - k.c000, k.c101 - k.c100, k.fx), sdf_lerp(k.c011 - k.c010, k.c111 - k.c110, k.fx), k.fy) * inv_h;
}
