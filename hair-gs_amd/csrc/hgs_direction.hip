// hgs_direction.hip -- the 3-D direction term of a strand model: every segment is compared with the hair line that the capture's
// direction volume holds at its midpoint (hgs_direction_loss_forward / _backward; utils/direction_term.py states the contract, its
// numpy path and the loop restatement in tests/direction_reference.py state the same thing).  Built with -ffp-contract=off: every
// operation below is float32, rounded once, in the order written.
//
// direction_loss_kernel: one lane per segment, 256 per block.  Two 12-byte endpoint loads; the range test of the midpoint; then the
//   eight 16-byte corners (dir.xyz, conf) of its cell, all issued before the first is consumed; the tracer's corner loop with the
//   segment in the place of the previous direction (hgs_trace.hip), so a node's sign does not matter; term = sin^2 of the angle
//   between the segment and the sampled line, gs = d term / d (b - a) with the line held constant.  term and the number of active
//   segments are summed in float64: a fixed butterfly within the wave, the 4 waves in wave order through LDS, one pair per block.
// direction_reduce_kernel: one wave adds the pairs, lane l taking rows l, l + 64, ... in order, then the same butterfly;
//   out[0] = float(sum / S), 0 for S = 0; out[1] = the active segments as int32 bits.  Bitwise reproducible.
// direction_bwd_kernel: one lane per endpoint walks its run of the incidence table in order and adds +-gs; d_points = acc *
//   (upstream / S), upstream read from device memory.  No atomics, no host synchronisation anywhere; every endpoint is written.
#include "hgs_common.h"

#include <math.h>

namespace {

#define DIR_BLOCK 256
#define DIR_WAVES (DIR_BLOCK / HGS_WAVE)

struct __attribute__((packed, aligned(4))) DirPoint { float x, y, z; };

__device__ __forceinline__ float dir_dot(float ax, float ay, float az, float bx, float by, float bz) {
  return (ax * bx + ay * by) + az * bz;
}

__global__ __launch_bounds__(DIR_BLOCK) void direction_loss_kernel(int S, const DirPoint* __restrict__ points,
                                                                   const long long* __restrict__ pairs, const float4* __restrict__ vol,
                                                                   int nx, int ny, int nz, float ox, float oy, float oz, float inv_h,
                                                                   float min_conf, float* __restrict__ gs, float* __restrict__ term_out,
                                                                   float* __restrict__ w_out, double* __restrict__ partials) {
  __shared__ double s_part[2 * DIR_WAVES];
  const int s = blockIdx.x * DIR_BLOCK + threadIdx.x;
  double mine = 0.0, count = 0.0;
  if (s < S) {
    const DirPoint a = points[pairs[2 * (size_t)s]], b = points[pairs[2 * (size_t)s + 1]];
    const float ux = b.x - a.x, uy = b.y - a.y, uz = b.z - a.z;
    const float mx = (a.x + b.x) * 0.5f, my = (a.y + b.y) * 0.5f, mz = (a.z + b.z) * 0.5f;
    const float uu = dir_dot(ux, uy, uz, ux, uy, uz);
    const float tx = (mx - ox) * inv_h, ty = (my - oy) * inv_h, tz = (mz - oz) * inv_h;
    // (a NaN fails every comparison, +inf the second: the range test precedes every load)
    const bool ok = tx >= 0.f && tx < (float)(nx - 1) && ty >= 0.f && ty < (float)(ny - 1) && tz >= 0.f && tz < (float)(nz - 1);
    float term = 0.f, w = 0.f, gx = 0.f, gy = 0.f, gz = 0.f;
    if (ok) {
      const float flx = floorf(tx), fly = floorf(ty), flz = floorf(tz);
      const float4* c0 = vol + ((size_t)(int)flz * ny + (int)fly) * nx + (int)flx;       // 0 <= i <= n - 2 on every axis
      const size_t sy = (size_t)nx, sz = (size_t)nx * ny;
      float4 c[8];
      c[0] = c0[0]; c[1] = c0[1]; c[2] = c0[sy]; c[3] = c0[sy + 1];
      c[4] = c0[sz]; c[5] = c0[sz + 1]; c[6] = c0[sz + sy]; c[7] = c0[sz + sy + 1];
      const float fx = tx - flx, fy = ty - fly, fz = tz - flz;
      const float wx[2] = {1.f - fx, fx}, wy[2] = {1.f - fy, fy}, wz[2] = {1.f - fz, fz};
      float vx = 0.f, vy = 0.f, vz = 0.f;
#pragma unroll
      for (int k = 0; k < 8; k++) {                                                      // z outermost, then y, then x
        const float tw = (wx[k & 1] * wy[(k >> 1) & 1]) * wz[k >> 2];
        float q = tw * c[k].w;
        w = w + q;
        if (dir_dot(c[k].x, c[k].y, c[k].z, ux, uy, uz) < 0.f) q = -q;
        vx = vx + q * c[k].x; vy = vy + q * c[k].y; vz = vz + q * c[k].z;
      }
      const float nn = dir_dot(vx, vy, vz, vx, vy, vz);
      if (w >= min_conf && nn > 0.f && nn < INFINITY && uu > 0.f && uu < INFINITY) {
        const float len = sqrtf(nn);
        const float dx = vx / len, dy = vy / len, dz = vz / len;
        const float cu = dir_dot(ux, uy, uz, dx, dy, dz);
        const float k = cu / uu;
        term = 1.f - cu * k;
        const float m2 = -2.f * k;
        gx = m2 * (dx - k * ux); gy = m2 * (dy - k * uy); gz = m2 * (dz - k * uz);
        count = 1.0;
      }
    }
    gs[3 * (size_t)s] = gx; gs[3 * (size_t)s + 1] = gy; gs[3 * (size_t)s + 2] = gz;
    if (term_out) term_out[s] = term;
    if (w_out) w_out[s] = w;
    mine = (double)term;
  }
  const int lane = threadIdx.x & (HGS_WAVE - 1), wv = threadIdx.x / HGS_WAVE;
  mine = wave_sum(mine);
  count = wave_sum(count);
  if (lane == 0) { s_part[2 * wv] = mine; s_part[2 * wv + 1] = count; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double acc = s_part[0], n = s_part[1];
    for (int k = 1; k < DIR_WAVES; k++) { acc += s_part[2 * k]; n += s_part[2 * k + 1]; }
    partials[2 * (size_t)blockIdx.x] = acc;
    partials[2 * (size_t)blockIdx.x + 1] = n;
  }
}

__global__ __launch_bounds__(HGS_WAVE) void direction_reduce_kernel(int S, int nb, const double* __restrict__ partials,
                                                                    float* __restrict__ out) {
  const int lane = threadIdx.x;
  double acc = 0.0, n = 0.0;
  for (int r = lane; r < nb; r += HGS_WAVE) { acc += partials[2 * (size_t)r]; n += partials[2 * (size_t)r + 1]; }
  acc = wave_sum(acc);
  n = wave_sum(n);
  if (lane == 0) {
    out[0] = S > 0 ? (float)(acc / (double)S) : 0.f;
    out[1] = __int_as_float((int)n);
  }
}

__global__ __launch_bounds__(DIR_BLOCK) void direction_bwd_kernel(int E, int S, const int* __restrict__ offsets,
                                                                  const int* __restrict__ entries, const float* __restrict__ gs,
                                                                  const float* __restrict__ upstream, float* __restrict__ d_points) {
  const int e = blockIdx.x * DIR_BLOCK + threadIdx.x;
  if (e >= E) return;
  const float scale = S > 0 ? upstream[0] / (float)S : 0.f;
  float ax = 0.f, ay = 0.f, az = 0.f;
  const int end = offsets[e + 1];
  for (int i = offsets[e]; i < end; i++) {
    const int ent = entries[i];                                                          // 2 s + side
    const float* g = gs + 3 * (size_t)(ent >> 1);
    if (ent & 1) { ax = ax + g[0]; ay = ay + g[1]; az = az + g[2]; }
    else { ax = ax + -g[0]; ay = ay + -g[1]; az = az + -g[2]; }
  }
  d_points[3 * (size_t)e] = ax * scale; d_points[3 * (size_t)e + 1] = ay * scale; d_points[3 * (size_t)e + 2] = az * scale;
}

}  // namespace

extern "C" int hgs_direction_loss_num_blocks(int S) { return S < 0 ? 0 : (S + DIR_BLOCK - 1) / DIR_BLOCK; }

extern "C" int hgs_direction_loss_forward(void* stream, int S, const float* points, const long long* pairs, const float* vol, int nx,
                                          int ny, int nz, float ox, float oy, float oz, float inv_h, float min_conf, float* gs,
                                          float* term, float* w, double* partials, float* out) {
  if (S < 0 || S > (1 << 28)) { hgs_set_error("hgs_direction_loss_forward: %d segments (0 to 2^28)", S); return 1; }
  if (nx < 2 || ny < 2 || nz < 2 || nx > 1024 || ny > 1024 || nz > 1024 || (long long)nx * ny * nz > (1ll << 26)) {
    hgs_set_error("hgs_direction_loss_forward: a grid of %d x %d x %d nodes (2 to 1024 an axis, at most 2^26 in all)", nx, ny, nz);
    return 1;
  }
  if (!(inv_h > 0.f) || !isfinite(inv_h) || !isfinite(ox) || !isfinite(oy) || !isfinite(oz) || !isfinite(min_conf)) {
    hgs_set_error("hgs_direction_loss_forward: origin (%g, %g, %g), 1/h = %g and min_conf %g must be finite, 1/h > 0", ox, oy, oz, inv_h,
                  min_conf);
    return 1;
  }
  if (!vol || !out) { hgs_set_error("hgs_direction_loss_forward: vol and out are required"); return 1; }
  if (((uintptr_t)vol & 15) != 0) { hgs_set_error("hgs_direction_loss_forward: vol must be 16-byte aligned"); return 1; }
  if (S > 0 && (!points || !pairs || !gs || !partials)) {
    hgs_set_error("hgs_direction_loss_forward: points, pairs, gs and partials are required");
    return 1;
  }
  hipStream_t st = (hipStream_t)stream;
  const int nb = hgs_direction_loss_num_blocks(S);
  if (nb > 0) {
    hipLaunchKernelGGL(direction_loss_kernel, dim3(nb), dim3(DIR_BLOCK), 0, st, S, (const DirPoint*)points, pairs, (const float4*)vol, nx,
                       ny, nz, ox, oy, oz, inv_h, min_conf, gs, term, w, partials);
    HGS_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(direction_reduce_kernel, dim3(1), dim3(HGS_WAVE), 0, st, S, nb, partials, out);
  HGS_CHECK_LAUNCH();
  return 0;
}

extern "C" int hgs_direction_loss_backward(void* stream, int E, int S, const int* offsets, const int* entries, const float* gs,
                                           const float* upstream, float* d_points) {
  if (E < 0 || E > (1 << 28) || S < 0 || S > (1 << 28)) {
    hgs_set_error("hgs_direction_loss_backward: %d points and %d segments (0 to 2^28 each)", E, S);
    return 1;
  }
  if (E == 0) return 0;
  if (!offsets || !upstream || !d_points || (S > 0 && (!entries || !gs))) {
    hgs_set_error("hgs_direction_loss_backward: offsets, entries, gs, upstream and d_points are required");
    return 1;
  }
  hipLaunchKernelGGL(direction_bwd_kernel, dim3((E + DIR_BLOCK - 1) / DIR_BLOCK), dim3(DIR_BLOCK), 0, (hipStream_t)stream, E, S, offsets,
                     entries, gs, upstream, d_points);
  HGS_CHECK_LAUNCH();
  return 0;
}
