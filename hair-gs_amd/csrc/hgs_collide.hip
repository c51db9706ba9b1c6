// hgs_collide.hip -- exported strands pushed out of the head, keeping their segment lengths (hgs_strand_collide;
// scene/strand_collide.py states the contract, its numpy path and the loop restatement in tests/collide_reference.py state the same
// thing).  gfx950, wave64.  Built with -ffp-contract=off: every operation below is rounded once, in the order written.  The strand
// arithmetic is float64, dot(u, v) = (u0*v0 + u1*v1) + u2*v2; the field is sampled by the float32 statement of hgs_sdf_sample.h, the
// one head_penalty_kernel uses.
//
// strand_collide_kernel: one lane per strand, 256 strands per workgroup.  The recurrence along a strand is sequential (joint j aims
//   at its original place and is put back a segment's length from the MOVED joint j - 1: follow the leader), the parallelism is the
//   strands.  A lane walks its own joints: 12-byte loads at a stride of one strand between neighbouring lanes, the plain form.  Per
//   joint: one sample of the field (eight gathers) where nothing is hit; per push one more.  The sample that ends the push loop is
//   the sample of the joint's final place whenever the push did not move it again, and is then not taken twice.  Nothing is shared
//   between lanes: no LDS, no atomics, bitwise reproducible.
#include "hgs_common.h"
#include "hgs_sdf_sample.h"

#include <math.h>

namespace {

#define COLLIDE_BLOCK 256

struct D3 { double x, y, z; };

__device__ __forceinline__ double cdot(const D3& u, const D3& v) { return (u.x * v.x + u.y * v.y) + u.z * v.z; }

struct Field {
  const float* __restrict__ phi;
  int nx, ny, nz;
  float ox, oy, oz, inv_h;
};

// S(x): the float32 statement at p = float32(x); a point that is not finite or out of range has ok false
__device__ __forceinline__ bool collide_sample(const Field& f, const D3& x, bool want_g, float& d, float& gx, float& gy, float& gz) {
  float tx, ty, tz;
  if (!sdf_grid_coords((float)x.x, (float)x.y, (float)x.z, f.ox, f.oy, f.oz, f.inv_h, f.nx, f.ny, f.nz, tx, ty, tz)) return false;
  const SdfCell cell = sdf_cell(f.phi, f.nx, f.ny, tx, ty, tz);
  d = sdf_value(cell);
  if (want_g) sdf_gradient(cell, f.inv_h, gx, gy, gz);
  return true;
}

// x put back at the segment's length L from the moved predecessor q; where that has no meaning, the original offset e
__device__ __forceinline__ D3 collide_relen(const D3& x, const D3& q, const D3& e, double L) {
  const D3 u = {x.x - q.x, x.y - q.y, x.z - q.z};
  const double lu = sqrt(cdot(u, u));
  if (isfinite(L) && isfinite(lu) && lu > 0.0) {
    const double s = L / lu;
    return {q.x + s * u.x, q.y + s * u.y, q.z + s * u.z};
  }
  return {q.x + e.x, q.y + e.y, q.z + e.z};
}

__global__ __launch_bounds__(COLLIDE_BLOCK) void strand_collide_kernel(int K, const long long* __restrict__ offsets, long long P,
                                                                      const float* __restrict__ points, Field f, float margin,
                                                                      float skin, int iters, float* __restrict__ out,
                                                                      int* __restrict__ moved_out, int* __restrict__ unresolved_out) {
  const int s = blockIdx.x * COLLIDE_BLOCK + threadIdx.x;
  if (s >= K) return;
  const long long a = offsets[s], b = offsets[s + 1];
  int n_moved = 0, n_unresolved = 0;
  // (the offsets are the caller's duty; a range that is not inside the P points is skipped, never followed out of the buffers)
  if (a >= 0 && b >= a && b <= P && b > a) {
    const float* const p = points + 3 * (size_t)a;
    float* const o = out + 3 * (size_t)a;
    const long long n = b - a;
    o[0] = p[0]; o[1] = p[1]; o[2] = p[2];                                  // the root never moves
    D3 prev = {(double)p[0], (double)p[1], (double)p[2]};                   // p_{j-1}, the original
    D3 q = prev;                                                            // q_{j-1}, the moved
    const double reach = (double)margin + (double)skin;
    bool moved = false;
    for (long long j = 1; j < n; j++) {
      const D3 pj = {(double)p[3 * j], (double)p[3 * j + 1], (double)p[3 * j + 2]};
      const D3 e = {pj.x - prev.x, pj.y - prev.y, pj.z - prev.z};
      const double L = sqrt(cdot(e, e));
      D3 x = pj;
      if (moved) x = collide_relen(x, q, e, L);
      bool hit = false;
      int state = 2;                       // how the push loop ended: 0 = x is outside, 1 = x is inside and stays, 2 = x is not sampled yet
      for (int it = 0; it < iters; it++) {
        float d = 0.f, gx = 0.f, gy = 0.f, gz = 0.f;
        const bool ok = collide_sample(f, x, true, d, gx, gy, gz);
        if (!(ok && d < margin)) { state = 0; break; }
        const D3 G = {(double)gx, (double)gy, (double)gz};
        const double gn = sqrt(cdot(G, G));
        if (!(isfinite(gn) && gn > 0.0)) { state = 1; break; }
        const double c = (reach - (double)d) / gn;
        x.x = x.x + c * G.x; x.y = x.y + c * G.y; x.z = x.z + c * G.z;
        hit = true;
        x = collide_relen(x, q, e, L);
      }
      if (hit) { moved = true; n_moved++; }
      o[3 * j] = (float)x.x; o[3 * j + 1] = (float)x.y; o[3 * j + 2] = (float)x.z;
      if (state == 2) {
        float d = 0.f, gx, gy, gz;
        state = (collide_sample(f, x, false, d, gx, gy, gz) && d < margin) ? 1 : 0;
      }
      n_unresolved += state;
      prev = pj;
      q = x;
    }
  }
  moved_out[s] = n_moved;
  unresolved_out[s] = n_unresolved;
}

}  // namespace

extern "C" int hgs_strand_collide(void* stream, int K, const long long* offsets, long long P, const float* points, const float* phi,
                                  int nx, int ny, int nz, float ox, float oy, float oz, float inv_h, float margin, float skin, int iters,
                                  float* out_points, int* moved, int* unresolved) {
  if (K < 0 || P < 0) { hgs_set_error("hgs_strand_collide: bad sizes (%d strands, %lld points)", K, P); return 1; }
  if (iters < 1 || iters > 32) { hgs_set_error("hgs_strand_collide: iters = %d outside [1, 32]", iters); return 1; }
  if (!(margin >= 0.f) || !isfinite(margin) || !(skin >= 0.f) || !isfinite(skin)) {
    hgs_set_error("hgs_strand_collide: margin %g and skin %g must be finite and >= 0", (double)margin, (double)skin);
    return 1;
  }
  if (nx < 2 || ny < 2 || nz < 2 || nx > 1024 || ny > 1024 || nz > 1024) {
    hgs_set_error("hgs_strand_collide: a grid of %d x %d x %d nodes (2 to 1024 an axis)", nx, ny, nz);
    return 1;
  }
  if (!(inv_h > 0.f) || !isfinite(inv_h) || !isfinite(ox) || !isfinite(oy) || !isfinite(oz)) {
    hgs_set_error("hgs_strand_collide: origin (%g, %g, %g) and 1/h = %g must be finite, 1/h > 0", (double)ox, (double)oy, (double)oz,
                  (double)inv_h);
    return 1;
  }
  if (K == 0) return 0;
  if (!offsets || !phi || !moved || !unresolved || (P > 0 && (!points || !out_points))) {
    hgs_set_error("hgs_strand_collide: null argument");
    return 1;
  }
  if (P > 0 && out_points == points) { hgs_set_error("hgs_strand_collide: out_points must not alias points"); return 1; }
  const Field f = {phi, nx, ny, nz, ox, oy, oz, inv_h};
  hipLaunchKernelGGL(strand_collide_kernel, dim3((unsigned)((K + COLLIDE_BLOCK - 1) / COLLIDE_BLOCK)), dim3(COLLIDE_BLOCK), 0,
                     (hipStream_t)stream, K, offsets, P, points, f, margin, skin, iters, out_points, moved, unresolved);
  HGS_CHECK_LAUNCH();
  return 0;
}
