// hgs_strand_smooth.hip -- exported strands smoothed without shrinking them (hgs_strand_smooth; scene/strand_smooth.py states the
// contract, its numpy path and the loop restatement in tests/smooth_reference.py state the same thing).  gfx950, wave64.  Built with
// -ffp-contract=off: every operation below is rounded once, in the order written.  All arithmetic is float64 on the float32 points,
// dot(u, v) = (u0*v0 + u1*v1) + u2*v2, results rounded once to float32.
//
// strand_smooth_kernel: one wavefront per strand, W = blockDim.x / 64 wavefronts per workgroup (4, 2 or 1), each with its own slice
//   of the dynamic LDS: five float64 rows of `slot` entries, x0 | x1 | x2 | a | b, `slot` the launch's longest eligible strand.  The
//   wavefront loads its strand once (lanes take 64 joints at a time, consecutive lanes consecutive joints), converts it to float64
//   in LDS, computes a_j / b_j once, runs all the sweeps out of LDS and writes the float32 result.
//   A sweep is IN PLACE, chunk by chunk: the lanes of a chunk read x_{j-1}, x_j, x_{j+1} (x_{j+1} of the chunk's last lane belongs to
//   the next chunk, which this sweep has not touched), every lane also reads the chunk's last joint (one address, a broadcast), a
//   fence, and then the lanes write x'_j.  Lane 0 of the next chunk takes its x_{j-1} from that register, not from LDS, where the
//   value of sweep t + 1 stands by now: Jacobi at every chunk edge.  The strand's two end joints are never written.
//   Synchronisation is within the wavefront only (strands differ in length, and a wavefront past K leaves at once: there is no
//   __syncthreads in this file).  wave_lds_fence() -- s_waitcnt lgkmcnt(0) with a memory clobber, the pattern of hgs_binning.hip --
//   stands between a chunk's reads and its writes and after its writes: the clobber keeps the compiler from moving an LDS access
//   across it, the wait keeps the hardware from having one outstanding across it.
//   SHORT / LONG are decided from the offsets, NONFINITE by a ballot after the load; such a strand is copied, bits and all.  No
//   atomics: clamped[s] is a sum of ballot counts.  Bitwise reproducible.
//   Bounds: a strand is touched only where 0 <= a <= b <= P; j < n <= slot indexes LDS; x[j + 1] is read only for j <= n - 2.
#include "hgs_common.h"

#include <math.h>

#define HGS_SMOOTH_MAX_JOINTS 1024
#define HGS_SMOOTH_MAX_ITERS 256
#define HGS_SMOOTH_LDS_BYTES 65536
#define HGS_SMOOTH_ROWS 5

namespace {

enum { SM_SMOOTHED = 0, SM_SHORT = 1, SM_LONG = 2, SM_NONFINITE = 3 };

__device__ __forceinline__ void wave_lds_fence() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

__device__ __forceinline__ bool finite32(float v) { return fabsf(v) < __builtin_inff(); }        // (false for a NaN)

__device__ __forceinline__ void copy_strand(const float* __restrict__ p, float* __restrict__ o, long long n, int lane) {
  for (long long i = lane; i < 3 * n; i += HGS_WAVE) o[i] = p[i];
}

__global__ __launch_bounds__(256) void strand_smooth_kernel(int K, const long long* __restrict__ offsets, long long P,
                                                            const float* __restrict__ points, int slot, int iters, double lam, double mu,
                                                            int has_max, double max_move, float* __restrict__ out_points,
                                                            int* __restrict__ status, int* __restrict__ clamped) {
  extern __shared__ double smooth_lds[];
  const int lane = threadIdx.x & (HGS_WAVE - 1), wave = threadIdx.x >> 6;
  const long long s = (long long)blockIdx.x * (blockDim.x >> 6) + wave;
  if (s >= K) return;                                                              // (the whole wavefront)
  const long long a0 = offsets[s], b0 = offsets[s + 1];
  // (the offsets are the caller's duty; a range that is not inside the P points counts as a strand without joints)
  const long long nn = (a0 >= 0 && b0 >= a0 && b0 <= P) ? b0 - a0 : 0;
  const float* const p = points + 3 * (size_t)(nn > 0 ? a0 : 0);
  float* const o = out_points + 3 * (size_t)(nn > 0 ? a0 : 0);
  if (nn < 3 || nn > slot) {                                                       // (slot <= 1024; a strand the slice cannot hold is LONG)
    copy_strand(p, o, nn, lane);
    if (lane == 0) { status[s] = nn < 3 ? SM_SHORT : SM_LONG; clamped[s] = 0; }
    return;
  }
  const int n = (int)nn;
  double* const X0 = smooth_lds + (size_t)wave * HGS_SMOOTH_ROWS * slot;
  double* const X1 = X0 + slot;
  double* const X2 = X1 + slot;
  double* const A = X2 + slot;
  double* const B = A + slot;
  // the load: float32 -> float64 in LDS
  bool bad = false;
  for (int j = lane; j < n; j += HGS_WAVE) {
    const float v0 = p[3 * j], v1 = p[3 * j + 1], v2 = p[3 * j + 2];
    bad = bad || !(finite32(v0) && finite32(v1) && finite32(v2));
    X0[j] = (double)v0; X1[j] = (double)v1; X2[j] = (double)v2;
  }
  if (__ballot(bad) != 0ull) {                                                     // (every lane went through the loop above)
    copy_strand(p, o, nn, lane);
    if (lane == 0) { status[s] = SM_NONFINITE; clamped[s] = 0; }
    return;
  }
  wave_lds_fence();
  // a_j, b_j of the inner joints, from the original segment lengths
  for (int j = lane; j < n; j += HGS_WAVE) {
    if (j >= 1 && j <= n - 2) {
      const double c0 = X0[j], c1 = X1[j], c2 = X2[j];
      const double d0 = c0 - X0[j - 1], d1 = c1 - X1[j - 1], d2 = c2 - X2[j - 1];  // e_{j-1} = p_j - p_{j-1}
      const double f0 = X0[j + 1] - c0, f1 = X1[j + 1] - c1, f2 = X2[j + 1] - c2;  // e_j = p_{j+1} - p_j
      const double lm = sqrt(dot3(d0, d1, d2, d0, d1, d2)), lc = sqrt(dot3(f0, f1, f2, f0, f1, f2));
      const double sj = lm + lc;
      const bool pos = sj > 0.0;
      A[j] = pos ? lc / sj : 0.5;
      B[j] = pos ? lm / sj : 0.5;
    }
  }
  wave_lds_fence();
  // the sweeps
  const int per = mu == 0.0 ? 1 : 2;
  for (int t = 0; t < iters * per; t++) {
    const double f = (per == 2 && (t & 1)) ? mu : lam;
    double k0 = 0.0, k1 = 0.0, k2 = 0.0;                                           // sweep t's joint in front of the chunk
    for (int base = 0; base < n; base += HGS_WAVE) {
      const int j = base + lane;
      const bool inner = j >= 1 && j <= n - 2;
      double r0 = 0.0, r1 = 0.0, r2 = 0.0;
      if (inner) {
        const bool carried = lane == 0;                                            // (j >= 1 on lane 0: base > 0)
        const double m0 = carried ? k0 : X0[j - 1], m1 = carried ? k1 : X1[j - 1], m2 = carried ? k2 : X2[j - 1];
        const double c0 = X0[j], c1 = X1[j], c2 = X2[j];
        const double a = A[j], b = B[j];
        r0 = c0 + f * ((a * m0 + b * X0[j + 1]) - c0);
        r1 = c1 + f * ((a * m1 + b * X1[j + 1]) - c1);
        r2 = c2 + f * ((a * m2 + b * X2[j + 1]) - c2);
      }
      const int last = min(base + HGS_WAVE - 1, n - 1);
      k0 = X0[last]; k1 = X1[last]; k2 = X2[last];
      wave_lds_fence();                                                            // every read of the chunk is in registers
      if (inner) { X0[j] = r0; X1[j] = r1; X2[j] = r2; }
      wave_lds_fence();
    }
  }
  // the clamp against the original points, and the float32 result
  int held = 0;
  for (int base = 0; base < n; base += HGS_WAVE) {
    const int j = base + lane;
    bool hit = false;
    if (j < n) {
      const float v0 = p[3 * j], v1 = p[3 * j + 1], v2 = p[3 * j + 2];
      if (j >= 1 && j <= n - 2) {
        double x0 = X0[j], x1 = X1[j], x2 = X2[j];
        if (has_max) {
          const double q0 = (double)v0, q1 = (double)v1, q2 = (double)v2;
          const double u0 = x0 - q0, u1 = x1 - q1, u2 = x2 - q2;
          const double du = sqrt(dot3(u0, u1, u2, u0, u1, u2));
          if (du > max_move) {
            const double g = max_move / du;
            x0 = q0 + g * u0; x1 = q1 + g * u1; x2 = q2 + g * u2;
            hit = true;
          }
        }
        o[3 * j] = (float)x0; o[3 * j + 1] = (float)x1; o[3 * j + 2] = (float)x2;
      } else {
        o[3 * j] = v0; o[3 * j + 1] = v1; o[3 * j + 2] = v2;                       // the two end joints: their input bits
      }
    }
    held += __popcll(__ballot(hit));
  }
  if (lane == 0) { status[s] = SM_SMOOTHED; clamped[s] = held; }
}

}  // namespace

extern "C" int hgs_strand_smooth(void* stream, int K, const long long* offsets, long long P, const float* points, int max_joints, int iters,
                                 double lam, double mu, int has_max_move, double max_move, float* out_points, int* status, int* clamped) {
  if (K < 0 || P < 0 || max_joints < 0 || max_joints > HGS_SMOOTH_MAX_JOINTS) {
    hgs_set_error("hgs_strand_smooth: bad sizes (%d strands, %lld points, max_joints = %d of at most %d)", K, P, max_joints,
                  HGS_SMOOTH_MAX_JOINTS);
    return 1;
  }
  if (iters < 1 || iters > HGS_SMOOTH_MAX_ITERS) {
    hgs_set_error("hgs_strand_smooth: iters = %d outside [1, %d]", iters, HGS_SMOOTH_MAX_ITERS); return 1;
  }
  if (!(lam > 0.0) || !(lam <= 1.0)) { hgs_set_error("hgs_strand_smooth: lam = %g (above 0, at most 1)", lam); return 1; }
  if (!(mu == 0.0 || (mu >= -1.0 && mu < -lam))) {
    hgs_set_error("hgs_strand_smooth: mu = %g (0, or from -1 to below -lam = %g)", mu, -lam); return 1;
  }
  if (!(fabs((1.0 - 2.0 * lam) * (1.0 - 2.0 * mu)) <= 1.0)) {
    hgs_set_error("hgs_strand_smooth: lam = %g with mu = %g: |(1 - 2 lam)(1 - 2 mu)| is above 1, the shortest waves would grow", lam, mu);
    return 1;
  }
  if (has_max_move && (!(max_move > 0.0) || !isfinite(max_move))) {
    hgs_set_error("hgs_strand_smooth: max_move = %g (finite and > 0, or has_max_move = 0 for none)", max_move); return 1;
  }
  if (K == 0) return 0;
  if (!offsets || !status || !clamped || (P > 0 && (!points || !out_points))) {
    hgs_set_error("hgs_strand_smooth: null argument");
    return 1;
  }
  if (P > 0 && ((const void*)out_points == (const void*)points || (const void*)out_points == (const void*)offsets)) {
    hgs_set_error("hgs_strand_smooth: out_points must not alias points or offsets"); return 1;
  }
  if ((const void*)status == (const void*)clamped || (const void*)status == (const void*)offsets || (const void*)clamped == (const void*)offsets ||
      (P > 0 && ((const void*)status == (const void*)points || (const void*)clamped == (const void*)points ||
                 (const void*)status == (const void*)out_points || (const void*)clamped == (const void*)out_points))) {
    hgs_set_error("hgs_strand_smooth: status and clamped must not alias each other or another argument"); return 1;
  }
  // W wavefronts a workgroup: the largest of 4, 2, 1 whose slices fit 64 KB (5 rows of max_joints float64 each; 1024 joints: 40 KB)
  const size_t slice = (size_t)HGS_SMOOTH_ROWS * sizeof(double) * (size_t)max_joints;
  int W = 4;
  while (W > 1 && (size_t)W * slice > HGS_SMOOTH_LDS_BYTES) W >>= 1;
  const unsigned blocks = (unsigned)(((long long)K + W - 1) / W);
  hipLaunchKernelGGL(strand_smooth_kernel, dim3(blocks), dim3((unsigned)(HGS_WAVE * W)), (size_t)W * slice, (hipStream_t)stream, K, offsets,
                     P, points, max_joints, iters, lam, mu, has_max_move, max_move, out_points, status, clamped);
  HGS_CHECK_LAUNCH();
  return 0;
}
