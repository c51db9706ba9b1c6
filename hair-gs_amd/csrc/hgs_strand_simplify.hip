// hgs_strand_simplify.hip -- exported strands simplified to a tolerance (hgs_strand_simplify; scene/strand_simplify.py states the
// contract, its numpy path and the recursive restatement in tests/simplify_reference.py state the same thing).  gfx950, wave64.  Built
// with -ffp-contract=off: every operation below is rounded once, in the order written.  All arithmetic is float64 on the float32
// points, dot(u, v) = (u0*v0 + u1*v1) + u2*v2.
//
// strand_simplify_kernel: one wavefront per strand, W = blockDim.x / 64 wavefronts per workgroup (4, 2 or 1), each with its own slice
//   of the dynamic LDS (hgs_strand_smooth.hip's idiom), `slot` = the launch's longest eligible strand:
//     x0 | x1 | x2 | d2   float64 [slot] each    the strand, and this round's deviation of every candidate
//     best                uint64  [slot]         per interval, at its LEFT end joint: the largest d2 of the round, as bits
//     kept                uint64  [16]           the keep flags, one bit a joint
//     first | left        int32   [slot] each    per interval, at its left end joint: the smallest joint with that d2;
//                                                per joint: the left end of its interval, or -1 where it is no candidate
//   which is 48 * slot + 128 bytes.  The wavefront loads its strand once (lanes take 64 joints at a time, consecutive lanes
//   consecutive joints), converts it to float64 in LDS and runs Douglas-Peucker round by round: all the intervals of one recursion
//   depth at once, which keeps the joints the recursion keeps (the contract says why).  A round:
//     0. best = 0, first = INT_MAX for every joint.
//     1. chunk by chunk, a lane owns joint j.  Where j is not kept, its interval's ends are the nearest kept joints below and above
//        it: bit scans of the chunk's own word of `kept`, and, where the word has no such bit, the last kept joint of the chunks
//        before (carried along) and the first of the chunks after (a wavefront-uniform scan of the words).  The lane forms d2; where
//        d2 > tol2 it is a candidate: d2 and the left end are stored, and ds_max_u64 puts its bits into best[left] -- a double that is
//        not negative orders as its bits do, so this is the exact maximum, whatever the order of arrival.  No candidate in any
//        chunk (a ballot): the strand is done.
//     2. every candidate whose bits equal best[left] puts j into first[left] with ds_min_i32: the smallest j among equals.
//     3. chunk by chunk, the candidates with first[left] == j are the round's winners; their ballot is or-ed into the chunk's word.
//   An interval may begin and end in any chunk: nothing above depends on where.  Integer atomics only, and the result does not depend
//   on their order: bitwise reproducible.  The loop runs at most n - 2 rounds (every round but the last keeps a joint).
//   Synchronisation is within the wavefront only (strands differ in length, and a wavefront past K leaves at once: there is no
//   __syncthreads in this file); wave_lds_fence() stands between the passes.
//   SHORT / LONG are decided from the offsets, NONFINITE by a ballot after the load; such a strand gets keep = 1 for every joint.
//   Bounds: a strand is touched only where 0 <= a <= b <= P; j < n <= slot indexes LDS; an interval's ends are kept joints of the
//   strand (joint 0 and joint n - 1 always are), so 0 <= left < j < right <= n - 1.
#include "hgs_common.h"

#include <limits.h>
#include <math.h>

#define HGS_SIMPLIFY_MAX_JOINTS 1024
#define HGS_SIMPLIFY_LDS_BYTES 65536
#define HGS_SIMPLIFY_WORDS (HGS_SIMPLIFY_MAX_JOINTS / 64)
#define HGS_SIMPLIFY_SLICE(slot) ((size_t)48 * (size_t)(slot) + 8 * HGS_SIMPLIFY_WORDS)

namespace {

enum { SI_OK = 0, SI_SHORT = 1, SI_LONG = 2, SI_NONFINITE = 3 };

__device__ __forceinline__ void wave_lds_fence() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

__device__ __forceinline__ bool finite32(float v) { return fabsf(v) < __builtin_inff(); }        // (false for a NaN)

// a value every lane holds alike, moved to scalar registers
__device__ __forceinline__ unsigned long long uniform64(unsigned long long v) {
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
  return ((unsigned long long)hi << 32) | lo;
}

__device__ __forceinline__ void keep_all(unsigned char* __restrict__ kp, long long n, int lane) {
  for (long long i = lane; i < n; i += HGS_WAVE) kp[i] = 1;
}

__global__ __launch_bounds__(256) void strand_simplify_kernel(int K, const long long* __restrict__ offsets, long long P,
                                                              const float* __restrict__ points, int slot, double tol2,
                                                              unsigned char* __restrict__ keep, int* __restrict__ status,
                                                              int* __restrict__ rounds) {
  extern __shared__ double simplify_lds[];
  const int lane = threadIdx.x & (HGS_WAVE - 1), wave = threadIdx.x >> 6;
  const long long s = (long long)blockIdx.x * (blockDim.x >> 6) + wave;
  if (s >= K) return;                                                              // (the whole wavefront)
  const long long a0 = offsets[s], b0 = offsets[s + 1];
  // (the offsets are the caller's duty; a range that is not inside the P points counts as a strand without joints)
  const long long nn = (a0 >= 0 && b0 >= a0 && b0 <= P) ? b0 - a0 : 0;
  const float* const p = points + 3 * (size_t)(nn > 0 ? a0 : 0);
  unsigned char* const kp = keep + (size_t)(nn > 0 ? a0 : 0);
  if (nn < 3 || nn > slot) {                                                       // (slot <= 1024; a strand the slice cannot hold is LONG)
    keep_all(kp, nn, lane);
    if (lane == 0) { status[s] = nn < 3 ? SI_SHORT : SI_LONG; rounds[s] = 0; }
    return;
  }
  const int n = (int)nn;
  double* const X0 = simplify_lds + (size_t)wave * (HGS_SIMPLIFY_SLICE(slot) / sizeof(double));
  double* const X1 = X0 + slot;
  double* const X2 = X1 + slot;
  double* const D = X2 + slot;
  unsigned long long* const BEST = (unsigned long long*)(D + slot);
  unsigned long long* const KEPT = BEST + slot;
  int* const FIRST = (int*)(KEPT + HGS_SIMPLIFY_WORDS);
  int* const LEFT = FIRST + slot;
  // the load: float32 -> float64 in LDS
  bool bad = false;
  for (int j = lane; j < n; j += HGS_WAVE) {
    const float v0 = p[3 * j], v1 = p[3 * j + 1], v2 = p[3 * j + 2];
    bad = bad || !(finite32(v0) && finite32(v1) && finite32(v2));
    X0[j] = (double)v0; X1[j] = (double)v1; X2[j] = (double)v2;
  }
  if (__ballot(bad) != 0ull) {                                                     // (every lane went through the loop above)
    keep_all(kp, nn, lane);
    if (lane == 0) { status[s] = SI_NONFINITE; rounds[s] = 0; }
    return;
  }
  const int chunks = (n + HGS_WAVE - 1) >> 6;
  if (lane < HGS_SIMPLIFY_WORDS) {                                                 // the two end joints are kept
    unsigned long long w = lane == 0 ? 1ull : 0ull;
    if (lane == ((n - 1) >> 6)) w |= 1ull << ((n - 1) & 63);
    KEPT[lane] = w;
  }
  wave_lds_fence();
  int depth = 0;
  for (int r = 0; r < n - 2; r++) {
    for (int j = lane; j < n; j += HGS_WAVE) { BEST[j] = 0ull; FIRST[j] = INT_MAX; }
    wave_lds_fence();
    // 1. the deviations, and every interval's largest
    unsigned long long any = 0ull;
    int below = 0;                                                                 // the last kept joint of the chunks before this one
    for (int c = 0; c < chunks; c++) {
      const unsigned long long w = uniform64(KEPT[c]);
      int above = n - 1;                                                           // the first kept joint of the chunks after this one
      for (int cc = c + 1; cc < chunks; cc++) {
        const unsigned long long v = uniform64(KEPT[cc]);
        if (v != 0ull) { above = cc * HGS_WAVE + __ffsll((long long)v) - 1; break; }
      }
      const int j = c * HGS_WAVE + lane;
      bool cand = false;
      if (j < n) {
        int left = -1;
        if (!((w >> lane) & 1ull)) {
          const unsigned long long lo = w & ((1ull << lane) - 1ull), hi = w & ~((2ull << lane) - 1ull);     // (2ull << 63 is 0: hi = 0)
          const int i = lo != 0ull ? c * HGS_WAVE + 63 - __clzll((long long)lo) : below;
          const int k = hi != 0ull ? c * HGS_WAVE + __ffsll((long long)hi) - 1 : above;
          const double ax = X0[i], ay = X1[i], az = X2[i];
          const double abx = X0[k] - ax, aby = X1[k] - ay, abz = X2[k] - az;
          const double apx = X0[j] - ax, apy = X1[j] - ay, apz = X2[j] - az;
          const double L2 = dot3(abx, aby, abz, abx, aby, abz);
          double t = L2 > 0.0 ? dot3(apx, apy, apz, abx, aby, abz) / L2 : 0.0;
          t = t < 0.0 ? 0.0 : t;
          t = t > 1.0 ? 1.0 : t;
          const double qx = apx - t * abx, qy = apy - t * aby, qz = apz - t * abz;
          const double d2 = dot3(qx, qy, qz, qx, qy, qz);
          cand = d2 > tol2;
          if (cand) {
            left = i;
            D[j] = d2;
            atomicMax(&BEST[i], (unsigned long long)__double_as_longlong(d2));
          }
        }
        LEFT[j] = left;
      }
      any |= __ballot(cand);
      if (w != 0ull) below = c * HGS_WAVE + 63 - __clzll((long long)w);
    }
    if (any == 0ull) break;                                                        // (wavefront-uniform)
    wave_lds_fence();
    // 2. the smallest joint among an interval's equals
    for (int j = lane; j < n; j += HGS_WAVE) {
      const int i = LEFT[j];
      if (i >= 0 && (unsigned long long)__double_as_longlong(D[j]) == BEST[i]) atomicMin(&FIRST[i], j);
    }
    wave_lds_fence();
    // 3. the winners are kept
    for (int c = 0; c < chunks; c++) {
      const int j = c * HGS_WAVE + lane;
      bool win = false;
      if (j < n) {
        const int i = LEFT[j];
        win = i >= 0 && FIRST[i] == j;
      }
      const unsigned long long m = __ballot(win);
      if (lane == 0 && m != 0ull) KEPT[c] |= m;
    }
    wave_lds_fence();
    depth++;
  }
  for (int c = 0; c < chunks; c++) {
    const int j = c * HGS_WAVE + lane;
    const unsigned long long w = KEPT[c];
    if (j < n) kp[j] = (unsigned char)((w >> lane) & 1ull);
  }
  if (lane == 0) { status[s] = SI_OK; rounds[s] = depth; }
}

}  // namespace

extern "C" int hgs_strand_simplify(void* stream, int K, const long long* offsets, long long P, const float* points, int max_joints, double tol,
                                   unsigned char* keep, int* status, int* rounds) {
  if (K < 0 || P < 0) { hgs_set_error("hgs_strand_simplify: bad sizes (%d strands, %lld points)", K, P); return 1; }
  if (!(tol >= 0.0) || !isfinite(tol)) { hgs_set_error("hgs_strand_simplify: tol = %g (finite and >= 0)", tol); return 1; }
  if (max_joints != 0 && (max_joints < 3 || max_joints > HGS_SIMPLIFY_MAX_JOINTS)) {
    hgs_set_error("hgs_strand_simplify: max_joints = %d (3 to %d, the launch's longest strand of that many joints; 0 where it has none)",
                  max_joints, HGS_SIMPLIFY_MAX_JOINTS);
    return 1;
  }
  if (K == 0) return 0;
  if (!offsets || !status || !rounds || (P > 0 && (!points || !keep))) {
    hgs_set_error("hgs_strand_simplify: null argument");
    return 1;
  }
  if ((const void*)status == (const void*)rounds || (const void*)status == (const void*)offsets || (const void*)rounds == (const void*)offsets ||
      (P > 0 && ((const void*)keep == (const void*)points || (const void*)keep == (const void*)offsets || (const void*)keep == (const void*)status ||
                 (const void*)keep == (const void*)rounds || (const void*)status == (const void*)points || (const void*)rounds == (const void*)points))) {
    hgs_set_error("hgs_strand_simplify: keep, status and rounds must not alias each other or an input"); return 1;
  }
  const double tol2 = tol * tol;                                                   // formed once
  // W wavefronts a workgroup: the largest of 4, 2, 1 whose slices fit 64 KB (1024 joints: 48.1 KB)
  const size_t slice = HGS_SIMPLIFY_SLICE(max_joints);
  int W = 4;
  while (W > 1 && (size_t)W * slice > HGS_SIMPLIFY_LDS_BYTES) W >>= 1;
  const unsigned blocks = (unsigned)(((long long)K + W - 1) / W);
  hipLaunchKernelGGL(strand_simplify_kernel, dim3(blocks), dim3((unsigned)(HGS_WAVE * W)), (size_t)W * slice, (hipStream_t)stream, K, offsets,
                     P, points, max_joints, tol2, keep, status, rounds);
  HGS_CHECK_LAUNCH();
  return 0;
}
