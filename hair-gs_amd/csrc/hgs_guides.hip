// hgs_guides.hip -- guide strands picked from an exported groom by Lloyd's k-means over the strands' sampled joints
// (hgs_guides_assign / hgs_guides_update / hgs_guides_pick; scene/strand_guides.py states the contract, its numpy path and the loop
// restatement in tests/guides_reference.py state the same thing).  gfx950, wave64.  Built with -ffp-contract=off: every operation
// below is rounded once, in the order written.  All arithmetic is float64 on the float32 points.
//
// The strands: N strands of M points each (points float32 [N*M][3]); strand i's feature is its S sampled points j_s =
// (s*(M-1)) / (S-1), s = 0 .. S-1, as doubles.  Centroids are float64 [K][S][3].
//
// The assignment is an N x K sweep: d2(i, k) from 0.0 over s in order, acc = acc + ((dx*dx + dy*dy) + dz*dz), and strand i takes the
// k smallest by (d2, k).  A workgroup of 4 wavefronts owns 64 * SP strands, and ALL FOUR wavefronts hold the same strands: they
// share the walk over k.  Centroids are staged through LDS as doubles in tiles; wavefront w takes the tile's entries (or groups of
// entries) w, w + 4, ..., every lane of a wavefront reads the same LDS address (a broadcast), and within a wavefront k ascends and a
// candidate replaces the best on strict <, so the smaller k stays in front among equals.  The four wavefronts' bests are combined
// through LDS by the explicit lexicographic rule (d2, then k), which reproduces the minimum over all k exactly.  The split gives a
// launch of 10^5 strands 4 x the wavefronts the strands alone would (one strand a lane fills 1563 of the part's 1024 SIMDs once).
//   S <= 16 (guides_assign_reg_kernel): a strand's 48 doubles live in registers, two strands a lane (96 doubles), so every centroid
//     coordinate read from LDS feeds two strands' arithmetic: 18 float64 operations per 24 bytes read.
//   16 < S <= 64 (guides_assign_lds_kernel): 96 or 192 doubles a strand do not fit beside the accumulators, so the workgroup's 64
//     strands live in LDS as the float32 they are, transposed -- feat[3s + c][lane], consecutive lanes consecutive words, no bank
//     conflict -- and are converted on the way in (exact).  One feature read feeds TK centroids' accumulators (4 for S <= 32, 2 above:
//     60 KB of LDS with the tile).
// The count of labels that changed against the previous assignment is one integer atomic add per wavefront (order-free); there are
// no float atomics in this file.
//
// hgs_guides_update: one wavefront per cluster, lanes over the 3S coordinates (up to three a lane), the members walked in ascending
// strand index through the member list (a stable sort of the labels), four members' loads in flight at a time, added in order.
// hgs_guides_pick: one wavefront per cluster, the member smallest by (dist2, i): lanes stride over the list, then a butterfly with
// the same lexicographic rule.
// Bounds: a strand is read only for 0 <= i < N with N*M <= n_points (checked on the host); j_s <= M - 1; a member list entry outside
// [0, N) and a cluster range outside [0, n_order] are skipped; tile and feature indices stay below their arrays' sizes by S <= bucket.
#include "hgs_common.h"

#include <math.h>

#define HGS_GUIDES_MAX_K 65536
#define HGS_GUIDES_MAX_S 64
#define GD_WAVES 4
#define GD_REG_S 16
#define GD_REG_SP 2
#define GD_REG_TILE 64

namespace {

__device__ __forceinline__ long long guides_joint(int s, int M, int S) { return ((long long)s * (M - 1)) / (S - 1); }

// the four wavefronts' bests of a strand -> its label and dist2, and the change against prev; `slot` indexes the strand in the workgroup
__device__ __forceinline__ void guides_finish(const double* cd, const int* ck, int per, int slot, long long i, int N, const int* __restrict__ status,
                                              const int* __restrict__ prev, int* __restrict__ label, double* __restrict__ dist2,
                                              int* __restrict__ changed, bool active) {
  bool differs = false;
  if (active && i < N) {
    double bd = HUGE_VAL;
    int bk = -1;
    if (status[i] == 0) {
#pragma unroll
      for (int w = 0; w < GD_WAVES; w++) {
        const double d = cd[w * per + slot];
        const int k = ck[w * per + slot];
        if (k >= 0 && (bk < 0 || d < bd || (d == bd && k < bk))) { bd = d; bk = k; }
      }
    }
    label[i] = bk;
    dist2[i] = bk < 0 ? HUGE_VAL : bd;
    differs = prev != nullptr && prev[i] != bk;
  }
  if (prev != nullptr) {                                                            // (uniform)
    const int n = __popcll(__ballot(differs));
    if (n > 0 && (threadIdx.x & (HGS_WAVE - 1)) == 0) atomicAdd(changed, n);
  }
}

// S <= 16: features in registers, SP strands a lane
template <int SP>
__global__ __launch_bounds__(256) void guides_assign_reg_kernel(int N, int M, int S, const float* __restrict__ points,
                                                                const int* __restrict__ status, int K, const double* __restrict__ cent,
                                                                const int* __restrict__ prev, int* __restrict__ label,
                                                                double* __restrict__ dist2, int* __restrict__ changed) {
  __shared__ double tile[GD_REG_TILE * 3 * GD_REG_S];                               // 24 KB; the combine reuses it
  const int lane = threadIdx.x & (HGS_WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long first = (long long)blockIdx.x * (HGS_WAVE * SP);
  const int D = 3 * S;
  double f[SP][3 * GD_REG_S];
#pragma unroll
  for (int p = 0; p < SP; p++) {
    const long long i = first + p * HGS_WAVE + lane;
    const bool live = i < N && status[i] == 0;
    const float* const base = points + 3 * (size_t)(live ? i : 0) * M;
#pragma unroll
    for (int s = 0; s < GD_REG_S; s++) {
      f[p][3 * s] = 0.0; f[p][3 * s + 1] = 0.0; f[p][3 * s + 2] = 0.0;
      if (s < S && live) {
        const float* const q = base + 3 * guides_joint(s, M, S);
        f[p][3 * s] = (double)q[0]; f[p][3 * s + 1] = (double)q[1]; f[p][3 * s + 2] = (double)q[2];
      }
    }
  }
  double bd[SP];
  int bk[SP];
#pragma unroll
  for (int p = 0; p < SP; p++) { bd[p] = HUGE_VAL; bk[p] = -1; }
  for (int base = 0; base < K; base += GD_REG_TILE) {
    const int m = K - base < GD_REG_TILE ? K - base : GD_REG_TILE;
    __syncthreads();                                                                // the previous tile has been read
    for (int e = threadIdx.x; e < m * D; e += 256) tile[e] = cent[(size_t)base * D + e];
    __syncthreads();
    for (int t = wave; t < m; t += GD_WAVES) {
      const double* const c = tile + t * D;
      double acc[SP];
#pragma unroll
      for (int p = 0; p < SP; p++) acc[p] = 0.0;
#pragma unroll
      for (int s = 0; s < GD_REG_S; s++) {
        if (s < S) {                                                                // (uniform; every index of f is a constant)
          const double cx = c[3 * s], cy = c[3 * s + 1], cz = c[3 * s + 2];
#pragma unroll
          for (int p = 0; p < SP; p++) {
            const double dx = f[p][3 * s] - cx, dy = f[p][3 * s + 1] - cy, dz = f[p][3 * s + 2] - cz;
            acc[p] = acc[p] + ((dx * dx + dy * dy) + dz * dz);
          }
        }
      }
#pragma unroll
      for (int p = 0; p < SP; p++) {
        if (acc[p] < bd[p]) { bd[p] = acc[p]; bk[p] = base + t; }
      }
    }
  }
  __syncthreads();                                                                  // the last tile has been read
  double* const cd = tile;                                                          // [4][64 SP]
  int* const ck = (int*)(tile + GD_WAVES * HGS_WAVE * SP);
#pragma unroll
  for (int p = 0; p < SP; p++) {
    cd[wave * (HGS_WAVE * SP) + p * HGS_WAVE + lane] = bd[p];
    ck[wave * (HGS_WAVE * SP) + p * HGS_WAVE + lane] = bk[p];
  }
  __syncthreads();
  const int slot = threadIdx.x;
  guides_finish(cd, ck, HGS_WAVE * SP, slot, first + slot, N, status, prev, label, dist2, changed, slot < HGS_WAVE * SP);
}

// 16 < S <= B: the workgroup's 64 strands in LDS as float32, transposed; TK centroids per feature read
template <int B, int TK>
__global__ __launch_bounds__(256) void guides_assign_lds_kernel(int N, int M, int S, const float* __restrict__ points,
                                                                const int* __restrict__ status, int K, const double* __restrict__ cent,
                                                                const int* __restrict__ prev, int* __restrict__ label,
                                                                double* __restrict__ dist2, int* __restrict__ changed) {
  constexpr int TILE = GD_WAVES * TK;
  __shared__ float feat[3 * B * HGS_WAVE];                                          // [3s + c][lane]
  __shared__ double tile[TILE * 3 * B];                                             // 12 KB; the combine reuses it
  const int lane = threadIdx.x & (HGS_WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long first = (long long)blockIdx.x * HGS_WAVE;
  const int D = 3 * S;
  for (int e = threadIdx.x; e < D * HGS_WAVE; e += 256) {
    const int d = e >> 6, q = e & (HGS_WAVE - 1);
    const long long i = first + q;
    float v = 0.f;
    if (i < N && status[i] == 0) v = points[3 * ((size_t)i * M + (size_t)guides_joint(d / 3, M, S)) + (d % 3)];
    feat[e] = v;
  }
  double bd = HUGE_VAL;
  int bk = -1;
  for (int base = 0; base < K; base += TILE) {
    const int m = K - base < TILE ? K - base : TILE;
    __syncthreads();                                                                // the features are in place; the previous tile has been read
    for (int e = threadIdx.x; e < m * D; e += 256) tile[e] = cent[(size_t)base * D + e];
    __syncthreads();
    const int t0 = wave * TK;
    if (t0 < m) {                                                                   // (uniform; rows from m on hold an earlier tile's values, computed and dropped)
      double acc[TK];
#pragma unroll
      for (int u = 0; u < TK; u++) acc[u] = 0.0;
      for (int s = 0; s < S; s++) {
        const double fx = (double)feat[(3 * s) * HGS_WAVE + lane], fy = (double)feat[(3 * s + 1) * HGS_WAVE + lane],
                     fz = (double)feat[(3 * s + 2) * HGS_WAVE + lane];
#pragma unroll
        for (int u = 0; u < TK; u++) {
          const double* const c = tile + (t0 + u) * D + 3 * s;
          const double dx = fx - c[0], dy = fy - c[1], dz = fz - c[2];
          acc[u] = acc[u] + ((dx * dx + dy * dy) + dz * dz);
        }
      }
#pragma unroll
      for (int u = 0; u < TK; u++) {
        if (t0 + u < m && acc[u] < bd) { bd = acc[u]; bk = base + t0 + u; }
      }
    }
  }
  __syncthreads();
  double* const cd = tile;                                                          // [4][64]
  int* const ck = (int*)(tile + GD_WAVES * HGS_WAVE);
  cd[wave * HGS_WAVE + lane] = bd;
  ck[wave * HGS_WAVE + lane] = bk;
  __syncthreads();
  const int slot = threadIdx.x;
  guides_finish(cd, ck, HGS_WAVE, slot, first + slot, N, status, prev, label, dist2, changed, slot < HGS_WAVE);
}

// one wavefront per cluster; lane l owns the coordinates l, l + 64, l + 128 of the 3S
__global__ __launch_bounds__(256) void guides_update_kernel(int N, int M, int S, const float* __restrict__ points, int K,
                                                            const long long* __restrict__ order, long long n_order,
                                                            const long long* __restrict__ start, double* __restrict__ cent,
                                                            int* __restrict__ count) {
  const int lane = threadIdx.x & (HGS_WAVE - 1);
  const int k = blockIdx.x * GD_WAVES + (int)(threadIdx.x >> 6);
  if (k >= K) return;                                                               // (the whole wavefront)
  long long a = start[k], b = start[k + 1];
  if (a < 0 || b < a || b > n_order) { a = 0; b = 0; }                              // (the list is the caller's duty; a range outside it counts as empty)
  const int D = 3 * S;
  bool valid[3];
  long long off[3];
  double acc[3];
#pragma unroll
  for (int r = 0; r < 3; r++) {
    const int d = lane + HGS_WAVE * r;
    valid[r] = d < D;
    off[r] = valid[r] ? 3 * guides_joint(d / 3, M, S) + (d % 3) : 0;
    acc[r] = 0.0;
  }
  int cnt = 0;
  for (long long q = a; q < b; q += 4) {
    long long id[4];
    float v[4][3];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      id[u] = q + u < b ? order[q + u] : -1;
      if (id[u] < 0 || id[u] >= N) id[u] = -1;
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const float* const base = points + 3 * (size_t)(id[u] < 0 ? 0 : id[u]) * M;
#pragma unroll
      for (int r = 0; r < 3; r++) v[u][r] = (id[u] >= 0 && valid[r]) ? base[off[r]] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      if (id[u] >= 0) {                                                             // (uniform)
#pragma unroll
        for (int r = 0; r < 3; r++) acc[r] = acc[r] + (double)v[u][r];
        cnt++;
      }
    }
  }
  if (cnt > 0) {
    const double n = (double)cnt;
#pragma unroll
    for (int r = 0; r < 3; r++) {
      if (valid[r]) cent[(size_t)k * D + lane + HGS_WAVE * r] = acc[r] / n;
    }
  }
  if (lane == 0) count[k] = cnt;
}

__device__ __forceinline__ bool guides_before(double d, long long i, double bd, long long bi) {
  return i >= 0 && (bi < 0 || d < bd || (d == bd && i < bi));
}

__global__ __launch_bounds__(256) void guides_pick_kernel(int N, int K, const long long* __restrict__ order, long long n_order,
                                                          const long long* __restrict__ start, const double* __restrict__ dist2,
                                                          long long* __restrict__ guide) {
  const int lane = threadIdx.x & (HGS_WAVE - 1);
  const int k = blockIdx.x * GD_WAVES + (int)(threadIdx.x >> 6);
  if (k >= K) return;                                                               // (the whole wavefront)
  long long a = start[k], b = start[k + 1];
  if (a < 0 || b < a || b > n_order) { a = 0; b = 0; }
  double bd = HUGE_VAL;
  long long bi = -1;
  for (long long q = a + lane; q < b; q += HGS_WAVE) {
    const long long i = order[q];
    if (i < 0 || i >= N) continue;
    const double d = dist2[i];
    if (guides_before(d, i, bd, bi)) { bd = d; bi = i; }
  }
#pragma unroll
  for (int o = HGS_WAVE / 2; o > 0; o >>= 1) {
    const double od = __shfl_xor(bd, o, HGS_WAVE);
    const long long oi = __shfl_xor(bi, o, HGS_WAVE);
    if (guides_before(od, oi, bd, bi)) { bd = od; bi = oi; }
  }
  if (lane == 0) guide[k] = bi;
}

int guides_check_strands(const char* who, int N, int M, int S, long long n_points) {
  if (N < 0 || n_points < 0) { hgs_set_error("%s: bad sizes (%d strands, %lld points)", who, N, n_points); return 1; }
  if (M < 2) { hgs_set_error("%s: M = %d (at least 2 points per strand)", who, M); return 1; }
  if (S < 2 || S > HGS_GUIDES_MAX_S || S > M) {
    hgs_set_error("%s: S = %d samples outside [2, min(%d, M = %d)]", who, S, HGS_GUIDES_MAX_S, M); return 1;
  }
  if ((long long)N * M > n_points) {
    hgs_set_error("%s: N M = %lld points for %d strands of %d, the point array holds %lld", who, (long long)N * M, N, M, n_points); return 1;
  }
  return 0;
}

int guides_check_k(const char* who, int K) {
  if (K < 1 || K > HGS_GUIDES_MAX_K) { hgs_set_error("%s: K = %d clusters outside [1, %d]", who, K, HGS_GUIDES_MAX_K); return 1; }
  return 0;
}

}  // namespace

extern "C" int hgs_guides_assign(void* stream, int N, int M, int S, long long n_points, const float* points, const int* status, int K,
                                 const double* centroids, const int* prev_label, int* label, double* dist2, int* changed) {
  if (guides_check_strands("hgs_guides_assign", N, M, S, n_points) || guides_check_k("hgs_guides_assign", K)) return 1;
  if (N == 0) return 0;
  if (!points || !status || !centroids || !label || !dist2 || (prev_label && !changed)) {
    hgs_set_error("hgs_guides_assign: null argument"); return 1;
  }
  if ((const void*)label == (const void*)prev_label || (const void*)label == (const void*)status) {
    hgs_set_error("hgs_guides_assign: label must not alias prev_label or status"); return 1;
  }
  hipStream_t s = (hipStream_t)stream;
  if (S <= GD_REG_S) {
    const unsigned blocks = (unsigned)(((long long)N + HGS_WAVE * GD_REG_SP - 1) / (HGS_WAVE * GD_REG_SP));
    hipLaunchKernelGGL(guides_assign_reg_kernel<GD_REG_SP>, dim3(blocks), dim3(256), 0, s, N, M, S, points, status, K, centroids, prev_label,
                       label, dist2, changed);
  } else {
    const unsigned blocks = (unsigned)(((long long)N + HGS_WAVE - 1) / HGS_WAVE);
    if (S <= 32) {
      hipLaunchKernelGGL((guides_assign_lds_kernel<32, 4>), dim3(blocks), dim3(256), 0, s, N, M, S, points, status, K, centroids, prev_label,
                         label, dist2, changed);
    } else {
      hipLaunchKernelGGL((guides_assign_lds_kernel<64, 2>), dim3(blocks), dim3(256), 0, s, N, M, S, points, status, K, centroids, prev_label,
                         label, dist2, changed);
    }
  }
  HGS_CHECK_LAUNCH();
  return 0;
}

extern "C" int hgs_guides_update(void* stream, int N, int M, int S, long long n_points, const float* points, int K, const long long* order,
                                 long long n_order, const long long* start, double* centroids, int* count) {
  if (guides_check_strands("hgs_guides_update", N, M, S, n_points) || guides_check_k("hgs_guides_update", K)) return 1;
  if (n_order < 0 || n_order > N) { hgs_set_error("hgs_guides_update: a member list of %lld entries for %d strands", n_order, N); return 1; }
  if (!start || !centroids || !count || (n_order > 0 && (!order || !points))) { hgs_set_error("hgs_guides_update: null argument"); return 1; }
  hipLaunchKernelGGL(guides_update_kernel, dim3((unsigned)((K + GD_WAVES - 1) / GD_WAVES)), dim3(256), 0, (hipStream_t)stream, N, M, S, points, K,
                     order, n_order, start, centroids, count);
  HGS_CHECK_LAUNCH();
  return 0;
}

extern "C" int hgs_guides_pick(void* stream, int N, int K, const long long* order, long long n_order, const long long* start,
                               const double* dist2, long long* guide) {
  if (N < 0) { hgs_set_error("hgs_guides_pick: bad sizes (%d strands)", N); return 1; }
  if (guides_check_k("hgs_guides_pick", K)) return 1;
  if (n_order < 0 || n_order > N) { hgs_set_error("hgs_guides_pick: a member list of %lld entries for %d strands", n_order, N); return 1; }
  if (!start || !guide || (n_order > 0 && (!order || !dist2))) { hgs_set_error("hgs_guides_pick: null argument"); return 1; }
  hipLaunchKernelGGL(guides_pick_kernel, dim3((unsigned)((K + GD_WAVES - 1) / GD_WAVES)), dim3(256), 0, (hipStream_t)stream, N, K, order, n_order,
                     start, dist2, guide);
  HGS_CHECK_LAUNCH();
  return 0;
}
