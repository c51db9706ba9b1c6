// hgs_groom.hip -- a dense groom interpolated from the trained strands, used as guides (scene/groom.py, export_strands.py
// --interpolate): hgs_groom_neighbours / hgs_groom_blend.  gfx950, wave64.
//
// The contract (one definition for the numpy path, these kernels and the tests; scene/groom.py states it in full): K guides of M
// points (float32 gp[K][M][3], attributes ga[K][M][C]), N roots (float64).  Root n takes the k candidates smallest by (d2, g) among the
// guides whose d2 = (dx*dx + dy*dy) + dz*dz to its root is finite and <= max_d2; rank 0 is kept, rank i >= 1 is kept iff both chords
// (last point - first point) have a length > 0 and (cix*c0x + ciy*c0y) + ciz*c0z >= cos_max * (len_i * len_0); d2_0 == 0 cuts the list
// to rank 0; w_i = d2_0 / d2_i (w_0 = 1), W = their sum in rank order from 0.0, w^_i = w_i / W.  Point j of a kept root is
// root + sum_i w^_i (gp[g_i][j] - gp[g_i][0]), attributes sum_i w^_i ga[g_i][j], both added up in rank order from 0.0.  Every operation
// is float64 on the given inputs, one rounding each (this file is built with -ffp-contract=off); results are rounded once to float32.
//
// The search is brute force: one lane per root walks all guide roots in ascending g, staged through LDS as doubles in tiles of 256
// (every lane reads the same address: broadcasts).  The k-best list lives in registers: k is a template parameter and every list
// index is a compile-time constant.  Insertion is on strict <, so among equal d2 the smaller g, which came first, stays in front.
#include "hgs_common.h"

namespace {

#define GROOM_TILE 256

struct Chord { double x, y, z, len; };

__device__ __forceinline__ Chord groom_chord(const float* __restrict__ gp, int M, int g) {
  const float* const a = gp + (size_t)g * M * 3;
  const float* const b = a + (size_t)(M - 1) * 3;
  Chord c;
  c.x = (double)b[0] - (double)a[0]; c.y = (double)b[1] - (double)a[1]; c.z = (double)b[2] - (double)a[2];
  c.len = sqrt((c.x * c.x + c.y * c.y) + c.z * c.z);
  return c;
}

// one lane per root, 256 roots per workgroup
template <int KK>
__global__ __launch_bounds__(256) void groom_neighbours_kernel(int N, const double* __restrict__ roots, int K, int M,
                                                               const float* __restrict__ gp, double max_d2, double cos_max,
                                                               int* __restrict__ idx, double* __restrict__ d2_out, double* __restrict__ w_out,
                                                               int* __restrict__ count) {
  __shared__ double tile[GROOM_TILE * 3];
  const int n = blockIdx.x * 256 + threadIdx.x;
  const bool live = n < N;
  double rx = 0.0, ry = 0.0, rz = 0.0;
  if (live) { rx = roots[3 * (size_t)n]; ry = roots[3 * (size_t)n + 1]; rz = roots[3 * (size_t)n + 2]; }
  double bd[KK];
  int bi[KK];
#pragma unroll
  for (int s = 0; s < KK; s++) { bd[s] = HUGE_VAL; bi[s] = -1; }
  for (int base = 0; base < K; base += GROOM_TILE) {
    const int m = K - base < GROOM_TILE ? K - base : GROOM_TILE;
    __syncthreads();                                   // the previous tile has been read
    if ((int)threadIdx.x < m) {
      const float* const p = gp + (size_t)(base + threadIdx.x) * M * 3;
      tile[3 * threadIdx.x] = (double)p[0]; tile[3 * threadIdx.x + 1] = (double)p[1]; tile[3 * threadIdx.x + 2] = (double)p[2];
    }
    __syncthreads();
    if (!live) continue;
    for (int t = 0; t < m; t++) {
      const double dx = rx - tile[3 * t], dy = ry - tile[3 * t + 1], dz = rz - tile[3 * t + 2];
      const double d2 = (dx * dx + dy * dy) + dz * dz;
      // (bd starts at +inf: a NaN or an infinite d2 is never < it)
      if (d2 <= max_d2 && d2 < bd[KK - 1]) {
        const int g = base + t;
#pragma unroll
        for (int s = KK - 1; s >= 1; s--) {
          const bool up = d2 < bd[s - 1], here = d2 < bd[s];
          bd[s] = up ? bd[s - 1] : (here ? d2 : bd[s]);
          bi[s] = up ? bi[s - 1] : (here ? g : bi[s]);
        }
        if (d2 < bd[0]) { bd[0] = d2; bi[0] = g; }
      }
    }
  }
  if (!live) return;
  // the parting rule, the weights and the compacted rows
  bool keep[KK];
  double w[KK];
  Chord c0 = {0.0, 0.0, 0.0, 0.0};
  if (bi[0] >= 0) c0 = groom_chord(gp, M, bi[0]);
  double W = 0.0;
  int cnt = 0;
#pragma unroll
  for (int s = 0; s < KK; s++) {
    keep[s] = false; w[s] = 0.0;
    if (bi[s] < 0) continue;
    if (s == 0) {
      keep[0] = true; w[0] = 1.0;
    } else if (bd[0] != 0.0) {
      const Chord c = groom_chord(gp, M, bi[s]);
      const double dot = (c.x * c0.x + c.y * c0.y) + c.z * c0.z;
      keep[s] = c.len > 0.0 && c0.len > 0.0 && dot >= cos_max * (c.len * c0.len);
      if (keep[s]) w[s] = bd[0] / bd[s];
    }
    if (keep[s]) { W = W + w[s]; cnt++; }
  }
  const size_t row = (size_t)n * KK;
  int o = 0;
#pragma unroll
  for (int s = 0; s < KK; s++) {
    if (keep[s]) { idx[row + o] = bi[s]; d2_out[row + o] = bd[s]; w_out[row + o] = w[s] / W; o++; }
  }
  for (; o < KK; o++) { idx[row + o] = -1; d2_out[row + o] = HUGE_VAL; w_out[row + o] = 0.0; }
  count[n] = cnt;
}

// one lane per output point of a kept root: lane n' M + j
__global__ __launch_bounds__(256) void groom_blend_kernel(int K, int M, int C, const float* __restrict__ gp, const float* __restrict__ ga,
                                                          const double* __restrict__ roots, int k, const int* __restrict__ idx,
                                                          const double* __restrict__ w, long long n_out, const int* __restrict__ kept,
                                                          float* __restrict__ out_points, float* __restrict__ out_attrs) {
  const long long lane = (long long)blockIdx.x * 256 + threadIdx.x;
  if (lane >= n_out) return;
  const long long np = lane / M;
  const int j = (int)(lane - np * M);
  const size_t n = (size_t)kept[np];
  int g[8];
  double wt[8];
  int cnt = 0;
#pragma unroll
  for (int s = 0; s < 8; s++) {
    g[s] = 0; wt[s] = 0.0;
    if (s < k && cnt == s) {                           // the rows are compacted: the first slot outside [0, K) ends the list
      const int gi = idx[n * k + s];
      if (gi >= 0 && gi < K) { g[s] = gi; wt[s] = w[n * k + s]; cnt = s + 1; }
    }
  }
#pragma unroll
  for (int c = 0; c < 3; c++) {
    double acc = 0.0;
#pragma unroll
    for (int s = 0; s < 8; s++) {
      if (s < cnt) {
        const float* const base = gp + (size_t)g[s] * M * 3;
        acc = acc + wt[s] * ((double)base[3 * j + c] - (double)base[c]);
      }
    }
    out_points[3 * lane + c] = (float)(roots[3 * n + c] + acc);
  }
  for (int a = 0; a < C; a++) {
    double acc = 0.0;
#pragma unroll
    for (int s = 0; s < 8; s++) {
      if (s < cnt) acc = acc + wt[s] * (double)ga[((size_t)g[s] * M + j) * C + a];
    }
    out_attrs[(size_t)C * lane + a] = (float)acc;
  }
}

template <int KK>
void groom_launch_neighbours(hipStream_t s, int N, const double* roots, int K, int M, const float* gp, double max_d2, double cos_max,
                             int* idx, double* d2, double* w, int* count) {
  hipLaunchKernelGGL(groom_neighbours_kernel<KK>, dim3((N + 255) / 256), dim3(256), 0, s, N, roots, K, M, gp, max_d2, cos_max, idx, d2, w,
                     count);
}

}  // namespace

extern "C" int hgs_groom_neighbours(void* stream, int N, const double* roots, int K, int M, const float* guide_points, int k, double max_d2,
                                    double cos_max, int* idx, double* d2, double* w, int* count) {
  if (N < 0 || K < 0) { hgs_set_error("hgs_groom_neighbours: bad sizes"); return 1; }
  if (k < 1 || k > 8) { hgs_set_error("hgs_groom_neighbours: k = %d outside [1, 8]", k); return 1; }
  if (M < 2) { hgs_set_error("hgs_groom_neighbours: M = %d (at least 2 points per guide)", M); return 1; }
  if (max_d2 != max_d2 || cos_max != cos_max) { hgs_set_error("hgs_groom_neighbours: max_d2 or cos_max is NaN"); return 1; }
  if (N == 0) return 0;
  if (!roots || !idx || !d2 || !w || !count || (K > 0 && !guide_points)) { hgs_set_error("hgs_groom_neighbours: null argument"); return 1; }
  hipStream_t s = (hipStream_t)stream;
  switch (k) {
    case 1: groom_launch_neighbours<1>(s, N, roots, K, M, guide_points, max_d2, cos_max, idx, d2, w, count); break;
    case 2: groom_launch_neighbours<2>(s, N, roots, K, M, guide_points, max_d2, cos_max, idx, d2, w, count); break;
    case 3: groom_launch_neighbours<3>(s, N, roots, K, M, guide_points, max_d2, cos_max, idx, d2, w, count); break;
    case 4: groom_launch_neighbours<4>(s, N, roots, K, M, guide_points, max_d2, cos_max, idx, d2, w, count); break;
    case 5: groom_launch_neighbours<5>(s, N, roots, K, M, guide_points, max_d2, cos_max, idx, d2, w, count); break;
    case 6: groom_launch_neighbours<6>(s, N, roots, K, M, guide_points, max_d2, cos_max, idx, d2, w, count); break;
    case 7: groom_launch_neighbours<7>(s, N, roots, K, M, guide_points, max_d2, cos_max, idx, d2, w, count); break;
    default: groom_launch_neighbours<8>(s, N, roots, K, M, guide_points, max_d2, cos_max, idx, d2, w, count); break;
  }
  HGS_CHECK_LAUNCH();
  return 0;
}

extern "C" int hgs_groom_blend(void* stream, int K, int M, int C, const float* guide_points, const float* guide_attrs, const double* roots,
                               int k, const int* idx, const double* w, int n_kept, const int* kept, float* out_points, float* out_attrs) {
  if (K < 0 || n_kept < 0) { hgs_set_error("hgs_groom_blend: bad sizes"); return 1; }
  if (k < 1 || k > 8) { hgs_set_error("hgs_groom_blend: k = %d outside [1, 8]", k); return 1; }
  if (M < 2) { hgs_set_error("hgs_groom_blend: M = %d (at least 2 points per guide)", M); return 1; }
  if (C < 1 || C > 16) { hgs_set_error("hgs_groom_blend: C = %d outside [1, 16]", C); return 1; }
  const long long n_out = (long long)n_kept * M;
  if (n_out > 0x7FFFFFFFll) { hgs_set_error("hgs_groom_blend: n_kept M = %lld: at most 2^31 - 1 points per call", n_out); return 1; }
  if (n_kept == 0) return 0;
  if (K == 0) { hgs_set_error("hgs_groom_blend: %d kept roots and no guide", n_kept); return 1; }
  if (!guide_points || !guide_attrs || !roots || !idx || !w || !kept || !out_points || !out_attrs) {
    hgs_set_error("hgs_groom_blend: null argument"); return 1;
  }
  hipLaunchKernelGGL(groom_blend_kernel, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, (hipStream_t)stream, K, M, C, guide_points,
                     guide_attrs, roots, k, idx, w, n_out, kept, out_points, out_attrs);
  HGS_CHECK_LAUNCH();
  return 0;
}
