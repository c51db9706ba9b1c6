// hgs_normals.hip -- point-cloud normals (utils/normals.py: the contract; pytorch3d.ops.estimate_pointcloud_normals in the
// reference's loaders).  For every point: its K <= 64 nearest points (itself included) in float64, ordered by (d2, index);
// the covariance about their mean; the unit eigenvector of the smallest eigenvalue; the sign by the neighbours' vote.
//
//   * Grid: the points are binned into a CUBIC grid of G = 2^L cells per axis over their float64 bounding box (cell edge =
//     largest extent / G), sorted by the key (Morton code of the cell) << 32 | index with the bitonic network of hgs_keysort.h,
//     gathered into that order, and a table gives every cell's [first, end).  The level aims at ~K/4 .. 2K points per cell of
//     a uniform cloud; hair and surfaces fill fewer, fuller cells.
//   * Search + normal: ONE WAVEFRONT PER POINT (normals_kernel).  Lane r holds the r-th best (d2, index) so far.  Candidates come
//     64 at a time, one per lane, from a cell's run of the sorted array; a ballot against the K-th best drops batches that
//     cannot matter; one that can is sorted in-wave (bitonic, __shfl_xor), merged with the reversed list by one min step and
//     cleaned up by six more.  The result is the K smallest (d2, index) pairs of everything visited: a function of the SET of
//     candidates, not of the order they arrived in.
//   * Walk: the own cell, then shells of growing Chebyshev radius R.  Pruning never reasons about face positions: the cell
//     coordinate cell_of(x) is a monotone function of x, so every point within r of p along an axis lies in a cell between
//     cell_of(p - r) and cell_of(p + r), with r the K-th best distance widened far beyond its rounding.  A cell outside that box
//     is skipped; the walk ends when the box lies inside the visited block.  The shell loop runs R = 0 .. G - 1 by an integer
//     bound whatever the floating-point values are: at R = G - 1 the block is the whole grid.
//   * Epilogue: the neighbours' float64 positions are fetched by index; sums are xor-butterflies over the 64 lanes (lanes >= K
//     add +0.0), so their association depends on ranks only; cyclic Jacobi on the 3 x 3 covariance, every lane redundantly
//     (scalars and ?: selects, nothing indexed at run time); the vote by a ballot; lanes 0-2 store the normal.
// Built with -ffp-contract=off: d2 = (dx*dx + dy*dy) + dz*dz is evaluated operation by operation.
#include <float.h>

#include "hgs_common.h"
#include "hgs_jacobi3.h"
#include "hgs_keysort.h"

#define NRM_MAX_K 64
#define NRM_MAX_N (1 << 27)      // keys, sorted positions and cell bounds are 32-bit; the padded key count must fit an int
#define NRM_MAX_LEVEL 7          // 2 M cells of 8 bytes
#define NRM_MM_BLOCKS 64

namespace {

struct alignas(32) NrmPoint { double x, y, z; long long id; };
struct NrmGrid { double mnx, mny, mnz, inv; };      // cell coordinate = (x - mn) * inv, truncated and clamped to [0, G - 1]
struct NrmScratch { double* mm; NrmGrid* grid; uint64_t* keys; NrmPoint* sorted; uint2* cells; };

int normals_level(size_t N, int K) {
  int L = 1;
  while (L < NRM_MAX_LEVEL && ((size_t)1 << (3 * (L + 1))) * (size_t)K <= 4 * N) L++;
  return L;
}

size_t normals_carve(char* base, size_t N, int K, NrmScratch& s) {
  char* cur = base;
  hgs_carve(cur, s.mm, 6 * NRM_MM_BLOCKS);
  hgs_carve(cur, s.grid, 1);
  hgs_carve(cur, s.keys, pad_pow2(N));
  hgs_carve(cur, s.sorted, N);
  hgs_carve(cur, s.cells, (size_t)1 << (3 * normals_level(N, K)));
  return hgs_align_up((size_t)(cur - base)) + HGS_ALIGN;
}

// Monotone non-decreasing in x for a fixed grid (a rounded subtraction, a rounded product with inv >= 0 and a truncation
// are each monotone); NaN -> 0.
__device__ __forceinline__ int cell_of(double x, double mn, double inv, int G) {
  const double t = (x - mn) * inv;
  return t >= (double)G ? G - 1 : (t > 0.0 ? (int)t : 0);
}

__global__ __launch_bounds__(256) void normals_minmax_kernel(int N, const double* __restrict__ pts, double* __restrict__ mm) {
  __shared__ double red[4][6];
  double mn[3] = {__builtin_inf(), __builtin_inf(), __builtin_inf()}, mx[3] = {-__builtin_inf(), -__builtin_inf(), -__builtin_inf()};
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)N; i += (size_t)NRM_MM_BLOCKS * 256)
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const double v = pts[3 * i + k];
      mn[k] = fmin(mn[k], v);
      mx[k] = fmax(mx[k], v);
    }
#pragma unroll
  for (int k = 0; k < 3; k++)
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      mn[k] = fmin(mn[k], __shfl_xor(mn[k], d, 64));
      mx[k] = fmax(mx[k], __shfl_xor(mx[k], d, 64));
    }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0)
    for (int k = 0; k < 3; k++) { red[wave][k] = mn[k]; red[wave][3 + k] = mx[k]; }
  __syncthreads();
  if (threadIdx.x < 6) {
    double v = red[0][threadIdx.x];
    for (int w = 1; w < 4; w++) v = threadIdx.x < 3 ? fmin(v, red[w][threadIdx.x]) : fmax(v, red[w][threadIdx.x]);
    mm[6 * (size_t)blockIdx.x + threadIdx.x] = v;
  }
}

// min / max are exact, so the order of folding the partial results does not matter
__global__ __launch_bounds__(64) void normals_grid_kernel(int G, const double* __restrict__ mm, NrmGrid* __restrict__ grid) {
  __shared__ double s[6];
  if (threadIdx.x < 6) {
    double v = mm[threadIdx.x];
    for (int b = 1; b < NRM_MM_BLOCKS; b++) v = threadIdx.x < 3 ? fmin(v, mm[6 * b + threadIdx.x]) : fmax(v, mm[6 * b + threadIdx.x]);
    s[threadIdx.x] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double ext = fmax(fmax(s[3] - s[0], s[4] - s[1]), s[5] - s[2]);
    const double inv = (ext > 0.0 && ext < __builtin_inf()) ? (double)G / ext : 0.0;     // no extent (or overflow): one cell
    NrmGrid g = {s[0], s[1], s[2], inv};
    *grid = g;
  }
}

__global__ __launch_bounds__(256) void normals_keys_kernel(int N, int Npad, int G, const double* __restrict__ pts,
                                                           const NrmGrid* __restrict__ grid, uint64_t* __restrict__ keys) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= Npad) return;
  if (i >= N) { keys[i] = ~0ull; return; }
  const NrmGrid g = *grid;
  const uint32_t cx = prep_morton((uint32_t)cell_of(pts[3 * (size_t)i], g.mnx, g.inv, G));
  const uint32_t cy = prep_morton((uint32_t)cell_of(pts[3 * (size_t)i + 1], g.mny, g.inv, G));
  const uint32_t cz = prep_morton((uint32_t)cell_of(pts[3 * (size_t)i + 2], g.mnz, g.inv, G));
  keys[i] = ((uint64_t)(cx | (cy << 1) | (cz << 2)) << 32) | (uint32_t)i;
}

// sorted order + the cells' [first, end) (the table was zeroed: an untouched cell is empty)
__global__ __launch_bounds__(256) void normals_gather_kernel(int N, const double* __restrict__ pts, const uint64_t* __restrict__ keys,
                                                             NrmPoint* __restrict__ sorted, uint2* __restrict__ cells) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const uint64_t key = keys[i];
  const uint32_t id = (uint32_t)key, c = (uint32_t)(key >> 32);
  NrmPoint p = {pts[3 * (size_t)id], pts[3 * (size_t)id + 1], pts[3 * (size_t)id + 2], (long long)id};
  sorted[i] = p;
  if (i == 0 || (uint32_t)(keys[i - 1] >> 32) != c) cells[c].x = (uint32_t)i;
  if (i == N - 1 || (uint32_t)(keys[i + 1] >> 32) != c) cells[c].y = (uint32_t)i + 1u;
}

// ---- in-wave ordered lists of (d2, index) ----------------------------------------------------------------------------------
__device__ __forceinline__ bool kv_less(double a, int ai, double b, int bi) { return a < b || (a == b && ai < bi); }
__device__ __forceinline__ void kv_cex(double& d, int& i, int lane, int j, bool up) {
  const double od = __shfl_xor(d, j, 64);
  const int oi = __shfl_xor(i, j, 64);
  const bool mine_less = kv_less(d, i, od, oi);
  const bool keep_min = ((lane & j) == 0) == up;
  if (mine_less != keep_min) { d = od; i = oi; }
}
__device__ __forceinline__ void kv_sort64(double& d, int& i, int lane) {
#pragma unroll
  for (int k = 2; k <= 64; k <<= 1)
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) kv_cex(d, i, lane, j, (lane & k) == 0 || k == 64);
}
__device__ __forceinline__ void kv_clean64(double& d, int& i, int lane) {      // bitonic -> ascending
#pragma unroll
  for (int j = 32; j > 0; j >>= 1) kv_cex(d, i, lane, j, true);
}
__device__ __forceinline__ double uniform_f64(double v) {    // a value that is the same in every lane, moved to scalar registers
  return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
}

__global__ __launch_bounds__(256) void normals_kernel(int N, int K, int L, const double* __restrict__ pts,
                                                      const NrmPoint* __restrict__ sorted, const uint2* __restrict__ cells,
                                                      const NrmGrid* __restrict__ grid, double* __restrict__ normals,
                                                      int* __restrict__ neighbors) {
#pragma clang fp contract(off)
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (w >= N) return;                                       // whole waves leave: every lane below is active
  const int G = 1 << L;
  const NrmGrid g = *grid;
  const NrmPoint me = sorted[w];
  const double px = me.x, py = me.y, pz = me.z;
  const int cpx = cell_of(px, g.mnx, g.inv, G), cpy = cell_of(py, g.mny, g.inv, G), cpz = cell_of(pz, g.mnz, g.inv, G);

  double bd = __builtin_inf();                              // lane r: the r-th best so far
  int bi = 0x7FFFFFFF;
  double kth = __builtin_inf();                             // wave-uniform copies of lane K - 1
  int kthi = 0x7FFFFFFF;
  int lox = 0, loy = 0, loz = 0, hix = G - 1, hiy = G - 1, hiz = G - 1;      // cells that can still hold one of the K best

  auto visit = [&](int cx, int cy, int cz) {
    if (cx < lox || cx > hix || cy < loy || cy > hiy || cz < loz || cz > hiz) return;
    const uint32_t c = prep_morton((uint32_t)cx) | (prep_morton((uint32_t)cy) << 1) | (prep_morton((uint32_t)cz) << 2);
    const uint2 run = cells[c];
    const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)run.x);
    uint32_t end = (uint32_t)__builtin_amdgcn_readfirstlane((int)run.y);
    if (end > (uint32_t)N) end = (uint32_t)N;
    for (uint32_t b = first; b < end; b += 64u) {
      double d = __builtin_inf();
      int id = 0x7FFFFFFF;
      if (b + (uint32_t)lane < end) {
        const NrmPoint q = sorted[b + lane];
        const double dx = q.x - px, dy = q.y - py, dz = q.z - pz;
        d = (dx * dx + dy * dy) + dz * dz;
        id = (int)q.id;
      }
      if (__ballot(kv_less(d, id, kth, kthi)) == 0ull) continue;
      kv_sort64(d, id, lane);
      const double rd = __shfl(d, 63 - lane, 64);
      const int ri = __shfl(id, 63 - lane, 64);
      if (kv_less(rd, ri, bd, bi)) { bd = rd; bi = ri; }
      kv_clean64(bd, bi, lane);
      kth = uniform_f64(__shfl(bd, K - 1, 64));
      kthi = __builtin_amdgcn_readfirstlane(__shfl(bi, K - 1, 64));
      if (kth < __builtin_inf()) {
        // a point with d2 <= kth is within r of p along every axis; r and the interval's ends are widened by orders of
        // magnitude more than the roundings of d2, of the square root and of p -+ r
        const double r = sqrt(kth) * 1.0000000001 + 1e-150;
        const double ex = (fabs(px) + r) * 4.5e-16, ey = (fabs(py) + r) * 4.5e-16, ez = (fabs(pz) + r) * 4.5e-16;
        lox = cell_of((px - r) - ex, g.mnx, g.inv, G); hix = cell_of((px + r) + ex, g.mnx, g.inv, G);
        loy = cell_of((py - r) - ey, g.mny, g.inv, G); hiy = cell_of((py + r) + ey, g.mny, g.inv, G);
        loz = cell_of((pz - r) - ez, g.mnz, g.inv, G); hiz = cell_of((pz + r) + ez, g.mnz, g.inv, G);
      }
    }
  };

  for (int R = 0; R < G; R++) {                             // at R = G - 1 the block is the whole grid
    // (the box only ever shrinks: what lies outside it now stays outside)
    const int z0 = max(cpz - R, loz), z1 = min(cpz + R, hiz), y0 = max(cpy - R, loy), y1 = min(cpy + R, hiy);
    const int x0 = max(cpx - R, lox), x1 = min(cpx + R, hix);
    for (int cz = z0; cz <= z1; cz++)
      for (int cy = y0; cy <= y1; cy++) {
        if (abs(cz - cpz) == R || abs(cy - cpy) == R) {
          for (int cx = x0; cx <= x1; cx++) visit(cx, cy, cz);
        } else {                                            // (R > 0 here)
          if (cpx - R >= 0) visit(cpx - R, cy, cz);
          if (cpx + R <= G - 1) visit(cpx + R, cy, cz);
        }
      }
    if (lox >= cpx - R && hix <= cpx + R && loy >= cpy - R && hiy <= cpy + R && loz >= cpz - R && hiz <= cpz + R) break;
  }

  // ---- the normal: lane r holds neighbour r -------------------------------------------------------------------------------
  const bool in = lane < K && (uint32_t)bi < (uint32_t)N;   // (a lane is left unfilled only when distances overflowed to NaN)
  const size_t nb = in ? (size_t)bi : (size_t)me.id;
  const double qx = pts[3 * nb], qy = pts[3 * nb + 1], qz = pts[3 * nb + 2];
  const double invK = 1.0 / (double)K;
  const double mx = wave_sum(in ? qx : 0.0) * invK, my = wave_sum(in ? qy : 0.0) * invK, mz = wave_sum(in ? qz : 0.0) * invK;
  const double x = in ? qx - mx : 0.0, y = in ? qy - my : 0.0, z = in ? qz - mz : 0.0;
  double a00 = wave_sum(x * x) * invK, a01 = wave_sum(x * y) * invK, a02 = wave_sum(x * z) * invK;
  double a11 = wave_sum(y * y) * invK, a12 = wave_sum(y * z) * invK, a22 = wave_sum(z * z) * invK;
  double v00, v01, v02, v10, v11, v12, v20, v21, v22;
  jacobi3_sweeps(a00, a01, a02, a11, a12, a22, v00, v01, v02, v10, v11, v12, v20, v21, v22);   // (the same path in every lane)
  const int m = a00 <= a11 ? (a22 < a00 ? 2 : 0) : (a22 < a11 ? 2 : 1);
  double nx = m == 0 ? v00 : (m == 1 ? v01 : v02), ny = m == 0 ? v10 : (m == 1 ? v11 : v12), nz = m == 0 ? v20 : (m == 1 ? v21 : v22);
  const double len = sqrt((nx * nx + ny * ny) + nz * nz);
  if (len > 0.5 && len < 2.0) { nx = nx / len; ny = ny / len; nz = nz / len; } else { nx = 1.0; ny = 0.0; nz = 0.0; }   // (non-finite covariance)
  const double proj = ((qx - px) * nx + (qy - py) * ny) + (qz - pz) * nz;
  const int votes = __popcll(__ballot(in && proj > 0.0));
  const double sg = 2 * votes < K ? -1.0 : 1.0;
  const size_t o = (size_t)me.id;
  if (lane < 3) normals[3 * o + lane] = sg * (lane == 0 ? nx : (lane == 1 ? ny : nz));
  if (neighbors && lane < K) neighbors[o * (size_t)K + lane] = in ? bi : -1;
}

}  // namespace

extern "C" size_t hgs_pointcloud_normals_scratch_bytes(int N, int K) {
  NrmScratch s;
  const size_t n = (size_t)(N > 0 ? (N > NRM_MAX_N ? NRM_MAX_N : N) : 0);
  return normals_carve(nullptr, n, K < 1 ? 1 : (K > NRM_MAX_K ? NRM_MAX_K : K), s);
}

extern "C" int hgs_pointcloud_normals(void* stream, int N, int K, const double* points, double* normals, int* neighbors,
                                      void* scratch, size_t scratch_bytes) {
  if (N < 0 || N > NRM_MAX_N) { hgs_set_error("hgs_pointcloud_normals: N = %d outside [0, %d]", N, NRM_MAX_N); return 1; }
  if (K < 1 || K > NRM_MAX_K) { hgs_set_error("hgs_pointcloud_normals: K = %d outside [1, %d]", K, NRM_MAX_K); return 1; }
  if (N == 0) return 0;
  if (K > N) { hgs_set_error("hgs_pointcloud_normals: K = %d exceeds the number of points N = %d", K, N); return 1; }
  if (!points || !normals || !scratch) { hgs_set_error("hgs_pointcloud_normals: null argument"); return 1; }
  const size_t need = hgs_pointcloud_normals_scratch_bytes(N, K);
  if (need > scratch_bytes || ((size_t)scratch & (HGS_ALIGN - 1))) {
    hgs_set_error("hgs_pointcloud_normals: scratch must be %d-byte aligned and >= %zu bytes (got %zu)", HGS_ALIGN, need, scratch_bytes);
    return 1;
  }
  hipStream_t st = (hipStream_t)stream;
  NrmScratch s;
  normals_carve((char*)scratch, (size_t)N, K, s);
  const size_t Npad = pad_pow2((size_t)N);
  const int L = normals_level((size_t)N, K), G = 1 << L;
  HgsProfScope _prof(st, HGS_K_KNN);
  hipLaunchKernelGGL(normals_minmax_kernel, dim3(NRM_MM_BLOCKS), dim3(256), 0, st, N, points, s.mm);
  hipLaunchKernelGGL(normals_grid_kernel, dim3(1), dim3(64), 0, st, G, s.mm, s.grid);
  hipLaunchKernelGGL(normals_keys_kernel, dim3((unsigned)((Npad + 255) / 256)), dim3(256), 0, st, N, (int)Npad, G, points, s.grid, s.keys);
  keysort_launch(st, s.keys, Npad);
  if (hgs_zero_async(st, s.cells, sizeof(uint2) << (3 * L))) return 1;
  hipLaunchKernelGGL(normals_gather_kernel, dim3((N + 255) / 256), dim3(256), 0, st, N, points, s.keys, s.sorted, s.cells);
  hipLaunchKernelGGL(normals_kernel, dim3((N + 3) / 4), dim3(256), 0, st, N, K, L, points, s.sorted, s.cells, s.grid, normals, neighbors);
  HGS_CHECK_LAUNCH();
  return 0;
}
