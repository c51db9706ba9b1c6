// hgs_knn.hip -- distCUDA2: mean squared distance to the 3 nearest neighbours (simple-knn/simple_knn.cu).
//
// Same plan as the reference (origin-including bounding box :192-201, 30-bit Morton codes :46-71, stable sort
// by code :207-214, 1024-point boxes :79-118, box-pruned exact search :148-184) with these CDNA4 choices:
//   * no host round trips: min/max stay on the device (the reference does two blocking D2H copies);
//   * the stable (code, index) sort is a sort by the unique 64-bit key code<<32|index -> plain bitonic network
//     (LDS for strides < 4096, global otherwise); called once per run, P <= a few million;
//   * points are gathered once into Morton order; the search (round 6) runs one lane per point over a GRID OF MORTON CELLS,
//     the one hgs_cellgrid.h holds (its plan is described there; the magnet term searches the same grid).  Rounds 1-5 tested
//     boxes of 1024 Morton-CONSECUTIVE points: such a run straddles the curve's jumps, its bounding box holds most of the scene,
//     every point lies inside most boxes and the pruning pruned nothing (3.8 ms for 50 k points, 96 % of the call in the search).
//     The three smallest distances of a point do not depend on the traversal, so the result is exactly the reference's (the
//     exact 3-NN in its arithmetic).
// Also here: the fixed-radius pair search (hgs_radius_pairs), the exhaustive 3-NN (hgs_knn3) and the float64 nearest distance
// (hgs_nearest_distance_f64).
#include "hgs_common.h"
#include "hgs_cellgrid.h"  // the grid of Morton cells: keys, gather, cell table, the search; Best3; hgs_keysort.h (the sort)

namespace {

struct KnnScratch { float* minmax; uint64_t* keys; float4* sorted; uint32_t* cells; };   // cells: 8 words per cell

// component-wise min/max with init (0,0,0) (simple_knn.cu:192): MM_BLOCKS partial results, folded by whoever reads them
#define MM_BLOCKS 64
__global__ __launch_bounds__(1024) void minmax_kernel(int P, const float* __restrict__ pts, float* __restrict__ mm) {
  __shared__ float red[16][6];
  float mn[3] = {0.f, 0.f, 0.f}, mx[3] = {0.f, 0.f, 0.f};
  for (size_t i = (size_t)blockIdx.x * 1024 + threadIdx.x; i < (size_t)P; i += (size_t)MM_BLOCKS * 1024)
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const float v = pts[3 * i + k];
      mn[k] = fminf(mn[k], v);
      mx[k] = fmaxf(mx[k], v);
    }
#pragma unroll
  for (int k = 0; k < 3; k++)
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      mn[k] = fminf(mn[k], __shfl_xor(mn[k], d, 64));
      mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], d, 64));
    }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0)
    for (int k = 0; k < 3; k++) { red[wave][k] = mn[k]; red[wave][3 + k] = mx[k]; }
  __syncthreads();
  if (threadIdx.x < 6) {
    float v = red[0][threadIdx.x];
    for (int w = 1; w < 16; w++) v = threadIdx.x < 3 ? fminf(v, red[w][threadIdx.x]) : fmaxf(v, red[w][threadIdx.x]);
    mm[8 * (size_t)blockIdx.x + threadIdx.x] = v;
  }
}

// distCUDA2 as a source of the grid: every one of the P points is live; the box is the fold of the MM_BLOCKS partial min / max
// (exact: the order of folding does not matter); non-finite points keep simple_knn.cu's treatment (hgs_cellgrid.h cellgrid_code)
struct KnnSource {
  const float* __restrict__ mm;
  static constexpr bool kGuarded = false;
  __device__ __forceinline__ int live(int P) const { return P; }
  __device__ __forceinline__ void load_box(float* box) const {
    if (threadIdx.x < 6) {
      float v = mm[threadIdx.x];
      for (int b = 1; b < MM_BLOCKS; b++) v = threadIdx.x < 3 ? fminf(v, mm[8 * b + threadIdx.x]) : fmaxf(v, mm[8 * b + threadIdx.x]);
      box[threadIdx.x] = v;
    }
    __syncthreads();
  }
};

// the three smallest distances, the point itself excluded (simple_knn.cu:132-146)
struct KnnBest {
  typedef float Out;          // out[point's index] = the mean of the three
  float knn[3];
  static constexpr bool kSelf = false, kGuarded = false;
  __device__ __forceinline__ void clear() { knn[0] = knn[1] = knn[2] = FLT_MAX; }
  __device__ __forceinline__ float third() const { return knn[2]; }
  __device__ __forceinline__ void add(float dist, uint32_t) {
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const float t = knn[j];
      const bool sw = t > dist;
      knn[j] = sw ? dist : t;
      dist = sw ? t : dist;
    }
  }
  __device__ __forceinline__ void store(float* __restrict__ out, const float4& me) const {
    out[__float_as_uint(me.w)] = (knn[0] + knn[1] + knn[2]) / 3.0f;
  }
};

size_t knn_carve(char* base, size_t P, size_t Npad, KnnScratch& s) {
  char* cur = base;
  hgs_carve(cur, s.minmax, 8 * MM_BLOCKS);
  hgs_carve(cur, s.keys, Npad);
  hgs_carve(cur, s.sorted, P + 1);
  hgs_carve(cur, s.cells, 8 * ((size_t)1 << (3 * cellgrid_level(P))));
  return hgs_align_up((size_t)(cur - base)) + HGS_ALIGN;
}
}  // namespace

size_t hgs_dist2_scratch(int P) {
  KnnScratch s;
  return knn_carve(nullptr, (size_t)P, pad_pow2((size_t)P), s);
}

int hgs_launch_dist2(hipStream_t st, int P, const float* points, float* out, void* scratch, size_t scratch_bytes) {
  const size_t Npad = pad_pow2((size_t)P);
  KnnScratch s;
  knn_carve((char*)scratch, (size_t)P, Npad, s);
  if (hgs_dist2_scratch(P) > scratch_bytes || ((size_t)scratch & (HGS_ALIGN - 1))) {
    hgs_set_error("hgs_dist2: scratch must be %d-byte aligned and >= %zu bytes (got %zu)", HGS_ALIGN, hgs_dist2_scratch(P), scratch_bytes);
    return 1;
  }
  HgsProfScope _prof(st, HGS_K_KNN);
  const KnnSource src{s.minmax};
  hipLaunchKernelGGL(minmax_kernel, dim3(MM_BLOCKS), dim3(1024), 0, st, P, points, s.minmax);
  hipLaunchKernelGGL((cellgrid_keys_kernel<KnnSource, float>), dim3((unsigned)((Npad + 255) / 256)), dim3(256), 0, st, src, P, (int)Npad, points, s.keys);
  keysort_launch(st, s.keys, Npad);
  const int L = cellgrid_level((size_t)P);
  const unsigned n_cells = 1u << (3 * L);
  hipLaunchKernelGGL((cellgrid_gather_kernel<KnnSource, float>), dim3((P + 255) / 256), dim3(256), 0, st, src, P, points, s.keys, s.sorted);
  hipLaunchKernelGGL(cells_clear_kernel, dim3((n_cells + 255) / 256), dim3(256), 0, st, n_cells, s.cells);
  hipLaunchKernelGGL(cellgrid_mark_kernel<KnnSource>, dim3((P + 255) / 256), dim3(256), 0, st, src, P, 30 - 3 * L, s.keys, s.sorted, s.cells);
  hipLaunchKernelGGL((cellgrid_search_kernel<KnnSource, KnnBest>), dim3((P + 255) / 256), dim3(256), 0, st, P, L, src, s.sorted, s.keys, s.cells, out);
  HGS_CHECK_LAUNCH();
  return 0;
}

// ---- fixed-radius pair search over strand ends (hgs_radius_pairs) ------------------------------------------------------
namespace {
__global__ __launch_bounds__(256) void radius_pairs_kernel(int N, const float* __restrict__ pos, const float* __restrict__ dir,
                                                           float r2, float min_cos, int bidirectional, int capacity,
                                                           int* __restrict__ pairs, float* __restrict__ dist,
                                                           int* __restrict__ count, float reach_x) {
  __shared__ float sp[256][3], sd[256][3];
  const int a = blockIdx.x * 256 + threadIdx.x;
  float ax = 0.f, ay = 0.f, az = 0.f, ux = 0.f, uy = 0.f, uz = 0.f;
  if (a < N) { ax = pos[3 * a]; ay = pos[3 * a + 1]; az = pos[3 * a + 2]; ux = dir[3 * a]; uy = dir[3 * a + 1]; uz = dir[3 * a + 2]; }
  // only tiles at or after this block's own: every unordered pair is tested once, by the block of its smaller index
  // reach_x >= 0: the points are sorted by x; a tile that starts farther than the radius beyond this block's last point
  // (and every tile after it) holds no partner
  const float block_max_x = reach_x >= 0.f ? pos[3 * min(N - 1, (int)blockIdx.x * 256 + 255)] + reach_x : 0.f;
  for (int t0 = blockIdx.x * 256; t0 < N; t0 += 256) {
    if (reach_x >= 0.f && pos[3 * t0] > block_max_x) break;
    const int j = t0 + threadIdx.x;
    __syncthreads();
    if (j < N) {
#pragma unroll
      for (int c = 0; c < 3; c++) { sp[threadIdx.x][c] = pos[3 * j + c]; sd[threadIdx.x][c] = dir[3 * j + c]; }
    }
    __syncthreads();
    const int nb = min(256, N - t0);
    if (a < N) {
      for (int k = 0; k < nb; k++) {                       // broadcast LDS reads
        const int b = t0 + k;
        if (b <= a) continue;
        const float dx = sp[k][0] - ax, dy = sp[k][1] - ay, dz = sp[k][2] - az;
        const float d2 = dx * dx + dy * dy + dz * dz;
        if (d2 > r2) continue;
        float dot = -(ux * sd[k][0] + uy * sd[k][1] + uz * sd[k][2]);
        if (bidirectional) dot = fabsf(dot);
        if (!(dot >= min_cos)) continue;
        const int slot = atomicAdd(count, 1);
        if (slot < capacity) { pairs[2 * slot] = a; pairs[2 * slot + 1] = b; dist[slot] = sqrtf(d2); }
      }
    }
  }
}
}  // namespace

extern "C" int hgs_radius_pairs(void* stream, int N, const float* pos, const float* dir, float radius, float min_cos,
                                int bidirectional, int capacity, int* pairs, float* dist, int* count, int sorted_by_x) {
  if (N <= 1) return 0;
  if (!pos || !dir || !count || capacity < 0 || (capacity > 0 && (!pairs || !dist))) { hgs_set_error("hgs_radius_pairs: bad arguments"); return 1; }
  hipStream_t s = (hipStream_t)stream;
  {
    HgsProfScope _prof(s, HGS_K_KNN);
    hipLaunchKernelGGL(radius_pairs_kernel, dim3((N + 255) / 256), dim3(256), 0, s, N, pos, dir, radius * radius, min_cos,
                       bidirectional, capacity, pairs, dist, count, sorted_by_x ? radius : -1.f);
  }
  HGS_CHECK_LAUNCH();
  return 0;
}

// ---- K = 3 nearest neighbours of every point within its own set (hgs_knn3) -----------------------------------------------
// What the magnet loss asks pytorch3d for (loss/losses.py:139-144: knn_points(ends, ends, K=3, return_sorted=True)) over
// the strand ends -- thousands to 10^5 points that move every iteration, so no tree: one query per lane, all points
// through LDS in 256-point tiles (broadcast reads), the three best kept sorted in registers.  The point itself is a
// candidate like any other (pytorch3d returns it first, at distance 0); ties are ordered by index.
namespace {
__global__ __launch_bounds__(256) void knn3_kernel(int N, const float* __restrict__ pos, int* __restrict__ idx, float* __restrict__ d2out) {
  __shared__ float sp[256][3];
  const int a = blockIdx.x * 256 + threadIdx.x;
  float ax = 0.f, ay = 0.f, az = 0.f;
  if (a < N) { ax = pos[3 * a]; ay = pos[3 * a + 1]; az = pos[3 * a + 2]; }
  Best3 b;
  best3_clear(b);
  for (int t0 = 0; t0 < N; t0 += 256) {
    const int j = t0 + threadIdx.x;
    __syncthreads();
    if (j < N) {
#pragma unroll
      for (int c = 0; c < 3; c++) sp[threadIdx.x][c] = pos[3 * j + c];
    }
    __syncthreads();
    const int nb = min(256, N - t0);
    for (int k = 0; k < nb; k++) {
      const float dx = ax - sp[k][0], dy = ay - sp[k][1], dz = az - sp[k][2];
      best3_push(b, dx * dx + dy * dy + dz * dz, t0, k);
    }
  }
  if (a < N) {
#pragma unroll
    for (int j = 0; j < 3; j++) { idx[3 * a + j] = b.i[j]; d2out[3 * a + j] = b.d[j]; }
  }
}
}  // namespace

extern "C" int hgs_knn3(void* stream, int N, const float* points, int* idx, float* dist2) {
  if (N <= 0) return 0;
  if (!points || !idx || !dist2) { hgs_set_error("hgs_knn3: null argument"); return 1; }
  hipStream_t s = (hipStream_t)stream;
  {
    HgsProfScope _prof(s, HGS_K_KNN);
    hipLaunchKernelGGL(knn3_kernel, dim3((N + 255) / 256), dim3(256), 0, s, N, points, idx, dist2);
  }
  HGS_CHECK_LAUNCH();
  return 0;
}

// ---- distance to the nearest of a small set of reference points, in float64 ------------------------------------------------
// What compute_strands_info asks a scipy cKDTree of the reference strand roots for (scene/hair_gaussian_model.py:1466-1470: the
// two ends of every strand, to orient it root -> tip): a few thousand roots against 10^5-10^6 strand ends.  One lane per point,
// the roots staged through LDS in float64; the distance is sqrt(dx^2 + dy^2 + dz^2) evaluated in float64 in that order (what a
// brute force over the tree's points gives).  torch.cdist's float64 kernel took 8 ms per call for this shape -- a third of the
// GPU time of a training run with the topology operators.
#define ND_TILE 1024
__global__ __launch_bounds__(256) void nearest_dist_f64_kernel(int N, int M, const float* __restrict__ pts, const double* __restrict__ refs,
                                                               double* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double r[ND_TILE * 3];
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool live = i < N;
  const double px = live ? (double)pts[3 * (size_t)i] : 0.0, py = live ? (double)pts[3 * (size_t)i + 1] : 0.0,
               pz = live ? (double)pts[3 * (size_t)i + 2] : 0.0;
  double best = __builtin_inf();
  for (int m0 = 0; m0 < M; m0 += ND_TILE) {
    const int cnt = min(ND_TILE, M - m0);
    __syncthreads();
    for (int k = threadIdx.x; k < cnt * 3; k += 256) r[k] = refs[(size_t)m0 * 3 + k];
    __syncthreads();
    for (int k = 0; k < cnt; k++) {
      const double dx = px - r[3 * k], dy = py - r[3 * k + 1], dz = pz - r[3 * k + 2];
      const double d2 = dx * dx + dy * dy + dz * dz;
      best = d2 < best ? d2 : best;
    }
  }
  if (live) out[i] = sqrt(best);
}

extern "C" int hgs_nearest_distance_f64(void* stream, int N, int M, const float* points, const double* refs, double* out) {
  if (N < 0 || M < 0) { hgs_set_error("hgs_nearest_distance_f64: bad sizes"); return 1; }
  if (N == 0) return 0;
  if (M == 0 || !points || !refs || !out) { hgs_set_error("hgs_nearest_distance_f64: no reference points / null argument"); return 1; }
  hipLaunchKernelGGL(nearest_dist_f64_kernel, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, N, M, points, refs, out);
  HGS_CHECK_LAUNCH();
  return 0;
}
