// hgs_keysort.h -- Morton bit spreading and the bitonic sort of unique 64-bit keys (code << 32 | index) that the grid searches
// share: distCUDA2 (hgs_knn.hip), the point-cloud normals (hgs_normals.hip) and the magnet term (hgs_magnet.hip).  Included into each translation unit's own
// anonymous namespace; the kernels are the ones hgs_knn.hip has always launched, in the same order.
#pragma once
#include "hgs_common.h"

namespace {

#define KNN_LDS_KEYS 4096

__device__ __forceinline__ uint32_t prep_morton(uint32_t x) {
  x = (x | (x << 16)) & 0x030000FF;
  x = (x | (x << 8)) & 0x0300F00F;
  x = (x | (x << 4)) & 0x030C30C3;
  x = (x | (x << 2)) & 0x09249249;
  return x;
}

// bitonic steps j = jstart .. 1 of stage k inside LDS chunks of KNN_LDS_KEYS keys (jstart < KNN_LDS_KEYS);
// with full=true runs every stage k = 2..KNN_LDS_KEYS (initial chunk sort)
__global__ __launch_bounds__(1024) void bitonic_lds_kernel(uint64_t* __restrict__ keys, int k_stage, int jstart, bool full) {
  __shared__ uint64_t sk[KNN_LDS_KEYS];
  const size_t base = (size_t)blockIdx.x * KNN_LDS_KEYS;
  for (int i = threadIdx.x; i < KNN_LDS_KEYS; i += 1024) sk[i] = keys[base + i];
  __syncthreads();
  const int k0 = full ? 2 : k_stage, k1 = full ? KNN_LDS_KEYS : k_stage;
  for (int k = k0; k <= k1; k <<= 1) {
    for (int j = full ? (k >> 1) : jstart; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < KNN_LDS_KEYS / 2; t += 1024) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const int l = i | j;
        const bool asc = (((base + i) & (size_t)k) == 0);
        const uint64_t x = sk[i], y = sk[l];
        if ((x > y) == asc) { sk[i] = y; sk[l] = x; }
      }
      __syncthreads();
    }
    if (!full) break;
  }
  for (int i = threadIdx.x; i < KNN_LDS_KEYS; i += 1024) keys[base + i] = sk[i];
}

__global__ __launch_bounds__(256) void bitonic_global_kernel(uint64_t* __restrict__ keys, size_t half, int k, int j) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= half) return;
  const size_t i = ((t & ~((size_t)j - 1)) << 1) | (t & ((size_t)j - 1));
  const size_t l = i | (size_t)j;
  const bool asc = (i & (size_t)k) == 0;
  const uint64_t x = keys[i], y = keys[l];
  if ((x > y) == asc) { keys[i] = y; keys[l] = x; }
}

// keys padded to a power of two >= KNN_LDS_KEYS (the padding holds ~0, which sorts last)
size_t pad_pow2(size_t P) {
  size_t n = KNN_LDS_KEYS;
  while (n < P) n <<= 1;
  return n;
}

// ascending sort of Npad = pad_pow2(..) keys: LDS for strides < KNN_LDS_KEYS, global otherwise
void keysort_launch(hipStream_t st, uint64_t* keys, size_t Npad) {
  const unsigned nchunks = (unsigned)(Npad / KNN_LDS_KEYS);
  hipLaunchKernelGGL(bitonic_lds_kernel, dim3(nchunks), dim3(1024), 0, st, keys, 0, 0, true);
  for (size_t k = 2 * KNN_LDS_KEYS; k <= Npad; k <<= 1) {
    size_t j = k >> 1;
    for (; j >= KNN_LDS_KEYS; j >>= 1)
      hipLaunchKernelGGL(bitonic_global_kernel, dim3((unsigned)((Npad / 2 + 255) / 256)), dim3(256), 0, st, keys, Npad / 2, (int)k, (int)j);
    hipLaunchKernelGGL(bitonic_lds_kernel, dim3(nchunks), dim3(1024), 0, st, keys, (int)k, (int)j, false);
  }
}

// ---- what the searches over a grid of Morton cells share (hgs_knn.hip: distCUDA2; hgs_magnet.hip: the magnet term) ----
// coordinate -> cell coordinate of the Morton kernels, saturating (NaN and negatives -> 0)
__device__ __forceinline__ uint32_t f2u_sat(float v) {
  if (!(v > 0.f)) return 0u;
  if (v >= 4294967040.f) return 0xFFFFFFFFu;
  return (uint32_t)v;
}

// squared distance of a point to a box, exactly as distBoxPoint (simple_knn.cu:120-130)
__device__ __forceinline__ float box_point_dist2(const float* bx, float x, float y, float z) {
  float d0 = 0.f, d1 = 0.f, d2 = 0.f;
  if (x < bx[0] || x > bx[3]) d0 = fminf(fabsf(x - bx[0]), fabsf(x - bx[3]));
  if (y < bx[1] || y > bx[4]) d1 = fminf(fabsf(y - bx[1]), fabsf(y - bx[4]));
  if (z < bx[2] || z > bx[5]) d2 = fminf(fabsf(z - bx[2]), fabsf(z - bx[5]));
  return d0 * d0 + d1 * d1 + d2 * d2;
}

// ---- the cell table: per cell of level L (code >> (30 - 3 L)) [first, end) in the sorted array and the points' bounding box.
// Floats are kept as order-preserving integers so that min / max are integer atomics (exact, order-independent).
__device__ __forceinline__ int fkey(float v) { const int b = __float_as_int(v); return b >= 0 ? b : b ^ 0x7FFFFFFF; }   // monotone: a < b <=> fkey(a) < fkey(b)
__device__ __forceinline__ float funkey(int k) { return __int_as_float(k >= 0 ? k : k ^ 0x7FFFFFFF); }

__global__ __launch_bounds__(256) void cells_clear_kernel(uint32_t n_cells, uint32_t* __restrict__ cells) {
  const uint32_t c = blockIdx.x * 256 + threadIdx.x;
  if (c >= n_cells) return;
  uint4* t = (uint4*)(cells + 8 * (size_t)c);
  t[0] = make_uint4(0u, 0u, (uint32_t)0x7FFFFFFF, (uint32_t)0x7FFFFFFF);              // first, end, min x, min y
  t[1] = make_uint4((uint32_t)0x7FFFFFFF, 0x80000000u, 0x80000000u, 0x80000000u);     // min z, max x, max y, max z
}

}  // namespace
