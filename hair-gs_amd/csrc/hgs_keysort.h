// hgs_keysort.h -- Morton bit spreading and the bitonic sort of unique 64-bit keys (code << 32 | index) that the grid searches
// share: the grid of Morton cells (hgs_cellgrid.h: distCUDA2 and the magnet term) and the point-cloud normals (hgs_normals.hip).
// Included into each translation unit's own anonymous namespace; the kernels are the ones hgs_knn.hip has always launched, in
// the same order.
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

}  // namespace
