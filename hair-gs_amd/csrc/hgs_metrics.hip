// hgs_metrics.hip -- strand metrics on the GPU (hgs_oriented_match / hgs_strand_votes; reference loss/metrics.py:12-85).
//
// The CPU path (loss/metrics.py) builds a cKDTree per threshold pair and direction, flattens the radius lists in Python and
// reduces them with numpy.  Here one pass tests every threshold pair at once:
//   * B's points go into a uniform grid of cell edge h = r_max (1 + 1e-6) (h above the largest radius keeps a true neighbour
//     within +-1 cell whatever floor((x - lo) / h) rounds to).  Cells are not stored densely (a metre-scale scene at
//     millimetre radii would not fit): a cell's key hashes into a power-of-two bucket table of at least 2 nB buckets, and a
//     counting sort (count, scan, scatter) lays B out bucket by bucket.  A bucket may hold points of several cells; every
//     candidate gets the exact test, so collisions cost time and never change a result.
//   * a query visits the buckets of its 27 cells and tests each candidate against all K <= 32 pairs, in float64, operation by
//     operation (built with -ffp-contract=off): d2 = (dx*dx + dy*dy) + dz*dz <= r_k*r_k, the form cKDTree.query_ball_point
//     decides by, and dot >= cos_k (|dot| when bidirectional; a NaN never matches, as in numpy).
//   * strand consistency (recall direction): one workgroup per A strand deduplicates its (point, B strand) matches in an LDS
//     hash set (value: the bitmask of pairs under which the point matched that strand), then per pair counts the points per B
//     strand in a second LDS table and keeps the largest count.  A strand whose set does not fit is reported, not truncated.
#include "hgs_common.h"

namespace {

#define HGS_METRICS_MAX_K 32
#define HGS_METRICS_MAX_CELLS (1 << 21)   // cells per axis
#define HGS_VOTE_MAX_CAPACITY 2048        // LDS entries of each vote table (20 bytes per entry: 40 KB)
#define MT_BLOCK 256
#define SCAN_CHUNK 1024                   // buckets per workgroup of the bucket scan (4 per lane)

struct MatchParams {
  double lo[3], h;
  int dims[3], K, bidirectional;
  uint32_t table_mask;
  double r2max;
  double r2[HGS_METRICS_MAX_K], cs[HGS_METRICS_MAX_K];
};

struct MatchScratch { uint32_t* starts; uint32_t* cursor; uint32_t* block_tot; uint32_t* bucket; double* spos; double* sdir; int* sidx; };

size_t match_table(int nB) {
  size_t T = SCAN_CHUNK;
  while (T < 2 * (size_t)nB) T <<= 1;
  return T;
}

size_t match_layout(int nB, char* base, MatchScratch* s) {
  const size_t T = match_table(nB);
  char* cur = base;
  auto take = [&](size_t bytes) { char* p = cur; cur += hgs_align_up(bytes); return p; };
  char* starts = take(4 * (T + 1));
  char* cursor = take(4 * T);
  char* block_tot = take(4 * (T / SCAN_CHUNK + 1));
  char* bucket = take(4 * (size_t)nB);
  char* spos = take(24 * (size_t)nB);
  char* sdir = take(24 * (size_t)nB);
  char* sidx = take(4 * (size_t)nB);
  if (s) *s = MatchScratch{(uint32_t*)starts, (uint32_t*)cursor, (uint32_t*)block_tot, (uint32_t*)bucket, (double*)spos,
                           (double*)sdir, (int*)sidx};
  return (size_t)(cur - base) + HGS_ALIGN;
}

__device__ __forceinline__ uint32_t cell_bucket(int cx, int cy, int cz, uint32_t mask) {
  uint64_t k = ((uint64_t)(uint32_t)(cx + 1) << 44) | ((uint64_t)(uint32_t)(cy + 1) << 22) | (uint64_t)(uint32_t)(cz + 1);
  k ^= k >> 31; k *= 0x7FB5D329728EA185ull; k ^= k >> 27; k *= 0x81DADEF4BC2DD44Dull; k ^= k >> 33;   // (murmur3-style finaliser)
  return (uint32_t)k & mask;
}

// floor((x - lo) / h) of one axis; false where the point has no cell within +-1 of the grid (outside it, or NaN)
__device__ __forceinline__ bool query_cell(double x, double lo, double h, int dims, int* c) {
  const double f = floor((x - lo) / h);
  if (!(f >= -1.0 && f <= (double)dims)) return false;
  *c = (int)f;
  return true;
}

__device__ __forceinline__ int grid_cell(double x, double lo, double h, int dims) {
  const double f = floor((x - lo) / h);
  return f >= 0.0 ? (f <= (double)(dims - 1) ? (int)f : dims - 1) : 0;   // (NaN -> 0: such a point never matches)
}

// bit k set iff B point j matches query (p, d) under pair k
__device__ __forceinline__ uint32_t pair_mask(const MatchParams& P, double px, double py, double pz, double ux, double uy, double uz,
                                              const double* __restrict__ spos, const double* __restrict__ sdir, uint32_t j) {
  const double dx = spos[3 * (size_t)j] - px, dy = spos[3 * (size_t)j + 1] - py, dz = spos[3 * (size_t)j + 2] - pz;
  const double d2 = (dx * dx + dy * dy) + dz * dz;
  if (!(d2 <= P.r2max)) return 0u;
  double dot = (ux * sdir[3 * (size_t)j] + uy * sdir[3 * (size_t)j + 1]) + uz * sdir[3 * (size_t)j + 2];
  if (P.bidirectional) dot = fabs(dot);
  uint32_t m = 0u;
  for (int k = 0; k < P.K; k++)
    if (d2 <= P.r2[k] && dot >= P.cs[k]) m |= 1u << k;
  return m;
}

__global__ __launch_bounds__(MT_BLOCK) void bucket_count_kernel(int nB, MatchParams P, const double* __restrict__ pts,
                                                                 uint32_t* __restrict__ bucket, uint32_t* __restrict__ count) {
  const int i = blockIdx.x * MT_BLOCK + threadIdx.x;
  if (i >= nB) return;
  const int cx = grid_cell(pts[3 * (size_t)i], P.lo[0], P.h, P.dims[0]);
  const int cy = grid_cell(pts[3 * (size_t)i + 1], P.lo[1], P.h, P.dims[1]);
  const int cz = grid_cell(pts[3 * (size_t)i + 2], P.lo[2], P.h, P.dims[2]);
  const uint32_t b = cell_bucket(cx, cy, cz, P.table_mask);
  bucket[i] = b;
  atomicAdd(&count[b], 1u);
}

// inclusive scan of s[0..255] (one value per lane) in LDS
__device__ __forceinline__ void lds_scan256(uint32_t* s) {
  for (int off = 1; off < MT_BLOCK; off <<= 1) {
    const uint32_t v = threadIdx.x >= (unsigned)off ? s[threadIdx.x - off] : 0u;
    __syncthreads();
    s[threadIdx.x] += v;
    __syncthreads();
  }
}

// exclusive scan of each SCAN_CHUNK buckets in place; chunk totals to tot[]
__global__ __launch_bounds__(MT_BLOCK) void scan_local_kernel(uint32_t* __restrict__ v, uint32_t* __restrict__ tot) {
  __shared__ uint32_t s[MT_BLOCK];
  uint32_t* p = v + (size_t)blockIdx.x * SCAN_CHUNK + 4 * threadIdx.x;
  const uint32_t a = p[0], b = p[1], c = p[2], d = p[3];
  s[threadIdx.x] = a + b + c + d;
  __syncthreads();
  lds_scan256(s);
  const uint32_t base = threadIdx.x ? s[threadIdx.x - 1] : 0u;
  p[0] = base; p[1] = base + a; p[2] = base + a + b; p[3] = base + a + b + c;
  if (threadIdx.x == MT_BLOCK - 1) tot[blockIdx.x] = s[MT_BLOCK - 1];
}

// exclusive scan of the n chunk totals in place (one workgroup, running carry); the grand total to *end
__global__ __launch_bounds__(MT_BLOCK) void scan_top_kernel(int n, uint32_t* __restrict__ tot, uint32_t* __restrict__ end) {
  __shared__ uint32_t s[MT_BLOCK];
  uint32_t carry = 0u;
  for (int c0 = 0; c0 < n; c0 += MT_BLOCK) {
    const int i = c0 + threadIdx.x;
    const uint32_t x = i < n ? tot[i] : 0u;
    s[threadIdx.x] = x;
    __syncthreads();
    lds_scan256(s);
    if (i < n) tot[i] = carry + s[threadIdx.x] - x;
    carry += s[MT_BLOCK - 1];
    __syncthreads();
  }
  if (threadIdx.x == 0) *end = carry;
}

__global__ __launch_bounds__(MT_BLOCK) void scan_add_kernel(uint32_t T, uint32_t* __restrict__ v, const uint32_t* __restrict__ tot) {
  const uint32_t i = blockIdx.x * MT_BLOCK + threadIdx.x;
  if (i < T) v[i] += tot[i / SCAN_CHUNK];
}

__global__ __launch_bounds__(MT_BLOCK) void bucket_scatter_kernel(int nB, const double* __restrict__ pts, const double* __restrict__ dirs,
                                                                  const uint32_t* __restrict__ bucket, const uint32_t* __restrict__ starts,
                                                                  uint32_t* __restrict__ cursor, double* __restrict__ spos,
                                                                  double* __restrict__ sdir, int* __restrict__ sidx) {
  const int i = blockIdx.x * MT_BLOCK + threadIdx.x;
  if (i >= nB) return;
  const uint32_t b = bucket[i];
  const uint32_t at = starts[b] + atomicAdd(&cursor[b], 1u);
#pragma unroll
  for (int c = 0; c < 3; c++) {
    spos[3 * (size_t)at + c] = pts[3 * (size_t)i + c];
    sdir[3 * (size_t)at + c] = dirs[3 * (size_t)i + c];
  }
  sidx[at] = i;
}

__global__ __launch_bounds__(MT_BLOCK) void oriented_match_kernel(int nA, MatchParams P, const double* __restrict__ a_pts,
                                                                  const double* __restrict__ a_dirs, const uint32_t* __restrict__ starts,
                                                                  const double* __restrict__ spos, const double* __restrict__ sdir,
                                                                  uint32_t* __restrict__ out) {
  const int i = blockIdx.x * MT_BLOCK + threadIdx.x;
  if (i >= nA) return;
  const double px = a_pts[3 * (size_t)i], py = a_pts[3 * (size_t)i + 1], pz = a_pts[3 * (size_t)i + 2];
  const double ux = a_dirs[3 * (size_t)i], uy = a_dirs[3 * (size_t)i + 1], uz = a_dirs[3 * (size_t)i + 2];
  uint32_t m = 0u;
  int cx, cy, cz;
  if (query_cell(px, P.lo[0], P.h, P.dims[0], &cx) && query_cell(py, P.lo[1], P.h, P.dims[1], &cy) &&
      query_cell(pz, P.lo[2], P.h, P.dims[2], &cz)) {
    for (int ox = max(cx - 1, 0); ox <= min(cx + 1, P.dims[0] - 1); ox++)
      for (int oy = max(cy - 1, 0); oy <= min(cy + 1, P.dims[1] - 1); oy++)
        for (int oz = max(cz - 1, 0); oz <= min(cz + 1, P.dims[2] - 1); oz++) {
          const uint32_t b = cell_bucket(ox, oy, oz, P.table_mask);
          const uint32_t e = starts[b + 1];
          for (uint32_t j = starts[b]; j < e; j++) m |= pair_mask(P, px, py, pz, ux, uy, uz, spos, sdir, j);
        }
  }
  out[i] = m;
}

#define VOTE_EMPTY64 0xFFFFFFFFFFFFFFFFull

// one workgroup per A strand s (its points a_pts[offsets[s] .. offsets[s+1]), strand order).  LDS: the (point, B strand) set
// (keys, pair masks) and the B strand count table, `cap` entries each (a power of two).  A count slot is one 64-bit word,
// the B strand number above its count, claimed as (number, 0): every bit pattern of a strand number is a key, and an empty
// slot is told apart by its count bits, all ones, which no count (<= cap) reaches.
__global__ __launch_bounds__(MT_BLOCK) void strand_votes_kernel(int S, MatchParams P, const double* __restrict__ a_pts,
                                                                const double* __restrict__ a_dirs, const long long* __restrict__ offsets,
                                                                const int* __restrict__ b_strand, const uint32_t* __restrict__ starts,
                                                                const double* __restrict__ spos, const double* __restrict__ sdir,
                                                                const int* __restrict__ sidx, int cap, int* __restrict__ best,
                                                                int* __restrict__ overflow, int* __restrict__ n_overflow) {
  extern __shared__ unsigned long long lds_words[];
  unsigned long long* set_key = lds_words;
  unsigned long long* cnt = set_key + cap;
  uint32_t* set_val = (uint32_t*)(cnt + cap);
  __shared__ int s_flag, s_max;
  const int s = blockIdx.x;
  const long long p0 = offsets[s], n = offsets[s + 1] - p0;
  for (int t = threadIdx.x; t < cap; t += MT_BLOCK) { set_key[t] = VOTE_EMPTY64; set_val[t] = 0u; }
  if (threadIdx.x == 0) { s_flag = 0; s_max = 0; }
  __syncthreads();
  const uint32_t cmask = (uint32_t)cap - 1u;
  // work items: (point, neighbour cell) pairs of the strand
  for (long long w = threadIdx.x; w < n * 27 && !s_flag; w += MT_BLOCK) {
    const long long li = w / 27;
    const int o = (int)(w - li * 27);
    const size_t i = (size_t)(p0 + li);
    const double px = a_pts[3 * i], py = a_pts[3 * i + 1], pz = a_pts[3 * i + 2];
    int cx, cy, cz;
    if (!(query_cell(px, P.lo[0], P.h, P.dims[0], &cx) && query_cell(py, P.lo[1], P.h, P.dims[1], &cy) &&
          query_cell(pz, P.lo[2], P.h, P.dims[2], &cz)))
      continue;
    cx += o / 9 - 1; cy += (o / 3) % 3 - 1; cz += o % 3 - 1;
    if (cx < 0 || cy < 0 || cz < 0 || cx >= P.dims[0] || cy >= P.dims[1] || cz >= P.dims[2]) continue;
    const double ux = a_dirs[3 * i], uy = a_dirs[3 * i + 1], uz = a_dirs[3 * i + 2];
    const uint32_t b = cell_bucket(cx, cy, cz, P.table_mask);
    const uint32_t e = starts[b + 1];
    for (uint32_t j = starts[b]; j < e; j++) {
      const uint32_t m = pair_mask(P, px, py, pz, ux, uy, uz, spos, sdir, j);
      if (!m) continue;
      const unsigned long long key = ((unsigned long long)li << 32) | (uint32_t)b_strand[sidx[j]];
      uint32_t slot = (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 32) & cmask;
      int probes = 0;
      for (; probes < cap; probes++, slot = (slot + 1) & cmask) {
        const unsigned long long prev = atomicCAS(&set_key[slot], VOTE_EMPTY64, key);
        if (prev == VOTE_EMPTY64 || prev == key) break;
      }
      if (probes == cap) { s_flag = 1; break; }
      atomicOr(&set_val[slot], m);
    }
  }
  __syncthreads();
  if (s_flag) {                      // the set did not fit: the caller counts this strand itself
    if (threadIdx.x == 0) overflow[atomicAdd(n_overflow, 1)] = s;
    return;
  }
  for (int k = 0; k < P.K; k++) {
    for (int t = threadIdx.x; t < cap; t += MT_BLOCK) cnt[t] = VOTE_EMPTY64;
    __syncthreads();
    for (int t = threadIdx.x; t < cap; t += MT_BLOCK) {
      const unsigned long long key = set_key[t];
      if (key == VOTE_EMPTY64 || !((set_val[t] >> k) & 1u)) continue;
      const uint32_t bs = (uint32_t)key;
      uint32_t slot = (bs * 0x9E3779B1u) & cmask;   // distinct B strands <= set entries <= cap: always finds a slot
      for (;; slot = (slot + 1) & cmask) {
        const unsigned long long prev = atomicCAS(&cnt[slot], VOTE_EMPTY64, (unsigned long long)bs << 32);
        if (prev == VOTE_EMPTY64 || (uint32_t)(prev >> 32) == bs) break;
      }
      atomicAdd(&cnt[slot], 1ull);                  // (the count is the low word: at most cap, no carry into the number)
    }
    __syncthreads();
    int mx = 0;
    for (int t = threadIdx.x; t < cap; t += MT_BLOCK)
      if (cnt[t] != VOTE_EMPTY64) mx = max(mx, (int)(uint32_t)cnt[t]);
    atomicMax(&s_max, mx);
    __syncthreads();
    if (threadIdx.x == 0) { best[(size_t)k * S + s] = s_max; s_max = 0; }
    __syncthreads();
  }
}

int match_params(const char* who, int nB, int K, const double* thresholds_host, int bidirectional, const double* box_host, MatchParams* P) {
  if (K < 1 || K > HGS_METRICS_MAX_K || !thresholds_host || !box_host) {
    hgs_set_error("%s: need 1 <= K <= %d threshold pairs and a box", who, HGS_METRICS_MAX_K);
    return 1;
  }
  double rmax = 0.0;
  for (int k = 0; k < K; k++) {
    const double r = thresholds_host[2 * k];
    if (!(r > 0.0) || !(r < __builtin_inf())) { hgs_set_error("%s: radius %d is %g, must be positive and finite", who, k, r); return 1; }
    P->r2[k] = r * r;
    P->cs[k] = thresholds_host[2 * k + 1];
    rmax = r > rmax ? r : rmax;
  }
  P->K = K;
  P->bidirectional = bidirectional != 0;
  P->r2max = rmax * rmax;   // (the largest r_k*r_k)
  P->h = rmax * (1.0 + 1e-6);
  for (int a = 0; a < 3; a++) {
    const double lo = box_host[a], hi = box_host[3 + a];
    const double cells = floor((hi - lo) / P->h) + 1.0;
    if (!(lo <= hi) || !(cells <= (double)HGS_METRICS_MAX_CELLS)) {
      hgs_set_error("%s: the box [%g, %g] of axis %d needs %g cells of %g (at most 2^21 per axis)", who, lo, hi, a, cells, P->h);
      return 1;
    }
    P->lo[a] = lo;
    P->dims[a] = (int)cells;
  }
  P->table_mask = (uint32_t)(match_table(nB) - 1);
  return 0;
}

}  // namespace

extern "C" size_t hgs_oriented_match_scratch_bytes(int nB) { return match_layout(nB < 0 ? 0 : nB, nullptr, nullptr); }

extern "C" int hgs_oriented_match(void* stream, int nA, int nB, int K, const double* a_pts, const double* a_dirs, const double* b_pts,
                                  const double* b_dirs, const double* thresholds_host, int bidirectional, const double* box_host,
                                  uint32_t* mask, void* scratch, size_t scratch_bytes) {
  if (nA < 0 || nB < 0) { hgs_set_error("hgs_oriented_match: bad sizes"); return 1; }
  if (nA == 0) return 0;
  if (!a_pts || !a_dirs || !mask) { hgs_set_error("hgs_oriented_match: null argument"); return 1; }
  hipStream_t st = (hipStream_t)stream;
  if (nB == 0) { return hgs_zero_async(st, mask, 4 * (size_t)nA); }
  if (!b_pts || !b_dirs || !scratch || ((uintptr_t)scratch % HGS_ALIGN) || scratch_bytes < hgs_oriented_match_scratch_bytes(nB)) {
    hgs_set_error("hgs_oriented_match: B arrays and a %d-byte aligned scratch of >= %zu bytes are required (got %zu)", HGS_ALIGN,
                  hgs_oriented_match_scratch_bytes(nB), scratch_bytes);
    return 1;
  }
  MatchParams P;
  if (match_params("hgs_oriented_match", nB, K, thresholds_host, bidirectional, box_host, &P)) return 1;
  MatchScratch s;
  match_layout(nB, (char*)scratch, &s);
  const uint32_t T = P.table_mask + 1;
  if (hgs_zero_async(st, s.starts, 4 * ((size_t)T + 1)) || hgs_zero_async(st, s.cursor, 4 * (size_t)T)) return 1;
  hipLaunchKernelGGL(bucket_count_kernel, dim3((nB + MT_BLOCK - 1) / MT_BLOCK), dim3(MT_BLOCK), 0, st, nB, P, b_pts, s.bucket, s.starts);
  HGS_CHECK_LAUNCH();
  hipLaunchKernelGGL(scan_local_kernel, dim3(T / SCAN_CHUNK), dim3(MT_BLOCK), 0, st, s.starts, s.block_tot);
  HGS_CHECK_LAUNCH();
  hipLaunchKernelGGL(scan_top_kernel, dim3(1), dim3(MT_BLOCK), 0, st, (int)(T / SCAN_CHUNK), s.block_tot, s.starts + T);
  HGS_CHECK_LAUNCH();
  hipLaunchKernelGGL(scan_add_kernel, dim3((T + MT_BLOCK - 1) / MT_BLOCK), dim3(MT_BLOCK), 0, st, T, s.starts, s.block_tot);
  HGS_CHECK_LAUNCH();
  hipLaunchKernelGGL(bucket_scatter_kernel, dim3((nB + MT_BLOCK - 1) / MT_BLOCK), dim3(MT_BLOCK), 0, st, nB, b_pts, b_dirs, s.bucket,
                     s.starts, s.cursor, s.spos, s.sdir, s.sidx);
  HGS_CHECK_LAUNCH();
  hipLaunchKernelGGL(oriented_match_kernel, dim3((nA + MT_BLOCK - 1) / MT_BLOCK), dim3(MT_BLOCK), 0, st, nA, P, a_pts, a_dirs, s.starts,
                     s.spos, s.sdir, mask);
  HGS_CHECK_LAUNCH();
  return 0;
}

extern "C" int hgs_strand_votes(void* stream, int S, int nB, int K, const double* a_pts, const double* a_dirs, const long long* offsets,
                                const int* b_strand, const double* thresholds_host, int bidirectional, const double* box_host,
                                const void* scratch, int capacity, int* best, int* overflow, int* n_overflow) {
  if (S < 0 || nB < 0) { hgs_set_error("hgs_strand_votes: bad sizes"); return 1; }
  if (S == 0) return 0;
  if (!a_pts || !a_dirs || !offsets || !best || !overflow || !n_overflow) { hgs_set_error("hgs_strand_votes: null argument"); return 1; }
  if (capacity < 1 || capacity > HGS_VOTE_MAX_CAPACITY || (capacity & (capacity - 1))) {
    hgs_set_error("hgs_strand_votes: capacity %d must be a power of two in [1, %d]", capacity, HGS_VOTE_MAX_CAPACITY);
    return 1;
  }
  hipStream_t st = (hipStream_t)stream;
  if (nB == 0) { return hgs_zero_async(st, best, 4 * (size_t)K * S); }
  if (!b_strand || !scratch || ((uintptr_t)scratch % HGS_ALIGN)) { hgs_set_error("hgs_strand_votes: B strand ids and the match scratch are required"); return 1; }
  MatchParams P;
  if (match_params("hgs_strand_votes", nB, K, thresholds_host, bidirectional, box_host, &P)) return 1;
  MatchScratch s;
  match_layout(nB, (char*)scratch, &s);
  hipLaunchKernelGGL(strand_votes_kernel, dim3(S), dim3(MT_BLOCK), (size_t)capacity * 20, st, S, P, a_pts, a_dirs, offsets, b_strand,
                     s.starts, s.spos, s.sdir, s.sidx, capacity, best, overflow, n_overflow);
  HGS_CHECK_LAUNCH();
  return 0;
}
