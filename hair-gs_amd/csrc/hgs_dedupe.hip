// hgs_dedupe.hip -- near-copy strands dropped from an exported groom (hgs_dedupe_count / hgs_dedupe_fill / hgs_dedupe_resolve;
// scene/strand_dedupe.py states the contract, its numpy path and the loop restatement in tests/dedupe_reference.py state the same
// thing).  gfx950, wave64.  Built with -ffp-contract=off: every operation below is rounded once, in the order written.  All
// arithmetic is float64 on the float32 points.
//
// The strands: N strands of M points each (points float32 [N*M][3]).  pair(i, j) holds iff d2_s = (dx*dx + dy*dy) + dz*dz <= tol2
// for every joint s, d = x_i[s] - x_j[s]; a NaN or an infinity makes the comparison false, so such a strand pairs with nothing.
//
// dedupe_search_kernel<FILL> is both passes of the all-pairs search: the count pass (FILL = false) writes how many lower
// neighbours j < i each strand has, the fill pass walks the same pairs again and writes them.  A lane owns ONE strand i with its
// root joint in registers as doubles; a workgroup of 4 wavefronts owns 256 consecutive strands and walks the root joints of the
// strands below its last one in tiles of 256, staged in LDS as doubles (x | y | z rows): every lane of a wavefront reads the same
// LDS address (a broadcast), 3 reads for 8 float64 operations.  Only a pair that passes the root test reads anything else: the tip
// joint next (tips spread most), then joints 1 .. M - 2 in order, from global memory, until one fails.  Every joint is tested
// before a pair is counted; the order of the tests is the path's own business (the conjunction is the contract).
//   A lane meets its j in ascending order, so its list comes out sorted, without atomics, the same bytes on every run.
//   The triangle j < i makes the last workgroup's walk N long and the first's empty: workgroups are numbered from the END of the
//   strands (blockIdx 0 owns the last 256), so that the heavy ones start first and the light ones fill the tail.
//   Even so 10^5 strands are 391 workgroups on 256 CUs, the heaviest of which walks all N roots alone.  Every workgroup's tiles are
//   therefore cut into HGS_DEDUPE_PARTS contiguous parts of ascending j, one workgroup each (blockIdx.y): part c of strand i counts
//   into counts[i*PARTS + c], and because the parts ascend in j, the exclusive prefix sum of the FLATTENED counts is at once every
//   part's place in the list and -- at c = 0 -- the strand's lower_offsets: the lists keep their bytes.  (Measured against the
//   uncut walk and other part counts: DESIGN.md section 8 has the figures.)
// Bounds: a strand is read only for 0 <= i < N with N*M <= n_points (checked on the host); a tile entry is read only for
// base + u < last < N; the fill pass writes lower[pos] only for starts[slot] <= pos < min(starts[slot + 1], n_pairs), slot = i*PARTS + c, -- a list
// that does not match the pairs (another tol, other points) is truncated, never overrun.
//
// dedupe_resolve_kernel is ONE Jacobi round of "keep a strand unless a kept earlier strand pairs with it": a lane owns a strand;
// an UNDECIDED strand whose lower neighbours are all decided in the round's INPUT state becomes DROPPED with kept_by = its smallest
// KEPT lower neighbour, or KEPT with kept_by = itself where it has none, and rounds = the round's number; every other strand's
// state is copied.  The strands still undecided are counted by a ballot per wavefront and one integer atomic add (order-free).
// There are no float atomics in this file.  Entries of a list outside [0, i) and ranges outside [0, n_pairs] are skipped.
#include "hgs_common.h"

#include <math.h>

#define DD_BLOCK 256
#define DD_PARTS HGS_DEDUPE_PARTS
#define DD_TILE 256

namespace {

enum { DD_UNDECIDED = 0, DD_KEPT = 1, DD_DROPPED = 2 };

__device__ __forceinline__ bool dedupe_joint(const float* __restrict__ a, const float* __restrict__ b, double tol2) {
  const double dx = (double)a[0] - (double)b[0], dy = (double)a[1] - (double)b[1], dz = (double)a[2] - (double)b[2];
  return (dx * dx + dy * dy) + dz * dz <= tol2;
}

template <bool FILL>
__global__ __launch_bounds__(DD_BLOCK) void dedupe_search_kernel(int N, int M, const float* __restrict__ points, double tol2,
                                                                 int* __restrict__ counts, const long long* __restrict__ starts,
                                                                 long long n_pairs, int* __restrict__ lower) {
  __shared__ double tx[DD_TILE], ty[DD_TILE], tz[DD_TILE];
  const int b = (int)(gridDim.x - 1u - blockIdx.x);                                 // the heavy workgroups first
  const int c = (int)blockIdx.y;                                                    // the part of the walk, 0 .. DD_PARTS - 1
  const long long first = (long long)b * DD_BLOCK;
  const long long i = first + threadIdx.x;
  const bool live = i < N;
  const long long last = (first + DD_BLOCK < N ? first + DD_BLOCK : (long long)N) - 1;      // the workgroup's last strand (first <= last < N)
  const int tiles = (int)((last + DD_TILE - 1) / DD_TILE);                          // tiles of the j in [0, last)
  const int t0 = (int)(((long long)tiles * c) / DD_PARTS), t1 = (int)(((long long)tiles * (c + 1)) / DD_PARTS);
  const float* const pi = points + 3 * (size_t)(live ? i : 0) * M;
  // (a lane without a strand holds NaNs: it passes no test)
  const double xi = live ? (double)pi[0] : (double)NAN, yi = live ? (double)pi[1] : (double)NAN, zi = live ? (double)pi[2] : (double)NAN;
  long long pos = 0, end = 0;
  if (FILL && live) {
    const long long slot = i * DD_PARTS + c;
    pos = starts[slot];
    end = slot + 1 < (long long)N * DD_PARTS ? starts[slot + 1] : n_pairs;
    if (end > n_pairs) end = n_pairs;
    if (pos < 0 || pos > end) pos = end;
  }
  int cnt = 0;
  for (int t = t0; t < t1; t++) {                                                   // (uniform over the workgroup)
    const long long base = (long long)t * DD_TILE;
    __syncthreads();                                                                // the previous tile has been read
    {
      const long long j = base + threadIdx.x;
      double x = 0.0, y = 0.0, z = 0.0;
      if (j < last) {
        const float* const q = points + 3 * (size_t)j * M;
        x = (double)q[0]; y = (double)q[1]; z = (double)q[2];
      }
      tx[threadIdx.x] = x; ty[threadIdx.x] = y; tz[threadIdx.x] = z;
    }
    __syncthreads();
    const int m = last - base < DD_TILE ? (int)(last - base) : DD_TILE;
    const long long mine = i - base;                                                // the lane's own j end at u < mine
#pragma unroll 4
    for (int u = 0; u < m; u++) {
      const double dx = xi - tx[u], dy = yi - ty[u], dz = zi - tz[u];
      if ((dx * dx + dy * dy) + dz * dz <= tol2 && u < mine) {                      // rare: the rest of the strand, from global memory
        const long long j = base + u;
        const float* const pj = points + 3 * (size_t)j * M;
        bool ok = dedupe_joint(pi + 3 * (size_t)(M - 1), pj + 3 * (size_t)(M - 1), tol2);
        for (int s = 1; ok && s < M - 1; s++) ok = dedupe_joint(pi + 3 * (size_t)s, pj + 3 * (size_t)s, tol2);
        if (ok) {
          if (FILL) {
            if (pos < end) lower[pos] = (int)j;
            pos++;
          }
          cnt++;
        }
      }
    }
  }
  if (!FILL && live) counts[i * DD_PARTS + c] = cnt;
}

__global__ __launch_bounds__(256) void dedupe_resolve_kernel(int N, const long long* __restrict__ offsets, long long n_pairs,
                                                             const int* __restrict__ lower, const unsigned char* __restrict__ state,
                                                             unsigned char* __restrict__ state_out, int round, long long* __restrict__ kept_by,
                                                             int* __restrict__ rounds, int* __restrict__ undecided) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  bool open = false;
  if (i < N) {
    unsigned char s = state[i];
    if (s == DD_UNDECIDED) {
      long long a = offsets[i], b = offsets[i + 1];
      if (a < 0 || b < a || b > n_pairs) { a = 0; b = 0; }                          // (the lists are the caller's duty; a range outside them counts as empty)
      long long kept = -1;
      for (long long q = a; q < b; q++) {
        const long long j = lower[q];
        if (j < 0 || j >= i) continue;
        const unsigned char sj = state[j];
        if (sj == DD_UNDECIDED) { open = true; break; }
        if (sj == DD_KEPT && (kept < 0 || j < kept)) kept = j;
      }
      if (!open) {
        s = kept < 0 ? DD_KEPT : DD_DROPPED;
        kept_by[i] = kept < 0 ? i : kept;
        rounds[i] = round;
      }
    }
    state_out[i] = s;
  }
  const int n = __popcll(__ballot(open));
  if (n > 0 && (threadIdx.x & (HGS_WAVE - 1)) == 0) atomicAdd(undecided, n);
}

int dedupe_check_search(const char* who, int N, int M, long long n_points, double tol) {
  if (N < 0 || n_points < 0) { hgs_set_error("%s: bad sizes (%d strands, %lld points)", who, N, n_points); return 1; }
  if (M < 2) { hgs_set_error("%s: M = %d (at least 2 points per strand)", who, M); return 1; }
  if ((long long)N * M > n_points) {
    hgs_set_error("%s: N M = %lld points for %d strands of %d, the point array holds %lld", who, (long long)N * M, N, M, n_points); return 1;
  }
  if (!(tol >= 0.0) || !isfinite(tol)) { hgs_set_error("%s: tol = %g (finite and >= 0)", who, tol); return 1; }
  return 0;
}

}  // namespace

extern "C" int hgs_dedupe_count(void* stream, int N, int M, long long n_points, const float* points, double tol, int* counts) {
  if (dedupe_check_search("hgs_dedupe_count", N, M, n_points, tol)) return 1;
  if (N == 0) return 0;
  if (!points || !counts) { hgs_set_error("hgs_dedupe_count: null argument"); return 1; }
  if ((const void*)counts == (const void*)points) { hgs_set_error("hgs_dedupe_count: counts must not alias points"); return 1; }
  const double tol2 = tol * tol;                                                    // formed once
  const unsigned blocks = (unsigned)(((long long)N + DD_BLOCK - 1) / DD_BLOCK);
  hipLaunchKernelGGL(dedupe_search_kernel<false>, dim3(blocks, DD_PARTS), dim3(DD_BLOCK), 0, (hipStream_t)stream, N, M, points, tol2,
                     counts, (const long long*)nullptr, 0ll, (int*)nullptr);
  HGS_CHECK_LAUNCH();
  return 0;
}

extern "C" int hgs_dedupe_fill(void* stream, int N, int M, long long n_points, const float* points, double tol,
                               const long long* starts, long long n_pairs, int* lower) {
  if (dedupe_check_search("hgs_dedupe_fill", N, M, n_points, tol)) return 1;
  if (n_pairs < 0) { hgs_set_error("hgs_dedupe_fill: bad sizes (%lld pairs)", n_pairs); return 1; }
  if (N == 0 || n_pairs == 0) return 0;
  if (!points || !starts || !lower) { hgs_set_error("hgs_dedupe_fill: null argument"); return 1; }
  if ((const void*)lower == (const void*)points || (const void*)lower == (const void*)starts || (const void*)starts == (const void*)points) {
    hgs_set_error("hgs_dedupe_fill: lower must not alias points or starts, nor starts points"); return 1;
  }
  const double tol2 = tol * tol;                                                    // formed once
  const unsigned blocks = (unsigned)(((long long)N + DD_BLOCK - 1) / DD_BLOCK);
  hipLaunchKernelGGL(dedupe_search_kernel<true>, dim3(blocks, DD_PARTS), dim3(DD_BLOCK), 0, (hipStream_t)stream, N, M, points, tol2,
                     (int*)nullptr, starts, n_pairs, lower);
  HGS_CHECK_LAUNCH();
  return 0;
}

extern "C" int hgs_dedupe_resolve(void* stream, int N, const long long* lower_offsets, long long n_pairs, const int* lower,
                                  const unsigned char* state, unsigned char* state_out, int round, long long* kept_by, int* rounds,
                                  int* undecided) {
  if (N < 0 || n_pairs < 0) { hgs_set_error("hgs_dedupe_resolve: bad sizes (%d strands, %lld pairs)", N, n_pairs); return 1; }
  if (round < 1) { hgs_set_error("hgs_dedupe_resolve: round = %d (rounds are numbered from 1)", round); return 1; }
  if (N == 0) return 0;
  if (!lower_offsets || !state || !state_out || !kept_by || !rounds || !undecided || (n_pairs > 0 && !lower)) {
    hgs_set_error("hgs_dedupe_resolve: null argument"); return 1;
  }
  const void* const in[] = {lower_offsets, lower, state};
  const void* const out[] = {state_out, kept_by, rounds, undecided};
  for (int a = 0; a < 4; a++) {
    for (int b = 0; b < 3; b++) {
      if (out[a] == in[b]) { hgs_set_error("hgs_dedupe_resolve: an output must not alias an input (state_out is another buffer than state)"); return 1; }
    }
    for (int b = a + 1; b < 4; b++) {
      if (out[a] == out[b]) { hgs_set_error("hgs_dedupe_resolve: the outputs must not alias each other"); return 1; }
    }
  }
  const unsigned blocks = (unsigned)(((long long)N + 255) / 256);
  hipLaunchKernelGGL(dedupe_resolve_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, N, lower_offsets, n_pairs, lower, state, state_out,
                     round, kept_by, rounds, undecided);
  HGS_CHECK_LAUNCH();
  return 0;
}
