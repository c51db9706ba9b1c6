// hgs_magnet.hip -- the magnet term of Stage III (loss/losses.py strand_joints_magnet_loss, reference loss/losses.py:106-172) as a
// device op: value and gradient, stream-only, capturable.
//
// Every quantity that moves between two topology events lives in device memory: which ends are valid (their own segment is
// longer than min_val), their rank in the compacted list the neighbour indices refer to, the three nearest of each, the
// selection, the rows of the mean.  The launch shapes depend on n (strand ends) and E (endpoints) only.
//
//   forward   flag -> compact (rank = exclusive scan of the flags; the valid ends' bounding box by integer atomics)
//             search, one of two paths with ONE result -- the three smallest (distance, position) pairs of every end, itself included,
//             distance = dx*dx + dy*dy + dz*dz in float32 without contraction (bit-equal to hgs_knn3 on the same points):
//               tiles  one query per lane, candidates staged through LDS as float4 (one broadcast 16-byte read each); for small n
//                      the candidate range is split over workgroups and the partial triples are merged in the same order
//               grid   the grid of Morton cells of hgs_cellgrid.h, which distCUDA2 searches too (keys -> keysort_launch -> cell
//                      table -> own cell, then the cells the third-best radius reaches); here positions are kept and break ties
//             select (statements (c)-(e) of include/hgs.h, per-workgroup float64 partial sums) -> finalize (value, rows)
//   backward  no float atomics: keys (selected position << 32 | own position) of the kept rows -> keysort_launch -> one lane per
//             destination sums its contributors in ascending order -> one store per end.  Same bits from run to run and under
//             either search path.  The sum of a destination is ONE lane's serial walk of its run: a strand end is selected by
//             a handful of ends at most, but nothing bounds it -- n coincident ends all select one of three positions, and
//             that lane then takes O(n) steps (correct and deterministic, slow; a cooperative sum in a fixed tree would bound
//             it and is not built).
#include <limits.h>

#include "hgs_common.h"
#include "hgs_cellgrid.h"

namespace {

#ifndef HGS_MAGNET_GRID_MIN
// automatic mode: the grid from this many ends on.  Measured on an MI355X: forward at 2 10^4 ends 0.36 ms
// through the tiles and 0.41 ms through the grid, at 2 10^5 ends 16.9 against 1.00 ms; the tiles grow with n^2, the grid with
// the sort's launches, and the two lines cross near 2.2 10^4.
#define HGS_MAGNET_GRID_MIN 22528
#endif

int g_magnet_search = -1;   // hgs_set_magnet_search

struct MagScratch {
  int* counts;          // [0] valid ends, [1] rows of the mean, [2..7] order-preserving keys of the valid finite ends' bounding box
  int* blk_count;       // valid ends per workgroup of 256 ends
  float4* cpts;         // the compacted list: position -> coordinates
  int2* cmeta;          // position -> (index into `ends`, partner's global id)
  Best3* part;          // [splits][n] partial triples (tiles), [n] triples (grid)
  uint64_t* keys;       // Npad sort keys (forward: Morton code << 32 | position; backward: selected << 32 | own)
  float4* sorted;       // grid: the valid ends in Morton order (w = position)
  uint32_t* cells;      // grid: 8 words per cell
  double* blk_sum;      // select: per-workgroup sum of the kept rows' squared squared distances
  int* blk_rows;        //         and their number
  float* nbsum;         // backward: per position the sum of its contributors' gradients
};

static int mag_splits(int n) {            // tiles: workgroups per block of queries, so that a few thousand ends still fill the chip
  const int qb = (n + 255) / 256;
  int S = 512 / (qb > 0 ? qb : 1);
  if (S > qb) S = qb;
  return S < 1 ? 1 : S;
}
static bool mag_use_grid(int n) { return g_magnet_search < 0 ? n >= HGS_MAGNET_GRID_MIN : g_magnet_search == 1; }

size_t mag_carve(char* base, size_t n, MagScratch& s) {      // (every array is per end: the size does not depend on E)
  char* cur = base;
  const size_t nb = (n + 255) / 256, Npad = pad_pow2(n);
  hgs_carve(cur, s.counts, 16);
  hgs_carve(cur, s.blk_count, nb + 1);
  hgs_carve(cur, s.cpts, n + 1);
  hgs_carve(cur, s.cmeta, n + 1);
  hgs_carve(cur, s.part, (size_t)mag_splits((int)n) * n + 1);
  hgs_carve(cur, s.keys, Npad);
  hgs_carve(cur, s.sorted, n + 1);
  hgs_carve(cur, s.cells, 8 * ((size_t)1 << (3 * cellgrid_level(n))));
  hgs_carve(cur, s.blk_sum, nb + 1);
  hgs_carve(cur, s.blk_rows, nb + 1);
  hgs_carve(cur, s.nbsum, 3 * n + 1);
  return hgs_align_up((size_t)(cur - base)) + HGS_ALIGN;
}

// (a): is end i's own segment longer than min_val?  (ids outside the table: not valid -- nothing is read through them)
__device__ __forceinline__ bool mag_valid(int i, int n, int E, const float* __restrict__ ep, const int* __restrict__ ends,
                                          const int* __restrict__ partner, float min_val, float4* p) {
  if (i >= n) return false;
  const int e = ends[i], c = partner[i];
  if (e < 0 || e >= E || c < 0 || c >= E) return false;
  const float x = ep[3 * (size_t)e], y = ep[3 * (size_t)e + 1], z = ep[3 * (size_t)e + 2];
  const float dx = x - ep[3 * (size_t)c], dy = y - ep[3 * (size_t)c + 1], dz = z - ep[3 * (size_t)c + 2];
  *p = make_float4(x, y, z, 0.f);
  return sqrtf(dx * dx + dy * dy + dz * dz) > min_val;
}

__global__ __launch_bounds__(256) void mag_flag_kernel(int n, int E, const float* __restrict__ ep, const int* __restrict__ ends,
                                                       const int* __restrict__ partner, float min_val, int* __restrict__ blk_count,
                                                       int* __restrict__ counts) {
  float4 p;
  const bool v = mag_valid(blockIdx.x * 256 + threadIdx.x, n, E, ep, ends, partner, min_val, &p);
  const int c = __syncthreads_count(v);
  if (threadIdx.x == 0) blk_count[blockIdx.x] = c;
  if (blockIdx.x == 0 && threadIdx.x < 6) counts[2 + threadIdx.x] = threadIdx.x < 3 ? INT_MAX : INT_MIN;
}

__global__ __launch_bounds__(256) void mag_compact_kernel(int n, int E, const float* __restrict__ ep, const int* __restrict__ ends,
                                                          const int* __restrict__ partner, float min_val,
                                                          const int* __restrict__ blk_count, int* __restrict__ counts,
                                                          float4* __restrict__ cpts, int2* __restrict__ cmeta) {
  __shared__ int red[4], wtot[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int part = 0;                                        // valid ends in front of this workgroup (integers: any order)
  for (int j = threadIdx.x; j < (int)blockIdx.x; j += 256) part += blk_count[j];
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) part += __shfl_xor(part, d, 64);
  const int i = blockIdx.x * 256 + threadIdx.x;
  float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
  const bool v = mag_valid(i, n, E, ep, ends, partner, min_val, &p);
  const unsigned long long m = __ballot(v);
  if (lane == 0) { red[wave] = part; wtot[wave] = __popcll(m); }
  __syncthreads();
  int rank = red[0] + red[1] + red[2] + red[3] + __popcll(m & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; w++) rank += wtot[w];
  if (v && rank < n) {
    cpts[rank] = p;
    cmeta[rank] = make_int2(i, partner[i]);
  }
  // the valid finite ends' bounding box: min / max of the order-preserving keys over the wavefront first, then one atomic per
  // wavefront and word (integers: exact in any order)
  const bool boxed = v && rank < n && isfinite(p.x) && isfinite(p.y) && isfinite(p.z);
  int lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {INT_MIN, INT_MIN, INT_MIN};
  if (boxed) {
    lo[0] = hi[0] = fkey(p.x); lo[1] = hi[1] = fkey(p.y); lo[2] = hi[2] = fkey(p.z);
  }
  if (__ballot(boxed)) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) {
        lo[k] = min(lo[k], __shfl_xor(lo[k], d, 64));
        hi[k] = max(hi[k], __shfl_xor(hi[k], d, 64));
      }
    }
    if (lane == 0) {
      atomicMin(&counts[2], lo[0]); atomicMin(&counts[3], lo[1]); atomicMin(&counts[4], lo[2]);
      atomicMax(&counts[5], hi[0]); atomicMax(&counts[6], hi[1]); atomicMax(&counts[7], hi[2]);
    }
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) counts[0] = red[0] + red[1] + red[2] + red[3] + wtot[0] + wtot[1] + wtot[2] + wtot[3];
}

// insert by (distance, position): what a walk in ascending position order gets from `d < b2` alone (knn3_kernel)
__device__ __forceinline__ void mag_insert(Best3& b, float d, int pos) {
  if (d < b.d[2] || (d == b.d[2] && pos < b.i[2])) {
    if (d < b.d[1] || (d == b.d[1] && pos < b.i[1])) {
      b.d[2] = b.d[1]; b.i[2] = b.i[1];
      if (d < b.d[0] || (d == b.d[0] && pos < b.i[0])) { b.d[1] = b.d[0]; b.i[1] = b.i[0]; b.d[0] = d; b.i[0] = pos; }
      else { b.d[1] = d; b.i[1] = pos; }
    } else { b.d[2] = d; b.i[2] = pos; }
  }
}

// ---- tiles: blockIdx.x = 256 queries, blockIdx.y = its share [y * chunk, (y + 1) * chunk) of the candidates
__global__ __launch_bounds__(256) void mag_tiles_kernel(int n, int chunk, const int* __restrict__ counts,
                                                        const float4* __restrict__ cpts, Best3* __restrict__ part) {
  __shared__ float4 sp[256];
  const int nv = min(counts[0], n);
  if ((int)blockIdx.x * 256 >= nv) return;
  const int a = blockIdx.x * 256 + threadIdx.x;
  const float4 me = a < nv ? cpts[a] : make_float4(0.f, 0.f, 0.f, 0.f);
  const int t_begin = min((int)blockIdx.y * chunk, nv), t_end = min(t_begin + chunk, nv);
  Best3 b;
  best3_clear(b);
  for (int t0 = t_begin; t0 < t_end; t0 += 256) {
    const int j = t0 + threadIdx.x;
    __syncthreads();
    if (j < t_end) sp[threadIdx.x] = cpts[j];
    __syncthreads();
    const int nbc = min(256, t_end - t0);
    for (int k = 0; k < nbc; k++) best3_push(b, point_dist2(me, sp[k]), t0, k);   // one broadcast 16-byte LDS read per candidate
  }
  if (a < nv) part[(size_t)blockIdx.y * n + a] = b;
}

// ---- grid (hgs_cellgrid.h)
// the magnet as a source of the grid: min(counts[0], n) valid ends, counted on the device (the op is captured in a graph); their
// bounding box in counts[2..7] as order-preserving keys; an end with a non-finite coordinate is in no cell
struct MagSource {
  const int* __restrict__ counts;
  static constexpr bool kGuarded = true;
  __device__ __forceinline__ int live(int n) const { return min(counts[0], n); }
  __device__ __forceinline__ void load_box(float* box) const {
    if (threadIdx.x < 6) box[threadIdx.x] = funkey(counts[2 + threadIdx.x]);
    __syncthreads();
  }
};

// the three smallest (distance, position) pairs, the end itself among them: mag_insert makes the triple independent of the traversal
struct MagBest : Best3 {
  typedef Best3 Out;          // part[position] = the triple
  static constexpr bool kSelf = true, kGuarded = true;
  __device__ __forceinline__ void clear() { best3_clear(*this); }
  __device__ __forceinline__ float third() const { return d[2]; }
  __device__ __forceinline__ void add(float dist, uint32_t pos) { mag_insert(*this, dist, (int)pos); }
  __device__ __forceinline__ void store(Best3* __restrict__ part, const float4& me) const { part[__float_as_uint(me.w)] = *this; }
};

// ---- select: merge the partial triples, statements (c)-(e), per-workgroup sums of the mean
__global__ __launch_bounds__(256) void mag_select_kernel(int n, int E, int S, const int* __restrict__ counts,
                                                         const int2* __restrict__ cmeta, const Best3* __restrict__ part,
                                                         const float* __restrict__ ep, const int* __restrict__ mapping, float min_val,
                                                         int* __restrict__ sel, float* __restrict__ sq, int* __restrict__ nn_idx,
                                                         float* __restrict__ nn_d2, double* __restrict__ blk_sum,
                                                         int* __restrict__ blk_rows) {
  __shared__ double ssum[256];
  __shared__ int srows[256];
  const int nv = min(counts[0], n);
  const int a = blockIdx.x * 256 + threadIdx.x;
  double contrib = 0.0;
  int kept = 0;
  if (a < n) {
    Best3 t;
    best3_clear(t);
    int chosen = -1, eidx = -1;
    float s = 0.f;
    if (a < nv) {
      for (int y = 0; y < S; y++) {
        const Best3 p = part[(size_t)y * n + a];
#pragma unroll
        for (int j = 0; j < 3; j++)
          if (p.i[j] >= 0 && p.i[j] < nv) mag_insert(t, p.d[j], p.i[j]);
      }
      const int2 meta = cmeta[a];
      eidx = meta.x;
      const bool found = t.i[0] >= 0 && t.i[1] >= 0 && t.i[2] >= 0;                     // (e)
      const int n1 = max(t.i[1], 0), n2 = max(t.i[2], 0);
      const bool second_ok = n1 != a && n1 != meta.y;                                 // (c): position against the partner's GLOBAL id
      const int q = second_ok ? n1 : n2;
      s = second_ok ? t.d[1] : t.d[2];
      bool ok = found && isfinite(s);
      if (ok) {                                                                       // (d): the position as a global id
        ok = false;
        if (q < E) {
          const int mp = mapping[q];
          if (mp >= 0 && mp < E) {
            const float dx = ep[3 * (size_t)q] - ep[3 * (size_t)mp], dy = ep[3 * (size_t)q + 1] - ep[3 * (size_t)mp + 1],
                        dz = ep[3 * (size_t)q + 2] - ep[3 * (size_t)mp + 2];
            ok = sqrtf(dx * dx + dy * dy + dz * dz) > min_val;
          }
        }
      }
      if (ok) { chosen = q; kept = 1; contrib = (double)(s * s); }                    // (f): the squared squared distance, in float32
    }
    sel[2 * (size_t)a] = chosen;
    sel[2 * (size_t)a + 1] = eidx;
    sq[a] = kept ? s : 0.f;
#pragma unroll
    for (int j = 0; j < 3; j++) { nn_idx[3 * (size_t)a + j] = t.i[j]; nn_d2[3 * (size_t)a + j] = t.d[j]; }
  }
  ssum[threadIdx.x] = contrib;
  srows[threadIdx.x] = kept;
  __syncthreads();
  for (int d = 128; d >= 1; d >>= 1) {                 // a fixed tree: the same bits every run
    if ((int)threadIdx.x < d) { ssum[threadIdx.x] += ssum[threadIdx.x + d]; srows[threadIdx.x] += srows[threadIdx.x + d]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { blk_sum[blockIdx.x] = ssum[0]; blk_rows[blockIdx.x] = srows[0]; }
}

// out[0] = the value, out[1] = the rows of the mean, out[2] = the valid ends (both as int32 bits)
__global__ __launch_bounds__(256) void mag_finalize_kernel(int nb, int n, const double* __restrict__ blk_sum, const int* __restrict__ blk_rows,
                                                           int* __restrict__ counts, float* __restrict__ out) {
  __shared__ double ssum[256];
  __shared__ int srows[256];
  double acc = 0.0;
  int rows = 0;
  for (int j = threadIdx.x; j < nb; j += 256) { acc += blk_sum[j]; rows += blk_rows[j]; }
  ssum[threadIdx.x] = acc;
  srows[threadIdx.x] = rows;
  __syncthreads();
  for (int d = 128; d >= 1; d >>= 1) {
    if ((int)threadIdx.x < d) { ssum[threadIdx.x] += ssum[threadIdx.x + d]; srows[threadIdx.x] += srows[threadIdx.x + d]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const int m = srows[0];
    out[0] = m > 0 ? (float)(ssum[0] / (double)m) : 0.f;
    out[1] = __int_as_float(m);
    out[2] = __int_as_float(nb > 0 ? min(counts[0], n) : 0);
    out[3] = 0.f;
    counts[1] = m;
  }
}

// ---- backward
// (g): row a's gradient to its own end, 4 s (p - q) / m times the upstream gradient; its neighbour gets the opposite
__device__ __forceinline__ bool mag_row_grad(int a, int n, int E, const float* __restrict__ ep, const int* __restrict__ ends,
                                             const int* __restrict__ sel, const float* __restrict__ sq, float coef, float* g) {
  const int q = sel[2 * (size_t)a];
  if (q < 0 || q >= n) return false;
  const int ea = sel[2 * (size_t)a + 1], eq = sel[2 * (size_t)q + 1];
  if (ea < 0 || ea >= n || eq < 0 || eq >= n) return false;
  const int ia = ends[ea], iq = ends[eq];
  if (ia < 0 || ia >= E || iq < 0 || iq >= E) return false;
  const float gs = 4.f * (coef * sq[a]);
#pragma unroll
  for (int c = 0; c < 3; c++) g[c] = gs * (ep[3 * (size_t)ia + c] - ep[3 * (size_t)iq + c]);
  return true;
}
__device__ __forceinline__ float mag_coef(const float* __restrict__ out, const float* __restrict__ grad_out, float weight) {
  const int m = __float_as_int(out[1]);
  return m > 0 ? (grad_out[0] * weight) / (float)m : 0.f;
}

__global__ __launch_bounds__(256) void mag_bwd_keys_kernel(int n, int Npad, const int* __restrict__ sel, uint64_t* __restrict__ keys,
                                                           float* __restrict__ nbsum) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= Npad) return;
  uint64_t k = ~0ull;
  if (i < n) {
    const int q = sel[2 * (size_t)i];
    if (q >= 0 && q < n) k = ((uint64_t)(uint32_t)q << 32) | (uint32_t)i;
    nbsum[3 * (size_t)i] = nbsum[3 * (size_t)i + 1] = nbsum[3 * (size_t)i + 2] = 0.f;
  }
  keys[i] = k;
}

// one lane per sorted key; the lane of a destination's first key sums the run -- ascending contributing position
__global__ __launch_bounds__(256) void mag_bwd_runs_kernel(int n, int E, const float* __restrict__ ep, const int* __restrict__ ends,
                                                           const int* __restrict__ sel, const float* __restrict__ sq,
                                                           const float* __restrict__ out, const float* __restrict__ grad_out,
                                                           float weight, const uint64_t* __restrict__ keys, float* __restrict__ nbsum) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint64_t k = keys[i];
  if (k == ~0ull) return;
  const uint32_t q = (uint32_t)(k >> 32);
  if (q >= (uint32_t)n) return;
  if (i > 0 && (uint32_t)(keys[i - 1] >> 32) == q) return;
  const float coef = mag_coef(out, grad_out, weight);
  float acc[3] = {0.f, 0.f, 0.f};
  for (int j = i; j < n; j++) {
    const uint64_t kj = keys[j];
    if ((uint32_t)(kj >> 32) != q) break;
    const uint32_t a = (uint32_t)kj;
    float g[3];
    if (a < (uint32_t)n && mag_row_grad((int)a, n, E, ep, ends, sel, sq, coef, g)) {
      acc[0] -= g[0]; acc[1] -= g[1]; acc[2] -= g[2];
    }
  }
  nbsum[3 * (size_t)q] = acc[0]; nbsum[3 * (size_t)q + 1] = acc[1]; nbsum[3 * (size_t)q + 2] = acc[2];
}

__global__ __launch_bounds__(256) void mag_bwd_store_kernel(int n, int E, const float* __restrict__ ep, const int* __restrict__ ends,
                                                            const int* __restrict__ sel, const float* __restrict__ sq,
                                                            const float* __restrict__ out, const float* __restrict__ grad_out,
                                                            float weight, const float* __restrict__ nbsum, float* __restrict__ d_ep) {
  const int a = blockIdx.x * 256 + threadIdx.x;
  if (a >= n) return;
  const int ea = sel[2 * (size_t)a + 1];
  if (ea < 0 || ea >= n) return;                       // behind the valid ends
  const int ia = ends[ea];
  if (ia < 0 || ia >= E) return;
  float g[3] = {0.f, 0.f, 0.f};
  if (!mag_row_grad(a, n, E, ep, ends, sel, sq, mag_coef(out, grad_out, weight), g)) g[0] = g[1] = g[2] = 0.f;
#pragma unroll
  for (int c = 0; c < 3; c++) d_ep[3 * (size_t)ia + c] = g[c] + nbsum[3 * (size_t)a + c];   // (every end is one endpoint: no two lanes share a destination)
}

}  // namespace

extern "C" int hgs_set_magnet_search(int mode) {
  const int was = g_magnet_search;
  g_magnet_search = mode < 0 ? -1 : (mode ? 1 : 0);
  return was;
}

extern "C" size_t hgs_magnet_scratch_bytes(int n_ends, int n_endpoints) {
  if (n_ends < 0 || n_endpoints < 0) return 0;
  MagScratch s;
  return mag_carve(nullptr, (size_t)n_ends, s);
}

extern "C" int hgs_magnet_forward(void* stream, int E, int n, const float* endpoints, const int* ends, const int* partner,
                                  const int* mapping, float min_val, void* scratch, size_t scratch_bytes, float* out, int* sel,
                                  float* sq, int* nn_idx, float* nn_d2) {
  if (E < 0 || n < 0 || n > E) { hgs_set_error("hgs_magnet_forward: bad sizes (E = %d, n = %d)", E, n); return 1; }
  if (!out || !scratch || (n > 0 && (!endpoints || !ends || !partner || !mapping || !sel || !sq || !nn_idx || !nn_d2))) {
    hgs_set_error("hgs_magnet_forward: null argument"); return 1;
  }
  if (hgs_magnet_scratch_bytes(n, E) > scratch_bytes || ((size_t)scratch & (HGS_ALIGN - 1))) {
    hgs_set_error("hgs_magnet_forward: scratch must be %d-byte aligned and >= %zu bytes (got %zu)", HGS_ALIGN,
                  hgs_magnet_scratch_bytes(n, E), scratch_bytes);
    return 1;
  }
  hipStream_t st = (hipStream_t)stream;
  MagScratch s;
  mag_carve((char*)scratch, (size_t)n, s);
  const int nb = (n + 255) / 256;
  HgsProfScope _prof(st, HGS_K_KNN);
  if (n > 0) {
    hipLaunchKernelGGL(mag_flag_kernel, dim3(nb), dim3(256), 0, st, n, E, endpoints, ends, partner, min_val, s.blk_count, s.counts);
    hipLaunchKernelGGL(mag_compact_kernel, dim3(nb), dim3(256), 0, st, n, E, endpoints, ends, partner, min_val, s.blk_count, s.counts,
                       s.cpts, s.cmeta);
    int S = 1;
    if (mag_use_grid(n)) {
      const size_t Npad = pad_pow2((size_t)n);
      const int L = cellgrid_level((size_t)n);
      const unsigned n_cells = 1u << (3 * L);
      const MagSource src{s.counts};
      hipLaunchKernelGGL((cellgrid_keys_kernel<MagSource, float4>), dim3((unsigned)((Npad + 255) / 256)), dim3(256), 0, st, src, n, (int)Npad, s.cpts, s.keys);
      keysort_launch(st, s.keys, Npad);
      hipLaunchKernelGGL((cellgrid_gather_kernel<MagSource, float4>), dim3(nb), dim3(256), 0, st, src, n, s.cpts, s.keys, s.sorted);
      hipLaunchKernelGGL(cells_clear_kernel, dim3((n_cells + 255) / 256), dim3(256), 0, st, n_cells, s.cells);
      hipLaunchKernelGGL(cellgrid_mark_kernel<MagSource>, dim3(nb), dim3(256), 0, st, src, n, 30 - 3 * L, s.keys, s.sorted, s.cells);
      hipLaunchKernelGGL((cellgrid_search_kernel<MagSource, MagBest>), dim3(nb), dim3(256), 0, st, n, L, src, s.sorted, s.keys, s.cells, s.part);
    } else {
      S = mag_splits(n);
      const int chunk = ((nb + S - 1) / S) * 256;
      hipLaunchKernelGGL(mag_tiles_kernel, dim3(nb, S), dim3(256), 0, st, n, chunk, s.counts, s.cpts, s.part);
    }
    hipLaunchKernelGGL(mag_select_kernel, dim3(nb), dim3(256), 0, st, n, E, S, s.counts, s.cmeta, s.part, endpoints, mapping, min_val,
                       sel, sq, nn_idx, nn_d2, s.blk_sum, s.blk_rows);
  }
  hipLaunchKernelGGL(mag_finalize_kernel, dim3(1), dim3(256), 0, st, nb, n, s.blk_sum, s.blk_rows, s.counts, out);
  HGS_CHECK_LAUNCH();
  return 0;
}

extern "C" int hgs_magnet_backward(void* stream, int E, int n, const float* endpoints, const int* ends, const int* sel, const float* sq,
                                   const float* out, const float* grad_out, float weight, void* scratch, size_t scratch_bytes,
                                   float* d_endpoints) {
  if (E < 0 || n < 0 || n > E) { hgs_set_error("hgs_magnet_backward: bad sizes (E = %d, n = %d)", E, n); return 1; }
  if (E == 0) return 0;
  if (!d_endpoints || !out || !grad_out || !scratch || (n > 0 && (!endpoints || !ends || !sel || !sq))) {
    hgs_set_error("hgs_magnet_backward: null argument"); return 1;
  }
  if (hgs_magnet_scratch_bytes(n, E) > scratch_bytes || ((size_t)scratch & (HGS_ALIGN - 1))) {
    hgs_set_error("hgs_magnet_backward: scratch must be %d-byte aligned and >= %zu bytes (got %zu)", HGS_ALIGN,
                  hgs_magnet_scratch_bytes(n, E), scratch_bytes);
    return 1;
  }
  hipStream_t st = (hipStream_t)stream;
  MagScratch s;
  mag_carve((char*)scratch, (size_t)n, s);
  HgsProfScope _prof(st, HGS_K_KNN);
  if (hgs_zero_async(st, d_endpoints, sizeof(float) * 3 * (size_t)E)) return 1;
  if (n > 0) {
    const size_t Npad = pad_pow2((size_t)n);
    const int nb = (n + 255) / 256;
    hipLaunchKernelGGL(mag_bwd_keys_kernel, dim3((unsigned)((Npad + 255) / 256)), dim3(256), 0, st, n, (int)Npad, sel, s.keys, s.nbsum);
    keysort_launch(st, s.keys, Npad);
    hipLaunchKernelGGL(mag_bwd_runs_kernel, dim3(nb), dim3(256), 0, st, n, E, endpoints, ends, sel, sq, out, grad_out, weight, s.keys,
                       s.nbsum);
    hipLaunchKernelGGL(mag_bwd_store_kernel, dim3(nb), dim3(256), 0, st, n, E, endpoints, ends, sel, sq, out, grad_out, weight, s.nbsum,
                       d_endpoints);
  }
  HGS_CHECK_LAUNCH();
  return 0;
}
