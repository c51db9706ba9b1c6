// hgs_chains.hip -- strand chains on the device: ordering the open polylines of the segment table (hgs_strand_walk_ends /
// hgs_strand_walk_fill) and growing the strand tips (hgs_strand_grow_plan / hgs_strand_grow_fill).  Built with -ffp-contract=off:
// the growth reproduces numpy's float32 bits.
#include "hgs_common.h"

// ---- strand walk (hgs_strand_walk_ends / hgs_strand_walk_fill) -------------------------------------------------------------------
// compute_strands_info (reference scene/hair_gaussian_model.py:1410-1498) orders every open polyline of the segment table from one
// end to the other.  The torch form (walk_chains_torch) doubles pointers over the 2 n arcs: ~10 rounds of gathers over every arc,
// ~120 launches, 2.7 ms on a 4 10^5-segment model, twice per topology event.  A strand is a CHAIN: here one lane per strand END
// walks it -- one 16-byte load per step from a node table (for every endpoint its at most two (row, neighbour) entries) -- first
// to find the other end and the length, then (one lane per strand, once the host side has numbered the strands and decided their
// direction) to write the ordered rows.  Chains of ~100 segments: ~100 dependent L2 hits, tens of microseconds, all strands in
// parallel.  Closed loops have no end and are never entered, like in the reference's walk.
struct WalkNode { int row0, nb0, row1, nb1; };      // (-1: no entry)

__global__ __launch_bounds__(256) void walk_nodes_kernel(int n, int n_ep, const long long* __restrict__ pairs, int* __restrict__ deg,
                                                         WalkNode* __restrict__ nodes, int* __restrict__ flags) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const long long a = pairs[2 * (size_t)r], b = pairs[2 * (size_t)r + 1];
  if (a < 0 || b < 0 || a >= n_ep || b >= n_ep) { flags[0] = 1; return; }
#pragma unroll
  for (int s = 0; s < 2; s++) {
    const int id = (int)(s ? b : a), nb = (int)(s ? a : b);
    const int slot = atomicAdd(&deg[id], 1);
    if (slot == 0) { nodes[id].row0 = r; nodes[id].nb0 = nb; }
    else if (slot == 1) { nodes[id].row1 = r; nodes[id].nb1 = nb; }
    else flags[0] = 1;                                   // an endpoint of degree > 2: not a set of chains
  }
}

// other[e] = the end the chain that starts at end e runs into, len[e] = its segments; -1 / 0 for ids that are no chain end
__global__ __launch_bounds__(256) void walk_ends_kernel(int n, int n_ep, const int* __restrict__ deg, const WalkNode* __restrict__ nodes,
                                                        int* __restrict__ other, int* __restrict__ len, int* __restrict__ flags) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n_ep) return;
  int o = -1, L = 0;
  if (deg[e] == 1) {
    const int4 first = *(const int4*)&nodes[e];
    int row = first.x, v = first.y;                      // arrived at v through `row`
    L = 1;
    while (L <= n) {
      const int4 nd = *(const int4*)&nodes[v];
      const bool use1 = nd.x == row;                     // leave through the entry that is not the row we came by
      const int nrow = use1 ? nd.z : nd.x, nnb = use1 ? nd.w : nd.y;
      if (nrow < 0) break;                               // v has no other row: the chain's other end
      row = nrow; v = nnb; L++;
    }
    if (L > n) { flags[0] = 1; L = 0; } else o = v;
  }
  other[e] = o; len[e] = L;
}

__global__ __launch_bounds__(64) void walk_fill_kernel(int S, const long long* __restrict__ starts, const long long* __restrict__ offsets,
                                                       const unsigned char* __restrict__ flip, const WalkNode* __restrict__ nodes,
                                                       long long* __restrict__ rows, long long* __restrict__ seg_rows,
                                                       int* __restrict__ id_to_strand) {
  const int s = blockIdx.x * 64 + threadIdx.x;
  if (s >= S) return;
  const long long o0 = offsets[s], o1 = offsets[s + 1];
  const bool rev = flip[s] != 0;
  int cur = (int)starts[s];
  const int4 first = *(const int4*)&nodes[cur];
  int row = first.x, v = first.y;
  id_to_strand[cur] = s;
  for (long long k = o0; k < o1; k++) {
    const long long at = rev ? o1 - 1 - (k - o0) : k;
    rows[2 * at] = rev ? v : cur;
    rows[2 * at + 1] = rev ? cur : v;
    seg_rows[at] = row;
    id_to_strand[v] = s;
    const int4 nd = *(const int4*)&nodes[v];
    const bool use1 = nd.x == row;
    cur = v;
    row = use1 ? nd.z : nd.x;
    v = use1 ? nd.w : nd.y;
  }
}

extern "C" int hgs_strand_walk_ends(void* stream, int n, int n_ep, const long long* pairs, int* deg, void* nodes, int* other, int* len,
                                    int* flags) {
  if (n < 0 || n_ep < 0) { hgs_set_error("hgs_strand_walk_ends: bad sizes"); return 1; }
  if (n_ep == 0) return 0;
  if ((n > 0 && !pairs) || !deg || !nodes || !other || !len || !flags || ((size_t)nodes & 15)) {
    hgs_set_error("hgs_strand_walk_ends: null argument (or nodes not 16-byte aligned)"); return 1;
  }
  hipStream_t s = (hipStream_t)stream;
  HGS_CHECK_HIP(hipMemsetAsync(deg, 0, sizeof(int) * (size_t)n_ep, s));
  HGS_CHECK_HIP(hipMemsetAsync(nodes, 0xFF, sizeof(WalkNode) * (size_t)n_ep, s));
  HGS_CHECK_HIP(hipMemsetAsync(flags, 0, sizeof(int), s));
  if (n > 0) hipLaunchKernelGGL(walk_nodes_kernel, dim3((n + 255) / 256), dim3(256), 0, s, n, n_ep, pairs, deg, (WalkNode*)nodes, flags);
  hipLaunchKernelGGL(walk_ends_kernel, dim3((n_ep + 255) / 256), dim3(256), 0, s, n, n_ep, deg, (const WalkNode*)nodes, other, len, flags);
  HGS_CHECK_LAUNCH();
  return 0;
}

extern "C" int hgs_strand_walk_fill(void* stream, int S, const long long* starts, const long long* offsets, const unsigned char* flip,
                                    const void* nodes, long long* rows, long long* seg_rows, int* id_to_strand) {
  if (S < 0) { hgs_set_error("hgs_strand_walk_fill: bad size"); return 1; }
  if (S == 0) return 0;
  if (!starts || !offsets || !flip || !nodes || !rows || !seg_rows || !id_to_strand) { hgs_set_error("hgs_strand_walk_fill: null argument"); return 1; }
  hipLaunchKernelGGL(walk_fill_kernel, dim3((S + 63) / 64), dim3(64), 0, (hipStream_t)stream, S, starts, offsets, flip, (const WalkNode*)nodes,
                     rows, seg_rows, id_to_strand);
  HGS_CHECK_LAUNCH();
  return 0;
}


// ---- strand growth (hgs_strand_grow_plan / hgs_strand_grow_fill) -----------------------------------------------------------------
// growing() (reference scene/hair_gaussian_model.py:1098-1200) extends every strand tip by one segment in the direction of its last
// k = min(n_seg, growth_averaging_points) non-collapsed segments; the new segment's attributes are the means of theirs.  The
// reference loops over the strands in Python (180 us a strand).  Here: one lane per strand decides (plan), the caller numbers the
// grown strands by a scan, and one wavefront per strand writes (fill: lane c = channel c of the new rows, so the loads of a kept
// row's attributes are consecutive).  Every value has the reference's float32 bits: numpy evaluates each operation in float32
// (this file is built with -ffp-contract=off), and its means are sums from +0 divided by the count -- over the leading axis of a
// [k, C] array one row after the other (directions, f_dc, f_rest), over a contiguous [k] run by numpy's pairwise_sum (the lengths,
// and the [k, 1] attributes opacity / mask / width, whose reduction numpy runs as one contiguous run): NpRunSum.
namespace {

struct NpRunSum {            // numpy's float32 add.reduce of a contiguous run of known length n <= 128 (pairwise_sum), from +0
  int n, t, blk;
  float r[8], res;
  __device__ __forceinline__ void init(int n_) { n = n_; t = 0; blk = n_ - (n_ & 7); res = 0.f; }
  __device__ __forceinline__ void add(float v) {
    if (n < 8) {
      res = t == 0 ? v : res + v;
    } else if (t < blk) {
#pragma unroll
      for (int j = 0; j < 8; j++)
        if (j == (t & 7)) r[j] = t < 8 ? v : r[j] + v;
      if (t == blk - 1) res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    } else {
      res = res + v;
    }
    t++;
  }
  __device__ __forceinline__ float total() const { return 0.f + res; }
};

__device__ __forceinline__ bool grow_segment(const long long* __restrict__ rows, long long row, const float* __restrict__ ep, int n_ep,
                                             float* d, float* len) {
  const long long a = rows[2 * row], b = rows[2 * row + 1];
  if (a < 0 || b < 0 || a >= n_ep || b >= n_ep) return false;
#pragma unroll
  for (int c = 0; c < 3; c++) d[c] = ep[3 * b + c] - ep[3 * a + c];
  *len = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);      // np.linalg.norm(axis=1) of 3 components
  return true;
}

// status[s]: 0 not grown (at num_points_strand, or every one of the last k segments collapsed), 1 grown, 2 not grown because its tip
// endpoint is shared with another row of the table (deg != 1), 3 an id out of range; keep[s] bit j: row o1 - k + j is kept
__global__ __launch_bounds__(256) void grow_plan_kernel(int S, const long long* __restrict__ offsets, const long long* __restrict__ rows,
                                                        const float* __restrict__ ep, int n_ep, const long long* __restrict__ deg, int n_deg,
                                                        int max_seg, int k_avg, float min_val, int* __restrict__ status,
                                                        unsigned* __restrict__ keep, float* __restrict__ mean_len) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= S) return;
  const long long o0 = offsets[s], o1 = offsets[s + 1], n = o1 - o0;
  int st = 0, cnt = 0;
  unsigned bits = 0;
  float ml = 0.f;
  if (n > 0 && n < max_seg) {
    const int k = (int)(n < k_avg ? n : k_avg);
    for (int j = 0; j < k; j++) {
      float d[3], len;
      if (!grow_segment(rows, o1 - k + j, ep, n_ep, d, &len)) { st = 3; break; }
      if (!(len < min_val)) { bits |= 1u << j; cnt++; }
    }
    if (st == 0 && cnt > 0) {
      NpRunSum acc;
      acc.init(cnt);
      for (int j = 0; j < k; j++) {
        if (!((bits >> j) & 1u)) continue;
        float d[3], len;
        grow_segment(rows, o1 - k + j, ep, n_ep, d, &len);
        acc.add(len);
      }
      ml = acc.total() / (float)cnt;
      const long long tip = rows[2 * (o1 - 1) + 1];
      st = (tip < n_deg && deg[tip] == 1) ? 1 : 2;
    }
  }
  status[s] = st;
  keep[s] = bits;
  mean_len[s] = ml;
}

// one wavefront per strand; channel c of the new row: 0-2 the endpoint, 3-5 f_dc, then f_rest, opacity, mask, width
__global__ __launch_bounds__(256) void grow_fill_kernel(int S, const long long* __restrict__ offsets, const long long* __restrict__ rows,
                                                        const long long* __restrict__ seg_rows, int P, const int* __restrict__ status,
                                                        const int* __restrict__ rank, const unsigned* __restrict__ keep, int k_avg,
                                                        const float* __restrict__ ep, int n_ep, float growth_length,
                                                        const float* __restrict__ length_src, const float* __restrict__ f_dc,
                                                        const float* __restrict__ f_rest, int R, const float* __restrict__ opacity,
                                                        const float* __restrict__ mask, const float* __restrict__ width,
                                                        long long* __restrict__ new_pairs, float* __restrict__ new_ep,
                                                        float* __restrict__ new_dc, float* __restrict__ new_rest,
                                                        float* __restrict__ new_opacity, float* __restrict__ new_mask,
                                                        float* __restrict__ new_width) {
  const int s = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (s >= S || status[s] != 1) return;
  const long long o1 = offsets[s + 1], n = o1 - offsets[s];
  const int k = (int)(n < k_avg ? n : k_avg), r = rank[s];
  const unsigned bits = keep[s];
  const int cnt = __popc(bits);
  const long long tip = rows[2 * (o1 - 1) + 1];
  if (lane == 0) { new_pairs[2 * (long long)r] = tip; new_pairs[2 * (long long)r + 1] = (long long)n_ep + r; }
  const int C = 9 + R;
  for (int c = lane; c < C; c += 64) {
    if (c < 3) {
      float acc = 0.f;
      for (int j = 0; j < k; j++) {
        if (!((bits >> j) & 1u)) continue;
        float d[3], len;
        grow_segment(rows, o1 - k + j, ep, n_ep, d, &len);
        acc = acc + (c == 0 ? d[0] : c == 1 ? d[1] : d[2]) / len;
      }
      const float dir = acc / (float)cnt;
      const float L = length_src ? length_src[0] : growth_length;
      new_ep[3 * (long long)r + c] = ep[3 * tip + c] + dir * L;
      continue;
    }
    const bool run = c >= 6 + R;                 // [k, 1] attributes: numpy reduces them as one contiguous run
    const float* src;
    float* dst;
    int w, off;
    if (c < 6) { src = f_dc; dst = new_dc; w = 3; off = c - 3; }
    else if (!run) { src = f_rest; dst = new_rest; w = R; off = c - 6; }
    else if (c == 6 + R) { src = opacity; dst = new_opacity; w = 1; off = 0; }
    else if (c == 7 + R) { src = mask; dst = new_mask; w = 1; off = 0; }
    else { src = width; dst = new_width; w = 1; off = 0; }
    NpRunSum pw;
    pw.init(cnt);
    float acc = 0.f;
    for (int j = 0; j < k; j++) {
      if (!((bits >> j) & 1u)) continue;
      const long long g = seg_rows[o1 - k + j];
      const float v = (g >= 0 && g < P) ? src[g * w + off] : 0.f;
      if (run) pw.add(v);
      else acc = acc + v;
    }
    dst[(long long)r * w + off] = (run ? pw.total() : acc) / (float)cnt;
  }
}

}  // namespace

extern "C" int hgs_strand_grow_plan(void* stream, int S, const long long* offsets, const long long* rows, const float* endpoints, int n_ep,
                                    const long long* deg, int n_deg, int max_segments, int k_avg, float min_val, int* status,
                                    unsigned* keep, float* mean_len) {
  if (S < 0 || n_ep < 0 || n_deg < 0) { hgs_set_error("hgs_strand_grow_plan: bad sizes"); return 1; }
  if (k_avg < 1 || k_avg > 32) { hgs_set_error("hgs_strand_grow_plan: k_avg = %d outside [1, 32]", k_avg); return 1; }
  if (S == 0) return 0;
  if (!offsets || !status || !keep || !mean_len || (n_ep > 0 && !endpoints) || (n_deg > 0 && !deg)) {
    hgs_set_error("hgs_strand_grow_plan: null argument"); return 1;
  }
  hipLaunchKernelGGL(grow_plan_kernel, dim3((S + 255) / 256), dim3(256), 0, (hipStream_t)stream, S, offsets, rows, endpoints, n_ep, deg,
                     n_deg, max_segments, k_avg, min_val, status, keep, mean_len);
  HGS_CHECK_LAUNCH();
  return 0;
}

extern "C" int hgs_strand_grow_fill(void* stream, int S, const long long* offsets, const long long* rows, const long long* seg_rows, int P,
                                    const int* status, const int* rank, const unsigned* keep, int k_avg, const float* endpoints, int n_ep,
                                    float growth_length, const float* length_src, const float* f_dc, const float* f_rest, int rest_floats,
                                    const float* opacity, const float* mask, const float* width, long long* new_pairs, float* new_endpoints,
                                    float* new_f_dc, float* new_f_rest, float* new_opacity, float* new_mask, float* new_width) {
  if (S < 0 || P < 0 || n_ep < 0 || rest_floats < 0) { hgs_set_error("hgs_strand_grow_fill: bad sizes"); return 1; }
  if (k_avg < 1 || k_avg > 32) { hgs_set_error("hgs_strand_grow_fill: k_avg = %d outside [1, 32]", k_avg); return 1; }
  if (S == 0) return 0;
  if (!offsets || !rows || !seg_rows || !status || !rank || !keep || !endpoints || !f_dc || !opacity || !mask || !width || !new_pairs ||
      !new_endpoints || !new_f_dc || !new_opacity || !new_mask || !new_width || (rest_floats > 0 && (!f_rest || !new_f_rest))) {
    hgs_set_error("hgs_strand_grow_fill: null argument"); return 1;
  }
  hipLaunchKernelGGL(grow_fill_kernel, dim3((S + 3) / 4), dim3(256), 0, (hipStream_t)stream, S, offsets, rows, seg_rows, P, status, rank,
                     keep, k_avg, endpoints, n_ep, growth_length, length_src, f_dc, f_rest, rest_floats, opacity, mask, width, new_pairs,
                     new_endpoints, new_f_dc, new_f_rest, new_opacity, new_mask, new_width);
  HGS_CHECK_LAUNCH();
  return 0;
}
