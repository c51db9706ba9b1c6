// hgs_export.hip -- arc-length resampling of the model's strands for the strand-file export (scene/strand_export.py,
// export_strands.py): hgs_strand_arclen / hgs_strand_resample.  gfx950, wave64.
//
// The contract (one definition for the numpy path, these kernels and the tests; scene/strand_export.py restates it): strand s has
// n segments on the vertices v_0..v_n (endpoint ids of rows[o + i], root -> tip); len_i = sqrt((dx*dx + dy*dy) + dz*dz),
// cum_0 = 0, cum_{i+1} = cum_i + len_i, L = cum_n; joint attributes a_0 = attr[seg_0], a_n = attr[seg_{n-1}], a_i = 0.5 (attr[seg_{i-1}]
// + attr[seg_i]); sample j of M sits at t = (j / (M - 1)) L on segment i = the largest index with cum_i <= t (at most n - 1), at
// w = (t - cum_i) / len_i (0 on a collapsed segment): v_i + w (v_{i+1} - v_i), a_i + w (a_{i+1} - a_i); samples 0 and M - 1 are the end
// joints themselves.  Every operation is float64 on the float32 inputs, one rounding each (this file is built with -ffp-contract=off),
// and the results are rounded once to float32.
//
// The running length is added up in SEGMENT ORDER, exactly as the definition states it: the lanes of a strand's wavefront compute
// their 64 segment lengths side by side, and the inclusive scan then walks the lanes one after the other (the running sum is
// wavefront-uniform, one add per segment), carrying the sum from one chunk of 64 into the next.  A tree-shaped scan would round
// differently from cum_{i+1} = cum_i + len_i -- 2 float64 units rms of L at 130 segments (tools/scan_order_trial.py, on the CPU) -- and with it the segment a sample
// near a joint falls on; in segment order `cum` and `length` have the definition's bits, the numpy path (np.cumsum) has them too, and
// the same float64 operations follow on every path (tools/export_timing.py times the kernels).
#include "hgs_common.h"

namespace {

struct Vtx { double x, y, z; bool ok; };

__device__ __forceinline__ Vtx export_vertex(const float* __restrict__ ep, int n_ep, long long id) {
  Vtx v = {0.0, 0.0, 0.0, false};
  if (id < 0 || id >= n_ep) return v;
  v.x = (double)ep[3 * id]; v.y = (double)ep[3 * id + 1]; v.z = (double)ep[3 * id + 2];
  v.ok = true;
  return v;
}

__device__ __forceinline__ double export_length(const Vtx& a, const Vtx& b) {
  const double dx = b.x - a.x, dy = b.y - a.y, dz = b.z - a.z;
  return sqrt((dx * dx + dy * dy) + dz * dz);
}

// vertex i (0..n) of the strand whose rows start at o
__device__ __forceinline__ long long export_vertex_id(const long long* __restrict__ rows, long long o, long long n, long long i) {
  return i < n ? rows[2 * (o + i)] : rows[2 * (o + n - 1) + 1];
}

// one wavefront per strand, four strands per workgroup
__global__ __launch_bounds__(256) void strand_arclen_kernel(int S, const long long* __restrict__ offsets, const long long* __restrict__ rows,
                                                            long long total, const float* __restrict__ ep, int n_ep,
                                                            double* __restrict__ cum, double* __restrict__ length, int* __restrict__ status) {
  const int s = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (s >= S) return;
  const long long o0 = offsets[s], o1 = offsets[s + 1], n = o1 - o0;
  if (o0 < 0 || n < 0 || o1 > total) {               // a table that does not describe `rows`: nothing of it is read or written
    if (lane == 0) { status[0] = 2; length[s] = 0.0; }
    return;
  }
  double* const run = cum + o0 + s;                  // n + 1 entries
  if (lane == 0) run[0] = 0.0;
  double carry = 0.0;                                // wavefront-uniform
  for (long long base = 0; base < n; base += 64) {
    const long long i = base + lane;
    double len = 0.0;
    if (i < n) {
      const Vtx a = export_vertex(ep, n_ep, rows[2 * (o0 + i)]), b = export_vertex(ep, n_ep, rows[2 * (o0 + i) + 1]);
      if (a.ok && b.ok) len = export_length(a, b);
      else status[0] = 1;                            // (every writer stores the same word)
    }
    const int m = (int)(n - base < 64 ? n - base : 64);
    double mine = 0.0;
    for (int k = 0; k < m; k++) {                    // in segment order: cum_{i+1} = cum_i + len_i
      carry = carry + __shfl(len, k, 64);
      if (lane == k) mine = carry;
    }
    if (i < n) run[i + 1] = mine;
  }
  if (lane == 0) length[s] = carry;
}

// The rows of attr behind joint i: a_0 = attr[seg_0], a_n = attr[seg_{n-1}], else the mean of the two segments that meet (g0 == g1 at the ends)
struct JointRows { long long g0, g1; };
__device__ __forceinline__ JointRows export_joint_rows(const long long* __restrict__ seg_rows, long long o, long long n, long long i) {
  JointRows r;
  r.g1 = seg_rows[o + (i < n ? i : n - 1)];
  r.g0 = (i == 0 || i == n) ? r.g1 : seg_rows[o + i - 1];
  return r;
}
__device__ __forceinline__ double export_attr_row(const float* __restrict__ attr, int P, int C, long long g, int c) {
  return (g >= 0 && g < P) ? (double)attr[g * C + c] : 0.0;
}
__device__ __forceinline__ double export_joint_attr(const float* __restrict__ attr, int P, int C, const JointRows& r, int c) {
  if (r.g0 == r.g1) return export_attr_row(attr, P, C, r.g1, c);
  return 0.5 * (export_attr_row(attr, P, C, r.g0, c) + export_attr_row(attr, P, C, r.g1, c));
}

// one lane per output sample; M >= 2: sample j of kept strand k is lane k M + j; M == 0 (native): the joints, lane out_offsets[k] + j
__global__ __launch_bounds__(256) void strand_resample_kernel(int S, const long long* __restrict__ offsets, const long long* __restrict__ rows,
                                                              const long long* __restrict__ seg_rows, long long total,
                                                              const float* __restrict__ ep, int n_ep, const float* __restrict__ attr, int P,
                                                              int C, const double* __restrict__ cum, int K, const int* __restrict__ kept, int M,
                                                              const long long* __restrict__ out_offsets, long long n_out,
                                                              float* __restrict__ out_points, float* __restrict__ out_attrs) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n_out) return;
  long long k, j;
  if (M > 0) {
    k = idx / M; j = idx - k * M;
  } else {
    long long lo = 0, hi = K;                         // largest k with out_offsets[k] <= idx
    while (hi - lo > 1) {
      const long long mid = (lo + hi) >> 1;
      if (out_offsets[mid] <= idx) lo = mid; else hi = mid;
    }
    k = lo; j = idx - out_offsets[k];
  }
  float px = 0.f, py = 0.f, pz = 0.f;
  long long o0 = 0, n = 0, i = 0;
  double w = 0.0;
  bool valid = false;
  const int s = kept[k];
  if (s >= 0 && s < S) {
    o0 = offsets[s];
    n = offsets[s + 1] - o0;
    valid = o0 >= 0 && n >= 1 && o0 + n <= total && j >= 0 && (M > 0 || j <= n);
  }
  if (valid) {
    if (M == 0) {
      i = j;                                          // the joint itself
    } else if (j == M - 1) {
      i = n;
    } else if (j > 0) {
      const double* const run = cum + o0 + s;
      const double t = ((double)j / (double)(M - 1)) * run[n];
      long long lo = 0, hi = n + 1;                   // largest i with cum_i <= t (cum_0 = 0 <= t)
      while (hi - lo > 1) {
        const long long mid = (lo + hi) >> 1;
        if (run[mid] <= t) lo = mid; else hi = mid;
      }
      i = lo < n - 1 ? lo : n - 1;
      const Vtx a = export_vertex(ep, n_ep, export_vertex_id(rows, o0, n, i)), b = export_vertex(ep, n_ep, export_vertex_id(rows, o0, n, i + 1));
      if (a.ok && b.ok) {
        const double len = export_length(a, b);
        w = len > 0.0 ? (t - run[i]) / len : 0.0;
        px = (float)(a.x + w * (b.x - a.x)); py = (float)(a.y + w * (b.y - a.y)); pz = (float)(a.z + w * (b.z - a.z));
      } else {
        valid = false;                               // an endpoint id outside the table: the row is written as zeros
      }
    }
    if (M == 0 || j == 0 || j == M - 1) {
      const Vtx a = export_vertex(ep, n_ep, export_vertex_id(rows, o0, n, i));
      if (a.ok) { px = (float)a.x; py = (float)a.y; pz = (float)a.z; }
      else valid = false;
    }
  }
  out_points[3 * idx] = px; out_points[3 * idx + 1] = py; out_points[3 * idx + 2] = pz;
  const bool joint = M == 0 || j == 0 || j == M - 1;
  JointRows r0 = {0, 0}, r1 = {0, 0};                // the two to four rows of attr behind the sample, resolved once
  if (valid) {
    r0 = export_joint_rows(seg_rows, o0, n, i);
    if (!joint) r1 = export_joint_rows(seg_rows, o0, n, i + 1);
  }
  for (int c = 0; c < C; c++) {
    float v = 0.f;
    if (valid) {
      const double a0 = export_joint_attr(attr, P, C, r0, c);
      v = joint ? (float)a0 : (float)(a0 + w * (export_joint_attr(attr, P, C, r1, c) - a0));
    }
    out_attrs[(long long)C * idx + c] = v;
  }
}

}  // namespace

extern "C" int hgs_strand_arclen(void* stream, int S, const long long* offsets, const long long* rows, long long total, const float* endpoints,
                                 int n_ep, double* cum, double* length, int* status) {
  if (S < 0 || total < 0 || n_ep < 0) { hgs_set_error("hgs_strand_arclen: bad sizes"); return 1; }
  if (S == 0) return 0;
  if (!offsets || !cum || !length || !status || (total > 0 && (!rows || !endpoints))) {
    hgs_set_error("hgs_strand_arclen: null argument"); return 1;
  }
  hipLaunchKernelGGL(strand_arclen_kernel, dim3((S + 3) / 4), dim3(256), 0, (hipStream_t)stream, S, offsets, rows, total, endpoints, n_ep,
                     cum, length, status);
  HGS_CHECK_LAUNCH();
  return 0;
}

extern "C" int hgs_strand_resample(void* stream, int S, const long long* offsets, const long long* rows, const long long* seg_rows,
                                   long long total, const float* endpoints, int n_ep, const float* attr, int P, int C, const double* cum,
                                   int K, const int* kept, int M, const long long* out_offsets, long long n_out, float* out_points,
                                   float* out_attrs) {
  if (S < 0 || total < 0 || n_ep < 0 || P < 0 || K < 0 || n_out < 0) { hgs_set_error("hgs_strand_resample: bad sizes"); return 1; }
  if (C < 1 || C > 16) { hgs_set_error("hgs_strand_resample: C = %d outside [1, 16]", C); return 1; }
  if (M < 0 || M == 1) { hgs_set_error("hgs_strand_resample: M = %d (0: the joints themselves, else at least 2 points per strand)", M); return 1; }
  if (K > S) { hgs_set_error("hgs_strand_resample: %d kept strands of %d", K, S); return 1; }
  if (M > 0 && n_out != (long long)K * M) { hgs_set_error("hgs_strand_resample: n_out = %lld, K M = %lld", n_out, (long long)K * M); return 1; }
  if (M == 0 && n_out > total + K) { hgs_set_error("hgs_strand_resample: n_out = %lld joints of %lld segments on %d strands", n_out, total, K); return 1; }
  if (n_out > 0x7FFFFFFFll) { hgs_set_error("hgs_strand_resample: n_out = %lld: at most 2^31 - 1 points per call", n_out); return 1; }
  if (K == 0 || n_out == 0) return 0;
  if (!offsets || !rows || !seg_rows || !endpoints || !attr || !cum || !kept || !out_points || !out_attrs || (M == 0 && !out_offsets)) {
    hgs_set_error("hgs_strand_resample: null argument"); return 1;
  }
  hipLaunchKernelGGL(strand_resample_kernel, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, (hipStream_t)stream, S, offsets, rows,
                     seg_rows, total, endpoints, n_ep, attr, P, C, cum, K, kept, M, out_offsets, n_out, out_points, out_attrs);
  HGS_CHECK_LAUNCH();
  return 0;
}
