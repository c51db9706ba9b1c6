// hgs_vision.hip -- orientation maps of input views on the GPU (hgs_orientation_field / hgs_orientation_confidence; the
// reference's utils/vision.py estimate_orientation_field, restated in utils/vision.py of this project).
//
// For N gray uint8 views of one size and A Gabor kernels of side S (odd, <= 63, built on the host):
//   * gabor_response_kernel: one workgroup of 4 waves per 64 x 32 output tile of one view.  The tile and its BORDER_REFLECT_101
//     halo are staged into LDS once, as float64, with the border indices resolved while staging; then, for every angle, each
//     lane owns one column and a run of 8 rows, and walks the kernel column by column: the S + 7 values of its LDS column feed
//     8 S FMAs (v_fma_f64) whose weights are wave-uniform scalar loads.  The weight table is repacked per (angle, column) and
//     padded with zero rows to SP = 8 ceil(S / 8) so the row loop unrolls at compile time (one instantiation per SP).
//     Each product uint8 x float32 is exact in float64, so the sum is within ~1e-9 of the exact correlation; it is rounded
//     half to even and saturated to [0, 255] (OpenCV's ddepth = -1) and stored as one byte per (view, angle, pixel).
//   * orientation_stats_kernel: one lane per pixel: the first maximum over the angles, sum r, and
//     var = sum_k (d_k d_k) r_k / (sum r + 1e-7) in plain k order, operation by operation (this file is built with
//     -ffp-contract=off), as the CPU path evaluates it; the per-view maximum of 1 / var^2 over var != 0 by an atomic max on
//     the bits of the positive double.
//   * orientation_confidence_kernel: conf = (1 / var^2) / max as float32 where var != 0, else 1.
#include "hgs_common.h"

namespace {

#define GR_R 8          // output rows per lane
#define GR_TW 64        // tile width: one column per lane
#define GR_TH 32        // tile height: 4 waves x GR_R rows
#define GR_BLOCK 256
#define OR_BLOCK 256
#define HGS_ORIENT_MAX_SIDE 63
#define HGS_ORIENT_MAX_ANGLES 256

// BORDER_REFLECT_101 for any index (repeated reflection when the view is narrower than the kernel's half-width)
__device__ __forceinline__ int reflect101(int i, int n) {
  if (n == 1) return 0;
  const int p = 2 * (n - 1);
  i = i < 0 ? -i : i;
  i %= p;
  return i < n ? i : p - i;
}

// w[A][S][S] (row ky, column kx) -> wt[A][S][SP] (column kx, row ky, rows S..SP-1 zero)
__global__ __launch_bounds__(OR_BLOCK) void gabor_repack_kernel(int A, int side, int SP, const double* __restrict__ w,
                                                                double* __restrict__ wt) {
  const int e = blockIdx.x * OR_BLOCK + threadIdx.x;
  if (e >= A * side * SP) return;
  const int t = e % SP, kx = (e / SP) % side, a = e / (SP * side);
  wt[e] = t < side ? w[((size_t)a * side + t) * side + kx] : 0.0;
}

template <int NC>
__global__ __launch_bounds__(GR_BLOCK) void gabor_response_kernel(int H, int W, int A, int side, const uint8_t* __restrict__ gray,
                                                                  const double* __restrict__ wt, uint8_t* __restrict__ resp) {
  constexpr int SP = NC * GR_R, ROWS = GR_TH + SP - 1, PITCH = GR_TW + SP - 1;
  __shared__ double tile[ROWS * PITCH];
  const int n = blockIdx.z, tx0 = blockIdx.x * GR_TW, ty0 = blockIdx.y * GR_TH, half = side >> 1;
  const size_t plane = (size_t)H * W;
  const uint8_t* img = gray + (size_t)n * plane;
  for (int e = threadIdx.x; e < ROWS * PITCH; e += GR_BLOCK) {
    const int r = e / PITCH, c = e - r * PITCH;
    tile[e] = (double)img[(size_t)reflect101(ty0 - half + r, H) * W + reflect101(tx0 - half + c, W)];
  }
  __syncthreads();
  const int lane = threadIdx.x & (HGS_WAVE - 1), wv = threadIdx.x / HGS_WAVE;
  const double* base = tile + wv * GR_R * PITCH + lane;   // rows wv*8 .. wv*8 + SP + 6 < ROWS, columns lane .. lane + S - 1 < PITCH
  const int x = tx0 + lane, y0 = ty0 + wv * GR_R;
  uint8_t* out = resp + (size_t)n * A * plane;
  for (int a = 0; a < A; a++) {
    double acc[GR_R];
#pragma unroll
    for (int j = 0; j < GR_R; j++) acc[j] = 0.0;
    const double* wa = wt + (size_t)a * side * SP;
    for (int kx = 0; kx < side; kx++) {
      const double* col = base + kx;
      const double* wk = wa + kx * SP;
#pragma unroll
      for (int i = 0; i < SP + GR_R - 1; i++) {
        const double v = col[i * PITCH];
#pragma unroll
        for (int j = 0; j < GR_R; j++) {
          const int t = i - j;
          if (t >= 0 && t < SP) acc[j] = __builtin_fma(wk[t], v, acc[j]);
        }
      }
    }
    if (x < W) {
#pragma unroll
      for (int j = 0; j < GR_R; j++) {
        if (y0 + j >= H) break;
        const double r = fmin(fmax(rint(acc[j]), 0.0), 255.0);
        out[(size_t)a * plane + (size_t)(y0 + j) * W + x] = (uint8_t)r;
      }
    }
  }
}

__global__ __launch_bounds__(OR_BLOCK) void orientation_stats_kernel(int HW, int A, const uint8_t* __restrict__ resp,
                                                                     const double* __restrict__ thetas, uint8_t* __restrict__ idx_out,
                                                                     double* __restrict__ var_out, unsigned long long* __restrict__ maxinv,
                                                                     uint8_t* __restrict__ responses) {
  __shared__ unsigned long long s_max[OR_BLOCK / HGS_WAVE];
  const int n = blockIdx.y, p = blockIdx.x * OR_BLOCK + threadIdx.x;
  unsigned long long bits = 0ull;   // 1 / var^2 as bits (positive doubles order as their bit patterns); 0: none
  if (p < HW) {
    const uint8_t* r = resp + (size_t)n * A * HW + p;
    int best = 0, rmax = -1;
    uint32_t sum = 0u;
    for (int k = 0; k < A; k++) {
      const int v = r[(size_t)k * HW];
      if (v > rmax) { rmax = v; best = k; }
      sum += (uint32_t)v;
    }
    const double th = thetas[best];
    const double half_pi = 1.5707963267948966;   // (np.pi / 2)
    double acc = 0.0;
    for (int k = 0; k < A; k++) {
      const int v = r[(size_t)k * HW];
      const double d = half_pi - fabs(fabs(th - thetas[k]) - half_pi);
      acc = acc + (d * d) * (double)v;
      if (responses) responses[((size_t)n * HW + p) * A + k] = (uint8_t)v;
    }
    const double var = acc / ((double)sum + 1e-7);
    idx_out[(size_t)n * HW + p] = (uint8_t)best;
    var_out[(size_t)n * HW + p] = var;
    if (var != 0.0) bits = (unsigned long long)__double_as_longlong(1.0 / (var * var));
  }
  for (int off = HGS_WAVE / 2; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(bits, off);
    bits = o > bits ? o : bits;
  }
  if ((threadIdx.x & (HGS_WAVE - 1)) == 0) s_max[threadIdx.x / HGS_WAVE] = bits;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long m = s_max[0];
    for (int w = 1; w < OR_BLOCK / HGS_WAVE; w++) m = s_max[w] > m ? s_max[w] : m;
    if (m) atomicMax(&maxinv[n], m);
  }
}

__global__ __launch_bounds__(OR_BLOCK) void orientation_confidence_kernel(int HW, const double* __restrict__ var,
                                                                          const double* __restrict__ maxinv, float* __restrict__ conf) {
  const int n = blockIdx.y, p = blockIdx.x * OR_BLOCK + threadIdx.x;
  if (p >= HW) return;
  const double v = var[(size_t)n * HW + p];
  conf[(size_t)n * HW + p] = v != 0.0 ? (float)((1.0 / (v * v)) / maxinv[n]) : 1.0f;
}

int padded_side(int side) { return (side + GR_R - 1) / GR_R * GR_R; }

size_t orientation_layout(int N, int H, int W, int A, int side, char* base, double** wt, uint8_t** resp) {
  char* cur = base;
  auto take = [&](size_t bytes) { char* p = cur; cur += hgs_align_up(bytes); return p; };
  char* w = take(8 * (size_t)A * side * padded_side(side));
  char* r = take((size_t)N * A * H * W);
  if (wt) *wt = (double*)w;
  if (resp) *resp = (uint8_t*)r;
  return (size_t)(cur - base) + HGS_ALIGN;
}

template <int NC>
void launch_response(hipStream_t st, int N, int H, int W, int A, int side, const uint8_t* gray, const double* wt, uint8_t* resp) {
  const dim3 grid((W + GR_TW - 1) / GR_TW, (H + GR_TH - 1) / GR_TH, N);
  hipLaunchKernelGGL(gabor_response_kernel<NC>, grid, dim3(GR_BLOCK), 0, st, H, W, A, side, gray, wt, resp);
}

bool orientation_sizes_ok(const char* who, int N, int H, int W) {
  if (N < 1 || N > 65535 || H < 1 || W < 1 || (long long)H * W > (1ll << 30)) {
    hgs_set_error("%s: bad sizes N=%d H=%d W=%d (1 <= N <= 65535, H W <= 2^30)", who, N, H, W);
    return false;
  }
  return true;
}

}  // namespace

extern "C" size_t hgs_orientation_scratch_bytes(int N, int H, int W, int A, int side) {
  if (N < 0 || H < 0 || W < 0 || A < 0 || side < 0) return 0;
  return orientation_layout(N, H, W, A, side, nullptr, nullptr, nullptr);
}

extern "C" int hgs_orientation_field(void* stream, int N, int H, int W, const uint8_t* gray, int A, int side, const double* weights,
                                     const double* thetas, uint8_t* idx_out, double* var_out, double* maxinv_out, uint8_t* responses,
                                     void* scratch, size_t scratch_bytes) {
  if (!orientation_sizes_ok("hgs_orientation_field", N, H, W)) return 1;
  if (A < 2 || A > HGS_ORIENT_MAX_ANGLES || side < 1 || side > HGS_ORIENT_MAX_SIDE || !(side & 1)) {
    hgs_set_error("hgs_orientation_field: need 2 <= A <= %d angles (got %d) and an odd kernel side <= %d (got %d)",
                  HGS_ORIENT_MAX_ANGLES, A, HGS_ORIENT_MAX_SIDE, side);
    return 1;
  }
  if (!gray || !weights || !thetas || !idx_out || !var_out || !maxinv_out) { hgs_set_error("hgs_orientation_field: null argument"); return 1; }
  const size_t need = hgs_orientation_scratch_bytes(N, H, W, A, side);
  if (!scratch || ((uintptr_t)scratch % HGS_ALIGN) || scratch_bytes < need) {
    hgs_set_error("hgs_orientation_field: a %d-byte aligned scratch of >= %zu bytes is required (got %zu)", HGS_ALIGN, need,
                  scratch_bytes);
    return 1;
  }
  hipStream_t st = (hipStream_t)stream;
  double* wt;
  uint8_t* resp;
  orientation_layout(N, H, W, A, side, (char*)scratch, &wt, &resp);
  const int SP = padded_side(side);
  if (hgs_zero_async(st, maxinv_out, 8 * (size_t)N)) return 1;
  hipLaunchKernelGGL(gabor_repack_kernel, dim3((A * side * SP + OR_BLOCK - 1) / OR_BLOCK), dim3(OR_BLOCK), 0, st, A, side, SP, weights, wt);
  HGS_CHECK_LAUNCH();
  switch (SP / GR_R) {
    case 1: launch_response<1>(st, N, H, W, A, side, gray, wt, resp); break;
    case 2: launch_response<2>(st, N, H, W, A, side, gray, wt, resp); break;
    case 3: launch_response<3>(st, N, H, W, A, side, gray, wt, resp); break;
    case 4: launch_response<4>(st, N, H, W, A, side, gray, wt, resp); break;
    case 5: launch_response<5>(st, N, H, W, A, side, gray, wt, resp); break;
    case 6: launch_response<6>(st, N, H, W, A, side, gray, wt, resp); break;
    case 7: launch_response<7>(st, N, H, W, A, side, gray, wt, resp); break;
    default: launch_response<8>(st, N, H, W, A, side, gray, wt, resp); break;
  }
  HGS_CHECK_LAUNCH();
  const int HW = H * W;
  hipLaunchKernelGGL(orientation_stats_kernel, dim3((HW + OR_BLOCK - 1) / OR_BLOCK, N), dim3(OR_BLOCK), 0, st, HW, A, resp, thetas,
                     idx_out, var_out, (unsigned long long*)maxinv_out, responses);
  HGS_CHECK_LAUNCH();
  return 0;
}

extern "C" int hgs_orientation_confidence(void* stream, int N, int H, int W, const double* var, const double* maxinv, float* conf_out) {
  if (!orientation_sizes_ok("hgs_orientation_confidence", N, H, W)) return 1;
  if (!var || !maxinv || !conf_out) { hgs_set_error("hgs_orientation_confidence: null argument"); return 1; }
  const int HW = H * W;
  hipLaunchKernelGGL(orientation_confidence_kernel, dim3((HW + OR_BLOCK - 1) / OR_BLOCK, N), dim3(OR_BLOCK), 0, (hipStream_t)stream, HW,
                     var, maxinv, conf_out);
  HGS_CHECK_LAUNCH();
  return 0;
}
