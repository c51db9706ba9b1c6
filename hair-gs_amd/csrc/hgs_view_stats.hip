// hgs_view_stats.hip -- per-view image statistics of rendered views against their capture (hgs_view_stats; the sums behind
// loss/image_metrics.py view_metrics, whose torch statements on CPU tensors are the contract this file restates).
//
// For V views of one size H x W:
//   * view_stats_kernel: grid (hgs_view_stats_num_blocks(H, W), V), 256 lanes (4 waves) per block.  Block b of view v visits
//     the pixels b * 256 + t + k * (nb * 256) in k order; every lane evaluates its pixel in float32, operation by operation (this
//     file is built with -ffp-contract=off), as the CPU path does, and adds into float64 sums (uint32 counters for the counts).
//     The lanes' values are reduced by a fixed butterfly within the wave, then over the 4 waves in wave order through LDS; the
//     block writes its row of HGS_VIEW_STATS_N partial sums.
//   * view_stats_reduce_kernel: one wave per view sums the view's nb rows, lane l taking rows l, l + 64, ... in order, then the
//     same butterfly.  Nothing depends on V or on timing: a view's sums are bitwise the same in every call and every batch.
// Per pixel (pred: the clamped render; NULL planes turn their statistics off):
//   e_c = (pred_c - gt_c) * (pred_c - gt_c); sse += e_0, e_1, e_2; a GT mask pixel (mask != 0) adds them to sse_mask as well;
//   fg >= fg_threshold counts as foreground, and also as intersection where the GT mask is set;
//   orientation (omap, viewmats and gt_theta non-NULL): px = (o0 v[0] + o1 v[4]) + o2 v[8], py likewise with v[1], v[5], v[9]
//   (omap @ world_view[:3,:3], row-major), r = sqrt(px px + py py), n = r + min_val, x = px / n, y = py / n, y += min_val where
//   y < min_val, theta = atan2(x, y) (+ pi where negative), diff = pi/2 - | |theta - gt| - pi/2 |; over the orientation mask (the
//   GT mask, else o != 0 in any channel) diff, diff * confidence (diff without a confidence plane), the count and the counts of
//   diff <= float(10 pi / 180) and <= float(20 pi / 180) are summed.
#include "hgs_common.h"

namespace {

#define VS_BLOCK 256
#define VS_WAVES (VS_BLOCK / HGS_WAVE)
#define VS_PIX_PER_LANE 16          // target pixels per lane: the block count follows from it
#define VS_MAX_BLOCKS 1024

__global__ __launch_bounds__(VS_BLOCK) void view_stats_kernel(int HW, int nb, const float* __restrict__ pred, const float* __restrict__ gt,
                                                              const uint8_t* __restrict__ mask, const float* __restrict__ fg, float fg_th,
                                                              const float* __restrict__ omap, const float* __restrict__ viewmats,
                                                              const float* __restrict__ gt_theta, const float* __restrict__ conf,
                                                              float min_val, double* __restrict__ partials) {
  __shared__ double s_part[VS_WAVES][HGS_VIEW_STATS_N];
  const int v = blockIdx.y, b = blockIdx.x;
  const size_t plane = (size_t)HW, vo = (size_t)v * plane;
  const float* pr = pred + 3 * vo;
  const float* g = gt + 3 * vo;
  const uint8_t* mk = mask ? mask + vo : nullptr;
  const float* fp = fg ? fg + vo : nullptr;
  const bool ori = omap && viewmats && gt_theta;
  const float* om = ori ? omap + 3 * vo : nullptr;
  const float* th = ori ? gt_theta + vo : nullptr;
  const float* cf = (ori && conf) ? conf + vo : nullptr;
  float w0 = 0.f, w4 = 0.f, w8 = 0.f, w1 = 0.f, w5 = 0.f, w9 = 0.f;
  if (ori) {
    const float* vm = viewmats + (size_t)v * 16;
    w0 = vm[0]; w4 = vm[4]; w8 = vm[8];
    w1 = vm[1]; w5 = vm[5]; w9 = vm[9];
  }
  const float half_pi = 1.57079632679489661923f;    // float(np.pi / 2)
  const float pi = 3.14159265358979323846f;         // float(np.pi)
  const float th10 = (float)(10.0 * 3.141592653589793 / 180.0), th20 = (float)(20.0 * 3.141592653589793 / 180.0);
  double sse = 0.0, sse_m = 0.0, o_abs = 0.0, o_w = 0.0;
  uint32_t n_m = 0u, n_fg = 0u, n_in = 0u, o_n = 0u, o_10 = 0u, o_20 = 0u;
  const int stride = nb * VS_BLOCK;
  for (int p = b * VS_BLOCK + (int)threadIdx.x; p < HW; p += stride) {
    const float d0 = pr[p] - g[p], d1 = pr[plane + p] - g[plane + p], d2 = pr[2 * plane + p] - g[2 * plane + p];
    const float e0 = d0 * d0, e1 = d1 * d1, e2 = d2 * d2;
    sse += (double)e0;
    sse += (double)e1;
    sse += (double)e2;
    const bool m = mk && mk[p] != 0;
    if (m) {
      sse_m += (double)e0;
      sse_m += (double)e1;
      sse_m += (double)e2;
      n_m++;
    }
    if (fp && fp[p] >= fg_th) {
      n_fg++;
      if (m) n_in++;
    }
    if (ori) {
      const float o0 = om[p], o1 = om[plane + p], o2 = om[2 * plane + p];
      const bool om_set = mk ? m : (o0 != 0.f || o1 != 0.f || o2 != 0.f);
      if (om_set) {
        const float px = o0 * w0 + o1 * w4 + o2 * w8;
        const float py = o0 * w1 + o1 * w5 + o2 * w9;
        const float n = sqrtf(px * px + py * py) + min_val;
        const float x = px / n;
        float y = py / n;
        y = y < min_val ? y + min_val : y;
        float t = atan2f(x, y);
        t = t < 0.f ? t + pi : t;
        const float diff = half_pi - fabsf(fabsf(t - th[p]) - half_pi);
        o_abs += (double)diff;
        o_w += (double)(cf ? diff * cf[p] : diff);
        o_n++;
        if (diff <= th10) o_10++;
        if (diff <= th20) o_20++;
      }
    }
  }
  double vals[HGS_VIEW_STATS_N] = {sse, sse_m, (double)n_m, (double)n_fg, (double)n_in, o_abs, o_w, (double)o_n, (double)o_10,
                                   (double)o_20};
  const int lane = threadIdx.x & (HGS_WAVE - 1), wv = threadIdx.x / HGS_WAVE;
#pragma unroll
  for (int s = 0; s < HGS_VIEW_STATS_N; s++) vals[s] = wave_sum(vals[s]);
  if (lane == 0) {
#pragma unroll
    for (int s = 0; s < HGS_VIEW_STATS_N; s++) s_part[wv][s] = vals[s];
  }
  __syncthreads();
  if (threadIdx.x < HGS_VIEW_STATS_N) {
    double acc = s_part[0][threadIdx.x];
    for (int w = 1; w < VS_WAVES; w++) acc += s_part[w][threadIdx.x];
    partials[((size_t)v * nb + b) * HGS_VIEW_STATS_N + threadIdx.x] = acc;
  }
}

__global__ __launch_bounds__(HGS_WAVE) void view_stats_reduce_kernel(int nb, const double* __restrict__ partials, double* __restrict__ out) {
  const int v = blockIdx.x, lane = threadIdx.x;
  const double* rows = partials + (size_t)v * nb * HGS_VIEW_STATS_N;
  for (int s = 0; s < HGS_VIEW_STATS_N; s++) {
    double acc = 0.0;
    for (int r = lane; r < nb; r += HGS_WAVE) acc += rows[(size_t)r * HGS_VIEW_STATS_N + s];
    acc = wave_sum(acc);
    if (lane == 0) out[(size_t)v * HGS_VIEW_STATS_N + s] = acc;
  }
}

}  // namespace

extern "C" int hgs_view_stats_num_blocks(int H, int W) {
  if (H < 1 || W < 1 || (long long)H * W > (1ll << 30)) return 0;
  const long long per_block = (long long)VS_BLOCK * VS_PIX_PER_LANE;
  const long long nb = ((long long)H * W + per_block - 1) / per_block;
  return (int)(nb < VS_MAX_BLOCKS ? nb : VS_MAX_BLOCKS);
}

extern "C" int hgs_view_stats(void* stream, int V, int H, int W, const float* pred, const float* gt, const unsigned char* gt_mask,
                              const float* fg, float fg_threshold, const float* omap, const float* viewmats, const float* gt_theta,
                              const float* confidence, float min_val, double* partials, double* out) {
  const int nb = hgs_view_stats_num_blocks(H, W);
  if (V < 1 || V > 65535 || nb < 1) {
    hgs_set_error("hgs_view_stats: bad sizes V=%d H=%d W=%d (1 <= V <= 65535, H, W >= 1, H W <= 2^30)", V, H, W);
    return 1;
  }
  if (!pred || !gt || !partials || !out) { hgs_set_error("hgs_view_stats: pred, gt, partials and out are required"); return 1; }
  if (omap && gt_theta && !viewmats) { hgs_set_error("hgs_view_stats: an orientation map needs its view matrices"); return 1; }
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(view_stats_kernel, dim3(nb, V), dim3(VS_BLOCK), 0, st, H * W, nb, pred, gt, gt_mask, fg, fg_threshold, omap,
                     viewmats, gt_theta, confidence, min_val, partials);
  HGS_CHECK_LAUNCH();
  hipLaunchKernelGGL(view_stats_reduce_kernel, dim3(V), dim3(HGS_WAVE), 0, st, nb, partials, out);
  HGS_CHECK_LAUNCH();
  return 0;
}
