// hgs_head_tail.h -- device code of the loss head's tail (include/hgs.h HgsHeadTail): the sums over the per-pixel kernel's
// partials and the entries of `out` that depend on them.  Shared by the head's own one-workgroup launch (hgs_losses.hip)
// and by the parameter backward kernels that run it in a spare workgroup of their launch (hgs_strands.hip), off the
// iteration's critical path.  256 threads; the same arithmetic wherever it runs.
#pragma once
#include "hgs_common.h"

__device__ __forceinline__ void hgs_head_tail_block(const HgsHeadTail& t) {
  __shared__ float tail_red[2][4];
  __shared__ double tail_red_b[4];
  float a[2] = {0.f, 0.f};
  // The mask term's partials are summed in float64 and divided by the pixel count, so the mean is rounded once, here.  It
  // reaches 1e2 with confident wrong logits, where an fp32 ulp is 4e-6: an fp32 sum of the partials and the product with
  // fp32(1 / HW) left it one ulp from the correctly rounded mean (tests/test_pixel_f64_gpu.py).  What remains is the rounding
  // of the fp32 block sums themselves, ~1e-8 of the mean over a frame's blocks.
  double ab = 0.0;
  // (all loads of a thread are independent: in flight together)
#pragma unroll 8
  for (int i = threadIdx.x; i < t.nb_pix; i += 256) {
#pragma unroll
    for (int c = 0; c < 2; c++) a[c] += t.pix_partials[3 * (size_t)i + c];
    ab += (double)t.pix_partials[3 * (size_t)i + 2];
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
    for (int c = 0; c < 2; c++) a[c] += __shfl_xor(a[c], d, 64);
    ab += __shfl_xor(ab, d, 64);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int c = 0; c < 2; c++) tail_red[c][threadIdx.x >> 6] = a[c];
    tail_red_b[threadIdx.x >> 6] = ab;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  float s[2];
#pragma unroll
  for (int c = 0; c < 2; c++) s[c] = (tail_red[c][0] + tail_red[c][1]) + (tail_red[c][2] + tail_red[c][3]);
  const float ori_s = s[0], ori_c = s[1];
  const double bce_s = (tail_red_b[0] + tail_red_b[1]) + (tail_red_b[2] + tail_red_b[3]);
  // H * W back from inv_hw = fp32(1 / (H * W)): exact below 8e6 pixels (beyond, within the relative error inv_hw itself has)
  const double hw = rint(1.0 / (double)t.inv_hw);
  float total = t.out[HGS_HEAD_TOTAL_FWD];      // (1 - lambda_dssim) L1 + lambda_dssim DSSIM, from the head's forward (the tail
                                                // may run twice: it must not read what it writes)
  float mask = 0.f, ori = 0.f;
  if (t.bce) { mask = (float)(bce_s / hw); total = fmaf(t.l_mask, mask, total); }     // (explicit: the same bits in every host kernel)
  if (t.ori) { ori = ori_s / ori_c; total = fmaf(t.l_ori, ori, total); }            // empty mask -> NaN, as the reference
  if (t.smooth) total = fmaf(t.l_smooth, t.out[HGS_HEAD_SMOOTH], total);
  t.out[HGS_HEAD_TOTAL] = total; t.out[HGS_HEAD_MASK] = mask; t.out[HGS_HEAD_ORIENTATION] = ori;
  t.out[HGS_HEAD_ORI_COUNT] = ori_c;
}
