// hgs_undistort.hip -- undistortion of a capture's images and masks into the pinhole camera of utils/undistort.py
// (undistort.py is the scene driver): hgs_undistort_images.  gfx950, wave64.
//
// The contract (one definition for the numpy path, this kernel and the tests; utils/undistort.py states it in full).  For the output
// pixel (x, y) of the pinhole camera (fx', fy', cx', cy'):
//   u = ((x + 0.5) - cx') / fx',  v = ((y + 0.5) - cy') / fy';  uu = u*u, vv = v*v, r2 = uu + vv
//   SIMPLE_RADIAL  rad = k*r2;   RADIAL, OPENCV  rad = k1*r2 + k2*(r2*r2);
//   FULL_OPENCV    r4 = r2*r2, r6 = r4*r2, rad = (((1 + k1*r2) + k2*r4) + k3*r6) / (((1 + k4*r2) + k5*r4) + k6*r6) - 1
//   du = u*rad, dv = v*rad;  OPENCV, FULL_OPENCV, uv = u*v:  du = (du + (2*p1)*uv) + p2*(r2 + 2*uu),  dv = (dv + (2*p2)*uv) + p1*(r2 + 2*vv)
//   sx = (fx*(u + du) + cx) - 0.5,  sy = (fy*(v + dv) + cy) - 0.5;  valid iff 0 <= sx <= Ws - 1 and 0 <= sy <= Hs - 1
//   x0 = floor(sx), x1 = min(x0 + 1, Ws - 1), wx = sx - x0 (likewise y);  value = (1 - wy)*((1 - wx)*p00 + wx*p01) + wy*((1 - wx)*p10 + wx*p11)
//   bilinear: floor(value + 0.5);  threshold: 255 where value >= 127.5, else 0;  0 where invalid.
// Every operation is float64 with one rounding (this file is built with -ffp-contract=off; + - * / are correctly rounded), so the
// source coordinates, the validity decision, the weights and the byte have the numpy path's bits.
//
// Work split: the coordinate map depends on the cameras only.  A lane owns a run of HGS_UNDIST_RUN = 4 output pixels of one row: it
// evaluates the map once for them, keeps the four tap offsets and weights in registers, and then walks the N images of the batch, so
// the distortion polynomial is paid once per pixel and not once per image.  Per image the lane gathers its taps (neighbouring lanes
// read neighbouring texels: the lines are shared in the vector L1) and stores its contiguous 4 C bytes -- as C dwords where they
// are 4-byte aligned, byte by byte otherwise (an odd row length, the last run of a row).  No LDS, no atomics.
#include "hgs_common.h"

#define HGS_UNDIST_RUN 4
enum { UD_SIMPLE_PINHOLE = 0, UD_PINHOLE = 1, UD_SIMPLE_RADIAL = 2, UD_RADIAL = 3, UD_OPENCV = 4, UD_FULL_OPENCV = 6 };   // COLMAP's model ids

namespace {

struct UndistortCameras {
  int model;
  double fx, fy, cx, cy, k1, k2, k3, k4, k5, k6, p1, p2;   // the source camera
  double dfx, dfy, dcx, dcy;                               // the output pinhole
};

struct Tap { int o00, dx, dy; bool valid; double wx, wy, omx, omy; };

__device__ __forceinline__ Tap undistort_tap(const UndistortCameras& c, int x, int y, int Hs, int Ws, int C) {
  const double u = (((double)x + 0.5) - c.dcx) / c.dfx, v = (((double)y + 0.5) - c.dcy) / c.dfy;
  double du = 0.0, dv = 0.0;
  if (c.model >= UD_SIMPLE_RADIAL) {                     // (wavefront-uniform)
    const double uu = u * u, vv = v * v, r2 = uu + vv;
    double rad;
    if (c.model == UD_SIMPLE_RADIAL) {
      rad = c.k1 * r2;
    } else if (c.model == UD_FULL_OPENCV) {
      const double r4 = r2 * r2, r6 = r4 * r2;
      rad = (((1.0 + c.k1 * r2) + c.k2 * r4) + c.k3 * r6) / (((1.0 + c.k4 * r2) + c.k5 * r4) + c.k6 * r6) - 1.0;
    } else {
      rad = c.k1 * r2 + c.k2 * (r2 * r2);
    }
    du = u * rad; dv = v * rad;
    if (c.model == UD_OPENCV || c.model == UD_FULL_OPENCV) {
      const double uv = u * v;
      du = (du + (2.0 * c.p1) * uv) + c.p2 * (r2 + 2.0 * uu);
      dv = (dv + (2.0 * c.p2) * uv) + c.p1 * (r2 + 2.0 * vv);
    }
  }
  const double sx = (c.fx * (u + du) + c.cx) - 0.5, sy = (c.fy * (v + dv) + c.cy) - 0.5;
  Tap t = {0, 0, 0, false, 0.0, 0.0, 1.0, 1.0};
  t.valid = sx >= 0.0 && sx <= (double)(Ws - 1) && sy >= 0.0 && sy <= (double)(Hs - 1);   // (false for a NaN)
  if (t.valid) {
    const double fx0 = floor(sx), fy0 = floor(sy);
    const int x0 = (int)fx0, y0 = (int)fy0;               // in [0, Ws - 1] x [0, Hs - 1]
    t.wx = sx - fx0; t.wy = sy - fy0;
    t.omx = 1.0 - t.wx; t.omy = 1.0 - t.wy;
    t.o00 = (y0 * Ws + x0) * C;
    t.dx = x0 + 1 <= Ws - 1 ? C : 0;
    t.dy = y0 + 1 <= Hs - 1 ? Ws * C : 0;
  }
  return t;
}

template <int C>
__global__ __launch_bounds__(256) void undistort_kernel(UndistortCameras cams, int N, int Hs, int Ws, int Hd, int Wd, int runs,
                                                        const unsigned char* __restrict__ src, unsigned char* __restrict__ dst,
                                                        unsigned char* __restrict__ valid, int mode) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)Hd * runs) return;
  const int y = (int)(idx / runs), xb = (int)(idx - (long long)y * runs) * HGS_UNDIST_RUN;
  const int npx = Wd - xb < HGS_UNDIST_RUN ? Wd - xb : HGS_UNDIST_RUN;      // 1..4 pixels of this lane
  Tap tap[HGS_UNDIST_RUN];
#pragma unroll
  for (int p = 0; p < HGS_UNDIST_RUN; p++) {
    tap[p] = undistort_tap(cams, xb + p < Wd ? xb + p : Wd - 1, y, Hs, Ws, C);
    if (p >= npx) tap[p].valid = false;
  }
  const size_t row = (size_t)y * Wd + xb;                  // first pixel of the run within an image
  if (valid) {
#pragma unroll
    for (int p = 0; p < HGS_UNDIST_RUN; p++)
      if (p < npx) valid[row + p] = tap[p].valid ? 1 : 0;
  }
  const size_t src_image = (size_t)Hs * Ws * C, dst_image = (size_t)Hd * Wd * C;
  for (int n = 0; n < N; n++) {
    const unsigned char* __restrict__ s = src + (size_t)n * src_image;
    unsigned int word[C] = {};                             // the run's 4 C bytes, little-endian
#pragma unroll
    for (int p = 0; p < HGS_UNDIST_RUN; p++) {
      if (!tap[p].valid) continue;                         // (its bytes stay 0: no source texel is read)
      const unsigned char* __restrict__ t0 = s + tap[p].o00;
      const unsigned char* __restrict__ t1 = t0 + tap[p].dy;
#pragma unroll
      for (int c = 0; c < C; c++) {
        const double p00 = (double)t0[c], p01 = (double)t0[tap[p].dx + c], p10 = (double)t1[c], p11 = (double)t1[tap[p].dx + c];
        const double value = tap[p].omy * (tap[p].omx * p00 + tap[p].wx * p01) + tap[p].wy * (tap[p].omx * p10 + tap[p].wx * p11);
        const unsigned int byte = mode == 0 ? (unsigned int)floor(value + 0.5) : (value >= 127.5 ? 255u : 0u);
        const int b = p * C + c;
        word[b >> 2] |= (byte & 0xFFu) << (8 * (b & 3));
      }
    }
    unsigned char* const d = dst + (size_t)n * dst_image + row * C;
    if (npx == HGS_UNDIST_RUN && ((size_t)d & 3) == 0) {
#pragma unroll
      for (int w = 0; w < C; w++) ((unsigned int*)d)[w] = word[w];
    } else {
#pragma unroll
      for (int b = 0; b < HGS_UNDIST_RUN * C; b++)
        if (b < npx * C) d[b] = (unsigned char)(word[b >> 2] >> (8 * (b & 3)));
    }
  }
}

}  // namespace

extern "C" int hgs_undistort_images(void* stream, int N, int C, int Hs, int Ws, int Hd, int Wd, int model, const double* src_params_host,
                                    const double* dst_pinhole_host, const unsigned char* src, unsigned char* dst, unsigned char* valid,
                                    int mode) {
  if (N <= 0 || Hs <= 0 || Ws <= 0 || Hd <= 0 || Wd <= 0) { hgs_set_error("hgs_undistort_images: bad sizes (N = %d, source %d x %d, output %d x %d)", N, Ws, Hs, Wd, Hd); return 1; }
  if (C != 1 && C != 3 && C != 4) { hgs_set_error("hgs_undistort_images: C = %d channels (1, 3 or 4)", C); return 1; }
  if (mode != 0 && mode != 1) { hgs_set_error("hgs_undistort_images: mode = %d (0: bilinear, 1: threshold)", mode); return 1; }
  if (model != UD_SIMPLE_PINHOLE && model != UD_PINHOLE && model != UD_SIMPLE_RADIAL && model != UD_RADIAL && model != UD_OPENCV &&
      model != UD_FULL_OPENCV) {
    hgs_set_error("hgs_undistort_images: camera model %d is not supported (SIMPLE_PINHOLE 0, PINHOLE 1, SIMPLE_RADIAL 2, RADIAL 3, OPENCV 4, FULL_OPENCV 6)", model);
    return 1;
  }
  if (!src_params_host || !dst_pinhole_host || !src || !dst) { hgs_set_error("hgs_undistort_images: null argument"); return 1; }
  if ((long long)Hs * Ws * C > 0x7FFFFFFFll || (long long)Hd * Wd * C > 0x7FFFFFFFll) {
    hgs_set_error("hgs_undistort_images: an image of more than 2^31 - 1 bytes"); return 1;
  }
  const double* p = src_params_host;
  UndistortCameras c = {};
  c.model = model;
  if (model == UD_SIMPLE_PINHOLE || model == UD_SIMPLE_RADIAL || model == UD_RADIAL) {
    c.fx = c.fy = p[0]; c.cx = p[1]; c.cy = p[2];
    if (model != UD_SIMPLE_PINHOLE) c.k1 = p[3];
    if (model == UD_RADIAL) c.k2 = p[4];
  } else {
    c.fx = p[0]; c.fy = p[1]; c.cx = p[2]; c.cy = p[3];
    if (model != UD_PINHOLE) { c.k1 = p[4]; c.k2 = p[5]; c.p1 = p[6]; c.p2 = p[7]; }
    if (model == UD_FULL_OPENCV) { c.k3 = p[8]; c.k4 = p[9]; c.k5 = p[10]; c.k6 = p[11]; }
  }
  c.dfx = dst_pinhole_host[0]; c.dfy = dst_pinhole_host[1]; c.dcx = dst_pinhole_host[2]; c.dcy = dst_pinhole_host[3];
  const int runs = (Wd + HGS_UNDIST_RUN - 1) / HGS_UNDIST_RUN;
  const long long lanes = (long long)Hd * runs;
  const dim3 grid((unsigned)((lanes + 255) / 256)), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (C == 1) hipLaunchKernelGGL(undistort_kernel<1>, grid, block, 0, s, c, N, Hs, Ws, Hd, Wd, runs, src, dst, valid, mode);
  else if (C == 3) hipLaunchKernelGGL(undistort_kernel<3>, grid, block, 0, s, c, N, Hs, Ws, Hd, Wd, runs, src, dst, valid, mode);
  else hipLaunchKernelGGL(undistort_kernel<4>, grid, block, 0, s, c, N, Hs, Ws, Hd, Wd, runs, src, dst, valid, mode);
  HGS_CHECK_LAUNCH();
  return 0;
}
