// hgs_rescale.hip -- downscaling of a capture's images, masks and orientation pairs by area averaging (utils/rescale.py; rescale.py is
// the scene driver): hgs_rescale_images, hgs_rescale_orientation.  gfx950, wave64.
//
// The contract (one definition for the numpy path, these kernels and the tests; utils/rescale.py states it in full).  A source plane
// [Hs, Ws] becomes [Hd, Wd] with Wd <= Ws and Hd <= Hs.  Output column x covers lo = (x*Ws)/Wd to hi = ((x + 1)*Ws)/Wd (the products
// are exact integers); i0 = floor(lo), Kx = (Ws + Wd - 1)/Wd + 1 taps, tap k reads column min(i0 + k, Ws - 1) with the weight
// wx = min(i0 + k + 1, hi) - max(i0 + k, lo), replaced by 0 unless it is > 0; rows likewise.  Terms are visited ky outer, kx inner,
// w = wy*wx; a zero-weight term adds exactly nothing and is skipped here (so is the rest of its row or column: once a weight is not
// positive past the first tap, the later ones are not either).
//   images:  acc += w*p, A += w;  average: min(255, floor(acc/A + 0.5));  threshold: 255 where acc/A >= 127.5, else 0
//   pairs (angle byte t, confidence byte c, mask byte m; every pixel counts without a mask), per term with m != 0:
//            g = w*c, X += g*C[t], Y += g*S[t], Am += w      (C, S: the double-angle table the host built)
//            confidence: 0 if Am == 0, else min(255, floor(sqrt(X*X + Y*Y)/Am + 0.5))
//            angle: 0 if X == 0 and Y == 0, else (the number of the 255 half-step boundaries (HC[j], HS[j]) that (X, Y) is at or past) mod 255
// Every operation is float64 with one rounding (this file is built with -ffp-contract=off; + - * / sqrt are correctly rounded), and no
// trigonometric function is evaluated here, so the bytes are the numpy path's.
//
// Work split: one lane per output pixel, 256 consecutive columns of one output row of one plane per workgroup (grid: column blocks x
// rows x planes), so consecutive lanes read consecutive footprints of a source row.  The pair kernel stages the four tables (8 KB) in
// LDS: the table index is a byte of the lane's own pixel and the boundary search branches per lane, so neither is wavefront-uniform.
// No atomics, no scratch.
#include "hgs_common.h"

#define HGS_RESCALE_BLOCK 256

namespace {

// The footprint of one output index along one axis: first tap, and the float64 bounds the weights come from.
struct Foot { int i0; double lo, hi; };

__device__ __forceinline__ Foot rescale_foot(int x, int S, int D) {
  Foot f;
  f.lo = (double)((long long)x * S) / (double)D;
  f.hi = (double)((long long)(x + 1) * S) / (double)D;
  f.i0 = (int)floor(f.lo);
  return f;
}

__device__ __forceinline__ double rescale_weight(const Foot& f, int k) {
  const double a = (double)(f.i0 + k), b = (double)(f.i0 + k + 1);
  return (b < f.hi ? b : f.hi) - (a > f.lo ? a : f.lo);
}

template <int C>
__global__ __launch_bounds__(HGS_RESCALE_BLOCK) void rescale_images_kernel(int Hs, int Ws, int Hd, int Wd, int Kx, int Ky,
                                                                           const unsigned char* __restrict__ src,
                                                                           unsigned char* __restrict__ dst, int mode) {
  const int x = blockIdx.x * HGS_RESCALE_BLOCK + threadIdx.x, y = blockIdx.y;
  if (x >= Wd) return;
  const size_t n = blockIdx.z;
  const unsigned char* __restrict__ s = src + n * ((size_t)Hs * Ws * C);
  const Foot fx = rescale_foot(x, Ws, Wd), fy = rescale_foot(y, Hs, Hd);
  double acc[C] = {}, A = 0.0;
  for (int ky = 0; ky < Ky; ky++) {
    const double wy = rescale_weight(fy, ky);
    if (!(wy > 0.0)) break;
    const int row = fy.i0 + ky < Hs - 1 ? fy.i0 + ky : Hs - 1;
    const unsigned char* __restrict__ r = s + (size_t)row * Ws * C;
    for (int kx = 0; kx < Kx; kx++) {
      const double wx = rescale_weight(fx, kx);
      if (!(wx > 0.0)) break;
      const int col = fx.i0 + kx < Ws - 1 ? fx.i0 + kx : Ws - 1;
      const double w = wy * wx;
      A = A + w;
#pragma unroll
      for (int c = 0; c < C; c++) acc[c] = acc[c] + w * (double)r[(size_t)col * C + c];
    }
  }
  unsigned char* const d = dst + ((n * Hd + y) * Wd + x) * C;
#pragma unroll
  for (int c = 0; c < C; c++) {
    const double v = acc[c] / A;
    unsigned int byte;
    if (mode == 0) {
      byte = (unsigned int)floor(v + 0.5);
      byte = byte < 255u ? byte : 255u;
    } else {
      byte = v >= 127.5 ? 255u : 0u;
    }
    d[c] = (unsigned char)byte;
  }
}

__device__ __forceinline__ bool rescale_upper(double x, double y) { return y > 0.0 || (y == 0.0 && x > 0.0); }

__global__ __launch_bounds__(HGS_RESCALE_BLOCK) void rescale_orientation_kernel(int Hs, int Ws, int Hd, int Wd, int Kx, int Ky,
                                                                                const unsigned char* __restrict__ angle,
                                                                                const unsigned char* __restrict__ conf,
                                                                                const unsigned char* __restrict__ mask,
                                                                                const double* __restrict__ tables,
                                                                                unsigned char* __restrict__ angle_out,
                                                                                unsigned char* __restrict__ conf_out) {
  __shared__ double tab[4 * 256];                           // C[256], S[256], HC[256], HS[256] (entry 0 of the last two is unused)
  for (int i = threadIdx.x; i < 4 * 256; i += HGS_RESCALE_BLOCK) tab[i] = tables[i];
  __syncthreads();
  const int x = blockIdx.x * HGS_RESCALE_BLOCK + threadIdx.x, y = blockIdx.y;
  if (x >= Wd) return;
  const size_t plane = (size_t)blockIdx.z * ((size_t)Hs * Ws);
  const Foot fx = rescale_foot(x, Ws, Wd), fy = rescale_foot(y, Hs, Hd);
  double X = 0.0, Y = 0.0, Am = 0.0;
  for (int ky = 0; ky < Ky; ky++) {
    const double wy = rescale_weight(fy, ky);
    if (!(wy > 0.0)) break;
    const int row = fy.i0 + ky < Hs - 1 ? fy.i0 + ky : Hs - 1;
    const size_t r = plane + (size_t)row * Ws;
    for (int kx = 0; kx < Kx; kx++) {
      const double wx = rescale_weight(fx, kx);
      if (!(wx > 0.0)) break;
      const int col = fx.i0 + kx < Ws - 1 ? fx.i0 + kx : Ws - 1;
      if (mask && mask[r + col] == 0) continue;
      const double w = wy * wx;
      const int t = angle[r + col];
      const double g = w * (double)conf[r + col];
      X = X + g * tab[t];
      Y = Y + g * tab[256 + t];
      Am = Am + w;
    }
  }
  unsigned int cbyte = 0, tbyte = 0;
  if (Am != 0.0) {
    cbyte = (unsigned int)floor(sqrt(X * X + Y * Y) / Am + 0.5);
    cbyte = cbyte < 255u ? cbyte : 255u;
  }
  if (!(X == 0.0 && Y == 0.0)) {
    const bool vu = rescale_upper(X, Y);
    int count = 0;                                          // the largest j in 1..255 whose boundary (X, Y) is at or past: they ascend
#pragma unroll
    for (int b = 128; b >= 1; b >>= 1) {
      const int j = count + b;                              // <= 255
      const double hc = tab[512 + j], hs = tab[768 + j];
      const bool hu = rescale_upper(hc, hs);
      const bool past = hu != vu ? hu : (hc * Y - hs * X >= 0.0);
      if (past) count = j;
    }
    tbyte = count == 255 ? 0u : (unsigned int)count;
  }
  const size_t o = ((size_t)blockIdx.z * Hd + y) * Wd + x;
  angle_out[o] = (unsigned char)tbyte;
  conf_out[o] = (unsigned char)cbyte;
}

// The checks the two entry points share; Kx, Ky on success.
int rescale_check(const char* who, int N, int C, int Hs, int Ws, int Hd, int Wd, int* Kx, int* Ky) {
  if (N <= 0 || Hs <= 0 || Ws <= 0 || Hd <= 0 || Wd <= 0) { hgs_set_error("%s: bad sizes (N = %d, source %d x %d, output %d x %d)", who, N, Ws, Hs, Wd, Hd); return 1; }
  if (Wd > Ws || Hd > Hs) { hgs_set_error("%s: the output (%d x %d) is larger than the source (%d x %d): enlarging is not supported", who, Wd, Hd, Ws, Hs); return 1; }
  if ((long long)Hs * Ws * C > 0x7FFFFFFFll) { hgs_set_error("%s: a plane of more than 2^31 - 1 bytes", who); return 1; }
  if (N > 65535 || Hd > 65535) { hgs_set_error("%s: N = %d planes or %d output rows exceed the grid (65535 each)", who, N, Hd); return 1; }
  *Kx = (Ws + Wd - 1) / Wd + 1;
  *Ky = (Hs + Hd - 1) / Hd + 1;
  return 0;
}

}  // namespace

extern "C" int hgs_rescale_images(void* stream, int N, int C, int Hs, int Ws, int Hd, int Wd, const unsigned char* src, unsigned char* dst,
                                  int mode) {
  if (C != 1 && C != 3 && C != 4) { hgs_set_error("hgs_rescale_images: C = %d channels (1, 3 or 4)", C); return 1; }
  if (mode != 0 && mode != 1) { hgs_set_error("hgs_rescale_images: mode = %d (0: average, 1: threshold)", mode); return 1; }
  int Kx, Ky;
  if (rescale_check("hgs_rescale_images", N, C, Hs, Ws, Hd, Wd, &Kx, &Ky)) return 1;
  if (!src || !dst) { hgs_set_error("hgs_rescale_images: null argument"); return 1; }
  const dim3 grid((unsigned)((Wd + HGS_RESCALE_BLOCK - 1) / HGS_RESCALE_BLOCK), (unsigned)Hd, (unsigned)N), block(HGS_RESCALE_BLOCK);
  hipStream_t s = (hipStream_t)stream;
  if (C == 1) hipLaunchKernelGGL(rescale_images_kernel<1>, grid, block, 0, s, Hs, Ws, Hd, Wd, Kx, Ky, src, dst, mode);
  else if (C == 3) hipLaunchKernelGGL(rescale_images_kernel<3>, grid, block, 0, s, Hs, Ws, Hd, Wd, Kx, Ky, src, dst, mode);
  else hipLaunchKernelGGL(rescale_images_kernel<4>, grid, block, 0, s, Hs, Ws, Hd, Wd, Kx, Ky, src, dst, mode);
  HGS_CHECK_LAUNCH();
  return 0;
}

extern "C" int hgs_rescale_orientation(void* stream, int N, int Hs, int Ws, int Hd, int Wd, const unsigned char* angle,
                                       const unsigned char* conf, const unsigned char* mask, const double* tables,
                                       unsigned char* angle_out, unsigned char* conf_out) {
  int Kx, Ky;
  if (rescale_check("hgs_rescale_orientation", N, 1, Hs, Ws, Hd, Wd, &Kx, &Ky)) return 1;
  if (!angle || !conf || !tables || !angle_out || !conf_out) { hgs_set_error("hgs_rescale_orientation: null argument"); return 1; }
  const dim3 grid((unsigned)((Wd + HGS_RESCALE_BLOCK - 1) / HGS_RESCALE_BLOCK), (unsigned)Hd, (unsigned)N), block(HGS_RESCALE_BLOCK);
  hipLaunchKernelGGL(rescale_orientation_kernel, grid, block, 0, (hipStream_t)stream, Hs, Ws, Hd, Wd, Kx, Ky, angle, conf, mask, tables,
                     angle_out, conf_out);
  HGS_CHECK_LAUNCH();
  return 0;
}
