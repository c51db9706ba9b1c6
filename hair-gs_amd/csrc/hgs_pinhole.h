// hgs_pinhole.h -- how a world point becomes a pixel of a calibrated pinhole view, and when it counts as seen: the only device
// definition (utils/views.py is the numpy one; include/hgs.h states it for the ABI).  hgs_carve.hip, hgs_lift.hip and hgs_scalp.hip
// project through it.
//
// The contract (one definition for the numpy path, the kernels and the tests' loop restatements).  A view k is a pinhole camera with
// its pose, R row-major world -> camera, and planes [H][W] at the record's offsets.  For the point (x, y, z), all float64, one rounding
// per operation in the order written (every file that includes this header is built with -ffp-contract=off):
//   xc = ((R00*x + R01*y) + R02*z) + tx        (yc, zc likewise, rows 1 and 2)
//   u  = fx*(xc/zc) + cx,   v = fy*(yc/zc) + cy
//   seen iff zc > 0 and 0 <= u < W and 0 <= v < H      (any NaN: not seen);   px = floor(u), py = floor(v)
#pragma once
#include "hgs_common.h"

struct Pinhole { double xc, yc, zc, u, v; };   // camera coordinates and image point of one point in one view

__device__ __forceinline__ Pinhole pinhole_project(const HgsCarveView& c, double x, double y, double z) {
  Pinhole p;
  p.xc = ((c.R[0] * x + c.R[1] * y) + c.R[2] * z) + c.t[0];
  p.yc = ((c.R[3] * x + c.R[4] * y) + c.R[5] * z) + c.t[1];
  p.zc = ((c.R[6] * x + c.R[7] * y) + c.R[8] * z) + c.t[2];
  p.u = c.fx * (p.xc / p.zc) + c.cx;
  p.v = c.fy * (p.yc / p.zc) + c.cy;
  return p;
}

// The view goes by pointer here, on purpose.  A reference parameter is marked dereferenceable, so the optimiser may load W and H
// ahead of the tests; the five comparisons then fold into one block and are vectorised as <4 x double>, and the vote kernels took
// 4 % (carve), 10 % (lift) and 12 % (scalp) longer on an MI355X.  Through a pointer W and H are loaded where they are needed, and
// the comparisons stay a chain of branches: zc and u first, v's division behind them.
__device__ __forceinline__ bool pinhole_seen(const HgsCarveView* c, const Pinhole& p) {   // (false for a NaN)
  return p.zc > 0.0 && p.u >= 0.0 && p.u < (double)c->W && p.v >= 0.0 && p.v < (double)c->H;
}

// py*W + px of a seen point: px in [0, W - 1], py in [0, H - 1]
__device__ __forceinline__ size_t pinhole_pixel(const HgsCarveView& c, const Pinhole& p) {
  return (size_t)(int)floor(p.v) * (size_t)c.W + (size_t)(int)floor(p.u);
}
