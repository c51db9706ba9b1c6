// hgs_jacobi3.h -- cyclic Jacobi on a symmetric 3 x 3 matrix held in registers (scalars and ?: selects, nothing indexed at run
// time): the eigen-solve of hgs_normals.hip (covariance of a point's neighbours) and hgs_lift.hip (moments of a point's image lines).
// What follows the sweeps -- column choice, sign rule, guards -- differs between the two and stays in each kernel.
#pragma once
#include "hgs_common.h"

#define HGS_JACOBI3_SWEEPS 12     // upper bound; a 3 x 3 matrix is diagonal to the last bit after 4-6

// One Jacobi rotation that annihilates a_pq of a symmetric 3 x 3 matrix (r: the third index); V's columns follow.
__device__ __forceinline__ void jacobi_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p, double& v0q,
                                              double& v1p, double& v1q, double& v2p, double& v2q, bool late) {
  if (apq == 0.0) return;
  const double g = 100.0 * fabs(apq);
  if (late && fabs(app) + g == fabs(app) && fabs(aqq) + g == fabs(aqq)) { apq = 0.0; return; }
  const double h = aqq - app;
  double t;
  if (fabs(h) + g == fabs(h)) {
    t = apq / h;
  } else {
    const double th = 0.5 * h / apq;
    t = 1.0 / (fabs(th) + sqrt(1.0 + th * th));
    if (th < 0.0) t = -t;
  }
  const double c = 1.0 / sqrt(1.0 + t * t), s = t * c, tau = s / (1.0 + c);
  const double hh = t * apq;
  app = app - hh;
  aqq = aqq + hh;
  apq = 0.0;
  const double p0 = arp, q0 = arq;
  arp = p0 - s * (q0 + p0 * tau);
  arq = q0 + s * (p0 - q0 * tau);
  double a, b;
  a = v0p; b = v0q; v0p = a - s * (b + a * tau); v0q = b + s * (a - b * tau);
  a = v1p; b = v1q; v1p = a - s * (b + a * tau); v1q = b + s * (a - b * tau);
  a = v2p; b = v2q; v2p = a - s * (b + a * tau); v2q = b + s * (a - b * tau);
}

// The sweeps: A is diagonalised in place (its eigenvalues end up in a00, a11, a22) and V, the identity to begin with, collects the
// rotations, so column j of V is the eigenvector of a_jj.  Every lane that holds the same A takes the same path.
__device__ __forceinline__ void jacobi3_sweeps(double& a00, double& a01, double& a02, double& a11, double& a12, double& a22, double& v00,
                                               double& v01, double& v02, double& v10, double& v11, double& v12, double& v20, double& v21,
                                               double& v22) {
  v00 = 1.0; v01 = 0.0; v02 = 0.0; v10 = 0.0; v11 = 1.0; v12 = 0.0; v20 = 0.0; v21 = 0.0; v22 = 1.0;
  for (int s = 0; s < HGS_JACOBI3_SWEEPS; s++) {
    if (fabs(a01) + fabs(a02) + fabs(a12) == 0.0) break;
    const bool late = s >= 3;
    jacobi_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21, late);
    jacobi_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22, late);
    jacobi_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22, late);
  }
}
