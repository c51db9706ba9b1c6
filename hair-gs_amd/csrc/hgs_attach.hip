// hgs_attach.hip -- exported strands rooted on the head (hgs_root_attach, hgs_strand_rejoin; scene/strand_attach.py states the
// contract, its numpy path and the loop restatement in tests/attach_reference.py state the same thing).  gfx950, wave64.  Built with
// -ffp-contract=off: every operation below is rounded once, in the order written.  The strand arithmetic is float64, dot(u, v) =
// (u0*v0 + u1*v1) + u2*v2; the head's field is sampled by the float32 statement of hgs_sdf_sample.h (the one head_penalty_kernel and
// strand_collide_kernel use), the direction volume by the corner loop of utils/trace.py's Trace statement.
//
// root_attach_kernel: one lane per strand, 256 strands per workgroup.  A march is a dependent chain of samples (eight gathers of the
//   field, and sixteen of the volume where one is given and the point is in its range), the parallelism is the strands.  Nothing is
//   shared between lanes: no LDS, no atomics, bitwise reproducible.  Every load has its range test in front of it; the loops are
//   bounded by max_steps and land_iters.
// strand_rejoin_kernel: one lane per strand.  A strand that did not reach the head is copied.  One that did gets its new joints
//   (the march in reverse, rounded once to float32) in front of its own, or, with M >= 2, M samples of that polyline by arc length:
//   the lane sums the total length in segment order, then walks the samples with a running cum_i (the same sum, so the same bits
//   as a cum table would hold) -- t grows with j, so the segment index only moves forward.
#include "hgs_common.h"
#include "hgs_sdf_sample.h"

#include <math.h>

#define HGS_ATTACH_MAX_STEPS 1024
#define HGS_ATTACH_MAX_LAND 8
#define HGS_ATTACH_MAX_CHANNELS 64

namespace {

#define ATTACH_BLOCK 256

enum { AT_REACHED = 0, AT_NEAR = 1, AT_DEGENERATE = 2, AT_RANGE = 3, AT_FLAT = 4, AT_STEPS = 5, AT_UNLANDED = 6, AT_FAR = 7 };

struct D3 { double x, y, z; };

__device__ __forceinline__ double adot(const D3& u, const D3& v) { return (u.x * v.x + u.y * v.y) + u.z * v.z; }
__device__ __forceinline__ bool positive_finite(double v) { return v > 0.0 && v < __builtin_inf(); }

struct Head {
  const float* __restrict__ phi;
  int nx, ny, nz;
  float ox, oy, oz, inv_h;
};

struct Volume {                       // dir == nullptr: no volume
  const double* __restrict__ dir;
  const double* __restrict__ conf;
  int nx, ny, nz;
  double ox, oy, oz, k, min_conf;
};

// S(x): the float32 statement at p = float32(x); a point that is not finite or out of range has ok false
__device__ __forceinline__ bool attach_sample(const Head& f, const D3& x, float& d, D3& G) {
  float tx, ty, tz;
  if (!sdf_grid_coords((float)x.x, (float)x.y, (float)x.z, f.ox, f.oy, f.oz, f.inv_h, f.nx, f.ny, f.nz, tx, ty, tz)) return false;
  const SdfCell cell = sdf_cell(f.phi, f.nx, f.ny, tx, ty, tz);
  d = sdf_value(cell);
  float gx, gy, gz;
  sdf_gradient(cell, f.inv_h, gx, gy, gz);
  G.x = (double)gx; G.y = (double)gy; G.z = (double)gz;
  return true;
}

// the volume's direction at x, sign-aligned to p (the corner loop of utils/trace.py); false where x is out of its range, the aligned
// mass is below min_conf or the sum has no direction
__device__ __forceinline__ bool attach_steer(const Volume& V, const D3& x, const D3& p, D3& f) {
  const double tx = (x.x - V.ox) * V.k, ty = (x.y - V.oy) * V.k, tz = (x.z - V.oz) * V.k;
  if (!(tx >= 0.0 && tx < (double)(V.nx - 1) && ty >= 0.0 && ty < (double)(V.ny - 1) && tz >= 0.0 && tz < (double)(V.nz - 1))) return false;
  const double flx = floor(tx), fly = floor(ty), flz = floor(tz);
  const int ix = (int)flx, iy = (int)fly, iz = (int)flz;                          // 0 <= i <= n - 2
  const double fx = tx - flx, fy = ty - fly, fz = tz - flz;
  const double gx0 = 1.0 - fx, gy0 = 1.0 - fy, gz0 = 1.0 - fz;
  const size_t sy = (size_t)V.nx, sz = (size_t)V.nx * V.ny;
  const size_t base = ((size_t)iz * V.ny + iy) * V.nx + ix;
  double w = 0.0, v0 = 0.0, v1 = 0.0, v2 = 0.0;
#pragma unroll
  for (int c = 0; c < 8; c++) {                                                   // z outermost, then y, then x, each 0 then 1
    const int cx = c & 1, cy = (c >> 1) & 1, cz = c >> 2;
    const size_t at = base + (cz ? sz : 0) + (cy ? sy : 0) + (size_t)cx;
    const double tw = ((cx ? fx : gx0) * (cy ? fy : gy0)) * (cz ? fz : gz0);
    double a = tw * V.conf[at];
    w = w + a;
    const double e0 = V.dir[3 * at], e1 = V.dir[3 * at + 1], e2 = V.dir[3 * at + 2];
    if (dot3(e0, e1, e2, p.x, p.y, p.z) < 0.0) a = -a;
    v0 = v0 + a * e0; v1 = v1 + a * e1; v2 = v2 + a * e2;
  }
  const double nn = dot3(v0, v1, v2, v0, v1, v2);
  if (!(w >= V.min_conf && positive_finite(nn))) return false;
  const double len = sqrt(nn);
  f.x = v0 / len; f.y = v1 / len; f.z = v2 / len;
  return true;
}

__global__ __launch_bounds__(ATTACH_BLOCK) void root_attach_kernel(int K, const long long* __restrict__ offsets, long long P,
                                                                   const float* __restrict__ points, Head H, Volume V, float margin,
                                                                   float tol, double step, int max_steps, int land_iters, double pull,
                                                                   double descent, double max_distance, double* __restrict__ ext,
                                                                   int* __restrict__ count, int* __restrict__ reason,
                                                                   float* __restrict__ landed) {
  const int s = blockIdx.x * ATTACH_BLOCK + threadIdx.x;
  if (s >= K) return;
  const long long a = offsets[s], b = offsets[s + 1];
  int n_ext = 0, why = AT_DEGENERATE;
  float d_out = __builtin_inff();
  // (the offsets are the caller's duty; a range that is not inside the P points counts as a strand without joints)
  if (a >= 0 && b <= P && b - a >= 2) {
    const float* const p01 = points + 3 * (size_t)a;
    double* const E = ext + 3 * (size_t)s * (size_t)(max_steps + 1);
    const double m = (double)margin, tl = (double)tol;
    D3 x = {(double)p01[0], (double)p01[1], (double)p01[2]};
    D3 G = {0.0, 0.0, 0.0};
    float d = 0.f;
    if (!attach_sample(H, x, d, G)) {
      why = AT_RANGE;
    } else if ((double)d <= m + tl) {
      why = AT_NEAR;
      d_out = d;
    } else if ((double)d - m > max_distance) {
      why = AT_FAR;
    } else {
      const D3 e = {x.x - (double)p01[3], x.y - (double)p01[4], x.z - (double)p01[5]};
      const double le = sqrt(adot(e, e));
      D3 p;
      if (positive_finite(le)) {
        p.x = e.x / le; p.y = e.y / le; p.z = e.z / le;
      } else {
        const double g0 = sqrt(adot(G, G));
        p.x = -G.x / g0; p.y = -G.y / g0; p.z = -G.z / g0;
      }
      why = AT_STEPS;
      for (int it = 0; it < max_steps; it++) {
        double gn = sqrt(adot(G, G));
        if (!positive_finite(gn)) { why = AT_FLAT; break; }
        if ((double)d - m <= step) {                                              // the landing: Newton steps along the gradient
          why = AT_UNLANDED;
          for (int l = 0; l < land_iters; l++) {
            const double c = (m - (double)d) / gn;
            x.x = x.x + (c * G.x) / gn; x.y = x.y + (c * G.y) / gn; x.z = x.z + (c * G.z) / gn;
            if (!attach_sample(H, x, d, G)) { why = AT_RANGE; break; }
            if (fabs((double)d - m) <= tl) {
              E[3 * n_ext] = x.x; E[3 * n_ext + 1] = x.y; E[3 * n_ext + 2] = x.z;
              n_ext++;
              d_out = d;
              why = AT_REACHED;
              break;
            }
            gn = sqrt(adot(G, G));
            if (!positive_finite(gn)) { why = AT_FLAT; break; }
          }
          break;
        }
        const D3 nrm = {-G.x / gn, -G.y / gn, -G.z / gn};
        D3 f = p;
        if (V.dir != nullptr) {
          D3 fv;
          if (attach_steer(V, x, p, fv)) f = fv;
        }
        const D3 v = {f.x + pull * nrm.x, f.y + pull * nrm.y, f.z + pull * nrm.z};
        const double vn = sqrt(adot(v, v));
        D3 dd = nrm;
        if (positive_finite(vn)) { dd.x = v.x / vn; dd.y = v.y / vn; dd.z = v.z / vn; }
        if (adot(dd, nrm) < descent) dd = nrm;
        x.x = x.x + step * dd.x; x.y = x.y + step * dd.y; x.z = x.z + step * dd.z;
        p = dd;
        E[3 * n_ext] = x.x; E[3 * n_ext + 1] = x.y; E[3 * n_ext + 2] = x.z;      // n_ext <= it < max_steps: inside the strand's rows
        n_ext++;
        if (!attach_sample(H, x, d, G)) { why = AT_RANGE; break; }
      }
    }
  }
  count[s] = n_ext;
  reason[s] = why;
  landed[s] = d_out;
}

// joint i of the joined polyline: the march's joints in reverse, rounded once to float32, then the strand's own
__device__ __forceinline__ D3 joined(const double* __restrict__ E, int cnt, const float* __restrict__ p, long long i) {
  if (i < cnt) {
    const double* r = E + 3 * (size_t)(cnt - 1 - i);
    return {(double)(float)r[0], (double)(float)r[1], (double)(float)r[2]};
  }
  const float* q = p + 3 * (size_t)(i - cnt);
  return {(double)q[0], (double)q[1], (double)q[2]};
}

__device__ __forceinline__ double seg_len(const D3& u, const D3& v) {
  const D3 e = {v.x - u.x, v.y - u.y, v.z - u.z};
  return sqrt(adot(e, e));
}

__global__ __launch_bounds__(ATTACH_BLOCK) void strand_rejoin_kernel(int K, const long long* __restrict__ offsets, long long P,
                                                                     const float* __restrict__ points, const float* __restrict__ attrs,
                                                                     int C, const double* __restrict__ ext, int ext_rows,
                                                                     const int* __restrict__ count, const int* __restrict__ reason, int M,
                                                                     const long long* __restrict__ out_offsets, long long n_out,
                                                                     float* __restrict__ out_points, float* __restrict__ out_attrs) {
  const int s = blockIdx.x * ATTACH_BLOCK + threadIdx.x;
  if (s >= K) return;
  const long long a = offsets[s], b = offsets[s + 1], oa = out_offsets[s], ob = out_offsets[s + 1];
  if (!(a >= 0 && b >= a && b <= P && oa >= 0 && ob >= oa && ob <= n_out)) return;
  const long long n = b - a;
  const int cnt = count[s];
  const bool reached = reason[s] == AT_REACHED && cnt >= 1 && cnt <= ext_rows && n >= 1;
  const long long want = !reached ? n : (M > 0 ? (long long)M : n + cnt);
  if (ob - oa != want) return;                                                     // (never written out of the caller's rows)
  const float* const p = points + 3 * (size_t)a;
  const float* const at = attrs + (size_t)C * (size_t)a;
  float* const o = out_points + 3 * (size_t)oa;
  float* const oat = out_attrs + (size_t)C * (size_t)oa;
  if (!reached) {
    for (long long j = 0; j < n; j++) {
      o[3 * j] = p[3 * j]; o[3 * j + 1] = p[3 * j + 1]; o[3 * j + 2] = p[3 * j + 2];
      for (int c = 0; c < C; c++) oat[(size_t)C * j + c] = at[(size_t)C * j + c];
    }
    return;
  }
  const double* const E = ext + 3 * (size_t)s * (size_t)ext_rows;
  if (M == 0) {
    for (int j = 0; j < cnt; j++) {
      const double* r = E + 3 * (size_t)(cnt - 1 - j);
      o[3 * j] = (float)r[0]; o[3 * j + 1] = (float)r[1]; o[3 * j + 2] = (float)r[2];
      for (int c = 0; c < C; c++) oat[(size_t)C * j + c] = at[c];                  // the new joints carry the root joint's attributes
    }
    for (long long j = 0; j < n; j++) {
      const long long k = cnt + j;
      o[3 * k] = p[3 * j]; o[3 * k + 1] = p[3 * j + 1]; o[3 * k + 2] = p[3 * j + 2];
      for (int c = 0; c < C; c++) oat[(size_t)C * k + c] = at[(size_t)C * j + c];
    }
    return;
  }
  const long long m = n + cnt;                                                     // joints of the joined polyline, >= 2
  double L = 0.0;
  {
    D3 u = joined(E, cnt, p, 0);
    for (long long i = 0; i + 1 < m; i++) {
      const D3 v = joined(E, cnt, p, i + 1);
      L = L + seg_len(u, v);
      u = v;
    }
  }
  // the end samples are the end joints themselves
  {
    const double* r = E + 3 * (size_t)(cnt - 1);
    o[0] = (float)r[0]; o[1] = (float)r[1]; o[2] = (float)r[2];
    const size_t z = (size_t)(M - 1);
    o[3 * z] = p[3 * (n - 1)]; o[3 * z + 1] = p[3 * (n - 1) + 1]; o[3 * z + 2] = p[3 * (n - 1) + 2];
    for (int c = 0; c < C; c++) {
      oat[c] = at[c];
      oat[(size_t)C * z + c] = at[(size_t)C * (n - 1) + c];
    }
  }
  long long i = 0;
  double cum = 0.0;
  D3 va = joined(E, cnt, p, 0), vb = joined(E, cnt, p, 1);
  double len = seg_len(va, vb);
  for (int j = 1; j < M - 1; j++) {
    const double t = ((double)j / (double)(M - 1)) * L;
    while (i < m - 2 && cum + len <= t) {                                          // the largest i with cum_i <= t, at most m - 2
      cum = cum + len;
      i++;
      va = vb;
      vb = joined(E, cnt, p, i + 1);
      len = seg_len(va, vb);
    }
    const double w = len > 0.0 ? (t - cum) / len : 0.0;
    o[3 * (size_t)j] = (float)(va.x + w * (vb.x - va.x));
    o[3 * (size_t)j + 1] = (float)(va.y + w * (vb.y - va.y));
    o[3 * (size_t)j + 2] = (float)(va.z + w * (vb.z - va.z));
    const float* const a0 = at + (size_t)C * (size_t)(i < cnt ? 0 : i - cnt);      // joint i's attributes, joint i + 1's
    const float* const a1 = at + (size_t)C * (size_t)(i + 1 < cnt ? 0 : i + 1 - cnt);
    for (int c = 0; c < C; c++) {
      const double u0 = (double)a0[c];
      oat[(size_t)C * j + c] = (float)(u0 + w * ((double)a1[c] - u0));
    }
  }
}

int head_check(const char* who, int nx, int ny, int nz, float ox, float oy, float oz, float inv_h) {
  if (nx < 2 || ny < 2 || nz < 2 || nx > 1024 || ny > 1024 || nz > 1024) {
    hgs_set_error("%s: a head field of %d x %d x %d nodes (2 to 1024 an axis)", who, nx, ny, nz);
    return 1;
  }
  if (!(inv_h > 0.f) || !isfinite(inv_h) || !isfinite(ox) || !isfinite(oy) || !isfinite(oz)) {
    hgs_set_error("%s: the head field's origin (%g, %g, %g) and 1/h = %g must be finite, 1/h > 0", who, (double)ox, (double)oy, (double)oz,
                  (double)inv_h);
    return 1;
  }
  return 0;
}

}  // namespace

extern "C" int hgs_root_attach(void* stream, int K, const long long* offsets, long long P, const float* points, const float* phi, int nx,
                               int ny, int nz, float ox, float oy, float oz, float inv_h, const double* vol_dir, const double* vol_conf,
                               int vnx, int vny, int vnz, double vox, double voy, double voz, double vh, double min_conf, float margin,
                               float tol, double step, int max_steps, int land_iters, double pull, double descent, double max_distance,
                               double* ext, int* count, int* reason, float* landed) {
  if (K < 0 || P < 0) { hgs_set_error("hgs_root_attach: bad sizes (%d strands, %lld points)", K, P); return 1; }
  if (max_steps < 1 || max_steps > HGS_ATTACH_MAX_STEPS) {
    hgs_set_error("hgs_root_attach: max_steps = %d outside [1, %d]", max_steps, HGS_ATTACH_MAX_STEPS); return 1;
  }
  if (land_iters < 1 || land_iters > HGS_ATTACH_MAX_LAND) {
    hgs_set_error("hgs_root_attach: land_iters = %d outside [1, %d]", land_iters, HGS_ATTACH_MAX_LAND); return 1;
  }
  if (!(margin >= 0.f) || !isfinite(margin) || !(tol >= 0.f) || !isfinite(tol)) {
    hgs_set_error("hgs_root_attach: margin %g and tol %g must be finite and >= 0", (double)margin, (double)tol);
    return 1;
  }
  if (!(step > 0.0) || !isfinite(step) || !(pull >= 0.0) || !isfinite(pull) || !(descent > 0.0) || !(descent <= 1.0) || !(max_distance >= 0.0)) {
    hgs_set_error("hgs_root_attach: step = %g (finite and > 0), pull = %g (finite and >= 0), descent = %g (0 < descent <= 1), "
                  "max_distance = %g (>= 0, may be infinite)", step, pull, descent, max_distance);
    return 1;
  }
  if (head_check("hgs_root_attach", nx, ny, nz, ox, oy, oz, inv_h)) return 1;
  if ((vol_dir == nullptr) != (vol_conf == nullptr)) { hgs_set_error("hgs_root_attach: the volume's dir and conf come together, or neither"); return 1; }
  if (vol_dir != nullptr) {
    if (vnx < 2 || vny < 2 || vnz < 2 || vnx > 1024 || vny > 1024 || vnz > 1024 || (long long)vnx * vny * vnz > (1ll << 26)) {
      hgs_set_error("hgs_root_attach: a volume of %d x %d x %d nodes (2 to 1024 an axis, at most 2^26 in all)", vnx, vny, vnz);
      return 1;
    }
    if (!(vh > 0.0) || !isfinite(vh) || !isfinite(vox) || !isfinite(voy) || !isfinite(voz) || !isfinite(1.0 / vh) || !(1.0 / vh > 0.0) ||
        !isfinite(min_conf)) {
      hgs_set_error("hgs_root_attach: the volume's origin (%g, %g, %g), spacing %g and min_conf %g must be finite, the spacing and "
                    "1/spacing > 0", vox, voy, voz, vh, min_conf);
      return 1;
    }
  }
  if (K == 0) return 0;
  if (!offsets || !phi || !ext || !count || !reason || !landed || (P > 0 && !points)) {
    hgs_set_error("hgs_root_attach: null argument");
    return 1;
  }
  if ((const void*)ext == (const void*)points || (const void*)ext == (const void*)phi || (const void*)ext == (const void*)vol_dir ||
      (const void*)ext == (const void*)vol_conf || (const void*)ext == (const void*)offsets || (const void*)count == (const void*)reason ||
      (const void*)landed == (const void*)phi || (const void*)landed == (const void*)points) {
    hgs_set_error("hgs_root_attach: the outputs must not alias the inputs or each other");
    return 1;
  }
  const Head H = {phi, nx, ny, nz, ox, oy, oz, inv_h};
  Volume V = {nullptr, nullptr, 2, 2, 2, 0.0, 0.0, 0.0, 1.0, 0.0};
  if (vol_dir != nullptr) V = {vol_dir, vol_conf, vnx, vny, vnz, vox, voy, voz, 1.0 / vh, min_conf};
  hipLaunchKernelGGL(root_attach_kernel, dim3((unsigned)((K + ATTACH_BLOCK - 1) / ATTACH_BLOCK)), dim3(ATTACH_BLOCK), 0, (hipStream_t)stream,
                     K, offsets, P, points, H, V, margin, tol, step, max_steps, land_iters, pull, descent, max_distance, ext, count, reason,
                     landed);
  HGS_CHECK_LAUNCH();
  return 0;
}

extern "C" int hgs_strand_rejoin(void* stream, int K, const long long* offsets, long long P, const float* points, const float* attrs, int C,
                                 const double* ext, int ext_rows, const int* count, const int* reason, int M, const long long* out_offsets,
                                 long long n_out, float* out_points, float* out_attrs) {
  if (K < 0 || P < 0 || n_out < 0) { hgs_set_error("hgs_strand_rejoin: bad sizes (%d strands, %lld points in, %lld out)", K, P, n_out); return 1; }
  if (C < 0 || C > HGS_ATTACH_MAX_CHANNELS) { hgs_set_error("hgs_strand_rejoin: %d attribute channels (0 to %d)", C, HGS_ATTACH_MAX_CHANNELS); return 1; }
  if (M < 0 || M == 1) { hgs_set_error("hgs_strand_rejoin: M = %d (0 for the joints themselves, else at least 2)", M); return 1; }
  if (ext_rows < 2 || ext_rows > HGS_ATTACH_MAX_STEPS + 1) {
    hgs_set_error("hgs_strand_rejoin: ext_rows = %d outside [2, %d]", ext_rows, HGS_ATTACH_MAX_STEPS + 1); return 1;
  }
  if (K == 0) return 0;
  if (!offsets || !out_offsets || !ext || !count || !reason || (P > 0 && (!points || (C > 0 && !attrs))) ||
      (n_out > 0 && (!out_points || (C > 0 && !out_attrs)))) {
    hgs_set_error("hgs_strand_rejoin: null argument");
    return 1;
  }
  if (n_out > 0 && ((const void*)out_points == (const void*)points || (const void*)out_points == (const void*)attrs ||
                    (const void*)out_points == (const void*)ext || (C > 0 && ((const void*)out_attrs == (const void*)attrs ||
                    (const void*)out_attrs == (const void*)points || (const void*)out_attrs == (const void*)ext ||
                    (const void*)out_attrs == (const void*)out_points)))) {
    hgs_set_error("hgs_strand_rejoin: the outputs must not alias the inputs or each other");
    return 1;
  }
  hipLaunchKernelGGL(strand_rejoin_kernel, dim3((unsigned)((K + ATTACH_BLOCK - 1) / ATTACH_BLOCK)), dim3(ATTACH_BLOCK), 0,
                     (hipStream_t)stream, K, offsets, P, points, attrs, C, ext, ext_rows, count, reason, M, out_offsets, n_out, out_points,
                     out_attrs);
  HGS_CHECK_LAUNCH();
  return 0;
}
