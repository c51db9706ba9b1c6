// hgs_raster.hip -- the line / triangle rasterizer of the dataset synthesis (scene/mesh_renderer.py states the contract; the
// reference renders its captures with OpenGL).  Every decision is made in integers and every float operation is float64, in the
// order the CPU path evaluates it (this file is built with -ffp-contract=off): the two backends give the same bytes.
//
// For V views of the selected models (an HgsRasterModel table in list order; primitive ids are draw indices):
//   * raster_vertex_kernel: one lane per (view, vertex): c = P (Vw p_w) -> snapped window X, Y (int32, 1/256 px), z_w, c.w;
//     X = INT_MIN marks a vertex that drops its primitives.
//   * raster_count_kernel: one lane per (view, primitive): the number of 32x32 screen tiles it reaches (lines: exactly, from the
//     column span, whose minor extent over a tile column is the band between its end columns; triangles: the bounding box of the
//     covered pixel centres), added to the tile's counter; dropped primitives are counted instead.
//   * (the caller scans the counters into offsets)
//   * raster_fill_kernel: the same enumeration again, placing the draw index into the tile's list through a per-tile cursor.
//     No sort: the depth key carries the draw order, so the order inside a list does not matter.
//   * raster_resolve_kernel: one 256-lane workgroup per (view, tile): the 32x32 keys (d << 32 | draw) live in 8 KB of LDS, cleared
//     to all ones; each lane rasterizes one listed primitive at a time into the tile through ds_min_u64; after a barrier each lane
//     takes 4 pixels, recomputes the winning primitive's interpolation from its id, shades it and writes RGB (and gray).
#include "hgs_common.h"

#include <climits>

namespace {

#define RS_BLOCK 256
#define RS_TILE 32
#define RS_DMAX 16777215ll              // 2^24 - 1
#define RS_NONE 0xFFFFFFFFFFFFFFFFull

struct VOut {
  double z, w;
  int X, Y;                             // X == INT_MIN: dropped vertex
};

__device__ __forceinline__ long long fdiv(long long a, long long b) {   // floor(a / b), b > 0
  long long q = a / b;
  if ((a % b) != 0 && a < 0) q--;
  return q;
}
__device__ __forceinline__ long long cdiv(long long a, long long b) { return -fdiv(-a, b); }

__device__ __forceinline__ double row4(const double* m, double x, double y, double z, double w) {
  return ((m[0] * x + m[1] * y) + m[2] * z) + m[3] * w;
}

__global__ __launch_bounds__(RS_BLOCK) void raster_vertex_kernel(int NV, int W, int H, const double* __restrict__ pw,
                                                                 const double* __restrict__ views, const double* __restrict__ projs,
                                                                 VOut* __restrict__ out) {
  const int i = blockIdx.x * RS_BLOCK + threadIdx.x, v = blockIdx.y;
  if (i >= NV) return;
  const double* Vm = views + 16 * v;
  const double* Pm = projs + 16 * v;
  const double x = pw[4 * (size_t)i], y = pw[4 * (size_t)i + 1], z = pw[4 * (size_t)i + 2], w = pw[4 * (size_t)i + 3];
  double e[4], c[4];
  for (int r = 0; r < 4; r++) e[r] = row4(Vm + 4 * r, x, y, z, w);
  for (int r = 0; r < 4; r++) c[r] = row4(Pm + 4 * r, e[0], e[1], e[2], e[3]);
  const double cw = c[3];
  const double xw = ((c[0] / cw) * 0.5 + 0.5) * (double)W;
  const double yw = ((c[1] / cw) * 0.5 + 0.5) * (double)H;
  const double zw = (c[2] / cw) * 0.5 + 0.5;
  const double lim = 16384.0;
  const bool ok = cw > 0.0 && fabs(c[2]) <= cw && fabs(xw) <= lim && fabs(yw) <= lim;
  VOut o;
  o.z = zw;
  o.w = cw;
  o.X = ok ? (int)rint(256.0 * xw) : INT_MIN;
  o.Y = ok ? (int)rint(256.0 * yw) : 0;
  out[(size_t)v * NV + i] = o;
}

__device__ __forceinline__ int find_model(const HgsRasterModel* t, int n, long long d) {
  int m = 0;
  for (int k = 1; k < n; k++)
    if (t[k].draw_base <= d) m = k;                  // (an empty model shares its base with the next one, which owns d)
  return m;
}

// A line in (major U, minor V) coordinates with its clipped major pixel range [k0, k1].
struct Line {
  long long Ua, Va, Ub, Vb, k0, k1;
  int xmaj, Wu, Wv;
};

__device__ __forceinline__ bool line_setup(const VOut& a, const VOut& b, int W, int H, Line& L) {
  const long long Xa = a.X, Ya = a.Y, Xb = b.X, Yb = b.Y;
  L.xmaj = llabs(Xb - Xa) >= llabs(Yb - Ya);
  L.Ua = L.xmaj ? Xa : Ya;
  L.Va = L.xmaj ? Ya : Xa;
  L.Ub = L.xmaj ? Xb : Yb;
  L.Vb = L.xmaj ? Yb : Xb;
  L.Wu = L.xmaj ? W : H;
  L.Wv = L.xmaj ? H : W;
  if (L.Ua <= L.Ub) {
    L.k0 = cdiv(L.Ua - 128, 256);
    L.k1 = cdiv(L.Ub - 128, 256) - 1;
  } else {
    L.k0 = fdiv(L.Ub - 128, 256) + 1;
    L.k1 = fdiv(L.Ua - 128, 256);
  }
  if (L.k0 < 0) L.k0 = 0;
  if (L.k1 > L.Wu - 1) L.k1 = L.Wu - 1;
  return L.k0 <= L.k1;
}

__device__ __forceinline__ long long line_minor(const Line& L, long long Cu) {
  long long num = (Cu - L.Ua) * (L.Vb - L.Va), dU = L.Ub - L.Ua;
  if (dU < 0) { num = -num; dU = -dU; }
  return L.Va + fdiv(num, dU);
}

__device__ __forceinline__ double line_t(const Line& L, long long Cu) { return (double)(Cu - L.Ua) / (double)(L.Ub - L.Ua); }

struct Tri {
  long long X0, Y0, X1, Y1, X2, Y2, A;
  int i0, i1, j0, j1;
};

__device__ __forceinline__ bool tri_setup(const VOut& a, const VOut& b, const VOut& c, int W, int H, Tri& T) {
  T.X0 = a.X; T.Y0 = a.Y; T.X1 = b.X; T.Y1 = b.Y; T.X2 = c.X; T.Y2 = c.Y;
  T.A = (T.X1 - T.X0) * (T.Y2 - T.Y0) - (T.X2 - T.X0) * (T.Y1 - T.Y0);
  if (T.A <= 0) return false;
  const long long xmn = min(T.X0, min(T.X1, T.X2)), xmx = max(T.X0, max(T.X1, T.X2));
  const long long ymn = min(T.Y0, min(T.Y1, T.Y2)), ymx = max(T.Y0, max(T.Y1, T.Y2));
  T.i0 = (int)max(cdiv(xmn - 128, 256), 0ll);
  T.i1 = (int)min(fdiv(xmx - 128, 256), (long long)W - 1);
  T.j0 = (int)max(cdiv(ymn - 128, 256), 0ll);
  T.j1 = (int)min(fdiv(ymx - 128, 256), (long long)H - 1);
  return T.i0 <= T.i1 && T.j0 <= T.j1;
}

__device__ __forceinline__ bool inside(long long E, long long dX, long long dY) {
  return E > 0 || (E == 0 && (dY < 0 || (dY == 0 && dX < 0)));
}

// coverage and barycentrics b_k = E_k / A at the centre of pixel (i, j)
__device__ __forceinline__ bool tri_bary(const Tri& T, int i, int j, double& b0, double& b1, double& b2) {
  const long long Px = 256ll * i + 128, Py = 256ll * j + 128;
  const long long E0 = (T.X2 - T.X1) * (Py - T.Y1) - (T.Y2 - T.Y1) * (Px - T.X1);
  const long long E1 = (T.X0 - T.X2) * (Py - T.Y2) - (T.Y0 - T.Y2) * (Px - T.X2);
  const long long E2 = (T.X1 - T.X0) * (Py - T.Y0) - (T.Y1 - T.Y0) * (Px - T.X0);
  const double A = (double)T.A;
  b0 = (double)E0 / A;
  b1 = (double)E1 / A;
  b2 = (double)E2 / A;
  return inside(E0, T.X2 - T.X1, T.Y2 - T.Y1) && inside(E1, T.X0 - T.X2, T.Y0 - T.Y2) && inside(E2, T.X1 - T.X0, T.Y1 - T.Y0);
}

__device__ __forceinline__ bool depth_key(double z, long long draw, unsigned long long& key) {
  long long d = (long long)rint(z * (double)RS_DMAX);
  if (d < 0) d = 0;
  key = ((unsigned long long)d << 32) | (unsigned long long)draw;
  return d < RS_DMAX;
}

// Calls f(tile index) for every tile a primitive reaches; returns false for a dropped primitive.
template <class F>
__device__ __forceinline__ bool for_tiles(const HgsRasterModel& m, long long p, const unsigned* __restrict__ idx,
                                          const VOut* __restrict__ vo, int W, int H, int TX, F f) {
  const unsigned* ix = idx + m.idx_offset + (size_t)m.kind * p;
  if (m.kind == 2) {
    const VOut a = vo[ix[0]], b = vo[ix[1]];
    if (a.X == INT_MIN || b.X == INT_MIN) return false;
    Line L;
    if (!line_setup(a, b, W, H, L)) return true;
    const int lo = (m.width - 1) / 2;
    for (long long tm = L.k0 >> 5; tm <= (L.k1 >> 5); tm++) {
      const long long ka = max(L.k0, tm * RS_TILE), kb = min(L.k1, tm * RS_TILE + RS_TILE - 1);
      const long long ma = fdiv(line_minor(L, 256 * ka + 128), 256) - lo, mb = fdiv(line_minor(L, 256 * kb + 128), 256) - lo;
      const long long mlo = max(min(ma, mb), 0ll), mhi = min(max(ma, mb) + m.width - 1, (long long)L.Wv - 1);
      for (long long tn = (mlo >> 5); mlo <= mhi && tn <= (mhi >> 5); tn++)
        f(L.xmaj ? (int)(tn * TX + tm) : (int)(tm * TX + tn));
    }
    return true;
  }
  const VOut a = vo[ix[0]], b = vo[ix[1]], c = vo[ix[2]];
  if (a.X == INT_MIN || b.X == INT_MIN || c.X == INT_MIN) return false;
  Tri T;
  if (!tri_setup(a, b, c, W, H, T)) return true;
  for (int ty = T.j0 >> 5; ty <= (T.j1 >> 5); ty++)
    for (int tx = T.i0 >> 5; tx <= (T.i1 >> 5); tx++) f(ty * TX + tx);
  return true;
}

__global__ __launch_bounds__(RS_BLOCK) void raster_count_kernel(int W, int H, int TX, int T, int n_models,
                                                                const HgsRasterModel* __restrict__ models, long long n_prims,
                                                                const unsigned* __restrict__ idx, int NV, const VOut* __restrict__ vout,
                                                                int* __restrict__ counts, unsigned long long* __restrict__ dropped) {
  const long long d = (long long)blockIdx.x * RS_BLOCK + threadIdx.x;
  const int v = blockIdx.y;
  if (d >= n_prims) return;
  const int mi = find_model(models, n_models, d);
  const HgsRasterModel m = models[mi];
  int* cnt = counts + (size_t)v * T;
  if (!for_tiles(m, d - m.draw_base, idx, vout + (size_t)v * NV, W, H, TX, [&](int t) { atomicAdd(cnt + t, 1); }))
    atomicAdd(dropped, 1ull);
}

__global__ __launch_bounds__(RS_BLOCK) void raster_fill_kernel(int W, int H, int TX, int T, int n_models,
                                                               const HgsRasterModel* __restrict__ models, long long n_prims,
                                                               const unsigned* __restrict__ idx, int NV, const VOut* __restrict__ vout,
                                                               const int* __restrict__ counts, const long long* __restrict__ offsets,
                                                               int* __restrict__ cursor, unsigned* __restrict__ list) {
  const long long d = (long long)blockIdx.x * RS_BLOCK + threadIdx.x;
  const int v = blockIdx.y;
  if (d >= n_prims) return;
  const int mi = find_model(models, n_models, d);
  const HgsRasterModel m = models[mi];
  const size_t vt = (size_t)v * T;
  for_tiles(m, d - m.draw_base, idx, vout + (size_t)v * NV, W, H, TX, [&](int t) {
    const int pos = atomicAdd(cursor + vt + t, 1);
    if (pos < counts[vt + t]) list[offsets[vt + t] + pos] = (unsigned)d;
  });
}

struct Light {
  double L[3], amb[3], dif[3];
  unsigned char bg[3];
};

__device__ __forceinline__ unsigned char unorm8(double v) {
  v = v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);
  return (unsigned char)floor(v * 255.0 + 0.5);
}

__global__ __launch_bounds__(RS_BLOCK) void raster_resolve_kernel(int W, int H, int TX, int T, int n_models,
                                                                  const HgsRasterModel* __restrict__ models,
                                                                  const unsigned* __restrict__ idx, int NV, const VOut* __restrict__ vout,
                                                                  const double* __restrict__ pw, const double* __restrict__ nw,
                                                                  const double* __restrict__ col, Light lt,
                                                                  const int* __restrict__ counts, const long long* __restrict__ offsets,
                                                                  const unsigned* __restrict__ list, uint8_t* __restrict__ rgb,
                                                                  uint8_t* __restrict__ gray) {
  __shared__ unsigned long long keys[RS_TILE * RS_TILE];
  __shared__ HgsRasterModel tab[HGS_RASTER_MAX_MODELS];
  const int t = blockIdx.x, v = blockIdx.y;
  const int tx = t % TX, ty = t / TX;
  const int ti0 = tx * RS_TILE, tj0 = ty * RS_TILE;
  const int ti1 = min(ti0 + RS_TILE, W) - 1, tj1 = min(tj0 + RS_TILE, H) - 1;
  for (int k = threadIdx.x; k < RS_TILE * RS_TILE; k += RS_BLOCK) keys[k] = RS_NONE;
  for (int k = threadIdx.x; k < n_models; k += RS_BLOCK) tab[k] = models[k];
  __syncthreads();
  const VOut* vo = vout + (size_t)v * NV;
  const size_t vt = (size_t)v * T + t;
  const int n = counts[vt];
  const unsigned* lst = list + offsets[vt];
  for (int e = threadIdx.x; e < n; e += RS_BLOCK) {
    const long long d = lst[e];
    const HgsRasterModel& m = tab[find_model(tab, n_models, d)];
    const unsigned* ix = idx + m.idx_offset + (size_t)m.kind * (d - m.draw_base);
    if (m.kind == 2) {
      const VOut a = vo[ix[0]], b = vo[ix[1]];
      Line L;
      if (!line_setup(a, b, W, H, L)) continue;
      const int u0 = L.xmaj ? ti0 : tj0, u1 = L.xmaj ? ti1 : tj1, w0 = L.xmaj ? tj0 : ti0, w1 = L.xmaj ? tj1 : ti1;
      const long long ka = max(L.k0, (long long)u0), kb = min(L.k1, (long long)u1);
      for (long long k = ka; k <= kb; k++) {
        const long long Cu = 256 * k + 128;
        const double tt = line_t(L, Cu);
        const double z = (1.0 - tt) * a.z + tt * b.z;
        unsigned long long key;
        if (!depth_key(z, d, key)) continue;
        const long long m0 = fdiv(line_minor(L, Cu), 256) - (m.width - 1) / 2;
        const long long r0 = max(m0, (long long)w0), r1 = min(m0 + m.width - 1, (long long)w1);
        for (long long r = r0; r <= r1; r++) {
          const int li = L.xmaj ? (int)(k - ti0) : (int)(r - ti0);
          const int lj = L.xmaj ? (int)(r - tj0) : (int)(k - tj0);
          atomicMin(&keys[lj * RS_TILE + li], key);
        }
      }
    } else {
      const VOut a = vo[ix[0]], b = vo[ix[1]], c = vo[ix[2]];
      Tri Tr;
      if (!tri_setup(a, b, c, W, H, Tr)) continue;
      const int i0 = max(Tr.i0, ti0), i1 = min(Tr.i1, ti1), j0 = max(Tr.j0, tj0), j1 = min(Tr.j1, tj1);
      for (int j = j0; j <= j1; j++)
        for (int i = i0; i <= i1; i++) {
          double b0, b1, b2;
          if (!tri_bary(Tr, i, j, b0, b1, b2)) continue;
          const double z = (b0 * a.z + b1 * b.z) + b2 * c.z;
          unsigned long long key;
          if (depth_key(z, d, key)) atomicMin(&keys[(j - tj0) * RS_TILE + (i - ti0)], key);
        }
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < RS_TILE * RS_TILE; k += RS_BLOCK) {
    const int i = ti0 + (k % RS_TILE), j = tj0 + (k / RS_TILE);
    if (i > ti1 || j > tj1) continue;
    const unsigned long long key = keys[k];
    unsigned char out[3] = {lt.bg[0], lt.bg[1], lt.bg[2]};
    if (key != RS_NONE) {
      const long long d = (long long)(key & 0xFFFFFFFFull);
      const HgsRasterModel& m = tab[find_model(tab, n_models, d)];
      const unsigned* ix = idx + m.idx_offset + (size_t)m.kind * (d - m.draw_base);
      double q[3];
      unsigned vid[3];
      int nv;
      if (m.kind == 2) {
        const VOut a = vo[ix[0]], b = vo[ix[1]];
        Line L;
        line_setup(a, b, W, H, L);
        const double tt = line_t(L, 256ll * (L.xmaj ? i : j) + 128);
        q[0] = (1.0 - tt) / a.w;
        q[1] = tt / b.w;
        vid[0] = ix[0]; vid[1] = ix[1];
        nv = 2;
      } else {
        const VOut a = vo[ix[0]], b = vo[ix[1]], c = vo[ix[2]];
        Tri Tr;
        tri_setup(a, b, c, W, H, Tr);
        double b0, b1, b2;
        tri_bary(Tr, i, j, b0, b1, b2);
        q[0] = b0 * (1.0 / a.w);
        q[1] = b1 * (1.0 / b.w);
        q[2] = b2 * (1.0 / c.w);
        vid[0] = ix[0]; vid[1] = ix[1]; vid[2] = ix[2];
        nv = 3;
      }
      const double den = nv == 2 ? q[0] + q[1] : (q[0] + q[1]) + q[2];
      // attr = ((q0 a0 + q1 a1) [+ q2 a2]) / den, per component
      auto interp = [&](const double* base, int stride, int comp) {
        double s = q[0] * base[(size_t)vid[0] * stride + comp] + q[1] * base[(size_t)vid[1] * stride + comp];
        if (nv == 3) s = s + q[2] * base[(size_t)vid[2] * stride + comp];
        return s / den;
      };
      double cc[3];
      for (int ch = 0; ch < 3; ch++) cc[ch] = interp(col, 3, ch);
      if (m.lit) {
        double p[3], nr[3];
        for (int ch = 0; ch < 3; ch++) { p[ch] = interp(pw, 4, ch); nr[ch] = interp(nw, 3, ch); }
        const double nn = (nr[0] * nr[0] + nr[1] * nr[1]) + nr[2] * nr[2];
        const double dx = lt.L[0] - p[0], dy = lt.L[1] - p[1], dz = lt.L[2] - p[2];
        const double dd = (dx * dx + dy * dy) + dz * dz;
        double cs = 0.0;
        if (nn != 0.0 && dd != 0.0) {
          const double sn = sqrt(nn), sl = sqrt(dd);
          const double c0 = (nr[0] / sn) * (dx / sl) + (nr[1] / sn) * (dy / sl);
          cs = c0 + (nr[2] / sn) * (dz / sl);
          cs = cs > 0.0 ? cs : 0.0;                 // (max(cos, 0); a NaN cos would give 0 here as in numpy's where)
        }
        for (int ch = 0; ch < 3; ch++) {
          const double light = m.ka * lt.amb[ch] + (m.kd * cs) * lt.dif[ch];
          out[ch] = unorm8(light * cc[ch]);
        }
      } else {
        for (int ch = 0; ch < 3; ch++) out[ch] = unorm8(cc[ch]);
      }
    }
    const size_t px = ((size_t)v * H + (size_t)(H - 1 - j)) * W + i;
    rgb[3 * px] = out[0];
    rgb[3 * px + 1] = out[1];
    rgb[3 * px + 2] = out[2];
    if (gray) gray[px] = (uint8_t)((4899 * out[0] + 9617 * out[1] + 1868 * out[2] + 8192) >> 14);
  }
}

bool raster_sizes_ok(const char* who, int V, int W, int H, int n_models) {
  if (V < 1 || V > 65535 || W < 1 || H < 1 || W > 16384 || H > 16384 || n_models < 1 || n_models > HGS_RASTER_MAX_MODELS) {
    hgs_set_error("%s: bad sizes V=%d W=%d H=%d models=%d (1 <= V <= 65535, 1 <= W, H <= 16384, 1 <= models <= %d)", who, V, W, H,
                  n_models, HGS_RASTER_MAX_MODELS);
    return false;
  }
  return true;
}

int tiles_x(int W) { return (W + RS_TILE - 1) / RS_TILE; }
int tiles_y(int H) { return (H + RS_TILE - 1) / RS_TILE; }

}  // namespace

extern "C" size_t hgs_raster_model_bytes(void) { return sizeof(HgsRasterModel); }
extern "C" size_t hgs_raster_vertex_bytes(void) { return sizeof(VOut); }
extern "C" int hgs_raster_tiles(int W, int H) { return W < 1 || H < 1 ? 0 : tiles_x(W) * tiles_y(H); }

extern "C" int hgs_raster_vertices(void* stream, int V, int NV, int W, int H, const double* pw, const double* views, const double* projs,
                                   void* vout) {
  if (!raster_sizes_ok("hgs_raster_vertices", V, W, H, 1)) return 1;
  if (NV < 0 || (NV > 0 && (!pw || !vout)) || !views || !projs) { hgs_set_error("hgs_raster_vertices: null argument or NV < 0"); return 1; }
  if (NV == 0) return 0;
  hipLaunchKernelGGL(raster_vertex_kernel, dim3((NV + RS_BLOCK - 1) / RS_BLOCK, V), dim3(RS_BLOCK), 0, (hipStream_t)stream, NV, W, H,
                     pw, views, projs, (VOut*)vout);
  HGS_CHECK_LAUNCH();
  return 0;
}

extern "C" int hgs_raster_count(void* stream, int V, int W, int H, int n_models, const HgsRasterModel* models, long long n_prims,
                                const unsigned* idx, int NV, const void* vout, int* tile_counts, unsigned long long* dropped) {
  if (!raster_sizes_ok("hgs_raster_count", V, W, H, n_models)) return 1;
  if (n_prims < 0 || n_prims > UINT_MAX || !models || !tile_counts || !dropped || (n_prims > 0 && (!idx || !vout))) {
    hgs_set_error("hgs_raster_count: null argument or bad primitive count %lld", n_prims);
    return 1;
  }
  if (n_prims == 0) return 0;
  const int TX = tiles_x(W), T = TX * tiles_y(H);
  hipLaunchKernelGGL(raster_count_kernel, dim3((unsigned)((n_prims + RS_BLOCK - 1) / RS_BLOCK), V), dim3(RS_BLOCK), 0,
                     (hipStream_t)stream, W, H, TX, T, n_models, models, n_prims, idx, NV, (const VOut*)vout, tile_counts, dropped);
  HGS_CHECK_LAUNCH();
  return 0;
}

extern "C" int hgs_raster_fill(void* stream, int V, int W, int H, int n_models, const HgsRasterModel* models, long long n_prims,
                               const unsigned* idx, int NV, const void* vout, const int* tile_counts, const long long* tile_offsets,
                               int* tile_cursor, unsigned* list) {
  if (!raster_sizes_ok("hgs_raster_fill", V, W, H, n_models)) return 1;
  if (n_prims < 0 || n_prims > UINT_MAX || !models || !tile_counts || !tile_offsets || !tile_cursor ||
      (n_prims > 0 && (!idx || !vout))) {
    hgs_set_error("hgs_raster_fill: null argument or bad primitive count %lld", n_prims);
    return 1;
  }
  if (n_prims == 0) return 0;
  if (!list) { hgs_set_error("hgs_raster_fill: null list"); return 1; }
  const int TX = tiles_x(W), T = TX * tiles_y(H);
  hipLaunchKernelGGL(raster_fill_kernel, dim3((unsigned)((n_prims + RS_BLOCK - 1) / RS_BLOCK), V), dim3(RS_BLOCK), 0,
                     (hipStream_t)stream, W, H, TX, T, n_models, models, n_prims, idx, NV, (const VOut*)vout, tile_counts, tile_offsets,
                     tile_cursor, list);
  HGS_CHECK_LAUNCH();
  return 0;
}

extern "C" int hgs_raster_resolve(void* stream, int V, int W, int H, int n_models, const HgsRasterModel* models, const unsigned* idx,
                                  int NV, const void* vout, const double* pw, const double* nw, const double* col,
                                  const double* light_host, const unsigned char* background_host, const int* tile_counts,
                                  const long long* tile_offsets, const unsigned* list, unsigned char* rgb, unsigned char* gray) {
  if (!raster_sizes_ok("hgs_raster_resolve", V, W, H, n_models)) return 1;
  if (!models || !light_host || !background_host || !tile_counts || !tile_offsets || !rgb) {
    hgs_set_error("hgs_raster_resolve: null argument");
    return 1;
  }
  Light lt;
  for (int k = 0; k < 3; k++) {
    lt.L[k] = light_host[k];
    lt.amb[k] = light_host[3 + k];
    lt.dif[k] = light_host[6 + k];
    lt.bg[k] = background_host[k];
  }
  const int TX = tiles_x(W), T = TX * tiles_y(H);
  hipLaunchKernelGGL(raster_resolve_kernel, dim3(T, V), dim3(RS_BLOCK), 0, (hipStream_t)stream, W, H, TX, T, n_models, models, idx, NV,
                     (const VOut*)vout, pw, nw, col, lt, tile_counts, tile_offsets, list, rgb, gray);
  HGS_CHECK_LAUNCH();
  return 0;
}
