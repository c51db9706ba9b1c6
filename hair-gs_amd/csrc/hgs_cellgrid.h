// hgs_cellgrid.h -- the exact 3-nearest-neighbour search over a grid of Morton cells, once; distCUDA2 (hgs_knn.hip) and the
// magnet term's grid path (hgs_magnet.hip) instantiate it, both built with -ffp-contract=off.  A point's key is its 30-bit Morton
// code << 32 | index; sorted, the points sharing the top 3 L bits are one run of the array and fill one cube, so a table of 8^L
// cells (first / end, exact bounding box) is an octree level with disjoint boxes.  A lane seeds a radius from its +-3 neighbours
// along the curve, walks its own cell, then the cells its radius reaches, each behind simple_knn.cu's box test.
// An owner supplies a SOURCE -- load_box(box[6]) (into LDS, ends in a barrier), live(n) (how many of the n points take part),
// kGuarded -- and an ACCUMULATOR -- clear(), third(), add(d, id), Out and store(out, me) (its result), kSelf (is the point its own candidate), kGuarded.
// kGuarded is the magnet's defensive form (its count is read on the device, its points may be non-finite): a non-finite point
// gets a code behind every cell and is in none, ids and cell runs are checked against the live count.
#pragma once
#include <float.h>

#include "hgs_keysort.h"

namespace {

#define CELLGRID_NONFINITE_CODE 0x7FFFFFFFu   // "code" of a point with a non-finite coordinate: behind every 30-bit code, in no cell

// level of the grid: about 16 points per cell of a uniform cloud (clustered data fills fewer, fuller cells)
static int cellgrid_level(size_t n) {
  int L = 1;
  while (L < 7 && ((size_t)1 << (3 * (L + 1))) * 16 <= n) L++;
  return L;
}

// coordinate -> cell coordinate, saturating (NaN and negatives -> 0)
__device__ __forceinline__ uint32_t f2u_sat(float v) {
  if (!(v > 0.f)) return 0u;
  if (v >= 4294967040.f) return 0xFFFFFFFFu;
  return (uint32_t)v;
}
// the quantisation q of one axis, monotone in v.  The clamp matters for the cube range (v +- r leaves the box) and for a box that
// does not hold the point; for a point inside its own finite box it is a no-op -- v <= mx gives v - mn <= mx - mn after rounding
// (rounding is monotone), a ratio <= 1 -- and so it is with a zero extent, an infinite box or a finite box whose extent mx - mn
// overflows to +inf: the ratio is then 0 or NaN, and both quantise to 0.
__device__ __forceinline__ uint32_t cellgrid_q(float v, float mn, float mx) { return min(f2u_sat(((v - mn) / (mx - mn)) * 1023), 1023u); }

// The Morton code of a point.  GUARDED: a non-finite coordinate gives CELLGRID_NONFINITE_CODE.  Otherwise (distCUDA2, whose box
// holds the origin and folds every point with fminf / fmaxf) the formula alone decides: NaN quantises to 0, the point sits in a
// real cell and never compares closer.
template <bool GUARDED>
__device__ __forceinline__ uint32_t cellgrid_code(const float* box, float x, float y, float z) {
  if (GUARDED && !(isfinite(x) && isfinite(y) && isfinite(z))) return CELLGRID_NONFINITE_CODE;
  return prep_morton(cellgrid_q(x, box[0], box[3])) | (prep_morton(cellgrid_q(y, box[1], box[4])) << 1) |
         (prep_morton(cellgrid_q(z, box[2], box[5])) << 2);
}

// squared distance of a point to a box, exactly as distBoxPoint (simple_knn.cu:120-130)
__device__ __forceinline__ float box_point_dist2(const float* bx, float x, float y, float z) {
  float d0 = 0.f, d1 = 0.f, d2 = 0.f;
  if (x < bx[0] || x > bx[3]) d0 = fminf(fabsf(x - bx[0]), fabsf(x - bx[3]));
  if (y < bx[1] || y > bx[4]) d1 = fminf(fabsf(y - bx[1]), fabsf(y - bx[4]));
  if (z < bx[2] || z > bx[5]) d2 = fminf(fabsf(z - bx[2]), fabsf(z - bx[5]));
  return d0 * d0 + d1 * d1 + d2 * d2;
}
__device__ __forceinline__ float point_dist2(const float4& a, const float4& q) {
  const float dx = a.x - q.x, dy = a.y - q.y, dz = a.z - q.z;
  return dx * dx + dy * dy + dz * dz;      // simple_knn.cu:135-136 (the sign of a difference does not reach its square)
}

// the points of an owner: packed xyz (distCUDA2) or float4 (the magnet's compacted list)
__device__ __forceinline__ float4 cellgrid_point(const float* pts, size_t i) { return make_float4(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], 0.f); }
__device__ __forceinline__ float4 cellgrid_point(const float4* pts, size_t i) { return pts[i]; }

// ---- the three best of a walk over 256-point tiles in ascending candidate order (hgs_knn3, the magnet's tiles): ascending by
// (distance, index), empty slots (+inf, -1).  Strict <: indices ascend along the walk, so an equal distance never displaces.
struct Best3 { float d[3]; int i[3]; };
__device__ __forceinline__ void best3_clear(Best3& b) {
  b.d[0] = b.d[1] = b.d[2] = INFINITY;
  b.i[0] = b.i[1] = b.i[2] = -1;
}
// candidate k of the tile that starts at index t0 (the index is formed only where it is stored: not on the path of a candidate
// that is no better)
__device__ __forceinline__ void best3_push(Best3& b, float d, int t0, int k) {
  if (d < b.d[2]) {
    if (d < b.d[1]) {
      b.d[2] = b.d[1]; b.i[2] = b.i[1];
      if (d < b.d[0]) { b.d[1] = b.d[0]; b.i[1] = b.i[0]; b.d[0] = d; b.i[0] = t0 + k; }
      else { b.d[1] = d; b.i[1] = t0 + k; }
    } else { b.d[2] = d; b.i[2] = t0 + k; }
  }
}

// ---- the cell table: per cell of level L (code >> (30 - 3 L)) [first, end) in the sorted array and the points' bounding box.
// Floats are kept as order-preserving integers so that min / max are integer atomics (exact, order-independent).
__device__ __forceinline__ int fkey(float v) { const int b = __float_as_int(v); return b >= 0 ? b : b ^ 0x7FFFFFFF; }   // monotone: a < b <=> fkey(a) < fkey(b)
__device__ __forceinline__ float funkey(int k) { return __int_as_float(k >= 0 ? k : k ^ 0x7FFFFFFF); }

template <class Source, class Point>
__global__ __launch_bounds__(256) void cellgrid_keys_kernel(Source src, int n, int Npad, const Point* __restrict__ pts,
                                                            uint64_t* __restrict__ keys) {
  __shared__ float box[6];
  src.load_box(box);
  const int nv = src.live(n);
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= Npad) return;
  if (i >= nv) { keys[i] = ~0ull; return; }
  const float4 p = cellgrid_point(pts, (size_t)i);
  keys[i] = ((uint64_t)cellgrid_code<Source::kGuarded>(box, p.x, p.y, p.z) << 32) | (uint32_t)i;
}

// the points in sorted order, w = the point's index
template <class Source, class Point>
__global__ __launch_bounds__(256) void cellgrid_gather_kernel(Source src, int n, const Point* __restrict__ pts,
                                                              const uint64_t* __restrict__ keys, float4* __restrict__ sorted) {
  const int nv = src.live(n);
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nv) return;
  const uint32_t id = (uint32_t)keys[i];
  float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
  if (!Source::kGuarded || id < (uint32_t)nv) p = cellgrid_point(pts, (size_t)id);
  p.w = __uint_as_float(id);
  sorted[i] = p;
}

__global__ __launch_bounds__(256) void cells_clear_kernel(uint32_t n_cells, uint32_t* __restrict__ cells) {
  const uint32_t c = blockIdx.x * 256 + threadIdx.x;
  if (c >= n_cells) return;
  uint4* t = (uint4*)(cells + 8 * (size_t)c);
  t[0] = make_uint4(0u, 0u, (uint32_t)0x7FFFFFFF, (uint32_t)0x7FFFFFFF);              // first, end, min x, min y
  t[1] = make_uint4((uint32_t)0x7FFFFFFF, 0x80000000u, 0x80000000u, 0x80000000u);     // min z, max x, max y, max z
}

template <class Source>
__global__ __launch_bounds__(256) void cellgrid_mark_kernel(Source src, int n, int shift, const uint64_t* __restrict__ keys,
                                                            const float4* __restrict__ sorted, uint32_t* __restrict__ cells) {
  const int nv = src.live(n);
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nv) return;
  const uint32_t code = (uint32_t)(keys[i] >> 32);
  if (Source::kGuarded && code >= 0x40000000u) return;
  const uint32_t c = code >> shift;
  const bool first = i == 0 || ((uint32_t)(keys[i - 1] >> 32) >> shift) != c;
  bool last = i == nv - 1;
  if (!last) {
    const uint32_t nc = (uint32_t)(keys[i + 1] >> 32);
    last = (Source::kGuarded && nc >= 0x40000000u) || (nc >> shift) != c;
  }
  uint32_t* t = cells + 8 * (size_t)c;
  if (first) t[0] = (uint32_t)i;
  if (last) t[1] = (uint32_t)i + 1u;
  const float4 p = sorted[i];
  atomicMin((int*)&t[2], fkey(p.x)); atomicMin((int*)&t[3], fkey(p.y)); atomicMin((int*)&t[4], fkey(p.z));
  atomicMax((int*)&t[5], fkey(p.x)); atomicMax((int*)&t[6], fkey(p.y)); atomicMax((int*)&t[7], fkey(p.z));
}

// The search: one lane per point of the sorted array.  The body sits in the kernel itself -- no aggregate crosses a call, so the
// accumulator stays in registers.  A guarded accumulator's point whose code is behind every cell compares closer to nothing: its
// empty result is stored.
template <class Source, class Acc>
__global__ __launch_bounds__(256) void cellgrid_search_kernel(int n, int L, Source src, const float4* __restrict__ sorted,
                                                              const uint64_t* __restrict__ keys, const uint32_t* __restrict__ cells,
                                                              typename Acc::Out* __restrict__ out) {
  __shared__ float box[6];
  src.load_box(box);
  const int nv = src.live(n);
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= nv) return;
  const float4 me = sorted[idx];
  if (Acc::kGuarded && __float_as_uint(me.w) >= (uint32_t)nv) return;
  auto code = [&]() { return (uint32_t)(keys[idx] >> 32); };           // this lane's Morton code
  Acc best;
  best.clear();
  if (Acc::kGuarded && code() >= 0x40000000u) { best.store(out, me); return; }
  {
    // a first radius from the neighbours along the curve
    const int lo = max(0, idx - 3), hi = min(nv - 1, idx + 3);
    for (int i = lo; i <= hi; i++) {
      if (!Acc::kSelf && i == idx) continue;
      const float4 q = sorted[i];
      best.add(point_dist2(me, q), __float_as_uint(q.w));
    }
  }
  const float reject = best.third();           // simple_knn.cu:163-165: a box farther than this holds none of the three nearest
  best.clear();
  const int shift = 30 - 3 * L;
  auto walk_cell = [&](uint32_t c) {
    const uint4 h0 = *(const uint4*)(cells + 8 * (size_t)c), h1 = *(const uint4*)(cells + 8 * (size_t)c + 4);
    if (Acc::kGuarded ? h0.x >= h0.y || h0.y > (uint32_t)nv : h0.x == h0.y) return;   // empty (guarded: or no run of the live points)
    const float bx[6] = {funkey((int)h0.z), funkey((int)h0.w), funkey((int)h1.x), funkey((int)h1.y), funkey((int)h1.z), funkey((int)h1.w)};
    const float dist = box_point_dist2(bx, me.x, me.y, me.z);
    if (dist > reject || dist > best.third()) return;                   // simple_knn.cu:173-175 (an equal distance is walked)
    for (uint32_t i = h0.x; i < h0.y; i++) {
      const float4 q = sorted[i];
      if (Acc::kSelf || (int)i != idx) best.add(point_dist2(me, q), __float_as_uint(q.w));
    }
  };
  // the own cell first: after it the third-best distance is (nearly always) the true one
  const uint32_t own = code() >> shift;
  walk_cell(own);
  // the cube of cells the radius reaches.  The quantisation q is monotone, so every point within r of this one along an axis has
  // its cell coordinate between q(x - r) and q(x + r).  The margin: sqrtf(r2) can round below the true distance, and x - r can
  // then round to the wrong side of a cell boundary (tests/knn_cases.py margin_cloud).
  const float r2 = fminf(reject, best.third());
  const float r = sqrtf(r2) * 1.000001f;
  const int cshift = 10 - L;
  int lo[3], hi[3];
  const float pc[3] = {me.x, me.y, me.z};
#pragma unroll
  for (int k = 0; k < 3; k++) {
    lo[k] = (int)(cellgrid_q(pc[k] - r, box[k], box[3 + k]) >> cshift);
    hi[k] = (int)(cellgrid_q(pc[k] + r, box[k], box[3 + k]) >> cshift);
    if (!(r < FLT_MAX)) { lo[k] = 0; hi[k] = (1 << L) - 1; }            // (fewer than three candidates: no radius yet)
  }
  for (int cz = lo[2]; cz <= hi[2]; cz++)
    for (int cy = lo[1]; cy <= hi[1]; cy++)
      for (int cx = lo[0]; cx <= hi[0]; cx++) {
        const uint32_t c = (prep_morton((uint32_t)cx << cshift) | (prep_morton((uint32_t)cy << cshift) << 1) |
                            (prep_morton((uint32_t)cz << cshift) << 2)) >> shift;
        if (c != own) walk_cell(c);
      }
  best.store(out, me);
}

}  // namespace
