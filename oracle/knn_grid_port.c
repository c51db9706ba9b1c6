/*
 * knn_grid_port.c -- CPU port of distCUDA2's search over a grid of Morton cells (hair-gs_amd/csrc/hgs_knn.hip: minmax_kernel,
 * KnnSource, KnnBest; csrc/hgs_cellgrid.h: cellgrid_level, cellgrid_keys_kernel, cellgrid_gather_kernel, cellgrid_mark_kernel,
 * cellgrid_search_kernel), statement by statement in the same float32 arithmetic (built with -ffp-contract=off), one loop
 * iteration per lane.
 *
 * TEST INFRASTRUCTURE ONLY.  It exists to show, without a GPU, which input catches which decision of the search:
 * `flags` switches single decisions off (tests/test_knn_hard_cpu.py).  As written (flags = 0) it equals the brute force bit
 * for bit.  A lane whose cube walk leaves the grid -- a cell index outside the table, or more steps than the grid has cells (cell
 * coordinates beyond 2^L wrap in the bit spreading, so the walk would go on for up to 2^31 steps) -- stops there and is counted
 * in *out_of_grid: on the GPU that is an out-of-bounds read or a lane that does not return.
 */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define GRID_NO_MARGIN 1    /* r = sqrtf(r2) without the 1.000001f */
#define GRID_NO_OWN_GUARD 2 /* the cube walk does not skip the lane's own cell */
#define GRID_NO_CLAMP 4     /* no min(..., 1023u) on the cube range */

static uint32_t prep_morton(uint32_t x) {
  x = (x | (x << 16)) & 0x030000FF;
  x = (x | (x << 8)) & 0x0300F00F;
  x = (x | (x << 4)) & 0x030C30C3;
  x = (x | (x << 2)) & 0x09249249;
  return x;
}
static uint32_t f2u_sat(float v) {
  if (!(v > 0.f)) return 0u;
  if (v >= 4294967040.f) return 0xFFFFFFFFu;
  return (uint32_t)v;
}
static float box_point_dist2(const float* bx, float x, float y, float z) {
  float d0 = 0.f, d1 = 0.f, d2 = 0.f;
  if (x < bx[0] || x > bx[3]) d0 = fminf(fabsf(x - bx[0]), fabsf(x - bx[3]));
  if (y < bx[1] || y > bx[4]) d1 = fminf(fabsf(y - bx[1]), fabsf(y - bx[4]));
  if (z < bx[2] || z > bx[5]) d2 = fminf(fabsf(z - bx[2]), fabsf(z - bx[5]));
  return d0 * d0 + d1 * d1 + d2 * d2;
}
static int fkey(float v) { int b; memcpy(&b, &v, 4); return b >= 0 ? b : b ^ 0x7FFFFFFF; }
static float funkey(int k) { int b = k >= 0 ? k : k ^ 0x7FFFFFFF; float v; memcpy(&v, &b, 4); return v; }
static void kbest3(float px, float py, float pz, float qx, float qy, float qz, float* knn) {
  const float dx = qx - px, dy = qy - py, dz = qz - pz;
  float dist = dx * dx + dy * dy + dz * dz;
  for (int j = 0; j < 3; j++) {
    const float t = knn[j];
    const int sw = t > dist;
    knn[j] = sw ? dist : t;
    dist = sw ? t : dist;
  }
}
static int cmp_key(const void* a, const void* b) {
  const uint64_t x = *(const uint64_t*)a, y = *(const uint64_t*)b;
  return x < y ? -1 : x > y;
}
static int cellgrid_level(size_t P) {
  int L = 1;
  while (L < 7 && ((size_t)1 << (3 * (L + 1))) * 16 <= P) L++;
  return L;
}
typedef struct { float x, y, z; uint32_t id; } Sorted;
typedef struct { const Sorted* sorted; const uint32_t* cells; uint32_t n_cells; int idx; float reject; float best[3]; int fault; } Lane;

static void walk_cell(Lane* l, uint32_t c) {
  if (c >= l->n_cells) { l->fault = 1; return; }
  const uint32_t* h = l->cells + 8 * (size_t)c;
  if (h[0] == h[1]) return;
  float bx[6];
  for (int k = 0; k < 6; k++) bx[k] = funkey((int)h[2 + k]);
  const Sorted me = l->sorted[l->idx];
  const float dist = box_point_dist2(bx, me.x, me.y, me.z);
  if (dist > l->reject || dist > l->best[2]) return;
  for (uint32_t i = h[0]; i < h[1]; i++) {
    const Sorted q = l->sorted[i];
    if ((int)i != l->idx) kbest3(me.x, me.y, me.z, q.x, q.y, q.z, l->best);
  }
}

void hgs_oracle_dist2_grid(int P, const float* pts, float* out, int flags, int64_t* out_of_grid) {
  *out_of_grid = 0;
  if (P <= 0) return;
  float smm[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int i = 0; i < P; i++)
    for (int k = 0; k < 3; k++) {
      smm[k] = fminf(smm[k], pts[3 * (size_t)i + k]);
      smm[3 + k] = fmaxf(smm[3 + k], pts[3 * (size_t)i + k]);
    }
  uint64_t* keys = (uint64_t*)malloc(8 * (size_t)P);
  for (int i = 0; i < P; i++) {
    const float x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
    const uint32_t cx = prep_morton(f2u_sat(((x - smm[0]) / (smm[3] - smm[0])) * 1023));
    const uint32_t cy = prep_morton(f2u_sat(((y - smm[1]) / (smm[4] - smm[1])) * 1023));
    const uint32_t cz = prep_morton(f2u_sat(((z - smm[2]) / (smm[5] - smm[2])) * 1023));
    keys[i] = ((uint64_t)(cx | (cy << 1) | (cz << 2)) << 32) | (uint32_t)i;
  }
  qsort(keys, (size_t)P, 8, cmp_key);              /* the keys are unique: any sort gives the bitonic network's order */
  Sorted* sorted = (Sorted*)malloc(sizeof(Sorted) * (size_t)P);
  for (int i = 0; i < P; i++) {
    const uint32_t id = (uint32_t)keys[i];
    const Sorted s = {pts[3 * (size_t)id], pts[3 * (size_t)id + 1], pts[3 * (size_t)id + 2], id};
    sorted[i] = s;
  }
  const int L = cellgrid_level((size_t)P), shift = 30 - 3 * L, cshift = 10 - L;
  const uint32_t n_cells = 1u << (3 * L);
  uint32_t* cells = (uint32_t*)malloc(32 * (size_t)n_cells);
  for (uint32_t c = 0; c < n_cells; c++) {
    uint32_t* t = cells + 8 * (size_t)c;
    t[0] = t[1] = 0u;
    t[2] = t[3] = t[4] = 0x7FFFFFFFu;
    t[5] = t[6] = t[7] = 0x80000000u;
  }
  for (int i = 0; i < P; i++) {
    const uint32_t c = (uint32_t)(keys[i] >> 32) >> shift;
    int* t = (int*)(cells + 8 * (size_t)c);
    if (i == 0 || ((uint32_t)(keys[i - 1] >> 32) >> shift) != c) t[0] = i;
    if (i == P - 1 || ((uint32_t)(keys[i + 1] >> 32) >> shift) != c) t[1] = i + 1;
    const float v[3] = {sorted[i].x, sorted[i].y, sorted[i].z};
    for (int k = 0; k < 3; k++) {
      if (fkey(v[k]) < t[2 + k]) t[2 + k] = fkey(v[k]);
      if (fkey(v[k]) > t[5 + k]) t[5 + k] = fkey(v[k]);
    }
  }
  for (int idx = 0; idx < P; idx++) {
    const Sorted me = sorted[idx];
    Lane l = {sorted, cells, n_cells, idx, 0.f, {FLT_MAX, FLT_MAX, FLT_MAX}, 0};
    const int wlo = idx - 3 > 0 ? idx - 3 : 0, whi = idx + 3 < P - 1 ? idx + 3 : P - 1;
    for (int i = wlo; i <= whi; i++) {
      if (i == idx) continue;
      kbest3(me.x, me.y, me.z, sorted[i].x, sorted[i].y, sorted[i].z, l.best);
    }
    l.reject = l.best[2];
    l.best[0] = l.best[1] = l.best[2] = FLT_MAX;
    const uint32_t own = (uint32_t)(keys[idx] >> 32) >> shift;
    walk_cell(&l, own);
    const float r2 = fminf(l.reject, l.best[2]);
    const float r = (flags & GRID_NO_MARGIN) ? sqrtf(r2) : sqrtf(r2) * 1.000001f;
    int64_t lo[3], hi[3];
    const float pc[3] = {me.x, me.y, me.z};
    for (int k = 0; k < 3; k++) {
      const float mn = smm[k], mx = smm[3 + k];
      uint32_t a = f2u_sat(((pc[k] - r - mn) / (mx - mn)) * 1023), b = f2u_sat(((pc[k] + r - mn) / (mx - mn)) * 1023);
      if (!(flags & GRID_NO_CLAMP)) { a = a < 1023u ? a : 1023u; b = b < 1023u ? b : 1023u; }
      lo[k] = (int)(a >> cshift);
      hi[k] = (int)(b >> cshift);
      if (!(r < FLT_MAX)) { lo[k] = 0; hi[k] = (1 << L) - 1; }
    }
    uint32_t steps = 0;
    for (int64_t cz = lo[2]; cz <= hi[2] && !l.fault; cz++)
      for (int64_t cy = lo[1]; cy <= hi[1] && !l.fault; cy++)
        for (int64_t cx = lo[0]; cx <= hi[0] && !l.fault; cx++) {
          const uint32_t c = (prep_morton((uint32_t)cx << cshift) | (prep_morton((uint32_t)cy << cshift) << 1) |
                              (prep_morton((uint32_t)cz << cshift) << 2)) >> shift;
          if (++steps > n_cells) { l.fault = 1; break; }
          if ((flags & GRID_NO_OWN_GUARD) || c != own) walk_cell(&l, c);
        }
    *out_of_grid += l.fault;
    out[me.id] = (l.best[0] + l.best[1] + l.best[2]) / 3.0f;
  }
  free(cells); free(sorted); free(keys);
}
