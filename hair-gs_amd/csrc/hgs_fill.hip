// hgs_fill.hip -- the direction volume filled between the scalp and the visible hair (utils/field_fill.py states the contract, its
// numpy path and the loop restatement in tests/fill_reference.py state the same thing; trace_strands.py --fill is the scene driver):
// hgs_field_fill.  gfx950, wave64.  Built with -ffp-contract=off: all arithmetic is float64, rounded once per operation, in the order
// written.
//
// field_fill_kernel: one Jacobi sweep.  One lane per FREE node, 256 per block, over the compact ascending list free_index: FIXED and
//   OUT nodes cost nothing, both buffers hold them already.  A lane reads the kind byte of its six face neighbours (-x, +x, -y, +y,
//   -z, +z; a neighbour counts iff it is on the grid and not OUT), then per tensor plane the six neighbour values of the source
//   buffer, adds them in that order to s = 0.0 -- a neighbour that does not count adds +0.0, and the addition is performed -- and
//   writes s / (double)c to the destination buffer (c == 0: the old value).  The 36 loads are unconditional (a neighbour that does
//   not count reads the lane's own node), so they are all in flight at once; consecutive lanes are mostly x-neighbours, so the
//   plane reads coalesce and the +-x reads hit the same lines.  An index outside the grid writes nothing.
// hgs_field_fill enqueues one plain launch per sweep, alternating source and destination: no cooperative launch, no grid-wide
//   barrier, no persistent workgroups.
#include "hgs_common.h"

#define HGS_FILL_MAX_NODES (1ll << 26)
#define HGS_FILL_MAX_SWEEPS 65536

namespace {

#define FILL_BLOCK 256
enum { KIND_OUT = 0, KIND_FREE = 1, KIND_FIXED = 2 };

__global__ __launch_bounds__(FILL_BLOCK) void field_fill_kernel(int F, const int* __restrict__ free_index,
                                                                const unsigned char* __restrict__ kind, int nx, int ny, int nz,
                                                                const double* __restrict__ src, double* __restrict__ dst) {
  const int j = blockIdx.x * FILL_BLOCK + threadIdx.x;
  if (j >= F) return;
  const int nodes = nx * ny * nz;                                                 // at most 2^26
  const int i = free_index[j];
  if (i < 0 || i >= nodes) return;
  const int ix = i % nx, rest = i / nx;
  const int iy = rest % ny, iz = rest / ny;
  const int sy = nx, sz = nx * ny;
  // the six neighbours: where one is off the grid the lane's own node stands in for the address and is never counted
  int at[6];
  bool on[6];
  on[0] = ix > 0;      at[0] = on[0] ? i - 1 : i;
  on[1] = ix < nx - 1; at[1] = on[1] ? i + 1 : i;
  on[2] = iy > 0;      at[2] = on[2] ? i - sy : i;
  on[3] = iy < ny - 1; at[3] = on[3] ? i + sy : i;
  on[4] = iz > 0;      at[4] = on[4] ? i - sz : i;
  on[5] = iz < nz - 1; at[5] = on[5] ? i + sz : i;
  int c = 0;
#pragma unroll
  for (int n = 0; n < 6; n++) {
    on[n] = on[n] && kind[at[n]] != KIND_OUT;
    c += on[n] ? 1 : 0;
  }
  if (c == 0) {
#pragma unroll
    for (int p = 0; p < 6; p++) dst[(size_t)p * nodes + i] = src[(size_t)p * nodes + i];
    return;
  }
  const double cd = (double)c;
#pragma unroll
  for (int p = 0; p < 6; p++) {
    const double* __restrict__ plane = src + (size_t)p * nodes;
    double v[6];
#pragma unroll
    for (int n = 0; n < 6; n++) v[n] = plane[at[n]];
    double s = 0.0;
#pragma unroll
    for (int n = 0; n < 6; n++) s = s + (on[n] ? v[n] : 0.0);
    dst[(size_t)p * nodes + i] = s / cd;
  }
}

}  // namespace

extern "C" int hgs_field_fill(void* stream, int nx, int ny, int nz, const unsigned char* kind, const int* free_index, int F, double* a,
                              double* b, int sweeps) {
  if (nx < 2 || ny < 2 || nz < 2 || nx > 1024 || ny > 1024 || nz > 1024 || (long long)nx * ny * nz > HGS_FILL_MAX_NODES) {
    hgs_set_error("hgs_field_fill: a grid of %d x %d x %d nodes (2 to 1024 an axis, at most 2^26 in all)", nx, ny, nz);
    return 1;
  }
  if (F < 0 || (long long)F > (long long)nx * ny * nz) {
    hgs_set_error("hgs_field_fill: %d free nodes on a grid of %lld", F, (long long)nx * ny * nz);
    return 1;
  }
  if (sweeps < 0 || sweeps > HGS_FILL_MAX_SWEEPS) {
    hgs_set_error("hgs_field_fill: sweeps = %d (0 to %d)", sweeps, HGS_FILL_MAX_SWEEPS);
    return 1;
  }
  if (F == 0 || sweeps == 0) return 0;
  if (!kind || !free_index || !a || !b) { hgs_set_error("hgs_field_fill: kind, free_index, a and b are required"); return 1; }
  if (a == b) { hgs_set_error("hgs_field_fill: a and b are one buffer"); return 1; }
  const dim3 grid((unsigned)((F + FILL_BLOCK - 1) / FILL_BLOCK)), block(FILL_BLOCK);
  for (int k = 0; k < sweeps; k++) {
    const double* src = (k & 1) ? b : a;
    double* dst = (k & 1) ? a : b;
    hipLaunchKernelGGL(field_fill_kernel, grid, block, 0, (hipStream_t)stream, F, free_index, kind, nx, ny, nz, src, dst);
    HGS_CHECK_LAUNCH();
  }
  return 0;
}
