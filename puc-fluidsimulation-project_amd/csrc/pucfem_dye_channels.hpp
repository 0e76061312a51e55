// Dye channels (PUCFEM_F_DYES, pucfem_sl_advect_multi, include/pucfem.h): the semi-Lagrangian step of up to
// DYE_MAX nodal fields from ONE back-trace and ONE point location per row.
//
// What makes advect_semilagrange (StokesColor.py:347-389) expensive is the departure point and its triangle: the
// lattice fast path, the general search, the centroid rank count.  They depend on u and the mesh, not on the field
// that is advected: once a row's triangle is known, one more field costs three gathers, the interpolation's last
// three products and one store.  The reference starts its dye three ways (the half plane StokesColor.py:495, the
// stripe good_visualization2.py:520-524, the blob good_visualization.py:555-559); the channels carry them through
// one run instead of one run each.
//
// One pass, one lane per row, blocks over rows as k_sl's (block_rows).  The locate is sl_locate_row
// (pucfem_locate.hpp): the steps k_sl and its second pass take, in one lane.  The passes' own design claim -- the
// general locate returns the fast path's triangle -- is what makes one pass legal.  Every channel's value is sl_value on that triangle, or the row's own value when none is
// accepted: the expressions of the single-dye kernels (the library is built with -ffp-contract=off), so channel k
// holds the bits c would hold in a run started from channel k's values (tests/test_gpu_dye_channels.py).
//
// Layout: channel-major, channel k the plain length-ld vector cin + k * ld, so sl_value, the samplers and k_mix2
// take a channel as they take c.  The launch reads one set of channels and writes another: rows of other blocks
// still gather from channel k's old values while this row's new value is stored, so no buffer of the input set
// can be an output of the same launch (a spare vector rotating through K + 1 would be written while it is read).
#pragma once
#include "pucfem_kernels_impl.hpp"

namespace pucfem {
namespace dev {

constexpr int DYE_MAX = 16;  // PUCFEM_MAX_DYES

// rows [row0, row0 + n): cout[k * ld + g] for every channel k < nch; notfound (n, or null): 0 found, 1 kept its own
// value (2: found by the general locate, under the locator's probe bit 1, as k_sl_slow marks it); nfpart[block]: the
// block's not-found rows -- the same for every channel, summed by the host in block order
template <class LOC>
__global__ __launch_bounds__(BS) void k_sl_multi(MeshDev M, LOC L, GridDev G, int64_t row0, int64_t n,
                                                 const double* __restrict__ ux, const double* __restrict__ uy,
                                                 double dt, int32_t nch, const double* __restrict__ cin, double* __restrict__ cout,
                                                 int64_t ld, int32_t* __restrict__ notfound,
                                                 int32_t* __restrict__ nfpart) {
  __shared__ double sh[4];
  double nnf = 0.0;
  int64_t r0, r1;
  block_rows(n, r0, r1);
  for (int64_t i = r0 + threadIdx.x; i < r1; i += BS) {
    const int64_t g = row0 + i;
    const double vx = ux[VS * i], vy = uy[VS * i];
    double xb, yb;
    sl_point(M, g, vx, vy, dt, xb, yb);
    SlTri r{};
    int32_t mark;
    const bool ok = sl_locate_row(M, L, G, g, vx, vy, xb, yb, r, mark);
    if (!ok) nnf += 1.0;
    if (notfound) notfound[i] = mark;
    for (int32_t k = 0; k < nch; ++k) {
      const double* __restrict__ c = cin + (int64_t)k * ld;
      stnt(cout + (int64_t)k * ld + g, ok ? sl_value(r, xb, yb, c) : c[g]);
    }
  }
  const double d = block_sum(nnf, sh);
  if (threadIdx.x == 0) nfpart[blockIdx.x] = (int32_t)d;
}

}  // namespace dev
}  // namespace pucfem
