// Inertia (pucfem_set_inertia, pucfem_sl_advect_vel, include/pucfem.h): the semi-Lagrangian step of a two-component
// nodal field stored as the velocity is, interleaved (x, y) pairs -- Stam's "stable fluids" advection
// u_a = SL(u; u, dt) in front of the viscous solve, each component advected by advect_semilagrange
// (StokesColor.py:347-389).
//
// The back-trace and the point location are k_sl_multi's (pucfem_dye_channels.hpp): sl_locate_row
// (pucfem_locate.hpp), with the same not-found marks and per-block partials.
//
// What differs is the layout.  k_sl_multi with K = 2 takes channel-major vectors: the velocity would need a
// de-interleave pass in front and a re-interleave pass behind.  Here a vertex's pair is one 16-byte gather (three per
// row) and the row's pair one 16-byte non-temporal store: sl_value's pair form, whose component k holds the bits
// sl_value gives for the plain vector of that component (tests/test_gpu_inertia.py).  A row that is not found keeps
// f[g].  The output must not alias f: rows of other blocks still gather from it.
#pragma once
#include "pucfem_kernels_impl.hpp"

namespace pucfem {
namespace dev {

// rows [row0, row0 + n): out[g] = SL(f; u, dt)[g]; f and out hold the (x, y) pairs of every mesh node, u those of the
// rows of this launch (f may be u); notfound (n, or null) and nfpart[block] as k_sl_multi writes them
template <class LOC>
__global__ __launch_bounds__(BS) void k_sl_vel(MeshDev M, LOC L, GridDev G, int64_t row0, int64_t n, const dbl2* u,
                                               double dt, const dbl2* f, dbl2* __restrict__ out,
                                               int32_t* __restrict__ notfound, int32_t* __restrict__ nfpart) {
  __shared__ double sh[4];
  double nnf = 0.0;
  int64_t r0, r1;
  block_rows(n, r0, r1);
  for (int64_t i = r0 + threadIdx.x; i < r1; i += BS) {
    const int64_t g = row0 + i;
    const dbl2 v = u[i];
    double xb, yb;
    sl_point(M, g, v.x, v.y, dt, xb, yb);
    SlTri r{};
    int32_t mark;
    const bool ok = sl_locate_row(M, L, G, g, v.x, v.y, xb, yb, r, mark);
    if (!ok) nnf += 1.0;
    if (notfound) notfound[i] = mark;
    stnt(out + g, ok ? sl_value(r, xb, yb, f) : f[g]);
  }
  const double d = block_sum(nnf, sh);
  if (threadIdx.x == 0) nfpart[blockIdx.x] = (int32_t)d;
}

}  // namespace dev
}  // namespace pucfem
