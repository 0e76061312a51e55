// Inertia (pucfem_set_inertia, pucfem_sl_advect_vel, include/pucfem.h): the semi-Lagrangian step of a two-component
// nodal field stored as the velocity is, interleaved (x, y) pairs -- Stam's "stable fluids" advection
// u_a = SL(u; u, dt) in front of the viscous solve, each component advected by advect_semilagrange
// (StokesColor.py:347-389).
//
// The back-trace and the point location are k_sl_multi's (pucfem_dye_channels.hpp), call for call: the zero-velocity
// rows from the build-time table (LatLocDev::self), the lattice fast path (sl_lat_cell + the accept tests of
// sl_lat_value), else the general locate (sl_best -> sl_fast || sl_rank_ok); the same not-found marks and per-block
// partials.  The sequence is restated here, not shared, so k_sl_multi compiles to what it did.
//
// What differs is the layout.  k_sl_multi with K = 2 takes channel-major vectors: the velocity would need a
// de-interleave pass in front and a re-interleave pass behind.  Here a vertex's pair is one 16-byte gather (three per
// row) and the row's pair one 16-byte non-temporal store.  The weights are sl_value's expressions, computed once (the
// library is built with -ffp-contract=off); component k is w1 * f[a].k + w2 * f[b].k + w3 * f[d].k in sl_value's
// operand order, so it holds the bits sl_value gives for the plain vector of that component
// (tests/test_gpu_inertia.py).  A row that is not found keeps f[g].  The output must not alias f: rows of other
// blocks still gather from it.
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
  constexpr bool LAT = std::is_same<LOC, LatLocDev>::value;
  __shared__ double sh[4];
  double nnf = 0.0;
  int64_t r0, r1;
  block_rows(n, r0, r1);
  for (int64_t i = r0 + threadIdx.x; i < r1; i += BS) {
    const int64_t g = row0 + i;
    const dbl2 v = u[i];
    const double vx = v.x, vy = v.y;
    double xb, yb;
    sl_point(M, g, vx, vy, dt, xb, yb);
    SlTri r{};
    bool ok = false, located = false;
    int32_t mark = 1;
    if constexpr (LAT) {
      if (vx == 0.0 && vy == 0.0 && L.self) {
        // q is the row's own node (no-slip walls): the answer settled once at build (k_sl_self)
        const int32_t t = L.self[g];
        if (t >= 0) {
          const int32_t va = M.tri[3 * (int64_t)t], vb = M.tri[3 * (int64_t)t + 1], vc = M.tri[3 * (int64_t)t + 2];
          r = SlTri{M.x[va], M.y[va], M.x[vb], M.y[vb], M.x[vc], M.y[vc], va, vb, vc, t};
          ok = true;
        }
        located = true;
        mark = ok ? 0 : 1;
      } else {
        int32_t v0, v1, v2, id;
        if (sl_lat_cell(L, L.home[g], xb, yb, v0, v1, v2, id)) {
          const double2 P1 = L.xy[v0], P2 = L.xy[v1], P3 = L.xy[v2];
          const float rho2 = L.rho2[id], rv1 = L.rv2[v0], rv2 = L.rv2[v1], rv3 = L.rv2[v2];
          double unused;  // (the stage's own value of a zero field: the pair's values follow below)
          if (sl_lat_value(L.probe, xb, yb, P1, P2, P3, 0.0, 0.0, 0.0, rho2, rv1, rv2, rv3, unused)) {
            r = SlTri{P1.x, P1.y, P2.x, P2.y, P3.x, P3.y, v0, v1, v2, id};
            ok = located = true;
            mark = 0;
          }
        }
      }
    }
    if (!located) {  // k_sl_slow's sequence
      double bestd;
      float rho2;
      const bool cand = sl_best(L, -1, xb, yb, r, bestd, rho2);
      ok = cand && (sl_fast(L, r, xb, yb, bestd, rho2) || sl_rank_ok(G, xb, yb, bestd, r.id, 0.0f, 0));
      mark = ok ? ((L.probe & 2) ? 2 : 0) : 1;
    }
    if (!ok) nnf += 1.0;
    if (notfound) notfound[i] = mark;
    dbl2 o;
    if (!ok) {
      o = f[g];
    } else {
      const dbl2 fa = f[r.a], fb = f[r.b], fd = f[r.d];
      // sl_value's weights (StokesColor.py:374-386), once for both components
      const double x1 = r.x1, y1 = r.y1, x2 = r.x2, y2 = r.y2, x3 = r.x3, y3 = r.y3;
      const double det = pdx(x2, x1) * (y3 - y1) - pdx(x3, x1) * (y2 - y1);
      const double w1 = (pdx(x2, xb) * (y3 - yb) - pdx(x3, xb) * (y2 - yb)) / det;
      const double w2 = (pdx(x3, xb) * (y1 - yb) - pdx(x1, xb) * (y3 - yb)) / det;
      const double w3 = 1.0 - w1 - w2;
      o.x = w1 * fa.x + w2 * fb.x + w3 * fd.x;
      o.y = w1 * fa.y + w2 * fb.y + w3 * fd.y;
    }
    stnt(out + g, o);
  }
  const double d = block_sum(nnf, sh);
  if (threadIdx.x == 0) nfpart[blockIdx.x] = (int32_t)d;
}

}  // namespace dev
}  // namespace pucfem
