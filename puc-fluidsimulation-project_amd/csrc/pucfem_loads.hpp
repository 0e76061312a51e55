// Swimmer loads (pucfem_swimmer_loads, pucfem_surface_traction, pucfem_set_loads_record, include/pucfem.h): what the
// fluid does to the swimmer and what the swimmer spends, reduced on the device from the current u and the last step's
// two projection pressures.  One launch: the first `nbe` blocks run the surface edges (one thread per edge), the other
// blocks the triangles (grid-stride); blockIdx.y is the ensemble member (0 on a single context).
//
// Definitions (every product and sum as written; the build has -ffp-contract=off, so a numpy line per operation gives
// the same per-edge bits: tests/loads_reference.py).  For triangle t with vertices 1, 2, 3 in the mesh's order:
//
//   b = (y2 - y3, y3 - y1, y1 - y2)      c = (x3 - x2, x1 - x3, x2 - x1)
//   det = x1 b1 + x2 b2 + x3 b3          inv = 1 / (|det| >= 1e-14 ? det : 1)
//   Gxx = (ux1 b1 + ux2 b2 + ux3 b3) inv     Gxy = (ux1 c1 + ux2 c2 + ux3 c3) inv     (Gyx, Gyy the same from uy)
//
// (the oracle's _divergence_sums form).  For surface edge (t, k) from vertex i = k to j = (k + 1) mod 3, o the third:
//
//   e = X_j - X_i     n = (e_y, -e_x), negated if n . (X_o - X_i) < 0      (length-weighted, out of the body)
//   P = ((p_i + p2_i) + (p_j + p2_j)) / 2       f_p = -(P n)
//   f_v = nu ((Gxx + Gxx) n_x + (Gxy + Gyx) n_y,  (Gxy + Gyx) n_x + (Gyy + Gyy) n_y)
//   r = (X_i + X_j) / 2 - center        torque = r_x f_y - r_y f_x
//   ub = (u_i + u_j) / 2                power = -(ub_x f_x + ub_y f_y)
//
// and per triangle with |det| >= 1e-14 the dissipation nu (|det| / 2) ((2 Gxx^2 + 2 Gyy^2) + (Gxy + Gyx)^2).
//
// The ten reduced values (LOADS_NV): f_p x, y; f_v x, y; torque of f_p, of f_v; power of f_p, of f_v; dissipation;
// perimeter.  Reduction order: a thread its items in order, block_sum, the blocks in order (red_finish); an edge
// block's triangle partial and a triangle block's edge partials are zeros.  For one mesh the grid in x is fixed, so two
// calls return the same bits and an ensemble member's values are those of a single run with its fields.
#pragma once
#include "pucfem_kernels.hpp"
#include "pucfem_locate.hpp"
#include "pucfem_ensemble.hpp"

namespace pucfem {
namespace dev {

constexpr int LOADS_NV = 10;          // reduced values
constexpr int LOADS_EV = 8;           // stored per-edge values: the first eight of the list above, per edge
constexpr int LOADS_ROW = 1 + LOADS_NV;  // a record row: the step count, then the values
// triangle blocks at the most: the chip holds 2,048 blocks of BS threads at once, and the reducing block's tail reads
// 10 partials per block (DESIGN.md §17's note on red_finish at 15k blocks)
constexpr int LOADS_TRI_MAXB = 2048;

// The record (pucfem_set_loads_record): a ring of `cap` rows per member and the rows appended so far, both in device
// memory.  The reducing block appends the row at index count mod cap and advances the count: no host value enters a
// captured launch.  ring null: no record.
struct LoadsRec {
  double* ring;
  int64_t* count;
  int32_t cap;
};

struct LoadsTri {
  int32_t v[3];
  double x[3], y[3];
  dbl2 u[3];
  double gxx, gxy, gyx, gyy, det;
  bool ok;
};
__device__ __forceinline__ LoadsTri loads_tri(const MeshDev& M, const dbl2* __restrict__ u, int64_t t) {
  LoadsTri R;
#pragma unroll
  for (int k = 0; k < 3; ++k) R.v[k] = M.tri[3 * t + k];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    R.x[k] = M.x[R.v[k]];
    R.y[k] = M.y[R.v[k]];
    R.u[k] = u[R.v[k]];
  }
  const double b1 = R.y[1] - R.y[2], b2 = R.y[2] - R.y[0], b3 = R.y[0] - R.y[1];
  const double c1 = R.x[2] - R.x[1], c2 = R.x[0] - R.x[2], c3 = R.x[1] - R.x[0];
  R.det = R.x[0] * b1 + R.x[1] * b2 + R.x[2] * b3;
  R.ok = fabs(R.det) >= 1e-14;
  const double inv = 1.0 / (R.ok ? R.det : 1.0);
  R.gxx = (R.u[0].x * b1 + R.u[1].x * b2 + R.u[2].x * b3) * inv;
  R.gxy = (R.u[0].x * c1 + R.u[1].x * c2 + R.u[2].x * c3) * inv;
  R.gyx = (R.u[0].y * b1 + R.u[1].y * b2 + R.u[2].y * b3) * inv;
  R.gyy = (R.u[0].y * c1 + R.u[1].y * c2 + R.u[2].y * c3) * inv;
  return R;
}
// element k (block- and wave-divergent) of three registers, without an indexed register array
template <class T>
__device__ __forceinline__ T loads_sel(int k, T a, T b, T c) {
  return k == 0 ? a : k == 1 ? b : c;
}

// edge: nE (triangle, local edge) pairs; u: interleaved pairs, p / p2: the pressures (ustride / pstride doubles
// between members); master_of non-null: p and p2 are read at a periodic slave's master (pressures kept in the solve's
// y, whose slave rows are not copied); eout non-null: the LOADS_EV per-edge values (estride doubles between members);
// part: LOADS_NV gridDim.x partials per member.
__global__ __launch_bounds__(BS) void k_loads(MeshDev M, const int2* __restrict__ edge, int32_t nE, int32_t nbe,
                                              const double* __restrict__ u, int64_t ustride,
                                              const double* __restrict__ p, const double* __restrict__ p2,
                                              int64_t pstride, const int32_t* __restrict__ master_of, double nu,
                                              double cx, double cy, double* __restrict__ eout, int64_t estride,
                                              double* part, RedOut ro, LoadsRec rec) {
  __shared__ double sh[4];
  const int32_t m = (int32_t)blockIdx.y;
  const dbl2* um = reinterpret_cast<const dbl2*>(u + (int64_t)m * ustride);
  const RedOut R = ens_red<LOADS_NV>(ro, m, part);
  double acc[LOADS_NV];
#pragma unroll
  for (int v = 0; v < LOADS_NV; ++v) acc[v] = 0.0;
  if ((int32_t)blockIdx.x < nbe) {
    const int32_t e = (int32_t)blockIdx.x * BS + (int32_t)threadIdx.x;
    if (e < nE) {
      const int2 tk = edge[e];
      const int k = tk.y;
      const LoadsTri T = loads_tri(M, um, tk.x);
      const int ki = k, kj = k == 2 ? 0 : k + 1, ko = k == 0 ? 2 : k - 1;
      const int32_t i = loads_sel(ki, T.v[0], T.v[1], T.v[2]), j = loads_sel(kj, T.v[0], T.v[1], T.v[2]);
      const double xi = loads_sel(ki, T.x[0], T.x[1], T.x[2]), yi = loads_sel(ki, T.y[0], T.y[1], T.y[2]);
      const double xj = loads_sel(kj, T.x[0], T.x[1], T.x[2]), yj = loads_sel(kj, T.y[0], T.y[1], T.y[2]);
      const double xo = loads_sel(ko, T.x[0], T.x[1], T.x[2]), yo = loads_sel(ko, T.y[0], T.y[1], T.y[2]);
      const dbl2 ui = loads_sel(ki, T.u[0], T.u[1], T.u[2]), uj = loads_sel(kj, T.u[0], T.u[1], T.u[2]);
      const double* pm = p + (int64_t)m * pstride;
      const double* qm = p2 + (int64_t)m * pstride;
      int32_t ip = i, jp = j;
      if (master_of) {
        if (master_of[i] >= 0) ip = master_of[i];
        if (master_of[j] >= 0) jp = master_of[j];
      }
      const double Pi = pm[ip] + qm[ip], Pj = pm[jp] + qm[jp];
      const double ex = xj - xi, ey = yj - yi;
      double nx = ey, ny = -ex;
      const double side = nx * (xo - xi) + ny * (yo - yi);
      if (side < 0.0) {
        nx = -nx;
        ny = -ny;
      }
      const double Pb = (Pi + Pj) * 0.5;
      const double fpx = -(Pb * nx), fpy = -(Pb * ny);
      const double sxx = T.gxx + T.gxx, sxy = T.gxy + T.gyx, syy = T.gyy + T.gyy;
      const double fvx = nu * (sxx * nx + sxy * ny), fvy = nu * (sxy * nx + syy * ny);
      const double ubx = (ui.x + uj.x) * 0.5, uby = (ui.y + uj.y) * 0.5;
      const double rx = (xi + xj) * 0.5 - cx, ry = (yi + yj) * 0.5 - cy;
      acc[0] = fpx;
      acc[1] = fpy;
      acc[2] = fvx;
      acc[3] = fvy;
      acc[4] = rx * fpy - ry * fpx;
      acc[5] = rx * fvy - ry * fvx;
      acc[6] = -(ubx * fpx + uby * fpy);
      acc[7] = -(ubx * fvx + uby * fvy);
      acc[9] = sqrt(ex * ex + ey * ey);
      if (eout) {
        dbl2* o = reinterpret_cast<dbl2*>(eout + (int64_t)m * estride + (int64_t)e * LOADS_EV);
#pragma unroll
        for (int q = 0; q < LOADS_EV / 2; ++q) o[q] = dbl2{acc[2 * q], acc[2 * q + 1]};
      }
    }
#pragma unroll
    for (int v = 0; v < LOADS_NV; ++v)
      if (v != 8) acc[v] = block_sum(acc[v], sh);
  } else {
    const int64_t nbt = (int64_t)gridDim.x - nbe, b = (int64_t)blockIdx.x - nbe;
    double d = 0.0;
    for (int64_t t = b * BS + threadIdx.x; t < M.T; t += nbt * BS) {
      const LoadsTri T = loads_tri(M, um, t);
      if (T.ok) {
        const double s = T.gxy + T.gyx;
        const double q = (2.0 * (T.gxx * T.gxx) + 2.0 * (T.gyy * T.gyy)) + s * s;
        d += nu * ((0.5 * fabs(T.det)) * q);
      }
    }
    acc[8] = block_sum(d, sh);
  }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int v = 0; v < LOADS_NV; ++v) red_part(R, part, v, acc[v]);
  }
  const bool last = red_finish<8>(R, part, sh);
  if (last && rec.ring && threadIdx.x == 0) {  // (thread 0 stored the values itself)
    const int64_t s = rec.count[m];
    double* row = rec.ring + ((int64_t)m * rec.cap + s % rec.cap) * LOADS_ROW;
    row[0] = (double)(s + 1);
#pragma unroll
    for (int v = 0; v < LOADS_NV; ++v) row[1 + v] = R.out[v];
    rec.count[m] = s + 1;
  }
}

}  // namespace dev
}  // namespace pucfem
