// Point location for the semi-Lagrangian kernels, the samplers and the streamlines: the locators' device structs,
// the per-candidate tests, and the "where did this row come from" sequences built on them.
//
// ONE layer, two forms.  Every kernel that locates a back-traced point calls one of
//   sl_locate_general  one lane per point: sl_best -> sl_fast || sl_rank_ok
//   sl_locate_row      one lane per row: the build-time table of the zero-velocity rows (LatLocDev::self), the
//                      lattice fast path (sl_lat_cell + the accept tests of sl_lat_value), else sl_locate_general
//   sl_locate_wave     one wave per point: sl_best_wave -> sl_fast || sl_rank_ok_wave (sl_row_wave: with the
//                      back-trace in front and the value behind)
// and interpolates with sl_value (one field, or an interleaved pair) on sl_weights.  What the layer guarantees, for
// the thread and the wave forms alike:
//   the same triangle    among the triangles that pass the reference's weight test (sl_test), the smallest
//                        (d^2, id) key in knn_less's order, accepted iff its rank among the centroids is below KNN.
//                        The wave forms test the candidates of the sequential scan with the same arithmetic each; the
//                        scan's early exits (an inner cell, a margin pass) are taken only at a triangle that is the
//                        only one passing, so they never change the answer;
//   the same key order   knn_less everywhere: the scan's running minimum, wave_min_key, both rank counts;
//   the same marks       sl_mark: 0 found, 1 not found (the row keeps its own value), 2 found by the general locate
//                        under probe bit 1; the self table and the fast path mark 0;
//   the same bits        every product and sum keeps the expression order of the single-dye kernels (the library is
//                        built with -ffp-contract=off), so a channel, a velocity component or an ensemble member
//                        holds the bits of the single run (tests/test_gpu_dye_channels.py, test_gpu_inertia.py,
//                        test_gpu_ensemble.py).
// A fix to an accept test, a mark or a key is made here, once.  The kernels keep their own parts: which rows they
// own, which field they interpolate, their stores and partials.
// What is still restated, each with a note where it stands: the code generated for k_sl (every row of a step), for
// k_sl_wq and for the samplers and streamlines had to stay instruction for instruction what it was, and these
// sharings changed it -- k_sl_wq's call sequence and sl_best_wave2's decode and winner broadcast; the near-cell
// predicate of the three lattice scans; the cell-to-vertex-ids step of sl_cell and sl_lat_cell.  The comparison of
// the generated code, kernel by kernel, and the measured rates: profiles/sl_locate_shared.txt.
#pragma once
#include <type_traits>

#include "pucfem_kernels.hpp"

namespace pucfem {
namespace dev {

struct MeshDev {
  const double* x;      // full mesh, internal numbering
  const double* y;
  const int32_t* tri;   // T*3 internal node ids, reference triangle order
  int64_t T;
};
struct GridDev {
  int32_t nx, ny;
  double x0, y0, hx, hy;
  const int32_t* start;
  const int32_t* item;
  const double* px;
  const double* py;
};

__device__ __forceinline__ int32_t gcell(double v, double v0, double hv, int32_t n) {
  const double f = floor((v - v0) / hv);
  if (!(f >= 0.0)) return 0;
  if (f >= (double)n) return n - 1;
  return (int32_t)f;
}

__device__ __forceinline__ bool knn_less(double d, int32_t i, double bd, int32_t bi) {
  return d < bd || (d == bd && i < bi);
}

// Point location for the semi-Lagrangian step (PointLocator.find, StokesColor.py:314-345).
// The reference takes the k=10 nearest centroids in (distance, id) order and returns the first
// whose barycentric weights are all >= 0.  Restated exactly, without sorting 10 candidates:
//   1. every triangle that passes the weight test for q has q inside it up to rounding, so it is
//      listed in q's cell of the inflated-bbox grid L; among those that pass, take the one with the
//      smallest (d^2, id) key T*.  A triangle whose weights are all >= SL_MARGIN contains q with a
//      margin no other triangle's test can reach, so the scan stops at it;
//   2. T* is the answer iff fewer than 10 centroids have a key below T*'s (its rank is < 10).  Fast
//      accept: every such centroid c has |c - c_T*| <= 2 R (R = |q - c_T*|), so 4 R^2 below the
//      squared distance from c_T* to its 10th nearest other centroid (rho2, precomputed) bounds the
//      rank by 9.  Otherwise they are counted over the centroid-grid cells meeting [q - R, q + R]^2.
// Otherwise no triangle among the 10 nearest passes and the reference keeps c[n].
// Records are stored in node order (triangles sorted by their smallest vertex id), not in the
// mesh's triangle order, and hold vertex ids only (16 B: a, b, d and the mesh's triangle id, which
// the (distance, id) keys keep); the vertex coordinates come from one interleaved (x, y) array in
// node order, which neighbouring triangles share.  Cells list record positions.
struct LocDev {
  int32_t nx, ny;
  double x0, y0, hx, hy;
  const int32_t* start;  // nx*ny+1
  const int32_t* item;   // record positions, ascending per cell
  const int4* rec;       // per position: vertex ids a b d, triangle id
  const double2* xy;     // node coordinates (internal numbering)
  // per position: squared distance from the centroid to the 10th nearest other centroid (rounded down)
  const float* rho2;
  const float* rv2;  // per node: squared distance to its (KNN + 1)-th nearest centroid (rounded down)
  // measurement knob (PUCFEM_SL_PROBE): bit 0 = accept T* without the rank count, bit 1 = not-found
  // output 2 for the rows k_sl_slow finished (pucfem_sl_advect)
  int32_t probe;
};
struct SlTri {
  double x1, y1, x2, y2, x3, y3;
  int32_t a, b, d, id;
};
__device__ __forceinline__ SlTri sl_tri(const LocDev& L, int32_t pos) {
  const int4 m = L.rec[pos];
  const double2 p = L.xy[m.x], q = L.xy[m.y], s = L.xy[m.z];
  return SlTri{p.x, p.y, q.x, q.y, s.x, s.y, m.x, m.y, m.z, m.w};
}
constexpr double SL_MARGIN = 1e-6;

// rank test of the best passing triangle (id best, squared centroid distance bestd), after sl_fast's
// accepts: true iff fewer than KNN centroids have a (d^2, id) key below it
__device__ __forceinline__ bool sl_rank_ok(const GridDev& G, double qx, double qy, double bestd, int32_t best) {
  const double R = sqrt(bestd) * (1.0 + 1e-9) + 1e-300;
  const int32_t i0 = gcell(qx - R, G.x0, G.hx, G.nx), i1 = gcell(qx + R, G.x0, G.hx, G.nx);
  const int32_t j0 = gcell(qy - R, G.y0, G.hy, G.ny), j1 = gcell(qy + R, G.y0, G.hy, G.ny);
  int cnt = 0;
  for (int32_t j = j0; j <= j1; ++j) {
    const int32_t f0 = G.start[(int64_t)j * G.nx + i0], f1 = G.start[(int64_t)j * G.nx + i1 + 1];
    for (int32_t e = f0; e < f1; ++e) {  // cells i0..i1 of row j are one contiguous entry range
      const double dx = G.px[e] - qx, dy = G.py[e] - qy;
      const double d = dx * dx + dy * dy;
      if (knn_less(d, G.item[e], bestd, best) && ++cnt >= KNN) return false;
    }
  }
  return true;
}

// the reference's weight test (StokesColor.py:325-333) and centroid distance of one candidate
__device__ __forceinline__ bool sl_test(const SlTri& r, double qx, double qy, double& d, bool& margin) {
  const double x1 = r.x1, y1 = r.y1, x2 = r.x2, y2 = r.y2, x3 = r.x3, y3 = r.y3;
  const double det = (x2 - x1) * (y3 - y1) - (x3 - x1) * (y2 - y1);
  if (!(fabs(det) >= 1e-14)) return false;
  const double w1 = ((x2 - qx) * (y3 - qy) - (x3 - qx) * (y2 - qy)) / det;
  const double w2 = ((x3 - qx) * (y1 - qy) - (x1 - qx) * (y3 - qy)) / det;
  const double w3 = 1.0 - w1 - w2;
  if (!(w1 >= 0.0 && w2 >= 0.0 && w3 >= 0.0)) return false;
  // centroid as StokesColor.py:321 / the centroid grid: (x1 + x2 + x3) / 3 in fp64
  const double dx = (x1 + x2 + x3) / 3.0 - qx, dy = (y1 + y2 + y3) / 3.0 - qy;
  d = dx * dx + dy * dy;
  margin = w1 >= SL_MARGIN && w2 >= SL_MARGIN && w3 >= SL_MARGIN;
  return true;
}

// Locate step (the rank test follows in k_sl_slow): the passing triangle with the smallest
// (d^2, id) key (false: none passes), its d^2 and its fast-accept radius.
// Record locator: the records listed in q's cell of the inflated-bbox grid.
__device__ __forceinline__ bool sl_best(const LocDev& L, int32_t, double qx, double qy, SlTri& out, double& bestd,
                                        float& rho2) {
  const int32_t ci = gcell(qx, L.x0, L.hx, L.nx), cj = gcell(qy, L.y0, L.hy, L.ny);
  const int64_t cell = (int64_t)cj * L.nx + ci;
  int32_t best = 0x7fffffff, bpos = -1;
  bestd = INFINITY;
  const int32_t e1 = L.start[cell + 1];
  for (int32_t e = L.start[cell]; e < e1; ++e) {
    const int32_t pos = L.item[e];
    const SlTri r = sl_tri(L, pos);
    double d;
    bool margin;
    if (sl_test(r, qx, qy, d, margin)) {
      if (knn_less(d, r.id, bestd, best)) {
        bestd = d;
        best = r.id;
        bpos = pos;
        out = r;
      }
      if (margin) break;
    }
  }
  if (bpos < 0) return false;
  rho2 = L.rho2[bpos];
  return true;
}

// Lattice locator (Ctx::lattice): the finest mesh is the coarse mesh red-refined L times, so the
// candidates of the weight test are found arithmetically instead of from per-triangle records: the
// macro faces listed in q's cell of a grid over the coarse triangles (inflated bboxes), q's lattice
// coordinates (u, v) = n M (q - A) in each, and the cells (i, j, s) whose closure holds (u, v) up to
// SL_LDEL lattice units (one cell away from edges, more only within 1e-7 of a lattice line, where the
// reference's weight test can pass in several triangles).  The rotation stored in the cell table
// gives the triangle's vertices in the mesh's own order, so the weight test and the (d^2, id) keys
// are the record locator's, bit for bit.
struct LatLocDev {
  int32_t nx, ny;
  double x0, y0, ihx, ihy;       // macro grid: origin, inverse cell sizes
  const int32_t* start;          // macro grid cells -> face ids
  const int32_t* item;
  const lat::SlFace* face;
  const uint32_t* cell;          // per lattice cell (lat::cell_index): (offset in face << 2) | rotation
  const double2* xy;             // node coordinates (internal numbering)
  const float* rho2;             // per triangle id
  const float* rv2;              // per node, as LocDev::rv2
  const int32_t* home;           // per row (internal id): its macro face (face-interior rows), else -1
  // per row: the triangle the locator returns for the row's own node (a zero velocity: walls), -1 when
  // none is accepted (k_sl_self, once at build); null until then
  const int32_t* self;
  int32_t n, probe;
};
constexpr double SL_LDEL = 1e-7;

// q's cell of the macro grid, by multiplication: a point within rounding of a cell line may land in
// either cell, and both list every face whose (inflated) bbox holds it
__device__ __forceinline__ int64_t lat_gcell(const LatLocDev& L, double qx, double qy) {
  const double gx = floor((qx - L.x0) * L.ihx), gy = floor((qy - L.y0) * L.ihy);
  const int32_t ci = !(gx >= 0.0) ? 0 : (gx >= (double)L.nx ? L.nx - 1 : (int32_t)gx);
  const int32_t cj = !(gy >= 0.0) ? 0 : (gy >= (double)L.ny ? L.ny - 1 : (int32_t)gy);
  return (int64_t)cj * L.nx + ci;
}
// one lattice cell of face S as an SlTri (vertices in the mesh's stored order: the cell's list
// rotated by the table's rotation; selects, not a dynamically indexed array, which would live in LDS)
__device__ __forceinline__ SlTri sl_cell(const LatLocDev& L, const lat::SlFace& S, int32_t i, int32_t j, int32_t s) {
  const uint32_t ent = L.cell[lat::cell_index(L.n, i, j, s)];
  const int32_t rot = (int32_t)(ent & 3u);
  int32_t pi[3], pj[3];
  lat::cell_vertices(i, j, s, pi, pj);
  const int32_t c0 = lat::vertex(S.tab, S.va, S.vb, S.vc, L.n, pi[0], pj[0]);
  const int32_t c1 = lat::vertex(S.tab, S.va, S.vb, S.vc, L.n, pi[1], pj[1]);
  const int32_t c2 = lat::vertex(S.tab, S.va, S.vb, S.vc, L.n, pi[2], pj[2]);
  const int32_t v0 = rot == 0 ? c0 : (rot == 1 ? c1 : c2);
  const int32_t v1 = rot == 0 ? c1 : (rot == 1 ? c2 : c0);
  const int32_t v2 = rot == 0 ? c2 : (rot == 1 ? c0 : c1);
  const double2 p = L.xy[v0], q = L.xy[v1], w = L.xy[v2];
  return SlTri{p.x, p.y, q.x, q.y, w.x, w.y, v0, v1, v2, (int32_t)(S.t0 + (int64_t)(ent >> 2))};
}

// q strictly inside one cell of face S (by SL_LDEL lattice units, hence inside the face and in no
// other triangle's weight test): that cell; its key d is the reference's, exactly
__device__ __forceinline__ bool sl_inner(const LatLocDev& L, const lat::SlFace& S, double qx, double qy, SlTri& out,
                                         double& bestd, double& u, double& v) {
  const int32_t n = L.n;
  const double dx = qx - S.ax, dy = qy - S.ay;
  u = (double)n * (S.m00 * dx + S.m01 * dy);
  v = (double)n * (S.m10 * dx + S.m11 * dy);
  const double fu = floor(u), fv = floor(v);
  const double a = u - fu, b = v - fv;
  const int32_t s = a + b > 1.0 ? 1 : 0;
  const bool inner = s == 0 ? (a >= SL_LDEL && b >= SL_LDEL && a + b <= 1.0 - SL_LDEL)
                            : (a <= 1.0 - SL_LDEL && b <= 1.0 - SL_LDEL && a + b >= 1.0 + SL_LDEL);
  if (!(inner && fu >= 0.0 && fv >= 0.0 && fu + fv <= (double)(n - 1 - s))) return false;
  out = sl_cell(L, S, (int32_t)fu, (int32_t)fv, s);
  // the weights are >= SL_LDEL up to rounding: the weight test passes; only its det guard remains
  const double det = (out.x2 - out.x1) * (out.y3 - out.y1) - (out.x3 - out.x1) * (out.y2 - out.y1);
  if (!(fabs(det) >= 1e-14)) return false;
  const double ex = (out.x1 + out.x2 + out.x3) / 3.0 - qx, ey = (out.y1 + out.y2 + out.y3) / 3.0 - qy;
  bestd = ex * ex + ey * ey;
  return true;
}

// Lattice locator.  Common case: q lies inside a macro face and inside one lattice cell by more than
// SL_LDEL, so no other triangle can pass the weight test: that cell alone is tested.  Otherwise every
// cell of every candidate face whose closure holds q up to SL_LDEL is tested, as the record locator
// tests every record of its grid cell.
__device__ __forceinline__ bool sl_best(const LatLocDev& L, int32_t home, double qx, double qy, SlTri& out,
                                        double& bestd, float& rho2) {
  double u, v;
  if (home >= 0 && sl_inner(L, L.face[home], qx, qy, out, bestd, u, v)) {
    rho2 = L.rho2[out.id];
    return true;
  }
  const int64_t gc = lat_gcell(L, qx, qy);
  const int32_t n = L.n;
  const double dn = (double)n;
  int32_t best = 0x7fffffff;
  bestd = INFINITY;
  bool done = false;
  const int32_t e1 = L.start[gc + 1];
  for (int32_t e = L.start[gc]; e < e1 && !done; ++e) {
    const lat::SlFace& S = L.face[L.item[e]];
    {
      SlTri r;
      double d;
      if (sl_inner(L, S, qx, qy, r, d, u, v)) {
        if (knn_less(d, r.id, bestd, best)) {
          bestd = d;
          best = r.id;
          out = r;
        }
        break;
      }
    }
    if (!(u >= -SL_LDEL && v >= -SL_LDEL && u + v <= dn + SL_LDEL)) continue;
    const int32_t i0 = min(max((int32_t)floor(u), 0), n - 1), j0 = min(max((int32_t)floor(v), 0), n - 1);
    for (int32_t j = max(j0 - 1, 0); j <= j0 + 1 && !done; ++j)
      for (int32_t i = max(i0 - 1, 0); i <= i0 + 1 && i + j <= n - 1 && !done; ++i) {
        const double a = u - i, b = v - j;
        for (int32_t s = 0; s < 2 && !done; ++s) {
          const bool near = s == 0 ? (a >= -SL_LDEL && b >= -SL_LDEL && a + b <= 1.0 + SL_LDEL)
                                   : (i + j <= n - 2 && a <= 1.0 + SL_LDEL && b <= 1.0 + SL_LDEL && a + b >= 1.0 - SL_LDEL);
          if (!near) continue;
          const SlTri r = sl_cell(L, S, i, j, s);
          double d;
          bool margin;
          if (sl_test(r, qx, qy, d, margin)) {
            if (knn_less(d, r.id, bestd, best)) {
              bestd = d;
              best = r.id;
              out = r;
            }
            done = margin;
          }
        }
      }
  }
  if (best == 0x7fffffff) return false;
  rho2 = L.rho2[best];
  return true;
}

__device__ __forceinline__ double pdx(double a, double b) {  // StokesColor.py:353-357
  double d = a - b;
  if (d > 0.5) d -= 1.0;
  if (d < -0.5) d += 1.0;
  return d;
}

// back-traced point of a node at (x, y) moving with (vx, vy) (StokesColor.py:361-372): x mod 1, y clamped
// into (0, 1).  One function per coordinate, by value: sl_point keeps its load of y behind the x arithmetic and
// k_sl's stage B its code (a single by-reference sl_point_xy changed both, profiles/sl_locate_shared.txt)
__device__ __forceinline__ double sl_point_x(double x, double vx, double dt) { return py_mod1(x - dt * vx * 1.0); }
__device__ __forceinline__ double sl_point_y(double y, double vy, double dt) {
  double yb = y - dt * vy * 1.0;
  if (yb < 0.0) yb = 1e-12;
  if (yb > 1.0) yb = 1.0 - 1e-12;
  return yb;
}
// ... of row g
__device__ __forceinline__ void sl_point(const MeshDev& M, int64_t g, double vx, double vy, double dt, double& xb,
                                         double& yb) {
  xb = sl_point_x(M.x[g], vx, dt);
  yb = sl_point_y(M.y[g], vy, dt);
}
// interpolation weights of (xb, yb) in the located triangle, with periodic x differences
// (StokesColor.py:374-386); only r's coordinates are read
struct SlW {
  double w1, w2, w3;
};
__device__ __forceinline__ SlW sl_weights(const SlTri& r, double xb, double yb) {
  const double x1 = r.x1, y1 = r.y1, x2 = r.x2, y2 = r.y2, x3 = r.x3, y3 = r.y3;
  const double det = pdx(x2, x1) * (y3 - y1) - pdx(x3, x1) * (y2 - y1);
  const double w1 = (pdx(x2, xb) * (y3 - yb) - pdx(x3, xb) * (y2 - yb)) / det;
  const double w2 = (pdx(x3, xb) * (y1 - yb) - pdx(x1, xb) * (y3 - yb)) / det;
  return SlW{w1, w2, 1.0 - w1 - w2};
}
// the interpolated value of a nodal field c
__device__ __forceinline__ double sl_value(const SlTri& r, double xb, double yb, const double* __restrict__ c) {
  const SlW w = sl_weights(r, xb, yb);
  return w.w1 * c[r.a] + w.w2 * c[r.b] + w.w3 * c[r.d];
}
// ... of a field of interleaved pairs: three 16-byte gathers, the weights once, component k in sl_value's
// operand order, so it holds the bits sl_value gives for the plain vector of that component
__device__ __forceinline__ dbl2 sl_value(const SlTri& r, double xb, double yb, const dbl2* f) {
  const dbl2 fa = f[r.a], fb = f[r.b], fd = f[r.d];
  const SlW w = sl_weights(r, xb, yb);
  return dbl2{w.w1 * fa.x + w.w2 * fb.x + w.w3 * fd.x, w.w1 * fa.y + w.w2 * fb.y + w.w3 * fd.y};
}

// Lattice fast path, in two stages so that k_sl can overlap one row's second stage with the next row's
// first.  Stage 1 (sl_lat_cell): q strictly inside a cell of its row's home face, else of the first face
// of q's macro-grid cell holding q so -> the cell triangle's vertices and id (false: the general
// locate of k_sl_slow decides).  Stage 2 (sl_lat_value): with the triangle's coordinates, field values
// and radii loaded (all issued together), the det guard, the rank settled by a fast accept (sl_fast's
// tests) and the interpolated value (false: k_sl_slow decides).  Scalars only (a struct here ends in
// scratch memory).
__device__ __forceinline__ bool sl_lat_cell(const LatLocDev& L, int32_t home, double qx, double qy, int32_t& v0,
                                            int32_t& v1, int32_t& v2, int32_t& id) {
  const int32_t n = L.n;
  int32_t f = -1;
  double fu = 0.0, fv = 0.0;
  int32_t s = 0;
  auto inner = [&](int32_t cand) {
    const lat::SlFace& S = L.face[cand];
    const double dx = qx - S.ax, dy = qy - S.ay;
    const double u = (double)n * (S.m00 * dx + S.m01 * dy), v = (double)n * (S.m10 * dx + S.m11 * dy);
    fu = floor(u);
    fv = floor(v);
    const double a = u - fu, b = v - fv;
    s = a + b > 1.0 ? 1 : 0;
    const bool in = s == 0 ? (a >= SL_LDEL && b >= SL_LDEL && a + b <= 1.0 - SL_LDEL)
                           : (a <= 1.0 - SL_LDEL && b <= 1.0 - SL_LDEL && a + b >= 1.0 + SL_LDEL);
    return in && fu >= 0.0 && fv >= 0.0 && fu + fv <= (double)(n - 1 - s);
  };
  if (home >= 0 && inner(home)) {
    f = home;
  } else {
    const int64_t gc = lat_gcell(L, qx, qy);
    const int32_t e1 = L.start[gc + 1];
    for (int32_t e = L.start[gc]; e < e1; ++e) {
      const int32_t cand = L.item[e];
      if (cand != home && inner(cand)) {
        f = cand;
        break;
      }
    }
    if (f < 0) return false;
  }
  // sl_cell's ids (restated: through a shared helper the samplers' and the streamlines' sl_best compiled to other code)
  const lat::SlFace& S = L.face[f];
  const int32_t i = (int32_t)fu, j = (int32_t)fv;
  const uint32_t ent = L.cell[lat::cell_index(n, i, j, s)];
  const int32_t rot = (int32_t)(ent & 3u);
  int32_t pi[3], pj[3];
  lat::cell_vertices(i, j, s, pi, pj);
  const int32_t c0 = lat::vertex(S.tab, S.va, S.vb, S.vc, n, pi[0], pj[0]);
  const int32_t c1 = lat::vertex(S.tab, S.va, S.vb, S.vc, n, pi[1], pj[1]);
  const int32_t c2 = lat::vertex(S.tab, S.va, S.vb, S.vc, n, pi[2], pj[2]);
  v0 = rot == 0 ? c0 : (rot == 1 ? c1 : c2);
  v1 = rot == 0 ? c1 : (rot == 1 ? c2 : c0);
  v2 = rot == 0 ? c2 : (rot == 1 ? c0 : c1);
  id = (int32_t)(S.t0 + (int64_t)(ent >> 2));
  return true;
}
// stage 2 on the loaded values: P1..P3 the vertex coordinates, f1..f3 the field values, rho2 the
// triangle's fast-accept radius, rv1..rv3 the vertices' radii
__device__ __forceinline__ bool sl_lat_value(int32_t probe, double qx, double qy, double2 P1, double2 P2, double2 P3,
                                             double f1, double f2, double f3, float rho2, float rv1, float rv2,
                                             float rv3, double& cn) {
  const double x1 = P1.x, y1 = P1.y, x2 = P2.x, y2 = P2.y, x3 = P3.x, y3 = P3.y;
  // the weights are >= SL_LDEL up to rounding: the weight test passes; only its det guard remains
  const double det0 = (x2 - x1) * (y3 - y1) - (x3 - x1) * (y2 - y1);
  if (!(fabs(det0) >= 1e-14)) return false;
  const double ex = (x1 + x2 + x3) / 3.0 - qx, ey = (y1 + y2 + y3) / 3.0 - qy;
  const double bestd = ex * ex + ey * ey;
  if (!(4.0 * bestd * (1.0 + 1e-9) < (double)rho2 || (probe & 1))) {
    const double d1 = (x1 - qx) * (x1 - qx) + (y1 - qy) * (y1 - qy);
    const double d2 = (x2 - qx) * (x2 - qx) + (y2 - qy) * (y2 - qy);
    const double d3 = (x3 - qx) * (x3 - qx) + (y3 - qy) * (y3 - qy);
    const bool k1 = d1 <= d2 && d1 <= d3, k2 = !k1 && d2 <= d3;
    const double rr = sqrt(k1 ? d1 : (k2 ? d2 : d3)) + sqrt(bestd);
    if (!(rr * rr * (1.0 + 1e-9) < (double)(k1 ? rv1 : (k2 ? rv2 : rv3)))) return false;
  }
  const SlW w = sl_weights(SlTri{x1, y1, x2, y2, x3, y3, 0, 0, 0, 0}, qx, qy);
  cn = w.w1 * f1 + w.w2 * f2 + w.w3 * f3;
  return true;
}

// Fast accepts of the rank test (T* among the KNN nearest centroids); every centroid whose key is
// below T*'s lies within R = |q - c_T*| of q.  (1) they lie within 2R of c_T*: fewer than KNN when
// 2R is below the distance from c_T* to its KNN-th nearest other centroid (rho2) -- settles points
// near the centroid; (2) they and c_T* lie within |q - v| + R of T*'s vertex v nearest to q: fewer
// than KNN + 1 in all when that is below the distance from v to its (KNN + 1)-th nearest centroid
// (rv2) -- settles points near vertices and edges, where back-traced points of slow flow gather.
template <class LOC>
__device__ __forceinline__ bool sl_fast(const LOC& L, const SlTri& r, double qx, double qy, double bestd, float rho2) {
  if (4.0 * bestd * (1.0 + 1e-9) < (double)rho2 || (L.probe & 1)) return true;
  const double d1 = (r.x1 - qx) * (r.x1 - qx) + (r.y1 - qy) * (r.y1 - qy);
  const double d2 = (r.x2 - qx) * (r.x2 - qx) + (r.y2 - qy) * (r.y2 - qy);
  const double d3 = (r.x3 - qx) * (r.x3 - qx) + (r.y3 - qy) * (r.y3 - qy);
  const bool k1 = d1 <= d2 && d1 <= d3, k2 = !k1 && d2 <= d3;
  const double rr = sqrt(k1 ? d1 : (k2 ? d2 : d3)) + sqrt(bestd);
  return rr * rr * (1.0 + 1e-9) < (double)L.rv2[k1 ? r.a : (k2 ? r.b : r.d)];
}

// (d, id) key minimum over the wave (every lane gets it)
__device__ __forceinline__ void wave_min_key(double& d, int32_t& id) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double od = __shfl_xor(d, o, 64);
    const int32_t oi = __shfl_xor(id, o, 64);
    if (knn_less(od, oi, d, id)) {
      d = od;
      id = oi;
    }
  }
}
// The winner of a wave's candidates: the smallest key over the lanes' own best (md, mid) and the triangle of the
// lane that holds it, for every lane (one lane holds the winning cell; ties are one triangle); the lane, or -1
// when no lane has a candidate.  The triangle's id is the key's, so nine shuffles, not ten.
__device__ __forceinline__ int wave_bcast_tri(const SlTri& mine, double md, int32_t mid, SlTri& out, double& bestd) {
  double bd = md;
  int32_t bid = mid;
  wave_min_key(bd, bid);
  if (bid == 0x7fffffff) return -1;
  const int src = __ffsll((unsigned long long)__ballot(md == bd && mid == bid)) - 1;
  out.x1 = __shfl(mine.x1, src, 64);
  out.y1 = __shfl(mine.y1, src, 64);
  out.x2 = __shfl(mine.x2, src, 64);
  out.y2 = __shfl(mine.y2, src, 64);
  out.x3 = __shfl(mine.x3, src, 64);
  out.y3 = __shfl(mine.y3, src, 64);
  out.a = __shfl(mine.a, src, 64);
  out.b = __shfl(mine.b, src, 64);
  out.d = __shfl(mine.d, src, 64);
  out.id = bid;
  bestd = bd;
  return src;
}
// the general lattice locate of one point by a whole wave (sl_best with home = -1): false when no cell passes
__device__ __forceinline__ bool sl_best_wave(const LatLocDev& L, double qx, double qy, SlTri& out, double& bestd,
                                             float& rho2) {
  const int lane = threadIdx.x & 63;
  const int64_t gc = lat_gcell(L, qx, qy);
  const int32_t n = L.n;
  const double dn = (double)n;
  const int32_t e0 = L.start[gc], e1 = L.start[gc + 1];
  double md = INFINITY;
  int32_t mid = 0x7fffffff;
  SlTri mine{};
  // candidate k = (face e0 + k / 18, cell k % 18): 3 rows j x 3 columns i x 2 orientations s around (u, v), the
  // sequential scan's cells; cell 0 of a face also reports its inner cell.  Chunks of 64 candidates, in the scan's
  // order, until one holds an inner cell or a margin pass (the only passing triangle then: the scan stops there too)
  const int32_t total = (e1 - e0) * 18;
  for (int32_t base = 0; base < total; base += 64) {
    const int32_t k = base + lane;
    bool hit = false;
    if (k < total) {
      const lat::SlFace& S = L.face[L.item[e0 + k / 18]];
      const int32_t c = k % 18;
      SlTri r;
      double d, u, v;
      if (sl_inner(L, S, qx, qy, r, d, u, v)) {
        hit = true;
        if (c == 0 && knn_less(d, r.id, md, mid)) {
          md = d;
          mid = r.id;
          mine = r;
        }
      } else if (u >= -SL_LDEL && v >= -SL_LDEL && u + v <= dn + SL_LDEL) {
        const int32_t i0 = min(max((int32_t)floor(u), 0), n - 1), j0 = min(max((int32_t)floor(v), 0), n - 1);
        const int32_t j = max(j0 - 1, 0) + c / 6, i = max(i0 - 1, 0) + (c / 2) % 3, s = c & 1;
        const double a = u - i, b = v - j;
        const bool near = !(j > j0 + 1 || i > i0 + 1 || i + j > n - 1) &&
                          (s == 0 ? (a >= -SL_LDEL && b >= -SL_LDEL && a + b <= 1.0 + SL_LDEL)
                                  : (i + j <= n - 2 && a <= 1.0 + SL_LDEL && b <= 1.0 + SL_LDEL && a + b >= 1.0 - SL_LDEL));
        if (near) {
          r = sl_cell(L, S, i, j, s);
          bool margin;
          if (sl_test(r, qx, qy, d, margin)) {
            hit = margin;
            if (knn_less(d, r.id, md, mid)) {
              md = d;
              mid = r.id;
              mine = r;
            }
          }
        }
      }
    }
    if (__ballot(hit)) break;
  }
  if (wave_bcast_tri(mine, md, mid, out, bestd) < 0) return false;
  rho2 = L.rho2[out.id];
  return true;
}
// sl_rank_ok by a whole wave: the centroids below (bestd, best) counted over the lanes (same result).  The grid rows
// of the box [q - R, q + R] are flattened into one entry range (each row's cells are one contiguous entry range; a
// wave scan of their lengths), so the lanes load entries of every row at once instead of one row after another
__device__ __forceinline__ bool sl_rank_ok_wave(const GridDev& G, double qx, double qy, double bestd, int32_t best) {
  const int lane = threadIdx.x & 63;
  const double R = sqrt(bestd) * (1.0 + 1e-9) + 1e-300;
  const int32_t i0 = gcell(qx - R, G.x0, G.hx, G.nx), i1 = gcell(qx + R, G.x0, G.hx, G.nx);
  const int32_t j0 = gcell(qy - R, G.y0, G.hy, G.ny), j1 = gcell(qy + R, G.y0, G.hy, G.ny);
  const int32_t nrow = j1 - j0 + 1;
  int cnt = 0;
  if (nrow > 64) {  // (a box taller than a wave: row after row)
    for (int32_t j = j0; j <= j1; ++j) {
      const int32_t f0 = G.start[(int64_t)j * G.nx + i0], f1 = G.start[(int64_t)j * G.nx + i1 + 1];
      for (int32_t e = f0; e < f1; e += 64) {
        bool below = false;
        if (e + lane < f1) {
          const double dx = G.px[e + lane] - qx, dy = G.py[e + lane] - qy;
          below = knn_less(dx * dx + dy * dy, G.item[e + lane], bestd, best);
        }
        cnt += __popcll(__ballot(below));
        if (cnt >= KNN) return false;
      }
    }
    return true;
  }
  int32_t f0 = 0, len = 0;
  if (lane < nrow) {
    const int64_t rb = (int64_t)(j0 + lane) * G.nx;
    f0 = G.start[rb + i0];
    len = G.start[rb + i1 + 1] - f0;
  }
  int32_t incl = len;  // inclusive scan of the row lengths
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int32_t y = __shfl_up(incl, o, 64);
    if (lane >= o) incl += y;
  }
  const int32_t total = __shfl(incl, 63, 64), excl = incl - len;
  for (int32_t base = 0; base < total; base += 64) {
    const int32_t t = base + lane;
    int32_t e = -1;
    for (int32_t r = 0; r < nrow; ++r) {  // (uniform loop: every lane shuffles)
      const int32_t ex = __shfl(excl, r, 64), ln = __shfl(len, r, 64), st = __shfl(f0, r, 64);
      if (t >= ex && t < ex + ln) e = st + (t - ex);
    }
    bool below = false;
    if (e >= 0) {
      const double dx = G.px[e] - qx, dy = G.py[e] - qy;
      below = knn_less(dx * dx + dy * dy, G.item[e], bestd, best);
    }
    cnt += __popcll(__ballot(below));
    if (cnt >= KNN) return false;
  }
  return true;
}
// the general lattice locate of one point by a whole wave, faces first: the lanes take the candidate faces of q's
// macro-grid cell (sl_inner: an inner cell is the only passing triangle), then the cells around (u, v) of every face
// whose closure holds q up to SL_LDEL -- the candidates the sequential scan tests, with the same arithmetic each (it
// stops early only at a pass that is the only passing triangle): two rounds of dependent loads per 64 faces where
// sl_best_wave's 64-candidate chunks (3.6 faces each) took one round per chunk
__device__ __forceinline__ bool sl_best_wave2(const LatLocDev& L, double qx, double qy, SlTri& out, double& bestd,
                                              float& rho2) {
  const int lane = threadIdx.x & 63;
  const int64_t gc = lat_gcell(L, qx, qy);
  const int32_t n = L.n;
  const double dn = (double)n;
  const int32_t e0 = L.start[gc], e1 = L.start[gc + 1];
  double md = INFINITY;
  int32_t mid = 0x7fffffff;
  SlTri mine{};
  for (int32_t base = e0; base < e1; base += 64) {
    const int32_t e = base + lane;
    bool inner = false, near = false;
    double u = 0.0, v = 0.0;
    int32_t fi = 0;
    if (e < e1) {
      fi = L.item[e];
      SlTri r;
      double d;
      if (sl_inner(L, L.face[fi], qx, qy, r, d, u, v)) {
        inner = true;
        if (knn_less(d, r.id, md, mid)) {
          md = d;
          mid = r.id;
          mine = r;
        }
      } else {
        near = u >= -SL_LDEL && v >= -SL_LDEL && u + v <= dn + SL_LDEL;
      }
    }
    if (__ballot(inner)) break;
    const uint64_t nm = __ballot(near);
    const int32_t ncand = 18 * __popcll(nm);
    bool stop = false;
    for (int32_t t0 = 0; t0 < ncand; t0 += 64) {
      const int32_t t = t0 + lane;
      int32_t fl = 0;  // the lane that holds candidate t's face: the (t / 18)-th near face
      if (t < ncand) {
        uint64_t m = nm;
        for (int32_t k = t / 18; k > 0; --k) m &= m - 1;
        fl = __ffsll((unsigned long long)m) - 1;
      }
      const double fu = __shfl(u, fl, 64), fv = __shfl(v, fl, 64);
      const int32_t ff = __shfl(fi, fl, 64);
      bool hit = false;
      if (t < ncand) {
        const int32_t c = t % 18;
        const int32_t i0 = min(max((int32_t)floor(fu), 0), n - 1), j0 = min(max((int32_t)floor(fv), 0), n - 1);
        const int32_t j = max(j0 - 1, 0) + c / 6, i = max(i0 - 1, 0) + (c / 2) % 3, s = c & 1;
        const double a = fu - i, b = fv - j;
        const bool cnear = !(j > j0 + 1 || i > i0 + 1 || i + j > n - 1) &&
                           (s == 0 ? (a >= -SL_LDEL && b >= -SL_LDEL && a + b <= 1.0 + SL_LDEL)
                                   : (i + j <= n - 2 && a <= 1.0 + SL_LDEL && b <= 1.0 + SL_LDEL && a + b >= 1.0 - SL_LDEL));
        if (cnear) {
          const SlTri r = sl_cell(L, L.face[ff], i, j, s);
          double d;
          bool margin;
          if (sl_test(r, qx, qy, d, margin)) {
            hit = margin;
            if (knn_less(d, r.id, md, mid)) {
              md = d;
              mid = r.id;
              mine = r;
            }
          }
        }
      }
      if (__ballot(hit)) {
        stop = true;
        break;
      }
    }
    if (stop) break;
  }
  // wave_bcast_tri, restated: k_sl_wq, which every step of the lattice locator runs, keeps its code
  // (profiles/sl_locate_shared.txt)
  double bd = md;
  int32_t bid = mid;
  wave_min_key(bd, bid);
  if (bid == 0x7fffffff) return false;
  const int src = __ffsll((unsigned long long)__ballot(md == bd && mid == bid)) - 1;
  out.x1 = __shfl(mine.x1, src, 64);
  out.y1 = __shfl(mine.y1, src, 64);
  out.x2 = __shfl(mine.x2, src, 64);
  out.y2 = __shfl(mine.y2, src, 64);
  out.x3 = __shfl(mine.x3, src, 64);
  out.y3 = __shfl(mine.y3, src, 64);
  out.a = __shfl(mine.a, src, 64);
  out.b = __shfl(mine.b, src, 64);
  out.d = __shfl(mine.d, src, 64);
  out.id = bid;
  bestd = bd;
  rho2 = L.rho2[bid];
  return true;
}
// Record locator (meshes without a red-refinement hierarchy: mesh.1, mesh_fine), whose k_sl has no fast path and
// queued every row for k_sl_slow's one lane per point: one wave per ROW instead, in one launch (k_sl_rec_wave), the
// records of q's grid cell tested by the lanes together (the passing record with the smallest (d^2, id) key, as
// sl_best's scan returns it) and the rank count as k_sl_wave's.  Same arithmetic per candidate: the same bits.
__device__ __forceinline__ bool sl_best_wave(const LocDev& L, double qx, double qy, SlTri& out, double& bestd,
                                             float& rho2) {
  const int lane = threadIdx.x & 63;
  const int32_t ci = gcell(qx, L.x0, L.hx, L.nx), cj = gcell(qy, L.y0, L.hy, L.ny);
  const int64_t cell = (int64_t)cj * L.nx + ci;
  const int32_t e0 = L.start[cell], e1 = L.start[cell + 1];
  double md = INFINITY;
  int32_t mid = 0x7fffffff, mpos = -1;
  SlTri mine{};
  for (int32_t base = e0; base < e1; base += 64) {  // (chunks until a margin pass, the only passing record then)
    const int32_t e = base + lane;
    bool hit = false;
    if (e < e1) {
      const int32_t pos = L.item[e];
      const SlTri r = sl_tri(L, pos);
      double d;
      bool margin;
      if (sl_test(r, qx, qy, d, margin)) {
        hit = margin;
        if (knn_less(d, r.id, md, mid)) {
          md = d;
          mid = r.id;
          mpos = pos;
          mine = r;
        }
      }
    }
    if (__ballot(hit)) break;
  }
  const int src = wave_bcast_tri(mine, md, mid, out, bestd);
  if (src < 0) return false;
  rho2 = L.rho2[__shfl(mpos, src, 64)];
  return true;
}

// ---- the locate sequences the kernels call (the account at the head of this file)
// the not-found output of a row that went through the general locate (probe bit 1: mark the slow rows)
template <class LOC>
__device__ __forceinline__ int32_t sl_mark(const LOC& L, bool ok) {
  return ok ? ((L.probe & 2) ? 2 : 0) : 1;
}
// one lane per point: the triangle PointLocator.find returns for (xb, yb), false when it returns none
template <class LOC>
__device__ __forceinline__ bool sl_locate_general(const LOC& L, const GridDev& G, double xb, double yb, SlTri& r) {
  double bestd;
  float rho2;
  return sl_best(L, -1, xb, yb, r, bestd, rho2) &&
         (sl_fast(L, r, xb, yb, bestd, rho2) || sl_rank_ok(G, xb, yb, bestd, r.id));
}
// one wave per point (every lane gets the answer), either locator.  (k_sl_wq spells the same sequence out with
// the faces-first sl_best_wave2: through this function it compiled to other code, profiles/sl_locate_shared.txt)
template <class LOC>
__device__ __forceinline__ bool sl_locate_wave(const LOC& L, const GridDev& G, double xb, double yb, SlTri& r) {
  double bestd;
  float rho2;
  return sl_best_wave(L, xb, yb, r, bestd, rho2) &&
         (sl_fast(L, r, xb, yb, bestd, rho2) || sl_rank_ok_wave(G, xb, yb, bestd, r.id));
}
// one lane per row g with velocity (vx, vy), (xb, yb) its back-traced point: the whole sequence of the one-pass
// kernels.  Lattice locator: a zero velocity makes q the row's own node (no-slip walls), on lattice lines where
// several triangles pass the weight test -- the answer settled once at build (k_sl_self), as k_sl reads it; then the
// fast path's two stages, so that the rows k_sl finishes cheaply do not pay the general search; else, and for the
// record locator, the general locate, which returns the fast path's triangle where both answer.  mark: the row's
// not-found output.
template <class LOC>
__device__ __forceinline__ bool sl_locate_row(const MeshDev& M, const LOC& L, const GridDev& G, int64_t g, double vx,
                                              double vy, double xb, double yb, SlTri& r, int32_t& mark) {
  if constexpr (std::is_same<LOC, LatLocDev>::value) {
    if (vx == 0.0 && vy == 0.0 && L.self) {
      const int32_t t = L.self[g];
      if (t >= 0) {
        const int32_t va = M.tri[3 * (int64_t)t], vb = M.tri[3 * (int64_t)t + 1], vc = M.tri[3 * (int64_t)t + 2];
        r = SlTri{M.x[va], M.y[va], M.x[vb], M.y[vb], M.x[vc], M.y[vc], va, vb, vc, t};
      }
      mark = t >= 0 ? 0 : 1;
      return t >= 0;
    }
    int32_t v0, v1, v2, id;
    if (sl_lat_cell(L, L.home[g], xb, yb, v0, v1, v2, id)) {
      const double2 P1 = L.xy[v0], P2 = L.xy[v1], P3 = L.xy[v2];
      const float rho2 = L.rho2[id], rv1 = L.rv2[v0], rv2 = L.rv2[v1], rv3 = L.rv2[v2];
      double unused;  // (the stage's own value of a zero field: the caller interpolates its fields)
      if (sl_lat_value(L.probe, xb, yb, P1, P2, P3, 0.0, 0.0, 0.0, rho2, rv1, rv2, rv3, unused)) {
        r = SlTri{P1.x, P1.y, P2.x, P2.y, P3.x, P3.y, v0, v1, v2, id};
        mark = 0;
        return true;
      }
    }
  }
  const bool ok = sl_locate_general(L, G, xb, yb, r);
  mark = sl_mark(L, ok);
  return ok;
}
// one wave per row g with velocity (vx, vy): back-trace, sl_locate_wave, and the new value of the field f (plain
// values or interleaved pairs) in every lane -- the row's own when no triangle is accepted (false)
template <class LOC, class F>
__device__ __forceinline__ bool sl_row_wave(const MeshDev& M, const LOC& L, const GridDev& G, int64_t g, double vx,
                                            double vy, double dt, const F* f, F& fn) {
  double xb, yb;
  sl_point(M, g, vx, vy, dt, xb, yb);
  SlTri r;
  const bool ok = sl_locate_wave(L, G, xb, yb, r);
  fn = ok ? sl_value(r, xb, yb, f) : f[g];
  return ok;
}

}  // namespace dev
}  // namespace pucfem
