// MacCormack advection (pucfem_set_advection, pucfem_sl_advect_mc, pucfem_sl_advect_vel_mc, include/pucfem.h): the
// unconditionally stable second-order scheme of Selle et al. (J. Sci. Comput. 35, 2008) on the semi-Lagrangian step
// advect_semilagrange (StokesColor.py:347-389) -- two advections and a clamp.
//
//   pass 1   ch = SL(c; u, +dt): the first-order step, and per row the triangle T1 its locate returned (16 B: the
//            vertex ids a, b, d and the mesh's triangle id, -1 when none was accepted), whatever the number of fields
//   pass 2   cb = SL(ch; u, -dt): the step run backwards from the same node; the error estimate
//            e = ch + 0.5 * (c - cb), clamped into [min, max] of c at T1's vertices -- the values the first-order
//            result is a convex combination of, so the limited result stays within the field's range
// A row whose back-trace found no triangle keeps c (as the first-order step does); one whose forward trace found
// none keeps ch: the scheme falls back to first order there.
//
// Pass 2 gathers ch at the vertices of other rows' triangles: it is a second launch, not a grid barrier, and its
// output may alias neither c nor ch (rows of other blocks still gather from both) -- three sets of fields.
//
// The locates are sl_locate_row (pucfem_locate.hpp), one lane per row, blocks over rows as k_sl_multi's; one velocity
// serves both passes, and a zero velocity makes both departure points the row's own node (LatLocDev::self).  Every
// field's ch and cb are sl_value on those triangles: the expressions of the single-dye kernels (the library is built
// with -ffp-contract=off), so ch holds the bits of pucfem_sl_advect(c, u, dt) and cb those of
// pucfem_sl_advect(ch, u, -dt) (tests/test_gpu_maccormack.py).
//
// Two forms of each pass: channel-major plain fields (k_sl_multi's layout; c is one extra field pointer, so that c and
// the dye channels share one locate per pass and row) and one field of interleaved pairs (k_sl_vel's).
#pragma once
#include "pucfem_kernels_impl.hpp"

namespace pucfem {
namespace dev {

// marks of pass 2, per row
constexpr int32_t MC_NO_BACK = 1;  // bit 0: the back-trace (pass 1) found no triangle: the row keeps c
constexpr int32_t MC_NO_FWD = 2;   // bit 1: the forward trace (pass 2) found none: the row keeps ch (c with bit 0)

// e clamped into [lo, hi] of (fa, fb, fd), the comparisons as written in DESIGN section 22; hit: e was outside
__device__ __forceinline__ double mc_limit(double e, double fa, double fb, double fd, bool& hit) {
  double lo = fa, hi = fa;
  if (fb < lo) lo = fb;
  if (fd < lo) lo = fd;
  if (fb > hi) hi = fb;
  if (fd > hi) hi = fd;
  hit = e < lo || e > hi;
  return e < lo ? lo : (e > hi ? hi : e);
}

// pass 1, plain fields, rows [row0, row0 + n): ch0[g] from c0 (null: no extra field) and chout[k * ld + g] from
// cin + k * ld for k < nch; rec[i] the row's T1; nfpart[block]: the block's not-found rows (nfd, or null: the same
// as a double, for the step record's reduction)
template <class LOC>
__global__ __launch_bounds__(BS) void k_mc_fwd(MeshDev M, LOC L, GridDev G, int64_t row0, int64_t n,
                                               const double* __restrict__ ux, const double* __restrict__ uy, double dt,
                                               const double* __restrict__ c0, double* __restrict__ ch0, int32_t nch,
                                               const double* __restrict__ cin, double* __restrict__ chout, int64_t ld,
                                               int4* __restrict__ rec, int32_t* __restrict__ nfpart,
                                               double* __restrict__ nfd) {
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
    rec[i] = ok ? make_int4(r.a, r.b, r.d, r.id) : make_int4(0, 0, 0, -1);
    if (c0) stnt(ch0 + g, ok ? sl_value(r, xb, yb, c0) : c0[g]);
    for (int32_t k = 0; k < nch; ++k) {
      const double* __restrict__ c = cin + (int64_t)k * ld;
      stnt(chout + (int64_t)k * ld + g, ok ? sl_value(r, xb, yb, c) : c[g]);
    }
  }
  const double d = block_sum(nnf, sh);
  if (threadIdx.x == 0) {
    nfpart[blockIdx.x] = (int32_t)d;
    if (nfd) nfd[blockIdx.x] = d;
  }
}

// one field of pass 2 at row g: T1 = t (t.w < 0: none), T2 = r (ok2), (xb, yb) the forward-traced point
__device__ __forceinline__ double mc_row(const int4 t, bool ok2, const SlTri& r, double xb, double yb, int64_t g,
                                         const double* __restrict__ c, const double* __restrict__ ch, int32_t& nclamp) {
  if (t.w < 0) return c[g];
  const double chg = ch[g];
  if (!ok2) return chg;
  const double cb = sl_value(r, xb, yb, ch);
  const double e = chg + 0.5 * (c[g] - cb);
  bool hit;
  const double v = mc_limit(e, c[t.x], c[t.y], c[t.z], hit);
  if (hit) ++nclamp;
  return v;
}

// ... of a field of interleaved pairs: the two components limited separately (each in the plain form's expression
// order: component k holds the bits of the plain form on that component); every clamped component counts
__device__ __forceinline__ dbl2 mc_row(const int4 t, bool ok2, const SlTri& r, double xb, double yb, int64_t g,
                                       const dbl2* f, const dbl2* ch, int32_t& nclamp) {
  dbl2 o = f[g];
  if (t.w >= 0) {
    const dbl2 chg = ch[g];
    if (!ok2) {
      o = chg;
    } else {
      const dbl2 cb = sl_value(r, xb, yb, ch);
      const dbl2 fa = f[t.x], fb = f[t.y], fd = f[t.z];
      bool hx, hy;
      const double ex = chg.x + 0.5 * (o.x - cb.x), ey = chg.y + 0.5 * (o.y - cb.y);
      o.x = mc_limit(ex, fa.x, fb.x, fd.x, hx);
      o.y = mc_limit(ey, fa.y, fb.y, fd.y, hy);
      if (hx) ++nclamp;
      if (hy) ++nclamp;
    }
  }
  return o;
}

// pass 2, plain fields: out0 / cout from (c0, ch0) / (cin, ch) and pass 1's rec; marks, tri (n each, or null): the
// row's MC_* bits and T1's mesh triangle id (-1); cnt[3 * block + (0, 1, 2)]: the block's rows without T1, rows
// without T2, clamped values (every field counts)
template <class LOC>
__global__ __launch_bounds__(BS) void k_mc_bwd(MeshDev M, LOC L, GridDev G, int64_t row0, int64_t n,
                                               const double* __restrict__ ux, const double* __restrict__ uy, double dt,
                                               const double* __restrict__ c0, const double* __restrict__ ch0,
                                               double* __restrict__ out0, int32_t nch, const double* __restrict__ cin,
                                               const double* __restrict__ ch, double* __restrict__ cout, int64_t ld,
                                               const int4* __restrict__ rec, int32_t* __restrict__ marks,
                                               int32_t* __restrict__ tri, int32_t* __restrict__ cnt) {
  __shared__ double sh[4];
  int32_t nb1 = 0, nb2 = 0, ncl = 0;  // (a lane's counts: integers, three registers)
  int64_t r0, r1;
  block_rows(n, r0, r1);
  for (int64_t i = r0 + threadIdx.x; i < r1; i += BS) {
    const int64_t g = row0 + i;
    const double vx = ux[VS * i], vy = uy[VS * i];
    double xb, yb;
    sl_point(M, g, vx, vy, -dt, xb, yb);
    SlTri r{};
    int32_t mark;
    const bool ok2 = sl_locate_row(M, L, G, g, vx, vy, xb, yb, r, mark);
    const int4 t = rec[i];
    if (t.w < 0) ++nb1;
    if (!ok2) ++nb2;
    if (marks) marks[i] = (t.w < 0 ? MC_NO_BACK : 0) | (ok2 ? 0 : MC_NO_FWD);
    if (tri) tri[i] = t.w;
    if (c0) stnt(out0 + g, mc_row(t, ok2, r, xb, yb, g, c0, ch0, ncl));
    for (int32_t k = 0; k < nch; ++k)
      stnt(cout + (int64_t)k * ld + g, mc_row(t, ok2, r, xb, yb, g, cin + (int64_t)k * ld, ch + (int64_t)k * ld, ncl));
  }
  const double a = block_sum((double)nb1, sh), b = block_sum((double)nb2, sh), d = block_sum((double)ncl, sh);
  if (threadIdx.x == 0) {
    cnt[3 * blockIdx.x] = (int32_t)a;
    cnt[3 * blockIdx.x + 1] = (int32_t)b;
    cnt[3 * blockIdx.x + 2] = (int32_t)d;
  }
}

// pass 1, interleaved pairs: ch[g] = SL(f; u, dt)[g]; f and ch hold the pairs of every mesh node, u those of the rows
// of this launch (f may be u); ch must not alias f
template <class LOC>
__global__ __launch_bounds__(BS) void k_mc_fwd_vel(MeshDev M, LOC L, GridDev G, int64_t row0, int64_t n, const dbl2* u,
                                                   double dt, const dbl2* f, dbl2* __restrict__ ch,
                                                   int4* __restrict__ rec, int32_t* __restrict__ nfpart) {
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
    rec[i] = ok ? make_int4(r.a, r.b, r.d, r.id) : make_int4(0, 0, 0, -1);
    stnt(ch + g, ok ? sl_value(r, xb, yb, f) : f[g]);
  }
  const double d = block_sum(nnf, sh);
  if (threadIdx.x == 0) nfpart[blockIdx.x] = (int32_t)d;
}

// pass 2, interleaved pairs: out from (f, ch) and rec, the two components limited separately (each in mc_row's
// expression order: component k holds the bits of the plain form on that component); out aliases neither f nor ch
template <class LOC>
__global__ __launch_bounds__(BS) void k_mc_bwd_vel(MeshDev M, LOC L, GridDev G, int64_t row0, int64_t n, const dbl2* u,
                                                   double dt, const dbl2* f, const dbl2* ch, dbl2* __restrict__ out,
                                                   const int4* __restrict__ rec, int32_t* __restrict__ marks,
                                                   int32_t* __restrict__ tri, int32_t* __restrict__ cnt) {
  __shared__ double sh[4];
  int32_t nb1 = 0, nb2 = 0, ncl = 0;  // (a lane's counts: integers, three registers)
  int64_t r0, r1;
  block_rows(n, r0, r1);
  for (int64_t i = r0 + threadIdx.x; i < r1; i += BS) {
    const int64_t g = row0 + i;
    const dbl2 v = u[i];
    double xb, yb;
    sl_point(M, g, v.x, v.y, -dt, xb, yb);
    SlTri r{};
    int32_t mark;
    const bool ok2 = sl_locate_row(M, L, G, g, v.x, v.y, xb, yb, r, mark);
    const int4 t = rec[i];
    if (t.w < 0) ++nb1;
    if (!ok2) ++nb2;
    if (marks) marks[i] = (t.w < 0 ? MC_NO_BACK : 0) | (ok2 ? 0 : MC_NO_FWD);
    if (tri) tri[i] = t.w;
    stnt(out + g, mc_row(t, ok2, r, xb, yb, g, f, ch, ncl));
  }
  const double a = block_sum((double)nb1, sh), b = block_sum((double)nb2, sh), d = block_sum((double)ncl, sh);
  if (threadIdx.x == 0) {
    cnt[3 * blockIdx.x] = (int32_t)a;
    cnt[3 * blockIdx.x + 1] = (int32_t)b;
    cnt[3 * blockIdx.x + 2] = (int32_t)d;
  }
}

}  // namespace dev
}  // namespace pucfem
