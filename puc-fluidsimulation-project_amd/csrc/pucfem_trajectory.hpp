// Midpoint trajectories (pucfem_set_trajectory, pucfem_sl_advect_traj, pucfem_sl_advect_vel_traj, include/pucfem.h,
// DESIGN.md section 27): the second-order back-trace of the semi-Lagrangian rows.  Per row g with velocity v = u[g]
//
//   (xm, ym) = sl_point(X_g, v, hdt)                       half a step along v          (hdt = 0.5 * dt, from the host)
//   w        = found ? sl_value(Tm, (xm, ym), u) : v       the velocity read there, else the row's own (an Euler row)
//   (xb, yb) = sl_point(X_g, w, dt)                        the whole step along w
//   value    = found ? sl_value(T, (xb, yb), field) : field[g]
//
// Both locates are sl_locate_row (pucfem_locate.hpp); the second is keyed on w, so the zero-velocity table
// (LatLocDev::self) answers where w is zero.  The fused row is the composition of two first-order launches,
// W = k_sl_vel(f = u, u, hdt) and then k_sl_multi / k_sl_vel / k_mc_* with W in place of u, expression for
// expression (the library is built with -ffp-contract=off): it holds that composition's bits
// (tests/test_gpu_trajectory.py).  w lives in registers and is never written to memory: that, and the saved launch, is
// what the fused kernel buys.
//
// u is the full mesh's interleaved pairs (single-rank contexts: the rows of a launch are rows of u).  The kernels are
// new ones beside k_sl_multi / k_sl_vel / k_mc_*: the instantiations an Euler step launches are untouched.
// Ensemble members run the wave-per-row forms of these kernels, k_ens_trj_fwd / k_ens_trj_bwd (pucfem_ensemble.hpp,
// DESIGN.md section 28), whose two phases are trj_locate's loop with sl_locate_wave in sl_locate_row's place.
#pragma once
#include "pucfem_maccormack.hpp"

namespace pucfem {
namespace dev {

// marks of the trajectory kernels, per row: bits 0 and 1 are MC_NO_BACK / MC_NO_FWD (of the final locates)
constexpr int32_t TRJ_NO_MID1 = 4;  // bit 2: pass 1's midpoint found no triangle: the pass traced along u[g]
constexpr int32_t TRJ_NO_MID2 = 8;  // bit 3: pass 2's (MacCormack only)

// The two locates of a row, as ONE loop body run twice (not unrolled): phase 0 traces half a step along (vx, vy),
// locates the midpoint and reads u there; phase 1 traces the whole step along that velocity and locates the final
// point.  A single inlined copy of sl_locate_row and a single SlTri: the registers of a one-pass kernel, no scratch
// (two inlined copies, each with its own triangle, left 72 bytes per lane in scratch memory).  In: (vx, vy) = u[g];
// out: (vx, vy) the velocity the row was traced with, (xb, yb) and r the final point and its triangle (when the
// result is true), okm whether the midpoint was found.
template <class LOC>
__device__ __forceinline__ bool trj_locate(const MeshDev& M, const LOC& L, const GridDev& G, int64_t g, double& vx,
                                           double& vy, double dt, double hdt, const dbl2* u, double& xb, double& yb,
                                           SlTri& r, bool& okm) {
  bool ok = false;
  okm = true;
#pragma unroll 1
  for (int ph = 0; ph < 2; ++ph) {
    sl_point(M, g, vx, vy, ph == 0 ? hdt : dt, xb, yb);
    int32_t mark;
    ok = sl_locate_row(M, L, G, g, vx, vy, xb, yb, r, mark);
    if (ph == 0) {
      okm = ok;
      if (ok) {
        const dbl2 w = sl_value(r, xb, yb, u);
        vx = w.x;
        vy = w.y;
      }
    }
  }
  return ok;
}

// pass 1's counts of a block: nfpart[block] the rows whose final locate found nothing (k_mc_fwd's; nfd, or null: the
// same as a double, for the step record's reduction), mid[block] those whose midpoint was not found
__device__ __forceinline__ void trj_counts(int32_t nnf, int32_t nmid, double* sh, int32_t* __restrict__ nfpart,
                                           double* __restrict__ nfd, int32_t* __restrict__ mid) {
  const double a = block_sum((double)nnf, sh), b = block_sum((double)nmid, sh);
  if (threadIdx.x == 0) {
    nfpart[blockIdx.x] = (int32_t)a;
    if (nfd) nfd[blockIdx.x] = a;
    mid[blockIdx.x] = (int32_t)b;
  }
}
// pass 2's: k_mc_bwd's three counts per block, and mid[block]
__device__ __forceinline__ void trj_counts2(int32_t nb1, int32_t nb2, int32_t ncl, int32_t nmid, double* sh,
                                            int32_t* __restrict__ cnt, int32_t* __restrict__ mid) {
  const double a = block_sum((double)nb1, sh), b = block_sum((double)nb2, sh), d = block_sum((double)ncl, sh),
               e = block_sum((double)nmid, sh);
  if (threadIdx.x == 0) {
    cnt[3 * blockIdx.x] = (int32_t)a;
    cnt[3 * blockIdx.x + 1] = (int32_t)b;
    cnt[3 * blockIdx.x + 2] = (int32_t)d;
    mid[blockIdx.x] = (int32_t)e;
  }
}

// pass 1 (and the whole of a one-pass step), plain fields: k_mc_fwd's arguments with u as pairs; rec (or null) the
// row's final triangle, marks (n, or null) bits 0 and 2
template <class LOC>
__global__ __launch_bounds__(BS) void k_trj_fwd(MeshDev M, LOC L, GridDev G, int64_t row0, int64_t n,
                                                const dbl2* __restrict__ u, double dt, double hdt,
                                                const double* __restrict__ c0, double* __restrict__ ch0, int32_t nch,
                                                const double* __restrict__ cin, double* __restrict__ chout, int64_t ld,
                                                int4* __restrict__ rec, int32_t* __restrict__ marks,
                                                int32_t* __restrict__ nfpart, double* __restrict__ nfd,
                                                int32_t* __restrict__ mid) {
  __shared__ double sh[4];
  int32_t nnf = 0, nmid = 0;
  int64_t r0, r1;
  block_rows(n, r0, r1);
  for (int64_t i = r0 + threadIdx.x; i < r1; i += BS) {
    const int64_t g = row0 + i;
    const dbl2 v = u[g];
    double wx = v.x, wy = v.y, xb, yb;
    SlTri r{};
    bool okm;
    const bool ok = trj_locate(M, L, G, g, wx, wy, dt, hdt, u, xb, yb, r, okm);
    if (!ok) ++nnf;
    if (!okm) ++nmid;
    if (rec) rec[i] = ok ? make_int4(r.a, r.b, r.d, r.id) : make_int4(0, 0, 0, -1);
    if (marks) marks[i] = (ok ? 0 : MC_NO_BACK) | (okm ? 0 : TRJ_NO_MID1);
    if (c0) stnt(ch0 + g, ok ? sl_value(r, xb, yb, c0) : c0[g]);
    for (int32_t k = 0; k < nch; ++k) {
      const double* __restrict__ c = cin + (int64_t)k * ld;
      stnt(chout + (int64_t)k * ld + g, ok ? sl_value(r, xb, yb, c) : c[g]);
    }
  }
  trj_counts(nnf, nmid, sh, nfpart, nfd, mid);
}

// pass 2, plain fields: k_mc_bwd's arguments; the midpoint is read from u with -hdt, the value from ch with -dt (the
// host passes dt and hdt, the kernel negates: k_mc_bwd's convention).  marks (or null): pass 1's bits 0 and 2 are in
// it, this pass adds bits 1 and 3.  cnt: k_mc_bwd's three counts per block; mid[block]: the rows whose pass-2
// midpoint was not found.  Three waves per SIMD asked for: the lattice instantiation fits (167 VGPRs, no scratch) and
// its launch at L7 went from 1.52 to 1.24 ms; k_trj_fwd's spills under the same bound and keeps two (DESIGN.md
// section 27).
template <class LOC>
__global__ __launch_bounds__(BS, 3) void k_trj_bwd(MeshDev M, LOC L, GridDev G, int64_t row0, int64_t n,
                                                const dbl2* __restrict__ u, double dt, double hdt,
                                                const double* __restrict__ c0, const double* __restrict__ ch0,
                                                double* __restrict__ out0, int32_t nch, const double* __restrict__ cin,
                                                const double* __restrict__ ch, double* __restrict__ cout, int64_t ld,
                                                const int4* __restrict__ rec, int32_t* __restrict__ marks,
                                                int32_t* __restrict__ tri, int32_t* __restrict__ cnt,
                                                int32_t* __restrict__ mid) {
  __shared__ double sh[4];
  int32_t nb1 = 0, nb2 = 0, ncl = 0, nmid = 0;
  int64_t r0, r1;
  block_rows(n, r0, r1);
  for (int64_t i = r0 + threadIdx.x; i < r1; i += BS) {
    const int64_t g = row0 + i;
    const dbl2 v = u[g];
    double wx = v.x, wy = v.y, xb, yb;
    SlTri r{};
    bool okm;
    const bool ok2 = trj_locate(M, L, G, g, wx, wy, -dt, -hdt, u, xb, yb, r, okm);
    const int4 t = rec[i];
    if (t.w < 0) ++nb1;
    if (!ok2) ++nb2;
    if (!okm) ++nmid;
    if (marks) marks[i] = marks[i] | (ok2 ? 0 : MC_NO_FWD) | (okm ? 0 : TRJ_NO_MID2);
    if (tri) tri[i] = t.w;
    if (c0) stnt(out0 + g, mc_row(t, ok2, r, xb, yb, g, c0, ch0, ncl));
    for (int32_t k = 0; k < nch; ++k)
      stnt(cout + (int64_t)k * ld + g, mc_row(t, ok2, r, xb, yb, g, cin + (int64_t)k * ld, ch + (int64_t)k * ld, ncl));
  }
  trj_counts2(nb1, nb2, ncl, nmid, sh, cnt, mid);
}

// pass 1 (and the whole of a one-pass step), interleaved pairs: ch[g] from f (f may be u; ch aliases neither)
template <class LOC>
__global__ __launch_bounds__(BS) void k_trj_fwd_vel(MeshDev M, LOC L, GridDev G, int64_t row0, int64_t n,
                                                    const dbl2* u, double dt, double hdt, const dbl2* f,
                                                    dbl2* __restrict__ ch, int4* __restrict__ rec,
                                                    int32_t* __restrict__ marks, int32_t* __restrict__ nfpart,
                                                    int32_t* __restrict__ mid) {
  __shared__ double sh[4];
  int32_t nnf = 0, nmid = 0;
  int64_t r0, r1;
  block_rows(n, r0, r1);
  for (int64_t i = r0 + threadIdx.x; i < r1; i += BS) {
    const int64_t g = row0 + i;
    const dbl2 v = u[g];
    double wx = v.x, wy = v.y, xb, yb;
    SlTri r{};
    bool okm;
    const bool ok = trj_locate(M, L, G, g, wx, wy, dt, hdt, u, xb, yb, r, okm);
    if (!ok) ++nnf;
    if (!okm) ++nmid;
    if (rec) rec[i] = ok ? make_int4(r.a, r.b, r.d, r.id) : make_int4(0, 0, 0, -1);
    if (marks) marks[i] = (ok ? 0 : MC_NO_BACK) | (okm ? 0 : TRJ_NO_MID1);
    stnt(ch + g, ok ? sl_value(r, xb, yb, f) : f[g]);
  }
  trj_counts(nnf, nmid, sh, nfpart, nullptr, mid);
}

// pass 2, interleaved pairs (k_mc_bwd_vel's arguments; marks and cnt as k_trj_bwd's)
template <class LOC>
__global__ __launch_bounds__(BS) void k_trj_bwd_vel(MeshDev M, LOC L, GridDev G, int64_t row0, int64_t n,
                                                    const dbl2* u, double dt, double hdt, const dbl2* f,
                                                    const dbl2* ch, dbl2* __restrict__ out,
                                                    const int4* __restrict__ rec, int32_t* __restrict__ marks,
                                                    int32_t* __restrict__ tri, int32_t* __restrict__ cnt,
                                                int32_t* __restrict__ mid) {
  __shared__ double sh[4];
  int32_t nb1 = 0, nb2 = 0, ncl = 0, nmid = 0;
  int64_t r0, r1;
  block_rows(n, r0, r1);
  for (int64_t i = r0 + threadIdx.x; i < r1; i += BS) {
    const int64_t g = row0 + i;
    const dbl2 v = u[g];
    double wx = v.x, wy = v.y, xb, yb;
    SlTri r{};
    bool okm;
    const bool ok2 = trj_locate(M, L, G, g, wx, wy, -dt, -hdt, u, xb, yb, r, okm);
    const int4 t = rec[i];
    if (t.w < 0) ++nb1;
    if (!ok2) ++nb2;
    if (!okm) ++nmid;
    if (marks) marks[i] = marks[i] | (ok2 ? 0 : MC_NO_FWD) | (okm ? 0 : TRJ_NO_MID2);
    if (tri) tri[i] = t.w;
    stnt(out + g, mc_row(t, ok2, r, xb, yb, g, f, ch, ncl));
  }
  trj_counts2(nb1, nb2, ncl, nmid, sh, cnt, mid);
}

}  // namespace dev
}  // namespace pucfem
