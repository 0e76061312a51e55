// Body forces (pucfem_set_force, pucfem_set_buoyancy, include/pucfem.h): the viscous right-hand side
// r = base + DT * b_force of the reference (StokesColor.py:485-486, 540-541, StokesFood.py:405-406, 444-445), with
// b_force a uniform vector, a nodal field, a Boussinesq buoyancy of the dye, or their sum:
//
//   f = (0, 0)
//   uniform F:   f = F
//   nodal fn:    f = f + fn[i]                      (no F: f = fn[i])
//   buoyancy:    b = beta_0 * (s_0[i] - ref_0);  b = b + beta_t * (s_t[i] - ref_t), t = 1 .. nterms - 1
//                f = (f.x + g.x * b, f.y + g.y * b)
//   r[i] = (base[i].x + dt * f.x, base[i].y + dt * f.y)
//
// every product and sum as written (the build has -ffp-contract=off), terms that are absent skipped and not added as
// zeros: a numpy line per term gives the same bits (tests/force_reference.py).
//
// One element-wise pass over the owned rows: base as one 16-byte pair, fn as one 16-byte pair, each s_t as 8 bytes,
// r as one 16-byte non-temporal store.  The term list travels by value (no device array: nothing to upload when a
// setting changes).
#pragma once
#include "pucfem_kernels_impl.hpp"

namespace pucfem {
namespace dev {

constexpr int FORCE_MAX_TERMS = 17;  // c and PUCFEM_MAX_DYES channels

struct ForceTerms {
  double fx, fy;                     // the uniform force
  double gx, gy;                     // the buoyancy direction (with its magnitude)
  const double* s[FORCE_MAX_TERMS];  // the dye fields, at the launch's first row
  double beta[FORCE_MAX_TERMS], ref[FORCE_MAX_TERMS];
  int32_t nterms;
};

// the total force of row i, in the order of the definition; s[t][i], beta[t], ref[t]: the buoyancy terms.  The flags
// are compile-time constants in k_force_rhs and block-uniform values in k_ens_force_rhs: one body, the same bits
__device__ __forceinline__ dbl2 force_row(bool uni, bool nod, bool buo, int64_t i, double Fx, double Fy,
                                          const dbl2* __restrict__ fn, double gx, double gy, int nterms,
                                          const double* const* s, const double* beta, const double* ref) {
  double fx = 0.0, fy = 0.0;
  if (uni) {
    fx = Fx;
    fy = Fy;
  }
  if (nod) {
    const dbl2 v = fn[i];
    if (uni) {
      fx = fx + v.x;
      fy = fy + v.y;
    } else {
      fx = v.x;
      fy = v.y;
    }
  }
  if (buo) {
    double b = beta[0] * (s[0][i] - ref[0]);
    for (int t = 1; t < nterms; ++t) b = b + beta[t] * (s[t][i] - ref[t]);
    fx = fx + gx * b;
    fy = fy + gy * b;
  }
  return dbl2{fx, fy};
}

// rows [0, n): RHS: r[i] = base[i] + dt * f[i]; else r[i] = f[i] (PUCFEM_F_FORCE, formed when read; base unused)
template <bool UNI, bool NOD, bool BUO, bool RHS>
__global__ __launch_bounds__(BS) void k_force_rhs(int64_t n, const dbl2* __restrict__ base, double dt,
                                                  const dbl2* __restrict__ fn, ForceTerms T, dbl2* __restrict__ r) {
  for (int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x; i < n; i += (int64_t)gridDim.x * BS) {
    const dbl2 f = force_row(UNI, NOD, BUO, i, T.fx, T.fy, fn, T.gx, T.gy, T.nterms, T.s, T.beta, T.ref);
    if constexpr (RHS) {
      const dbl2 u = base[i];
      stnt(r + i, dbl2{u.x + dt * f.x, u.y + dt * f.y});
    } else {
      stnt(r + i, f);
    }
  }
}

// The same per ensemble member (pucfem_ens_set_force, pucfem_ens_set_buoyancy): the member is blockIdx.y, the grid in x
// the single path's.  mask[m]: the member's terms (1 uniform, 2 nodal, 4 buoyancy; 0: the member is not written);
// parm: ENS_FORCE_PARM doubles per member (Fx, Fy, gx, gy, beta, ref -- members have c only); fnod: the members' nodal
// planes (M x 2n, or null while no member has one); u, ua, c, r: M x 2n, M x 2n, M x n, M x 2n.  A member whose
// inertia flag is on (advon non-null) takes its plane of ua as base.  RHS false: the member's f itself, for every
// member (PUCFEM_F_FORCE; an unforced member's plane is zeros).
constexpr int ENS_FORCE_PARM = 8;
template <bool RHS>
__global__ __launch_bounds__(BS) void k_ens_force_rhs(int64_t n, const int32_t* __restrict__ mask,
                                                      const double* __restrict__ parm, const dbl2* __restrict__ fnod,
                                                      const dbl2* __restrict__ u, const dbl2* __restrict__ ua,
                                                      const int32_t* __restrict__ advon, const double* __restrict__ c,
                                                      double dt, dbl2* __restrict__ r) {
  const int64_t m = blockIdx.y;
  const int32_t k = mask[m];
  if (RHS && k == 0) return;
  const double* q = parm + m * ENS_FORCE_PARM;
  const double Fx = q[0], Fy = q[1], gx = q[2], gy = q[3];
  const double beta[1] = {q[4]}, ref[1] = {q[5]};
  const double* s[1] = {c + m * n};
  const dbl2* fn = fnod ? fnod + m * n : nullptr;
  const dbl2* base = (advon && advon[m] ? ua : u) + m * n;
  dbl2* out = r + m * n;
  for (int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x; i < n; i += (int64_t)gridDim.x * BS) {
    const dbl2 f = force_row((k & 1) != 0, (k & 2) != 0, (k & 4) != 0, i, Fx, Fy, fn, gx, gy, 1, s, beta, ref);
    if constexpr (RHS) {
      const dbl2 b = base[i];
      stnt(out + i, dbl2{b.x + dt * f.x, b.y + dt * f.y});
    } else {
      stnt(out + i, f);
    }
  }
}

}  // namespace dev
}  // namespace pucfem
