// Brownian tracers: a random walk per tracer and per tracer step with diffusivity D on top of
// the deterministic move, pucfem_set_tracer_diffusion / pucfem_ens_set_tracer_diffusion.
//
//   r0..r3 = Philox4x32-10(counter = (k, stepno, 0, 0), key = (seed low, seed high))
//   U1, U2 = 53-bit uniforms in [0, 1) from (r0, r1) and (r2, r3)
//   n      = (p + v dt) + a (2 U - 1),  a = sqrt(6 D dt)   (uniform on [-a, a]: variance 2 D dt per coordinate)
//   x mod 1, one reflection of y at the walls ylo / yhi, store, then tracer_move's capture test
//
// The stream depends on (seed, k, stepno) only: not on the kernel form, the grid, the member or the launch count, so
// every kernel form gives the same bits and two ensemble members with one seed draw the same increments.  No
// transcendental function is used: a numpy restatement holds the bits (tests/brownian_reference.py).  A tracer whose
// status is 1 when its step starts is absorbed food: the kernels neither load nor store its position (the freeze
// belongs to D > 0 only: with D = 0 the kernels run tracer_move, the plain step).
#pragma once
#include <cstdint>
#include <type_traits>

#include <hip/hip_runtime.h>

#include "pucfem_kernels.hpp"

namespace pucfem {
namespace dev {

// the single path's setting, by value in the kernel arguments (a = 0 never reaches a BROWN kernel there)
struct Brown {
  double a;          // sqrt(6 D dt), from the host
  uint32_t k0, k1;   // the Philox key: seed low, seed high
  double ylo, yhi;   // the walls: the mesh's smallest and largest node y
};
struct BrownOff {};  // the plain kernels' (empty) argument
template <bool BROWN>
using BrownArg = std::conditional_t<BROWN, Brown, BrownOff>;
// the members' settings in device memory (a[m], key[m]): read with m = blockIdx.y, a[m] == 0 is the plain move
struct EnsBrown {
  const double* a;
  const uint2* key;
  double ylo, yhi;
};
struct EnsBrownOff {};
template <bool BROWN>
using EnsBrownArg = std::conditional_t<BROWN, EnsBrown, EnsBrownOff>;

// Philox4x32-10 (Salmon et al., SC'11): ten rounds of two 32 x 32 -> 64 multiplies, the key bumped between rounds.
// ~100 integer operations in registers: no table, no LDS.
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                              uint32_t k1, uint32_t (&r)[4]) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint32_t hi0 = __umulhi(M0, c0), lo0 = M0 * c0;
    const uint32_t hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0;
    c1 = lo1;
    c2 = n2;
    c3 = lo0;
    k0 += W0;
    k1 += W1;
  }
  r[0] = c0;
  r[1] = c1;
  r[2] = c2;
  r[3] = c3;
}
// 53 random bits (27 of hi, 26 of lo) as a double in [0, 1): every step exact
__device__ __forceinline__ double brown_uniform(uint32_t hi, uint32_t lo) {
  return ((double)(hi >> 5) * 67108864.0 + (double)(lo >> 6)) * (1.0 / 9007199254740992.0);
}

// tracer_move with the random increment, for a free tracer (status != 1 at the start of the step; the caller has
// counted 1.0 for an absorbed one): forward Euler plus the increment, x mod 1, one reflection at the walls, then
// tracer_move's capture test.  NaN (a tracer outside the mesh) fails both wall comparisons and stays NaN.
__device__ __forceinline__ double tracer_move_brownian(double* tx, double* ty, double* status, int32_t* capstep,
                                                       int32_t k, double px, double py, double vx, double vy,
                                                       double dt, double cx, double cy, double capture,
                                                       int32_t stepno, const Brown& b) {
  uint32_t r[4];
  philox4x32_10((uint32_t)k, (uint32_t)stepno, 0u, 0u, b.k0, b.k1, r);
  const double u1 = brown_uniform(r[0], r[1]), u2 = brown_uniform(r[2], r[3]);
  double nx_ = (px + vx * dt) + b.a * (2.0 * u1 - 1.0);
  double ny_ = (py + vy * dt) + b.a * (2.0 * u2 - 1.0);
  nx_ = py_mod(nx_, 1.0);
  if (ny_ < b.ylo) ny_ = b.ylo + (b.ylo - ny_);
  else if (ny_ > b.yhi) ny_ = b.yhi - (ny_ - b.yhi);
  tx[k] = nx_;
  ty[k] = ny_;
  const double ddx = nx_ - cx, ddy = ny_ - cy;
  const double dist = sqrt(ddx * ddx + ddy * ddy);
  if (dist <= capture) {
    capstep[k] = stepno;
    status[k] = 1.0;
    return 1.0;
  }
  return status[k];  // (as tracer_move: the value read behind the move, not carried across it)
}

}  // namespace dev
}  // namespace pucfem
