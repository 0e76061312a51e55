// Time-dependent strokes (pucfem_set_stroke, pucfem_ens_set_stroke, include/pucfem.h): the squirmer's Dirichlet values
// rewritten on the device in front of every step from a periodic table of mode amplitudes.  With s the steps taken
// since the stroke was set (a counter in device memory, read and advanced here), the step being taken imposes, for
// driven entry i,
//
//   row    = (start + s) mod P
//   vt     = amp[row][0] * shape[i][0]
//   vt     = vt + amp[row][j] * shape[i][j]        j = 1 .. K - 1, in this order
//   val[q[i]] = (vt * dir[i].x, vt * dir[i].y)
//
// every product and sum as written (the build has -ffp-contract=off): a numpy line per product and sum gives the same
// bits (tests/stroke_reference.py).  q[i] is the entry's position in the value array the BC kernels read (the kept
// entries of the Dirichlet list, in build's order); entries no q names -- the walls -- keep their values.
//
// The counter without atomics: one block per context (per member), every thread reads the counter before the block's
// barrier and thread 0 stores the new count after it (k_tracer's pattern), so no thread reads an advanced count.  The
// block loops over the driven entries: 16 B of dir, 8 K B of shape and a 16 B store per entry, the table row from the
// cache.
#pragma once
#include "pucfem_kernels_impl.hpp"

namespace pucfem {
namespace dev {

constexpr int STROKE_MAX_MODES = 8;
constexpr int STROKE_MAX_PERIOD = 65536;
constexpr int ENS_STROKE_PARM = 4;  // per member: K (0: no stroke), P, start, the offset of its table (in doubles)

// the value of one driven entry from its table row a[0 .. K), in the order of the definition
__device__ __forceinline__ dbl2 stroke_value(int K, const double* __restrict__ a, const double* __restrict__ sh,
                                             dbl2 d) {
  double vt = a[0] * sh[0];
  for (int j = 1; j < K; ++j) vt = vt + a[j] * sh[j];
  return dbl2{vt * d.x, vt * d.y};
}

// one block's pass over the driven entries [0, n): the body of both kernels
__device__ __forceinline__ void stroke_entries(int K, const double* __restrict__ a, int32_t n,
                                               const int32_t* __restrict__ q, const double* __restrict__ shape,
                                               const dbl2* __restrict__ dir, dbl2* __restrict__ val) {
  for (int32_t i = threadIdx.x; i < n; i += blockDim.x) val[q[i]] = stroke_value(K, a, shape + (int64_t)i * K, dir[i]);
}

// One block.  ctr non-null: the step's launch -- the row from the counter, which is advanced; ctr null: row `row`
// (pucfem_stroke_apply and the probe: val is a scratch array).
__global__ __launch_bounds__(BS) void k_stroke_bc(int K, int64_t P, int64_t start, int64_t* ctr, int64_t row,
                                                  const double* __restrict__ amp, int32_t n,
                                                  const int32_t* __restrict__ q, const double* __restrict__ shape,
                                                  const dbl2* __restrict__ dir, dbl2* __restrict__ val) {
  int64_t s = 0;
  if (ctr) {
    s = *ctr;
    row = (start + s) % P;
  }
  stroke_entries(K, amp + row * K, n, q, shape, dir, val);
  if (ctr) {
    __syncthreads();
    if (threadIdx.x == 0) *ctr = s + 1;
  }
}

// The same per ensemble member: member m0 + blockIdx.x, one block each.  parm: ENS_STROKE_PARM values per member; a
// member with K = 0 is skipped, its counter and values left alone.  amp: the members' tables one behind the other;
// ctr: one counter per member; shape, dir, q: shared (one mesh, one swimmer).  row < 0: the step's launch into the
// member's block of val (stride doubles apart); row >= 0: that row into val itself, the counter untouched
// (pucfem_stroke_apply for a member, on a scratch array).
__global__ __launch_bounds__(BS) void k_ens_stroke_bc(int32_t m0, const int64_t* __restrict__ parm, int64_t* ctr,
                                                      int64_t row, const double* __restrict__ amp, int32_t n,
                                                      const int32_t* __restrict__ q,
                                                      const double* __restrict__ shape, const dbl2* __restrict__ dir,
                                                      double* val, int64_t stride) {
  const int64_t m = (int64_t)m0 + blockIdx.x;
  const int64_t* p = parm + m * ENS_STROKE_PARM;
  const int K = (int)p[0];
  if (K == 0) return;  // (block-uniform)
  const bool step = row < 0;
  int64_t s = 0;
  if (step) {
    s = ctr[m];
    row = (p[2] + s) % p[1];
  }
  stroke_entries(K, amp + p[3] + row * K, n, q, shape, dir, reinterpret_cast<dbl2*>(step ? val + m * stride : val));
  if (step) {
    __syncthreads();
    if (threadIdx.x == 0) ctr[m] = s + 1;
  }
}

}  // namespace dev
}  // namespace pucfem
