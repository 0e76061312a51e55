// Streamline kernels (pucfem_streamlines, pucfem_ens_streamlines, include/pucfem.h): the frozen velocity integrated
// from many seeds on the device -- the ax.streamplot(...) of the reference's flow pictures (stokes_flow.py:536,
// good_visualization.py:738) without a copy of u and without one sampler call per integrator stage.
//
// A line is a chain of dependent locates and gathers: latency, not bandwidth.  So one thread owns one line and
// keeps it in registers from seed to end; a wave runs up to 64 lines side by side (SlnArgs::lanes below).  The
// outputs are step-major (point s of line e next to point s of line e + 1), so a wave stores adjacent addresses
// at every step; the host returns the transposed view.
//
// Locating is the samplers' (pucfem_sample.hpp): sl_best without the rank test, the smallest (d^2, id) key, the
// point taken as given; the velocity and every extra field are sl_value on the located triangle.  Every product
// and sum of the step below is written as include/pucfem.h states it (the library is built with
// -ffp-contract=off), so a numpy restatement reproduces a line bit for bit (tests/test_gpu_streamlines.py).
//
// The locator's hint is carried from one locate to the next (consecutive points of a line are a step apart):
//   lattice locator: the `home` face of sl_best -- the macro face of the last located triangle, read from its
//     face-interior vertices (LatLocDev::home; a cell whose three vertices lie on the skeleton gives none);
//   record locator: the last triangle itself is tested first and accepted only when sl_test passes with its
//     margin flag (all weights >= SL_MARGIN: no other triangle passes, so it is what sl_best returns).
// Either way the hint only shortens the search: the located triangle, hence every output bit, is the same.
#pragma once
#include "pucfem_sample.hpp"

namespace pucfem {
namespace dev {

// One-wave blocks, of which the first `lanes` threads own a line each (SlnArgs::lanes, 1 .. 64, chosen by the host).
// A wave runs as long as its slowest lane and takes every branch one of its lanes takes (a lane whose hint misses
// sends the wave through the full search), so a few thousand lines run faster a few to a wave, spread over all
// SIMDs, than 64 to a wave on a few of them.  The host doubles the lanes while the launch keeps a number of waves
// taken from measurements at 256 to 65536 lines: up to SLN_MANY lines the record locator is fastest
// one line to a wave until every SIMD of 256 CUs holds its 4 waves (SLN_WAVES_REC), the lattice locator, whose face
// constants a wave's lanes share, with far fewer and fuller waves (SLN_WAVES_LAT); above, both with SLN_WAVES_MANY.
// A tuning choice only: a line's arithmetic does not depend on its thread.
constexpr int SLN_BS = 64;
constexpr int64_t SLN_WAVES_REC = 4096, SLN_WAVES_LAT = 512, SLN_MANY = 16384, SLN_WAVES_MANY = 2048;
constexpr int32_t SLN_UNIT = 1, SLN_EULER = 2, SLN_BOTH = 4;  // pucfem_streamline_flag
constexpr int32_t SLN_COMPLETE = 0, SLN_LEFT = 1, SLN_STAGNANT = 2, SLN_SEED_OUTSIDE = 3;

// the call's scalars
struct SlnArgs {
  int64_t nseeds, lines;
  double h, vmin;
  int32_t nsteps, flags, hint, lanes;
};
// the line of this thread, -1: none
__device__ __forceinline__ int64_t sln_thread_line(const SlnArgs& A) {
  if ((int32_t)threadIdx.x >= A.lanes) return -1;
  const int64_t e = (int64_t)blockIdx.x * A.lanes + threadIdx.x;
  return e < A.lines ? e : -1;
}

// T(q) with the hint of the last locate.  r: in, the last located triangle (when hint >= 0); out, T(q).
__device__ __forceinline__ bool sln_locate(const LocDev& L, bool use, int32_t& hint, double qx, double qy, SlTri& r) {
  if (use && hint >= 0) {
    double d;
    bool margin;
    if (sl_test(r, qx, qy, d, margin) && margin) return true;
  }
  double bestd;
  float rho2;
  SlTri t;
  if (!sl_best(L, -1, qx, qy, t, bestd, rho2)) return false;
  r = t;
  hint = 0;
  return true;
}
__device__ __forceinline__ bool sln_locate(const LatLocDev& L, bool use, int32_t& hint, double qx, double qy,
                                           SlTri& r) {
  double bestd;
  float rho2;
  if (!sl_best(L, use ? hint : -1, qx, qy, r, bestd, rho2)) return false;
  if (use) {
    const int32_t ha = L.home[r.a], hb = L.home[r.b], hd = L.home[r.d];
    hint = ha >= 0 ? ha : (hb >= 0 ? hb : hd);
  }
  return true;
}

// D(V(p)) on the located triangle r: false when the line is stagnant there
__device__ __forceinline__ bool sln_dir(const SlTri& r, double px, double py, const double* __restrict__ ux,
                                        const double* __restrict__ uy, int32_t stride, double vmin, bool unit,
                                        double& dx, double& dy) {
  const SlTri q = sample_strided(r, stride);
  const double vx = sl_value(q, px, py, ux), vy = sl_value(q, px, py, uy);
  const double ax = fabs(vx), ay = fabs(vy);
  if (!(ax > vmin || ay > vmin)) return false;
  if (unit) {
    const double m = ax > ay ? ax : ay;
    dx = vx / m;
    dy = vy / m;
  } else {
    dx = vx;
    dy = vy;
  }
  return true;
}

// One line, seed to end.  points / values: the line's first entries (point 0), `lines` entries between two steps;
// values: component k a further (nsteps + 1) * lines entries on.  F.ncomp == 0: no values.
template <class LOC>
__device__ __forceinline__ void sln_line(const LOC& L, const SlnArgs& A, int64_t e, const double* __restrict__ seeds,
                                         const double* __restrict__ ux, const double* __restrict__ uy, int32_t stride,
                                         const SampleFields& F, double* __restrict__ points,
                                         int32_t* __restrict__ status, int32_t* __restrict__ npts,
                                         double* __restrict__ values) {
  const int64_t seed = e < A.nseeds ? e : e - A.nseeds;
  const double h = e < A.nseeds ? A.h : -A.h, hh = 0.5 * h;
  const bool unit = (A.flags & SLN_UNIT) != 0, euler = (A.flags & SLN_EULER) != 0, use = A.hint != 0;
  const int64_t plane = (int64_t)(A.nsteps + 1) * A.lines;
  double px = seeds[2 * seed], py = seeds[2 * seed + 1];
  SlTri r;
  int32_t hint = -1, st = SLN_COMPLETE, n = 0;
  auto store = [&](int32_t s) {
    points[(int64_t)s * A.lines * 2] = px;
    points[(int64_t)s * A.lines * 2 + 1] = py;
    for (int32_t k = 0; k < F.ncomp; ++k)
      values[(int64_t)k * plane + (int64_t)s * A.lines] =
          sl_value(sample_strided(r, F.stride[k]), px, py, F.ptr[k]);
  };
  if (!sln_locate(L, use, hint, px, py, r)) {
    st = SLN_SEED_OUTSIDE;
  } else {
    store(0);
    n = 1;
    for (int32_t s = 1; s <= A.nsteps; ++s) {
      double dx, dy;
      if (!sln_dir(r, px, py, ux, uy, stride, A.vmin, unit, dx, dy)) {
        st = SLN_STAGNANT;
        break;
      }
      if (!euler) {
        const double qx = py_mod1(px + hh * dx), qy = py + hh * dy;
        if (!sln_locate(L, use, hint, qx, qy, r)) {
          st = SLN_LEFT;
          break;
        }
        if (!sln_dir(r, qx, qy, ux, uy, stride, A.vmin, unit, dx, dy)) {
          st = SLN_STAGNANT;
          break;
        }
      }
      const double nx = py_mod1(px + h * dx), ny = py + h * dy;
      if (!sln_locate(L, use, hint, nx, ny, r)) {
        st = SLN_LEFT;
        break;
      }
      px = nx;
      py = ny;
      store(s);
      n = s + 1;
    }
  }
  for (int32_t s = n; s <= A.nsteps; ++s) {  // past the end of the line: NaN
    points[(int64_t)s * A.lines * 2] = (double)NAN;
    points[(int64_t)s * A.lines * 2 + 1] = (double)NAN;
    for (int32_t k = 0; k < F.ncomp; ++k) values[(int64_t)k * plane + (int64_t)s * A.lines] = (double)NAN;
  }
  *status = st;
  *npts = n;
}

// pucfem_streamlines: one thread per line.  points: (nsteps + 1) x lines x 2; values: ncomp x (nsteps + 1) x lines.
template <class LOC>
__global__ __launch_bounds__(SLN_BS) void k_streamlines(LOC L, SlnArgs A, const double* __restrict__ seeds,
                                                        const double* __restrict__ ux, const double* __restrict__ uy,
                                                        SampleFields F, double* __restrict__ points,
                                                        int32_t* __restrict__ status, int32_t* __restrict__ npts,
                                                        double* __restrict__ values) {
  const int64_t e = sln_thread_line(A);
  if (e < 0) return;
  sln_line(L, A, e, seeds, ux, uy, VS, F, points + 2 * e, status + e, npts + e, values ? values + e : values);
}

// pucfem_ens_streamlines: grid.y the members m0 .. m0 + gridDim.y - 1 (as k_ens_tracer_cloud's), each locating
// for itself -- the members' velocities differ, so their lines do.  u: the ensemble's interleaved velocities
// (2 n per member).  Outputs member-major from m0; no values.
__global__ __launch_bounds__(SLN_BS) void k_ens_streamlines(LocDev L, SlnArgs A, const double* __restrict__ seeds,
                                                            const double* __restrict__ u, int64_t n, int32_t m0,
                                                            double* __restrict__ points, int32_t* __restrict__ status,
                                                            int32_t* __restrict__ npts) {
  const int64_t e = sln_thread_line(A);
  if (e < 0) return;
  const int64_t mi = blockIdx.y;
  const double* ux = u + (int64_t)(m0 + mi) * 2 * n;
  const SampleFields F{};
  sln_line(L, A, e, seeds, ux, ux + 1, VS, F, points + (mi * (int64_t)(A.nsteps + 1) * A.lines + e) * 2,
           status + mi * A.lines + e, npts + mi * A.lines + e, (double*)nullptr);
}

}  // namespace dev
}  // namespace pucfem
