// Sampling and rasterising kernels (pucfem_sample_points, pucfem_raster, pucfem_ens_raster, include/pucfem.h): the
// fields of a context read at caller-given points, or at the pixel centres of a window, on the device -- the
// interpolation at arbitrary points of StokesFood.py:482-487 and the frames of scripts/good_visualization2.py:536-571
// without a copy of the whole fields.
//
// One definition for both locators: for a query point q, taken as given (no wrap, no clamp), the triangle is the
// one sl_best returns -- among the triangles that pass the reference's weight test (sl_test) the smallest
// (squared centroid distance, triangle id) key in knn_less's order -- and the value is sl_value on it.  The k-NN
// rank test of the semi-Lagrangian step (sl_fast / sl_rank_ok: PointLocator's restriction on a back-traced point)
// is not applied: a sampler wants containment.  No passing triangle (outside the mesh, inside the swimmer, a
// non-finite q): NaN, triangle -1.  The lattice locator's weight test and keys are the record locator's bit for
// bit, so the result does not depend on the locator, and with -ffp-contract=off a brute force over all triangles
// reproduces it bit for bit (tests/test_gpu_sample.py).
//
// The kernels read the context's (or the ensemble's) fields in the internal numbering and layouts and write only
// their own outputs.
#pragma once
#include "pucfem_kernels.hpp"
#include "pucfem_locate.hpp"

namespace pucfem {
namespace dev {

constexpr int SMP_MAXC = 16;  // components per call (the 8 sampled fields hold 10)

// the requested components, in output order: base pointer and element stride in the internal numbering (VS for a
// component of the interleaved velocity), and the distance between two members of an ensemble (0: a context)
struct SampleFields {
  int32_t ncomp;
  int32_t stride[SMP_MAXC];
  const double* ptr[SMP_MAXC];
  int64_t member[SMP_MAXC];
};

// pixel (i, j) of a W x H raster of the window [x0, x1] x [y0, y1]: its centre; row j = 0 is the lowest y
struct RasterWin {
  double x0, y0, x1, y1;
  int32_t W, H;
};
__device__ __forceinline__ void raster_centre(const RasterWin& R, int32_t i, int32_t j, double& qx, double& qy) {
  qx = R.x0 + ((double)i + 0.5) * (R.x1 - R.x0) / (double)R.W;
  qy = R.y0 + ((double)j + 0.5) * (R.y1 - R.y0) / (double)R.H;
}
// Threads to pixels: a block of BS = 256 threads covers 16 x 16 pixels, each of its 4 waves a compact 8 x 8 tile
// (lane = 8 * row + column), so the lanes of a wave mostly share a macro face and neighbouring lattice cells (the
// face constants and cell table entries are fetched once per wave, the vertex gathers fall into few lines).  The
// blocks stride over the 16 x 16 tiles of the raster; ragged tiles mask their outside pixels.
constexpr int RT = 16;
__device__ __forceinline__ bool raster_pixel(const RasterWin& R, int64_t tile, int32_t tiles_x, int32_t& i, int32_t& j) {
  const int32_t ty = (int32_t)(tile / tiles_x), tx = (int32_t)(tile - (int64_t)ty * tiles_x);
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  i = tx * RT + (wv & 1) * 8 + (lane & 7);
  j = ty * RT + (wv >> 1) * 8 + (lane >> 3);
  return i < R.W && j < R.H;
}

// the located triangle with its vertex ids scaled to a component's element stride: sl_value then indexes the
// component's array directly (the interleaved velocity's ids stay below 2^31: N < 2^30)
__device__ __forceinline__ SlTri sample_strided(const SlTri& r, int32_t s) {
  SlTri q = r;
  q.a = r.a * s;
  q.b = r.b * s;
  q.d = r.d * s;
  return q;
}

// pucfem_sample_points: one thread per point, located once, every requested component interpolated from the
// located triangle's three vertices.  out: fp64, component-major (ncomp x np); tri (or null): the triangle id in
// the caller's numbering (the locators' keys carry it), -1 when none passes.
template <class LOC>
__global__ __launch_bounds__(BS) void k_sample_points(LOC L, int64_t np, const double* __restrict__ xy, SampleFields F,
                                                      double* __restrict__ out, int32_t* __restrict__ tri) {
  for (int64_t e = (int64_t)blockIdx.x * BS + threadIdx.x; e < np; e += (int64_t)gridDim.x * BS) {
    const double qx = xy[2 * e], qy = xy[2 * e + 1];
    SlTri r;
    double bestd;
    float rho2;
    const bool found = sl_best(L, -1, qx, qy, r, bestd, rho2);
    if (tri) tri[e] = found ? r.id : -1;
    for (int32_t k = 0; k < F.ncomp; ++k)
      out[(int64_t)k * np + e] = found ? sl_value(sample_strided(r, F.stride[k]), qx, qy, F.ptr[k]) : (double)NAN;
  }
}

// pucfem_raster: one thread per pixel (raster_pixel's mapping).  out: fp32, [component][H][W].
template <class LOC>
__global__ __launch_bounds__(BS) void k_raster(LOC L, RasterWin R, int32_t tiles_x, int64_t ntiles, SampleFields F,
                                               float* __restrict__ out) {
  const int64_t plane = (int64_t)R.W * R.H;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    int32_t i, j;
    if (!raster_pixel(R, tile, tiles_x, i, j)) continue;
    double qx, qy;
    raster_centre(R, i, j, qx, qy);
    SlTri r;
    double bestd;
    float rho2;
    const bool found = sl_best(L, -1, qx, qy, r, bestd, rho2);
    const int64_t px = (int64_t)j * R.W + i;
    for (int32_t k = 0; k < F.ncomp; ++k)
      out[(int64_t)k * plane + px] = found ? (float)sl_value(sample_strided(r, F.stride[k]), qx, qy, F.ptr[k]) : NAN;
  }
}

// pucfem_ens_raster: the same pixel mapping; a pixel is located ONCE and then interpolated for members
// [m0, m0 + nm) in a loop inside the thread (the members share the mesh, so the locate -- the dependent loads of
// the cell scan, most of a pixel's time -- is not repeated per member, as member tiles on blockIdx.y would; a
// member adds three gathers per component, from arrays of a small mesh that stay in cache).
// out: fp32, [member - m0][component][H][W].
template <class LOC>
__global__ __launch_bounds__(BS) void k_ens_raster(LOC L, RasterWin R, int32_t tiles_x, int64_t ntiles, SampleFields F,
                                                   int32_t m0, int32_t nm, float* __restrict__ out) {
  const int64_t plane = (int64_t)R.W * R.H;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    int32_t i, j;
    if (!raster_pixel(R, tile, tiles_x, i, j)) continue;
    double qx, qy;
    raster_centre(R, i, j, qx, qy);
    SlTri r;
    double bestd;
    float rho2;
    const bool found = sl_best(L, -1, qx, qy, r, bestd, rho2);
    const int64_t px = (int64_t)j * R.W + i;
    for (int32_t m = 0; m < nm; ++m)
      for (int32_t k = 0; k < F.ncomp; ++k) {
        const double* f = F.ptr[k] + (int64_t)(m0 + m) * F.member[k];
        out[((int64_t)m * F.ncomp + k) * plane + px] =
            found ? (float)sl_value(sample_strided(r, F.stride[k]), qx, qy, f) : NAN;
      }
  }
}

// pucfem_raster_probe's pixel bookkeeping (measurement): cnt[0] pixels no triangle holds, cnt[1] pixels the
// lattice locator answers with the inner test of the first face listed in the pixel's macro-grid cell (sl_best's
// common case: one cell table entry and three vertices; the others take its general search).  The record locator
// has no such case: cnt[1] stays 0.
__device__ __forceinline__ bool sample_first_face(const LocDev&, double, double) { return false; }
__device__ __forceinline__ bool sample_first_face(const LatLocDev& L, double qx, double qy) {
  const int64_t gc = lat_gcell(L, qx, qy);
  const int32_t e = L.start[gc];
  if (e >= L.start[gc + 1]) return false;
  SlTri r;
  double d, u, v;
  return sl_inner(L, L.face[L.item[e]], qx, qy, r, d, u, v);
}
template <class LOC>
__global__ __launch_bounds__(BS) void k_raster_count(LOC L, RasterWin R, int32_t tiles_x, int64_t ntiles,
                                                     unsigned long long* cnt) {
  unsigned long long miss = 0, first = 0;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    int32_t i, j;
    if (!raster_pixel(R, tile, tiles_x, i, j)) continue;
    double qx, qy;
    raster_centre(R, i, j, qx, qy);
    SlTri r;
    double bestd;
    float rho2;
    if (!sl_best(L, -1, qx, qy, r, bestd, rho2)) ++miss;
    else if (sample_first_face(L, qx, qy)) ++first;
  }
  if (miss) atomicAdd(cnt, miss);
  if (first) atomicAdd(cnt + 1, first);
}

}  // namespace dev
}  // namespace pucfem
