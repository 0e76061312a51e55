// Projection-pass lab (standalone, gfx950): the row bodies of the library's k_mdot2<M> (pending-direction form,
// the right-hand side formed in the pass), k_pcomb<M> and k_reseed on synthetic data of the L7 size, with
//   basis loads   dword (the library's tiled layout, G = 1)  |  dwordx4 (the grouped layout, G = 4:
//                 element (i, r) at (((r >> 6) ld + (i & ~3)) << 6) + (r & 63) 4 + (i & 3)),
//   prefetch      none  |  the next grid-stride row's operands loaded before the current row's arithmetic,
//   basis loads   plain |  non-temporal,
//   k_pcomb's new column (G = 4): a 4-byte store at 16-byte stride | the whole group rewritten from registers.
// Every variant keeps the thread's rows, its accumulators and the order of its operations; its partial arrays /
// outputs are compared bit for bit with the literal HEAD form (h_*) before it is timed.
// Timing: 20 launches between two events, 5 repeats, median / min / max; TB/s from the algorithmic bytes per row.
// Build:  hipcc -O3 --offload-arch=gfx950 -std=c++17 -ffp-contract=off tools/proj_lab.hip -o tools/_bin/proj_lab
// Resources per variant: add -Rpass-analysis=kernel-resource-usage to the build line.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

#define CK(x)                                                                  \
  do {                                                                         \
    hipError_t e_ = (x);                                                       \
    if (e_ != hipSuccess) {                                                    \
      fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); \
      exit(1);                                                                 \
    }                                                                          \
  } while (0)

constexpr int BS = 256, MAXB = 32768, GRID = 2048;
constexpr int PROJ_MAX = 32, PROJ_KEEP_MAX = 16;
typedef float flt4 __attribute__((ext_vector_type(4)));

template <class T>
__device__ __forceinline__ T ldnt(const T* p) {
  return __builtin_nontemporal_load(p);
}
template <class T>
__device__ __forceinline__ void stnt(T* p, T v) {
  __builtin_nontemporal_store(v, p);
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
template <int G>
__host__ __device__ __forceinline__ int64_t pxi(int i, int64_t r, int64_t ld) {
  return (((r >> 6) * ld + (i & ~(G - 1))) << 6) + (r & 63) * G + (i & (G - 1));
}

// ------------------------------------------------------------------------------------------- HEAD forms
template <int M>
__global__ __launch_bounds__(BS) void h_mdot2(int64_t n, const float* __restrict__ X, int64_t ld,
                                              const double* __restrict__ av, const int32_t* __restrict__ master_of,
                                              double* part, const double* rf, const double* v, const double* braw,
                                              const int32_t* slave_of, const double* sum, double inv_nfree, double* bh) {
  constexpr int NA = 2 * M + 4;
  __shared__ double sh[NA][4];
  const double mean = sum[0] * inv_nfree;
  const int64_t step = (int64_t)gridDim.x * BS;
  double acc[NA];
#pragma unroll
  for (int i = 0; i < NA; ++i) acc[i] = 0.0;
  for (int64_t r = (int64_t)blockIdx.x * BS + threadIdx.x; r < n; r += step) {
    double br;
    if (master_of[r] >= 0) {
      br = 0.0;
    } else {
      br = braw[r];
      if (slave_of[r] >= 0) br += braw[slave_of[r]];
      br = br - mean;
    }
    stnt(bh + r, br);
    const double ar = av[r] - rf[r];
    const double vr = v[r];
    float x[M];
#pragma unroll
    for (int i = 0; i < M; ++i) x[i] = X[pxi<1>(i, r, ld)];
#pragma unroll
    for (int i = 0; i < M; ++i) {
      acc[i] += (double)x[i] * br;
      acc[M + i] += (double)x[i] * ar;
    }
    acc[2 * M] += vr * br;
    acc[2 * M + 1] += vr * ar;
    if (master_of[r] < 0) {
      acc[2 * M + 2] += vr;
      acc[2 * M + 3] += br;
    }
  }
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    const double t = wave_sum(acc[i]);
    if ((threadIdx.x & 63) == 0) sh[i][threadIdx.x >> 6] = t;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < NA; i += BS)
    part[(int64_t)i * MAXB + blockIdx.x] = (sh[i][0] + sh[i][1]) + (sh[i][2] + sh[i][3]);
}

template <int M>
__global__ __launch_bounds__(BS) void h_pcomb(int64_t n, const float* __restrict__ X, int64_t ld,
                                              const double* __restrict__ K, const double* v,
                                              const int32_t* __restrict__ master_of, float* __restrict__ xm_out,
                                              double* y) {
  double ka[M], kc[M];
#pragma unroll
  for (int i = 0; i < M; ++i) {
    ka[i] = K[i];
    kc[i] = K[M + i];
  }
  const double s = K[2 * M], mu = K[2 * M + 1], alpha = K[2 * M + 2];
  for (int64_t r = (int64_t)blockIdx.x * BS + threadIdx.x; r < n; r += (int64_t)gridDim.x * BS) {
    float x[M];
#pragma unroll
    for (int i = 0; i < M; ++i) x[i] = X[pxi<1>(i, r, ld)];
    const double vr = v[r];
    double sa = 0.0, sc = 0.0;
#pragma unroll
    for (int i = 0; i < M; ++i) {
      sa += ka[i] * (double)x[i];
      sc += kc[i] * (double)x[i];
    }
    const double xm = s * (vr - ((master_of[r] < 0) ? mu : 0.0) - sc);
    const double g = sa + alpha * xm;
    stnt(xm_out + pxi<1>(0, r, ld), (float)xm);
    stnt(y + r, g);
  }
}

__global__ __launch_bounds__(BS) void h_reseed(int64_t n, const float* __restrict__ X, int64_t ld, int m,
                                               const double* __restrict__ Q, int kq, float* __restrict__ out) {
  __shared__ double q[PROJ_KEEP_MAX * PROJ_MAX];
  for (int t = threadIdx.x; t < PROJ_KEEP_MAX * PROJ_MAX; t += BS) q[t] = Q[t];
  __syncthreads();
  for (int64_t r = (int64_t)blockIdx.x * BS + threadIdx.x; r < n; r += (int64_t)gridDim.x * BS) {
    double acc[PROJ_KEEP_MAX];
#pragma unroll
    for (int i = 0; i < PROJ_KEEP_MAX; ++i) acc[i] = 0.0;
    for (int j = 0; j < m; ++j) {
      const double x = (double)X[pxi<1>(j, r, ld)];
#pragma unroll
      for (int i = 0; i < PROJ_KEEP_MAX; ++i) acc[i] += q[i * PROJ_MAX + j] * x;
    }
#pragma unroll
    for (int i = 0; i < PROJ_KEEP_MAX; ++i)
      if (i < kq) out[pxi<1>(i, r, ld)] = (float)acc[i];
  }
}

// ------------------------------------------------------------------------------------------- variants
// a row's basis values: M of them (G = 1), or the row's ceil(M / 4) groups in full (G = 4)
template <int M, int G>
constexpr int nx() {
  return (M + G - 1) / G * G;
}
template <int M, int G, bool NT>
__device__ __forceinline__ void load_x(const float* X, int64_t r, int64_t ld, float (&x)[nx<M, G>()]) {
  if constexpr (G == 1) {
#pragma unroll
    for (int i = 0; i < M; ++i) x[i] = NT ? ldnt(X + pxi<1>(i, r, ld)) : X[pxi<1>(i, r, ld)];
  } else {
    const flt4* p = reinterpret_cast<const flt4*>(X + pxi<4>(0, r, ld));
#pragma unroll
    for (int g = 0; g < nx<M, 4>() / 4; ++g) {
      const flt4 t = NT ? ldnt(p + 64 * g) : p[64 * g];
      x[4 * g] = t.x;
      x[4 * g + 1] = t.y;
      x[4 * g + 2] = t.z;
      x[4 * g + 3] = t.w;
    }
  }
}

struct MArgs {
  const double *av, *rf, *v, *braw;
  const int32_t *master_of, *slave_of;
  double* bh;
};
template <int M, int G>
struct MRow {
  float x[nx<M, G>()];
  double braw, av, rf, v;
  int32_t mo, so;
};
template <int M, int G, bool NT>
__device__ __forceinline__ void m_load(MRow<M, G>& w, const float* X, int64_t ld, const MArgs& A, int64_t r) {
  w.mo = A.master_of[r];
  w.braw = A.braw[r];
  w.so = A.slave_of[r];
  w.av = A.av[r];
  w.rf = A.rf[r];
  w.v = A.v[r];
  load_x<M, G, NT>(X, r, ld, w.x);
}
template <int M, int G>
__device__ __forceinline__ void m_comp(const MRow<M, G>& w, const MArgs& A, double mean, int64_t r,
                                       double (&acc)[2 * M + 4]) {
  double br;
  if (w.mo >= 0) {
    br = 0.0;
  } else {
    br = w.braw;
    if (w.so >= 0) br += A.braw[w.so];
    br = br - mean;
  }
  stnt(A.bh + r, br);
  const double ar = w.av - w.rf;
  const double vr = w.v;
#pragma unroll
  for (int i = 0; i < M; ++i) {
    acc[i] += (double)w.x[i] * br;
    acc[M + i] += (double)w.x[i] * ar;
  }
  acc[2 * M] += vr * br;
  acc[2 * M + 1] += vr * ar;
  if (w.mo < 0) {
    acc[2 * M + 2] += vr;
    acc[2 * M + 3] += br;
  }
}
template <int M, int G, bool PF, bool NT>
__global__ __launch_bounds__(BS) void v_mdot2(int64_t n, const float* __restrict__ X, int64_t ld, MArgs A,
                                              double* part, const double* sum, double inv_nfree) {
  constexpr int NA = 2 * M + 4;
  __shared__ double sh[NA][4];
  const double mean = sum[0] * inv_nfree;
  const int64_t step = (int64_t)gridDim.x * BS;
  double acc[NA];
#pragma unroll
  for (int i = 0; i < NA; ++i) acc[i] = 0.0;
  int64_t r = (int64_t)blockIdx.x * BS + threadIdx.x;
  if constexpr (!PF) {
    for (; r < n; r += step) {
      MRow<M, G> w;
      m_load<M, G, NT>(w, X, ld, A, r);
      m_comp<M, G>(w, A, mean, r, acc);
    }
  } else {
    MRow<M, G> a, b;
    if (r < n) m_load<M, G, NT>(a, X, ld, A, r);
    while (r < n) {
      const int64_t r2 = r + step;
      if (r2 < n) m_load<M, G, NT>(b, X, ld, A, r2);
      m_comp<M, G>(a, A, mean, r, acc);
      if (r2 >= n) break;
      r = r2 + step;
      if (r < n) m_load<M, G, NT>(a, X, ld, A, r);
      m_comp<M, G>(b, A, mean, r2, acc);
    }
  }
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    const double t = wave_sum(acc[i]);
    if ((threadIdx.x & 63) == 0) sh[i][threadIdx.x >> 6] = t;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < NA; i += BS)
    part[(int64_t)i * MAXB + blockIdx.x] = (sh[i][0] + sh[i][1]) + (sh[i][2] + sh[i][3]);
}

template <int M, int G>
struct PRow {
  float x[nx<M, G>()];
  double v;
  int32_t mo;
};
template <int M, int G, bool NT>
__device__ __forceinline__ void p_load(PRow<M, G>& w, const float* X, int64_t ld, const double* v,
                                       const int32_t* master_of, int64_t r) {
  load_x<M, G, NT>(X, r, ld, w.x);
  w.v = v[r];
  w.mo = master_of[r];
}
// ST (G = 4): the new column's group rewritten whole (members below M from the registers, pads 0)
template <int M, int G, bool ST>
__device__ __forceinline__ void p_comp(const PRow<M, G>& w, const double (&ka)[M], const double (&kc)[M], double s,
                                       double mu, double alpha, float* X, int64_t ld, double* y, int64_t r) {
  double sa = 0.0, sc = 0.0;
#pragma unroll
  for (int i = 0; i < M; ++i) {
    sa += ka[i] * (double)w.x[i];
    sc += kc[i] * (double)w.x[i];
  }
  const double xm = s * (w.v - ((w.mo < 0) ? mu : 0.0) - sc);
  const double g = sa + alpha * xm;
  if constexpr (G == 4 && ST) {
    constexpr int g0 = M & ~3, k = M & 3;
    flt4 o;
    o.x = k == 0 ? (float)xm : w.x[g0 < nx<M, G>() ? g0 : 0];
    o.y = k == 1 ? (float)xm : (k > 1 ? w.x[g0 + 1 < nx<M, G>() ? g0 + 1 : 0] : 0.0f);
    o.z = k == 2 ? (float)xm : (k > 2 ? w.x[g0 + 2 < nx<M, G>() ? g0 + 2 : 0] : 0.0f);
    o.w = k == 3 ? (float)xm : 0.0f;
    stnt(reinterpret_cast<flt4*>(X + pxi<4>(g0, r, ld)), o);
  } else {
    stnt(X + pxi<G>(M, r, ld), (float)xm);
  }
  stnt(y + r, g);
}
// (ST rewrites values the thread read through X: no __restrict__ on the basis then)
template <bool R>
using XPtr = std::conditional_t<R, const float* __restrict__, const float*>;
template <bool R>
using OPtr = std::conditional_t<R, float* __restrict__, float*>;
template <int M, int G, bool PF, bool NT, bool ST>
__global__ __launch_bounds__(BS) void v_pcomb(int64_t n, XPtr<!ST> X, int64_t ld, const double* __restrict__ K,
                                              const double* v, const int32_t* __restrict__ master_of, OPtr<!ST> Xo,
                                              double* y) {
  double ka[M], kc[M];
#pragma unroll
  for (int i = 0; i < M; ++i) {
    ka[i] = K[i];
    kc[i] = K[M + i];
  }
  const double s = K[2 * M], mu = K[2 * M + 1], alpha = K[2 * M + 2];
  const int64_t step = (int64_t)gridDim.x * BS;
  int64_t r = (int64_t)blockIdx.x * BS + threadIdx.x;
  if constexpr (!PF) {
    for (; r < n; r += step) {
      PRow<M, G> w;
      p_load<M, G, NT>(w, X, ld, v, master_of, r);
      p_comp<M, G, ST>(w, ka, kc, s, mu, alpha, Xo, ld, y, r);
    }
  } else {
    PRow<M, G> a, b;
    if (r < n) p_load<M, G, NT>(a, X, ld, v, master_of, r);
    while (r < n) {
      const int64_t r2 = r + step;
      if (r2 < n) p_load<M, G, NT>(b, X, ld, v, master_of, r2);
      p_comp<M, G, ST>(a, ka, kc, s, mu, alpha, Xo, ld, y, r);
      if (r2 >= n) break;
      r = r2 + step;
      if (r < n) p_load<M, G, NT>(a, X, ld, v, master_of, r);
      p_comp<M, G, ST>(b, ka, kc, s, mu, alpha, Xo, ld, y, r2);
    }
  }
}

// G = 4: a group per load, its members in the order j of HEAD's loop; whole groups stored (pads 0)
template <int G, bool NT>
__global__ __launch_bounds__(BS) void v_reseed(int64_t n, const float* __restrict__ X, int64_t ld, int m,
                                               const double* __restrict__ Q, int kq, float* __restrict__ out) {
  __shared__ double q[PROJ_KEEP_MAX * PROJ_MAX];
  for (int t = threadIdx.x; t < PROJ_KEEP_MAX * PROJ_MAX; t += BS) q[t] = Q[t];
  __syncthreads();
  for (int64_t r = (int64_t)blockIdx.x * BS + threadIdx.x; r < n; r += (int64_t)gridDim.x * BS) {
    double acc[PROJ_KEEP_MAX];
#pragma unroll
    for (int i = 0; i < PROJ_KEEP_MAX; ++i) acc[i] = 0.0;
    if constexpr (G == 1) {
      for (int j = 0; j < m; ++j) {
        const float* p = X + pxi<1>(j, r, ld);
        const double x = (double)(NT ? ldnt(p) : *p);
#pragma unroll
        for (int i = 0; i < PROJ_KEEP_MAX; ++i) acc[i] += q[i * PROJ_MAX + j] * x;
      }
#pragma unroll
      for (int i = 0; i < PROJ_KEEP_MAX; ++i)
        if (i < kq) out[pxi<1>(i, r, ld)] = (float)acc[i];
    } else {
      const flt4* p = reinterpret_cast<const flt4*>(X + pxi<4>(0, r, ld));
      for (int g = 0; 4 * g < m; ++g) {
        const flt4 t = NT ? ldnt(p + 64 * g) : p[64 * g];
        const float xs[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int j = 4 * g + k;
          if (j < m) {
            const double x = (double)xs[k];
#pragma unroll
            for (int i = 0; i < PROJ_KEEP_MAX; ++i) acc[i] += q[i * PROJ_MAX + j] * x;
          }
        }
      }
      flt4* o = reinterpret_cast<flt4*>(out + pxi<4>(0, r, ld));
#pragma unroll
      for (int g = 0; g < PROJ_KEEP_MAX / 4; ++g)
        if (4 * g < kq) {
          flt4 t;
          t.x = (float)acc[4 * g];
          t.y = 4 * g + 1 < kq ? (float)acc[4 * g + 1] : 0.0f;
          t.z = 4 * g + 2 < kq ? (float)acc[4 * g + 2] : 0.0f;
          t.w = 4 * g + 3 < kq ? (float)acc[4 * g + 3] : 0.0f;
          o[64 * g] = t;
        }
    }
  }
}

// ------------------------------------------------------------------------------------------- data and checks
__device__ __forceinline__ uint32_t mix(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return (uint32_t)((z ^ (z >> 31)) >> 32);
}
__device__ __forceinline__ double unit(uint64_t key) { return (double)mix(key) * (2.0 / 4294967296.0) - 1.0; }
template <int G>
__global__ void k_fill_x(int64_t n, int64_t ld, float* X) {
  for (int64_t t = (int64_t)blockIdx.x * BS + threadIdx.x; t < n * ld; t += (int64_t)gridDim.x * BS) {
    const int64_t r = t / ld;
    const int i = (int)(t % ld);
    X[pxi<G>(i, r, ld)] = (float)(1e-3 * unit((uint64_t)t + 0x1234567ull));
  }
}
__global__ void k_fill_v(int64_t n, double* p, uint64_t seed) {
  for (int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x; i < n; i += (int64_t)gridDim.x * BS)
    p[i] = unit((uint64_t)i * 2654435761ull + seed);
}
__global__ void k_fill_maps(int64_t n, int32_t* master_of, int32_t* slave_of) {
  for (int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x; i < n; i += (int64_t)gridDim.x * BS) {
    master_of[i] = i % 997 == 5 ? (int32_t)((i * 7) % n) : -1;
    slave_of[i] = i % 991 == 3 ? (int32_t)((i * 13) % n) : -1;
  }
}
// columns [c0, c1) of a G-layout basis set to a NaN pattern (a store that is missed shows)
template <int G>
__global__ void k_poison(int64_t n, int64_t ld, float* X, int c0, int c1) {
  for (int64_t r = (int64_t)blockIdx.x * BS + threadIdx.x; r < n; r += (int64_t)gridDim.x * BS)
    for (int c = c0; c < c1; ++c) X[pxi<G>(c, r, ld)] = __uint_as_float(0x7fc00123u);
}
__global__ void k_cmp_vec(int64_t n, const double* a, const double* b, unsigned long long* cnt) {
  for (int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x; i < n; i += (int64_t)gridDim.x * BS)
    if (__double_as_longlong(a[i]) != __double_as_longlong(b[i])) atomicAdd(cnt, 1ull);
}
// columns [0, c1) of a G-layout basis against the G = 1 one, and columns [c1, cz) against +0
template <int G>
__global__ void k_cmp_x(int64_t n, int64_t ld, const float* X1, const float* XG, int c1, int cz,
                        unsigned long long* cnt) {
  for (int64_t r = (int64_t)blockIdx.x * BS + threadIdx.x; r < n; r += (int64_t)gridDim.x * BS) {
    for (int c = 0; c < c1; ++c)
      if (__float_as_uint(X1[pxi<1>(c, r, ld)]) != __float_as_uint(XG[pxi<G>(c, r, ld)])) atomicAdd(cnt, 1ull);
    for (int c = c1; c < cz; ++c)
      if (__float_as_uint(XG[pxi<G>(c, r, ld)]) != 0u) atomicAdd(cnt, 1ull);
  }
}

struct Lab {
  int64_t n, ld = PROJ_MAX, nx;
  int iters = 20, reps = 5;
  float *X1, *X4, *O1, *O4;  // the basis in both layouts, and the re-seed targets
  double *av, *rf, *v, *braw, *bh, *bh_ref, *y, *y_ref, *part, *K, *Q, *sum;
  int32_t *master_of, *slave_of;
  unsigned long long* cnt;
  std::vector<double> part_ref, part_h;
  hipEvent_t e0, e1;
  int bad = 0;

  unsigned long long count() {
    unsigned long long c = 0;
    CK(hipMemcpy(&c, cnt, sizeof c, hipMemcpyDeviceToHost));
    CK(hipMemset(cnt, 0, sizeof c));
    return c;
  }
  template <class F>
  void time(const char* name, double bytes_row, bool ok, F&& launch) {
    std::vector<float> ms(reps);
    launch();  // (warm)
    CK(hipDeviceSynchronize());
    for (int k = 0; k < reps; ++k) {
      CK(hipEventRecord(e0, 0));
      for (int it = 0; it < iters; ++it) launch();
      CK(hipEventRecord(e1, 0));
      CK(hipEventSynchronize(e1));
      CK(hipEventElapsedTime(&ms[k], e0, e1));
      ms[k] /= (float)iters;
    }
    std::sort(ms.begin(), ms.end());
    const double med = ms[reps / 2];
    printf("%-34s %8.1f %8.1f %8.1f us  %5.2f TB/s  bits %s\n", name, 1e3 * med, 1e3 * ms[0], 1e3 * ms[reps - 1],
           bytes_row * (double)n / (med * 1e-3) / 1e12, ok ? "same" : "DIFFER");
    fflush(stdout);
    if (!ok) bad = 1;
  }

  template <int M>
  void mdot2_ref() {
    CK(hipMemset(part, 0, sizeof(double) * (2 * M + 4) * MAXB));
    hipLaunchKernelGGL(h_mdot2<M>, dim3(GRID), dim3(BS), 0, 0, n, (const float*)X1, ld, (const double*)av,
                       (const int32_t*)master_of, part, (const double*)rf, (const double*)v, (const double*)braw,
                       (const int32_t*)slave_of, (const double*)sum, 1.0 / (double)n, bh_ref);
    part_ref.resize((size_t)(2 * M + 4) * MAXB);
    CK(hipMemcpy(part_ref.data(), part, sizeof(double) * part_ref.size(), hipMemcpyDeviceToHost));
    char name[64];
    snprintf(name, sizeof name, "mdot2<%d> HEAD", M);
    time(name, 4.0 * M + 44.0, true, [&] {
      hipLaunchKernelGGL(h_mdot2<M>, dim3(GRID), dim3(BS), 0, 0, n, (const float*)X1, ld, (const double*)av,
                         (const int32_t*)master_of, part, (const double*)rf, (const double*)v, (const double*)braw,
                         (const int32_t*)slave_of, (const double*)sum, 1.0 / (double)n, bh_ref);
    });
  }
  template <int M, int G, bool PF, bool NT>
  void mdot2_var() {
    const MArgs A{av, rf, v, braw, master_of, slave_of, bh};
    const float* X = G == 1 ? X1 : X4;
    auto launch = [&] {
      hipLaunchKernelGGL((v_mdot2<M, G, PF, NT>), dim3(GRID), dim3(BS), 0, 0, n, X, ld, A, part, (const double*)sum,
                         1.0 / (double)n);
    };
    CK(hipMemset(part, 0, sizeof(double) * (2 * M + 4) * MAXB));
    CK(hipMemset(bh, 0xff, sizeof(double) * n));
    launch();
    part_h.resize(part_ref.size());
    CK(hipMemcpy(part_h.data(), part, sizeof(double) * part_h.size(), hipMemcpyDeviceToHost));
    hipLaunchKernelGGL(k_cmp_vec, dim3(GRID), dim3(BS), 0, 0, n, (const double*)bh, (const double*)bh_ref, cnt);
    const bool ok = memcmp(part_h.data(), part_ref.data(), sizeof(double) * part_h.size()) == 0 && count() == 0;
    char name[64];
    snprintf(name, sizeof name, "mdot2<%d> %s %s %s", M, G == 4 ? "x4   " : "dword", PF ? "pf" : "--", NT ? "nt" : "--");
    time(name, 4.0 * M + 44.0, ok, launch);
  }
  template <int M>
  void pcomb_ref() {
    hipLaunchKernelGGL(k_poison<1>, dim3(GRID), dim3(BS), 0, 0, n, ld, X1, M, M + 1);
    auto launch = [&] {
      hipLaunchKernelGGL(h_pcomb<M>, dim3(GRID), dim3(BS), 0, 0, n, (const float*)X1, ld, (const double*)K,
                         (const double*)v, (const int32_t*)master_of, X1 + pxi<1>(M, 0, ld), y_ref);
    };
    char name[64];
    snprintf(name, sizeof name, "pcomb<%d> HEAD", M);
    time(name, 4.0 * M + 24.0, true, launch);
  }
  // (after pcomb_ref<M>: X1's column M holds HEAD's new direction)
  template <int M, int G, bool PF, bool NT, bool ST>
  void pcomb_var() {
    // G = 1 writes the reference's own column: the check is then against a copy in O1
    float* X = G == 1 ? O1 : X4;
    if (G == 1) CK(hipMemcpy(O1, X1, sizeof(float) * nx, hipMemcpyDeviceToDevice));
    const int cz = (M + 4) & ~3;  // the end of the new column's group
    if (G == 1) hipLaunchKernelGGL(k_poison<1>, dim3(GRID), dim3(BS), 0, 0, n, ld, X, M, M + 1);
    else hipLaunchKernelGGL(k_poison<4>, dim3(GRID), dim3(BS), 0, 0, n, ld, X, M, ST ? cz : M + 1);
    CK(hipMemset(y, 0xff, sizeof(double) * n));
    auto launch = [&] {
      hipLaunchKernelGGL((v_pcomb<M, G, PF, NT, ST>), dim3(GRID), dim3(BS), 0, 0, n, X, ld, (const double*)K,
                         (const double*)v, (const int32_t*)master_of, X, y);
    };
    launch();
    hipLaunchKernelGGL(k_cmp_vec, dim3(GRID), dim3(BS), 0, 0, n, (const double*)y, (const double*)y_ref, cnt);
    if (G == 1) hipLaunchKernelGGL(k_cmp_x<1>, dim3(GRID), dim3(BS), 0, 0, n, ld, (const float*)X1, (const float*)X, M + 1, M + 1, cnt);
    else hipLaunchKernelGGL(k_cmp_x<4>, dim3(GRID), dim3(BS), 0, 0, n, ld, (const float*)X1, (const float*)X, M + 1, ST ? cz : M + 1, cnt);
    const bool ok = count() == 0;
    char name[64];
    snprintf(name, sizeof name, "pcomb<%d> %s %s %s %s", M, G == 4 ? "x4   " : "dword", PF ? "pf" : "--",
             NT ? "nt" : "--", G == 4 ? (ST ? "group" : "4B   ") : "");
    time(name, 4.0 * M + 24.0, ok, launch);
  }
  void reseed_ref(int m, int kq) {
    auto launch = [&] {
      hipLaunchKernelGGL(h_reseed, dim3(GRID), dim3(BS), 0, 0, n, (const float*)X1, ld, m, (const double*)Q, kq, O1);
    };
    char name[64];
    snprintf(name, sizeof name, "reseed m=%d kq=%d HEAD", m, kq);
    time(name, 4.0 * (m + kq), true, launch);
  }
  template <int G, bool NT>
  void reseed_var(int m, int kq) {
    float* O = O4;  // (G = 1 too: O1 keeps the reference)
    CK(hipMemset(O, 0xff, sizeof(float) * nx));
    auto launch = [&] {
      hipLaunchKernelGGL((v_reseed<G, NT>), dim3(GRID), dim3(BS), 0, 0, n, (const float*)(G == 1 ? X1 : X4), ld, m,
                         (const double*)Q, kq, O);
    };
    launch();
    hipLaunchKernelGGL(k_cmp_x<G>, dim3(GRID), dim3(BS), 0, 0, n, ld, (const float*)O1, (const float*)O, kq,
                       G == 4 ? (kq + 3) & ~3 : kq, cnt);
    const bool ok = count() == 0;
    char name[64];
    snprintf(name, sizeof name, "reseed m=%d kq=%d %s %s", m, kq, G == 4 ? "x4   " : "dword", NT ? "nt" : "--");
    time(name, 4.0 * (m + kq), ok, launch);
  }

  template <int M>
  void size() {
    // the basis (both layouts) afresh: pcomb's column and the poison of an earlier size are gone
    hipLaunchKernelGGL(k_fill_x<1>, dim3(4096), dim3(BS), 0, 0, n, ld, X1);
    hipLaunchKernelGGL(k_fill_x<4>, dim3(4096), dim3(BS), 0, 0, n, ld, X4);
    mdot2_ref<M>();
    mdot2_var<M, 1, false, false>();
    mdot2_var<M, 1, false, true>();
    mdot2_var<M, 1, true, false>();
    mdot2_var<M, 1, true, true>();
    mdot2_var<M, 4, false, false>();
    mdot2_var<M, 4, false, true>();
    mdot2_var<M, 4, true, false>();
    mdot2_var<M, 4, true, true>();
    pcomb_ref<M>();
    pcomb_var<M, 1, false, false, false>();
    pcomb_var<M, 1, false, true, false>();
    pcomb_var<M, 1, true, false, false>();
    pcomb_var<M, 1, true, true, false>();
    pcomb_var<M, 4, false, false, false>();
    pcomb_var<M, 4, false, false, true>();
    pcomb_var<M, 4, false, true, false>();
    pcomb_var<M, 4, false, true, true>();
    pcomb_var<M, 4, true, false, false>();
    pcomb_var<M, 4, true, false, true>();
    pcomb_var<M, 4, true, true, false>();
    pcomb_var<M, 4, true, true, true>();
  }
};

int main(int argc, char** argv) {
  Lab L;
  L.n = argc > 1 ? atoll(argv[1]) : 14230528;
  if (argc > 2) L.iters = atoi(argv[2]);
  const int64_t n = L.n, tiles = (n + 63) / 64;
  L.nx = tiles * 64 * L.ld;
  for (float** p : {&L.X1, &L.X4, &L.O1, &L.O4}) CK(hipMalloc(p, sizeof(float) * L.nx));
  for (double** p : {&L.av, &L.rf, &L.v, &L.braw, &L.bh, &L.bh_ref, &L.y, &L.y_ref}) CK(hipMalloc(p, sizeof(double) * n));
  CK(hipMalloc(&L.part, sizeof(double) * (2 * PROJ_MAX + 4) * MAXB));
  CK(hipMalloc(&L.K, sizeof(double) * (2 * PROJ_MAX + 4)));
  CK(hipMalloc(&L.Q, sizeof(double) * PROJ_KEEP_MAX * PROJ_MAX));
  CK(hipMalloc(&L.sum, sizeof(double)));
  CK(hipMalloc(&L.master_of, sizeof(int32_t) * n));
  CK(hipMalloc(&L.slave_of, sizeof(int32_t) * n));
  CK(hipMalloc(&L.cnt, sizeof(unsigned long long)));
  CK(hipMemset(L.cnt, 0, sizeof(unsigned long long)));
  for (float* p : {L.X1, L.X4, L.O1, L.O4}) CK(hipMemset(p, 0, sizeof(float) * L.nx));
  uint64_t seed = 11;
  for (double* p : {L.av, L.rf, L.v, L.braw}) hipLaunchKernelGGL(k_fill_v, dim3(4096), dim3(BS), 0, 0, n, p, seed += 1000003);
  hipLaunchKernelGGL(k_fill_v, dim3(1), dim3(BS), 0, 0, (int64_t)(2 * PROJ_MAX + 4), L.K, 77ull);
  hipLaunchKernelGGL(k_fill_v, dim3(2), dim3(BS), 0, 0, (int64_t)(PROJ_KEEP_MAX * PROJ_MAX), L.Q, 99ull);
  hipLaunchKernelGGL(k_fill_v, dim3(1), dim3(BS), 0, 0, (int64_t)1, L.sum, 5ull);
  hipLaunchKernelGGL(k_fill_maps, dim3(4096), dim3(BS), 0, 0, n, L.master_of, L.slave_of);
  CK(hipDeviceSynchronize());
  CK(hipEventCreate(&L.e0));
  CK(hipEventCreate(&L.e1));
  printf("n = %lld rows, ld = %lld, grid %d x %d, %d launches per timing, %d repeats\n", (long long)n, (long long)L.ld,
         GRID, BS, L.iters, L.reps);
  printf("%-34s %8s %8s %8s\n", "kernel  loads  prefetch  nt  store", "median", "min", "max");
  L.size<16>();
  L.size<24>();
  L.size<31>();
  hipLaunchKernelGGL(k_fill_x<1>, dim3(4096), dim3(BS), 0, 0, n, L.ld, L.X1);
  hipLaunchKernelGGL(k_fill_x<4>, dim3(4096), dim3(BS), 0, 0, n, L.ld, L.X4);
  for (int kq : {16, 13}) {
    L.reseed_ref(32, kq);
    L.reseed_var<1, false>(32, kq);
    L.reseed_var<1, true>(32, kq);
    L.reseed_var<4, false>(32, kq);
    L.reseed_var<4, true>(32, kq);
  }
  CK(hipDeviceSynchronize());
  printf("%s\n", L.bad ? "FAILED: a variant's bits differ" : "all variants: same bits as HEAD");
  return L.bad;
}
