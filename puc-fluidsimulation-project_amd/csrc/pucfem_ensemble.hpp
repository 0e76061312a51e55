// Ensemble kernels (pucfem_ens_*, include/pucfem.h): M members stepped together on one built small-mesh context
// (Ctx::dense) -- the reference's experiment, the same mesh and fluid under several squirmers (README.md:43-45:
// neutral / pusher / puller), in one launch chain.
//
// Members share every operator of the context (Vinv / Pinv, the SELL gradient / divergence coefficients, the
// record locator, the tracer grid) and differ in their Dirichlet values, fields and tracers.  State arrays are
// member-major in the context's internal row numbering and layouts (u / u*: interleaved pairs).  The member is
// blockIdx.y; the dense products take a compile-time tile of ENS_TM members per block, so each loaded matrix
// element is applied to ENS_TM members (one accumulator each) before the next is loaded.
//
// Arithmetic contract: per member, every kernel here performs the single path's operations in the single path's
// order (the same j = lane, lane + 64, ... accumulation and wave_sum of the dense products, the same ax / d forms,
// the single path's sl_* / tracer_* device functions, the same per-block partials and red_finish's order for the
// reductions, on the single path's grid in x).  With -ffp-contract=off a member's fields are therefore the bits
// of a single-context run with its boundary values (tests/test_gpu_ensemble.py).
#pragma once
#include "pucfem_kernels.hpp"
#include "pucfem_kernels_impl.hpp"
#include "pucfem_maccormack.hpp"

namespace pucfem {
namespace dev {

constexpr int ENS_TM = 4;     // members per block of the dense products
// per-member value slots (k_stats' layout in 0..6; 8: scratch maximum, 9: sum(braw), 10: not-found rows of the
// member's last inertial launch; 11 / 12: rows without T2 and clamped values of its last MacCormack dye launch,
// 13 / 14: the same of its last MacCormack velocity launch; 15 is free)
constexpr int ENS_VALS = 16;
// a member's flag as the inertial kernels read it (Ens::adv_on_dev): off, first order (k_ens_sl_vel), MacCormack
// (k_ens_mc_fwd / k_ens_mc_bwd); the consumers of ua (k_ens_force_rhs, k_ens_mv2_bc) read any non-zero value as on
constexpr int32_t ENS_ADV_OFF = 0, ENS_ADV_SL = 1, ENS_ADV_MC = 2;
// ... with the midpoint trajectory (k_ens_trj_fwd / k_ens_trj_bwd<dbl2>): values k_ens_sl_vel and k_ens_mc_*<dbl2> skip
constexpr int32_t ENS_ADV_SL_MID = 3, ENS_ADV_MC_MID = 4;
// a member's dye flag (Ens::mc_on_dev): 0 k_ens_sl moves its dye; 1 k_ens_mc_*<double>; 2 / 3 the midpoint trajectory
// with one pass / with MacCormack's two (k_ens_trj_*<double>).  k_ens_sl leaves, and k_ens_wsum runs, on any non-zero
constexpr int32_t ENS_DYE_SL = 0, ENS_DYE_MC = 1, ENS_DYE_SL_MID = 2, ENS_DYE_MC_MID = 3;
// the members' trajectory counts (Ens::trj_vals, stride ENS_VALS like vals): 0 the rows of the last dye launch whose
// pass-1 midpoint was not found, 1 / 2 pass 2's rows without T2 and clamped values (copied into vals 11 / 12), 3 its
// rows without midpoint; 4..7 the same of the last velocity launch (5 / 6 copied into vals 13 / 14); 8 the tracers of
// the last launch that fell back to their Euler step
constexpr int ENS_TRJ_DYE = 0, ENS_TRJ_VEL = 4, ENS_TRJ_FELL = 8;
// The slots above by name, for the host code that places reductions and reads counts (no kernel reads these names).
// ENS_V_*: a member's vals; ENS_T_*: within the dye's or the velocity's four slots of its trj_vals.
enum : int {
  ENS_V_DIV_STAR = 0,   // max |div u*|
  ENS_V_FINAL_DIV = 1,  // max |final div|
  ENS_V_SL = 2,         // sum wc, sum w (and k_ens_sl's not-found rows behind them)
  ENS_V_DYE_NF = 4,     // not-found rows of the last dye launch
  ENS_V_MIX = 5,        // the mixing variance
  ENS_V_EATEN = 6,      // tracers eaten
  ENS_V_SCRATCH = 8,    // a maximum that is not recorded
  ENS_V_BSUM = 9,       // sum(braw)
  ENS_V_VEL_NF = 10,    // not-found rows of the last inertial launch
  ENS_V_DYE_MC = 11,    // rows without T2, clamped values: the last MacCormack dye launch
  ENS_V_VEL_MC = 13,    // ... velocity launch
  ENS_T_MID1 = 0,       // rows without pass 1's midpoint
  ENS_T_MC = 1,         // pass 2's rows without T2, clamped values
  ENS_T_MID2 = 3,       // rows without pass 2's midpoint
};

// the member's reduction: the launch's RedOut template moved to the member's values, counter and partials
// (NP partial arrays of gridDim.x blocks per member)
template <int NP = 3>
__device__ __forceinline__ RedOut ens_red(const RedOut& ro, int32_t m, double*& part) {
  RedOut R = ro;
  R.out = ro.out + (int64_t)ENS_VALS * m;
  R.out1 = ro.out1 ? ro.out1 + (int64_t)ENS_VALS * m : nullptr;
  R.cnt = ro.cnt + m;
  R.stride = (int)gridDim.x;
  part += (int64_t)m * NP * gridDim.x;
  return R;
}

// k_dense_mv2_bc for a tile of members: u* = A_visc^-1 u with the velocity BCs of the result.  u, us: M x 2n;
// dval: M x dstride (the member's Dirichlet values in the context's entry order).  Dynamic LDS: 2 n ENS_TM doubles
// (component-major per member: consecutive lanes read consecutive doubles).  A ragged last tile computes its
// missing members as copies of the last member and does not store them.  With inertia (advon non-null: the members'
// flags) a member whose flag is set stages its plane of ua (M x 2n, k_ens_sl_vel's output) instead of its u: the
// single path's viscous product takes u_a as its input.  With body forces (fmask non-null: the members' term masks)
// a member whose mask is not 0 stages its plane of r (M x 2n, k_ens_force_rhs's output) instead.  The rows'
// accumulation is the same either way.
template <int TM>
__global__ __launch_bounds__(BS) void k_ens_mv2_bc(int64_t n, int32_t M, const double* __restrict__ Ainv,
                                                   const double* __restrict__ u, double* __restrict__ us,
                                                   const int32_t* __restrict__ bsrc, const int32_t* __restrict__ bdir,
                                                   const double* __restrict__ dval, int64_t dstride,
                                                   const double* __restrict__ ua, const int32_t* __restrict__ advon,
                                                   const double* __restrict__ fr, const int32_t* __restrict__ fmask) {
  extern __shared__ __align__(16) double ens_xl[];
  const int32_t m0 = (int32_t)blockIdx.y * TM;
#pragma unroll
  for (int t = 0; t < TM; ++t) {
    const int32_t mt = m0 + t < M ? m0 + t : M - 1;
    const dbl2* x =
        reinterpret_cast<const dbl2*>(fmask && fmask[mt] ? fr : advon && advon[mt] ? ua : u) + (int64_t)mt * n;
    for (int64_t j = threadIdx.x; j < n; j += BS) {
      const dbl2 q = x[j];
      ens_xl[(2 * t) * n + j] = q.x;
      ens_xl[(2 * t + 1) * n + j] = q.y;
    }
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < n; row += (int64_t)gridDim.x * 4) {
    const int32_t d = bdir[row];
    if (d >= 0) {
      if (lane < TM && m0 + lane < M) {
        const double* dv = dval + (int64_t)(m0 + lane) * dstride;
        reinterpret_cast<dbl2*>(us)[(int64_t)(m0 + lane) * n + row] = dbl2{dv[2 * d], dv[2 * d + 1]};
      }
      continue;
    }
    const double* a = Ainv + (int64_t)bsrc[row] * n;
    double s0[TM], s1[TM];
#pragma unroll
    for (int t = 0; t < TM; ++t) s0[t] = s1[t] = 0.0;
    for (int64_t j = lane; j < n; j += 64) {
      const double v = a[j];
#pragma unroll
      for (int t = 0; t < TM; ++t) {
        s0[t] += v * ens_xl[(2 * t) * n + j];
        s1[t] += v * ens_xl[(2 * t + 1) * n + j];
      }
    }
#pragma unroll
    for (int t = 0; t < TM; ++t) {
      s0[t] = wave_sum(s0[t]);
      s1[t] = wave_sum(s1[t]);
    }
#pragma unroll
    for (int t = 0; t < TM; ++t)
      if (lane == 0 && m0 + t < M) reinterpret_cast<dbl2*>(us)[(int64_t)(m0 + t) * n + row] = dbl2{s0[t], s1[t]};
  }
}

// k_dense_pres for a tile of members: the restated right-hand side from the member's braw and its reduced sum
// (vals slot 9), the pseudo-inverse product, p with every slave taking its master's value.  braw, p: M x n.
// Dynamic LDS: n ENS_TM doubles.
template <int TM>
__global__ __launch_bounds__(BS) void k_ens_pres(int64_t n, int32_t M, const double* __restrict__ Pinv,
                                                 const double* __restrict__ braw, const int32_t* __restrict__ slave_of,
                                                 const int32_t* __restrict__ master_of, const double* __restrict__ vals,
                                                 double inv_nfree, double* __restrict__ p) {
  extern __shared__ __align__(16) double ens_bl[];
  const int32_t m0 = (int32_t)blockIdx.y * TM;
#pragma unroll
  for (int t = 0; t < TM; ++t) {
    const int32_t mt = m0 + t < M ? m0 + t : M - 1;
    const double* br = braw + (int64_t)mt * n;
    const double mean = vals[(int64_t)ENS_VALS * mt + 9] * inv_nfree;
    for (int64_t j = threadIdx.x; j < n; j += BS) {
      double b;
      if (master_of[j] >= 0) {
        b = 0.0;
      } else {
        b = br[j];
        if (slave_of[j] >= 0) b += br[slave_of[j]];
        b = b - mean;
      }
      ens_bl[t * n + j] = b;
    }
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < n; row += (int64_t)gridDim.x * 4) {
    if (master_of[row] >= 0) continue;  // (a slave row's p is its master's; nothing else reads its product)
    const double* a = Pinv + row * n;
    double acc[TM];
#pragma unroll
    for (int t = 0; t < TM; ++t) acc[t] = 0.0;
    for (int64_t j = lane; j < n; j += 64) {
      const double v = a[j];
#pragma unroll
      for (int t = 0; t < TM; ++t) acc[t] += v * ens_bl[t * n + j];
    }
#pragma unroll
    for (int t = 0; t < TM; ++t) acc[t] = wave_sum(acc[t]);
    const int32_t sl = slave_of[row];
#pragma unroll
    for (int t = 0; t < TM; ++t)
      if (lane == 0 && m0 + t < M) {
        double* pm = p + (int64_t)(m0 + t) * n;
        pm[row] = 1.0 * acc[t];
        if (sl >= 0) pm[sl] = 1.0 * acc[t];
      }
  }
}

// k_div (SELL rows, interleaved velocity) per member: max |div| and, with braw, the pressure right-hand side and
// its sum.  u: M x 2n, braw: M x n (or null), part: M x 3 gridDim.x.  gridDim.x: the single path's div grid.
template <bool C16>
__global__ __launch_bounds__(BS) void k_ens_div(SellDev A, const double* __restrict__ gx, const double* __restrict__ gy,
                                                const double* __restrict__ u, const double* __restrict__ as1,
                                                const double* __restrict__ mp, double negidt, double* __restrict__ braw,
                                                double* part, RedOut ro) {
  __shared__ double sh[4];
  const int32_t m = (int32_t)blockIdx.y;
  const int64_t n = A.n_own;
  const dbl2* um = reinterpret_cast<const dbl2*>(u) + (int64_t)m * n;
  double* bm = braw ? braw + (int64_t)m * n : nullptr;
  const RedOut R = ens_red(ro, m, part);
  double mx = 0.0, sb = 0.0;
  int64_t s0, s1;
  block_slices_n(A.nslices, gridDim.x, blockIdx.x, s0, s1);
  const int lane = threadIdx.x & 63, wv = wave_id();
  for (int64_t s = s0 + wv; s < s1; s += 4) {
    const int64_t off = A.off[s];
    const int w = A.w[s];
    const int64_t row = sell_row(A, s, lane);
    const int32_t base = (int32_t)(s * 64);
    double acc = 0.0;
    for (int k = 0; k < w; ++k) {
      const int64_t e = off + (int64_t)k * 64 + lane;
      const dbl2 q = um[sell_col<C16, false>(A, e, base)];
      acc += gx[e] * q.x + gy[e] * q.y;
    }
    if (row >= 0) {
      const double d = acc / as1[row];
      mx = fmax(mx, fabs(d));
      if (bm) {
        const double b = mp[row] * (negidt * d);
        bm[row] = b;
        sb += b;
      }
    }
  }
  const double t = block_max(mx, sh);
  const double v = block_sum(sb, sh);
  if (threadIdx.x == 0) {
    red_part(R, part, 0, t);
    red_part(R, part, 1, v);
  }
  red_finish(R, part, sh);
}

// k_div<CURL> (SELL rows, interleaved velocity) per member: the vorticity of the member's u as the divergence of
// (u_y, -u_x), in k_ens_div's operation order, and the four flow partials in the single path's order (max |w|,
// sum wt w^2, sum wt |u|^2, max |u|^2 with wt = area_sum + 1e-12; the last two only with `energy`).
// u: M x 2n, vort: M x n (or null), part: M x 4 gridDim.x.  gridDim.x: the single path's div grid.
template <bool C16>
__global__ __launch_bounds__(BS) void k_ens_curl(SellDev A, const double* __restrict__ gx, const double* __restrict__ gy,
                                                 const double* __restrict__ u, const double* __restrict__ as1,
                                                 double* __restrict__ vort, int energy, double* part, RedOut ro) {
  __shared__ double sh[4];
  const int32_t m = (int32_t)blockIdx.y;
  const int64_t n = A.n_own;
  const dbl2* um = reinterpret_cast<const dbl2*>(u) + (int64_t)m * n;
  double* vm = vort ? vort + (int64_t)m * n : nullptr;
  const RedOut R = ens_red<4>(ro, m, part);
  double mx = 0.0, sb = 0.0, se = 0.0, mu = 0.0;
  int64_t s0, s1;
  block_slices_n(A.nslices, gridDim.x, blockIdx.x, s0, s1);
  const int lane = threadIdx.x & 63, wv = wave_id();
  for (int64_t s = s0 + wv; s < s1; s += 4) {
    const int64_t off = A.off[s];
    const int w = A.w[s];
    const int64_t row = sell_row(A, s, lane);
    const int32_t base = (int32_t)(s * 64);
    double acc = 0.0;
    for (int k = 0; k < w; ++k) {
      const int64_t e = off + (int64_t)k * 64 + lane;
      const dbl2 q = rot<true>(um[sell_col<C16, false>(A, e, base)]);
      acc += gx[e] * q.x + gy[e] * q.y;
    }
    if (row >= 0) {
      const double wt = as1[row];
      const double d = acc / wt;
      if (vm) vm[row] = d;
      mx = fmax(mx, fabs(d));
      sb += wt * (d * d);
      if (energy) {
        const dbl2 q = um[row];
        const double q2 = q.x * q.x + q.y * q.y;
        se += wt * q2;
        mu = fmax(mu, q2);
      }
    }
  }
  const double t = block_max(mx, sh);
  const double v = block_sum(sb, sh);
  const double e = block_sum(se, sh);
  const double x = block_max(mu, sh);
  if (threadIdx.x == 0) {
    red_part(R, part, 2, e);
    red_part(R, part, 3, x);
    red_part(R, part, 0, t);
    red_part(R, part, 1, v);
  }
  red_finish<8>(R, part, sh);
}

// k_grad_proj_bc per member: the first projection with the velocity BCs.  p: M x n, us / u: M x 2n.
template <bool C16>
__global__ __launch_bounds__(BS) void k_ens_grad_proj_bc(SellDev A, const double* __restrict__ gx,
                                                         const double* __restrict__ gy, const double* __restrict__ p,
                                                         const double* __restrict__ as1, double dt, const double* us,
                                                         double* u, const int32_t* __restrict__ bsrc,
                                                         const int32_t* __restrict__ bdir,
                                                         const int32_t* __restrict__ spos,
                                                         const double* __restrict__ dval, int64_t dstride) {
  const int32_t m = (int32_t)blockIdx.y;
  const int64_t n = A.n_own;
  const double* pm = p + (int64_t)m * n;
  const dbl2* usm = reinterpret_cast<const dbl2*>(us) + (int64_t)m * n;
  dbl2* um = reinterpret_cast<dbl2*>(u) + (int64_t)m * n;
  const double* dv = dval + (int64_t)m * dstride;
  for (int64_t t = (int64_t)blockIdx.x * BS + threadIdx.x; t < A.nslices * 64; t += (int64_t)gridDim.x * BS) {
    const int64_t row = sell_row(A, t >> 6, (int)(t & 63));
    if (row < 0) continue;
    const int32_t dj = bdir[row];
    if (dj >= 0) {
      um[row] = dbl2{dv[2 * dj], dv[2 * dj + 1]};
      continue;
    }
    const int32_t src = bsrc[row];
    const int64_t pos = src == row ? t : (int64_t)spos[src];
    const int64_t ss = pos >> 6;
    const int lane = (int)(pos & 63);
    const int64_t off = A.off[ss];
    const int w = A.w[ss];
    const int32_t base = (int32_t)(ss * 64);
    const dbl2 o = usm[src];
    const double d = as1[src];
    double ax = 0.0, ay = 0.0;
    for (int k = 0; k < w; ++k) {
      const int64_t e = off + (int64_t)k * 64 + lane;
      const double pj = pm[sell_col<C16, false>(A, e, base)];
      ax += gx[e] * pj;
      ay += gy[e] * pj;
    }
    um[row] = dbl2{o.x - dt * (ax / d), o.y - dt * (ay / d)};
  }
}

// k_grad_proj mode 1 (SELL rows) per member: u[interior] -= DT grad p2.
template <bool C16>
__global__ __launch_bounds__(BS) void k_ens_grad_proj1(SellDev A, const double* __restrict__ gx,
                                                       const double* __restrict__ gy, const double* __restrict__ p,
                                                       const double* __restrict__ as1, double dt,
                                                       const uint8_t* __restrict__ dirflag, double* u) {
  const int32_t m = (int32_t)blockIdx.y;
  const int64_t n = A.n_own;
  const double* pm = p + (int64_t)m * n;
  dbl2* um = reinterpret_cast<dbl2*>(u) + (int64_t)m * n;
  int64_t s0, s1;
  block_slices_n(A.nslices, gridDim.x, blockIdx.x, s0, s1);
  const int lane = threadIdx.x & 63, wv = wave_id();
  for (int64_t s = s0 + wv; s < s1; s += 4) {
    const int64_t off = A.off[s];
    const int w = A.w[s];
    const int64_t row = sell_row(A, s, lane);
    const int32_t base = (int32_t)(s * 64);
    const int64_t rr = row >= 0 ? row : 0;
    const dbl2 o = um[rr];
    const double d = as1[rr];
    const bool dirichlet = dirflag[rr] != 0;
    double ax = 0.0, ay = 0.0;
    for (int k = 0; k < w; ++k) {
      const int64_t e = off + (int64_t)k * 64 + lane;
      const double pj = pm[sell_col<C16, false>(A, e, base)];
      ax += gx[e] * pj;
      ay += gy[e] * pj;
    }
    if (row >= 0 && !dirichlet) um[row] = dbl2{o.x - dt * (ax / d), o.y - dt * (ay / d)};
  }
}

// k_sl_rec_wave per member (row0 = 0: one rank): one wave per row, the single path's sl_row_wave (pucfem_locate.hpp).
// u: M x 2n, c / cout: M x n, part: M x 3 gridDim.x.  mc (M, or null: no member's dye moves by MacCormack): a member
// whose flag is set leaves at once, as in k_ens_sl_vel -- k_ens_mc_fwd / k_ens_mc_bwd / k_ens_wsum write its cout and
// its sums.
__global__ __launch_bounds__(BS) void k_ens_sl(MeshDev Mh, LocDev L, GridDev G, int64_t n, const double* __restrict__ u,
                                               double dt, const double* __restrict__ c, double* __restrict__ cout,
                                               const double* __restrict__ wmix, double* part, RedOut ro,
                                               const int32_t* __restrict__ mc) {
  __shared__ double sw_[3][BS / 64];
  __shared__ double sh[4];
  const int32_t m = (int32_t)blockIdx.y;
  if (mc && mc[m]) return;
  const double* ux = u + (int64_t)m * 2 * n;
  const double* uy = ux + 1;
  const double* cm = c + (int64_t)m * n;
  double* com = cout + (int64_t)m * n;
  const RedOut R = ens_red(ro, m, part);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * (BS / 64) + wv;
  double swc = 0.0, sw = 0.0, nnf = 0.0;
  if (i < n) {
    double cn;
    if (!sl_row_wave(Mh, L, G, i, ux[VS * i], uy[VS * i], dt, cm, cn)) nnf = 1.0;
    if (lane == 0) com[i] = cn;
    const double w = wmix[i];
    sw = w;
    swc = w * cn;
  }
  if (lane == 0) {
    sw_[0][wv] = swc;
    sw_[1][wv] = sw;
    sw_[2][wv] = nnf;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int v = 0; v < 3; ++v) {
      double a = 0.0;
      for (int k = 0; k < BS / 64; ++k) a += sw_[v][k];
      red_part(R, part, v, a);
    }
  }
  red_finish(R, part, sh);
}

// The inertial launch per member (pucfem_ens_set_inertia): ua = SL(u; u, dt) of the member's own interleaved
// velocity, in front of k_ens_mv2_bc.  k_ens_sl's sl_row_wave on k_ens_sl's grid in x (one wave per row), with
// k_sl_vel's field (pucfem_inertia.hpp): sl_value's pair form, so a member's ua holds the bits of the single path's
// u_adv.  Three 16-byte gathers from the member's u, one 16-byte store into its plane of ua; a row that is not found
// keeps its own pair.  A member whose flag is not ENS_ADV_SL (off, or MacCormack: k_ens_mc_* form its ua) leaves at
// once (a block-uniform exit in front of every barrier: its ticket is not drawn).  The not-found rows of each member: per-block partials, summed by red_finish in block order.
// u, ua: M x 2n (ua must not alias u: rows of other blocks still gather from u); on: M; part: M x gridDim.x.
__global__ __launch_bounds__(BS) void k_ens_sl_vel(MeshDev Mh, LocDev L, GridDev G, int64_t n,
                                                   const double* __restrict__ u, double dt,
                                                   const int32_t* __restrict__ on, double* __restrict__ ua, double* part,
                                                   RedOut ro) {
  __shared__ double sw_[BS / 64];
  __shared__ double sh[4];
  const int32_t m = (int32_t)blockIdx.y;
  if (on[m] != ENS_ADV_SL) return;
  const dbl2* f = reinterpret_cast<const dbl2*>(u) + (int64_t)m * n;
  dbl2* out = reinterpret_cast<dbl2*>(ua) + (int64_t)m * n;
  const RedOut R = ens_red<1>(ro, m, part);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * (BS / 64) + wv;
  double nnf = 0.0;
  if (i < n) {
    const dbl2 v = f[i];
    dbl2 o;
    if (!sl_row_wave(Mh, L, G, i, v.x, v.y, dt, f, o)) nnf = 1.0;
    if (lane == 0) out[i] = o;
  }
  if (lane == 0) sw_[wv] = nnf;
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0.0;
    for (int k = 0; k < BS / 64; ++k) a += sw_[k];
    red_part(R, part, 0, a);
  }
  red_finish(R, part, sh);
}

// MacCormack advection per member (pucfem_ens_set_advection; pucfem_maccormack.hpp): the two passes of k_mc_fwd /
// k_mc_bwd (F = double: the dye) and of k_mc_fwd_vel / k_mc_bwd_vel (F = dbl2: the velocity's interleaved pairs), one
// wave per row on k_ens_sl's grid in x, with the locate members already run (sl_point, sl_locate_wave, sl_value: the
// triangle of the single path's lane-per-row locate, pucfem_locate.hpp), so ch, the record and the result hold the bits
// of the single path's.  A member whose flag on[m] is not `want` leaves at once: a block-uniform exit in front of every
// barrier and of the ticket, as in k_ens_sl_vel.  u: M x 2n (the velocity that traces), f / ch / out: M x n values of
// F, rec: M x n.
//
// Pass 1: ch = SL(f; u, +dt) and the row's T1 (a, b, d, id; id = -1: none, and ch keeps f).  The member's rows
// without T1: per-block partials, summed by red_finish in block order.  part: M x gridDim.x.
template <class F>
__global__ __launch_bounds__(BS) void k_ens_mc_fwd(MeshDev Mh, LocDev L, GridDev G, int64_t n,
                                                   const double* __restrict__ u, double dt,
                                                   const int32_t* __restrict__ on, int32_t want, const F* f,
                                                   F* __restrict__ ch, int4* __restrict__ rec, double* part, RedOut ro) {
  __shared__ double sw_[BS / 64];
  __shared__ double sh[4];
  const int32_t m = (int32_t)blockIdx.y;
  if (on[m] != want) return;
  const dbl2* um = reinterpret_cast<const dbl2*>(u) + (int64_t)m * n;
  const F* fm = f + (int64_t)m * n;
  F* chm = ch + (int64_t)m * n;
  int4* rm = rec + (int64_t)m * n;
  const RedOut R = ens_red<1>(ro, m, part);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * (BS / 64) + wv;
  double nnf = 0.0;
  if (i < n) {
    const dbl2 v = um[i];
    double xb, yb;
    sl_point(Mh, i, v.x, v.y, dt, xb, yb);
    SlTri r{};
    const bool ok = sl_locate_wave(L, G, xb, yb, r);
    if (!ok) nnf = 1.0;
    const F o = ok ? sl_value(r, xb, yb, fm) : fm[i];
    if (lane == 0) {
      chm[i] = o;
      rm[i] = ok ? make_int4(r.a, r.b, r.d, r.id) : make_int4(0, 0, 0, -1);
    }
  }
  if (lane == 0) sw_[wv] = nnf;
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0.0;
    for (int k = 0; k < BS / 64; ++k) a += sw_[k];
    red_part(R, part, 0, a);
  }
  red_finish(R, part, sh);
}
// Pass 2, its own launch (it gathers ch at the vertices of other rows' triangles): the trace with -dt, pass 1's record
// and mc_row / mc_limit (pucfem_maccormack.hpp) on (f, ch).  out aliases neither f nor ch.  The member's rows without
// T2 and its clamped values (both components of a pair count): per-block partials, summed by red_finish in block
// order.  part: M x 2 gridDim.x.
template <class F>
__global__ __launch_bounds__(BS) void k_ens_mc_bwd(MeshDev Mh, LocDev L, GridDev G, int64_t n,
                                                   const double* __restrict__ u, double dt,
                                                   const int32_t* __restrict__ on, int32_t want, const F* f,
                                                   const F* ch, F* __restrict__ out, const int4* __restrict__ rec,
                                                   double* part, RedOut ro) {
  __shared__ double sw_[2][BS / 64];
  __shared__ double sh[4];
  const int32_t m = (int32_t)blockIdx.y;
  if (on[m] != want) return;
  const dbl2* um = reinterpret_cast<const dbl2*>(u) + (int64_t)m * n;
  const F* fm = f + (int64_t)m * n;
  const F* chm = ch + (int64_t)m * n;
  F* om = out + (int64_t)m * n;
  const int4* rm = rec + (int64_t)m * n;
  const RedOut R = ens_red<2>(ro, m, part);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * (BS / 64) + wv;
  double nb2 = 0.0;
  int32_t ncl = 0;
  if (i < n) {
    const dbl2 v = um[i];
    double xb, yb;
    sl_point(Mh, i, v.x, v.y, -dt, xb, yb);
    SlTri r{};
    const bool ok2 = sl_locate_wave(L, G, xb, yb, r);
    if (!ok2) nb2 = 1.0;
    const F o = mc_row(rm[i], ok2, r, xb, yb, i, fm, chm, ncl);
    if (lane == 0) om[i] = o;
  }
  if (lane == 0) {
    sw_[0][wv] = nb2;
    sw_[1][wv] = (double)ncl;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      double a = 0.0;
      for (int k = 0; k < BS / 64; ++k) a += sw_[v][k];
      red_part(R, part, v, a);
    }
  }
  red_finish(R, part, sh);
}
// k_wsum per member, for the members whose dye moved by MacCormack (on[m] set; the others leave at once): sum w c and
// sum w of the new dye cn in the single path's grouping -- its grid in x (Ctx::nb_dye), block_rows, the lanes' strided
// accumulation, block_sum -- and red_finish, whose order over these few blocks is k_reduce's.  cn: M x n,
// part: M x 2 gridDim.x.
__global__ __launch_bounds__(BS) void k_ens_wsum(int64_t n, const int32_t* __restrict__ on,
                                                 const double* __restrict__ cn, const double* __restrict__ wmix,
                                                 double* part, RedOut ro) {
  __shared__ double sh[4];
  const int32_t m = (int32_t)blockIdx.y;
  if (!on[m]) return;
  const double* c = cn + (int64_t)m * n;
  const RedOut R = ens_red<2>(ro, m, part);
  double swc = 0.0, sw = 0.0;
  int64_t r0, r1;
  block_rows(n, r0, r1);
  for (int64_t i = r0 + threadIdx.x; i < r1; i += BS) {
    const double w = wmix[i];
    swc += w * c[i];
    sw += w;
  }
  const double a = block_sum(swc, sh), b = block_sum(sw, sh);
  if (threadIdx.x == 0) {
    red_part(R, part, 0, a);
    red_part(R, part, 1, b);
  }
  red_finish(R, part, sh);
}

// Midpoint trajectories per member (pucfem_ens_set_trajectory; pucfem_trajectory.hpp): the
// wave-per-row forms of k_trj_fwd / k_trj_bwd (F = double: the dye) and of k_trj_fwd_vel / k_trj_bwd_vel (F = dbl2: the
// velocity's interleaved pairs), on k_ens_sl's grid in x, with the locate members already run (sl_point,
// sl_locate_wave, sl_value).  The single path's sl_locate_row is, for the record locator, sl_locate_general, whose
// triangle sl_locate_wave returns (pucfem_locate.hpp): the midpoint velocity, the final point and the value hold the
// single path's bits.  A member whose flag on[m] is not `want` leaves at once (block-uniform, in front of every barrier
// and of the ticket), as in k_ens_mc_*.
//
// The two locates of a row as one loop body run twice (trj_locate's form: one inlined locate and one SlTri, so that the
// kernel keeps the registers of a one-pass kernel and no scratch).  In: (vx, vy) = u[g]; out: the velocity the row was
// traced with (in registers only), (xb, yb) and r the final point and its triangle, okm whether the midpoint was found.
__device__ __forceinline__ bool ens_trj_locate(const MeshDev& Mh, const LocDev& L, const GridDev& G, int64_t g,
                                               double& vx, double& vy, double dt, double hdt, const dbl2* um,
                                               double& xb, double& yb, SlTri& r, bool& okm) {
  bool ok = false;
  okm = true;
#pragma unroll 1
  for (int ph = 0; ph < 2; ++ph) {
    sl_point(Mh, g, vx, vy, ph == 0 ? hdt : dt, xb, yb);
    ok = sl_locate_wave(L, G, xb, yb, r);
    if (ph == 0) {
      okm = ok;
      if (ok) {
        const dbl2 w = sl_value(r, xb, yb, um);
        vx = w.x;
        vy = w.y;
      }
    }
  }
  return ok;
}
// Pass 1 (and the whole of a one-pass step): out = SL(f; w, +dt) along the midpoint velocity w, and with rec the row's
// T1 (id = -1: none, and out keeps f).  u: M x 2n, f / out: M x n values of F (out aliases neither u nor f), rec: M x n
// or null.  Per member, per-block partials summed by red_finish in block order: value 0 the rows whose final locate
// found nothing (ro.out), value 1 those whose midpoint was not found (ro.out1).  part: M x 2 gridDim.x.
template <class F>
__global__ __launch_bounds__(BS) void k_ens_trj_fwd(MeshDev Mh, LocDev L, GridDev G, int64_t n,
                                                    const double* __restrict__ u, double dt, double hdt,
                                                    const int32_t* __restrict__ on, int32_t want, const F* f,
                                                    F* __restrict__ out, int4* __restrict__ rec, double* part,
                                                    RedOut ro) {
  __shared__ double sw_[2][BS / 64];
  __shared__ double sh[4];
  const int32_t m = (int32_t)blockIdx.y;
  if (on[m] != want) return;
  const dbl2* um = reinterpret_cast<const dbl2*>(u) + (int64_t)m * n;
  const F* fm = f + (int64_t)m * n;
  F* om = out + (int64_t)m * n;
  int4* rm = rec ? rec + (int64_t)m * n : nullptr;
  const RedOut R = ens_red<2>(ro, m, part);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * (BS / 64) + wv;
  double nnf = 0.0, nmid = 0.0;
  if (i < n) {
    const dbl2 v = um[i];
    double wx = v.x, wy = v.y, xb, yb;
    SlTri r{};
    bool okm;
    const bool ok = ens_trj_locate(Mh, L, G, i, wx, wy, dt, hdt, um, xb, yb, r, okm);
    if (!ok) nnf = 1.0;
    if (!okm) nmid = 1.0;
    const F o = ok ? sl_value(r, xb, yb, fm) : fm[i];
    if (lane == 0) {
      om[i] = o;
      if (rm) rm[i] = ok ? make_int4(r.a, r.b, r.d, r.id) : make_int4(0, 0, 0, -1);
    }
  }
  if (lane == 0) {
    sw_[0][wv] = nnf;
    sw_[1][wv] = nmid;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      double a = 0.0;
      for (int k = 0; k < BS / 64; ++k) a += sw_[v][k];
      red_part(R, part, v, a);
    }
  }
  red_finish(R, part, sh);
}
// Pass 2 (MacCormack members): the same two locates from the same node with -dt and -hdt (the midpoint read from u),
// pass 1's record and mc_row on (f, ch).  out aliases neither f nor ch.  Per member, values 0..2 into ro.out: the rows
// without T2, the clamped values, the rows whose pass-2 midpoint was not found; the block that reduced copies the first
// two into cnt2 (the member's MacCormack slots of vals: thread 0 stored them itself).  part: M x 3 gridDim.x.
template <class F>
__global__ __launch_bounds__(BS) void k_ens_trj_bwd(MeshDev Mh, LocDev L, GridDev G, int64_t n,
                                                    const double* __restrict__ u, double dt, double hdt,
                                                    const int32_t* __restrict__ on, int32_t want, const F* f,
                                                    const F* ch, F* __restrict__ out, const int4* __restrict__ rec,
                                                    double* part, RedOut ro, double* __restrict__ cnt2) {
  __shared__ double sw_[3][BS / 64];
  __shared__ double sh[4];
  const int32_t m = (int32_t)blockIdx.y;
  if (on[m] != want) return;
  const dbl2* um = reinterpret_cast<const dbl2*>(u) + (int64_t)m * n;
  const F* fm = f + (int64_t)m * n;
  const F* chm = ch + (int64_t)m * n;
  F* om = out + (int64_t)m * n;
  const int4* rm = rec + (int64_t)m * n;
  const RedOut R = ens_red<3>(ro, m, part);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * (BS / 64) + wv;
  double nb2 = 0.0, nmid = 0.0;
  int32_t ncl = 0;
  if (i < n) {
    const dbl2 v = um[i];
    double wx = v.x, wy = v.y, xb, yb;
    SlTri r{};
    bool okm;
    const bool ok2 = ens_trj_locate(Mh, L, G, i, wx, wy, -dt, -hdt, um, xb, yb, r, okm);
    if (!ok2) nb2 = 1.0;
    if (!okm) nmid = 1.0;
    const F o = mc_row(rm[i], ok2, r, xb, yb, i, fm, chm, ncl);
    if (lane == 0) om[i] = o;
  }
  if (lane == 0) {
    sw_[0][wv] = nb2;
    sw_[1][wv] = (double)ncl;
    sw_[2][wv] = nmid;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int v = 0; v < 3; ++v) {
      double a = 0.0;
      for (int k = 0; k < BS / 64; ++k) a += sw_[v][k];
      red_part(R, part, v, a);
    }
  }
  if (red_finish(R, part, sh) && threadIdx.x == 0) {
    double* c2 = cnt2 + (int64_t)ENS_VALS * m;
    c2[0] = R.out[0];
    c2[1] = R.out[1];
  }
}

// k_mix2 per member: sum w (c - mu)^2 of the new dye cn (mu from vals 2 / 3), copied into c.  cn, c: M x n.
__global__ __launch_bounds__(BS) void k_ens_mix2(int64_t n, const double* __restrict__ cn, const double* __restrict__ wmix,
                                                 const double* vals, double* part, RedOut ro, double* __restrict__ c) {
  __shared__ double sh[4];
  const int32_t m = (int32_t)blockIdx.y;
  const double* cnm = cn + (int64_t)m * n;
  double* cm = c + (int64_t)m * n;
  const double* vm = vals + (int64_t)ENS_VALS * m;
  const RedOut R = ens_red(ro, m, part);
  const double swc = reduce_partials(vm + 2, 1, sh);
  const double sw = reduce_partials(vm + 3, 1, sh);
  const double mu = swc / sw;
  double acc = 0.0;
  int64_t r0, r1;
  block_rows(n, r0, r1);
  for (int64_t i = r0 + threadIdx.x; i < r1; i += BS) {
    const double ci = cnm[i];
    cm[i] = ci;
    const double d = ci - mu;
    acc += wmix[i] * (d * d);
  }
  const double t = block_sum(acc, sh);
  if (threadIdx.x == 0) red_part(R, part, 0, t);
  red_finish(R, part, sh);
}

// member m's setting of the BROWN kernels (block-uniform); a = 0 in the plain instantiation
template <bool BROWN>
__device__ __forceinline__ Brown ens_brown(const EnsBrownArg<BROWN>& eb, int32_t m) {
  if constexpr (BROWN) {
    const uint2 key = eb.key[m];
    return Brown{eb.a[m], key.x, key.y, eb.ylo, eb.yhi};
  } else {
    return Brown{0.0, 0u, 0u, 0.0, 0.0};
  }
}

// midpoint tracer steps per member (pucfem_ens_set_trajectory, PUCFEM_TRJ_TRACERS), the MID variants' argument:
// on[m] != 0: member m takes tracer_mid's velocity (a block-uniform branch, as a[m] == 0 is for BROWN); fell: the
// members' counts of their last midpoint launch (stride ENS_VALS), the tracers that had a velocity and lost their
// midpoint -- stored (not added) by every launch for the members that are on, so nothing is zeroed outside the chain
struct EnsMid {
  const int32_t* on;
  double hdt;  // 0.5 * dt, from the host
  double* fell;
};
struct EnsMidOff {};  // the Euler kernels' (empty) argument
template <bool MID>
using EnsMidArg = std::conditional_t<MID, EnsMid, EnsMidOff>;
// tracer stretching per member (pucfem_ens_set_tracer_stretch), the STRETCH variants' argument: on[m] != 0: member m's
// tracers carry F (M x ntr x 4), a block-uniform branch as MID's; a member that is off leaves its rows alone
struct EnsStretch {
  const int32_t* on;
  double* F;
};
struct EnsStretchOff {};  // the plain kernels' (empty) argument
template <bool STRETCH>
using EnsStretchArg = std::conditional_t<STRETCH, EnsStretch, EnsStretchOff>;

// k_tracer per member (one block each): the single path's locate / interpolate / move.  tx, ty, status: M x ntr.
// BROWN (pucfem_brownian.hpp): the member's amplitude and key from device memory; a block-uniform branch, a[m] == 0
// the plain move.  MID: tracer_mid itself for the members whose flag is set, and their count of the launch.
template <bool BROWN, bool MID = false, bool STRETCH = false>
__global__ __launch_bounds__(BS) void k_ens_tracer(MeshDev Mh, GridDev G, int64_t n, const double* __restrict__ u,
                                                   int32_t ntr, double* tx, double* ty, double* status,
                                                   int32_t* capstep, int32_t* stepctr, double dt, double cx, double cy,
                                                   double capture, double* vals, EnsBrownArg<BROWN> eb,
                                                   EnsMidArg<MID> em,
                                                   EnsStretchArg<STRETCH> es = EnsStretchArg<STRETCH>{}) {
  __shared__ double sh[4];
  const int32_t m = (int32_t)blockIdx.y;
  const double* ux = u + (int64_t)m * 2 * n;
  const double* uy = ux + 1;
  double* txm = tx + (int64_t)m * ntr;
  double* tym = ty + (int64_t)m * ntr;
  double* stm = status + (int64_t)m * ntr;
  int32_t* cpm = capstep + (int64_t)m * ntr;
  const int32_t stepno = stepctr[m] + 1;  // (the member's own count: k_tracer's)
  const Brown br = ens_brown<BROWN>(eb, m);
  double eaten = 0.0;
  [[maybe_unused]] int32_t fell = 0;
  [[maybe_unused]] bool mid = false;
  if constexpr (MID) mid = em.on[m] != 0;
  [[maybe_unused]] bool str = false;
  [[maybe_unused]] double* Fm = nullptr;
  if constexpr (STRETCH) {
    str = es.on[m] != 0;
    Fm = es.F + (int64_t)m * 4 * ntr;
  }
  for (int32_t k = threadIdx.x; k < ntr; k += blockDim.x) {
    if (BROWN && br.a != 0.0) {
      if (stm[k] == 1.0) {
        eaten += 1.0;
        continue;
      }
    }
    const double px = txm[k], py = tym[k];
    double vx = NAN, vy = NAN;
    if constexpr (STRETCH) {  // (the same velocity; a member whose flag is on: F[k] <- J F[k])
      double hdt = 0.0;
      if constexpr (MID) hdt = em.hdt;
      tracer_velocity<MID, true>(Mh, G, ux, uy, px, py, mid, hdt, dt, str, Fm, k, vx, vy, fell);
    } else {
      const int32_t found = tracer_locate(Mh, G, px, py);
      if (found >= 0) tracer_interp(Mh, found, ux, uy, VS, px, py, vx, vy);
      if constexpr (MID) {
        if (mid && !tracer_mid(Mh, G, ux, uy, px, py, em.hdt, vx, vy) && found >= 0) ++fell;
      }
    }
    if (BROWN && br.a != 0.0)
      eaten += tracer_move_brownian(txm, tym, stm, cpm, k, px, py, vx, vy, dt, cx, cy, capture, stepno, br);
    else
      eaten += tracer_move(txm, tym, stm, cpm, k, vx, vy, dt, cx, cy, capture, stepno);
  }
  if constexpr (MID) {
    const double f = block_sum((double)fell, sh);
    if (threadIdx.x == 0 && mid) em.fell[(int64_t)ENS_VALS * m] = f;
  }
  const double t = block_sum(eaten, sh);
  if (threadIdx.x == 0) {
    vals[(int64_t)ENS_VALS * m + 6] = t;
    stepctr[m] = stepno;
  }
}
// k_tracer_cloud per member: grid (blocks, M), the member's partials, ticket and step count (ro.out: vals + 6; MID:
// value 1 of the reduction is the member's fell-back count, into ro.out1)
template <bool BROWN, bool MID = false, bool STRETCH = false>
__global__ __launch_bounds__(BS) void k_ens_tracer_cloud(MeshDev Mh, GridDev G, int64_t n, const double* __restrict__ u,
                                                         int32_t ntr, double* tx, double* ty, double* status,
                                                         int32_t* capstep, int32_t* stepctr, double dt, double cx,
                                                         double cy, double capture, double* part, RedOut ro,
                                                         EnsBrownArg<BROWN> eb, EnsMidArg<MID> em,
                                                         EnsStretchArg<STRETCH> es = EnsStretchArg<STRETCH>{}) {
  __shared__ double sh[4];
  const int32_t m = (int32_t)blockIdx.y;
  const double* ux = u + (int64_t)m * 2 * n;
  const double* uy = ux + 1;
  double* txm = tx + (int64_t)m * ntr;
  double* tym = ty + (int64_t)m * ntr;
  double* stm = status + (int64_t)m * ntr;
  int32_t* cpm = capstep + (int64_t)m * ntr;
  RedOut R = ens_red(ro, m, part);
  const int32_t stepno = stepctr[m] + 1;
  const Brown br = ens_brown<BROWN>(eb, m);
  double eaten = 0.0;
  [[maybe_unused]] int32_t fell = 0;
  [[maybe_unused]] bool mid = false;
  if constexpr (MID) {
    mid = em.on[m] != 0;
    if (!mid) R.nv = 1;  // (the launch reduces two values: a member off keeps its count of its last midpoint launch)
  }
  [[maybe_unused]] bool str = false;
  [[maybe_unused]] double* Fm = nullptr;
  if constexpr (STRETCH) {
    str = es.on[m] != 0;
    Fm = es.F + (int64_t)m * 4 * ntr;
  }
  for (int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x; i < ntr; i += (int64_t)gridDim.x * BS) {
    const int32_t k = (int32_t)i;
    if (BROWN && br.a != 0.0) {
      if (stm[k] == 1.0) {  // (this lane's iteration only: red_finish's barrier and ticket are behind the loop)
        eaten += 1.0;
        continue;
      }
    }
    const double px = txm[k], py = tym[k];
    double vx = NAN, vy = NAN;
    if constexpr (STRETCH) {  // (the same velocity; a member whose flag is on: F[k] <- J F[k])
      double hdt = 0.0;
      if constexpr (MID) hdt = em.hdt;
      tracer_velocity<MID, true>(Mh, G, ux, uy, px, py, mid, hdt, dt, str, Fm, k, vx, vy, fell);
    } else {
      const int32_t found = tracer_locate(Mh, G, px, py);
      if (found >= 0) tracer_interp(Mh, found, ux, uy, VS, px, py, vx, vy);
      if constexpr (MID) {
        if (mid && !tracer_mid(Mh, G, ux, uy, px, py, em.hdt, vx, vy) && found >= 0) ++fell;
      }
    }
    if (BROWN && br.a != 0.0)
      eaten += tracer_move_brownian(txm, tym, stm, cpm, k, px, py, vx, vy, dt, cx, cy, capture, stepno, br);
    else
      eaten += tracer_move(txm, tym, stm, cpm, k, vx, vy, dt, cx, cy, capture, stepno);
  }
  if constexpr (MID) {
    const double f = block_sum((double)fell, sh);
    if (threadIdx.x == 0 && mid) red_part(R, part, 1, f);
  }
  const double t = block_sum(eaten, sh);
  if (threadIdx.x == 0) red_part(R, part, 0, t);
  if (red_finish(R, part, sh) && threadIdx.x == 0) stepctr[m] = stepno;
}

// Dye channels per member (pucfem_ens_set_dyes): the with-channels forms of k_ens_sl,
// k_ens_mc_fwd / k_ens_mc_bwd<double> and k_ens_trj_fwd / k_ens_trj_bwd<double>, launched in their place while the
// ensemble carries K > 0 channels.  Their grid, their block-uniform exit for members whose flag is not `want` and their
// locate sequence (sl_point, sl_locate_wave; MID: ens_trj_locate), so the row's triangle is theirs.  After the locate
// every lane of the wave holds the triangle: lane 0 takes the member's c and lane k (1..K) channel k - 1, each with the
// single field's expression (sl_value, the row's own value, mc_row) and one store; lanes above K compute lane 0's value
// again and store nothing.  Channel k of member m is the plain vector at (m K + k) n of dy (M x K x n).
//
// Pass 1 (and the whole of a one-pass step).  c -> cout and dy -> dyout; rec (or null): the row's T1.  Three uses:
//   wmix != null (the plain SL members, MID = false): k_ens_sl's three values in its grouping -- sum w c of lane 0's
//     value, sum w, the not-found rows; per wave, thread 0 over the block's waves, red_finish in block order
//   MID = false, wmix == null (MacCormack pass 1): k_ens_mc_fwd's one value, the rows without T1
//   MID = true: k_ens_trj_fwd's two, the rows whose final locate found nothing and those without midpoint (ro.out1)
// on: the members' flags (null: every member's is 0).  part: M x ro.nv gridDim.x.
template <bool MID>
__global__ __launch_bounds__(BS) void k_ens_dye_fwd(MeshDev Mh, LocDev L, GridDev G, int64_t n,
                                                    const double* __restrict__ u, double dt, double hdt,
                                                    const int32_t* __restrict__ on, int32_t want, int32_t K,
                                                    const double* c, const double* dy, double* __restrict__ cout,
                                                    double* __restrict__ dyout, int4* __restrict__ rec,
                                                    const double* __restrict__ wmix, double* part, RedOut ro) {
  __shared__ double sw_[3][BS / 64];
  __shared__ double sh[4];
  const int32_t m = (int32_t)blockIdx.y;
  if ((on ? on[m] : 0) != want) return;
  const dbl2* um = reinterpret_cast<const dbl2*>(u) + (int64_t)m * n;
  RedOut R = ro;
  R.out = ro.out + (int64_t)ENS_VALS * m;
  R.out1 = ro.out1 ? ro.out1 + (int64_t)ENS_VALS * m : nullptr;
  R.cnt = ro.cnt + m;
  R.stride = (int)gridDim.x;
  part += (int64_t)m * ro.nv * gridDim.x;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int fl = lane <= K ? lane : 0;  // this lane's field: 0 the member's c, k the channel k - 1
  const int64_t fo = fl == 0 ? (int64_t)m * n : ((int64_t)m * K + (fl - 1)) * n;
  const double* fin = (fl == 0 ? c : dy) + fo;
  double* fout = (fl == 0 ? cout : dyout) + fo;
  int4* rm = rec ? rec + (int64_t)m * n : nullptr;
  const int64_t i = (int64_t)blockIdx.x * (BS / 64) + wv;
  double swc = 0.0, sw = 0.0, nnf = 0.0, nmid = 0.0;
  if (i < n) {
    const dbl2 v = um[i];
    double xb, yb;
    SlTri r{};
    bool ok;
    if constexpr (MID) {
      double wx = v.x, wy = v.y;
      bool okm;
      ok = ens_trj_locate(Mh, L, G, i, wx, wy, dt, hdt, um, xb, yb, r, okm);
      if (!okm) nmid = 1.0;
    } else {
      sl_point(Mh, i, v.x, v.y, dt, xb, yb);
      ok = sl_locate_wave(L, G, xb, yb, r);
    }
    if (!ok) nnf = 1.0;
    const double o = ok ? sl_value(r, xb, yb, fin) : fin[i];
    if (lane <= K) fout[i] = o;
    if (lane == 0 && rm) rm[i] = ok ? make_int4(r.a, r.b, r.d, r.id) : make_int4(0, 0, 0, -1);
    if (wmix) {
      const double w = wmix[i];
      sw = w;
      swc = w * o;  // (read from lane 0 below: the member's c)
    }
  }
  if (lane == 0) {
    if (wmix) {
      sw_[0][wv] = swc;
      sw_[1][wv] = sw;
      sw_[2][wv] = nnf;
    } else {
      sw_[0][wv] = nnf;
      sw_[1][wv] = nmid;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int v = 0; v < R.nv; ++v) {
      double a = 0.0;
      for (int k = 0; k < BS / 64; ++k) a += sw_[v][k];
      red_part(R, part, v, a);
    }
  }
  red_finish(R, part, sh);
}
// Pass 2 (MacCormack members), its own launch: the trace with -dt (MID: -dt and -hdt), pass 1's record and mc_row on
// the lane's (field, ch).  c / ch / cout: M x n, dy / dch / dyout: M x K x n; the outputs alias none of the inputs.
// The wave's clamp count is the sum of the K + 1 lanes' counts (integers in doubles: the order is free).  Values
// 0..nv-1 into ro.out: the rows without T2, the clamped values, MID: the rows whose pass-2 midpoint was not found; MID:
// the block that reduced copies the first two into cnt2 (k_ens_trj_bwd's).  part: M x ro.nv gridDim.x.
template <bool MID>
__global__ __launch_bounds__(BS) void k_ens_dye_bwd(MeshDev Mh, LocDev L, GridDev G, int64_t n,
                                                    const double* __restrict__ u, double dt, double hdt,
                                                    const int32_t* __restrict__ on, int32_t want, int32_t K,
                                                    const double* c, const double* ch, const double* dy,
                                                    const double* dch, double* __restrict__ cout,
                                                    double* __restrict__ dyout, const int4* __restrict__ rec,
                                                    double* part, RedOut ro, double* __restrict__ cnt2) {
  __shared__ double sw_[3][BS / 64];
  __shared__ double sh[4];
  const int32_t m = (int32_t)blockIdx.y;
  if (on[m] != want) return;
  const dbl2* um = reinterpret_cast<const dbl2*>(u) + (int64_t)m * n;
  RedOut R = ro;
  R.out = ro.out + (int64_t)ENS_VALS * m;
  R.cnt = ro.cnt + m;
  R.stride = (int)gridDim.x;
  part += (int64_t)m * ro.nv * gridDim.x;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int fl = lane <= K ? lane : 0;
  const int64_t fo = fl == 0 ? (int64_t)m * n : ((int64_t)m * K + (fl - 1)) * n;
  const double* fin = (fl == 0 ? c : dy) + fo;
  const double* chin = (fl == 0 ? ch : dch) + fo;
  double* fout = (fl == 0 ? cout : dyout) + fo;
  const int4* rm = rec + (int64_t)m * n;
  const int64_t i = (int64_t)blockIdx.x * (BS / 64) + wv;
  double nb2 = 0.0, nmid = 0.0, ncl = 0.0;
  if (i < n) {
    const dbl2 v = um[i];
    double xb, yb;
    SlTri r{};
    bool ok2;
    if constexpr (MID) {
      double wx = v.x, wy = v.y;
      bool okm;
      ok2 = ens_trj_locate(Mh, L, G, i, wx, wy, -dt, -hdt, um, xb, yb, r, okm);
      if (!okm) nmid = 1.0;
    } else {
      sl_point(Mh, i, v.x, v.y, -dt, xb, yb);
      ok2 = sl_locate_wave(L, G, xb, yb, r);
    }
    if (!ok2) nb2 = 1.0;
    int32_t hit = 0;
    const double o = mc_row(rm[i], ok2, r, xb, yb, i, fin, chin, hit);
    if (lane <= K) fout[i] = o;
    ncl = wave_sum(lane <= K ? (double)hit : 0.0);
  }
  if (lane == 0) {
    sw_[0][wv] = nb2;
    sw_[1][wv] = ncl;
    sw_[2][wv] = nmid;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int v = 0; v < R.nv; ++v) {
      double a = 0.0;
      for (int k = 0; k < BS / 64; ++k) a += sw_[v][k];
      red_part(R, part, v, a);
    }
  }
  const bool red = red_finish(R, part, sh);
  if constexpr (MID) {
    if (red && threadIdx.x == 0) {
      double* c2 = cnt2 + (int64_t)ENS_VALS * m;
      c2[0] = R.out[0];
      c2[1] = R.out[1];
    }
  }
}
// the channels' next set into their current set behind the advection (a one-step graph holds fixed pointers), as
// k_ens_mix2 copies cn into c: a streaming copy of count doubles
__global__ __launch_bounds__(BS) void k_ens_dye_copy(int64_t count, const double* __restrict__ src,
                                                     double* __restrict__ dst) {
  for (int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x; i < count; i += (int64_t)gridDim.x * BS) dst[i] = src[i];
}
// pucfem_ens_dyes_mixing: the reduction of pucfem_mixing_index for every (member, channel) plane f (planes x n) in one
// launch per stage, blockIdx.y the plane, gridDim.x the single reduction's grid (Ctx::nb_rows): k_dot2's block sums
// (sum w c, and sum w as w * 1) and k_mix2's (sum w (c - mu)^2, mu from the plane's reduced sums), the blocks' partials
// summed by red_finish in block order -- k_reduce's order over these few blocks.  vals: planes x ENS_VALS, slots 2, 3
// (stage 0) and 5 (stage 1); part: planes x 2 gridDim.x; cnt: planes.
__global__ __launch_bounds__(BS) void k_ens_dyes_mix(int64_t n, int stage, const double* __restrict__ f,
                                                     const double* __restrict__ wmix, double* vals, double* part,
                                                     unsigned* cnt) {
  __shared__ double sh[4];
  const int64_t q = blockIdx.y;
  const double* c = f + q * n;
  double* vq = vals + (int64_t)ENS_VALS * q;
  part += q * 2 * gridDim.x;
  const RedOut R{vq + (stage == 0 ? 2 : 5), nullptr, cnt + q, stage == 0 ? 2 : 1, (int)gridDim.x, 0u};
  int64_t r0, r1;
  block_rows(n, r0, r1);
  if (stage == 0) {
    double s1 = 0.0, s2 = 0.0;
    for (int64_t i = r0 + threadIdx.x; i < r1; i += BS) {
      s1 += wmix[i] * c[i];
      s2 += wmix[i] * 1.0;
    }
    const double t1 = block_sum(s1, sh), t2 = block_sum(s2, sh);
    if (threadIdx.x == 0) {
      red_part(R, part, 0, t1);
      red_part(R, part, 1, t2);
    }
  } else {
    const double mu = vq[2] / vq[3];
    double acc = 0.0;
    for (int64_t i = r0 + threadIdx.x; i < r1; i += BS) {
      const double d = c[i] - mu;
      acc += wmix[i] * (d * d);
    }
    const double t = block_sum(acc, sh);
    if (threadIdx.x == 0) red_part(R, part, 0, t);
  }
  red_finish(R, part, sh);
}
// ... and the planes' (I, mu, var): k_stats' arithmetic (stats_body) on each plane's values; out: planes x 3
__global__ void k_ens_dyes_stats(int32_t planes, const double* vals, double* out) {
  const int32_t q = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
  if (q >= planes) return;
  double r[8];
  stats_body(vals + (int64_t)ENS_VALS * q, r, 4);
  out[3 * q] = r[2];
  out[3 * q + 1] = r[3];
  out[3 * q + 2] = r[4];
}

// the step's record of every member (k_stats_ring per member): slot count[m] of the ring (steps x M x 8)
__global__ void k_ens_record(int32_t M, const double* vals, double* ring, int* count) {
  const int32_t m = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
  if (m >= M) return;
  const int k = count[m];
  stats_body(vals + (int64_t)ENS_VALS * m, ring + 8 * ((int64_t)k * M + m), 7);
  count[m] = k + 1;
}

}  // namespace dev
}  // namespace pucfem
