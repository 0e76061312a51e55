// libpucfem C ABI (include/pucfem.h): context, device memory, solver orchestration, RCCL halo /
// all-reduce, and the Stokes / heat / Poisson step loops.  One HIP stream per context; every
// kernel of a step is enqueued back to back and the host synchronises only to poll CG
// convergence (once per chunk of iterations) and to return results.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <memory>
#include <numeric>
#include <stdexcept>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "pucfem.h"
#include "pucfem_comm.hpp"
#include "pucfem_host.hpp"
#include "pucfem_kernels.hpp"
#include "pucfem_kernels_impl.hpp"
#include "pucfem_ensemble.hpp"
#include "pucfem_sample.hpp"
#include "pucfem_streamline.hpp"
#include "pucfem_dye_channels.hpp"
#include "pucfem_inertia.hpp"
#include "pucfem_force.hpp"
#include "pucfem_maccormack.hpp"
#include "pucfem_trajectory.hpp"
#include "pucfem_stroke.hpp"
#include "pucfem_loads.hpp"

using namespace pucfem;
using namespace pucfem::dev;

// Kernel launches of this thread (pucfem_counters): every launch of the library goes through
// hipLaunchKernelGGL (redefined here to count) or Ctx::klaunch.
namespace {
thread_local int64_t g_nlaunch = 0;
}
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernelName, ...) \
  do {                                      \
    ++g_nlaunch;                            \
    hipLaunchKernelGGLInternal((kernelName), __VA_ARGS__); \
  } while (0)

// LocalComm reduction (fixed rank order -> identical result on every rank)
__global__ void pucfem::k_comm_reduce(int world, int is_max, size_t n, const double* const* bufs, double* out) {
  for (size_t i = threadIdx.x; i < n; i += blockDim.x) {
    double a = bufs[0][i];
    for (int r = 1; r < world; ++r) a = is_max ? fmax(a, bufs[r][i]) : a + bufs[r][i];
    out[i] = a;
  }
}

namespace {

constexpr int64_t DENSE_MAX = 1500;  // small-mesh direct-solve threshold (mesh_fine: 1,067 nodes)
static_assert(DENSE_MAX <= dev::DENSE_LDS, "the dense solves stage their vectors in LDS");

struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

#define HIPCHK(x)                                                                                 \
  do {                                                                                            \
    hipError_t e_ = (x);                                                                          \
    if (e_ != hipSuccess)                                                                         \
      throw Error(PUCFEM_EHIP, std::string(#x) + ": " + hipGetErrorString(e_));                   \
  } while (0)
#define NCCLCHK(x)                                                                                \
  do {                                                                                            \
    ncclResult_t r_ = (x);                                                                        \
    if (r_ != ncclSuccess) throw Error(PUCFEM_ENCCL, std::string(#x) + ": " + ncclGetErrorString(r_)); \
  } while (0)
#define KCHK() HIPCHK(hipGetLastError())

std::string g_err;  // errors of context-free calls

struct DevSell {
  int64_t* off = nullptr;
  int32_t* w = nullptr;
  int32_t* col = nullptr;
  int16_t* c16 = nullptr;  // int16 column deltas (square operators whose band fits), else null
  int64_t nslices = 0, nrows = 0, nnz = 0, padded = 0;
  int32_t wrap = 0;        // c16 modulus (local vector length)
  int32_t* rows = nullptr; // row list (lattice operators: the skeleton rows), else null
  int64_t n_own = 0;       // owned rows of the vector space (0: nrows)
  // deep halos (Sell::gk0): slices [nslices, nslices_g) hold ghost rows one layer out, which the launches that
  // compute them redundantly (step pairs, residuals, last smoothing steps on W > 1 ranks) include: with_ghosts()
  int64_t nslices_g = 0;
  SellDev view() const { return SellDev{off, w, col, nslices, nrows, c16, wrap, rows, n_own ? n_own : nrows}; }
  bool has_ghost_rows() const { return nslices_g > nslices; }
  DevSell with_ghosts() const {
    DevSell d = *this;
    if (nslices_g > nslices) d.nslices = nslices_g;
    return d;
  }
  // after a row-listed upload of S: the own rows' slices only by default, the ghost rows' ones behind with_ghosts()
  void ghost_slices(const pucfem::Sell& S) {
    if (S.gk0 < 0) return;
    nslices_g = S.nslices;
    nslices = S.nslices_own;
    nrows = S.nrows - (int64_t)S.grow.size();
  }
  double idx_bytes() const { return c16 ? 2.0 : 4.0; }  // per stored entry
  double row_bytes() const { return rows ? 4.0 : 0.0; }  // per row (the row list)
  int64_t own() const { return n_own ? n_own : nrows; }   // rows of the vector space
};

// A lattice operator's face part on the host (pucfem_lattice.hpp): the FaceDev image and its work
// items.  Partial-producing launches cap the face blocks (the partial arrays hold MAXB blocks in all;
// at L7 every item still gets its own block), the others give every item a block.
constexpr int32_t FACE_PART_BLOCKS = MAXB - 8192;
struct HFace {
  FaceDev d{};
  int32_t items = 0;
  int64_t rows = 0;  // face-interior rows (algorithmic bytes)
  FaceDev part() const {
    FaceDev f = d;
    f.nb = std::min(items, FACE_PART_BLOCKS);
    return f;
  }
  FaceDev full() const {
    FaceDev f = d;
    f.nb = items;
    return f;
  }
};
// An ensemble (pucfem_ens_*, pucfem_ensemble.hpp): M members stepped together on the context's shared small-mesh
// operators.  It owns its state (member-major, the context's internal numbering), reduction buffers, record ring
// and graphs; the context's own fields, graphs and records are not touched.
struct Ens {
  int32_t M = 0, ntr = 0;
  int64_t n = 0, dstride = 0, steps = 0;
  size_t bytes = 0;
  double *u = nullptr, *us = nullptr, *p = nullptr, *p2 = nullptr, *braw = nullptr, *c = nullptr, *cn = nullptr;
  double *dval = nullptr, *trx = nullptr, *try_ = nullptr, *trs = nullptr, *vals = nullptr;
  double *part_d = nullptr, *part_sl = nullptr, *part_mx = nullptr, *ring = nullptr;
  unsigned* cnt = nullptr;  // ticket counters: 4 launch sites (divergence, advection, mixing, tracer cloud) x M
  int32_t* trcap = nullptr;   // capture steps (M x ntr, -1: not captured)
  int32_t* trstep = nullptr;  // per member: tracer steps since its tracers were set
  double* part_tr = nullptr;  // k_ens_tracer_cloud's partials
  // vorticity and flow summaries (k_ens_curl), allocated at first use and kept: the members' vorticity (M x n), its
  // partials (M x 4 nb_div), the reduced values (M x ENS_VALS, slots 0..3) and the launch's ticket counters (M)
  double *vort = nullptr, *part_curl = nullptr, *flow = nullptr;
  unsigned* cnt_curl = nullptr;
  // inertia per member (pucfem_ens_set_inertia; k_ens_sl_vel), allocated when a flag is first switched on and kept:
  // the members' u_a (M x 2n), the flags as the kernels read them (M), the launch's partials (M x nb_sl) and ticket
  // counters (M).  A member's not-found count of its last inertial launch is slot 10 of its vals.
  double *ua = nullptr, *part_adv = nullptr;
  int32_t* adv_on_dev = nullptr;
  unsigned* cnt_adv = nullptr;
  size_t adv_bytes = 0;
  std::vector<int32_t> adv_on;     // the flags (empty: never enabled)
  std::vector<int64_t> adv_steps;  // per member: inertial steps since it was switched on
  std::vector<double> adv_vals;    // host copy of vals, current while !adv_stale (the not-found counts)
  bool adv_stale = true;
  int adv_any = 0;                 // members with their flag on
  bool chain_adv = false;          // the captured graphs hold the inertial launch
  // MacCormack advection per member (pucfem_ens_set_advection; k_ens_mc_fwd / k_ens_mc_bwd / k_ens_wsum), one set of
  // buffers for the dye and one for the velocity, each allocated when its scheme is first switched on and kept: the
  // members' ch (M x n doubles / M x 2n), pass 1's records (M x n int4), the partials of the set's launches and their
  // ticket counters.  The dye's flags as the kernels read them are mc_on_dev (M); the velocity's are the value
  // ENS_ADV_MC of adv_on_dev.  A member's counts are slots 4, 11, 12 (dye) and 10, 13, 14 (velocity) of its vals.
  double *mc_ch = nullptr, *mc_part = nullptr, *mc_part_ws = nullptr;
  double *mcv_ch = nullptr, *mcv_part = nullptr;
  int4 *mc_rec = nullptr, *mcv_rec = nullptr;
  int32_t* mc_on_dev = nullptr;
  unsigned *mc_cnt = nullptr, *mcv_cnt = nullptr;  // 3 M (pass 1, pass 2, sums) / 2 M
  size_t mc_bytes = 0;
  std::vector<int32_t> mc_dye, mc_vel;       // the schemes (empty: never switched on)
  std::vector<int64_t> mc_steps, mcv_steps;  // per member: MacCormack steps since the scheme was switched on
  int mc_dye_any = 0;                        // members whose dye moves by MacCormack
  int mc_vel_any = 0;                        // members with inertia on whose velocity does
  bool chain_mcd = false, chain_mcv = false; // the captured graphs hold the dye's / the velocity's MacCormack launches
  int nb_ws = 1;                             // blocks in x of k_ens_wsum: the single path's k_wsum grid
  // midpoint trajectories per member (pucfem_ens_set_trajectory; k_ens_trj_fwd / k_ens_trj_bwd and the MID tracer
  // kernels), allocated when a part is first switched on and kept: the members' counts (M x ENS_VALS, the slots
  // ENS_TRJ_*) and the launches' ticket counters (4 M: dye pass 1 / 2, velocity pass 1 / 2); per part the launches'
  // partials (M x 5 nb_sl) or the tracers' flags as the kernels read them (M).  The dye's order rides in mc_on_dev
  // (ENS_DYE_*), the velocity's in adv_on_dev (ENS_ADV_*); a MacCormack-and-midpoint member uses the MacCormack set's
  // ch and records.
  double *trj_vals = nullptr, *trj_part_d = nullptr, *trj_part_v = nullptr;
  unsigned* trj_cnt = nullptr;
  int32_t* trj_trc_dev = nullptr;
  size_t trj_bytes = 0;
  std::vector<int32_t> trj_dye, trj_vel, trj_trc;            // the orders (empty: never switched on)
  std::vector<int64_t> trjd_steps, trjv_steps, trjt_steps;   // per member: steps taken with the part on
  std::vector<double> trj_host;                              // host copy of trj_vals, current while !trj_stale
  bool trj_stale = true;
  int dye_n[4] = {0, 0, 0, 0};     // members per dye flag ENS_DYE_*
  int vel_n[5] = {0, 0, 0, 0, 0};  // members per inertial flag ENS_ADV_*
  int trjt_any = 0;                // members whose tracers take the midpoint
  int chain_trj = 0;               // the midpoint launches the captured graphs hold (trj_chain's mask)
  int trj_chain() const {
    return (dye_n[2] > 0 ? 1 : 0) | (dye_n[3] > 0 ? 2 : 0) | (vel_n[3] > 0 ? 4 : 0) | (vel_n[4] > 0 ? 8 : 0) |
           (trjt_any > 0 ? 16 : 0);
  }
  // body forces per member (pucfem_ens_set_force, pucfem_ens_set_buoyancy; k_ens_force_rhs), allocated when a member
  // is first forced and kept: the members' r (M x 2n), their term masks (M) and parameters (M x ENS_FORCE_PARM) as
  // the kernel reads them; the nodal planes (M x 2n) when a member is first given a field
  double *frhs = nullptr, *fparm = nullptr, *fnod = nullptr;
  int32_t* fmask_dev = nullptr;
  size_t force_bytes = 0;
  std::vector<int32_t> fmask;      // the masks (empty: never forced)
  std::vector<double> fpar;        // the parameters
  std::vector<int64_t> fsteps;     // per member: forced steps since its setting last changed
  int force_any = 0;               // members with a force
  bool chain_force = false;        // the captured graphs hold the force launch ...
  bool chain_fnod = false;         // ... with the nodal planes' pointer
  // Brownian tracers per member (pucfem_ens_set_tracer_diffusion; the BROWN tracer kernels), allocated when a member
  // is first switched on and kept: the members' amplitudes sqrt(6 D dt) and Philox keys as the kernels read them (M
  // each); a[m] == 0 is the plain move
  double* br_a = nullptr;
  uint2* br_key = nullptr;
  std::vector<double> br_D;        // the settings (empty: never enabled)
  std::vector<uint64_t> br_seed;
  int br_any = 0;                  // members with D > 0
  bool chain_br = false;           // the captured graphs hold the BROWN tracer launch
  // time-dependent strokes per member (pucfem_ens_set_stroke; k_ens_stroke_bc), allocated when a member is first given
  // one and kept: the members' parameters (M x ENS_STROKE_PARM) and step counters (M) as the kernel reads them, their
  // tables one behind the other (sk_cap doubles, grown by reallocation), and the shared shapes, directions and value
  // positions of the driven entries.  dval0: the values pucfem_ens_create uploaded, which clearing a stroke restores.
  int64_t *sk_parm = nullptr, *sk_ctr = nullptr;
  double *sk_tab = nullptr, *sk_shape = nullptr, *sk_dir = nullptr;
  int32_t* sk_q = nullptr;
  size_t sk_cap = 0, stroke_bytes = 0;
  int32_t sk_n = 0;                          // driven entries (shared)
  int sk_K = 0;                              // modes of the shared shapes
  std::vector<int64_t> sk_par;               // the parameters (empty: never stroked)
  std::vector<std::vector<double>> sk_amp;   // the members' tables
  std::vector<int32_t> sk_nodes;             // the shared driven nodes (caller numbering), shapes and directions
  std::vector<double> sk_shape_h, sk_dir_h, dval0;
  int stroke_any = 0;                        // members with a stroke
  bool chain_stroke = false;                 // the captured graphs hold the stroke launch
  // dye channels per member (pucfem_ens_set_dyes; k_ens_dye_fwd / k_ens_dye_bwd / k_ens_dye_copy), the same K for
  // every member: the current and the next set (M x K x n each, channel k of member m at (m K + k) n), the MacCormack
  // set's ch of the channels (the same size, allocated by ens_dye_ch_fit when a member's dye scheme is on while K > 0)
  // and what pucfem_ens_dyes_mixing reduces with (per plane: ENS_VALS values, 2 nb_mix partials, a ticket counter, the
  // three results).  Not in `allocs`: pucfem_ens_set_dyes frees them when K changes.
  // swimmer loads per member (pucfem_swimmer_loads, pucfem_set_loads_record; k_loads with the member in blockIdx.y),
  // allocated at first use and kept: the launch's partials (M x LOADS_NV grid), the reduced values (M x ENS_VALS), the
  // per-edge values (M x E x LOADS_EV) and ticket counters (M).  The record's ring (M x cap rows) and row counts (M)
  // are not in `allocs`: a changed capacity frees them.  ld_cap: the capacity the ring was made for (the context's).
  double *ld_part = nullptr, *ld_out = nullptr, *ld_eout = nullptr, *ld_ring = nullptr;
  unsigned* ld_cnt = nullptr;
  int64_t* ld_count = nullptr;
  int32_t ld_cap = 0;
  void drop_loads_ring() {
    for (void* q : {(void*)ld_ring, (void*)ld_count})
      if (q) (void)hipFree(q);
    ld_ring = nullptr;
    ld_count = nullptr;
    ld_cap = 0;
  }
  int dy_K = 0;
  double *dy_cur = nullptr, *dy_nxt = nullptr, *dy_ch = nullptr;
  double *dy_mvals = nullptr, *dy_mpart = nullptr, *dy_mout = nullptr;
  unsigned* dy_mcnt = nullptr;
  size_t dy_bytes = 0;
  std::vector<int64_t> dy_steps;             // per member: channel steps since its channels were last set
  void drop_dyes() {
    for (void* q : {(void*)dy_cur, (void*)dy_nxt, (void*)dy_ch, (void*)dy_mvals, (void*)dy_mpart, (void*)dy_mout,
                    (void*)dy_mcnt})
      if (q) (void)hipFree(q);
    dy_cur = dy_nxt = dy_ch = dy_mvals = dy_mpart = dy_mout = nullptr;
    dy_mcnt = nullptr;
    dy_K = 0;
    dy_bytes = 0;
    dy_steps.clear();
  }
  // tracer stretching per member (pucfem_ens_set_tracer_stretch; the STRETCH tracer kernels and k_tracer_stretch),
  // allocated when a member is first switched on and kept: the members' F (M x ntr x 4, identity rows for a member that
  // is off), their flags as the kernels read them (M) and what the summary reduces with (per member STRETCH_NV
  // TRACER_CLOUD_MAXB partials, STRETCH_NV values and a ticket)
  double *str_F = nullptr, *str_part = nullptr, *str_out = nullptr;
  int32_t* str_on_dev = nullptr;
  unsigned* str_cnt = nullptr;
  size_t str_bytes = 0;
  std::vector<int32_t> str_on;     // the flags (empty: never switched on)
  std::vector<int64_t> str_steps;  // per member: tracer steps taken with it on since its F was last reset
  int str_any = 0;                 // members with their flag on
  bool chain_str = false;          // the captured graphs hold the STRETCH tracer launch
  int nb_tr = 1;             // blocks in x of the tracer launch (1: k_ens_tracer)
  int tr_blocks = 0, tr_threads = 0;  // the last tracer launch (pucfem_tracer_info)
  int* count = nullptr;     // per member: records in the ring
  int ring_steps = 0;
  int gx_dense = 1, nb_div = 1, nb_sl = 1, nb_mix = 1;
  size_t lds_mv = 0, lds_pres = 0;
  hipGraph_t graph = nullptr, graph_k = nullptr;
  hipGraphExec_t gexec = nullptr, gexec_k = nullptr;
  std::vector<void*> allocs;
  template <class T>
  T* alloc(size_t count_, hipStream_t st) {
    void* q = nullptr;
    const size_t b = sizeof(T) * std::max<size_t>(1, count_);
    HIPCHK(hipMalloc(&q, b));
    allocs.push_back(q);
    HIPCHK(hipMemsetAsync(q, 0, b, st));
    bytes += b;
    return (T*)q;
  }
  // the cached step graphs (the caller has synchronised the stream): the next pucfem_ens_step captures again
  void drop_graphs() {
    if (gexec) (void)hipGraphExecDestroy(gexec);
    if (graph) (void)hipGraphDestroy(graph);
    if (gexec_k) (void)hipGraphExecDestroy(gexec_k);
    if (graph_k) (void)hipGraphDestroy(graph_k);
    graph = graph_k = nullptr;
    gexec = gexec_k = nullptr;
  }
  ~Ens() {
    drop_graphs();
    drop_dyes();
    drop_loads_ring();
    for (void* a : allocs) (void)hipFree(a);
  }
};

// f(std::true_type) when A carries int16 columns, f(std::false_type) otherwise: one launch site
// instantiates both SpMV variants
template <class F>
void with_c16(const DevSell& A, F&& f) {
  if (A.c16) f(std::true_type{});
  else f(std::false_type{});
}

struct Red {  // a (possibly globally reduced) partial array
  const double* p;
  int nb;
  int stride;
};

struct Timer {
  bool on = false;
  uint32_t mask = ~0u;  // timed kernel classes
  std::vector<hipEvent_t> pool;
  struct Pend { int cls; hipEvent_t a, b; double bytes; bool keep = false; };  // (cls < 0: not accounted)
  std::vector<Pend> pend;
  // classes: 0 k_cheb (finest), 1 k_cg_dir, 2 k_cg_upd, 3 k_grad_proj, 4 k_sl, 5 k_resid (finest), 6 / 7 the
  // finest level's restriction / prolongation, 8 k_sl_slow, 9 k_vcheb (whole-grid steps), 10 k_cheb_pair,
  // 11 k_div, 12 k_vcheb_pair, 13 k_visc_prep, 14 k_mdot2, 15 k_pcomb
  static constexpr int NCLS = 16;
  double ms[NCLS] = {};
  double bytes[NCLS] = {};
  int64_t n[NCLS] = {};
  hipEvent_t get() {
    if (pool.empty())  // in batches: the samples stay pending until their solve's test is read
      for (int k = 0; k < 256; ++k) {
        hipEvent_t e;
        HIPCHK(hipEventCreate(&e));
        pool.push_back(e);
      }
    hipEvent_t e = pool.back();
    pool.pop_back();
    return e;
  }
  size_t done = 0;  // samples accounted so far (the absolute index of pend[0])
  size_t mark() const { return done + pend.size(); }
  void account(const Pend& p) {
    if (p.cls >= 0) {
      float t = 0;
      HIPCHK(hipEventElapsedTime(&t, p.a, p.b));
      ms[p.cls] += t;
      bytes[p.cls] += p.bytes;
      n[p.cls]++;
    }
    pool.push_back(p.a);
    pool.push_back(p.b);
  }
  void flush() {
    for (auto& p : pend) {
      HIPCHK(hipEventSynchronize(p.b));
      account(p);
    }
    done += pend.size();
    pend.clear();
  }
  // account the finished samples before absolute index `limit` without waiting: called while the GPU runs the
  // work just enqueued, so the host's event reads overlap it (a blocking flush after a solve's convergence
  // read idled the GPU ~0.12 ms per pressure solve, r10x trace)
  void flush_ready(size_t limit) {
    size_t i = 0;
    for (; i < pend.size() && done + i < limit; ++i)
      if (hipEventQuery(pend[i].b) != hipSuccess) break;
    for (size_t k = 0; k < i; ++k) account(pend[k]);
    pend.erase(pend.begin(), pend.begin() + (std::ptrdiff_t)i);
    done += i;
  }
  // drop the pending samples from absolute index k on (launches that found the solve converged and returned
  // without work: counting them would credit their bytes to a near-zero duration)
  // (samples marked `keep` stay: a gated gradient projection behind the read that found the solve converged)
  void drop_from(size_t k) {
    size_t w = k > done ? k - done : 0;
    for (size_t i = w; i < pend.size(); ++i) {
      if (pend[i].keep) {
        pend[w++] = pend[i];
        continue;
      }
      pool.push_back(pend[i].a);
      pool.push_back(pend[i].b);
    }
    if (w < pend.size()) pend.resize(w);
  }
  ~Timer() {
    for (auto e : pool) (void)hipEventDestroy(e);
    for (auto& p : pend) {
      (void)hipEventDestroy(p.a);
      (void)hipEventDestroy(p.b);
    }
  }
};

template <typename T>
struct MgBufs {
  T *Aval = nullptr, *Prval = nullptr, *Rval = nullptr, *dinv = nullptr;
  T *x = nullptr, *x2 = nullptr, *b = nullptr, *d = nullptr, *res = nullptr, *sendbuf = nullptr;
  // fp16 copy of the level operator's values (fp32 cycle, when every value is representable): the
  // smoother and residual stream 2 B per entry instead of 4, arithmetic stays fp32
  _Float16* Aval16 = nullptr;
  template <class F>
  void with_vals(F&& f) const {
    if constexpr (std::is_same<T, float>::value) {
      if (Aval16) {
        f((const _Float16*)Aval16);
        return;
      }
    }
    f((const T*)Aval);
  }
  double val_bytes() const { return Aval16 ? 2.0 : (double)sizeof(T); }
};

// face-interior node -> its macro face (the deep halos' face-stencil ghost rows, face_ghost_rows)
struct FaceLookup {
  std::vector<std::pair<i64, i32>> starts;  // (first interior node, face), ascending
  LocalPlan full;                           // the level's whole range: to_local = the global id
  void init(const Macro& M, const LatticeLevel& LL) {
    starts.clear();
    for (i64 f = 0; f < M.nf; ++f)
      if (LL.face_start[f] >= 0) starts.push_back({LL.face_start[f], (i32)f});
    std::sort(starts.begin(), starts.end());
    full.r0 = 0;
    full.r1 = (i64)LL.type.size();
    full.n_own = full.r1;
  }
  // face-interior node g -> (face, offset t)
  void find(i64 g, i32& f, i32& t) const {
    auto it = std::upper_bound(starts.begin(), starts.end(), std::make_pair(g, (i32)INT32_MAX));
    --it;
    f = it->second;
    t = (i32)(g - it->first);
  }
};
GhostRowFn face_ghost_rows(const Macro& M, const LatticeLevel& LL, const FaceLookup& FL, const std::vector<i32>* dof,
                           int l, double dtnu) {
  return [&M, &LL, &FL, dof, l, dtnu](i32 g, std::vector<i32>& cols, std::vector<double>& vals) -> bool {
    if (LL.F == 0 || LL.type[g] != 0) return false;
    i32 f, t;
    FL.find(g, f, t);
    std::vector<lat::FaceTab> tab;
    lattice_tabs(M, LL, {f}, 0, FL.full, dof, tab);
    std::vector<double> rec;
    lattice_coefs(M, {f}, l, dtnu, rec);
    const i32 n = LL.n;
    i32 i, j, nb[6];
    bool in[6];
    lat::coords(t, n, 1.0f / (float)(n - 1), i, j);
    lat::neighbours(tab[0], n, t, i, j, nb, in);
    cols.assign({g, nb[0], nb[1], nb[2], nb[3], nb[4], nb[5]});
    const double kab = rec[lat::C_KAB], kac = rec[lat::C_KAC], kbc = rec[lat::C_KBC];
    vals.assign({rec[lat::C_KD], kab, kab, kac, kac, kbc, kbc});
    return true;
  };
}
double face_dinv(const Macro& M, const LatticeLevel& LL, const FaceLookup& FL, int l, i64 g) {
  i32 f, t;
  FL.find(g, f, t);
  std::vector<double> rec;
  lattice_coefs(M, {f}, l, 0.0, rec);
  return rec[lat::C_DINV];
}

// One level of the geometric multigrid hierarchy (pressure preconditioner).  Level 0 is the
// coarsest (the caller's base mesh, solved densely), the last level is the simulation mesh.
struct MgLevel {
  HostMesh mesh;            // coarse levels only (the finest is Ctx::mesh)
  std::vector<i32> ea, eb;  // edge endpoints of the level below (midpoint parents), caller numbering
  Ordering ord;
  Csr P, Pp, Pr, R;         // pattern, merged pressure operator, prolongation from l-1, restriction to l-1
  std::vector<i32> dof, master_of, slave_of;
  std::vector<std::pair<i64, i64>> pairs;
  std::vector<i64> rs;      // partition of this level's internal ids
  LocalPlan lp;
  double lmax = 2.0;
  double lam_dev = 0.0;  // the device power iteration's last Rayleigh quotient (0: not run; pucfem_mg_lmax)
  // device
  Sell sA, sPr, sR;         // host SELL images (built with the plans, also on host-only contexts)
  DevSell dA, dPr, dR;
  MgBufs<double> f64;       // the V-cycle's values and vectors: one of the two sets is allocated
  MgBufs<float> f32;        // (fp32 = the mixed-precision cycle, prm.mg_single)
  int32_t* dsend = nullptr;
  i64 nsend = 0, nloc = 0;
  // multi-rank runs: coarse levels of <= mg_rep_nodes nodes are REPLICATED (every rank holds and
  // smooths the whole level, no halos); the restriction into the finest replicated level computes
  // the rows of the strip partition (rs) and an all-gather (broadcast group) completes the vector
  bool rep = false;
  // deep halos (W > 1, lattice, PUCFEM_DEEP_HALO): the plan's ghosts reach two layers out (make_local_plan2's G2) and
  // the operator's SELL carries the ghost rows one layer out (g1, global ids) behind DevSell::with_ghosts().  Then
  // - a step pair runs its first step on those rows too (one exchange of x for two steps; pairs at W > 1),
  // - res_deep: the residual runs on them too, so the restriction reads no exchanged residual,
  // - the post-smoothing's last step runs on them (x and d exchanged before it, as x alone was), so its output is
  //   current at the ghosts the next consumer gathers: z for the PCG's A z (finest), x for the prolongation into
  //   the finer level (xc_deep, on that finer level: its prolongation's coarse columns lie in own + G1).
  // Every rank takes the same path (the flags are all-reduced at build).
  // - pr_deep: the prolongation into this level also runs on its ghost rows (x there is current since the exchange
  //   before the residual), its coarse columns in level l - 1's own + G1 rows: the post-smoothing's first pair needs
  //   no exchange of x.
  std::vector<i32> g1;
  bool deep = false, res_deep = false, xc_deep = false, pr_deep = false;
  FaceLookup flook;  // (deep lattice levels) face-interior node -> face
  i64 r_r0 = 0;  // first row of this level's restriction operator (rows live on level l-1)
  i64 own0(int rank) const { return rep ? 0 : rs[rank]; }
  // lattice face parts (Ctx::lattice): the faces whose interiors are this rank's rows of this level,
  // their tables (plain: K / G / A_visc; merged: the periodic-merged pressure operator) and records;
  // the prolongation into this level gathers the same faces on level l-1 (pr_tab2, merged), the
  // restriction into level l-1 writes the faces of its rows [r_r0, r_r0 + nr) (r_tab, bases from
  // r_r0) from this level's nodes (r_tab2, plain)
  LatticeLevel latl;
  std::vector<i32> lf_faces, r_faces;
  std::vector<lat::FaceTab> lf_plain, lf_merged, pr_tab2, r_tab, r_tab2;
  std::vector<double> lf_coef;
  HFace hA, hPr, hR;  // level operator (merged), prolongation into / restriction from this level
};
template <typename T> MgBufs<T>& bufs(MgLevel& L);
template <> MgBufs<double>& bufs<double>(MgLevel& L) { return L.f64; }
template <> MgBufs<float>& bufs<float>(MgLevel& L) { return L.f32; }

void spmv_on(hipStream_t st, const DevSell& A, const FaceDev& fc, const double* val, const double* x, double* y);
// k_mdot2 / k_pcomb for basis size m (0..PROJ_MAX): one instance per size, picked from a table (every
// instance has the same signature, so the launch goes through Ctx::klaunch like any other kernel)
using Mdot2K = decltype(&k_mdot2<0>);
using PcombK = decltype(&k_pcomb<0>);
template <int... M>
constexpr std::array<Mdot2K, sizeof...(M)> mdot2_table(std::integer_sequence<int, M...>) {
  return {&k_mdot2<M>...};
}
template <int... M>
constexpr std::array<PcombK, sizeof...(M)> pcomb_table(std::integer_sequence<int, M...>) {
  return {&k_pcomb<M>...};
}
Mdot2K mdot2_kernel(int m) {
  static constexpr auto tab = mdot2_table(std::make_integer_sequence<int, PROJ_MAX + 1>{});
  if (m < 0 || m > PROJ_MAX) throw Error(PUCFEM_EINVAL, "projection basis size out of range");
  return tab[m];
}
PcombK pcomb_kernel(int m) {
  static constexpr auto tab = pcomb_table(std::make_integer_sequence<int, PROJ_MAX>{});
  if (m < 0 || m >= PROJ_MAX) throw Error(PUCFEM_EINVAL, "projection basis size out of range");
  return tab[m];
}

struct Ctx {
  std::string err;
  int device = -1;
  bool host_only = true;
  int rank = 0, world = 1;
  // the data-path communicator: RCCL (or the LocalComm test backend) on multi-rank runs; also RCCL on a
  // ONE-rank context created from a real unique id (pucfem_ctx_create_dist with world 1), which then
  // takes every multi-rank code path -- all-reduces, broadcasts, the dye range exchange -- through RCCL
  std::unique_ptr<Comm> comm;
  bool dist() const { return comm != nullptr; }
  hipStream_t st = nullptr;
  std::vector<void*> allocs;
  Timer timer;
  // algorithmic bytes of the launched kernels (pucfem_counters: the step's HBM floor): each vector
  // counted once per row it is read or written, stored operators per entry; launches that find their
  // solve already converged (no work) are taken back once the host learns the iteration count
  double algo_bytes = 0.0;
  // per kernel class (Timer's classes), every launch timed or not: launches and algorithmic bytes
  // (pucfem_class_counters: bench.py weighs the classes over the whole timed window with them)
  double cls_bytes[Timer::NCLS] = {};
  int64_t cls_n[Timer::NCLS] = {};
  struct ByteMark {  // the counters at one point (launches after a solve's convergence are taken back)
    double total;
    double cb[Timer::NCLS];
    int64_t cn[Timer::NCLS];
  };
  ByteMark bmark_now() const {
    ByteMark m{algo_bytes, {}, {}};
    for (int k = 0; k < Timer::NCLS; ++k) {
      m.cb[k] = cls_bytes[k];
      m.cn[k] = cls_n[k];
    }
    return m;
  }
  void bmark_restore(const ByteMark& m) {
    algo_bytes = m.total;
    for (int k = 0; k < Timer::NCLS; ++k) {
      cls_bytes[k] = m.cb[k];
      cls_n[k] = m.cn[k];
    }
  }

  // ---- inputs
  HostMesh mesh;
  bool has_mesh = false;
  std::vector<std::pair<i64, i64>> op_pairs, bc_pairs;
  std::vector<i32> dir_nodes;
  std::vector<double> dir_vals;
  int dir_ncomp = 0;
  std::vector<float> g_tri;
  pucfem_params prm{};
  bool built = false;
  std::unique_ptr<Ens> ens;  // pucfem_ens_create (one per context)

  // ---- host structures (internal numbering)
  Ordering ord;
  Csr P, Pp, Lit;
  Assembly as;
  std::vector<double> litb, Kv;
  std::vector<i64> row_start;
  LocalPlan lp;
  Sell sP, sPp, sLit;
  std::vector<i32> dof, slave_of, master_of;  // global internal ids
  i64 n_free = 0;
  int scheme = 0;

  // ---- device operators
  DevSell dP, dPp, dLit;
  double *dK = nullptr, *dGx = nullptr, *dGy = nullptr, *dKv = nullptr, *dKp = nullptr, *dLitv = nullptr;
  double *dsv = nullptr, *dsp = nullptr, *dlit_dinv = nullptr;
  double *das1 = nullptr, *dmp = nullptr, *dwmix = nullptr;
  uint8_t* ddir = nullptr;
  int32_t *dslave_of = nullptr, *dmaster_of = nullptr;
  int32_t *dcdst = nullptr, *dcsrc = nullptr, *ddnode = nullptr;
  double *ddval = nullptr, *dbctmp = nullptr;
  int32_t *dbcsrc = nullptr, *dbcdir = nullptr;  // dense path: k_dense_mv2_bc's row maps
  int ncopy = 0, ndir = 0;
  bool bc_gather = true;  // some copy source is also written: k_bc_gather saves the sources first
  int32_t* dsend = nullptr;
  double* dsendbuf = nullptr;
  i64 nsend = 0;

  // ---- device fields (local: n_own + n_ghost)
  i64 nloc = 0;
  double *ux = nullptr, *uy = nullptr, *usx = nullptr, *usy = nullptr, *p = nullptr, *p2 = nullptr;
  double *yp = nullptr, *yp2 = nullptr, *yvx = nullptr, *yvy = nullptr;
  double *div_star = nullptr, *div_u = nullptr, *final_div = nullptr, *braw = nullptr, *bh = nullptr;
  double *bvx = nullptr, *bvy = nullptr;
  double *cg_r[2] = {nullptr, nullptr}, *cg_pa[2] = {nullptr, nullptr}, *cg_pb[2] = {nullptr, nullptr},
         *cg_q[2] = {nullptr, nullptr};
  double *part_a = nullptr, *part_b = nullptr, *part_c = nullptr, *part_d = nullptr;
  double* scal = nullptr;
  int* ctl = nullptr;
  int* h_ctl = nullptr;  // pinned
  double* redbuf = nullptr;  // small buffers for all-reduced scalars (64 x 8)
  double* vals = nullptr;    // per-step diagnostic slots (16)
  double* scalar = nullptr;  // heat u / poisson f
  double* litw[10] = {};     // BiCGStab workspace
  double* bicg_sc = nullptr;
  double* h_pinned = nullptr;

  // ---- full-mesh replica (SL, tracers)
  double *mx = nullptr, *my = nullptr;
  int32_t* mtri = nullptr;
  GridDev cgrid{}, tgrid{};
  LocDev lgrid{};
  // implicit FEM dye variant (prm.dye_scheme == 1, good_visualization.py:700-718)
  bool dye_impl = false;
  DevSell dDye{};              // the merged (Pp) pattern, every row stored
  DyeDev dye{};
  double *dDyeVal = nullptr, *dDyeM = nullptr, *dDyeW = nullptr, *dDyeDinv = nullptr, *dDyeB = nullptr;
  int64_t* dDyeDiag = nullptr;  // SELL slot of each row's diagonal
  int32_t *dDyeSrow = nullptr, *dDyeSk = nullptr, *dDyeSc = nullptr;
  int64_t* dDyeSptr = nullptr;
  int32_t dye_nsrow = 0;
  int last_dye_it = 0;
  bool lmax_dev = false;            // the finest level's lmax: power iteration on the device
  // multi-rank dye replica: a wide halo instead of an all-gather (dye_halo)
  std::vector<double> strip_ylo, strip_yhi;  // per strip (internal order): the y extent of its nodes
  std::vector<i64> rank_s0, rank_s1;         // per rank: its strips [s0, s1)
  std::vector<double> rank_ylo, rank_yhi;    // per rank: the y extent of its nodes
  double tri_hy = 0.0;                       // largest y extent of a triangle
  double* part_u = nullptr;                  // back-traced y range partials (1 - min, max)
  double *yr_own = nullptr, *yr_all = nullptr;  // this rank's (1 - min, max); every rank's (2 W)
  std::vector<double> h_yr;
  double* trv = nullptr;                     // multi-rank tracer velocities (3 x ntr, all-reduced)
  int32_t* dghost_global = nullptr;          // lp.ghost_global on the device
  i64 dye_halo_values = 0;                   // values received by the last dye_halo (diagnostics)
  std::vector<double> lmax_dinv;    // its D^-1 (host, Gershgorin pass)
  DyeOp dyeop;  // host data of the implicit dye operator (built with the host operators)
  LatLocDev llgrid{};  // lattice locator (lat_sl): replaces lgrid's records on lattice hierarchies
  bool lat_sl = false;
  // f(the context's locator), llgrid or lgrid: one launch site instantiates a kernel for both (as with_c16)
  template <class F>
  void with_loc(F&& f) const {
    if (lat_sl) f(llgrid);
    else f(lgrid);
  }
  bool has_locator() const { return lat_sl ? llgrid.face != nullptr : lgrid.rec != nullptr; }
  double* part_sl = nullptr;  // k_sl partials, 3 x SLB
  int32_t* sl_queue = nullptr; // k_sl -> k_sl_slow: rows off the lattice fast path (mesh.N)
  int32_t* sl_qcnt = nullptr; // per wave of k_sl: queued entries (SLB * BS / 64)
  int32_t* sl_qoff = nullptr; // k_sl_qscan: the queues' first entry numbers (SLB * BS / 64 + 1)
  bool has_cgrid = false, has_tgrid = false;
  // pucfem_sample_points / pucfem_raster / pucfem_ens_raster (pucfem_sample.hpp): device buffers allocated at a
  // call's first need and kept (grown when a later call needs more).  Slot 0 the points, 1 the output, 2 the
  // triangle ids, 3 the probe's counters, 4.. the fields that are formed when read (p / p2 kept in y, div u*,
  // the final divergence, 8 the vorticity): the samplers form them here and write no field of the context.
  // Slot 9: the partials of the vorticity pass (4 x MAXB) and, behind them, pucfem_flow_info's four reduced values
  // Slots 10..13: pucfem_streamlines / pucfem_ens_streamlines (pucfem_streamline.hpp): the seeds, the points, the
  // status and npts (one buffer), the values along the lines
  // Slots 14..16: pucfem_sl_advect_multi / pucfem_dyes_probe (pucfem_dye_channels.hpp) and pucfem_sl_advect_vel /
  // pucfem_inertia_probe (pucfem_inertia.hpp): the fields in, the fields out, the blocks' not-found counts
  // Slots 17..21: pucfem_sl_advect_mc / pucfem_sl_advect_vel_mc / pucfem_advection_probe (pucfem_maccormack.hpp): the
  // intermediate fields, the records, the marks, the triangle ids, pass 2's counts
  // Slot 22: pucfem_stroke_apply / pucfem_stroke_probe (pucfem_stroke.hpp): a copy of the Dirichlet values and, behind
  // it, the probe's counter
  // Slot 23: pucfem_sl_advect_traj / pucfem_sl_advect_vel_traj / pucfem_trajectory_probe (pucfem_trajectory.hpp): the
  // blocks' midpoint counts of the two passes (they share slots 14..21 with the operations above)
  // Slot 24: pucfem_loads_apply (pucfem_loads.hpp): the caller's p and, behind it, a plane of zeros for p2
  static constexpr int SMP_SLOTS = 25;
  void* smp_buf[SMP_SLOTS] = {};
  size_t smp_cap[SMP_SLOTS] = {};
  template <class T>
  T* smp_scratch(int slot, size_t count) {
    const size_t bytes = sizeof(T) * std::max<size_t>(1, count);
    if (smp_cap[slot] < bytes) {
      if (smp_buf[slot]) {
        HIPCHK(hipStreamSynchronize(st));
        (void)hipFree(smp_buf[slot]);
        smp_buf[slot] = nullptr;
        smp_cap[slot] = 0;
      }
      HIPCHK(hipMalloc(&smp_buf[slot], bytes));
      smp_cap[slot] = bytes;
    }
    return static_cast<T*>(smp_buf[slot]);
  }
  double *c_full = nullptr, *c_new = nullptr, *ufx = nullptr, *ufy = nullptr;
  int32_t* dnotfound = nullptr;
  int32_t ntr = 0;
  double *trx = nullptr, *try_ = nullptr, *trs = nullptr, *d_eaten = nullptr;
  int32_t* trcap = nullptr;   // capture steps (-1: not captured), written by tracer_move
  int32_t* trstep = nullptr;  // tracer steps since the set was set: read and advanced on the device (a captured step's
                              // arguments are fixed)
  double* part_tr = nullptr;  // the cloud kernels' per-block eaten partials (TRACER_CLOUD_MAXB)
  unsigned long long* trcensus = nullptr;  // pucfem_tracer_info's two counts
  int tr_blocks = 0, tr_threads = 0;       // the last tracer launch
  // Brownian tracers (pucfem_set_tracer_diffusion, pucfem_brownian.hpp): the context's own setting, host values only
  // (the kernels take them as arguments: a changed setting drops the captured step graphs).  tr_ylo / tr_yhi: the
  // reflecting walls, the mesh's smallest and largest node y, from the build.
  double tr_D = 0.0;
  uint64_t tr_seed = 0;
  double tr_ylo = 0.0, tr_yhi = 0.0;
  // the single-rank Stokes context the tracers' diffusion lives on (decided before the device is asked for)
  void brownian_ready() const {
    need_built();
    if (!(scheme == PUCFEM_STOKES_COLOR || scheme == PUCFEM_STOKES_FOOD))
      throw Error(PUCFEM_ESTATE, "tracer diffusion needs a Stokes context");
    if (dist() || world != 1) throw Error(PUCFEM_ESTATE, "tracer diffusion is single-rank");
  }
  // iteration count of the last solve per `which` slot (the next solve's first host check): 0 viscous,
  // 1 / 2 the two pressure solves of a step, 3 / 4 standalone viscous / pressure solves (pucfem_solve)
  int last_it[6] = {0, 0, 0, 0, 0, 0};
  bool solved_before[6] = {false, false, false, false, false, false};  // last_it[which] holds a real count
  // per slot: whether each of the last 8 solves that followed a solve of <= 1 iteration passed at its
  // initial guess (bit 0 the latest) -- pcg_mg's pre-check policy
  unsigned zero_hist[6] = {0u, 0u, 0u, 0u, 0u, 0u};
  bool lds_attr[3] = {false, false, false};  // k_cg_block<NR>: dynamic-LDS attribute set on this device
  double* solve_tmp = nullptr;  // pucfem_solve scratch (4 x nloc): standalone solves never touch the step state
  int* dits = nullptr;  // per-step iteration counts written by single-workgroup solves (no host sync)
  int cur_step = 0;
  bool block_cg = true;  // small operators: whole CG in one workgroup
  // small meshes (N <= DENSE_MAX, one rank): both linear solves are dense direct solves with
  // precomputed inverses -- the reference's np.linalg.solve, factorised once instead of per call
  bool dense = false;
  double *dVinv = nullptr, *dPinv = nullptr;
  // small literal operators (heat / Poisson, N <= DENSE_MAX): the inverse of the literal operator
  // (heatEq.py:321 / poisson.py:283 solve with it every step: np.linalg.solve, factorised once here)
  double* dLitInv = nullptr;
  // small meshes: one StokesColor/StokesFood step captured once into a hipGraph and replayed
  bool graph_mode = false;
  hipGraphExec_t gexec = nullptr;
  hipGraph_t graph = nullptr;
  // and GK = 8 consecutive steps in one graph (PUCFEM_GRAPH_STEPS, measurement knob; 1 = one step per replay): one
  // launch per 8 steps, whose ~8 us between replays (r14u trace) the steps inside a graph do not pay; the same bits
  // (test_graph_of_k_steps_equals_single_step_graph).  mesh_fine 12.3-12.6k -> 13.1-13.5k steps/s (r14x; with the
  // step's earlier 13 launches, 8-step graphs measured slower, r14b)
  int gk = std::getenv("PUCFEM_GRAPH_STEPS") ? std::max(1, std::min(64, std::atoi(std::getenv("PUCFEM_GRAPH_STEPS")))) : 8;
  hipGraphExec_t gexec_k = nullptr;
  hipGraph_t graph_k = nullptr;
  double* gstats = nullptr;
  // the replayed step's records: a device ring of GRING steps (k_stats_ring), copied out per call / full ring
  static constexpr int GRING = 1024;
  double* gring = nullptr;
  int* gcount = nullptr;
  bool gcapture = false;  // (the step being captured)
  // the captured step's record appended by k_mix2's reducing block (otherwise k_stats_ring)
  bool ring_in_mix = false;

  // ---- lattice operators (pucfem_lattice.hpp): multigrid hierarchies with faces of interior nodes
  bool lattice = false;
  // deep halos on W > 1 ranks (MgLevel::deep; PUCFEM_DEEP_HALO=0 keeps one-layer halos and single smoothing steps,
  // a test / measurement knob)
  bool deep_halo = !(std::getenv("PUCFEM_DEEP_HALO") && std::atoi(std::getenv("PUCFEM_DEEP_HALO")) == 0);
  bool z_cur = false;  // the finest level's last smoothing step wrote z at the ghost rows one layer out too
  // PUCFEM_DEEP_MASK (diagnostic knob, default all): 1 multigrid step pairs, 2 residual rows, 4 last smoothing step
  // (+ the skipped z / x exchanges), 8 prolongation rows, 16 the viscous first pair -- each use of the ghost rows
  int deep_mask = std::getenv("PUCFEM_DEEP_MASK") ? std::atoi(std::getenv("PUCFEM_DEEP_MASK")) : 31;
  Macro macro;
  LatticeLevel lat_fine;  // the finest level's layout until build_mg_host moves it into mg.back()
  HFace fK, fVisc, fP;  // finest level: K / Gx / Gy (plain table), scaled A_visc (plain), pressure (merged)
  // Gershgorin radius of the Jacobi-scaled A_visc, max_i sum_{j != i} |a_ij| / sqrt(a_ii a_jj): its spectrum
  // lies in [1 - visc_R, 1 + visc_R] (the Chebyshev viscous solve's interval)
  double visc_R = 1.0, visc_lo = 0.0;
  int visc_solver = 0;  // 0 = Chebyshev iteration when visc_R < 0.25 (multi-kernel path), 1 = CG
  // a-posteriori check of the Chebyshev bound (vcheb): the last step of a solve also reduces |r_{k}|^2 of
  // the iterate it starts from (k = K - 1), copied to h_pinned[32 ..]; the next solve compares it with
  // |r_0| / T_k(sigma) -- a spectrum outside [visc_lo, 1 + visc_R] (a wrong interval) breaks the bound.  A
  // violation switches the viscous solves to the CG (visc_check_fail counts them, pucfem_path_info)
  struct ViscCheck {
    bool pending = false;
    int nr = 0;
    double bound2[2] = {0.0, 0.0}, floor2[2] = {0.0, 0.0};
  } vcc;
  int visc_check_fail = 0;
  // step pairs of the viscous Chebyshev solve (k_vcheb_pair, single rank with a face part): PUCFEM_VISC_PAIR=0
  // runs every step as its own k_vcheb (a measurement knob); the pair's third x buffer and second d
  // buffer are allocated on first use
  bool visc_pair = !(std::getenv("PUCFEM_VISC_PAIR") && std::atoi(std::getenv("PUCFEM_VISC_PAIR")) == 0);
  int64_t visc_pairs = 0;  // pairs launched (pucfem_path_info)
  // step pairs of the finest level's smoothing in the fp32 V-cycle (k_cheb_pair, single rank):
  // PUCFEM_MG_PAIR=0 runs every step as its own k_cheb (a measurement knob); a third x buffer and a second
  // d buffer of the finest level are allocated on first use
  bool mg_pair = !(std::getenv("PUCFEM_MG_PAIR") && std::atoi(std::getenv("PUCFEM_MG_PAIR")) == 0);
  int64_t mg_pairs = 0;
  float* mgp_x = nullptr;
  float* mgp_d = nullptr;
  double* dwsk = nullptr;  // scaled A_visc skeleton column weights
  static FaceDev nof() { return FaceDev{}; }

  // ---- multigrid
  HostMesh coarse;
  int mg_levels = 0;  // refinements from `coarse` to `mesh` (0: no hierarchy given)
  bool use_mg = false;
  std::vector<MgLevel> mg;
  double* dKp_raw = nullptr;        // unscaled finest pressure operator on sPp
  // dense pseudo-inverse of the coarsest level's operator (replicated).  The dense solve one level up instead gained
  // nothing within the spread and halved the L7 parity margin (r12f / r12g).
  double* dAinv = nullptr;
  bool mg_single = false;                        // fp32 V-cycle
  double* z = nullptr;              // preconditioned residual (finest; the fp64 V-cycle's)
  // the fp32 V-cycle's z: its last smoothing step computes in fp32, so z is fp32-exact -- stored as such,
  // the direction kernel gathers 4 B per point instead of 8 and p = z + beta p_old is the same
  float* z32 = nullptr;
  // successive right-hand sides: per pressure solve (which = 1: p, 2: p2) an A-orthonormal basis of
  // up to proj_k solution directions, the projected guess x0 and the new direction
  // (which = 3, 4: the viscous solve's x and y components, proj_k_visc directions each)
  int proj_k = 0, proj_k_visc = 0;
  ProjT* projX[5] = {};
  // the basis of slot w: its ld argument (the capacity) and the offset of its vector i
  i64 pld(int w) const { return w <= 2 ? proj_k : proj_k_visc; }
  i64 pcol(int, int i) const { return 64 * (i64)i; }
  double* proj_x0[5] = {};
  int proj_m[5] = {0, 0, 0, 0, 0};
  // Deferred update (project_guess): after a solve only v = y - x0 and A v are formed; the next
  // guess of the same solve orthogonalises v against X, appends it and projects the new right-hand
  // side in one multi-dot and one combination pass over X.  h_coef (pinned) receives each guess's
  // coefficients, read at the next guess to track the coordinates of the recent solutions in the
  // basis (re-seeding a full basis, proj_reseed, which keeps proj_keep seeds).
  static constexpr int NCOEF = 2 * PROJ_MAX + 4;
  double* h_coef = nullptr;
  ProjT* projXalt[5] = {};
  struct ProjHist {
    std::vector<std::vector<double>> sols;  // coordinates of the last solutions
    std::vector<double> gamma;              // coordinates of the last guess x0
    int coef_m = -1;                        // h_coef holds a guess over coef_m directions (-1: none)
  } proj_hist[5];
  static constexpr int proj_keep = PROJ_KEEP_MAX;
  double *proj_part = nullptr, *proj_d = nullptr, *proj_coef = nullptr;
  double* dqm = nullptr;  // re-seed coefficients (QMat) on the device
  bool proj_pend[5] = {false, false, false, false, false};  // v / A v wait for the next guess
  double *pv[5] = {}, *pav[5] = {};
  // Pressure directions left pending (one rank, lattice, multigrid, shared-basis-free or shared): after a solve
  // the projection update's v = y - x0 and A v = r0 - r_final are not stored; the next solve's k_mdot2 /
  // k_pcomb form them from y, x0, pav (r0) and cg_r[0] (r_final) -- the same values, 60 B/row of k_diff2_fin
  // saved for 24 B/row more in those passes -- and the gradient projection gathers the solution y through
  // the merged (slave -> master) face tables and SELL columns instead of a separate p = y with the slaves
  // copied (p_s = p_m exactly, so the same values).  proj_materialize() stores a pending direction
  // (k_diff2) before anything could overwrite its inputs.
  bool p_from_y = false;
  DevSell dPm;  // dP with merged columns (the gradient's gathers of y)
  bool pend_otf[5] = {};
  const double* pend_y[5] = {};
  // the solve after a projected guess accumulates its correction v = sum alpha_k p_k in pv[slot] (k_cg_upd's
  // vacc; k_pcomb clears it with the guess): pend_acc -- the pending / stored v is that accumulator, not y - x0
  bool pend_acc[5] = {};
  // the accumulated v of slot is zero (its solve passed at the guess: no update ran, so the accumulator, which the
  // first update starts instead of a cleared buffer, was not written); k_mdot2 / k_pcomb then read no v
  bool pend_vzero[5] = {};
  double* cg_vacc = nullptr;  // pcg_mg's accumulator of the current solve (null: none)
  // keep: a slot whose pending direction stays (its r_final is the one cg_r[0] still holds)
  void proj_materialize(int keep = 0) {
    for (int w = 1; w <= 2; ++w) {
      if (!pend_otf[w] || w == keep) continue;
      const i64 n = lp.n_own;
      algo_bytes += 48.0 * (double)n;
      hipLaunchKernelGGL(k_diff2, dim3(grid_ew(n)), dim3(BS), 0, st, n, pend_y[w], (const double*)proj_x0[w],
                         pend_acc[w] ? (double*)nullptr : pv[w],
                         (const double*)pav[w], (const double*)cg_r[0], pav[w]);
      KCHK();
      pend_otf[w] = false;
    }
  }
  // viscous warm start u^n + a polynomial extrapolation of the increments u* - u of the last steps:
  // dvinc[0..1] the last (x, y), [2..3] the one before, [4..5] the one before that, ...;
  // PUCFEM_VISC_EXTRAP (measurement knob): the order, 0 (off) .. VINC_MAX, default 5 (round 2, L7 driver
  // command with the Chebyshev solve: 77 / 71 / 67 viscous steps per 20 steps for orders 3 / 4 / 5,
  // 106.1 / 107.0 / 107.2 steps/s, r5e; orders 6 / 7: 64 steps, within the spread, r6e; L7, 40 steps,
  // round 1: viscous iterations per step 5 / 4 / 3 / 2-3 for orders 0-3, 17.47 / 16.82 / 16.12 /
  // 15.75 ms per step)
  float* dvinc[2 * VINC_MAX] = {};
  int have_vinc = 0;
  int visc_extrap = std::getenv("PUCFEM_VISC_EXTRAP") ? std::max(0, std::min(VINC_MAX, std::atoi(std::getenv("PUCFEM_VISC_EXTRAP")))) : 5;
  // the operator a basis is A-orthonormal for: the pressure solves' unscaled merged operator (null
  // space: constants on the free dofs, cleared from new directions) or the Jacobi-scaled A_visc
  struct ProjOp {
    const DevSell* A;
    const double* val;
    const int32_t* null_free;  // master_of (free rows: < 0) when the operator has the constants' null space
    int kmax;
    FaceDev fc;
  };
  ProjOp proj_op(int which) const {
    return which <= 2 ? ProjOp{&dPp, dKp_raw, dmaster_of, proj_k, fP.full()}
                      : ProjOp{&dP, dKv, nullptr, proj_k_visc, fVisc.full()};
  }
  float* r32 = nullptr;             // fp32 copy of the CG residual: the fp32 V-cycle's right-hand side

  ~Ctx() {
    if (!host_only) {
      if (st) (void)hipStreamSynchronize(st);
      ens.reset();
      if (gexec) (void)hipGraphExecDestroy(gexec);
      if (graph) (void)hipGraphDestroy(graph);
      if (gexec_k) (void)hipGraphExecDestroy(gexec_k);
      if (graph_k) (void)hipGraphDestroy(graph_k);
      for (void* a : allocs) (void)hipFree(a);
      drop_dyes();
      drop_inertia();
      drop_force();
      drop_stroke(false);
      drop_advection();
      drop_trajectory();
      drop_stretch();
      drop_loads();
      for (void* a : smp_buf)
        if (a) (void)hipFree(a);
      if (h_ctl) (void)hipHostFree(h_ctl);
      if (h_coef) (void)hipHostFree(h_coef);
      if (h_pinned) (void)hipHostFree(h_pinned);
      if (h_yr_pin) (void)hipHostFree(h_yr_pin);
      if (ev_yr) (void)hipEventDestroy(ev_yr);
      for (int k = 0; k < 2; ++k) {
        if (stage[k]) (void)hipHostFree(stage[k]);
        if (stage_ev[k]) (void)hipEventDestroy(stage_ev[k]);
      }
      comm.reset();
      if (st_sl) (void)hipStreamSynchronize(st_sl);
      if (ev_u) (void)hipEventDestroy(ev_u);
      if (ev_sl) (void)hipEventDestroy(ev_sl);
      if (ev_gate) (void)hipEventDestroy(ev_gate);
      if (ev_wait) (void)hipEventDestroy(ev_wait);
      if (st_sl) (void)hipStreamDestroy(st_sl);
      if (st) (void)hipStreamDestroy(st);
    }
  }

  template <class T>
  T* dalloc(i64 n) {
    if (n <= 0) n = 1;
    void* p = nullptr;
    HIPCHK(hipMalloc(&p, sizeof(T) * (size_t)n));
    HIPCHK(hipMemsetAsync(p, 0, sizeof(T) * (size_t)n, st));
    allocs.push_back(p);
    return (T*)p;
  }
  template <class T>
  T* upload(const std::vector<T>& v) {
    T* p = dalloc<T>((i64)v.size());
    if (!v.empty()) h2d(p, v.data(), sizeof(T) * v.size());
    return p;
  }
  // Setup copies of large pageable arrays through two pinned staging buffers (double-buffered; the host
  // side of every chunk copied by the host threads): a pageable hipMemcpy moved 3 GB of device-assembly
  // results in 0.66 s at L7.  h2d is ordered on st like hipMemcpyAsync; d2h returns with the data in dst.
  static constexpr size_t STAGE_BYTES = size_t(64) << 20;
  char* stage[2] = {nullptr, nullptr};
  hipEvent_t stage_ev[2] = {nullptr, nullptr};
  bool stage_busy[2] = {false, false};
  void stage_wait(int k) {
    if (!stage[k]) {
      HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&stage[k]), STAGE_BYTES));
      HIPCHK(hipEventCreateWithFlags(&stage_ev[k], hipEventDisableTiming));
    }
    if (stage_busy[k]) HIPCHK(hipEventSynchronize(stage_ev[k]));
    stage_busy[k] = false;
  }
  static void host_copy(char* dst, const char* src, size_t len) {
    parallel_for((i64)len, [&](i64 a, i64 b) { std::memcpy(dst + a, src + a, (size_t)(b - a)); });
  }
  void h2d(void* dst, const void* src, size_t bytes) {
    if (bytes < (size_t(8) << 20)) {
      HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st));
      return;
    }
    for (size_t off = 0, i = 0; off < bytes; off += STAGE_BYTES, ++i) {
      const size_t len = std::min(STAGE_BYTES, bytes - off);
      const int k = (int)(i & 1);
      stage_wait(k);
      host_copy(stage[k], static_cast<const char*>(src) + off, len);
      HIPCHK(hipMemcpyAsync(static_cast<char*>(dst) + off, stage[k], len, hipMemcpyHostToDevice, st));
      HIPCHK(hipEventRecord(stage_ev[k], st));
      stage_busy[k] = true;
    }
  }
  void d2h(void* dst, const void* src, size_t bytes) {
    if (bytes < (size_t(8) << 20)) {
      HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      return;
    }
    size_t prev_off = 0, prev_len = 0;
    int prev_k = -1;
    for (size_t off = 0, i = 0; off < bytes; off += STAGE_BYTES, ++i) {
      const size_t len = std::min(STAGE_BYTES, bytes - off);
      const int k = (int)(i & 1);
      stage_wait(k);
      HIPCHK(hipMemcpyAsync(stage[k], static_cast<const char*>(src) + off, len, hipMemcpyDeviceToHost, st));
      HIPCHK(hipEventRecord(stage_ev[k], st));
      stage_busy[k] = true;
      if (prev_k >= 0) {  // the previous chunk, while this one is in flight
        stage_wait(prev_k);
        host_copy(static_cast<char*>(dst) + prev_off, stage[prev_k], prev_len);
      }
      prev_off = off;
      prev_len = len;
      prev_k = k;
    }
    if (prev_k >= 0) {
      stage_wait(prev_k);
      host_copy(static_cast<char*>(dst) + prev_off, stage[prev_k], prev_len);
    }
  }
  // A caller-numbered host array <-> device buffers in internal numbering (to_internal / to_caller,
  // pucfem_host.hpp): rows r0 .. r0 + n - 1 of `o`, comp values per row, `planes` whole fields on the caller's
  // side; on the device the window alone, planes dense, comp interleaved in d0 or (pairs) split into d0 and d1.
  // put is ordered on st and does not synchronise: h2d has consumed the staging vector when it returns (its
  // small branch is a pageable hipMemcpyAsync, which the runtime completes before it returns; its large branch
  // copies into the pinned chunks itself), so the vector may die here.  get returns with the data in dst (d2h
  // waits for st).  pinned = false: the pageable copy at every size, for a run's u, u* and c, as before this layer: at 14 MB
  // u measured slower through the pinned chunks (profiles/field_io_time.txt; larger sizes not measured).
  template <class T, class S>
  void put(const Ordering& o, i64 r0, i64 n, int comp, i64 planes, const S* src, T* d0, T* d1 = nullptr,
           bool pinned = true) {
    const i64 per = (d1 ? 1 : comp) * n, half = d1 ? planes * per : 0;
    if (planes * per == 0) return;
    std::vector<T> h((size_t)(planes * per + half));
    to_internal(o, r0, n, comp, planes, comp * (i64)o.new2old.size(), src, per, h.data(), d1 ? h.data() + half : nullptr);
    auto copy = [&](T* d, const T* s) {
      if (pinned) h2d(d, s, sizeof(T) * (size_t)(planes * per));
      else HIPCHK(hipMemcpyAsync(d, s, sizeof(T) * (size_t)(planes * per), hipMemcpyHostToDevice, st));
    };
    copy(d0, h.data());
    if (d1) copy(d1, h.data() + half);
  }
  template <class T, class D>
  void get(const Ordering& o, i64 r0, i64 n, int comp, i64 planes, D* dst, const T* d0, const T* d1 = nullptr,
           bool pinned = true) {
    const i64 per = (d1 ? 1 : comp) * n, half = d1 ? planes * per : 0;
    if (planes * per == 0) return;
    std::vector<T> h((size_t)(planes * per + half));
    auto copy = [&](T* d, const T* s) {
      if (pinned) return d2h(d, s, sizeof(T) * (size_t)(planes * per));
      HIPCHK(hipMemcpyAsync(d, s, sizeof(T) * (size_t)(planes * per), hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
    };
    copy(h.data(), d0);
    if (d1) copy(h.data() + half, d1);
    to_caller(o, r0, n, comp, planes, comp * (i64)o.new2old.size(), dst, per, h.data(), d1 ? h.data() + half : nullptr);
  }
  // the whole single-rank field / this rank's owned rows, in the context's own ordering
  template <class T, class S>
  void put_all(int comp, i64 planes, const S* src, T* d0, T* d1 = nullptr) { put(ord, 0, mesh.N, comp, planes, src, d0, d1); }
  template <class T, class D>
  void get_all(int comp, i64 planes, D* dst, const T* d0, const T* d1 = nullptr) { get(ord, 0, mesh.N, comp, planes, dst, d0, d1); }
  // int16 column deltas for a square operator's SELL (prm.idx32 = 0 and the band fits); nloc: the
  // local vector length (owned + ghost), the wrap modulus
  void attach_c16(const Sell& S, i64 nloc, DevSell& D) {
    if (!S.rows.empty()) return;  // row lists (lattice skeleton rows): int32 columns
    std::vector<int16_t> c16;
    if (!prm.idx32 && sell_col16(S, nloc, c16)) {
      D.c16 = upload(c16);
      D.wrap = (int32_t)nloc;
    }
  }
  // operator assembly on the device (prm.assembly 0 on a context bound to a device)
  bool dev_asm() const { return !host_only && prm.assembly == 0; }
  void need_dev() const {
    if (host_only) throw Error(PUCFEM_ENODEV, "compute call on a host-only context");
  }
  void need_built() const {
    if (!built) throw Error(PUCFEM_ESTATE, "pucfem_build_operators has not been called");
  }

  static int nb_for(i64 nslices) { return (int)std::max<i64>(1, std::min<i64>(EWB, (nslices + 3) / 4)); }
  // grid of the V-cycle kernels that produce no partials (more waves in flight than MAXB blocks)
  static int nb_mg(i64 nslices) { return (int)std::max<i64>(1, std::min<i64>(16384, (nslices + 3) / 4)); }
  int nb_rows(i64 n) const { return nb_for((n + 63) / 64); }
  // semi-Lagrangian grid: latency-bound gathers want more waves in flight than MAXB blocks give
  // PUCFEM_SL_WAVE (measurement knob): the lattice locator's second pass -- 2 (default) the numbered list
  // (k_sl_qscan + k_sl_wq + k_sl_qsum), 1 k_sl_wave (each wave its own queue), 0 k_sl_slow (one lane per point)
  int sl_wave_mode = std::getenv("PUCFEM_SL_WAVE") ? std::atoi(std::getenv("PUCFEM_SL_WAVE")) : 2;
  bool sl_wave = sl_wave_mode != 0;
  int nb_sl(i64 n) const {
    if (sl_rec_wave(n)) return (int)((n + BS / 64 - 1) / (BS / 64));  // k_sl_rec_wave: a wave per row
    return (int)std::max<i64>(1, std::min<i64>(SLB, (n + 4 * 64 - 1) / (4 * 64)));
  }
  // the record locator on a small mesh (mesh.1, mesh_fine): one wave per row in one launch instead of k_sl queueing
  // every row for k_sl_slow's one lane per point (PUCFEM_SL_WAVE=0 keeps the two passes)
  bool sl_rec_wave(i64 n) const { return !lat_sl && sl_wave && n <= SLB * (BS / 64); }
  static int grid_ew(i64 n) { return (int)std::max<i64>(1, std::min<i64>(2048, (n + BS - 1) / BS)); }
  // k_mdot2's 2,048 blocks do not all fit the chip (at the 96 VGPRs of r14 1,280 were resident, the rest a second
  // round).  Virtual blocks on a resident grid gave the same bits and no speed (461 vs 465 us, r14g); capping the grid itself was faster (442 -> 397 us) but
  // regroups the partials, and the L7 per-step margins went 5.7x / 7.5x -> 2.8x / 2.6x (r14d / r14e): the plain grid
  // stays.

  // ------------------------------------------------------------------ timing helpers
  // Launch on the library stream.  When timing (cls >= 0), the start / stop events are taken by the
  // kernel's dispatch itself (hipExtLaunchKernelGGL): the sample is the kernel's own duration, as
  // rocprofv3 reports it, without the command-processor gap a separately recorded event adds.
  template <typename... KArgs, typename... Args>
  void klaunch(int cls, double bytes, void (*kernel)(KArgs...), dim3 g, dim3 b, Args... args) {
    algo_bytes += bytes;
    if (cls >= 0) {
      cls_bytes[cls] += bytes;
      ++cls_n[cls];
    }
    if (timer.on && cls >= 0 && ((timer.mask >> cls) & 1u)) {
      hipEvent_t a = timer.get(), e = timer.get();
      ++g_nlaunch;
      hipExtLaunchKernelGGL(kernel, g, b, 0, st, a, e, 0, args...);
      timer.pend.push_back({cls, a, e, bytes});
      if (timer.pend.size() > 4096) timer.flush();  // bounded number of live events
    } else {
      hipLaunchKernelGGL(kernel, g, b, 0, st, args...);
    }
  }
  // The solvers' host reads (convergence tests, |r_0|) wait by polling the event instead of a blocking
  // synchronize: a blocking wait that outlasts the runtime's short active spin sleeps on an interrupt, and
  // its wake-up left the GPU idle ~0.1 ms after every pressure solve (r10x trace: 124 us before each
  // k_grad_proj).
  static constexpr int spin_us = 500;
  hipEvent_t ev_wait = nullptr;
  void wait_event(hipEvent_t e) {
    // a bounded spin (the solvers' reads wait tens of microseconds): a longer wait blocks, so no host core
    // stays pinned beside other ranks' and the setup's threads
    const auto t0 = std::chrono::steady_clock::now();
    for (int k = 0;; ++k) {
      const hipError_t q = hipEventQuery(e);
      if (q == hipSuccess) return;
      if (q != hipErrorNotReady) HIPCHK(q);
      if ((k & 63) == 63 && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(spin_us)) {
        HIPCHK(hipEventSynchronize(e));
        return;
      }
#if defined(__x86_64__)
      __builtin_ia32_pause();
#endif
    }
  }
  void sync_st() {  // hipStreamSynchronize(st) for the solvers' reads
    if (!ev_wait) HIPCHK(hipEventCreateWithFlags(&ev_wait, hipEventDisableTiming));
    HIPCHK(hipEventRecord(ev_wait, st));
    wait_event(ev_wait);
  }

  // k_sl over rows [row0, row0 + n) of the full replica c (cout: the new values), either locator
  void sl_launch(int nb, i64 row0, i64 n, const double* vx, const double* vy, double dt, const double* cf, double* cn,
                 const double* w, int32_t* nf, RedOut ro = RedOut{}) {
    const MeshDev M{mx, my, mtri, mesh.T};
    if (lat_sl) {
      // per row: coordinates 16, u 16, c 8 (the departure triangle's vertices lie near the row: their
      // coordinate and c lines are the rows' own), home face 4, lattice cell entries 8 and fast-accept
      // radii 8 (two triangles per node), the mixing weight 8, c_new written 8
      const double sl_bytes = (16.0 + 16.0 + 8.0 + 4.0 + 8.0 + 8.0 + (w ? 8.0 : 0.0) + 8.0) * (double)n;
      klaunch(4, sl_bytes, k_sl<LatLocDev>, dim3(nb), dim3(BS), M, llgrid, (int64_t)row0, (int64_t)n, vx,
              vy, dt, cf, cn, w, nf, part_sl, sl_queue, sl_qcnt);
      // the queued rows: one wave per point (k_sl_wave, on k_sl's grid), or -- with the fused reductions (a
      // measurement knob) or PUCFEM_SL_WAVE=0 -- k_sl_slow on k_sl's grid, one lane per point
      if (sl_wave_mode == 2 && !ro.out) {
        const int32_t nq = nb * (BS / 64);
        if (nq > QSCAN_BS * QSCAN_PER) throw Error(PUCFEM_ESTATE, "k_sl grid larger than k_sl_qscan covers");
        hipLaunchKernelGGL(k_sl_qscan, dim3(1), dim3(QSCAN_BS), 0, st, (const int32_t*)sl_qcnt, nq, sl_qoff);
        KCHK();
        klaunch(8, 0.0, k_sl_wq, dim3(nb), dim3(BS), M, llgrid, cgrid, (int64_t)row0, (int64_t)n, (int32_t)nb, vx, vy,
                dt, cf, cn, nf, sl_queue, (const int32_t*)sl_qoff, nq);
        KCHK();
        hipLaunchKernelGGL(k_sl_qsum, dim3(nb), dim3(BS), 0, st, (int64_t)row0, (int64_t)n, (const double*)cn, w,
                           part_sl, (const int32_t*)sl_queue, (const int32_t*)sl_qcnt);
      } else if (sl_wave && !ro.out)
        klaunch(8, 0.0, k_sl_wave, dim3(nb), dim3(BS), M, llgrid, cgrid, (int64_t)row0, (int64_t)n, vx, vy, dt, cf, cn,
                w, nf, part_sl, (const int32_t*)sl_queue, (const int32_t*)sl_qcnt);
      else
        klaunch(8, 0.0, k_sl_slow<LatLocDev>, dim3(nb), dim3(BS), M, llgrid, cgrid, (int64_t)row0, (int64_t)n, vx, vy,
                dt, cf, cn, w, nf, part_sl, (const int32_t*)sl_queue, (const int32_t*)sl_qcnt, ro);
    } else if (sl_rec_wave(n)) {
      klaunch(4, 8.0 * 6 * (double)n, k_sl_rec_wave, dim3(nb), dim3(BS), M, lgrid, cgrid, (int64_t)row0, (int64_t)n, vx,
              vy, dt, cf, cn, w, nf, part_sl, ro);
    } else {
      klaunch(4, 8.0 * 6 * (double)n, k_sl<LocDev>, dim3(nb), dim3(BS), M, lgrid, (int64_t)row0, (int64_t)n, vx, vy,
              dt, cf, cn, w, nf, part_sl, sl_queue, sl_qcnt);
      klaunch(8, 0.0, k_sl_slow<LocDev>, dim3(nb), dim3(BS), M, lgrid, cgrid, (int64_t)row0, (int64_t)n, vx, vy, dt,
              cf, cn, w, nf, part_sl, (const int32_t*)sl_queue, (const int32_t*)sl_qcnt, ro);
    }
  }

  // ------------------------------------------------------------------ dye channels (pucfem_dye_channels.hpp)
  // K extra dye fields advected beside c (PUCFEM_F_DYES), channel-major in the internal numbering: two K x N sets,
  // swapped after every launch (a launch cannot write a vector that other rows still gather from).  The buffers are
  // freed when the channels are dropped (they are not in `allocs`).
  int ndye = 0;
  double *dye_cur = nullptr, *dye_nxt = nullptr;
  int32_t* dye_nfpart = nullptr;  // per block of the last channel launch: its not-found rows
  int dye_nb = 0;                 // that launch's blocks (0: none since the channels were set)
  i64 dye_steps = 0;
  static int nb_dye(i64 n) { return (int)std::max<i64>(1, std::min<i64>(SLB, (n + BS - 1) / BS)); }
  // the not-found rows of the last one-pass launch (k_sl_multi, k_sl_vel): its nb blocks' counts, in block order
  int64_t nf_rows(const int32_t* nfpart, int nb) {
    if (!nfpart || nb <= 0) return 0;
    std::vector<int32_t> part((size_t)nb);
    d2h(part.data(), nfpart, sizeof(int32_t) * part.size());
    return std::accumulate(part.begin(), part.end(), (int64_t)0);
  }
  // per row: coordinates 16, u 16 and the locator's share as sl_launch counts it (lattice: home face 4, cell
  // entries 8, radii 8); per channel and row: the old value read 8 (the vertices' lines are the rows' own), the
  // new one written 8
  double dye_launch_bytes(int nch, i64 n) const { return ((lat_sl ? 52.0 : 32.0) + 16.0 * nch) * (double)n; }
  // the single-rank explicit-dye Stokes context the channels live on
  void dye_ready() const {
    need_built();
    auto state = [](bool ok, const char* msg) {
      if (!ok) throw Error(PUCFEM_ESTATE, msg);
    };
    state(scheme == PUCFEM_STOKES_COLOR, "dye channels need a STOKES_COLOR context");
    state(!dist() && world == 1,
          "dye channels are single-rank (a multi-rank context would need the dye's wide halo per channel)");
    state(!dye_impl, "dye channels follow the semi-Lagrangian dye (dye_scheme = 0)");
    need_dev();
    state(has_cgrid && has_locator(), "the context has no point locator");
  }
  void drop_dyes() {
    if (!dye_cur && !dye_nfpart) {
      ndye = 0;
      return;
    }
    if (st) (void)hipStreamSynchronize(st);
    if (st_sl) (void)hipStreamSynchronize(st_sl);
    for (void* q : {(void*)dye_cur, (void*)dye_nxt, (void*)dye_nfpart})
      if (q) (void)hipFree(q);
    dye_cur = dye_nxt = nullptr;
    dye_nfpart = nullptr;
    ndye = dye_nb = 0;
    dye_steps = 0;
  }
  // K channels from buf (K x N, the caller's numbering); K = 0 removes them
  void set_dyes(int K, const double* buf) {
    const i64 N = mesh.N;
    for (int t = 0; t < b_n; ++t)
      if (b_field[t] != PUCFEM_F_C) {  // (a buoyancy term names a channel being removed or redefined: buoyancy off)
        b_n = 0;
        force_changed();
      }
    if (K != ndye) {
      drop_dyes();
      if (K > 0) {
        const size_t bytes = sizeof(double) * (size_t)K * (size_t)N;
        HIPCHK(hipMalloc(reinterpret_cast<void**>(&dye_cur), bytes));
        HIPCHK(hipMalloc(reinterpret_cast<void**>(&dye_nxt), bytes));
        HIPCHK(hipMalloc(reinterpret_cast<void**>(&dye_nfpart), sizeof(int32_t) * SLB));
        HIPCHK(hipMemsetAsync(dye_nxt, 0, bytes, st));
        HIPCHK(hipMemsetAsync(dye_nfpart, 0, sizeof(int32_t) * SLB, st));
        ndye = K;
      }
    }
    dye_steps = 0;
    dye_nb = 0;
    if (mc_ch) mc_dye_fit();  // (the MacCormack set holds one field per channel)
    put_all(1, K, buf, dye_cur);
    HIPCHK(hipStreamSynchronize(st));
  }
  size_t dye_dev_bytes() const {
    return ndye ? 2 * sizeof(double) * (size_t)ndye * (size_t)mesh.N + sizeof(int32_t) * SLB : 0;
  }

  // ------------------------------------------------------------------ inertia (pucfem_inertia.hpp)
  // With inertia on, stokes_step advects the velocity by itself, u_a = SL(u^n; u^n, dt), in front of the viscous
  // solve, which then reads u_a wherever it read u^n: as its right-hand side and as the base of its start and of its
  // increments.  u_adv is one N x 2 interleaved buffer in the internal numbering, allocated when inertia is first
  // switched on and freed by drop_inertia (it is not in `allocs`): a context that never enables it holds no new
  // memory and launches nothing new.
  bool inertia = false;
  double* u_adv = nullptr;
  int32_t* adv_nfpart = nullptr;  // per block of the last inertial launch: its not-found rows
  int adv_nb = 0;                 // that launch's blocks (0: none since inertia was switched on)
  i64 adv_steps = 0;              // inertial steps since inertia was switched on
  bool adv_valid = false;         // u_adv holds the u_a of an inertial step
  // per row: coordinates 16, u 16, the locator's share as sl_launch counts it (lattice: home face 4, cell entries 8,
  // radii 8), the pair written 16 (the gathered vertices' lines are the rows' own)
  double vel_launch_bytes(i64 n) const { return (48.0 + (lat_sl ? 20.0 : 0.0)) * (double)n; }
  // the single-rank Stokes context inertia lives on
  void inertia_ready() const {
    need_built();
    auto state = [](bool ok, const char* msg) {
      if (!ok) throw Error(PUCFEM_ESTATE, msg);
    };
    state(scheme == PUCFEM_STOKES_COLOR || scheme == PUCFEM_STOKES_FOOD, "inertia needs a Stokes context");
    state(!dist() && world == 1, "inertia is single-rank (a multi-rank context would need a wide halo of u)");
    need_dev();
    state(has_cgrid && has_locator(), "the context has no point locator");
  }
  // the inertial part of a step, on the main stream in front of the viscous solve (f = u = the current velocity),
  // into the same buffers and counts under every mode
  void inertia_step() {
    if (!inertia) return;
    const TransportMode m{adv_vel, trj_vel};
    TransportWork w;
    w.nfpart = adv_nfpart;
    if (m.mc()) w.ch = mcv_ch, w.rec = mcv_rec, w.cnt = mcv_cnt;
    if (m.mid()) w.mid = trjv_mid;
    transport_pairs(m, lp.r0, lp.n_own, ux, prm.dt, ux, u_adv, w);
    const int nb = nb_dye(lp.n_own);
    if (m.mc()) mcv_nb = nb, ++mcv_steps;
    if (m.mid()) trjv_nb = nb, ++trjv_steps;
    adv_nb = nb;
    ++adv_steps;
    adv_valid = true;
  }
  void drop_inertia() {
    inertia = false;
    adv_nb = 0;
    adv_steps = 0;
    adv_valid = false;
    if (!u_adv && !adv_nfpart) return;
    if (st) (void)hipStreamSynchronize(st);
    for (void* q : {(void*)u_adv, (void*)adv_nfpart})
      if (q) (void)hipFree(q);
    u_adv = nullptr;
    adv_nfpart = nullptr;
  }
  void set_inertia(bool on) {
    inertia_ready();
    if (on && ens) throw Error(PUCFEM_ESTATE, "inertia cannot be switched on while the context has an ensemble");
    if (on == inertia) return;
    if (on && !u_adv) {
      const size_t bytes = sizeof(double) * 2 * (size_t)mesh.N;
      HIPCHK(hipMalloc(reinterpret_cast<void**>(&u_adv), bytes));
      HIPCHK(hipMalloc(reinterpret_cast<void**>(&adv_nfpart), sizeof(int32_t) * SLB));
      HIPCHK(hipMemsetAsync(u_adv, 0, bytes, st));
      HIPCHK(hipMemsetAsync(adv_nfpart, 0, sizeof(int32_t) * SLB, st));
      HIPCHK(hipStreamSynchronize(st));
    }
    inertia = on;
    if (on) {
      adv_steps = 0;
      adv_nb = 0;
    }
    have_vinc = 0;  // the viscous solve's right-hand side changes its meaning: no last increment
  }
  size_t inertia_dev_bytes() const {
    return u_adv ? sizeof(double) * 2 * (size_t)mesh.N + sizeof(int32_t) * SLB : 0;
  }

  // ------------------------------------------------------------------ body forces (pucfem_force.hpp)
  // With a force set, stokes_step forms r = base + dt * f (base: u^n, or u_a with inertia on) behind inertia_step and
  // in front of the viscous solve, which then reads r wherever it read base.  u_rhs is one interleaved buffer over the
  // owned rows, allocated when a force is first set and freed by drop_force (it is not in `allocs`), as the nodal
  // field is: a context that never sets a force holds no new memory and launches nothing new.
  bool f_uni = false;
  double f_F[2] = {0.0, 0.0};
  double* f_nodal = nullptr;  // the nodal field's pairs, owned rows in the internal numbering (null: none)
  int b_n = 0;                // buoyancy terms (0: off)
  int32_t b_field[FORCE_MAX_TERMS] = {};
  double b_beta[FORCE_MAX_TERMS] = {}, b_ref[FORCE_MAX_TERMS] = {}, b_g[2] = {0.0, 0.0};
  double* u_rhs = nullptr;
  bool rhs_valid = false;  // u_rhs holds the r of a forced step
  i64 force_steps = 0;     // forced steps since the setting last changed
  int force_mask() const { return (f_uni ? 1 : 0) | (f_nodal ? 2 : 0) | (b_n ? 4 : 0); }
  bool forced() const { return force_mask() != 0; }
  // a built Stokes context (checked before the device is asked for)
  void force_ready() const {
    need_built();
    if (scheme != PUCFEM_STOKES_COLOR && scheme != PUCFEM_STOKES_FOOD)
      throw Error(PUCFEM_ESTATE, "body forces need a Stokes context");
  }
  // buoyancy reads the dye at the start of the step: a single-rank STOKES_COLOR context (a partitioned one finishes
  // step n's dye behind step n + 1's viscous solve, dye_tail_dist)
  void buoyancy_ready() const {
    force_ready();
    if (scheme != PUCFEM_STOKES_COLOR) throw Error(PUCFEM_ESTATE, "buoyancy needs a STOKES_COLOR context: STOKES_FOOD has no dye");
    if (dist() || world != 1)
      throw Error(PUCFEM_ESTATE, "buoyancy is single-rank (a partitioned step's dye is finished after the next viscous solve)");
  }
  double force_launch_bytes(int mask, int nterms, i64 n) const {
    return (32.0 + ((mask & 2) ? 16.0 : 0.0) + ((mask & 4) ? 8.0 * nterms : 0.0)) * (double)n;
  }
  // the current setting as the kernel takes it (the dye pointers as they stand now: call after sl_join)
  ForceTerms force_terms() const {
    ForceTerms T{};
    T.fx = f_F[0];
    T.fy = f_F[1];
    T.gx = b_g[0];
    T.gy = b_g[1];
    T.nterms = b_n;
    for (int t = 0; t < b_n; ++t) {
      T.s[t] = b_field[t] == PUCFEM_F_C ? c_full + lp.r0 : dye_cur + (size_t)(b_field[t] - PUCFEM_F_DYE0) * (size_t)mesh.N;
      T.beta[t] = b_beta[t];
      T.ref[t] = b_ref[t];
    }
    return T;
  }
  // k_force_rhs over the owned rows on the current stream: out = base + dt * f (RHS), or f itself
  template <bool RHS>
  void force_launch(const double* base2, double dt, double* out2) {
    const i64 n = lp.n_own;
    const int mask = force_mask();
    const ForceTerms T = force_terms();
    const dbl2* base = reinterpret_cast<const dbl2*>(base2);
    const dbl2* fn = reinterpret_cast<const dbl2*>(f_nodal);
    dbl2* out = reinterpret_cast<dbl2*>(out2);
    const double bytes = force_launch_bytes(mask, b_n, n) - (RHS ? 0.0 : 16.0 * (double)n);
    auto go = [&](auto uni, auto nod, auto buo) {
      klaunch(-1, bytes, k_force_rhs<decltype(uni)::value, decltype(nod)::value, decltype(buo)::value, RHS>,
              dim3(grid_ew(n)), dim3(BS), (int64_t)n, base, dt, fn, T, out);
    };
    using Y = std::true_type;
    using N = std::false_type;
    switch (mask) {
      case 0: go(N{}, N{}, N{}); break;  // (f = 0: PUCFEM_F_FORCE and pucfem_force_apply with nothing set)
      case 1: go(Y{}, N{}, N{}); break;
      case 2: go(N{}, Y{}, N{}); break;
      case 3: go(Y{}, Y{}, N{}); break;
      case 4: go(N{}, N{}, Y{}); break;
      case 5: go(Y{}, N{}, Y{}); break;
      case 6: go(N{}, Y{}, Y{}); break;
      default: go(Y{}, Y{}, Y{}); break;
    }
    KCHK();
  }
  // the forced part of a step, on the main stream behind inertia_step.  Buoyancy reads c^n, which the previous step's
  // overlapped dye tail writes on the side stream: the main stream joins it first (and c_full is read after the join:
  // the tail swapped c_full / c_new when it was queued)
  void force_step() {
    if (!forced()) return;
    if (b_n) sl_join();
    force_launch<true>(inertia ? u_adv : ux, prm.dt, u_rhs);
    ++force_steps;
    rhs_valid = true;
  }
  void force_alloc() {
    if (u_rhs) return;
    const size_t bytes = sizeof(double) * 2 * (size_t)std::max<i64>(1, lp.n_own);
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&u_rhs), bytes));
    HIPCHK(hipMemsetAsync(u_rhs, 0, bytes, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  // a setting changed: the counts start again and the viscous solve's right-hand side changes its meaning
  void force_changed() {
    force_steps = 0;
    have_vinc = 0;
    if (forced()) force_alloc();
  }
  void drop_force() {
    f_uni = false;
    f_F[0] = f_F[1] = 0.0;
    b_n = 0;
    force_steps = 0;
    rhs_valid = false;
    if (!u_rhs && !f_nodal) return;
    if (st) (void)hipStreamSynchronize(st);
    for (void* q : {(void*)u_rhs, (void*)f_nodal})
      if (q) (void)hipFree(q);
    u_rhs = f_nodal = nullptr;
  }
  size_t force_dev_bytes() const {
    const size_t plane = sizeof(double) * 2 * (size_t)std::max<i64>(1, lp.n_own);
    return (u_rhs ? plane : 0) + (f_nodal ? plane : 0);
  }

  // ------------------------------------------------------------------ swimmer loads (pucfem_loads.hpp)
  // The surface edge list (host, caller numbering: surf) and its device image, (triangle, local edge) pairs: mtri keeps
  // the caller's triangle order and vertex order, so the pairs need no renumbering.  Everything here is allocated at
  // a call's first need and freed by drop_loads (not in `allocs`): a context that never asks holds no new memory, and
  // with the record off (ld_cap == 0) a step launches nothing new.
  SurfaceEdges surf;
  bool surf_valid = false;
  int2* ld_edge = nullptr;
  int32_t ld_nE = 0;
  double *ld_part = nullptr, *ld_out = nullptr, *ld_eout = nullptr, *ld_ring = nullptr;
  unsigned* ld_cnt = nullptr;
  int64_t* ld_count = nullptr;
  int32_t ld_cap = 0;  // record capacity (0: off), the context's and its ensemble's
  const SurfaceEdges& surface() {
    if (!has_mesh) throw Error(PUCFEM_ESTATE, "no mesh has been uploaded");
    if (!surf_valid) {
      surface_edges(mesh, surf);
      surf_valid = true;
    }
    return surf;
  }
  // a built single-rank Stokes context; member >= 0 needs its ensemble (all checked before the device is asked for)
  void loads_ready(int32_t member) const {
    need_built();
    if (scheme != PUCFEM_STOKES_COLOR && scheme != PUCFEM_STOKES_FOOD)
      throw Error(PUCFEM_ESTATE, "swimmer loads need a Stokes context");
    if (dist() || world != 1) throw Error(PUCFEM_ESTATE, "swimmer loads are single-rank");
    if (member >= 0 && !ens) throw Error(PUCFEM_ESTATE, "no ensemble on this context: call pucfem_ens_create first");
    need_dev();
  }
  int loads_nbe() const { return std::max(1, (ld_nE + BS - 1) / BS); }
  int loads_nbt() const { return (int)std::max<i64>(1, std::min<i64>(LOADS_TRI_MAXB, (mesh.T + BS - 1) / BS)); }
  int loads_grid() const { return loads_nbe() + loads_nbt(); }
  template <class T>
  T* loads_alloc(size_t count) {
    void* q = nullptr;
    const size_t b = sizeof(T) * std::max<size_t>(1, count);
    HIPCHK(hipMalloc(&q, b));
    HIPCHK(hipMemsetAsync(q, 0, b, st));
    return (T*)q;
  }
  void loads_bufs() {
    if (ld_edge) return;
    const SurfaceEdges& S = surface();
    std::vector<int2> h((size_t)S.size());
    for (i64 e = 0; e < S.size(); ++e) {
      const i32 t = S.tri[e];
      const int k = mesh.tri[3 * (i64)t] == S.a[e] ? 0 : mesh.tri[3 * (i64)t + 1] == S.a[e] ? 1 : 2;
      h[e] = int2{t, k};
    }
    ld_nE = (int32_t)S.size();
    ld_edge = loads_alloc<int2>(h.size());
    if (!h.empty()) h2d(ld_edge, h.data(), sizeof(int2) * h.size());
    ld_part = loads_alloc<double>((size_t)LOADS_NV * loads_grid());
    ld_out = loads_alloc<double>(ENS_VALS);
    ld_eout = loads_alloc<double>((size_t)LOADS_EV * ld_nE);
    ld_cnt = loads_alloc<unsigned>(1);
  }
  // algorithmic bytes of a launch that stores no per-edge values: the triangles' ids once, every node's coordinates
  // and velocity once (each vector counted once per row, as everywhere), an edge's record and four pressures
  double loads_launch_bytes() const {
    return 12.0 * (double)mesh.T + 32.0 * (double)mesh.N + (8.0 + 32.0) * (double)ld_nE;
  }
  // k_loads on the current stream over nm members (1: a single context's fields, or one member's planes); eout null:
  // no per-edge values stored
  void loads_launch(int32_t nm, const double* u, i64 ustride, const double* pa, const double* pb, i64 pstride,
                    const int32_t* mo, double* eout, double* part, const RedOut& r, const LoadsRec& rec) {
    hipLaunchKernelGGL(k_loads, dim3(loads_grid(), nm), dim3(BS), 0, st, MeshDev{mx, my, mtri, mesh.T},
                       (const int2*)ld_edge, ld_nE, (int32_t)loads_nbe(), u, (int64_t)ustride, pa, pb, (int64_t)pstride,
                       mo, prm.nu, prm.center_x, prm.center_y, eout, (int64_t)LOADS_EV * ld_nE, part, r, rec);
    KCHK();
  }
  // the context's own u and the last step's pressures (kept in the solves' y on the p_from_y path, where a periodic
  // slave's value is its master's)
  void loads_own(double* eout, const LoadsRec& rec) {
    loads_bufs();
    const RedOut r{ld_out, nullptr, ld_cnt, LOADS_NV, 0, 0u};
    loads_launch(1, ux, 0, p_from_y ? yp : p, p_from_y ? yp2 : p2, 0, p_from_y ? dmaster_of : nullptr, eout, ld_part,
                 r, rec);
  }
  // the record's part of a step, behind the step's final u and p2 on the main stream
  void loads_step() {
    if (ld_cap > 0) loads_own(nullptr, LoadsRec{ld_ring, ld_count, ld_cap});
  }
  void loads_record_set(int32_t cap) {
    if (st) HIPCHK(hipStreamSynchronize(st));
    for (void* q : {(void*)ld_ring, (void*)ld_count})
      if (q) (void)hipFree(q);
    ld_ring = nullptr;
    ld_count = nullptr;
    ld_cap = cap;
    if (cap > 0) {
      loads_bufs();
      ld_ring = loads_alloc<double>((size_t)cap * LOADS_ROW);
      ld_count = loads_alloc<int64_t>(1);
    }
  }
  void drop_loads() {
    surf_valid = false;
    ld_cap = 0;
    ld_nE = 0;
    if (!ld_edge && !ld_ring) return;
    if (st) (void)hipStreamSynchronize(st);
    for (void* q : {(void*)ld_edge, (void*)ld_part, (void*)ld_out, (void*)ld_eout, (void*)ld_ring, (void*)ld_cnt,
                    (void*)ld_count})
      if (q) (void)hipFree(q);
    ld_edge = nullptr;
    ld_part = ld_out = ld_eout = ld_ring = nullptr;
    ld_cnt = nullptr;
    ld_count = nullptr;
  }

  // ------------------------------------------------------------------ time-dependent strokes (pucfem_stroke.hpp)
  // With a stroke set, stokes_step rewrites the driven entries of ddval in front of everything else from row
  // (start + s) mod P of the table; s is sk_ctr, in device memory.  The buffers are allocated when a stroke is set and
  // freed by drop_stroke (they are not in `allocs`): a context that never sets one holds no new memory and launches
  // nothing new.  dval_build: the values build uploaded, which clearing the stroke restores.
  int sk_K = 0;  // modes (0: off)
  i64 sk_P = 0, sk_start = 0;
  int32_t sk_n = 0;  // driven entries
  double *sk_amp = nullptr, *sk_shape = nullptr, *sk_dir = nullptr;
  int32_t* sk_q = nullptr;
  i64* sk_ctr = nullptr;
  std::vector<double> dval_build;
  bool stroked() const { return sk_K > 0; }
  // a built single-rank Stokes context (checked before the device is asked for)
  void stroke_ready() const {
    need_built();
    if (scheme != PUCFEM_STOKES_COLOR && scheme != PUCFEM_STOKES_FOOD)
      throw Error(PUCFEM_ESTATE, "strokes need a Stokes context");
    if (dist() || world != 1) throw Error(PUCFEM_ESTATE, "strokes are single-rank");
    need_dev();
    if (dir_ncomp != 2) throw Error(PUCFEM_ESTATE, "strokes need two-component Dirichlet values");
  }
  // the position in ddval of every caller node's kept Dirichlet entry (-1: not a Dirichlet node), as build orders them
  std::vector<i32> dir_positions() const {
    std::vector<i32> pos((size_t)mesh.N, -1);
    std::vector<i64> last((size_t)mesh.N, -1);
    for (size_t k = 0; k < dir_nodes.size(); ++k) last[dir_nodes[k]] = (i64)k;
    i32 q = 0;
    for (size_t k = 0; k < dir_nodes.size(); ++k)
      if (last[dir_nodes[k]] == (i64)k) pos[dir_nodes[k]] = q++;
    if (q != ndir) throw Error(PUCFEM_ESTATE, "Dirichlet list changed since the build");
    return pos;
  }
  double stroke_launch_bytes() const { return (32.0 + 8.0 * sk_K) * (double)sk_n; }
  // k_stroke_bc on the current stream: the row of counter ctr, which is advanced (the step's launch: sk_ctr into
  // ddval), or with ctr null row `row`, into val
  void stroke_launch(i64* ctr, i64 row, double* val) {
    klaunch(-1, stroke_launch_bytes(), k_stroke_bc, dim3(1), dim3(BS), sk_K, (int64_t)sk_P, (int64_t)sk_start,
            (int64_t*)ctr, (int64_t)row, (const double*)sk_amp, sk_n,
            (const int32_t*)sk_q, (const double*)sk_shape, reinterpret_cast<const dbl2*>(sk_dir),
            reinterpret_cast<dbl2*>(val));
    KCHK();
  }
  // the stroke's part of a step, on the main stream in front of inertia_step: nothing on the side stream reads ddval
  void stroke_step() {
    if (stroked()) stroke_launch(sk_ctr, 0, ddval);
  }
  // off: the buffers freed and, with `restore`, build's values back in ddval
  void drop_stroke(bool restore) {
    const bool was = stroked();
    sk_K = 0;
    sk_P = sk_start = 0;
    sk_n = 0;
    if (!sk_ctr && !was) return;
    if (st) (void)hipStreamSynchronize(st);
    for (void* q : {(void*)sk_amp, (void*)sk_shape, (void*)sk_dir, (void*)sk_q, (void*)sk_ctr})
      if (q) (void)hipFree(q);
    sk_amp = sk_shape = sk_dir = nullptr;
    sk_q = nullptr;
    sk_ctr = nullptr;
    if (restore && was && ddval && !dval_build.empty()) {
      h2d(ddval, dval_build.data(), sizeof(double) * dval_build.size());
      HIPCHK(hipStreamSynchronize(st));
      have_vinc = 0;  // (as a force change: the boundary data of the viscous solve changed)
    }
  }
  // a stroke buffer of its own (freed by drop_stroke): a copy of src, or zeros
  template <class T>
  T* stroke_buf(const T* src, size_t count) {
    T* p = nullptr;
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&p), sizeof(T) * std::max<size_t>(1, count)));
    if (src) h2d(p, src, sizeof(T) * count);
    else HIPCHK(hipMemsetAsync(p, 0, sizeof(T) * std::max<size_t>(1, count), st));
    return p;
  }

  // ------------------------------------------------------------------ MacCormack advection (pucfem_maccormack.hpp)
  // pucfem_set_advection: the dye (c and its channels) and, with inertia on, the velocity move by the two-pass
  // limited MacCormack step instead of the first-order one.  Per transported set: the intermediate fields ch, one
  // 16-byte record per row (pass 1's triangle) and the blocks' counts.  The dye's and the velocity's sets are
  // separate: a step's dye tail runs on the side stream beside the next step's inertial launch.  Allocated when a
  // scheme is first switched on and freed by drop_advection (they are not in `allocs`): a context that never enables
  // it holds no new memory and launches nothing new.
  int adv_dye = 0, adv_vel = 0;  // PUCFEM_ADV_SL / PUCFEM_ADV_MACCORMACK
  double* mc_ch = nullptr;       // (1 + K) x N: c's ch, then the channels'
  int mc_fields = 0;             // the fields mc_ch holds
  int4* mc_rec = nullptr;        // N
  int32_t* mc_nfpart = nullptr;  // pass 1's not-found counts when there are no channels (else dye_nfpart) (SLB)
  double* mc_nfd = nullptr;      // the same as doubles, for the step record's reduction (SLB)
  int32_t* mc_cnt = nullptr;     // pass 2's three counts per block (3 x SLB)
  int mc_nb = 0;                 // blocks of the last dye launch (0: none since the scheme was set)
  i64 mc_steps = 0;
  double* mcv_ch = nullptr;      // N x 2 interleaved
  int4* mcv_rec = nullptr;
  int32_t* mcv_cnt = nullptr;
  int mcv_nb = 0;
  i64 mcv_steps = 0;
  // pass 1 as dye_launch_bytes / vel_launch_bytes count a first-order launch, plus the record written 16; pass 2: the
  // coordinates, u and the locator's share again, the record read 16, per field c and ch read and the result written
  double mc_bytes1(int nf, i64 n) const { return dye_launch_bytes(nf, n) + 16.0 * (double)n; }
  double mc_bytes2(int nf, i64 n) const { return ((lat_sl ? 52.0 : 32.0) + 16.0 + 24.0 * nf) * (double)n; }
  double mcv_bytes1(i64 n) const { return vel_launch_bytes(n) + 16.0 * (double)n; }
  // (the pair form counts f as vel_launch_bytes does: the gathered vertices' lines are the rows' own, f = u)
  double mcv_bytes2(i64 n) const { return ((lat_sl ? 52.0 : 32.0) + 16.0 + 32.0) * (double)n; }
  // the three counts of a pass-2 launch, its nb blocks summed in block order
  void mc_counts(const int32_t* cnt, int nb, int64_t* out3) {
    out3[0] = out3[1] = out3[2] = 0;
    if (!cnt || nb <= 0) return;
    std::vector<int32_t> part(3 * (size_t)nb);
    d2h(part.data(), cnt, sizeof(int32_t) * part.size());
    for (int b = 0; b < nb; ++b)
      for (int j = 0; j < 3; ++j) out3[j] += part[3 * (size_t)b + j];
  }
  // mc_ch sized for c and the current channels
  void mc_dye_fit() {
    if (mc_ch && mc_fields == 1 + ndye) return;
    if (st) (void)hipStreamSynchronize(st);
    if (st_sl) (void)hipStreamSynchronize(st_sl);
    if (mc_ch) (void)hipFree(mc_ch);
    mc_ch = nullptr;
    mc_fields = 1 + ndye;
    const size_t bytes = sizeof(double) * (size_t)mc_fields * (size_t)mesh.N;
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&mc_ch), bytes));
    HIPCHK(hipMemsetAsync(mc_ch, 0, bytes, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  void drop_advection() {
    adv_dye = adv_vel = 0;
    mc_nb = mcv_nb = 0;
    mc_steps = mcv_steps = 0;
    mc_fields = 0;
    if (!mc_rec && !mcv_rec) return;
    if (st) (void)hipStreamSynchronize(st);
    if (st_sl) (void)hipStreamSynchronize(st_sl);
    for (void* q : {(void*)mc_ch, (void*)mc_rec, (void*)mc_nfpart, (void*)mc_nfd, (void*)mc_cnt, (void*)mcv_ch,
                    (void*)mcv_rec, (void*)mcv_cnt})
      if (q) (void)hipFree(q);
    mc_ch = mc_nfd = mcv_ch = nullptr;
    mc_rec = mcv_rec = nullptr;
    mc_nfpart = mc_cnt = mcv_cnt = nullptr;
  }
  template <class T>
  void mc_alloc(T*& p, size_t count) {
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&p), sizeof(T) * count));
    HIPCHK(hipMemsetAsync(p, 0, sizeof(T) * count, st));
  }
  void set_advection(int what, int sch) {
    if (what & ~(PUCFEM_ADV_DYE | PUCFEM_ADV_VELOCITY) || what == 0)
      throw Error(PUCFEM_EINVAL, "what is a mask of PUCFEM_ADV_DYE and PUCFEM_ADV_VELOCITY");
    if (sch != PUCFEM_ADV_SL && sch != PUCFEM_ADV_MACCORMACK) throw Error(PUCFEM_EINVAL, "unknown advection scheme");
    if (what & PUCFEM_ADV_DYE) dye_ready();
    if (what & PUCFEM_ADV_VELOCITY) inertia_ready();
    if (sch && ens) throw Error(PUCFEM_ESTATE, "MacCormack advection cannot be switched on while the context has an ensemble");
    const size_t N = (size_t)mesh.N;
    if ((what & PUCFEM_ADV_DYE) && sch != adv_dye) {
      if (st_sl) HIPCHK(hipStreamSynchronize(st_sl));
      if (sch) {
        mc_dye_fit();
        if (!mc_rec) {
          mc_alloc(mc_rec, N);
          mc_alloc(mc_nfpart, (size_t)SLB);
          mc_alloc(mc_nfd, (size_t)SLB);
          mc_alloc(mc_cnt, 3 * (size_t)SLB);
          HIPCHK(hipStreamSynchronize(st));
        }
        mc_steps = 0;
        mc_nb = 0;
      }
      adv_dye = sch;
    }
    if ((what & PUCFEM_ADV_VELOCITY) && sch != adv_vel) {
      if (sch) {
        if (!mcv_rec) {
          mc_alloc(mcv_ch, 2 * N);
          mc_alloc(mcv_rec, N);
          mc_alloc(mcv_cnt, 3 * (size_t)SLB);
          HIPCHK(hipStreamSynchronize(st));
        }
        mcv_steps = 0;
        mcv_nb = 0;
      }
      adv_vel = sch;
      have_vinc = 0;  // (as switching inertia: the advected right-hand side changes)
    }
  }
  size_t advection_dev_bytes() const {
    const size_t N = (size_t)mesh.N;
    size_t b = 0;
    if (mc_ch) b += sizeof(double) * (size_t)mc_fields * N;
    if (mc_rec) b += sizeof(int4) * N + sizeof(int32_t) * 4 * SLB + sizeof(double) * SLB;
    if (mcv_rec) b += sizeof(double) * 2 * N + sizeof(int4) * N + sizeof(int32_t) * 3 * SLB;
    return b;
  }

  // ------------------------------------------------------------------ midpoint trajectories (pucfem_trajectory.hpp)
  // pucfem_set_trajectory: the dye (c and its channels), the inertial step's velocity and the tracers follow the
  // midpoint trace instead of one straight step.  The fields keep their buffers (the dye's channel sets, u_adv, the
  // MacCormack sets): a part that is on launches k_trj_* where the Euler step launches k_sl / k_sl_multi / k_sl_vel /
  // k_mc_*, one launch per pass.  What a part holds of its own are the blocks' counts, allocated when it is first
  // switched on and freed by drop_trajectory (they are not in `allocs`).
  int trj_dye = PUCFEM_TRJ_EULER, trj_vel = PUCFEM_TRJ_EULER, trj_trc = PUCFEM_TRJ_EULER;
  int32_t* trjd_mid = nullptr;     // dye: the blocks' midpoint-not-found rows, pass 1 then pass 2 (2 x SLB)
  int32_t* trjd_nfpart = nullptr;  // ... final not-found rows where no other buffer takes them (SLB)
  double* trjd_nfd = nullptr;      // ... as doubles, for the step record (SLB)
  int32_t* trjv_mid = nullptr;     // velocity: as trjd_mid (2 x SLB)
  int32_t* trjt_fell = nullptr;    // tracers: the last launch's count (1)
  int trjd_nb = 0, trjv_nb = 0;    // blocks of the last dye / velocity launch with the part on (0: none)
  bool trjt_ran = false;
  i64 trjd_steps = 0, trjv_steps = 0, trjt_steps = 0;
  bool trj_any() const {
    return trj_dye == PUCFEM_TRJ_MIDPOINT || trj_vel == PUCFEM_TRJ_MIDPOINT || trj_trc == PUCFEM_TRJ_MIDPOINT;
  }
  // a fused pass reads what the composition's two launches read, less the midpoint velocity's store and load (32 B)
  double trj_bytes1(int nf, i64 n, bool rec) const {
    return dye_launch_bytes(nf, n) + vel_launch_bytes(n) - 32.0 * (double)n + (rec ? 16.0 * (double)n : 0.0);
  }
  double trj_bytes2(int nf, i64 n) const { return mc_bytes2(nf, n) + vel_launch_bytes(n) - 32.0 * (double)n; }
  double trjv_bytes1(i64 n, bool rec) const {
    return 2.0 * vel_launch_bytes(n) - 32.0 * (double)n + (rec ? 16.0 * (double)n : 0.0);
  }
  double trjv_bytes2(i64 n) const { return mcv_bytes2(n) + vel_launch_bytes(n) - 32.0 * (double)n; }
  // the single-rank STOKES_FOOD context the tracers live on
  void tracers_ready() const {
    need_built();
    auto state = [](bool ok, const char* msg) {
      if (!ok) throw Error(PUCFEM_ESTATE, msg);
    };
    state(scheme == PUCFEM_STOKES_FOOD, "tracer trajectories need a STOKES_FOOD context (the tracers)");
    state(!dist() && world == 1, "midpoint trajectories are single-rank (the midpoint would need a wide halo of u)");
    need_dev();
    state(has_tgrid, "the context has no tracer grid");
  }

  // ------------------------------------------------------------------ tracer stretching
  // pucfem_set_tracer_stretch: every tracer carries the deformation gradient F of the flow map along its path, updated
  // by the STRETCH instantiations of the tracer kernels in the tracer launch itself.  str_F (ntr x 4) is allocated
  // when the setting is switched on and freed when it is switched off (not in `allocs`); the summary's partials,
  // values and ticket are allocated at the first pucfem_tracer_stretch_info and freed with F.
  bool str_on = false;
  double* str_F = nullptr;
  i64 str_rows = 0;   // the rows str_F holds
  i64 str_steps = 0;  // tracer steps taken with it on since F was last reset
  double *str_part = nullptr, *str_out = nullptr;
  unsigned* str_cnt = nullptr;
  // the single-rank STOKES_FOOD context with tracers it lives on (decided before the device is asked for)
  void stretch_ready() const {
    need_built();
    auto state = [](bool ok, const char* msg) {
      if (!ok) throw Error(PUCFEM_ESTATE, msg);
    };
    state(scheme == PUCFEM_STOKES_FOOD, "tracer stretching needs a STOKES_FOOD context (the tracers)");
    state(!dist() && world == 1, "tracer stretching is single-rank (the multi-rank tracer step has no STRETCH form)");
    need_dev();
    state(has_tgrid, "the context has no tracer grid");
  }
  // n rows of F at `first` <- the identity (ordered on st)
  void stretch_identity(double* F, i64 first, i64 n) {
    if (n <= 0) return;
    std::vector<double> id(4 * (size_t)n, 0.0);
    for (i64 k = 0; k < n; ++k) id[4 * k] = id[4 * k + 3] = 1.0;
    h2d(F + 4 * first, id.data(), sizeof(double) * id.size());
  }
  void drop_stretch() {
    str_on = false;
    str_steps = 0;
    str_rows = 0;
    if (!str_F && !str_part) return;
    if (st) (void)hipStreamSynchronize(st);
    for (void* q : {(void*)str_F, (void*)str_part, (void*)str_out, (void*)str_cnt})
      if (q) (void)hipFree(q);
    str_F = str_part = str_out = nullptr;
    str_cnt = nullptr;
  }
  // F for the context's ntr tracers, the identity
  void stretch_fit() {
    if (str_rows != ntr || !str_F) {
      HIPCHK(hipStreamSynchronize(st));
      if (str_F) (void)hipFree(str_F);
      str_F = nullptr;
      mc_alloc(str_F, 4 * (size_t)std::max<i64>(1, ntr));
      str_rows = ntr;
    }
    stretch_identity(str_F, 0, ntr);
    str_steps = 0;
  }
  void set_stretch(bool on) {
    stretch_ready();
    if (ens)
      throw Error(PUCFEM_ESTATE,
                  "tracer stretching cannot be set while the context has an ensemble (members carry their own: "
                  "pucfem_ens_set_tracer_stretch)");
    if (ntr <= 0) throw Error(PUCFEM_ESTATE, "tracer stretching needs a context with tracers (set PUCFEM_F_TRACERS)");
    if (on == str_on) return;
    if (on) {
      stretch_fit();
      HIPCHK(hipStreamSynchronize(st));
      str_on = true;
    } else {
      drop_stretch();
    }
    // (a small-mesh context steps uncaptured while it is on; its captured graphs hold the plain step and are kept)
  }

  // ------------------------------------------------------------------ the transport layer
  // The one place that knows which kernels move a field under a mode, over rows [row0, row0 + n) of a single-rank
  // context on the current stream (u2: the full mesh's interleaved pairs):
  //   (SL, Euler)     k_sl_multi / k_sl_vel                 one pass
  //   (MC, Euler)     k_mc_fwd, k_mc_bwd (_vel)             two passes
  //   (SL, midpoint)  k_trj_fwd (_vel)                      one pass, straight into the result
  //   (MC, midpoint)  k_trj_fwd, k_trj_bwd (_vel)           two passes
  // The step (dye_transport_step, inertia_step), the unit entry points and the probes all launch through
  // transport_fields / transport_pairs; a new scheme or order is added to these two (and to ens_transport, their
  // ensemble twin).  c itself under (SL, Euler) is not here: it stays on sl_launch, whose k_sl fuses the mixing sums
  // and is a different kernel.
  struct TransportMode {
    int scheme = PUCFEM_ADV_SL, order = PUCFEM_TRJ_EULER;
    bool mc() const { return scheme == PUCFEM_ADV_MACCORMACK; }
    bool mid() const { return order == PUCFEM_TRJ_MIDPOINT; }
  };
  // a launch's work buffers; null where the mode (or the caller) has no use for one
  struct TransportWork {
    double* ch = nullptr;        // two-pass: pass 1's fields (c0's first where there is one, then the channels'; pairs)
    int4* rec = nullptr;         // two-pass: pass 1's triangle per row
    int32_t* marks = nullptr;    // per row: the not-found flag (SL, Euler) or the mode's marks
    int32_t* tri = nullptr;      // two-pass: pass 2's triangle per row
    int32_t* nfpart = nullptr;   // per block: the not-found rows (pass 1's)
    double* nfd = nullptr;       // ... as doubles (plain fields, beside a c0)
    int32_t* cnt = nullptr;      // two-pass: pass 2's three counts per block
    int32_t* mid = nullptr;      // midpoint: the blocks' midpoint-not-found rows, pass 1 then pass 2 (2 x SLB)
  };
  // plain fields: c0 -> out0 (optional; not under (SL, Euler), where k_sl_multi moves the channels only) and nch
  // channels cin -> cout of leading dimension N.  pass & 1: the first pass (the whole of a one-pass mode), pass & 2:
  // the second
  void transport_fields(TransportMode m, i64 row0, i64 n, const double* u2, double dt, const double* c0, double* out0,
                        int nch, const double* cin, double* cout, const TransportWork& w, int pass = 3) {
    const MeshDev M{mx, my, mtri, mesh.T};
    const dim3 nb(nb_dye(n));
    const double *vx = u2, *vy = u2 + 1, hdt = 0.5 * dt;
    const dbl2* u = reinterpret_cast<const dbl2*>(u2);
    const int nf = nch + (c0 ? 1 : 0);
    const int64_t N = mesh.N;
    double* ch0 = c0 ? w.ch : nullptr;            // (two-pass) c0's intermediate field ...
    double* chn = c0 && w.ch ? w.ch + N : w.ch;  // ... and the channels'
    with_loc([&](const auto& L) {
      using Loc = std::decay_t<decltype(L)>;
      if (m.mid()) {
        if ((pass & 1) && m.mc())
          klaunch(-1, trj_bytes1(nf, n, true), k_trj_fwd<Loc>, nb, dim3(BS), M, L, cgrid, (int64_t)row0, (int64_t)n, u,
                  dt, hdt, c0, ch0, (int32_t)nch, cin, chn, N, w.rec, w.marks, w.nfpart, w.nfd, w.mid);
        else if (pass & 1)
          klaunch(-1, trj_bytes1(nf, n, false), k_trj_fwd<Loc>, nb, dim3(BS), M, L, cgrid, (int64_t)row0, (int64_t)n,
                  u, dt, hdt, c0, out0, (int32_t)nch, cin, cout, N, (int4*)nullptr, w.marks, w.nfpart, w.nfd, w.mid);
        if ((pass & 2) && m.mc())
          klaunch(-1, trj_bytes2(nf, n), k_trj_bwd<Loc>, nb, dim3(BS), M, L, cgrid, (int64_t)row0, (int64_t)n, u, dt,
                  hdt, c0, (const double*)ch0, out0, (int32_t)nch, cin, (const double*)chn, cout, N,
                  (const int4*)w.rec, w.marks, w.tri, w.cnt, w.mid + SLB);
      } else if (m.mc()) {
        if (pass & 1)
          klaunch(-1, mc_bytes1(nf, n), k_mc_fwd<Loc>, nb, dim3(BS), M, L, cgrid, (int64_t)row0, (int64_t)n, vx, vy, dt,
                  c0, ch0, (int32_t)nch, cin, chn, N, w.rec, w.nfpart, w.nfd);
        if (pass & 2)
          klaunch(-1, mc_bytes2(nf, n), k_mc_bwd<Loc>, nb, dim3(BS), M, L, cgrid, (int64_t)row0, (int64_t)n, vx, vy, dt,
                  c0, (const double*)ch0, out0, (int32_t)nch, cin, (const double*)chn, cout, N, (const int4*)w.rec,
                  w.marks, w.tri, w.cnt);
      } else if (pass & 1) {
        klaunch(-1, dye_launch_bytes(nch, n), k_sl_multi<Loc>, nb, dim3(BS), M, L, cgrid, (int64_t)row0, (int64_t)n, vx,
                vy, dt, (int32_t)nch, cin, cout, N, w.marks, w.nfpart);
      }
    });
    KCHK();
  }
  // interleaved pairs: out = transport(f; u, dt); f, out and (two-pass) w.ch are three buffers
  void transport_pairs(TransportMode m, i64 row0, i64 n, const double* u2, double dt, const double* f2, double* out2,
                       const TransportWork& w, int pass = 3) {
    const MeshDev M{mx, my, mtri, mesh.T};
    const dim3 nb(nb_dye(n));
    const dbl2* u = reinterpret_cast<const dbl2*>(u2);
    const dbl2* f = reinterpret_cast<const dbl2*>(f2);
    dbl2* ch = reinterpret_cast<dbl2*>(w.ch);
    dbl2* out = reinterpret_cast<dbl2*>(out2);
    const double hdt = 0.5 * dt;
    with_loc([&](const auto& L) {
      using Loc = std::decay_t<decltype(L)>;
      if (m.mid()) {
        if ((pass & 1) && m.mc())
          klaunch(-1, trjv_bytes1(n, true), k_trj_fwd_vel<Loc>, nb, dim3(BS), M, L, cgrid, (int64_t)row0, (int64_t)n, u,
                  dt, hdt, f, ch, w.rec, w.marks, w.nfpart, w.mid);
        else if (pass & 1)
          klaunch(-1, trjv_bytes1(n, false), k_trj_fwd_vel<Loc>, nb, dim3(BS), M, L, cgrid, (int64_t)row0, (int64_t)n,
                  u, dt, hdt, f, out, (int4*)nullptr, w.marks, w.nfpart, w.mid);
        if ((pass & 2) && m.mc())
          klaunch(-1, trjv_bytes2(n), k_trj_bwd_vel<Loc>, nb, dim3(BS), M, L, cgrid, (int64_t)row0, (int64_t)n, u, dt,
                  hdt, f, (const dbl2*)ch, out, (const int4*)w.rec, w.marks, w.tri, w.cnt, w.mid + SLB);
      } else if (m.mc()) {
        if (pass & 1)
          klaunch(-1, mcv_bytes1(n), k_mc_fwd_vel<Loc>, nb, dim3(BS), M, L, cgrid, (int64_t)row0, (int64_t)n, u, dt, f,
                  ch, w.rec, w.nfpart);
        if (pass & 2)
          klaunch(-1, mcv_bytes2(n), k_mc_bwd_vel<Loc>, nb, dim3(BS), M, L, cgrid, (int64_t)row0, (int64_t)n, u, dt, f,
                  (const dbl2*)ch, out, (const int4*)w.rec, w.marks, w.tri, w.cnt);
      } else if (pass & 1) {
        klaunch(-1, vel_launch_bytes(n), k_sl_vel<Loc>, nb, dim3(BS), M, L, cgrid, (int64_t)row0, (int64_t)n, u, dt, f,
                out, w.marks, w.nfpart);
      }
    });
    KCHK();
  }
  // the dye's part of a step, on the stream of the step's tail, with the step's final u: c_full -> cnew and the
  // channels dye_cur -> dye_nxt (swapped here: a launch cannot write a set that other rows still gather from).
  // (SL, Euler): sl_launch with the fused reduction rs, then the channels' launch; every other mode moves c and the
  // channels together and leaves k_wsum's mixing sums of cnew in part_sl, as the implicit dye forms them
  void dye_transport_step(double* cnew, const RedOut& rs) {
    const i64 n = lp.n_own;
    const TransportMode m{adv_dye, trj_dye};
    const int nb = nb_dye(n);
    const bool fused = m.mc() || m.mid();
    TransportWork w;
    w.nfpart = dye_nfpart;
    if (fused) {
      if (!ndye) w.nfpart = m.mid() ? trjd_nfpart : mc_nfpart;
      w.nfd = m.mid() ? trjd_nfd : mc_nfd;
      if (m.mc()) w.ch = mc_ch, w.rec = mc_rec, w.cnt = mc_cnt;
      if (m.mid()) w.mid = trjd_mid;
      transport_fields(m, lp.r0, n, ux, prm.dt, c_full, cnew, ndye, dye_cur, dye_nxt, w);
      if (m.mc()) mc_nb = nb, ++mc_steps;
      if (m.mid()) trjd_nb = nb, ++trjd_steps;
    } else {
      sl_launch(nb_sl(n), lp.r0, n, ux, uy, prm.dt, c_full, cnew, dwmix, nullptr, rs);
      KCHK();
      if (ndye) transport_fields(m, lp.r0, n, ux, prm.dt, nullptr, nullptr, ndye, dye_cur, dye_nxt, w);
    }
    if (ndye) {
      std::swap(dye_cur, dye_nxt);
      dye_nb = nb;
      ++dye_steps;
    }
    if (fused) {
      hipLaunchKernelGGL(k_wsum, dim3(nb), dim3(BS), 0, st, lp.r0, n, (const double*)cnew, (const double*)dwmix,
                         part_sl);
      KCHK();
    }
  }
  // ... and its sums into the step record: sum wc, sum w and the not-found rows (the final locate's; pass 1's under
  // MacCormack).  (SL, Euler): k_sl's three partials, unless rs reduced them in the launch (done: red_done follows)
  void dye_transport_reduce(const RedOut& rs, bool done) {
    const TransportMode m{adv_dye, trj_dye};
    if (m.mc() || m.mid()) {
      reduce_into(part_sl, nb_dye(lp.n_own), 2, false, 2, SLB);
      reduce_into(m.mid() ? trjd_nfd : mc_nfd, nb_dye(lp.n_own), 1, false, 4, SLB);
    } else if (!rs.out) {
      reduce_into(part_sl, nb_sl(lp.n_own), 3, false, 2, SLB);
    } else if (done) {
      red_done(vals + 2, 3, false);
    }
  }
  // the rows of the last launch whose midpoint was not found (pass 1's and, with pass2, pass 2's), in block order
  int64_t trj_mid_rows(const int32_t* mid, int nb, bool pass2) {
    return nf_rows(mid, nb) + (pass2 ? nf_rows(mid + SLB, nb) : 0);
  }
  void drop_trajectory() {
    trj_dye = trj_vel = trj_trc = PUCFEM_TRJ_EULER;
    trjd_nb = trjv_nb = 0;
    trjt_ran = false;
    trjd_steps = trjv_steps = trjt_steps = 0;
    if (!trjd_mid && !trjv_mid && !trjt_fell) return;
    if (st) (void)hipStreamSynchronize(st);
    if (st_sl) (void)hipStreamSynchronize(st_sl);
    for (void* q : {(void*)trjd_mid, (void*)trjd_nfpart, (void*)trjd_nfd, (void*)trjv_mid, (void*)trjt_fell})
      if (q) (void)hipFree(q);
    trjd_mid = trjd_nfpart = trjv_mid = trjt_fell = nullptr;
    trjd_nfd = nullptr;
  }
  void set_trajectory(int what, int order) {
    constexpr int all = PUCFEM_TRJ_DYE | PUCFEM_TRJ_VELOCITY | PUCFEM_TRJ_TRACERS;
    if (what & ~all || what == 0)
      throw Error(PUCFEM_EINVAL, "what is a mask of PUCFEM_TRJ_DYE, PUCFEM_TRJ_VELOCITY and PUCFEM_TRJ_TRACERS");
    if (order != PUCFEM_TRJ_EULER && order != PUCFEM_TRJ_MIDPOINT)
      throw Error(PUCFEM_EINVAL, "unknown trajectory order");
    if (what & PUCFEM_TRJ_DYE) dye_ready();
    if (what & PUCFEM_TRJ_VELOCITY) inertia_ready();
    if (what & PUCFEM_TRJ_TRACERS) tracers_ready();
    if (ens)
      throw Error(PUCFEM_ESTATE,
                  "the trajectory order cannot be set while the context has an ensemble (members carry their own: "
                  "pucfem_ens_set_trajectory)");
    const bool mid = order == PUCFEM_TRJ_MIDPOINT;
    if ((what & PUCFEM_TRJ_DYE) && order != trj_dye) {
      if (st_sl) HIPCHK(hipStreamSynchronize(st_sl));
      if (mid) {
        if (!trjd_mid) {
          mc_alloc(trjd_mid, 2 * (size_t)SLB);
          mc_alloc(trjd_nfpart, (size_t)SLB);
          mc_alloc(trjd_nfd, (size_t)SLB);
          HIPCHK(hipStreamSynchronize(st));
        }
        trjd_steps = 0;
        trjd_nb = 0;
      }
      trj_dye = order;
    }
    if ((what & PUCFEM_TRJ_VELOCITY) && order != trj_vel) {
      if (mid) {
        if (!trjv_mid) {
          mc_alloc(trjv_mid, 2 * (size_t)SLB);
          HIPCHK(hipStreamSynchronize(st));
        }
        trjv_steps = 0;
        trjv_nb = 0;
      }
      trj_vel = order;
      have_vinc = 0;  // (as set_advection: the advected right-hand side changes)
    }
    if ((what & PUCFEM_TRJ_TRACERS) && order != trj_trc) {
      if (mid) {
        if (!trjt_fell) {
          mc_alloc(trjt_fell, (size_t)1);
          HIPCHK(hipStreamSynchronize(st));
        }
        trjt_steps = 0;
        trjt_ran = false;
      }
      trj_trc = order;
    }
    // (a small-mesh context steps uncaptured while a part is on; its captured graphs hold the Euler step and are
    // kept: with every part off again pucfem_step replays them)
  }
  size_t trajectory_dev_bytes() const {
    size_t b = 0;
    if (trjd_mid) b += sizeof(int32_t) * 3 * SLB + sizeof(double) * SLB;
    if (trjv_mid) b += sizeof(int32_t) * 2 * SLB;
    if (trjt_fell) b += sizeof(int32_t);
    return b;
  }


  // ------------------------------------------------------------------ fused reductions
  // The step's partial-producing kernels reduce their own partials (RedOut: the last block to finish
  // sums them, pucfem_kernels.hpp) instead of a k_reduce launch after them.  One ticket counter per
  // launch site (a site's launches are ordered on its stream; the dye stream's sites have their own).
  // Off by default (PUCFEM_FUSED_RED=1 turns it on, a measurement knob): at L7 the fused path ran 101.4
  // steps/s against 107.2 with k_reduce (r8a/r8b, same box type): under streaming load each block's
  // write-through partial store and returned ticket (two memory round trips in the block's tail) cost
  // 10-25 us per producer launch, more than the 9-14 us k_reduce launch they remove.
  enum { CNT_VCHEB, CNT_INIT, CNT_RZ, CNT_DIR, CNT_UPD, CNT_DIV, CNT_MDOT, CNT_MIX, CNT_SL, CNT_TRACER,
         CNT_DYE_DIV = 16, CNT_DYE_SL, CNT_DYE_MIX, CNT_FLOW, CNT_N = 32 };
  unsigned* dcnt = nullptr;
  bool fused_red = std::getenv("PUCFEM_FUSED_RED") && std::atoi(std::getenv("PUCFEM_FUSED_RED")) != 0;
  RedOut ro(double* out, int cnt, int nv, int stride = MAXB, unsigned maxmask = 0u, double* out1 = nullptr) const {
    if (!fused_red || !dcnt) return RedOut{};
    return RedOut{out, out1, dcnt + cnt, nv, stride, maxmask};
  }
  // after a fused reduction into out[0..nv): the all-reduce across ranks
  void red_done(double* out, int nv, bool is_max) {
    if (dist()) comm->allreduce(out, nv, is_max, st);
  }
  RedOut ro_rz{};  // the finest level's last smoothing step (<r, z>), set by pcg_mg around precondition()

  // ------------------------------------------------------------------ communication
  // partials of a producer kernel -> nv final values in redbuf slot `slot` (one 1-block kernel, then
  // the all-reduce across ranks): consumers read one scalar instead of re-reducing up to MAXB
  // partials in each of their blocks
  // the dye stream's reductions run in 256-thread blocks: a 1,024-thread block needs 16 free wave slots on
  // one CU, which the main stream's kernels rarely leave (the k_sl sums waited ~270 us for a CU, r10a)
  bool red_small = false;
  void launch_reduce(const double* part, int nb, int stride, int nv, bool is_max, double* out) {
    // one block per value (k_reduce_t)
    if (red_small)
      hipLaunchKernelGGL(k_reduce_t<256>, dim3(std::max(1, nv)), dim3(256), 0, st, part, nb, stride, nv,
                         is_max ? 1 : 0, out);
    else
      hipLaunchKernelGGL(k_reduce, dim3(std::max(1, nv)), dim3(RB), 0, st, part, nb, stride, nv, is_max ? 1 : 0, out);
  }
  Red reduce_global(double* part, int nb, int nv, bool is_max, int slot) {
    double* buf = redbuf + 8 * slot;
    launch_reduce(part, nb, MAXB, nv, is_max, buf);
    KCHK();
    if (dist()) comm->allreduce(buf, nv, is_max, st);
    return Red{buf, 1, 1};
  }
  // reduce partials into vals[slot..slot+nv) (+ all-reduce)
  void reduce_into(double* part, int nb, int nv, bool is_max, int slot, int stride = MAXB) {
    launch_reduce(part, nb, stride, nv, is_max, vals + slot);
    KCHK();
    if (dist())
      comm->allreduce(vals + slot, nv, is_max, st);
  }
  // refresh the ghost entries of up to two local vectors
  void halo(double* a, double* b = nullptr) { halo_lp(lp, dsend, dsendbuf, nsend, a, b); }
  template <typename T>
  void halo_lp(const LocalPlan& P, const int32_t* sidx, T* sbuf, i64 ns, T* a, T* b = nullptr) {
    if (!dist() || (P.send_peer.empty() && P.recv_peer.empty())) return;
    if (ns > 0) {
      hipLaunchKernelGGL(k_pack<T>, dim3(grid_ew(ns)), dim3(BS), 0, st, ns, sidx, a, b, sbuf);
      KCHK();
    }
    comm->group_start();
    for (size_t k = 0; k < P.send_peer.size(); ++k) {
      comm->send(sbuf + P.send_off[k], P.send_cnt[k], P.send_peer[k], st);
      if (b) comm->send(sbuf + ns + P.send_off[k], P.send_cnt[k], P.send_peer[k], st);
    }
    for (size_t k = 0; k < P.recv_peer.size(); ++k) {
      comm->recv(a + P.n_own + P.recv_off[k], P.recv_cnt[k], P.recv_peer[k], st);
      if (b) comm->recv(b + P.n_own + P.recv_off[k], P.recv_cnt[k], P.recv_peer[k], st);
    }
    comm->group_end(st);
  }
  template <typename T>
  void mg_halo(MgLevel& L, T* a, T* b = nullptr) {  // (two vectors: one grouped exchange; sendbuf holds 2 nsend)
    if (&L == &mg.back()) halo_lp(lp, dsend, bufs<T>(L).sendbuf, nsend, a, b);
    else halo_lp(L.lp, L.dsend, bufs<T>(L).sendbuf, L.nsend, a, b);
  }
  // Before the semi-Lagrangian step on W > 1 ranks: refresh the dye replica where this step's
  // back-traced points can reach -- the strips within dt max|u_y| + (largest triangle height) of each
  // rank's own y extent -- with point-to-point copies of contiguous internal-id ranges (every rank's
  // own segment is current: its SL wrote it).  Replaces the all-gather of the whole field (SURVEY.md
  // §8e: the departure distance bounds the gather).
  // The wide halo in two halves.  dye_range_start: every rank's range of back-traced y (StokesColor.py:361-372),
  // all-gathered as a max-reduction of a 2 W vector holding (1 - min, max) in each rank's slot, copied to pinned
  // host memory behind an event.  dye_halo_exchange: once that copy has landed, the point-to-point copies of the
  // strip ranges each rank reads.  The step (stokes_step) queues the first half at its end and the second half at
  // the next step, after that step's viscous solve, whose host round trip has seen the copy land -- no blocking
  // read of its own (round 5 synchronised the stream here every step).
  double* h_yr_pin = nullptr;  // 2 W (pinned)
  hipEvent_t ev_yr = nullptr;
  void dye_range_start(const double* vy, double dt) {
    const i64 n = lp.n_own;
    const int nb = nb_rows(n);
    if (!h_yr_pin) {
      HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&h_yr_pin), sizeof(double) * 2 * world));
      HIPCHK(hipEventCreateWithFlags(&ev_yr, hipEventDisableTiming));
    }
    hipLaunchKernelGGL(k_yrange, dim3(nb), dim3(BS), 0, st, n, my + lp.r0, vy, dt, part_u);
    KCHK();
    hipLaunchKernelGGL(k_reduce, dim3(2), dim3(RB), 0, st, part_u, nb, MAXB, 2, 1, yr_own);
    hipLaunchKernelGGL(k_place2, dim3(1), dim3(64), 0, st, world, rank, (const double*)yr_own, yr_all);
    KCHK();
    comm->allreduce(yr_all, 2 * (size_t)world, true, st);
    HIPCHK(hipMemcpyAsync(h_yr_pin, yr_all, sizeof(double) * 2 * world, hipMemcpyDeviceToHost, st));
    HIPCHK(hipEventRecord(ev_yr, st));
  }
  void dye_halo_exchange() {
    wait_event(ev_yr);  // (at the step's use: long complete, a query)
    std::copy(h_yr_pin, h_yr_pin + 2 * world, h_yr.begin());
    const i64 S = (i64)strip_ylo.size();
    auto need = [&](int j, i64& a, i64& b) {  // internal-id range rank j reads: the strips that meet
      // its back-traced y range widened by a triangle height (the located triangle's vertices)
      const double lo = (1.0 - h_yr[2 * j]) - tri_hy - 1e-9, hi = h_yr[2 * j + 1] + tri_hy + 1e-9;
      i64 sa = 0, sb = S;
      while (sa < S && strip_yhi[sa] < lo) ++sa;
      while (sb > sa && strip_ylo[sb - 1] > hi) --sb;
      a = ord.strip_ptr[sa];
      b = ord.strip_ptr[sb];
    };
    const i64 o0 = row_start[rank], o1 = row_start[rank + 1];
    dye_halo_values = 0;
    comm->group_start();
    for (int j = 0; j < world; ++j) {
      if (j == rank) continue;
      i64 a, b;
      need(j, a, b);
      a = std::max(a, o0);
      b = std::min(b, o1);
      if (b > a) comm->send(c_full + a, (size_t)(b - a), j, st);
    }
    i64 a0, b0;
    need(rank, a0, b0);
    for (int j = 0; j < world; ++j) {
      if (j == rank) continue;
      const i64 a = std::max(a0, row_start[j]), b = std::min(b0, row_start[j + 1]);
      if (b > a) {
        comm->recv(c_full + a, (size_t)(b - a), j, st);
        dye_halo_values += b - a;
      }
    }
    comm->group_end(st);
  }
  // full replica <- every rank's owned segment (internal numbering is rank-contiguous)
  void allgather_full(double* full) {
    if (!dist()) return;
    comm->group_start();
    for (int r = 0; r < world; ++r) {
      const i64 o = row_start[r], n = row_start[r + 1] - row_start[r];
      comm->bcast(full + o, n, r, st);
    }
    comm->group_end(st);
  }

  // ------------------------------------------------------------------ CG
  template <int NR>
  int cg(const DevSell& A, const HFace& hf, const double* val, double* const y[NR], const double* const b[NR],
         double tol, int maxit, int which) {
    if (!dist() && block_cg && !hf.items && A.nrows <= (int64_t)CGB_THREADS * CGB_MAXR) {
      const size_t vec = (size_t)NR * A.nrows * sizeof(double);
      const size_t mat = (size_t)A.padded * (sizeof(double) + sizeof(int32_t));
      const bool mat_lds = vec + mat <= (size_t)150 * 1024;
      const size_t lds = vec + (mat_lds ? mat : 0);
      // the attribute is per device and function: set it once per context (a context is bound to one
      // device; a second context on the same device sets it again, which is harmless)
      if (!lds_attr[NR]) {
        HIPCHK(hipFuncSetAttribute((const void*)k_cg_block<NR>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   150 * 1024));
        lds_attr[NR] = true;
      }
      int* slot = dits ? dits + 3 * cur_step + which : nullptr;
      hipLaunchKernelGGL((k_cg_block<NR>), dim3(1), dim3(CGB_THREADS), lds, st, A.view(), val, y[0],
                         NR > 1 ? y[1] : (double*)nullptr, b[0], NR > 1 ? b[1] : (const double*)nullptr, tol * tol,
                         maxit, mat_lds ? 1 : 0, ctl, slot);
      KCHK();
      if (dits) return -1;  // collected after the step loop
      HIPCHK(hipMemcpyAsync(h_ctl, ctl, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      if (h_ctl[0] == 3) throw Error(PUCFEM_ENOCONV, "CG residual is not finite");
      if (h_ctl[0] != 1) throw Error(PUCFEM_ENOCONV, "CG did not converge within maxit=" + std::to_string(maxit));
      return h_ctl[1];
    }
    // multi-kernel Jacobi-scaled CG with the direction updated in place (k_cgr_*): an iteration is
    // the SpMV with its three dots, the update (y, r, p) with the exact <r, r>, and the control test
    const FaceDev fc = hf.part();
    const int nb = grid_part(fc, A);
    CgVecs<NR> v;
    for (int c = 0; c < NR; ++c) {
      v.y[c] = y[c];
      v.b[c] = b[c];
      v.r[c] = cg_r[c];
      v.po[c] = cg_pa[c];  // the direction p
      v.pn[c] = cg_pb[c];
      v.q[c] = cg_q[c];
    }
    auto halo_p = [&]() {
      if (NR == 2) halo(cg_pa[0], cg_pa[1]);
      else halo(cg_pa[0]);
    };
    if (NR == 2) halo(y[0], y[1]);
    else halo(y[0]);
    HIPCHK(hipMemsetAsync(ctl, 0, 2 * sizeof(int), st));
    algo_bytes += (8.0 + A.idx_bytes()) * (double)A.nnz + A.row_bytes() * (double)A.nrows + 32.0 * NR * (double)A.own();
    with_c16(A, [&](auto c16) {
      hipLaunchKernelGGL((k_cg_init<NR, decltype(c16)::value>), dim3(nb), dim3(BS), 0, st, A.view(), fc, val, v,
                         lp.n_ghost, part_a, part_b, (float*)nullptr, 1, RedOut{});
    });
    KCHK();
    Red rr = reduce_global(part_a, nb, NR, false, 0);
    Red bb = reduce_global(part_b, nb, NR, false, 1);
    const double tol2 = tol * tol;
    hipLaunchKernelGGL(k_cgr_ctl, dim3(1), dim3(64), 0, st, rr.p, bb.p, tol2, ctl, 0, maxit, NR);
    KCHK();
    halo_p();
    // algorithmic bytes: dir gathers p once per row and reads r, writes q; upd reads y, p, r, q and
    // writes y, r, p
    const double bytes_dir =
        (8.0 + A.idx_bytes()) * (double)A.nnz + A.row_bytes() * (double)A.nrows + 24.0 * NR * (double)A.own();
    const double bytes_upd = 56.0 * NR * (double)A.own();
    int it = 0;
    // host convergence checks: the first after as many iterations as the last solve took (the control
    // test after each update lets the check see convergence without a further launch)
    int chunk = std::max(1, std::min(maxit + 1, last_it[which] > 0 ? last_it[which] : 4));
    std::vector<ByteMark> bmark;  // the byte counters at the start of each iteration of the current chunk
    for (;;) {
      const int it0 = it;
      bmark.clear();
      for (int k = 0; k < chunk; ++k, ++it) {
        bmark.push_back(bmark_now());
        // HIP-event timing samples every 8th iteration (bounded event count for long solves)
        const bool samp = (it & 7) == 0;
        with_c16(A, [&](auto c16) {
          klaunch(samp ? 1 : -1, bytes_dir, k_cgr_dir<NR, decltype(c16)::value>, dim3(nb), dim3(BS), A.view(), fc,
                  val, v, (const int*)ctl, part_c);
        });
        KCHK();
        Red dots = reduce_global(part_c, nb, 3 * NR, false, 2);
        klaunch(samp ? 2 : -1, bytes_upd, k_cgr_upd<NR>, dim3(nb_rows(A.own())), dim3(BS), v, A.own(),
                (const double*)dots.p, (const double*)rr.p, (const int*)ctl, part_a);
        KCHK();
        rr = reduce_global(part_a, nb_rows(A.own()), NR, false, 0);
        hipLaunchKernelGGL(k_cgr_ctl, dim3(1), dim3(64), 0, st, rr.p, bb.p, tol2, ctl, it + 1, maxit, NR);
        KCHK();
        halo_p();
      }
      HIPCHK(hipMemcpyAsync(h_ctl, ctl, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      if (timer.on) timer.flush();
      // iterations from the converged one on were launched but did no work
      if (h_ctl[0] && h_ctl[1] >= it0 && h_ctl[1] < it) bmark_restore(bmark[h_ctl[1] - it0]);
      if (h_ctl[0]) break;
      chunk = std::max(1, std::min(64, it / 8));
    }
    last_it[which] = h_ctl[1];
    if (h_ctl[0] == 3) throw Error(PUCFEM_ENOCONV, "CG residual is not finite (iteration " + std::to_string(h_ctl[1]) + ")");
    if (h_ctl[0] != 1)
      throw Error(PUCFEM_ENOCONV, "CG did not converge within maxit=" + std::to_string(maxit));
    return h_ctl[1];
  }

  // Chebyshev iteration for the Jacobi-scaled viscous system (k_vcheb), both components at once in the
  // interleaved (dbl2) vectors: y (warm start, overwritten only through the buffers) and b; the converged
  // iterate is returned in *out (y itself or one of the x buffers).  Target: the CG's test
  // <r, r> <= tol^2 <b, b> per component, met through the a-priori residual bound of the interval (below).
  // fin (optional): the viscous finish (k_visc_fin: u* = S y, the fp32 increment u* - u) for the solve's
  // last step to do in place of its x_out; *fin_done tells whether it did
  struct ViscFin {
    const double* s;
    const double* u[2];
    double* us[2];
    float* inc[2];
  };
  // the interleaved vectors of the viscous Chebyshev solve (allocated with the operators): the start / x
  // buffers, b, and the fp32 increments d (a step pair writes its d to the second buffer)
  dbl2 *vx2[3] = {nullptr, nullptr, nullptr}, *vb2 = nullptr;
  flt2* vd2[2] = {nullptr, nullptr};
  // halo of an interleaved vector (both components of each ghost row)
  void halo2(dbl2* a, dbl2* b = nullptr) {  // (b: a second interleaved vector in the same grouped exchange)
    const LocalPlan& P = lp;
    if (!dist() || (P.send_peer.empty() && P.recv_peer.empty())) return;
    if (nsend > 0) {
      hipLaunchKernelGGL(k_pack<dbl2>, dim3(grid_ew(nsend)), dim3(BS), 0, st, nsend, dsend, (const dbl2*)a,
                         (const dbl2*)b, reinterpret_cast<dbl2*>(dsendbuf));
      KCHK();
    }
    comm->group_start();
    for (size_t k = 0; k < P.send_peer.size(); ++k) {
      comm->send(dsendbuf + 2 * P.send_off[k], 2 * P.send_cnt[k], P.send_peer[k], st);
      if (b) comm->send(dsendbuf + 2 * (nsend + P.send_off[k]), 2 * P.send_cnt[k], P.send_peer[k], st);
    }
    for (size_t k = 0; k < P.recv_peer.size(); ++k) {
      comm->recv(reinterpret_cast<double*>(a + P.n_own + P.recv_off[k]), 2 * P.recv_cnt[k], P.recv_peer[k], st);
      if (b) comm->recv(reinterpret_cast<double*>(b + P.n_own + P.recv_off[k]), 2 * P.recv_cnt[k], P.recv_peer[k], st);
    }
    comm->group_end(st);
  }
  int vcheb(const DevSell& A, const HFace& hf, const double* val, dbl2* y, const dbl2* b, double tol, int maxit,
            int which, dbl2** out, const ViscFin* vfin = nullptr, bool* fin_done = nullptr) {
    constexpr int NR = 2;
    if (fin_done) *fin_done = false;
    const FaceDev fc = hf.part();
    const int nb = grid_part(fc, A);
    // step pairs (k_vcheb_pair): a face part of lattice size <= VP_HALO.  On W > 1 ranks only the solve's first pair
    // (0, 1), whose first step also runs on the ghost rows one layer out (deep halos: x and b exchanged two layers
    // out together, one exchange for the two steps); later pairs would need d exchanged too, so single steps
    const bool deepv = dist() && A.has_ghost_rows() && use_mg && mg.back().deep && (deep_mask & 16);
    const DevSell Ag = A.with_ghosts();  // (= A without ghost rows)
    const int nbs = nb_for(Ag.nslices);  // a pair's SELL grids (its first launch covers the ghost rows)
    const bool pairs_ok = visc_pair && hf.items > 0 && fc.n <= VP_HALO &&
                          nbs + hf.items <= MAXB;  // (the check's partials of both halves)
    const bool pairs = pairs_ok && !dist();
    dbl2* xa = y;
    dbl2* xb = vx2[1];
    dbl2* xc = vx2[2];  // step pairs: x_{a+2}
    flt2* dcur = vd2[0];  // the fp32 increments d (in place for single steps)
    flt2* dalt = vd2[1];  // step pairs: d_{a+2}
    HIPCHK(hipMemsetAsync(ctl, 0, 2 * sizeof(int), st));
    const bool pair0 = (pairs || (pairs_ok && deepv)) && !ro(redbuf, CNT_VCHEB, 2 * NR).out;
    if (pair0 && deepv) halo2(xa, const_cast<dbl2*>(b));  // (b's ghosts: the first step on the ghost rows)
    else halo2(xa);
    // the interval [visc_lo, 1 + visc_R]: theta its centre, delta its half-width
    const double hi = 1.0 + visc_R, lo = visc_lo;
    const double theta = 0.5 * (hi + lo), delta = 0.5 * (hi - lo), sigma = theta / delta, tol2 = tol * tol;
    // algorithmic bytes: x gathered once, b, d (fp32; not at the first step) read, d and x_out written
    const double bytes = (8.0 + A.idx_bytes()) * (double)A.nnz + A.row_bytes() * (double)A.nrows +
                         32.0 * NR * (double)A.own();
    // One step: x_out = x_in + d, d = c1 d + c2 (b - A^ x_in); the first step also yields |r_0| and |b|.
    auto step = [&](int it, double c1, double c2, bool check = false, bool fin = false) {
      ChebVecs2 v{};
      v.xin = xa;
      v.xout = xb;
      v.b = b;
      v.d = dcur;
      if (fin) {
        v.s = vfin->s;
        for (int c = 0; c < NR; ++c) {
          v.u[c] = vfin->u[c];
          v.us[c] = vfin->us[c];
          v.inc[c] = vfin->inc[c];
        }
      }
      // timing class 9; the first step reads no d (4 B/row per right-hand side less)
      // step 0 reduces its own partials (fused): |r_0|^2 into redbuf[0 .. NR), |b|^2 into redbuf[NR .. 2 NR)
      const RedOut r0 = it == 0 ? ro(redbuf, CNT_VCHEB, 2 * NR) : RedOut{};
      double* pb = it == 0 ? (r0.out ? part_a + NR * MAXB : part_b) : (double*)nullptr;
      // check: the post-check's |r_it|^2 partials (part_c)
      double* pr = it == 0 ? part_a : (check ? part_c : (double*)nullptr);
      with_c16(A, [&](auto c16) {
        // fin: + s, u read and u*, the increment written - d, x_out
        klaunch(9, (it == 0 ? bytes - 4.0 * NR * (double)A.own() : bytes) + (fin ? 12.0 * NR * (double)A.own() : 0.0),
                k_vcheb<decltype(c16)::value>, dim3(nb),
                dim3(BS), A.view(), fc, val, v, c1, c2, it == 0 ? 1 : 0, (const int*)ctl, pr, pb, r0);
      });
      KCHK();
      if (fin) return;  // the solve's output is u* (haloed by viscous()), x_out was not written
      halo2(xb);
      std::swap(xa, xb);
    };
    // Two steps a, a + 1 in three launches: the skeleton rows' step a (k_vcheb on the SELL part alone),
    // both steps on the face interiors (k_vcheb_pair: x_{a+1} in LDS), the skeleton rows' step a + 1.
    // check: the |r_{a+1}|^2 partials of both halves in part_c (SELL blocks first); fin: step a + 1 is
    // the solve's last and writes u* and the increment.
    const double bytes_sk = (8.0 + A.idx_bytes()) * (double)A.nnz + A.row_bytes() * (double)A.nrows +
                            32.0 * NR * (double)(A.own() - hf.rows);
    // first: the pair is the solve's steps 0 and 1: step 0 reads no d and both halves write the |r_0|^2 /
    // |b|^2 partials (part_a / part_b: the SELL blocks at their block indices, the face items after them)
    auto pair_step = [&](double c1a, double c2a, double c1b, double c2b, bool check, bool fin, bool first = false) {
      FaceDev fs = fc;
      fs.nb = 0;
      ChebVecs2 v1{}, v2{};
      VPairVecs p{};
      v1.xin = xa;
      v1.xout = xb;
      v1.b = b;
      v1.d = dcur;
      v2.xin = xb;
      v2.xout = xc;
      v2.b = b;
      v2.d = dcur;
      v2.dout = dalt;
      p.xa = xa;
      p.xb = xb;
      p.xc = xc;
      p.b = b;
      p.da = dcur;
      p.dc = dalt;
      if (fin) {
        v2.s = p.s = vfin->s;
        for (int c = 0; c < NR; ++c) {
          v2.u[c] = p.u[c] = vfin->u[c];
          v2.us[c] = p.us[c] = vfin->us[c];
          v2.inc[c] = p.inc[c] = vfin->inc[c];
        }
      }
      // face rows: x_a, b, d_a read, x_{a+2}, d_{a+2} written (fin: + s, u read, u*, the increment
      // written - x, d), x_{a+1} written at the rows next to the skeleton (3 (n - 3) per face)
      const double bnd_rows = fc.n > 3 ? 3.0 * (fc.n - 3) * (double)fc.nf : 0.0;
      const double bytes_f = (32.0 * NR + (fin ? 12.0 * NR : 0.0)) * (double)hf.rows + 8.0 * NR * bnd_rows;
      const double fin_sk = fin ? 12.0 * NR * (double)(A.own() - hf.rows) : 0.0;
      double* pc = check ? part_c : nullptr;
      with_c16(A, [&](auto c16) {
        klaunch(-1, bytes_sk - (first ? 4.0 * NR * (double)(A.own() - hf.rows) : 0.0), k_vcheb<decltype(c16)::value>,
                dim3(nbs), dim3(BS), Ag.view(), fs, val, v1, c1a, c2a, first ? 1 : 0, (const int*)ctl,
                first ? part_a : (double*)nullptr, first ? part_b : (double*)nullptr, RedOut{});
        KCHK();
        klaunch(12, bytes_f - (first ? 4.0 * NR * (double)hf.rows : 0.0), k_vcheb_pair, dim3(hf.items), dim3(BS), fc, p,
                c1a, c2a, c1b, c2b, (const int*)ctl, pc, (int32_t)nbs, first ? 1 : 0,
                first ? part_a : (double*)nullptr, first ? part_b : (double*)nullptr);
        KCHK();
        klaunch(-1, bytes_sk + fin_sk, k_vcheb<decltype(c16)::value>, dim3(nbs), dim3(BS), A.view(), fs, val, v2,
                c1b, c2b, 0, (const int*)ctl, pc, (double*)nullptr, RedOut{});
        KCHK();
      });
      ++visc_pairs;
      if (fin) return;
      // x_{a+2} is current; x_a, x_{a+1} are free
      dbl2* t = xa;
      xa = xc;
      xc = xb;
      xb = t;
      std::swap(dcur, dalt);
      if (dist()) halo2(xa);  // (W > 1: the next single step gathers x_{a+2}'s ghosts)
    };
    // Step 0 gives r_0 = b - A^ x_0.  The residual polynomial of the Chebyshev iteration on an interval
    // holding the spectrum is bounded by 1 / T_k(sigma) there, so |r_k| <= |r_0| / T_k(sigma): the step
    // count K that meets the CG's test |r_K| <= rtol |b| is known after step 0, and steps 1 .. K-1 run with
    // no residual checks, no reductions and no host round trip.  (The bound is rigorous for the interval
    // [visc_lo, 1 + visc_R], which tests/test_host_assembly.py checks against the spectrum; the
    // adaptive test it replaces needed one extra step per solve to see the passing residual.)
    // With step pairs the solve starts with the pair (0, 1) -- one face pass where step 0 and a single step
    // 1 took two -- and the step count K decides the rest: K <= 2 is done (the finish runs as k_visc_fin),
    // K = 3 / 4 add a single step / a pair with the finish.  Without pairs: step 0 alone.
    double rho_old = 1.0 / sigma;
    int done = 1;
    int nb0 = nb;  // the first step's partial count
    if (pair0) {
      const double rho = 1.0 / (2.0 * sigma - rho_old);
      pair_step(0.0, 1.0 / theta, rho * rho_old, 2.0 * rho / delta, true, false, true);
      rho_old = rho;
      done = 2;
      nb0 = nbs + (int)hf.items;
    } else {
      step(0, 0.0, 1.0 / theta);
    }
    Red rr{redbuf, 1, 1}, bb{redbuf + NR, 1, 1};
    if (!pair0 && ro(redbuf, CNT_VCHEB, 2 * NR).out) {
      red_done(redbuf, 2 * NR, false);
    } else {
      rr = reduce_global(part_a, nb0, NR, false, 0);
      bb = reduce_global(part_b, nb0, NR, false, 1);
    }
    HIPCHK(hipMemcpyAsync(h_pinned, rr.p, NR * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(h_pinned + 8, bb.p, NR * sizeof(double), hipMemcpyDeviceToHost, st));
    hipEvent_t have_r0 = timer.get();
    HIPCHK(hipEventRecord(have_r0, st));
    // while the host waits for |r_0|, the GPU already runs the steps the last solve certainly needed
    // (one fewer than its count): the round trip hides behind them
    // (step pairs: two steps per pass while at least two are due)
    auto pair_coefs = [&](double& c1a, double& c2a, double& c1b, double& c2b) {
      const double ra = 1.0 / (2.0 * sigma - rho_old), rb = 1.0 / (2.0 * sigma - ra);
      c1a = ra * rho_old;
      c2a = 2.0 * ra / delta;
      c1b = rb * ra;
      c2b = 2.0 * rb / delta;
      rho_old = rb;
    };
    auto advance = [&](int upto) {
      while (done < upto) {
        if (pairs && upto - done >= 2) {
          double c1a, c2a, c1b, c2b;
          pair_coefs(c1a, c2a, c1b, c2b);
          pair_step(c1a, c2a, c1b, c2b, false, false);
          done += 2;
          continue;
        }
        const double rho = 1.0 / (2.0 * sigma - rho_old);
        step(done, rho * rho_old, 2.0 * rho / delta);
        rho_old = rho;
        ++done;
      }
    };
    // with step pairs only whole pairs go ahead of the round trip, and at least the last two steps
    // wait for it (so that they can run as one pair with the finish)
    advance(pair0 ? 2 + 2 * std::max(0, (last_it[which] - 4) / 2)
                  : (pairs ? 1 + 2 * std::max(0, (last_it[which] - 3) / 2) : std::max(1, last_it[which] - 1)));
    // the last solve took at most two steps (past the transient: always): the finish from x_2 (k_visc_fin, as
    // viscous() would launch it) goes ahead of the round trip, so the GPU works while the host waits; it stands
    // when the count is again at most two and is rewritten by the solve's real last step (or by viscous() from
    // x_0 when x_0 passes) otherwise
    const bool spec_fin = pair0 && vfin && done == 2 && last_it[which] <= 2 && fin_done;
    if (spec_fin) {
      const i64 n = A.own();
      algo_bytes += 64.0 * (double)n;  // s, x_2, u read; u*, the fp32 increment written
      hipLaunchKernelGGL(k_visc_fin, dim3(grid_ew(n)), dim3(BS), 0, st, (int64_t)n, vfin->s, (const dbl2*)xa,
                         vfin->u[0], vfin->u[1], vfin->us[0], vfin->us[1], vfin->inc[0], vfin->inc[1]);
      KCHK();
    }
    wait_event(have_r0);
    timer.pool.push_back(have_r0);
    if (vcc.pending) {  // the previous solve's post-check (its copy preceded step 0 on the stream)
      vcc.pending = false;
      for (int c = 0; c < vcc.nr; ++c)
        if (!(h_pinned[32 + c] <= vcc.bound2[c] * 1.0201 + vcc.floor2[c])) {
          ++visc_check_fail;
          visc_solver = 1;  // the interval does not hold the spectrum: CG from the next solve on
        }
    }
    int K = 1;  // x_1 exists now; x_0 (y) is the answer when r_0 already passes
    bool pass0 = true;
    for (int c = 0; c < NR; ++c) {
      const double r0 = h_pinned[c], bn = h_pinned[8 + c];
      if (!std::isfinite(r0) || !std::isfinite(bn)) throw Error(PUCFEM_ENOCONV, "Chebyshev residual is not finite");
      if (r0 <= tol2 * bn) continue;
      pass0 = false;
      // smallest k with T_k(sigma) >= |r_0| / (rtol |b|)
      const double need = std::sqrt(r0 / (tol2 * bn));
      double tm = 1.0, tk = sigma;
      int k = 1;
      while (tk < need && k < maxit) {
        const double tn = 2.0 * sigma * tk - tm;
        tm = tk;
        tk = tn;
        ++k;
      }
      if (tk < need) throw Error(PUCFEM_ENOCONV, "Chebyshev iteration would not converge within maxit=" + std::to_string(maxit));
      K = std::max(K, k);
    }
    if (pass0 && (done == 1 || (pair0 && done == 2))) {  // y itself passes (the first pair left it intact)
      *out = y;
      last_it[which] = 0;
      return 0;
    }
    // the a-posteriori check of the next solve: |r_kc|^2 (kc = K - 1, reduced from part_c) against
    // |r_0| / T_kc(sigma)
    auto post_check = [&](int kc, int nck) {
      hipLaunchKernelGGL(k_reduce, dim3(NR), dim3(RB), 0, st, (const double*)part_c, nck, MAXB, NR, 0, redbuf + 48);
      KCHK();
      if (dist()) comm->allreduce(redbuf + 48, NR, false, st);
      HIPCHK(hipMemcpyAsync(h_pinned + 32, redbuf + 48, NR * sizeof(double), hipMemcpyDeviceToHost, st));
      double tm = 1.0, tk = sigma;  // T_kc(sigma)
      for (int k = 1; k < kc; ++k) {
        const double tn = 2.0 * sigma * tk - tm;
        tm = tk;
        tk = tn;
      }
      vcc.pending = true;
      vcc.nr = NR;
      for (int c = 0; c < NR; ++c) {
        vcc.bound2[c] = h_pinned[c] / (tk * tk);
        vcc.floor2[c] = 1e-28 * h_pinned[8 + c];  // rounding: |r| ~ 1e-14 |b| is as far as it resolves
      }
    };
    if (pair0 && done >= K) {  // the first pair did it (x_2, or more steps already launched)
      if (K >= 2) post_check(1, nbs + (int)hf.items);  // |r_1|^2: the first pair's check partials
      if (spec_fin) *fin_done = true;  // (the finish from x_2 = xa ran: k_visc_fin's launch, its values)
      *out = xa;
      last_it[which] = std::max(K, 1);
      return done;
    }
    if (done < K) {
      // the last step also reduces |r_{K-1}|^2 (its input's residual) for the a-posteriori check; with
      // step pairs it is the second step of a pair when an even number of steps is left
      const bool fuse = vfin != nullptr;
      const bool last_pair = pairs && (K - done) % 2 == 0;
      advance(last_pair ? K - 2 : K - 1);
      int kc, nck;
      if (last_pair) {
        double c1a, c2a, c1b, c2b;
        pair_coefs(c1a, c2a, c1b, c2b);
        pair_step(c1a, c2a, c1b, c2b, true, fuse);
        kc = done + 1;
        done += 2;
        nck = nbs + (int)hf.items;
      } else {
        const double rho = 1.0 / (2.0 * sigma - rho_old);
        step(done, rho * rho_old, 2.0 * rho / delta, true, fuse);
        rho_old = rho;
        kc = done;
        ++done;
        nck = nb;
      }
      if (fuse) *fin_done = true;
      post_check(kc, nck);
    }
    advance(K);  // (steps beyond K, already launched, only reduce the residual further)
    *out = xa;  // x_done, done >= K
    last_it[which] = K;
    return done;
  }

  // ------------------------------------------------------------------ multigrid V-cycle / PCG
  // Polynomial smoothing (deg steps) for D^-1 A: Chebyshev on [lmax / mg_ratio, lmax] (mg_kind 1), or
  // the fourth-kind Chebyshev recurrence on [0, lmax] (mg_kind 4, Lottes 2022: d_0 = 4/(3 lmax) D^-1 r,
  // d_i = (2i-1)/(2i+3) d_(i-1) + (8i+4)/((2i+3) lmax) D^-1 r_i).  Both are d = c1 d + c2 D^-1 (b - A x),
  // x += d with step-dependent scalars.
  // x_in (nullable: zero initial guess) -> returns the buffer holding the result; with zout the
  // last step writes its result (in fp64) to zout instead and nullptr is returned.
  // launch grids of a lattice operator: its face blocks, then the SELL blocks (launches that write
  // partials stay within MAXB blocks)
  // The SELL blocks come first and their count is a multiple of 8, so the face blocks' hardware ids
  // keep their XCD (id % 8) for the XCD-aware item order of face_rows.
  static int sell_blocks(int nb, const FaceDev& f) {
    if (!f.nb) return nb;
    return std::min((nb + 7) & ~7, (MAXB - f.nb) & ~7);
  }
  static int grid_part(const FaceDev& f, const DevSell& A) { return f.nb + sell_blocks(nb_for(A.nslices), f); }
  int grid_full(const FaceDev& f, const DevSell& A) const {
    return f.nb + (f.nb ? (nb_mg(A.nslices) + 7) & ~7 : nb_mg(A.nslices));
  }

  template <typename T, typename TB>
  // toz: the last step writes the preconditioned residual (z32 in the fp32 cycle, z in the fp64 one)
  // last_g (deep halos): the last step also runs on the ghost rows one layer out (x and d exchanged before it)
  // xin_cur (deep halos): xin's ghosts (two layers) are current, the first step needs no exchange
  T* mg_smooth(MgLevel& L, const DevSell& A, const HFace& hf, MgBufs<T>& B, const TB* b, T* xin, T* xa, T* xb,
               bool tozr, const double* rdot, double* part, int deg, bool last_g = false, bool xin_cur = false) {
    const double lmax = L.lmax, lmin = lmax / prm.mg_ratio;
    const double theta = 0.5 * (lmax + lmin), delta = 0.5 * (lmax - lmin), sigma = theta / delta;
    double rho_old = 1.0 / sigma;
    T* cur = xin;
    deg = std::max(1, deg);
    const bool finest = &L == &mg.back();
    // the step coefficients: d = c1 d + c2 Dinv (b - A x)
    std::vector<double> c1s(deg), c2s(deg);
    for (int k = 0; k < deg; ++k) {
      double c1 = 0.0, c2 = 1.0 / theta;
      if (prm.mg_kind == 4) {
        c1 = k == 0 ? 0.0 : (2.0 * k - 1.0) / (2.0 * k + 3.0);
        c2 = k == 0 ? 4.0 / (3.0 * lmax) : (8.0 * k + 4.0) / ((2.0 * k + 3.0) * lmax);
      } else if (k > 0) {
        const double rho = 1.0 / (2.0 * sigma - rho_old);
        c1 = rho * rho_old;
        c2 = 2.0 * rho / delta;
        rho_old = rho;
      }
      c1s[k] = c1;
      c2s[k] = c2;
    }
    // step pairs (k_cheb_pair) on the finest level of the fp32 cycle, one rank: two steps per pass on the
    // face interiors; not the step that writes z / the <r, z> partials
    bool pairs = false;
    // deep halos (W > 1): a pair's first step also runs on the ghost rows one layer out, so a pair needs one
    // exchange (x, two layers) where two single steps needed two -- pairs on every partitioned level
    const bool dg = dist() && L.deep && (deep_mask & 1);
    if constexpr (std::is_same<T, float>::value && std::is_same<TB, float>::value)
      // (one rank: the finest level only; pairs on L6 / L5 too measured neutral to -0.7 %, r10m)
      pairs = mg_pair && hf.items > 0 && hf.d.n <= VP_HALO &&
              (dist() ? dg : &L == &mg.back());
    if (pairs && !mgp_x) {  // (sized for the finest level: every pair level uses them in turn)
      mgp_x = dalloc<float>(mg.back().nloc);
      mgp_d = dalloc<float>(mg.back().nloc);
    }
    T* dcur = B.d;  // the current d (a pair writes its d to the other buffer)
    double c20 = 0.0;
    for (int k = 0; k < deg; ++k) {
      const double c1 = c1s[k], c2 = c2s[k];
      // zero initial guess and >= 2 steps: step 0 is folded into step 1 (mode 2; b's ghosts are
      // current, see vcycle)
      const bool fuse = cur == nullptr && k == 0 && deg >= 2;
      if (fuse) {
        c20 = c2;
        continue;
      }
      const int mode = (cur == nullptr && k == 0) ? 0 : (cur == nullptr ? 2 : 1);
      if constexpr (std::is_same<T, float>::value && std::is_same<TB, float>::value) {
        const bool next_last = k + 1 == deg - 1;
        // (W > 1: a general-step pair only where d_a is not read, c1 = 0: d is not exchanged before it)
        if (pairs && mode != 0 && k + 1 < deg && !(next_last && (tozr || rdot || last_g)) &&
            (!dg || mode == 2 || c1 == 0.0)) {
          if (dg && mode == 1 && !(xin_cur && cur == xin)) mg_halo(L, cur);  // x_a two layers out: the first step
                                                                              // runs on the ghost rows
          // steps k, k + 1: x_a = cur (mode 1) -> x_{a+1} in p1 (skeleton rows, the face rows next to
          // them) -> x_{a+2} in p2; d_a = dcur -> d_{a+2} in the other d buffer
          float* p1 = mode == 2 ? xa : (cur == xa ? xb : xa);
          float* p2 = mode == 2 ? xb : mgp_x;
          if (mode == 1 && cur == mgp_x) {  // (cur is the extra buffer after an earlier pair)
            p1 = xa;
            p2 = xb;
          }
          float* dn = dcur == B.d ? mgp_d : B.d;
          FaceDev fs = hf.full();
          fs.nb = 0;
          const int nbs = nb_mg(A.nslices);
          const DevSell Ag = dg ? A.with_ghosts() : A;  // the first SELL launch: + the ghost rows one layer out
          const int nbg = nb_mg(Ag.nslices);
          // skeleton rows: the SELL part of a k_cheb step (bytes as in the single step, SELL rows only)
          const double sk_row = (mode == 1 ? 3.0 * sizeof(T) : 1.0 * sizeof(T)) + sizeof(TB) + 2.0 * sizeof(T);
          const double bytes_sk = (B.val_bytes() + A.idx_bytes()) * (double)A.nnz +
                                  (double)A.nrows * (sk_row + A.row_bytes());
          const double bytes_sk1 = (B.val_bytes() + A.idx_bytes()) * (double)A.nnz +
                                   (double)A.nrows * (5.0 * sizeof(T) + sizeof(TB) + A.row_bytes());
          // face rows: x_a and d_a (mode 1) and b read once, x_{a+2} and d_{a+2} written, x_{a+1} at the
          // 3 (n - 3) rows per face next to the skeleton
          const double bnd_rows = hf.d.n > 3 ? 3.0 * (hf.d.n - 3) * (double)hf.d.nf : 0.0;
          const double bytes_f = (double)hf.rows * ((mode == 1 ? 8.0 : 0.0) + 4.0 + 8.0) + 4.0 * bnd_rows;
          MgPairVecs pv{(const float*)b, (const float*)B.dinv, (const float*)cur, p1, p2, (const float*)dcur, dn};
          B.with_vals([&](auto* val) {
            using VT = std::remove_const_t<std::remove_pointer_t<decltype(val)>>;
            with_c16(A, [&](auto c16) {
              constexpr bool C = decltype(c16)::value;
              klaunch(-1, bytes_sk, k_cheb<T, TB, T, VT, C, 1>, dim3(nbg), dim3(BS), Ag.view(), fs, val,
                      (const T*)B.dinv, b, (const T*)(mode == 1 ? cur : nullptr), p1, dcur, c1, c2, c20, mode,
                      (const int*)ctl, (const double*)nullptr, (double*)nullptr, RedOut{}, (T*)nullptr);
              KCHK();
              if (mode == 1)
                klaunch(finest ? 10 : -1, bytes_f, k_cheb_pair<1>, dim3(hf.items), dim3(BS), hf.full(), pv, (float)c1, (float)c2,
                        (float)c20, (float)c1s[k + 1], (float)c2s[k + 1], (const int*)ctl);
              else
                klaunch(finest ? 10 : -1, bytes_f, k_cheb_pair<2>, dim3(hf.items), dim3(BS), hf.full(), pv, (float)c1, (float)c2,
                        (float)c20, (float)c1s[k + 1], (float)c2s[k + 1], (const int*)ctl);
              KCHK();
              klaunch(-1, bytes_sk1, k_cheb<T, TB, T, VT, C, 1>, dim3(nbs), dim3(BS), A.view(), fs, val,
                      (const T*)B.dinv, b, (const T*)p1, p2, dcur, c1s[k + 1], c2s[k + 1], c20, 1, (const int*)ctl,
                      (const double*)nullptr, (double*)nullptr, RedOut{}, dn);
              KCHK();
            });
          });
          ++mg_pairs;
          cur = p2;
          dcur = dn;
          ++k;
          continue;
        }
      }
      T* out = (cur == xa) ? xb : xa;
      const bool last = k == deg - 1;
      // the last step on the ghost rows one layer out too (deep halos): x two layers out and d one layer out
      const bool gl = last && last_g && dist() && L.deep;
      if (mode == 1) {
        if (gl) mg_halo(L, cur, dcur);
        else if (!(xin_cur && cur == xin && k == 0)) mg_halo(L, cur);
      }
      const DevSell& As = gl ? A.with_ghosts() : A;
      const bool timed = finest && mode != 0;
      const double* rd = last ? rdot : nullptr;
      const bool toz = last && tozr;
      if (toz) z_cur = gl;
      const FaceDev fc = rd ? hf.part() : hf.full();
      // (the grid of the own rows also with the ghost rows, whose slices its SELL blocks share: the <r, z> partials
      // keep the block count the PCG's reduction reads)
      const int nb = rd ? grid_part(fc, A) : grid_full(fc, A);
      const T* xi = mode == 1 ? cur : nullptr;
      // algorithmic bytes: matrix (value + column) per entry; per row x_in (mode 1) or b and dinv
      // (mode 2) gathered once, b, dinv, d read (mode 1), d and x_out written, <r, z>'s r; face rows
      // read no matrix and no dinv (per-face constants)
      const double rd_row = (mode == 1 ? 3.0 * sizeof(T) : 1.0 * sizeof(T)) + sizeof(TB) + (rd ? 8.0 : 0.0);
      const double rd_face = (mode == 1 ? 2.0 * sizeof(T) : 0.0) + sizeof(TB) + (rd ? 8.0 : 0.0);
      const double wr_row = 2.0 * sizeof(T);
      const double bytes = (B.val_bytes() + A.idx_bytes()) * (double)A.nnz +
                           (double)A.nrows * (rd_row + wr_row + A.row_bytes()) + (double)hf.rows * (rd_face + wr_row);
      B.with_vals([&](auto* val) {
        using VT = std::remove_const_t<std::remove_pointer_t<decltype(val)>>;
        with_c16(A, [&](auto c16) {
          constexpr bool C = decltype(c16)::value;
          T* zo = nullptr;
          if constexpr (std::is_same<T, float>::value) zo = z32;
          else zo = z;
          if (toz)
            klaunch(timed ? 0 : -1, bytes, k_cheb<T, TB, T, VT, C, 1>, dim3(nb), dim3(BS), As.view(), fc, val,
                    (const T*)B.dinv, b, xi, zo, dcur, c1, c2, c20, mode, (const int*)ctl, rd, part,
                    rd ? ro_rz : RedOut{}, (T*)nullptr);
          else if (finest)
            klaunch(timed ? 0 : -1, bytes, k_cheb<T, TB, T, VT, C, 1>, dim3(nb), dim3(BS), As.view(), fc, val,
                    (const T*)B.dinv, b, xi, out, dcur, c1, c2, c20, mode, (const int*)ctl, rd, part, RedOut{},
                    (T*)nullptr);
          else
            klaunch(-1, bytes, k_cheb<T, TB, T, VT, C, 0>, dim3(nb), dim3(BS), As.view(), fc, val, (const T*)B.dinv, b,
                    xi, out, dcur, c1, c2, c20, mode, (const int*)ctl, rd, part, RedOut{}, (T*)nullptr);
        });
      });
      KCHK();
      cur = toz ? nullptr : out;
    }
    return cur;
  }
  // The cycle's pieces, one launch site each: vcycle strings them together and pucfem_mg_probe runs them one at a
  // time against a reference.
  template <typename T>
  struct MgAt {
    MgLevel& L;
    MgBufs<T>& B;
    const DevSell& A;
    const HFace& hf;
    bool finest;
  };
  template <typename T>
  MgAt<T> mg_at(int l) {
    const bool finest = l == (int)mg.size() - 1;
    return MgAt<T>{mg[l], bufs<T>(mg[l]), finest ? dPp : mg[l].dA, finest ? fP : mg[l].hA, finest};
  }
  // coarse solve (level 0): dense pseudo-inverse (replicated on every rank of a multi-rank run)
  template <typename T>
  T* mg_coarse(const T* b) {
    MgLevel& L = mg[0];
    T* xa = bufs<T>(L).x;
    const i64 N0 = (i64)L.ord.new2old.size();
    const dim3 g((unsigned)std::min<i64>(4096, (N0 + 3) / 4));
    algo_bytes += 8.0 * (double)N0 * (double)N0 + 2.0 * sizeof(T) * (double)N0;
    hipLaunchKernelGGL(k_dense_mv<T>, g, dim3(BS), 0, st, N0, (const double*)dAinv, b, xa, ctl);
    KCHK();
    return xa;
  }
  // pre-smoothing from a zero guess
  template <typename T, typename TB>
  T* mg_pre(int l, const TB* b) {
    const MgAt<T> m = mg_at<T>(l);
    const int pre = prm.mg_degree;
    if constexpr (std::is_same<T, TB>::value) {
      // coarse levels: the fused first smoothing step reads b at ghost columns
      if (pre >= 2) mg_halo(m.L, const_cast<T*>(b));
    }
    return mg_smooth<T, TB>(m.L, m.A, m.hf, m.B, b, nullptr, m.B.x, m.B.x2, false, nullptr, nullptr, pre);
  }
  // res = b - A x (into the level's res buffer)
  template <typename T, typename TB>
  void mg_resid(int l, const TB* b, const T* x) {
    const MgAt<T> m = mg_at<T>(l);
    MgLevel& L = m.L;
    const MgBufs<T>& B = m.B;
    const DevSell& A = m.A;
    // residual: matrix entries, x gathered once, b read, res written; deep halos: also on the ghost rows one layer
    // out, which the restriction gathers (no exchange of the residual)
    const bool rg = dist() && L.res_deep && (deep_mask & 2);
    const DevSell& Ar = rg ? A.with_ghosts() : A;
    const double bytes_res = (B.val_bytes() + A.idx_bytes()) * (double)A.nnz + A.row_bytes() * (double)A.nrows +
                             (double)A.own() * (2.0 * sizeof(T) + sizeof(TB));
    const FaceDev fr = m.hf.full();
    B.with_vals([&](auto* val) {
      using VT = std::remove_const_t<std::remove_pointer_t<decltype(val)>>;
      with_c16(A, [&](auto c16) {
        if (m.finest)
          klaunch(5, bytes_res, k_resid<T, TB, VT, decltype(c16)::value, 1>, dim3(grid_full(fr, Ar)), dim3(BS),
                  Ar.view(), fr, val, b, x, B.res, (const int*)ctl);
        else
          klaunch(-1, bytes_res, k_resid<T, TB, VT, decltype(c16)::value, 0>, dim3(grid_full(fr, Ar)), dim3(BS),
                  Ar.view(), fr, val, b, x, B.res, (const int*)ctl);
      });
    });
    KCHK();
    if (!rg) mg_halo(L, B.res);
  }
  // level l's res -> level l - 1's b
  template <typename T>
  void mg_restrict(int l) {
    const MgAt<T> m = mg_at<T>(l);
    MgLevel& L = m.L;
    const MgBufs<T>& B = m.B;
    MgLevel& C = mg[l - 1];
    MgBufs<T>& CB = bufs<T>(C);
    const bool gather = C.rep && !L.rep && dist();  // into the finest replicated level
    T* cb = gather ? CB.b + L.r_r0 : CB.b;
    // restriction: entries (value + column), fine residual read once, coarse rhs written
    const FaceDev frs = L.hR.full();
    klaunch(m.finest ? 6 : -1,
            (double)(sizeof(T) + 4) * (double)L.dR.nnz + L.dR.row_bytes() * (double)L.dR.nrows +
                (double)sizeof(T) * (double)(m.A.own() + L.dR.nrows + L.hR.rows),
            k_transfer<T>, dim3(grid_full(frs, L.dR)), dim3(BS), L.dR.view(), frs, (const T*)B.Rval, (const T*)B.res,
            cb, 0, (const int*)ctl);
    KCHK();
    if (gather) {
      comm->group_start();
      for (int r = 0; r < world; ++r) comm->bcast(CB.b + C.rs[r], C.rs[r + 1] - C.rs[r], r, st);
      comm->group_end(st);
    }
  }
  // x += P xc; returns pr_deep (the prolongation also ran on this level's ghost rows)
  template <typename T>
  bool mg_prolong(int l, T* xc, T* x) {
    const MgAt<T> m = mg_at<T>(l);
    MgLevel& L = m.L;
    MgLevel& C = mg[l - 1];
    if (!(dist() && L.xc_deep && (deep_mask & 4))) mg_halo(C, xc);  // (xc_deep: level l - 1's last step wrote its ghosts one layer out)
    // prolongation: entries, coarse x read once, fine x read + written; pr_deep: also on this level's ghost rows (x
    // there is current since the exchange before the residual), so the post-smoothing starts without an exchange
    const bool pg = dist() && L.pr_deep && (deep_mask & 8) && ((deep_mask & 4) || C.rep);
    const DevSell& Apr = pg ? L.dPr.with_ghosts() : L.dPr;
    const FaceDev fpr = L.hPr.full();
    klaunch(m.finest ? 7 : -1,
            (double)(sizeof(T) + 4) * (double)L.dPr.nnz + L.dPr.row_bytes() * (double)L.dPr.nrows +
                (double)sizeof(T) * (double)(2 * m.A.own() + L.dR.nrows + L.hR.rows),
            k_transfer<T>, dim3(grid_full(fpr, Apr)), dim3(BS), Apr.view(), fpr, (const T*)m.B.Prval, (const T*)xc,
            x, 1, (const int*)ctl);
    KCHK();
    return pg;
  }
  // post-smoothing from x; toz: the last step writes z (the cycle's finest level), and nullptr is returned
  template <typename T, typename TB>
  T* mg_post(int l, const TB* b, T* x, bool toz, const double* rdot, double* part, bool pg = false) {
    const MgAt<T> m = mg_at<T>(l);
    MgLevel& L = m.L;
    // the smoother rotates through the level's two x buffers, the first being x's own.  After a pre-smoothing that
    // ended in a general pair (mg_degree 5, 9, ...) x is the pairs' extra buffer: taking it for one of the two made
    // the next pair write x_{a+1} over the x_a it reads (tests/test_gpu_mg_cycle.py, V(5,4))
    T* first = (x == m.B.x2) ? m.B.x2 : m.B.x;
    T* other = (first == m.B.x) ? m.B.x2 : m.B.x;
    const int post = prm.mg_post > 0 ? prm.mg_post : prm.mg_degree;
    // the last step on the ghost rows one layer out where its consumer gathers them: the prolongation into level
    // l + 1 (xc_deep), and z for the PCG's A z on the finest level -- there the ghost rows must repeat the owners'
    // arithmetic bit for bit (the outer fp64 PCG needs w = A z of ONE vector z: its recurrences s = A p and
    // r = b - A y hold only then), which face_ghost_rows ensures: face-interior ghost rows are their face stencils
    const bool last_g = dist() && L.deep && (deep_mask & 4) && (m.finest || mg[l + 1].xc_deep);
    return mg_smooth<T, TB>(L, m.A, m.hf, m.B, b, x, first, other, toz, rdot, part, post, last_g, pg);
  }
  // z = M^-1 r on level l (b = r_l); the finest level passes rdot = r for the <r, z> partials and
  // writes z (fp64) directly from its last smoothing step
  // (every level smooths with the finest level's degrees: fewer steps on the latency-bound coarse levels
  // cost more pressure iterations than their launches save, round 3 r8e / r8f)
  template <typename T, typename TB>
  T* vcycle(int l, const TB* b, const double* rdot, double* part) {
    if (l == 0) {
      if constexpr (std::is_same<T, TB>::value) return mg_coarse<T>(b);
      else throw Error(PUCFEM_ESTATE, "multigrid hierarchy has a single level");
    }
    T* x = mg_pre<T, TB>(l, b);
    mg_halo(mg[l], x);
    mg_resid<T, TB>(l, b, (const T*)x);
    mg_restrict<T>(l);
    T* xc = vcycle<T, T>(l - 1, bufs<T>(mg[l - 1]).b, nullptr, nullptr);
    const bool pg = mg_prolong<T>(l, xc, x);
    return mg_post<T, TB>(l, b, x, l == (int)mg.size() - 1, rdot, part, pg);
  }
  // z = M^-1 r (finest level), <r, z> partials in part_d + 2 MAXB.  The fp32 cycle reads r32 (owned
  // rows written by k_cg_init / k_cg_upd; its ghosts are exchanged by the cycle); the fp64 one r itself
  void precondition(double* rz_part = nullptr) {
    if (!rz_part) rz_part = part_d + 2 * MAXB;
    z_cur = false;
    if (mg_single) {
      vcycle<float, float>((int)mg.size() - 1, r32, cg_r[0], rz_part);
    } else {
      halo(cg_r[0]);
      vcycle<double, double>((int)mg.size() - 1, cg_r[0], cg_r[0], rz_part);
    }
  }
  // precondition() as the standard PCG calls it, with <r, z> reduced (nb: the grid of the cycle's last step)
  Red precondition_rz(int nb) {
    ro_rz = ro(redbuf + 32, CNT_RZ, 1);
    precondition();
    ro_rz = RedOut{};
    Red rz{redbuf + 32, 1, 1};
    if (ro(redbuf + 32, CNT_RZ, 1).out) red_done(redbuf + 32, 1, false);
    else rz = reduce_global(part_d + 2 * MAXB, nb, 1, false, 4);
    return rz;
  }
  // Chronopoulos-Gear PCG (k_cgcg_*): the multi-rank pressure solves, one all-reduce per iteration instead of three;
  // PUCFEM_CGCG=1 / 0 forces it on / off (measurement and test knob: the single-rank path keeps the standard form,
  // 24 B/row less per iteration)
  int cgcg_env = std::getenv("PUCFEM_CGCG") ? std::atoi(std::getenv("PUCFEM_CGCG")) : -1;
  bool use_cgcg() const { return cgcg_env >= 0 ? cgcg_env != 0 : dist(); }
  double* part_cc = nullptr;  // CGCG_NV x MAXB partials
  double* cgcg_sc = nullptr;  // k_cgcg_coef's scalars (8)
  int64_t cgcg_iters = 0;     // iterations run in the single-reduction form (pucfem_path_info bit 7)
  // preconditioned CG on the unscaled merged pressure operator (finest level = dPp / dKp_raw)
  // prm.proj_shared: both pressure solves of a step project onto ONE basis (the same merged operator, so
  // one A-orthonormal basis serves both) that collects the solutions of both -- slot 1 for both; else a
  // basis per solve.  Separate bases stop improving at 16 directions; a shared one keeps improving up to
  // PROJ_MAX = 32 (r8l: 72 -> 63 pressure iterations over the driver window, +2 % steps/s)
  // PUCFEM_PCG_TRACE=1 (diagnostic): the relative residual of every pressure PCG iteration on stderr (a host
  // round trip per iteration)
  bool pcg_trace = false;  // (read at every solve)
  long n_pcg_traced = 0;
  void trace_pcg(int which, int it) {
    double h[5];
    HIPCHK(hipMemcpyAsync(h, redbuf, sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(h + 1, redbuf + 8, sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(h + 2, redbuf + 32, sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(h + 3, ctl, sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    int cc[2];
    std::memcpy(cc, h + 3, sizeof(cc));
    if (it == 0) ++n_pcg_traced;
    std::fprintf(stderr, "[pcg] solve %ld (slot %d) it %d |r|/|b| %.3e <r,z> %.3e ctl %d/%d\n", n_pcg_traced, which, it,
                 std::sqrt(h[0] / h[1]), h[2], cc[0], cc[1]);
  }
  // the PCG's initial <r, r> and <b, b> beside the control word (k_conv / k_reduce_conv write them at iteration
  // 0; pcg_mg's control reads bring them along): the projected guess's quality, h_note() after a solve
  double* ctl_note() const { return reinterpret_cast<double*>(ctl + 2); }
  double guess_rel() const {
    const double* h = reinterpret_cast<const double*>(h_ctl + 2);
    return h[1] > 0.0 ? std::sqrt(h[0] / h[1]) : 0.0;
  }
  // Guess monitor (round 5).  A projection basis whose A-orthonormality has decayed (rounding of the fp32 basis
  // through repeated re-seeds; with 12 directions, re-seeded every solve, steady L7 steps went from 0-1 to 5
  // iterations per solve, r11g) gives guesses orders of magnitude worse than the last ones while the flow
  // changes smoothly; the decay builds up over a few solves (r11h: 5e-8 -> 1e-4 of b in ~4 solves).  When a
  // projected guess's relative residual exceeds 50x the best of the last 8 projected guesses of its basis (and
  // 10x the tolerance), the basis restarts from the next solution (Fischer's restart).  Healthy steady guesses
  // spread over ~10x (2.6e-8 .. 2.9e-7 at L7, r11e); in the start-up transient they fall step by step.
  static constexpr int GUESS_HIST = 8;
  double guess_last[5] = {0, 0, 0, 0, 0};
  double guess_hist[5][GUESS_HIST] = {};
  int guess_n[5] = {0, 0, 0, 0, 0};
  int64_t n_restart = 0;
  bool guess_decayed(int slot, double g) {
    double best = 0.0;
    const int k = std::min(guess_n[slot], GUESS_HIST);
    for (int i = 0; i < k; ++i) best = i == 0 ? guess_hist[slot][i] : std::min(best, guess_hist[slot][i]);
    guess_hist[slot][guess_n[slot] % GUESS_HIST] = g;
    ++guess_n[slot];
    guess_last[slot] = g;
    return k > 0 && g > 50.0 * best && g > 10.0 * prm.rtol_pres;
  }
  void proj_restart(int slot) {
    proj_m[slot] = 0;
    proj_pend[slot] = false;
    pend_otf[slot] = false;
    pend_acc[slot] = false;
    pend_vzero[slot] = false;
    proj_hist[slot] = ProjHist{};
    guess_n[slot] = 0;
    ++n_restart;
  }
  bool proj_shared = false;  // prm.proj_shared
  int proj_slot(int which) const { return proj_shared && which == 2 ? 1 : which; }
  int pcg_mg(double* y, const double* b, double tol, int maxit, int which) {
    const FaceDev fc = fP.part();
    const int nb = grid_part(fc, dPp);  // also the grid of the V-cycle's last smoothing step (<r, z> partials)
    const i64 n = dPp.own();
    const int nbu = nb_rows(n);
    CgVecs<1> v;
    v.y[0] = y;
    v.b[0] = b;
    v.r[0] = z;  // the gathered "r" of k_cg_dir is the preconditioned residual
    v.zf[0] = z32;  // (in fp32 from the fp32 V-cycle)
    v.po[0] = cg_pa[0];
    v.pn[0] = cg_pb[0];
    v.q[0] = cg_q[0];
    CgVecs<1> vi = v;
    vi.r[0] = cg_r[0];
    halo(y);
    HIPCHK(hipMemsetAsync(ctl, 0, 2 * sizeof(int), st));
    float* r32o = mg_single ? r32 : nullptr;
    // the projection's update takes A (y - x0) = r0 - r_final from the CG's residuals: k_cg_init
    // keeps r0 in pav (its "first direction" output; pcg_mg's directions live elsewhere)
    const bool keep_r0 = proj_k > 0 && (which == 1 || which == 2);
    if (keep_r0) vi.po[0] = pav[proj_slot(which)];
    algo_bytes += (8.0 + dPp.idx_bytes()) * (double)dPp.nnz + dPp.row_bytes() * (double)dPp.nrows +
                  (24.0 + (mg_single ? 4.0 : 0.0) + (keep_r0 ? 8.0 : 0.0)) * (double)n;
    // fused reductions: <r, r> -> redbuf slot 0, <b, b> -> slot 1 (as k_reduce would place them)
    const RedOut ri = ro(redbuf, CNT_INIT, 2, MAXB, 0u, redbuf + 8);
    with_c16(dPp, [&](auto c16) {
      hipLaunchKernelGGL((k_cg_init<1, decltype(c16)::value>), dim3(nb), dim3(BS), 0, st, dPp.view(), fc, dKp_raw, vi,
                         lp.n_ghost, part_a, ri.out ? part_a + MAXB : part_b, r32o, keep_r0 ? 1 : 0, ri);
    });
    KCHK();
    Red rr{redbuf, 1, 1}, bb{redbuf + 8, 1, 1};
    const double tol2 = tol * tol;
    // single rank with k_reduce: the reduction of <b, b> (and, per iteration, of <r, r>) also runs the
    // convergence test (k_reduce_conv: one launch instead of k_reduce + k_conv; multi-rank runs test after
    // the all-reduce)
    const bool merged_conv = !dist() && !ri.out;
    if (ri.out) {
      red_done(redbuf, 1, false);
      red_done(redbuf + 8, 1, false);
    } else {
      rr = reduce_global(part_a, nb, 1, false, 0);
      if (merged_conv) {
        hipLaunchKernelGGL(k_reduce_conv, dim3(1), dim3(RB), 0, st, (const double*)part_b, nb, MAXB, redbuf + 8,
                           (const double*)rr.p, (const double*)(redbuf + 8), tol2, ctl, 0, ctl_note());
        KCHK();
      } else {
        bb = reduce_global(part_b, nb, 1, false, 1);
      }
    }
    const RedOut rdir = ro(redbuf + 16, CNT_DIR, 1), rupd = ro(redbuf, CNT_UPD, 1);
    // (iteration, first timing sample): samples from the converged iteration on are dropped
    std::vector<std::pair<int, size_t>> marks;
    std::vector<std::pair<int, ByteMark>> bmarks;  // (iteration, the byte counters at its start) of the current chunk
    if (!merged_conv) {
      hipLaunchKernelGGL(k_conv, dim3(1), dim3(64), 0, st, rr.p, bb.p, tol2, ctl, 0, 1, ctl_note());
      KCHK();
    }
    // direction: z (4 B in the fp32 cycle) and p_old gathered once, p and q written
    const double bytes_dir = (8.0 + dPp.idx_bytes()) * (double)dPp.nnz + dPp.row_bytes() * (double)dPp.nrows +
                             (mg_single ? 28.0 : 32.0) * (double)n;
    const double bytes_upd = (48.0 + (mg_single ? 4.0 : 0.0)) * (double)n;  // + the fp32 r copy
    // the single-reduction form: w = A z (z gathered once, r and s_old read, w written), the update (z, w, p, s,
    // y, r read; p, s, y, r written; the fp32 r copy, the accumulated correction)
    const bool cgcg = use_cgcg();
    const double zb = mg_single ? 4.0 : 8.0;
    const double bytes_w = (8.0 + dPp.idx_bytes()) * (double)dPp.nnz + dPp.row_bytes() * (double)dPp.nrows +
                           (zb + 24.0) * (double)n;
    const double bytes_cu = (zb + 72.0 + (mg_single ? 4.0 : 0.0) + (cg_vacc ? 16.0 : 0.0)) * (double)n;
    const double* rho0 = rr.p;  // the initial <r, r> (k_cgcg_coef's rho at iteration 0)
    int it = 0;
    // an iteration = V-cycle, direction, update, convergence test (k_conv): the host checks right
    // after a test, so a solve that converges at a check launches no V-cycle after it.  The first
    // check comes one iteration before the last solve's count (a no-op iteration costs more than a
    // check's round trip), then every iteration while the solve is short.  Past the start-up transient
    // the projected guess often passes the test itself (0 iterations): when the last solve took at most
    // one iteration and, of the last 8 such solves, at least 2 passed at their guess, the host reads the
    // initial test before launching any (one round trip, where an iteration of early-exiting launches --
    // the V-cycle's ~70 -- costs ~0.3 ms of GPU time; in the start-up transient, where no solve passes at
    // its guess, the round trip would only idle the GPU: +0.25 ms per step in the driver window, r10b)
    pcg_trace = std::getenv("PUCFEM_PCG_TRACE") && std::atoi(std::getenv("PUCFEM_PCG_TRACE")) != 0;
    if (pcg_trace) trace_pcg(which, 0);
    const bool seen = solved_before[which];
    solved_before[which] = true;
    int chunk = std::max(1, std::min(maxit + 1, !seen ? 4 : (last_it[which] > 1 ? last_it[which] - 1 : 1)));
    bool done0 = false;
    const bool eligible = seen && last_it[which] <= 1;
    if (eligible && __builtin_popcount(zero_hist[which] & 0xffu) >= 2) {
      read_ctl();
      done0 = h_ctl[0] != 0;
    }
    for (bool first = true; !done0; first = false) {
      if (!first) marks.clear();  // the previous chunk's samples are flushed
      bmarks.clear();
      for (int k = 0; k < chunk; ++k, ++it) {
        marks.push_back({it, timer.mark()});  // this iteration's V-cycle works iff not converged at it
        bmarks.push_back({it, bmark_now()});
        if (cgcg) {  // single-reduction iteration (k_cgcg_*)
          ++cgcg_iters;
          precondition(part_cc + 3 * MAXB);
          if (!z_cur) {  // (deep halos: the last smoothing step wrote z's ghosts one layer out, bit for bit)
            if (mg_single) mg_halo(mg.back(), z32);
            else halo(z);
          }
          with_c16(dPp, [&](auto c16) {
            if (mg_single)
              klaunch(1, bytes_w, k_cgcg_w<decltype(c16)::value, true>, dim3(nb), dim3(BS), dPp.view(), fc,
                      (const double*)dKp_raw, (const double*)nullptr, (const float*)z32, (const double*)cg_r[0],
                      it > 0 ? (const double*)cg_q[0] : (const double*)nullptr, cg_pb[0], part_cc, (const int*)ctl);
            else
              klaunch(1, bytes_w, k_cgcg_w<decltype(c16)::value, false>, dim3(nb), dim3(BS), dPp.view(), fc,
                      (const double*)dKp_raw, (const double*)z, (const float*)nullptr, (const double*)cg_r[0],
                      it > 0 ? (const double*)cg_q[0] : (const double*)nullptr, cg_pb[0], part_cc, (const int*)ctl);
          });
          KCHK();
          launch_reduce(part_cc, nb, MAXB, CGCG_NV, false, redbuf + 64);
          KCHK();
          if (dist()) comm->allreduce(redbuf + 64, CGCG_NV, false, st);
          hipLaunchKernelGGL(k_cgcg_coef, dim3(1), dim3(64), 0, st, (const double*)(redbuf + 64), (const double*)bb.p,
                             cgcg_sc, tol2, ctl, it, maxit, (const double*)rho0);
          KCHK();
          if (mg_single)
            klaunch(2, bytes_cu - (cg_vacc && it == 0 ? 8.0 * (double)n : 0.0), k_cgcg_upd<true>, dim3(nb), dim3(BS),
                    (int64_t)n, (const double*)nullptr,
                    (const float*)z32, (const double*)cg_pb[0], cg_pa[0], cg_q[0], y, cg_r[0], r32o, cg_vacc,
                    (const double*)cgcg_sc, (const int*)ctl, it, part_cc);
          else
            klaunch(2, bytes_cu - (cg_vacc && it == 0 ? 8.0 * (double)n : 0.0), k_cgcg_upd<false>, dim3(nb), dim3(BS),
                    (int64_t)n, (const double*)z,
                    (const float*)nullptr, (const double*)cg_pb[0], cg_pa[0], cg_q[0], y, cg_r[0], r32o, cg_vacc,
                    (const double*)cgcg_sc, (const int*)ctl, it, part_cc);
          KCHK();
          if (pcg_trace) trace_pcg(which, it + 1);
          continue;
        }
        const Red rz = precondition_rz(nb);
        if (!z_cur) {
          if (mg_single) mg_halo(mg.back(), z32);
          else halo(z);
        }
        with_c16(dPp, [&](auto c16) {
          if (mg_single)
            klaunch(1, bytes_dir, k_cg_dir<1, 8, true, decltype(c16)::value, true>, dim3(nb), dim3(BS), dPp.view(), fc,
                    (const double*)dKp_raw, v, lp.n_ghost, rz.p, rz.nb, rz.stride, bb.p, bb.nb, bb.stride, scal, ctl,
                    it, maxit, tol2, part_c, rr.p, rr.nb, rr.stride, rdir);
          else
            klaunch(1, bytes_dir, k_cg_dir<1, 8, true, decltype(c16)::value>, dim3(nb), dim3(BS), dPp.view(), fc,
                    (const double*)dKp_raw, v, lp.n_ghost, rz.p, rz.nb, rz.stride, bb.p, bb.nb, bb.stride, scal, ctl,
                    it, maxit, tol2, part_c, rr.p, rr.nb, rr.stride, rdir);
        });
        KCHK();
        Red pq{redbuf + 16, 1, 1};
        if (rdir.out) red_done(redbuf + 16, 1, false);
        else pq = reduce_global(part_c, nb, 1, false, 2);
        CgVecs<1> vu = v;
        vu.r[0] = cg_r[0];
        klaunch(2, bytes_upd + (cg_vacc ? (it == 0 ? 8.0 : 16.0) * (double)n : 0.0), k_cg_upd<1>, dim3(nbu), dim3(BS),
                vu, n, pq.p, pq.nb, pq.stride, (const double*)scal, (const int*)ctl, part_a, r32o, rupd, cg_vacc,
                it == 0 ? 1 : 0);
        KCHK();
        if (rupd.out) rr = Red{redbuf, 1, 1}, red_done(redbuf, 1, false);
        else if (!merged_conv) rr = reduce_global(part_a, nbu, 1, false, 0);
        if (merged_conv) {
          rr = Red{redbuf, 1, 1};
          hipLaunchKernelGGL(k_reduce_conv, dim3(1), dim3(RB), 0, st, (const double*)part_a, nbu, MAXB, redbuf,
                             (const double*)redbuf, (const double*)bb.p, tol2, ctl, it + 1);
        } else {
          hipLaunchKernelGGL(k_conv, dim3(1), dim3(64), 0, st, rr.p, bb.p, tol2, ctl, it + 1, 1);
        }
        KCHK();
        std::swap(v.po[0], v.pn[0]);
        if (pcg_trace) trace_pcg(which, it + 1);
      }
      // the samples before this chunk, while the GPU runs it (this chunk's stay pending until its test is read)
      if (timer.on && !marks.empty()) timer.flush_ready(marks.front().second);
      read_ctl(it >= last_it[which]);
      if (timer.on && h_ctl[0])  // iterations from the converged one on launched kernels that did no work
        for (auto& mk : marks)
          if (mk.first >= h_ctl[1]) {
            timer.drop_from(mk.second);
            break;
          }
      if (h_ctl[0])  // the bytes of the iterations that found the solve converged did not move
        for (auto& bm : bmarks)
          if (bm.first >= h_ctl[1]) {
            bmark_restore(bm.second);
            break;
          }
      if (h_ctl[0]) break;
      chunk = it < 8 ? 1 : std::min(16, it / 4);
    }
    last_it[which] = h_ctl[1];
    if (eligible) zero_hist[which] = (zero_hist[which] << 1) | (h_ctl[1] == 0 ? 1u : 0u);
    if (h_ctl[0] == 3) throw Error(PUCFEM_ENOCONV, "MG-PCG residual is not finite (iteration " + std::to_string(h_ctl[1]) + ")");
    if (h_ctl[0] != 1) throw Error(PUCFEM_ENOCONV, "MG-PCG did not converge within maxit=" + std::to_string(maxit));
    return h_ctl[1];
  }

  // ------------------------------------------------------------------ building blocks of the step
  // makePerBCU + makeDirBCU on owned rows: the interleaved velocity (a = its x components, b = a + 1), or with
  // b null one plain vector (the heat / Poisson scalar)
  void bc(double* a, double* b) {
    const int vs = b ? VS : 1;
    if (ncopy == 0 && ndir == 0) return;
    const int nb = (int)std::min<i64>(1024, std::max<i64>(1, (ncopy + ndir + BS - 1) / BS));
    if (bc_gather && ncopy > 0) {
      hipLaunchKernelGGL(k_bc_gather, dim3(std::min(1024, (ncopy + BS - 1) / BS)), dim3(BS), 0, st, ncopy, dcsrc,
                         dbctmp, dir_ncomp, a, b, vs);
      KCHK();
    }
    hipLaunchKernelGGL(k_bc_apply, dim3(nb), dim3(BS), 0, st, ncopy, dcdst, dcsrc,
                       bc_gather ? (const double*)dbctmp : nullptr, ndir, ddnode, ddval, dir_ncomp, a, b, vs);
    KCHK();
  }
  // halo of the interleaved velocity u / u* (component pointers)
  void halo_v(double* vx) { halo2(reinterpret_cast<dbl2*>(vx)); }
  int viscous(int& iters) {  // StokesColor.py:540-547
    const i64 n = lp.n_own;
    // the right-hand side and the base of the start and of the increments: u^n, or with inertia on the advected u_a
    // (inertia_step ran in front); with a body force r = that + dt * f (force_step ran behind it)
    const double *rx = forced() ? u_rhs : inertia ? u_adv : ux, *ry = rx + 1;
    if (dense) {  // u* = A_visc^-1 (u + DT * 0)
      if (dbcsrc && dir_ncomp == 2) {  // (velocity BCs: both components copied / set)
        hipLaunchKernelGGL(k_dense_mv2_bc, dim3((int)std::min<i64>(2048, (n + 3) / 4)), dim3(BS), 0, st, n, dVinv, rx,
                           ry, usx, usy, (const int32_t*)dbcsrc, (const int32_t*)dbcdir, (const double*)ddval,
                           dir_ncomp);
        KCHK();
      } else {
        hipLaunchKernelGGL(k_dense_mv2, dim3((int)std::min<i64>(2048, (n + 3) / 4)), dim3(BS), 0, st, n, dVinv, rx, ry,
                           usx, usy);
        KCHK();
        bc(usx, usy);
      }
      iters = 0;
      return 0;
    }
    const bool ext = dvinc[0] != nullptr && !proj_k_visc;
    VincDev vd{};
    vd.order = ext ? std::min(have_vinc, visc_extrap) : 0;
    for (int k = 0; k < 2 * VINC_MAX; ++k) vd.d[k] = dvinc[k];
    const bool proj = proj_k_visc > 0;
    // the Chebyshev iteration (interleaved vectors); the CG (SoA vectors) when the interval is too wide, the
    // post-check failed, the operator is small enough for the one-workgroup CG, or the projection guess of
    // the viscous solve is on (a measurement knob whose bases hold SoA vectors)
    const bool cheb = visc_solver == 0 && visc_R < 0.25 && !proj &&
                      !(!dist() && block_cg && !fVisc.items && dP.nrows <= (int64_t)CGB_THREADS * CGB_MAXR);
    // (k_visc_prep folded into the solve's first step was measured 9 % slower in round 3, r9i: the window
    // recomputes the start's 64 B/row of inputs on 25 % more rows, so the fusion saved no bytes)
    // (folded into the previous step's second k_grad_proj, which holds the final u in registers: bit-identical,
    // ~50 us less kernel time per step, yet 0.4-1.4 % slower in four A/B pairs with and without the dye
    // overlap, r11s; not kept)
    // u, s, the increments read; b, y written
    const double prep_bytes = (56.0 + 8.0 * vd.order) * (double)n;
    if (cheb)
      klaunch(13, prep_bytes, k_visc_prep<true>, dim3(grid_ew(n)), dim3(BS), (int64_t)n, (const double*)dsv,
              rx, ry, reinterpret_cast<double*>(vb2),
              (double*)nullptr, reinterpret_cast<double*>(vx2[0]), (double*)nullptr, vd);
    else
      klaunch(13, prep_bytes, k_visc_prep<false>, dim3(grid_ew(n)), dim3(BS), (int64_t)n, (const double*)dsv,
              rx, ry, bvx, bvy, yvx, yvy, vd);
    KCHK();
    // with the extrapolated start the solve's last Chebyshev step also does k_visc_fin's work
    const int last = 2 * (visc_extrap - 1);
    bool fin_done = false;
    if (cheb) {
      ViscFin vf{};
      const bool fuse = ext;
      if (fuse) vf = ViscFin{dsv, {rx, ry}, {usx, usy}, {dvinc[last], dvinc[last + 1]}};
      dbl2* yo = vx2[0];  // the converged iterate (one of the solve's buffers)
      iters = vcheb(dP, fVisc, dKv, vx2[0], vb2, prm.rtol_visc, prm.maxit_visc, 0, &yo, fuse ? &vf : nullptr,
                    &fin_done);
      if (!fin_done) {  // u* = S y (and the increment)
        algo_bytes += (ext ? 64.0 : 40.0) * (double)n;  // s, y (, u) read; u* (, the fp32 increment) written
        hipLaunchKernelGGL(k_visc_fin, dim3(grid_ew(n)), dim3(BS), 0, st, (int64_t)n, (const double*)dsv,
                           (const dbl2*)yo, rx, ry, usx, usy,
                           ext ? dvinc[last] : (float*)nullptr, ext ? dvinc[last + 1] : (float*)nullptr);
      }
    } else {
      proj_materialize();  // (the CG's vectors include cg_r[0], a pending pressure direction's input)
      double* y[2] = {yvx, yvy};
      const double* b[2] = {bvx, bvy};
      if (proj) {  // the warm start u^n is replaced by the projection onto earlier solutions
        project_guess(3, bvx, yvx);
        project_guess(4, bvy, yvy);
      }
      iters = cg<2>(dP, fVisc, dKv, y, b, prm.rtol_visc, prm.maxit_visc, 0);
      if (proj) {
        project_update(3, yvx);
        project_update(4, yvy);
      }
      if (ext) {
        algo_bytes += 64.0 * (double)n;  // s, y, u read; u*, the fp32 increment written
        hipLaunchKernelGGL(k_visc_fin_soa, dim3(grid_ew(n)), dim3(BS), 0, st, (int64_t)n, (const double*)dsv,
                           (const double*)yvx, (const double*)yvy, rx, ry, usx, usy,
                           dvinc[last], dvinc[last + 1]);
      } else {
        algo_bytes += 40.0 * (double)n;
        hipLaunchKernelGGL(k_cg_fin, dim3(grid_ew(n)), dim3(BS), 0, st, n, 2, dsv, yvx, yvy, usx, usy,
                           (const int32_t*)nullptr, VS);
      }
    }
    if (ext) {  // the new increment replaces the oldest: (d1, d2, d3) <- (new, d1, d2)
      for (int k = last; k >= 2; k -= 2) {
        std::swap(dvinc[k], dvinc[k - 2]);
        std::swap(dvinc[k + 1], dvinc[k - 1]);
      }
      have_vinc = std::min(have_vinc + 1, visc_extrap);
    }
    KCHK();
    bc(usx, usy);
    halo_v(usx);
    return 0;
  }
  // grid of k_div (its partials: max |div|, sum braw)
  int div_grid() const { return grid_part(fK.part(), dP); }
  void div(const double* ax, const double* ay, double* out, bool rhs, double* part = nullptr, RedOut r = RedOut{}) {
    const FaceDev fc = fK.part();
    with_c16(dP, [&](auto c16) {
      // ux, uy gathered once; div (when stored) and braw (the pressure rhs) written
      klaunch(11,
              (16.0 + dP.idx_bytes()) * (double)dP.nnz + dP.row_bytes() * (double)dP.nrows +
                  (16.0 + (out ? 8.0 : 0.0) + (rhs ? 8.0 : 0.0)) * (double)lp.n_own,
              k_div<decltype(c16)::value, true>, dim3(div_grid()), dim3(BS), dP.view(), fc, (const double*)dGx,
              (const double*)dGy, ax, ay, (const double*)das1, out, (const double*)dmp, -(1.0 / prm.dt),
              rhs ? braw : (double*)nullptr, part ? part : part_d, r);
    });
    KCHK();
  }
  // k_div<CURL> on the interleaved velocity a (pucfem.h: PUCFEM_F_VORTICITY, pucfem_flow_info): the vorticity into
  // out (null: not stored) and the flow partials into flow_part(), with the |u|^2 pair when energy; r reduces them
  // in the launch.  Formed when read, outside the step: no kernel class, no counters, no step buffer written.
  double* flow_part() { return smp_scratch<double>(9, 4 * MAXB + 4); }
  void curl(const double* a, double* out, bool energy, RedOut r = RedOut{}) {
    const FaceDev fc = fK.part();
    double* part = flow_part();
    with_c16(dP, [&](auto c16) {
      hipLaunchKernelGGL((k_div<decltype(c16)::value, true, true>), dim3(div_grid()), dim3(BS), 0, st, dP.view(), fc,
                         (const double*)dGx, (const double*)dGy, a, (const double*)nullptr, (const double*)das1, out,
                         energy ? a : (const double*)nullptr, 0.0, (double*)nullptr, part, r);
    });
    KCHK();
  }
  // Where the owned rows of a one-component field lie (null: not such a field).  The fields the step does not store
  // are formed first, on st, into dst() -- called only then: p / p2 kept in y (the slaves not copied), div u*, the
  // final divergence (the implicit dye variant keeps its own copy) and the vorticity, from u (whose ghosts are
  // current after every write of u).  pucfem_get_field forms them in place, the samplers in buffers of their own.
  template <class Dst>
  const double* formed(int32_t field, Dst&& dst) {
    const bool stokes = scheme == PUCFEM_STOKES_COLOR || scheme == PUCFEM_STOKES_FOOD;
    switch (field) {
      case PUCFEM_F_P:
      case PUCFEM_F_P2: {
        const bool first = field == PUCFEM_F_P;
        if (!p_from_y) return first ? p : p2;
        double* s = dst();
        hipLaunchKernelGGL(k_cg_fin, dim3(grid_ew(lp.n_own)), dim3(BS), 0, st, lp.n_own, 1, (const double*)nullptr,
                           (const double*)(first ? yp : yp2), (const double*)nullptr, s, (double*)nullptr,
                           (const int32_t*)dmaster_of);
        KCHK();
        return s;
      }
      case PUCFEM_F_DIV_STAR:
      case PUCFEM_F_FINAL_DIV: {
        const bool star = field == PUCFEM_F_DIV_STAR;
        if (!stokes || (!star && dye_impl)) return star ? div_star : final_div;
        double* s = dst();
        div(star ? usx : ux, star ? usy : uy, s, false);
        return s;
      }
      case PUCFEM_F_VORTICITY: {
        if (!stokes) throw Error(PUCFEM_ESTATE, "vorticity needs a Stokes context");
        double* s = dst();
        curl(ux, s, false);
        return s;
      }
      case PUCFEM_F_DIV_U: return div_u;
      case PUCFEM_F_SCALAR: return scalar;
      default: return nullptr;
    }
  }
  // the context's interleaved-u scratch (x at [0], y at [1], stride 2; 4 x nloc in all, pucfem_solve's four vectors):
  // the unit operations put a caller's u here as the step stores it, and the step's state stays untouched
  double* u_scratch() {
    if (!solve_tmp) solve_tmp = dalloc<double>(4 * nloc);
    return solve_tmp;
  }
  // sb_fused: the preceding k_div reduced sum(braw) into redbuf slot 3 itself (div_rhs)
  // PUCFEM_RHS_FUSE=0 (measurement knob): the pressure right-hand side always in its own pass (k_pres_rhs)
  bool rhs_fuse = !(std::getenv("PUCFEM_RHS_FUSE") && std::atoi(std::getenv("PUCFEM_RHS_FUSE")) == 0);
  int pressure(double* yst, double* pout, int which, bool sb_fused = false) {  // StokesColor.py:554-555 (restated)
    const int nb = div_grid();
    Red sb{redbuf + 24, 1, 1};
    if (!sb_fused) sb = reduce_global(part_d + MAXB, nb, 1, false, 3);
    const i64 n = lp.n_own;
    const double* sc = (use_mg || dense) ? nullptr : dsp;  // MG and dense paths solve the unscaled system
    const bool proj = use_mg && proj_k > 0 && (which == 1 || which == 2);
    // with a projected guess k_mdot2 (the first pass over the rows) forms the right-hand side itself
    const bool rhs_in_mdot = proj && rhs_fuse && !sc && proj_pend[proj_slot(which)];
    if (dense) {  // small meshes: right-hand side, dense solve and p in one launch (k_dense_pres)
      algo_bytes += 8.0 * (double)n * (double)n + 48.0 * (double)n;
      hipLaunchKernelGGL(k_dense_pres, dim3((int)std::min<i64>(2048, (n + 3) / 4)), dim3(BS), 0, st, n,
                         (const double*)dPinv, (const double*)braw, (const int32_t*)dslave_of,
                         (const int32_t*)dmaster_of, sb.p, sb.nb, 1.0 / (double)n_free, yst, pout);
      KCHK();
      halo(pout);
      return 0;
    }
    if (!rhs_in_mdot) {
      algo_bytes += 24.0 * (double)n;  // braw, slave_of, master_of read; bh written
      hipLaunchKernelGGL(k_pres_rhs, dim3(grid_ew(n)), dim3(BS), 0, st, n, braw, dslave_of, dmaster_of, sc,
                         sb.p, sb.nb, 1.0 / (double)n_free, bh);
      KCHK();
    }
    if (!prm.warm_start) HIPCHK(hipMemsetAsync(yst, 0, sizeof(double) * nloc, st));
    const RhsIn rin{braw, dslave_of, sb.p, 1.0 / (double)n_free, bh};
    const bool projected = proj && project_guess(proj_slot(which), bh, yst, rhs_in_mdot ? &rin : nullptr);
    const bool acc = projected;  // the CG accumulates v (k_pcomb cleared pv)
    int it;
    if (dense) {
      hipLaunchKernelGGL(k_dense_mv<double>, dim3((int)std::min<i64>(2048, (n + 3) / 4)), dim3(BS), 0, st, n, dPinv, bh, yst,
                         (const int*)nullptr);
      KCHK();
      it = 0;
    } else if (use_mg) {
      // separate bases: the other slot's pending direction reads the r_final this solve overwrites
      proj_materialize(proj ? proj_slot(which) : 0);
      cg_vacc = acc ? pv[proj_slot(which)] : nullptr;
      it = pcg_mg(yst, bh, prm.rtol_pres, prm.maxit_pres, which);
      cg_vacc = nullptr;
      // (the projection update and the finish in one pass: sc is null on the multigrid path)
      if (proj) {
        const int slot = proj_slot(which);
        pend_acc[slot] = acc;
        pend_vzero[slot] = acc && it == 0;
        if (p_from_y && proj_m[slot] > 0) {  // the direction stays pending (the next solve forms it)
          pend_otf[slot] = true;
          pend_y[slot] = yst;
          proj_pend[slot] = true;
        } else {
          project_update(slot, yst, bh, cg_r[0], pout);
        }
        if (projected && guess_decayed(slot, guess_rel())) proj_restart(slot);
      }
    } else {
      double* y[1] = {yst};
      const double* b[1] = {bh};
      it = cg<1>(dPp, HFace{}, dKp, y, b, prm.rtol_pres, prm.maxit_pres, which);
    }
    if (use_mg && proj && p_from_y) {  // p stays in y: the gradient gathers y's ghosts
      halo(yst);
      return it;
    }
    if (!(use_mg && proj)) {
      algo_bytes += (20.0 + (sc ? 8.0 : 0.0)) * (double)n;  // master_of, y (, s) read; p written
      hipLaunchKernelGGL(k_cg_fin, dim3(grid_ew(n)), dim3(BS), 0, st, n, 1, sc, yst, (const double*)nullptr, pout,
                         (double*)nullptr, dmaster_of);
      KCHK();
    }
    halo(pout);
    return it;
  }
  // Successive right-hand sides (Fischer 1998) with a deferred update.
  // Guess for the right-hand side b: x0 = sum_i <X_i, b> X_i, the A-projection of the new solution
  // onto span X (X A-orthonormal).  Before it, the last solve's direction v = y - x0 (with A v) is
  // A-orthogonalised against X, cleared of the operator's null space and appended:
  //   X_m = s (v - mu 1_free - sum_i c_i X_i),  c_i = <X_i, A v>,  s = (<v, A v> - |c|^2)^-1/2,
  //   <X_m, b> = s (<v, b> - mu sum_free b - sum_i c_i <X_i, b>),
  // so one multi-dot pass over X (dots with b and A v, k_mdot2) and one combination pass (X_m and
  // x0 together, k_pcomb) do both: 2m + 9 vector passes per solve where a separate update took
  // 4m + 15.  A full basis is re-seeded first (proj_reseed).  With an empty basis the solve keeps
  // its warm start (x0 = 0).
  // returns whether a guess was projected (false: the first solve of the basis keeps its warm start)
  // rin: the right-hand side b is formed (and stored) by k_mdot2 from the divergence instead of read
  bool project_guess(int which, const double* b, double* y, const RhsIn* rin = nullptr) {
    const i64 n = lp.n_own;
    const ProjOp op = proj_op(which);
    ProjHist& H = proj_hist[which];
    proj_coords(which);
    int m = proj_m[which];
    if (!proj_pend[which]) {  // first solve: no direction yet
      HIPCHK(hipMemsetAsync(proj_x0[which], 0, sizeof(double) * n, st));
      H.gamma.clear();
      return false;
    }
    const int nb = grid_ew(n);
    const RedOut rmd = ro(proj_d, CNT_MDOT, 2 * m + 4);
    // k_mdot2: X (fp32), b, A v, v read
    const bool otf = pend_otf[which];
    // a pending direction: A v from the residuals; v accumulated (pend_acc) or y - x0 (the first direction)
    const bool vdiff = otf && !pend_acc[which];
    const bool vz0 = pend_vzero[which];  // (v = 0: neither v nor y - x0 is read)
    const double* vp = vz0 ? nullptr : (const double*)pv[which];
    const PendDir pd = otf ? PendDir{vz0 ? nullptr : pend_y[which], (const double*)proj_x0[which], (const double*)cg_r[0],
                                     pend_acc[which] ? vp : nullptr}
                           : PendDir{nullptr, nullptr, nullptr, nullptr};
    // (rin: braw and slave_of read and b written instead of b read)
    klaunch(14,
            (4.0 * m + 24.0 + (otf ? 8.0 : 0.0) + (vdiff ? 8.0 : 0.0) - (vz0 ? 8.0 : 0.0) + (rin ? 12.0 : 0.0)) *
                (double)n,
            mdot2_kernel(m), dim3(nb), dim3(BS), (int64_t)n,
            (const ProjT*)projX[which], (int64_t)pld(which), b, (const double*)pav[which], vp,
            op.null_free, proj_part, rmd, pd, rin ? *rin : RhsIn{});
    if (!rmd.out) launch_reduce(proj_part, nb, MAXB, 2 * m + 4, false, proj_d);
    KCHK();
    if (dist()) comm->allreduce(proj_d, 2 * m + 4, false, st);
    QMat qm{};
    int kq = m;
    if (m == op.kmax) kq = proj_reseed(which, m, qm);  // full: X' = Q X, the dots follow as Q a, Q c
    hipLaunchKernelGGL(k_pcoef, dim3(1), dim3(64), 0, st, (const double*)proj_d, m, (const double*)dqm,
                       m == op.kmax ? kq : -1,
                       1.0 / (double)n_free, proj_coef);
    KCHK();
    HIPCHK(hipMemcpyAsync(h_coef + which * NCOEF, proj_coef, sizeof(double) * NCOEF, hipMemcpyDeviceToHost, st));
    // k_pcomb: X, v read; the new direction, y and x0 written (not x0 when the coming solve accumulates its
    // correction: the first update starts the accumulator, so it needs no clearing either)
    const bool acc_next = which <= 2;
    klaunch(15, (4.0 * kq + (acc_next ? 24.0 : 32.0) + (vdiff ? 8.0 : 0.0) - (vz0 ? 8.0 : 0.0)) * (double)n,
            pcomb_kernel(kq), dim3(nb), dim3(BS), (int64_t)n,
            (const ProjT*)projX[which], (int64_t)pld(which), (const double*)proj_coef, vp,
            op.null_free, projX[which] + pcol(which, kq), y, acc_next ? (double*)nullptr : proj_x0[which],
            vdiff ? pend_y[which] : (const double*)nullptr, (double*)nullptr);
    pend_vzero[which] = false;
    KCHK();
    pend_otf[which] = false;
    H.coef_m = kq;
    proj_m[which] = kq + 1;
    proj_pend[which] = false;
    return true;
  }
  // coordinates bookkeeping: the last guess's coefficients (h_coef, copied with it; read after the
  // solve's host synchronisation) give the last solution y = x0 + v in the basis,
  // [gamma_i + c_i, 1 / s], and the last guess x0, [a_i, alpha_new]
  void proj_coords(int which) {
    ProjHist& H = proj_hist[which];
    if (H.coef_m < 0) return;
    const int m = H.coef_m;
    const double* K = h_coef + which * NCOEF;  // a (m), c (m), s, mu, alpha_new
    std::vector<double> y(m + 1, 0.0);
    for (int i = 0; i < m; ++i) y[i] = (i < (int)H.gamma.size() ? H.gamma[i] : 0.0) + K[m + i];
    y[m] = K[2 * m] > 0.0 ? 1.0 / K[2 * m] : 0.0;
    H.sols.push_back(std::move(y));
    if ((int)H.sols.size() > PROJ_KEEP_MAX) H.sols.erase(H.sols.begin());
    H.gamma.assign(K, K + m);
    H.gamma.push_back(K[2 * m + 2]);
    H.coef_m = -1;
  }
  // Full basis: re-seed it with the span of the last solutions and the last guess x0 (the pending
  // direction v then completes the span of the last solution).  In an A-orthonormal basis A-inner
  // products are coordinate dot products, so a Gram-Schmidt of the coordinate rows gives the new
  // basis' coefficients Q, X' = Q X (k_reseed, one pass over X).  Two Gram-Schmidt passes:
  // successive solutions are nearly parallel, one pass leaves Q orthogonal only to eps / |residual|,
  // and a basis that is not A-orthonormal makes the projection formula wrong, not just weaker;
  // seeds within 1e-6 of the span of the earlier ones add only their coordinates' noise.  Fischer's
  // restart (drop everything) costs a run of solves of 7, 5, 4, 3 iterations where the full basis
  // gives 1-2.  Returns the new basis size (<= kmax - 1).
  int64_t n_reseed = 0;  // full bases re-seeded so far (pucfem_path_info)
  int proj_reseed(int which, int m, QMat& qm) {
    ProjHist& H = proj_hist[which];
    ++n_reseed;
    const int cap = std::min(proj_keep, m - 1);
    std::vector<std::vector<double>> seeds;
    const int nh = std::min<int>((int)H.sols.size(), cap - 1);
    for (int k = (int)H.sols.size() - nh; k < (int)H.sols.size(); ++k) seeds.push_back(H.sols[k]);
    seeds.push_back(H.gamma);
    for (auto& v : seeds) v.resize(m, 0.0);
    std::vector<std::vector<double>> Q, R(seeds.size());
    for (size_t a = 0; a < seeds.size(); ++a) {
      std::vector<double> w = seeds[a];
      const double n0 = std::sqrt(std::inner_product(w.begin(), w.end(), w.begin(), 0.0));
      R[a].assign(PROJ_KEEP_MAX, 0.0);
      for (int pass = 0; pass < 2; ++pass)
        for (size_t b2 = 0; b2 < Q.size(); ++b2) {
          const double d = std::inner_product(w.begin(), w.end(), Q[b2].begin(), 0.0);
          R[a][b2] += d;
          for (int j = 0; j < m; ++j) w[j] -= d * Q[b2][j];
        }
      const double nw = std::sqrt(std::inner_product(w.begin(), w.end(), w.begin(), 0.0));
      if (nw > 1e-6 * n0 && nw > 0.0 && (int)Q.size() < cap) {
        R[a][Q.size()] = nw;
        for (double& x : w) x /= nw;
        Q.push_back(std::move(w));
      }
    }
    const int kq = (int)Q.size();
    for (int i = 0; i < kq; ++i)
      for (int j = 0; j < m; ++j) qm.q[i][j] = Q[i][j];
    // (pageable source: the copy is staged before the call returns)
    HIPCHK(hipMemcpyAsync(dqm, &qm, sizeof(QMat), hipMemcpyHostToDevice, st));
    const i64 n = lp.n_own;
    algo_bytes += 4.0 * (double)(m + kq) * (double)n;
    hipLaunchKernelGGL(k_reseed, dim3(grid_ew(n)), dim3(BS), 0, st, n, (const ProjT*)projX[which], pld(which), m,
                       (const double*)dqm, kq,
                       projXalt[which]);
    KCHK();
    std::swap(projX[which], projXalt[which]);
    H.sols.clear();
    for (int a = 0; a + 1 < (int)seeds.size(); ++a) H.sols.emplace_back(R[a].begin(), R[a].begin() + kq);
    H.gamma.assign(R.back().begin(), R.back().begin() + kq);
    return kq;
  }
  // after a solve: the new direction v = y - x0 and A v, for the next guess.  b, r_final (optional):
  // the solve's right-hand side and final CG residual, with its initial residual r0 = b - A x0 saved
  // in pav[which]: then A v = r0 - r_final (A y = b - r_final for the first direction, whose solve
  // started from the warm start with x0 = 0) instead of an SpMV -- exact up to the CG recurrence's
  // rounding drift.
  // pfin (with r_final): also the pressure solve's finish p = y with the slaves copied from their masters
  // (k_cg_fin's work, unscaled), in the same pass
  void project_update(int which, const double* y, const double* b = nullptr, const double* r_final = nullptr,
                      double* pfin = nullptr) {
    const i64 n = lp.n_own;
    const ProjOp op = proj_op(which);
    double *v = pv[which], *av = pav[which];
    if (r_final) {  // v = y - x0 (unless the solve accumulated it) and A v = r0 - r_final in one pass
      const bool whole = proj_m[which] == 0;
      double* vout = pend_acc[which] ? nullptr : v;
      if (pfin) {
        algo_bytes += (vout ? 68.0 : 52.0) * (double)n;  // + master_of read, p written
        hipLaunchKernelGGL(k_diff2_fin, dim3(grid_ew(n)), dim3(BS), 0, st, (int64_t)n, y,
                           (const double*)proj_x0[which], vout, whole ? b : (const double*)av, r_final, av,
                           (const int32_t*)dmaster_of, pfin);
      } else {
        algo_bytes += (vout ? 48.0 : 24.0) * (double)n;
        hipLaunchKernelGGL(k_diff2, dim3(grid_ew(n)), dim3(BS), 0, st, n, y, (const double*)proj_x0[which], vout,
                           whole ? b : (const double*)av, r_final, av);
      }
      KCHK();
    } else {
      hipLaunchKernelGGL(k_diff, dim3(grid_ew(n)), dim3(BS), 0, st, n, y, proj_x0[which], v);
      KCHK();
      halo(v);
      spmv_on(st, *op.A, op.fc, op.val, v, av);
    }
    proj_pend[which] = true;
  }
  // k_div with the pressure right-hand side; max |div| into maxout (a vals slot, or scratch), sum(braw)
  // into redbuf slot 3 (pressure's sb) -- fused when enabled (returns whether it was)
  bool div_rhs(const double* ax, const double* ay, double* out, double* maxout) {
    const RedOut r = ro(maxout, CNT_DIV, 2, MAXB, 1u, redbuf + 24);
    div(ax, ay, out, true, nullptr, r);
    if (!r.out) return false;
    if (maxout != redbuf + 40) red_done(maxout, 1, true);  // (redbuf slot 5: an unrecorded maximum)
    red_done(redbuf + 24, 1, false);
    return true;
  }
  // pp: p, or with p_from_y the pressure solve's y (gathered through the merged tables and columns)
  // gate (optional): the PCG's control word -- the projection runs only if the solve has finished by then
  double grad_proj(const double* pp, int mode, const int* gate = nullptr) {
    const FaceDev fc = p_from_y ? fP.full() : fK.full();
    const DevSell& A = p_from_y ? dPm : dP;
    const double bytes = (16.0 + A.idx_bytes()) * (double)A.nnz + A.row_bytes() * (double)A.nrows + 40.0 * (double)lp.n_own;
    with_c16(A, [&](auto c16) {
      klaunch(3, bytes, k_grad_proj<decltype(c16)::value>, dim3(grid_full(fc, A)), dim3(BS), A.view(), fc,
              (const double*)dGx, (const double*)dGy, pp, (const double*)das1, prm.dt, mode, (const uint8_t*)ddir,
              (const double*)usx, (const double*)usy, ux, uy, gate);
    });
    KCHK();
    return bytes;
  }
  // small meshes: the first projection with the velocity BCs (k_grad_proj_bc; the faces are empty there)
  int32_t* dspos = nullptr;  // the projection operator's (slice, lane) position of each row
  // (the position map is built before any graph capture: an allocation inside a captured step is not allowed)
  void prep_grad_proj_bc() {
    if (!dense || !dbcsrc || dspos) return;
    const DevSell& A = p_from_y ? dPm : dP;
    const int nb = (int)std::max<i64>(1, std::min<i64>(1024, (A.nslices * 64 + BS - 1) / BS));
    dspos = dalloc<int32_t>(std::max<i64>(1, lp.n_own));
    hipLaunchKernelGGL(k_sell_pos, dim3(nb), dim3(BS), 0, st, A.view(), dspos);
    KCHK();
  }
  void grad_proj_bc(const double* pp) {
    const DevSell& A = p_from_y ? dPm : dP;
    const int nb = (int)std::max<i64>(1, std::min<i64>(1024, (A.nslices * 64 + BS - 1) / BS));
    algo_bytes += (16.0 + A.idx_bytes()) * (double)A.nnz + A.row_bytes() * (double)A.nrows + 40.0 * (double)lp.n_own;
    with_c16(A, [&](auto c16) {
      hipLaunchKernelGGL(k_grad_proj_bc<decltype(c16)::value>, dim3(nb), dim3(BS), 0, st, A.view(), (const double*)dGx,
                         (const double*)dGy, pp, (const double*)das1, prm.dt, (const double*)usx, ux,
                         (const int32_t*)dbcsrc, (const int32_t*)dbcdir, (const int32_t*)dspos, (const double*)ddval,
                         dir_ncomp);
    });
    KCHK();
  }
  // The gradient projection after a pressure solve, enqueued behind the solve's convergence reads and gated on its
  // control word: when the read finds the solve converged the GPU has been running the
  // projection during the host's round trip (the r13g trace: ~50 us idle before each k_grad_proj), and when it finds
  // it not converged the launch did nothing and the next read enqueues it again.  Single rank, multigrid path with
  // p kept in y (nothing is launched between the solve's last read and the projection there).
  struct GpGate {
    bool on = false, done = false;
    const double* pp = nullptr;
    int mode = 0;
    double bytes = 0.0;
  } gp_gate;
  // a pressure solve with the gated projection armed (disarmed if the solve throws)
  int gated_pressure(const GpGate& g, double* yst, double* pout, int which, bool sb_fused) {
    gp_gate = g;
    try {
      return pressure(yst, pout, which, sb_fused);
    } catch (...) {
      gp_gate = GpGate{};
      throw;
    }
  }
  // after the solve: whether the gated projection ran (then its bytes are counted here)
  bool gp_gate_end() {
    const bool d = gp_gate.done;
    if (d) {
      algo_bytes += gp_gate.bytes;
      cls_bytes[3] += gp_gate.bytes;
      ++cls_n[3];
    }
    gp_gate = GpGate{};
    return d;
  }
  // the PCG's control-word read (h_ctl), with the gated projection behind it
  // arm: enqueue the gated projection behind this read (pcg_mg: when the solve has reached the last solve's count, so
  // that a read unlikely to find it converged adds no launch that does nothing)
  void read_ctl(bool arm = true) {
    HIPCHK(hipMemcpyAsync(h_ctl, ctl, 6 * sizeof(int), hipMemcpyDeviceToHost, st));  // (+ the note)
    if (!gp_gate.on || !arm) {
      sync_st();
      return;
    }
    if (!ev_wait) HIPCHK(hipEventCreateWithFlags(&ev_wait, hipEventDisableTiming));
    HIPCHK(hipEventRecord(ev_wait, st));
    sl_join();  // (the dye tail reads u)
    const size_t np = timer.pend.size();
    const double b = grad_proj(gp_gate.pp, gp_gate.mode, ctl);
    const bool timed = timer.on && timer.pend.size() == np + 1;
    if (timed) timer.pend.back().keep = true;
    // its bytes are counted by the caller once the solve has returned (the solve takes back the counts of launches
    // behind its converged iteration)
    algo_bytes -= b;
    cls_bytes[3] -= b;
    --cls_n[3];
    gp_gate.bytes = b;
    wait_event(ev_wait);
    if (h_ctl[0]) {
      gp_gate.done = true;
      gp_gate.on = false;
    } else if (timed) {
      timer.pend[np].cls = -1;  // (the launch found the solve unfinished: no sample)
    }
  }

  // side stream of the overlapped dye advection (stokes_step)
  hipStream_t st_sl = nullptr;
  hipEvent_t ev_u = nullptr, ev_sl = nullptr;
  bool sl_overlap = true, sl_pending = false;
  double* part_mx = nullptr;  // k_mix2 partials (part_b belongs to the solvers of the main stream)
  double* part_fd = nullptr;  // final-divergence partials (part_d: the main stream's)
  struct StreamSwap {  // run the enclosed launches on the other stream (restored on unwind)
    hipStream_t &a, &b;
    StreamSwap(hipStream_t& x, hipStream_t& y) : a(x), b(y) { std::swap(a, b); }
    ~StreamSwap() { std::swap(a, b); }
  };
  // order the main stream after the pending dye advection
  void sl_join() {
    if (!sl_pending) return;
    HIPCHK(hipStreamWaitEvent(st, ev_sl, 0));
    sl_pending = false;
  }

  // one StokesColor / StokesFood step (StokesColor.py:537-586, StokesFood.py:441-505)
  RedOut sl_ro{};
  // The dye tail of a step (final-divergence record, semi-Lagrangian advection, mixing sums, its part of
  // the step record) on the side stream, after the main stream's event `gate`.  (Round 3 measured the
  // tail enqueued after the next step's viscous solve instead, beside the pressure solve: the time moved
  // between the streams, the step rate stayed, r8j.)
  // (round 4 measured the tail released after the next step's first viscous step and after its viscous
  // solve: neutral, r10f; it is released at the end of the step)
  hipEvent_t ev_gate = nullptr;
  struct SmallRed {  // (reset on unwind)
    bool& f;
    explicit SmallRed(bool& x) : f(x) { f = true; }
    ~SmallRed() { f = false; }
  };
  void dye_tail(double* rec) {
    HIPCHK(hipEventRecord(ev_gate, st));
    HIPCHK(hipStreamWaitEvent(st_sl, ev_gate, 0));
    {
      StreamSwap sw(st, st_sl);
      SmallRed small_red(red_small);
      const RedOut rf = ro(vals + 1, CNT_DYE_DIV, 1, MAXB, 1u);
      div(ux, uy, nullptr, false, part_fd, rf);  // (the final div field is computed when read)
      if (!rf.out) reduce_into(part_fd, div_grid(), 1, true, 1);  // max |final div|
      dye_tail_sl(rec);
    }
    HIPCHK(hipEventRecord(ev_sl, st_sl));
    sl_pending = true;
  }
  // the semi-Lagrangian part of the tail (launched on st_sl: the caller swapped the streams) and the step record
  void dye_tail_sl(double* rec) {
    const RedOut rs = ro(vals + 2, CNT_DYE_SL, 3, SLB);
    // (c and the channels, before ev_sl is recorded: sl_join also orders the next write of u after the channels' reads)
    dye_transport_step(c_new, rs);
    std::swap(c_full, c_new);
    dye_transport_reduce(rs, false);  // sum wc, sum w, not-found
    const int nbm = nb_rows(lp.n_own);
    algo_bytes += 16.0 * (double)lp.n_own;  // c, w
    const RedOut rm = ro(vals + 5, CNT_DYE_MIX, 1);
    hipLaunchKernelGGL(k_mix2, dim3(nbm), dim3(BS), 0, st, lp.r0, lp.n_own, c_full, dwmix, vals + 2, 1, 1,
                       part_mx, rm);
    KCHK();
    if (!rm.out) reduce_into(part_mx, nbm, 1, false, 5);
    hipLaunchKernelGGL(k_stats, dim3(1), dim3(64), 0, st, vals, rec, 6);
    KCHK();
  }
  // W > 1, StokesColor: the second half of a step's dye tail (dye_range_start queued the first at its end): the
  // wide halo, the semi-Lagrangian advection of the owned rows, the mixing sums and the rest of the step record.
  // It reads the step's final u and c; the next step's viscous solve writes neither, and its first write to u (the
  // gradient projection) follows in stream order.
  bool tail_pend = false;
  double* tail_rec = nullptr;
  void dye_tail_dist() {
    if (!tail_pend) return;
    tail_pend = false;
    dye_halo_exchange();
    const int nb = nb_sl(lp.n_own);
    sl_ro = ro(vals + 2, CNT_SL, 3, SLB);
    sl_launch(nb, lp.r0, lp.n_own, ux, uy, prm.dt, c_full, c_new, dwmix, nullptr, sl_ro);
    KCHK();
    // (the replica keeps its halo values; k_mix2 copies the new owned segment into it)
    if (sl_ro.out) red_done(vals + 2, 3, false);
    else reduce_into(part_sl, nb, 3, false, 2, SLB);  // sum wc, sum w, not-found
    sl_ro = RedOut{};
    const int nbm = nb_rows(lp.n_own);
    algo_bytes += 16.0 * (double)lp.n_own;
    const RedOut rm = ro(vals + 5, CNT_MIX, 1);
    hipLaunchKernelGGL(k_mix2, dim3(nbm), dim3(BS), 0, st, lp.r0, lp.n_own, (const double*)c_new, dwmix, vals + 2, 1, 1,
                       part_mx, rm, c_full);
    KCHK();
    if (rm.out) red_done(vals + 5, 1, false);
    else reduce_into(part_mx, nbm, 1, false, 5);
    hipLaunchKernelGGL(k_stats, dim3(1), dim3(64), 0, st, vals, tail_rec, 4);
    KCHK();
  }
  void stokes_step(double* rec, int32_t* its) {
    int itv = 0;
    ring_in_mix = false;
    stroke_step();   // (the step's boundary values, in front of everything that reads ddval)
    inertia_step();  // (reads u, as the previous step's dye tail on the side stream does: no join)
    force_step();    // (buoyancy reads c^n: it joins the tail)
    viscous(itv);
    dye_tail_dist();  // (W > 1: the previous step's dye tail)
    // max |div u*| -> vals[0]; the div u* field itself is computed when read (pucfem_get_field): nothing in the
    // step reads it, and its 8 B/row store is a quarter of the kernel's bytes
    const bool f1 = div_rhs(usx, usy, nullptr, vals);
    if (!f1) reduce_into(part_d, div_grid(), 1, true, 0);
    const bool gpg = use_mg && proj_k > 0 && p_from_y && !dist();
    // (a solve that throws leaves no gated projection armed for later calls: gated_pressure resets it on unwind)
    const int itp = gated_pressure(GpGate{gpg, false, yp, 0, 0.0}, yp, p, 1, f1);
    const bool gp1 = gp_gate_end();
    sl_join();  // the previous step's dye advection still reads u: it must finish before u is rewritten
    if (dense && dspos && dir_ncomp == 2 && !gp1 && (p_from_y ? fP : fK).rows == 0) {
      grad_proj_bc(p_from_y ? yp : p);  // (the BCs inside the projection: small meshes)
    } else {
      if (!gp1) grad_proj(p_from_y ? yp : p, 0);
      bc(ux, uy);
    }
    halo_v(ux);
    const bool f2 = div_rhs(ux, uy, div_u, redbuf + 40);  // (its max is not recorded: scratch slot 5)
    const int itp2 = gated_pressure(GpGate{gpg, false, yp2, 1, 0.0}, yp2, p2, 2, f2);
    const bool gp2 = gp_gate_end();
    if (!gp2) grad_proj(p_from_y ? yp2 : p2, 1);
    halo_v(ux);
    // single-rank explicit dye: the final-divergence record and the advection of this step (they read
    // the final u and c, write final_div, c_new and their own partials) run on a side stream,
    // overlapped with the next step's viscous solve and first pressure solve; the main stream waits
    // for them before its next write to u (sl_join above)
    const bool ovl = sl_overlap && scheme == PUCFEM_STOKES_COLOR && !dye_impl && !graph_mode && !dist();
    if (!ovl) {
      const RedOut r = ro(vals + 1, CNT_DIV, 1, MAXB, 1u);
      // (a captured small-mesh step with this record on a forked branch of the graph gave the same bits and ran
      // 10.0k steps/s against 12.5k in one chain, r14q)
      div(ux, uy, dye_impl ? final_div : nullptr, false, nullptr, r);  // (the implicit dye reads it)
      if (r.out) red_done(vals + 1, 1, true);
      else reduce_into(part_d, div_grid(), 1, true, 1);  // max |final div|
    }
    if (ovl) {
      if (!st_sl) {
        // (stream priorities and CU masks for the side stream were measured and changed nothing or lost,
        // rounds 2-3: r4d, r6c)
        HIPCHK(hipStreamCreateWithFlags(&st_sl, hipStreamNonBlocking));
        HIPCHK(hipEventCreateWithFlags(&ev_u, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&ev_sl, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&ev_gate, hipEventDisableTiming));
      }
      hipLaunchKernelGGL(k_stats, dim3(1), dim3(64), 0, st, vals, rec, 1);  // max |div u*|
      KCHK();
      dye_tail(rec);
    } else if (scheme == PUCFEM_STOKES_COLOR) {
      const int nb = nb_sl(lp.n_own);
      if (dye_impl) {
        last_dye_it = dye_step(ux, uy, final_div, c_full, c_new);
        hipLaunchKernelGGL(k_wsum, dim3(nb), dim3(BS), 0, st, lp.r0, lp.n_own, (const double*)c_new,
                           (const double*)dwmix, part_sl);
      } else if (dist()) {
        // W > 1: the back-traced ranges now, the rest of the tail at the next step (dye_tail_dist)
        hipLaunchKernelGGL(k_stats, dim3(1), dim3(64), 0, st, vals, rec, 3);  // max |div u*|, max |final div|
        KCHK();
        dye_range_start(uy, prm.dt);
        tail_pend = true;
        tail_rec = rec;
        its[0] = itv;
        its[1] = itp;
        its[2] = itp2;
        return;
      } else {
        if (!adv_dye && trj_dye == PUCFEM_TRJ_EULER) sl_ro = ro(vals + 2, CNT_SL, 3, SLB);
        dye_transport_step(c_new, sl_ro);
      }
      KCHK();
      // fixed buffers inside a captured graph: k_mix2 copies the new values back instead of a swap
      const bool mix_copy = graph_mode && !dye_impl;
      if (graph_mode && dye_impl) {
        HIPCHK(hipMemcpyAsync(c_full + lp.r0, c_new + lp.r0, sizeof(double) * lp.n_own, hipMemcpyDeviceToDevice, st));
      } else if (!mix_copy) {
        std::swap(c_full, c_new);
      }
      // sum wc, sum w, not-found (the implicit dye: k_wsum's partials, no fused reduction)
      if (dye_impl) reduce_into(part_sl, nb, 3, false, 2, SLB);
      else dye_transport_reduce(sl_ro, true);
      sl_ro = RedOut{};
      const int nbm = nb_rows(lp.n_own);
      algo_bytes += 16.0 * (double)lp.n_own;
      const RedOut rm = ro(vals + 5, CNT_MIX, 1);
      // (captured small-mesh step with the fused reduction: k_mix2's reducing block appends the step record)
      ring_in_mix = gcapture && rm.out && !ovl;
      hipLaunchKernelGGL(k_mix2, dim3(nbm), dim3(BS), 0, st, lp.r0, lp.n_own, mix_copy ? (const double*)c_new : c_full,
                         dwmix, vals + 2, 1, 1, part_mx, rm, mix_copy ? c_full : (double*)nullptr, (const double*)vals,
                         ring_in_mix ? gring : (double*)nullptr, ring_in_mix ? gcount : (int*)nullptr, 7);
      KCHK();
      if (rm.out) red_done(vals + 5, 1, false);
      else reduce_into(part_mx, nbm, 1, false, 5);
    } else {
      tracer_advance(prm.dt);
    }
    if (!ovl) {
      if (gcapture) {
        if (!ring_in_mix) hipLaunchKernelGGL(k_stats_ring, dim3(1), dim3(64), 0, st, vals, gring, gcount, 7);
      } else {
        hipLaunchKernelGGL(k_stats, dim3(1), dim3(64), 0, st, vals, rec, 7);
      }
      KCHK();
    }
    loads_step();  // (the record's row, from the step's final u and pressures: nothing unless the record is on)
    its[0] = itv;
    its[1] = itp;
    its[2] = itp2;
  }

  // the finest multigrid level's lmax (lmax_estimate's power iteration, on the device operator):
  // min(Gershgorin bound gersh, 1.1 x 30 steps of x <- D^-1 A x / |D^-1 A x|)
  double lmax_device(double gersh, double* lam_out) {
    const i64 n = lp.n_own;
    struct Scratch {  // setup scratch: freed on return, not kept with the context
      double* p = nullptr;
      Scratch(i64 m) { HIPCHK(hipMalloc(&p, sizeof(double) * (size_t)std::max<i64>(1, m))); }
      ~Scratch() { (void)hipFree(p); }
    } xt(nloc), yt(nloc), dt(n);
    double *x = xt.p, *y = yt.p, *dinv = dt.p;
    std::vector<double> x0;  // (global row index: a partitioned run iterates the single-rank vector)
    host_alloc_fresh(x0, n);
    parallel_for(n, [&](i64 i0, i64 i1) {
      for (i64 i = i0; i < i1; ++i) x0[i] = 1.0 + 0.5 * std::sin((double)(lp.r0 + i));
    });
    h2d(dinv, lmax_dinv.data() + lp.r0, sizeof(double) * n);
    h2d(x, x0.data(), sizeof(double) * n);
    const int nb = nb_rows(n), ge = grid_ew(n);
    double lam = 0.0;
    for (int it = 0; it < 30; ++it) {
      halo(x);
      spmv_on(st, dPp, fP.full(), dKp_raw, x, y);
      hipLaunchKernelGGL(k_vmul, dim3(ge), dim3(BS), 0, st, n, (const double*)y, dinv, y);
      hipLaunchKernelGGL(k_dot2, dim3(nb), dim3(BS), 0, st, n, (const double*)x, (const double*)x, (const double*)y,
                         (const double*)y, part_a);
      hipLaunchKernelGGL(k_reduce, dim3(2), dim3(RB), 0, st, part_a, nb, MAXB, 2, 0, redbuf);
      KCHK();
      if (dist()) comm->allreduce(redbuf, 2, false, st);
      HIPCHK(hipMemcpyAsync(h_pinned, redbuf, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      const double nx = h_pinned[0], ny = h_pinned[1];
      lam = std::sqrt(ny / nx);
      hipLaunchKernelGGL(k_axpbypcz, dim3(ge), dim3(BS), 0, st, n, (const double*)nullptr, (const double*)y,
                         (const double*)nullptr, (const double*)nullptr, (const double*)nullptr, (const double*)nullptr,
                         1.0 / std::sqrt(ny), 0.0, 0.0, x);
      KCHK();
    }
    HIPCHK(hipStreamSynchronize(st));
    lmax_dinv.clear();
    lmax_dinv.shrink_to_fit();
    *lam_out = lam;
    return std::min(gersh, 1.1 * lam);
  }

  // a coarse multigrid level's lmax: lmax_estimate's 30-step power iteration on the level's device operator
  // (its V-cycle values: fp32 in the fp32 cycle) instead of on the host, min(Gershgorin bound gersh, 1.1 lam);
  // a partitioned level exchanges its halo before each product and all-reduces the norms
  template <typename T>
  double lmax_level_device(MgLevel& L, double gersh) {
    MgBufs<T>& B = bufs<T>(L);
    const i64 n = L.lp.n_own, r0 = L.own0(rank);
    std::vector<T> x0;
    host_alloc_fresh(x0, n);
    parallel_for(n, [&](i64 i0, i64 i1) {
      for (i64 i = i0; i < i1; ++i) x0[i] = (T)(1.0 + 0.5 * std::sin((double)(r0 + i)));
    });
    h2d(B.x, x0.data(), sizeof(T) * n);
    HIPCHK(hipMemsetAsync(B.b, 0, sizeof(T) * L.nloc, st));
    HIPCHK(hipMemsetAsync(ctl, 0, 2 * sizeof(int), st));
    const FaceDev fr = L.hA.full();
    const DevSell& A = L.dA;
    const int nb = nb_rows(n), ge = grid_ew(n);
    double lam = 0.0;
    for (int it = 0; it < 30; ++it) {
      mg_halo(L, B.x);
      B.with_vals([&](auto* val) {
        using VT = std::remove_const_t<std::remove_pointer_t<decltype(val)>>;
        with_c16(A, [&](auto c16) {
          hipLaunchKernelGGL((k_resid<T, T, VT, decltype(c16)::value, 0>), dim3(grid_full(fr, A)), dim3(BS), 0, st,
                             A.view(), fr, val, (const T*)B.b, (const T*)B.x, B.res, (const int*)ctl);
        });
      });
      hipLaunchKernelGGL(k_pow_step<T>, dim3(nb), dim3(BS), 0, st, (int64_t)n, (const T*)B.x, (const T*)B.res,
                         (const T*)B.dinv, B.x2, part_a);
      hipLaunchKernelGGL(k_reduce, dim3(2), dim3(RB), 0, st, part_a, nb, MAXB, 2, 0, redbuf);
      KCHK();
      if (dist() && !L.rep) comm->allreduce(redbuf, 2, false, st);
      HIPCHK(hipMemcpyAsync(h_pinned, redbuf, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      const double nx = h_pinned[0], ny = h_pinned[1];
      lam = std::sqrt(ny / nx);
      hipLaunchKernelGGL(k_pow_scale<T>, dim3(ge), dim3(BS), 0, st, (int64_t)n, (const T*)B.x2, 1.0 / std::sqrt(ny),
                         B.x);
      KCHK();
    }
    HIPCHK(hipStreamSynchronize(st));
    L.lam_dev = lam;
    return std::min(gersh, 1.1 * lam);
  }

  // implicit dye step (good_visualization.py:700-718) from cin with velocity (vx, vy) and its lumped
  // divergence dv into cout: assemble the merged operator, rhs = M c, BiCGStab from c, periodic copies
  int dye_step(const double* vx, const double* vy, const double* dv, const double* cin, double* cout) {
    const i64 n = lp.n_own;
    hipLaunchKernelGGL(k_dye_w, dim3(grid_ew(mesh.T)), dim3(BS), 0, st, MeshDev{mx, my, mtri, mesh.T}, vx, vy, dDyeW);
    hipLaunchKernelGGL(k_dye_assemble, dim3(grid_ew(dye.nslots)), dim3(BS), 0, st, dye, (const double*)dDyeW, dv,
                       prm.dt, prm.dye_diffusivity, dDyeVal);
    hipLaunchKernelGGL(k_dye_dinv, dim3(grid_ew(n)), dim3(BS), 0, st, n, (const int64_t*)dDyeDiag,
                       (const double*)dDyeVal, dDyeDinv);
    KCHK();
    with_c16(dDye, [&](auto c16) {
      hipLaunchKernelGGL(k_spmv<decltype(c16)::value>, dim3(nb_for(dDye.nslices)), dim3(BS), 0, st, dDye.view(), nof(),
                         (const double*)dDyeM, cin, dDyeB);
    });
    KCHK();
    if (dye_nsrow > 0) {
      hipLaunchKernelGGL(k_dye_rhs_fix, dim3(std::min(256, (dye_nsrow + BS - 1) / BS)), dim3(BS), 0, st, dye_nsrow,
                         (const int32_t*)dDyeSrow, (const int64_t*)dDyeSptr, (const int32_t*)dDyeSk,
                         (const int32_t*)dDyeSc, dye, (const double*)dDyeW, dv, prm.dt, prm.dye_diffusivity, cin, dDyeB);
      KCHK();
    }
    HIPCHK(hipMemcpyAsync(cout, cin, sizeof(double) * n, hipMemcpyDeviceToDevice, st));
    const int it = bicgstab(cout, dDyeB, std::max(prm.rtol_lin, 1e-13), prm.maxit_lin, &dDye, dDyeVal, dDyeDinv);
    if (ncopy > 0) {  // c[slave] = c[master] (good_visualization.py:715-716)
      if (bc_gather) {
        hipLaunchKernelGGL(k_bc_gather, dim3(std::min(1024, (ncopy + BS - 1) / BS)), dim3(BS), 0, st, ncopy, dcsrc,
                           dbctmp, 1, cout, cout, 1);
        KCHK();
      }
      hipLaunchKernelGGL(k_bc_apply, dim3(std::min(1024, (ncopy + BS - 1) / BS)), dim3(BS), 0, st, ncopy, dcdst, dcsrc,
                         bc_gather ? (const double*)dbctmp : nullptr, 0, ddnode, ddval, 1, cout, cout, 1);
      KCHK();
    }
    return it;
  }

  void tracer_advance(double dt) {
    if (ntr == 0) {
      HIPCHK(hipMemsetAsync(vals + 6, 0, sizeof(double), st));
      return;
    }
    if (!has_tgrid) throw Error(PUCFEM_ESTATE, "tracer grid not built (scheme is not STOKES_FOOD)");
    double *fx = ux, *fy = uy;
    // TRACER_CLOUD_MIN tracers and more: one tracer per thread on a grid, the eaten count through the kernel's own
    // ticket (always fused: the count is exact in any order, and a k_reduce launch would cost more than the kernel)
    const int nbt = tracer_blocks(ntr);
    const bool cloud = nbt > 1;
    const RedOut rt{vals + 6, nullptr, dcnt + CNT_TRACER, 1, TRACER_CLOUD_MAXB, 0u};
    tr_blocks = nbt;
    tr_threads = BS;
    if (dist()) {
      // no replica of u: each rank interpolates the tracers in its own triangles from its owned and
      // ghost values (placed at their global ids), then one all-reduce of 3 x ntr values hands every
      // rank all the velocities (StokesFood's 488 tracers: ~12 KB per step instead of the whole u)
      hipLaunchKernelGGL(k_unstride, dim3(grid_ew(lp.n_own)), dim3(BS), 0, st, lp.n_own, (const double*)ux, VS,
                         ufx + lp.r0);
      hipLaunchKernelGGL(k_unstride, dim3(grid_ew(lp.n_own)), dim3(BS), 0, st, lp.n_own, (const double*)uy, VS,
                         ufy + lp.r0);
      if (lp.n_ghost > 0) {
        hipLaunchKernelGGL(k_scatter_ghosts, dim3(grid_ew(lp.n_ghost)), dim3(BS), 0, st, lp.n_ghost,
                           (const int32_t*)dghost_global, (const double*)(ux + VS * lp.n_own), ufx, VS);
        hipLaunchKernelGGL(k_scatter_ghosts, dim3(grid_ew(lp.n_ghost)), dim3(BS), 0, st, lp.n_ghost,
                           (const int32_t*)dghost_global, (const double*)(uy + VS * lp.n_own), ufy, VS);
      }
      hipLaunchKernelGGL(k_tracer_vel, dim3((ntr + BS - 1) / BS), dim3(BS), 0, st, MeshDev{mx, my, mtri, mesh.T},
                         tgrid, (const double*)ufx, (const double*)ufy, ntr, (const double*)trx, (const double*)try_,
                         (int64_t)lp.r0, (int64_t)lp.r1, trv);
      KCHK();
      comm->allreduce(trv, 3 * (size_t)ntr, false, st);
      if (cloud)
        hipLaunchKernelGGL(k_tracer_move_cloud, dim3(nbt), dim3(BS), 0, st, ntr, trx, try_, trs, trcap, trstep,
                           (const double*)trv, dt, prm.center_x, prm.center_y, prm.capture_radius, part_tr, rt);
      else
        hipLaunchKernelGGL(k_tracer_move, dim3(1), dim3(BS), 0, st, ntr, trx, try_, trs, trcap, trstep,
                           (const double*)trv, dt, prm.center_x, prm.center_y, prm.capture_radius, vals + 6);
      KCHK();
      return;
    }
    if (str_on) {  // tracer stretching: the same launch, the STRETCH instantiation of whichever kernel is due
      const MeshDev M{mx, my, mtri, mesh.T};
      const bool mid = trj_trc == PUCFEM_TRJ_MIDPOINT;
      if (mid) HIPCHK(hipMemsetAsync(trjt_fell, 0, sizeof(int32_t), st));
      const Stretch sa{str_F};
      auto go = [&](auto brown, auto midp) {
        constexpr bool B = decltype(brown)::value, MI = decltype(midp)::value;
        BrownArg<B> br{};
        if constexpr (B)
          br = Brown{std::sqrt(6.0 * tr_D * dt), (uint32_t)(tr_seed & 0xffffffffu), (uint32_t)(tr_seed >> 32), tr_ylo,
                     tr_yhi};
        TrjMidArg<MI> md{};
        if constexpr (MI) md = TrjMid{0.5 * dt, trjt_fell};
        if (cloud)
          hipLaunchKernelGGL((k_tracer_cloud<B, MI, true>), dim3(nbt), dim3(BS), 0, st, M, tgrid, fx, fy, ntr, trx,
                             try_, trs, trcap, trstep, dt, prm.center_x, prm.center_y, prm.capture_radius, part_tr, rt,
                             br, md, sa);
        else
          hipLaunchKernelGGL((k_tracer<B, MI, true>), dim3(1), dim3(BS), 0, st, M, tgrid, fx, fy, ntr, trx, try_, trs,
                             trcap, trstep, dt, prm.center_x, prm.center_y, prm.capture_radius, vals + 6, br, md, sa);
      };
      if (tr_D > 0.0) {
        if (mid) go(std::true_type{}, std::true_type{});
        else go(std::true_type{}, std::false_type{});
      } else {
        if (mid) go(std::false_type{}, std::true_type{});
        else go(std::false_type{}, std::false_type{});
      }
      KCHK();
      if (mid) {
        trjt_ran = true;
        ++trjt_steps;
      }
      ++str_steps;
      return;
    }
    if (trj_trc == PUCFEM_TRJ_MIDPOINT) {  // midpoint trajectories: the same launch, the MID instantiations
      const MeshDev M{mx, my, mtri, mesh.T};
      const TrjMid md{0.5 * dt, trjt_fell};
      HIPCHK(hipMemsetAsync(trjt_fell, 0, sizeof(int32_t), st));
      if (tr_D > 0.0) {
        const Brown br{std::sqrt(6.0 * tr_D * dt), (uint32_t)(tr_seed & 0xffffffffu), (uint32_t)(tr_seed >> 32), tr_ylo,
                       tr_yhi};
        if (cloud)
          hipLaunchKernelGGL((k_tracer_cloud<true, true>), dim3(nbt), dim3(BS), 0, st, M, tgrid, fx, fy, ntr, trx, try_,
                             trs, trcap, trstep, dt, prm.center_x, prm.center_y, prm.capture_radius, part_tr, rt, br, md);
        else
          hipLaunchKernelGGL((k_tracer<true, true>), dim3(1), dim3(BS), 0, st, M, tgrid, fx, fy, ntr, trx, try_, trs,
                             trcap, trstep, dt, prm.center_x, prm.center_y, prm.capture_radius, vals + 6, br, md);
      } else if (cloud) {
        hipLaunchKernelGGL((k_tracer_cloud<false, true>), dim3(nbt), dim3(BS), 0, st, M, tgrid, fx, fy, ntr, trx, try_,
                           trs, trcap, trstep, dt, prm.center_x, prm.center_y, prm.capture_radius, part_tr, rt,
                           BrownOff{}, md);
      } else {
        hipLaunchKernelGGL((k_tracer<false, true>), dim3(1), dim3(BS), 0, st, M, tgrid, fx, fy, ntr, trx, try_, trs,
                           trcap, trstep, dt, prm.center_x, prm.center_y, prm.capture_radius, vals + 6, BrownOff{}, md);
      }
      KCHK();
      trjt_ran = true;
      ++trjt_steps;
      return;
    }
    if (tr_D > 0.0) {  // Brownian tracers: the same launch, the BROWN instantiation
      const Brown br{std::sqrt(6.0 * tr_D * dt), (uint32_t)(tr_seed & 0xffffffffu), (uint32_t)(tr_seed >> 32), tr_ylo,
                     tr_yhi};
      if (cloud)
        hipLaunchKernelGGL(k_tracer_cloud<true>, dim3(nbt), dim3(BS), 0, st, MeshDev{mx, my, mtri, mesh.T}, tgrid, fx,
                           fy, ntr, trx, try_, trs, trcap, trstep, dt, prm.center_x, prm.center_y, prm.capture_radius,
                           part_tr, rt, br, TrjMidOff{});
      else
        hipLaunchKernelGGL(k_tracer<true>, dim3(1), dim3(BS), 0, st, MeshDev{mx, my, mtri, mesh.T}, tgrid, fx, fy, ntr,
                           trx, try_, trs, trcap, trstep, dt, prm.center_x, prm.center_y, prm.capture_radius, vals + 6,
                           br, TrjMidOff{});
      KCHK();
      return;
    }
    if (cloud)
      hipLaunchKernelGGL(k_tracer_cloud<false>, dim3(nbt), dim3(BS), 0, st, MeshDev{mx, my, mtri, mesh.T}, tgrid, fx,
                         fy, ntr, trx, try_, trs, trcap, trstep, dt, prm.center_x, prm.center_y, prm.capture_radius,
                         part_tr, rt, BrownOff{}, TrjMidOff{});
    else
      hipLaunchKernelGGL(k_tracer<false>, dim3(1), dim3(BS), 0, st, MeshDev{mx, my, mtri, mesh.T}, tgrid, fx, fy, ntr,
                         trx, try_, trs, trcap, trstep, dt, prm.center_x, prm.center_y, prm.capture_radius, vals + 6,
                         BrownOff{}, TrjMidOff{});
    KCHK();
  }
  // blocks in x of a tracer launch over n tracers: 1 = the one-block kernels, else the cloud kernels' capped grid
  static int tracer_blocks(i64 n) {
    return n < TRACER_CLOUD_MIN ? 1 : (int)std::min<i64>(TRACER_CLOUD_MAXB, (n + BS - 1) / BS);
  }
  // the small-mesh step graphs hold the tracer arrays and their count as kernel arguments: dropped when those
  // change, recaptured by the next pucfem_step
  void drop_step_graphs() {
    if (gexec) {
      (void)hipGraphExecDestroy(gexec);
      (void)hipGraphDestroy(graph);
      gexec = nullptr;
      graph = nullptr;
      graph_mode = false;
    }
    if (gexec_k) {
      (void)hipGraphExecDestroy(gexec_k);
      (void)hipGraphDestroy(graph_k);
      gexec_k = nullptr;
      graph_k = nullptr;
    }
  }

  // ------------------------------------------------------------------ literal operators (heat / Poisson)
  // Jacobi-preconditioned BiCGStab on the literal operator (heat / Poisson) or, given A / av / dinv,
  // on another fully stored SELL operator (the implicit dye system)
  int bicgstab(double* x, const double* b, double tol, int maxit, const DevSell* A = nullptr,
               const double* av = nullptr, const double* dinv_op = nullptr) {
    const i64 n = lp.n_own;
    const int nb = nb_rows(n), ge = grid_ew(n);
    double *r = litw[0], *rh = litw[1], *pp = litw[2], *v = litw[3], *s = litw[4], *t = litw[5], *ph = litw[6],
           *sh = litw[7];
    const DevSell& AA = A ? *A : dLit;
    const double* AV = A ? av : dLitv;
    const double* dlit_dinv = A ? dinv_op : this->dlit_dinv;
    auto spmv = [&](const double* in, double* out) {
      with_c16(AA, [&](auto c16) {
        hipLaunchKernelGGL(k_spmv<decltype(c16)::value>, dim3(nb_for(AA.nslices)), dim3(BS), 0, st, AA.view(), nof(),
                           AV, in, out);
      });
      KCHK();
    };
    spmv(x, t);
    hipLaunchKernelGGL(k_axpbypcz, dim3(ge), dim3(BS), 0, st, n, (const double*)nullptr, b, (const double*)nullptr,
                       (const double*)t, (const double*)nullptr, (const double*)nullptr, 1.0, -1.0, 0.0, r);
    KCHK();
    HIPCHK(hipMemcpyAsync(rh, r, sizeof(double) * n, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemsetAsync(pp, 0, sizeof(double) * n, st));
    HIPCHK(hipMemsetAsync(v, 0, sizeof(double) * n, st));
    const double init[8] = {1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    HIPCHK(hipMemcpyAsync(bicg_sc, init, sizeof(init), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_dot2, dim3(nb), dim3(BS), 0, st, n, b, b, (const double*)r, (const double*)r, part_a);
    KCHK();
    hipLaunchKernelGGL(k_reduce, dim3(2), dim3(RB), 0, st, part_a, nb, MAXB, 2, 0, bicg_sc + 8);
    KCHK();
    HIPCHK(hipMemcpyAsync(h_pinned, bicg_sc + 8, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const double bb = h_pinned[0];
    double rr = h_pinned[1];
    const double tol2 = tol * tol * bb;
    int it = 0;
    while (!(rr <= tol2)) {
      if (it >= maxit || !std::isfinite(rr)) throw Error(PUCFEM_ENOCONV, "BiCGStab did not converge");
      hipLaunchKernelGGL(k_dot2, dim3(nb), dim3(BS), 0, st, n, rh, r, (const double*)nullptr, (const double*)nullptr, part_a);
      hipLaunchKernelGGL(k_bicg_scalar, dim3(1), dim3(BS), 0, st, 0, part_a, nb, bicg_sc);
      hipLaunchKernelGGL(k_bicg_p, dim3(ge), dim3(BS), 0, st, n, r, pp, v, dlit_dinv, ph, bicg_sc);
      spmv(ph, v);
      hipLaunchKernelGGL(k_dot2, dim3(nb), dim3(BS), 0, st, n, rh, v, (const double*)nullptr, (const double*)nullptr, part_a);
      hipLaunchKernelGGL(k_bicg_scalar, dim3(1), dim3(BS), 0, st, 1, part_a, nb, bicg_sc);
      hipLaunchKernelGGL(k_bicg_s, dim3(ge), dim3(BS), 0, st, n, r, v, dlit_dinv, s, sh, bicg_sc);
      spmv(sh, t);
      hipLaunchKernelGGL(k_dot2, dim3(nb), dim3(BS), 0, st, n, t, s, (const double*)t, (const double*)t, part_a);
      hipLaunchKernelGGL(k_bicg_scalar, dim3(1), dim3(BS), 0, st, 2, part_a, nb, bicg_sc);
      hipLaunchKernelGGL(k_bicg_x, dim3(ge), dim3(BS), 0, st, n, x, ph, sh, s, t, r, bicg_sc);
      hipLaunchKernelGGL(k_dot2, dim3(nb), dim3(BS), 0, st, n, r, r, (const double*)nullptr, (const double*)nullptr, part_a);
      hipLaunchKernelGGL(k_reduce, dim3(1), dim3(RB), 0, st, part_a, nb, MAXB, 1, 0, bicg_sc + 5);
      KCHK();
      HIPCHK(hipMemcpyAsync(h_pinned, bicg_sc + 5, sizeof(double), hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      rr = h_pinned[0];
      ++it;
    }
    return it;
  }
};

Ctx* C(void* p) { return static_cast<Ctx*>(p); }

void spmv_on(hipStream_t st, const DevSell& A, const FaceDev& fc, const double* val, const double* x, double* y) {
  with_c16(A, [&](auto c16) {
    hipLaunchKernelGGL(k_spmv<decltype(c16)::value>, dim3(Ctx::grid_part(fc, A)), dim3(BS), 0, st, A.view(),
                       fc, val, x, y);
  });
}

template <class F>
int guard(void* ctx, F&& f) {
  try {
    f();
    return PUCFEM_OK;
  } catch (const Error& e) {
    (ctx ? C(ctx)->err : g_err) = e.what();
    return e.code;
  } catch (const std::bad_alloc&) {
    (ctx ? C(ctx)->err : g_err) = "out of host memory";
    return PUCFEM_ENOMEM;
  } catch (const std::exception& e) {
    (ctx ? C(ctx)->err : g_err) = e.what();
    return PUCFEM_EINVAL;
  }
}

// const char* overload first: a check inside a hot loop must not build a std::string per call
inline void require(bool ok, const char* msg) {
  if (!ok) throw Error(PUCFEM_EINVAL, msg);
}
inline void require(bool ok, const std::string& msg) {
  if (!ok) throw Error(PUCFEM_EINVAL, msg);
}

// ------------------------------------------------------------------ multigrid hierarchy (host)
// min(Gershgorin bound, 1.1 x 30-step power iteration) of D^-1 A; rows in fixed chunks (threads),
// the norms summed per chunk and then in chunk order: the same value on every machine.  power = false:
// the Gershgorin bound only, with D^-1 in *dinv_out (the finest level's power iteration then runs on
// the device, Ctx::lmax_device)
double lmax_estimate(const Csr& A, bool power = true, std::vector<double>* dinv_out = nullptr,
                     double* lam_out = nullptr) {
  const i64 n = A.nrows;
  std::vector<double> dinv(n), x(power ? n : 0), y(power ? n : 0);
  std::vector<double> cg(PAR_CHUNKS, 0.0), cx(PAR_CHUNKS), cy(PAR_CHUNKS);
  parallel_chunks(n, [&](int ch, i64 r0, i64 r1) {
    for (i64 r = r0; r < r1; ++r) {
      double d = 1.0, s = 0.0;
      for (i64 k = A.rowptr[r]; k < A.rowptr[r + 1]; ++k) {
        if (A.col[k] == r) d = A.val[k];
        s += std::fabs(A.val[k]);
      }
      dinv[r] = 1.0 / d;
      cg[ch] = std::max(cg[ch], s / d);
    }
  });
  double gersh = 0.0;
  for (double g : cg) gersh = std::max(gersh, g);
  if (!power) {
    if (dinv_out) dinv_out->swap(dinv);
    return gersh;
  }
  parallel_for(n, [&](i64 i0, i64 i1) {
    for (i64 i = i0; i < i1; ++i) x[i] = 1.0 + 0.5 * std::sin((double)i);
  });
  double lam = 0.0;
  for (int it = 0; it < 30; ++it) {
    parallel_chunks(n, [&](int ch, i64 r0, i64 r1) {
      double nx = 0.0, ny = 0.0;
      for (i64 r = r0; r < r1; ++r) {
        double a = 0.0;
        for (i64 k = A.rowptr[r]; k < A.rowptr[r + 1]; ++k) a += A.val[k] * x[A.col[k]];
        y[r] = dinv[r] * a;
        nx += x[r] * x[r];
        ny += y[r] * y[r];
      }
      cx[ch] = nx;
      cy[ch] = ny;
    });
    double nx = 0.0, ny = 0.0;
    for (int ch = 0; ch < PAR_CHUNKS; ++ch) {
      nx += cx[ch];
      ny += cy[ch];
    }
    lam = std::sqrt(ny / nx);
    const double inv = 1.0 / std::sqrt(ny);
    parallel_for(n, [&](i64 r0, i64 r1) {
      for (i64 r = r0; r < r1; ++r) x[r] = y[r] * inv;
    });
  }
  if (lam_out) *lam_out = lam;
  return std::min(gersh, 1.1 * lam);
}

// wall time per setup phase on stderr (PUCFEM_SETUP_TIMING=1)
struct SetupClock {
  bool on = std::getenv("PUCFEM_SETUP_TIMING") != nullptr;
  std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
  void mark(const char* what) {
    if (!on) return;
    const auto n = std::chrono::steady_clock::now();
    std::fprintf(stderr, "[setup] %-34s %8.3f s\n", what, std::chrono::duration<double>(n - t).count());
    t = n;
  }
};

void assemble_device(Ctx& c, const HostMesh& m, const Ordering& ord, Csr& P, Assembly& A);

// the red refinements of the hierarchy (host only: levels' meshes and their midpoint parents); build()
// runs it on a thread beside the finest level's assembly and pressure merge, which do not touch c.mg
void mg_refine(Ctx& c) {
  const int Lv = c.mg_levels;
  c.mg[0].mesh = c.coarse;
  for (int l = 1; l <= Lv; ++l) {
    HostMesh tmp;
    red_refine(c.mg[l - 1].mesh, tmp, &c.mg[l].ea, &c.mg[l].eb);
    if (l < Lv) {
      c.mg[l].mesh = std::move(tmp);
    } else {
      require(tmp.N == c.mesh.N && tmp.T == c.mesh.T && tmp.x == c.mesh.x && tmp.y == c.mesh.y &&
                  tmp.tri == c.mesh.tri,
              "the uploaded mesh is not the red refinement of the hierarchy's coarse mesh");
    }
  }
}
double diag_of(const Csr& A, const std::vector<double>& val, i64 g);
// the dense pseudo-inverse of a coarse level's merged operator, constants regularised on the free dofs
static std::vector<double> dense_coarse_inverse(const MgLevel& L0) {
  const i64 n0 = L0.mesh.N;
  require(n0 <= 8192, "multigrid coarse level too large for the dense coarse solve (<= 8192 nodes)");
  std::vector<double> D(n0 * n0, 0.0);
  const Csr& A = L0.Pp;
  double dsum = 0.0;
  i64 nf = 0;
  for (i64 r = 0; r < n0; ++r) {
    for (i64 k = A.rowptr[r]; k < A.rowptr[r + 1]; ++k) D[r * n0 + A.col[k]] += A.val[k];
    if (L0.master_of[r] < 0) {
      dsum += diag_of(A, A.val, r);
      ++nf;
    }
  }
  const double cc = dsum / (double)nf / (double)nf;
  for (i64 i = 0; i < n0; ++i)
    if (L0.master_of[i] < 0)
      for (i64 j = 0; j < n0; ++j)
        if (L0.master_of[j] < 0) D[i * n0 + j] += cc;
  require(spd_inverse(D, n0), "coarse operator is not SPD after regularisation");
  return D;
}

void build_mg_host(Ctx& c, SetupClock& clk) {  // (after mg_refine)
  const int Lv = c.mg_levels;
  for (int l = 0; l < Lv; ++l) {
    MgLevel& L = c.mg[l];
    if (c.lattice) lattice_ordering(L.mesh, c.macro, l, L.ord, L.latl);
    else make_ordering_cuts(L.mesh, c.ord.cuts, L.ord);
    Assembly A;
    if (c.dev_asm()) {
      assemble_device(c, L.mesh, L.ord, L.P, A);
    } else {
      Incidence inc;
      build_incidence(L.mesh, L.ord, inc);
      build_pattern(L.mesh, L.ord, L.P, &inc);
      assemble_stokes(L.mesh, L.ord, L.P, A, &inc);
    }
    L.pairs = level_pairs(L.mesh, 1.0, 1e-6, 1.0);
    const i64 n = L.mesh.N;
    L.dof.resize(n);
    for (i64 i = 0; i < n; ++i) L.dof[i] = (i32)i;
    L.master_of.assign(n, -1);
    L.slave_of.assign(n, -1);
    for (auto& pr : L.pairs) {
      const i32 mi = L.ord.old2new[pr.first], si = L.ord.old2new[pr.second];
      require(L.master_of[si] < 0 && L.dof[mi] == mi && L.slave_of[si] < 0, "multigrid level has chained pairs");
      L.dof[si] = mi;
      L.master_of[si] = mi;
      L.slave_of[mi] = si;
    }
    build_pressure(L.P, A.K, L.dof, L.slave_of, L.Pp);
    L.P = Csr();  // only the merged operator is needed on coarse levels
  }
  clk.mark("  mg: coarse level operators");
  MgLevel& F = c.mg[Lv];
  F.ord = c.ord;
  if (c.lattice) F.latl = std::move(c.lat_fine);
  F.dof = c.dof;
  F.master_of = c.master_of;
  // the transfers of every level (serial builders, one thread per level) and the lmax estimates (each
  // parallel inside) read only what the level operators above produced: they run concurrently
  // the finest level's power iteration runs on the device at the end of build() (every rank its strip:
  // halos before the products, the two norms all-reduced)
  c.lmax_dev = !c.host_only;
  {
    ThreadGroup g;  // joined on every exit path; a level's exception reaches the caller from join()
    for (int l = 1; l <= Lv; ++l)
      g.spawn([&c, l] {
        MgLevel& L = c.mg[l];
        const MgLevel& C = c.mg[l - 1];
        build_prolongation(C.mesh.N, L.ea, L.eb, L.ord, C.ord, C.dof, L.master_of, L.Pr);
        transpose(L.Pr, C.mesh.N, L.R);
      });
    std::exception_ptr e0;
    try {
      for (int l = 0; l <= Lv; ++l)  // (device power iterations: the Gershgorin bound here, the rest in build())
        c.mg[l].lmax = l == Lv && c.lmax_dev ? lmax_estimate(c.Pp, false, &c.lmax_dinv)
                                             : lmax_estimate(l == Lv ? c.Pp : c.mg[l].Pp, !(c.lmax_dev && l >= 1));
    } catch (...) {
      e0 = std::current_exception();
    }
    clk.mark("  mg: lmax estimates (host)");
    g.join();
    if (e0) std::rethrow_exception(e0);
  }
  clk.mark("  mg: transfers (joined)");
}

// ------------------------------------------------------------------ operator build
double diag_of(const Csr& A, const std::vector<double>& val, i64 g) {
  for (i64 k = A.rowptr[g]; k < A.rowptr[g + 1]; ++k)
    if (A.col[k] == g) return val[k];
  return 1.0;
}

// binary SELL image: int64 nslices, nrows, padded; int64 slice_off[nslices+1]; int32 slice_w[nslices];
// int32 col[padded]; double val[padded]
void dump_sell(const char* path, const Sell& S, const std::vector<double>& val) {
  FILE* f = std::fopen(path, "wb");
  require(f != nullptr, std::string("cannot write ") + path);
  const int64_t h[3] = {S.nslices, S.nrows, S.padded};
  std::fwrite(h, sizeof(h), 1, f);
  std::fwrite(S.slice_off.data(), sizeof(int64_t), S.slice_off.size(), f);
  std::fwrite(S.slice_w.data(), sizeof(int32_t), S.slice_w.size(), f);
  std::fwrite(S.col.data(), sizeof(int32_t), S.col.size(), f);
  std::fwrite(val.data(), sizeof(double), val.size(), f);
  std::fclose(f);
}

// fp16 image of operator values for the fp32 V-cycle: null when disabled (prm.mg_f32_vals 1: every
// level, 2: the finest level) or when some value is not a finite fp16 (|v| >= 65504)
_Float16* upload_f16(Ctx& c, const std::vector<double>& v, bool finest) {
  if (c.prm.mg_f32_vals == 1 || (c.prm.mg_f32_vals == 2 && finest)) return nullptr;
  std::vector<_Float16> h(v.size());
  for (size_t k = 0; k < v.size(); ++k) {
    if (!(std::fabs(v[k]) < 65504.0)) return nullptr;
    h[k] = (_Float16)v[k];
  }
  return c.upload(h);
}

template <typename T>
T* upload_as(Ctx& c, const std::vector<double>& v) {
  if constexpr (std::is_same<T, double>::value) {
    return c.upload(v);
  } else {
    std::vector<T> w(v.begin(), v.end());
    return c.upload(w);
  }
}

// ------------------------------------------------------------------ device assembly
// Scratch device buffer of one setup phase (freed on scope exit, not kept with the context).
template <class T>
struct DevTmp {
  T* p = nullptr;
  explicit DevTmp(i64 n, hipStream_t st) {
    HIPCHK(hipMalloc(&p, sizeof(T) * (size_t)std::max<i64>(1, n)));
    HIPCHK(hipMemsetAsync(p, 0, sizeof(T) * (size_t)std::max<i64>(1, n), st));
  }
  DevTmp(const std::vector<T>& v, hipStream_t st) : DevTmp((i64)v.size(), st) {
    if (!v.empty()) HIPCHK(hipMemcpyAsync(p, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice, st));
  }
  ~DevTmp() { (void)hipFree(p); }
  DevTmp(const DevTmp&) = delete;
  DevTmp& operator=(const DevTmp&) = delete;
  void get(std::vector<T>& v, i64 n, hipStream_t st) const {
    v.resize((size_t)n);
    if (n > 0) HIPCHK(hipMemcpyAsync(v.data(), p, sizeof(T) * (size_t)n, hipMemcpyDeviceToHost, st));
  }
  // through the context's pinned staging buffers (returns with the data on the host)
  void get(std::vector<T>& v, i64 n, Ctx& c) const {
    host_alloc_fresh(v, (size_t)n);
    if (n > 0) c.d2h(v.data(), p, sizeof(T) * (size_t)n);
  }
};

// The stiffness pattern P and the K / Gx / Gy / lumped-mass / area-sum values of a mesh assembled on the
// device (pucfem_kernels_impl.hpp k_inc_* / k_pat_* / k_asm): the same arrays pucfem_host.cpp's
// build_incidence + build_pattern + assemble_stokes produce, bit for bit (tests/test_gpu_assembly.py).
// Only the two prefix sums (row counts -> offsets) run on the host.
void assemble_device(Ctx& c, const HostMesh& m, const Ordering& ord, Csr& P, Assembly& A) {
  hipStream_t st = c.st;
  const i64 N = m.N, T = m.T;
  SetupClock ck;  // (PUCFEM_SETUP_TIMING: the phases inside)
  const int nb = (int)std::min<i64>(16384, std::max<i64>(1, (3 * T + BS - 1) / BS));
  const int nbr = (int)std::min<i64>(16384, std::max<i64>(1, (N + BS - 1) / BS));
  DevTmp<i32> dtri(m.tri, st), dold2new(ord.old2new, st);
  DevTmp<double> dx(m.x, st), dy(m.y, st);
  if (ck.on) {
    HIPCHK(hipStreamSynchronize(st));
    ck.mark("  asm: mesh upload");
  }
  // incidence
  DevTmp<i32> cnt(N, st);
  hipLaunchKernelGGL(k_inc_count, dim3(nb), dim3(BS), 0, st, 3 * T, (const i32*)dtri.p, (const i32*)dold2new.p, cnt.p);
  KCHK();
  std::vector<i32> hc;
  cnt.get(hc, N, st);
  HIPCHK(hipStreamSynchronize(st));
  std::vector<i64> ptr(N + 1, 0);
  for (i64 i = 0; i < N; ++i) ptr[i + 1] = ptr[i] + hc[i];
  DevTmp<i64> dptr(ptr, st);
  DevTmp<i32> cur(N, st), itri(ptr[N], st), err(1, st);
  hipLaunchKernelGGL(k_inc_fill, dim3(nb), dim3(BS), 0, st, 3 * T, (const i32*)dtri.p, (const i32*)dold2new.p,
                     (const i64*)dptr.p, cur.p, itri.p);
  KCHK();
  hipLaunchKernelGGL(k_inc_sort, dim3(nbr), dim3(BS), 0, st, N, (const i64*)dptr.p, itri.p, err.p);
  KCHK();
  // pattern
  hipLaunchKernelGGL(k_pat_count, dim3(nbr), dim3(BS), 0, st, N, (const i64*)dptr.p, (const i32*)itri.p,
                     (const i32*)dtri.p, (const i32*)dold2new.p, cnt.p);
  KCHK();
  int herr = 0;
  HIPCHK(hipMemcpyAsync(&herr, err.p, sizeof(int), hipMemcpyDeviceToHost, st));
  cnt.get(hc, N, st);
  HIPCHK(hipStreamSynchronize(st));
  require(herr == 0, "device assembly: a node has more than 32 incident triangles (use assembly = 1)");
  P.nrows = N;
  P.rowptr.assign(N + 1, 0);
  for (i64 i = 0; i < N; ++i) P.rowptr[i + 1] = P.rowptr[i] + hc[i];
  const i64 nnz = P.rowptr[N];
  DevTmp<i64> drow(P.rowptr, st);
  DevTmp<i32> dcol(nnz, st);
  hipLaunchKernelGGL(k_pat_fill, dim3(nbr), dim3(BS), 0, st, N, (const i64*)dptr.p, (const i32*)itri.p,
                     (const i32*)dtri.p, (const i32*)dold2new.p, (const i64*)drow.p, dcol.p);
  KCHK();
  // values
  DevTmp<double> K(nnz, st), Gx(nnz, st), Gy(nnz, st), M(N, st), as(N, st);
  hipLaunchKernelGGL(k_asm, dim3(nbr), dim3(BS), 0, st, N, (const i64*)dptr.p, (const i32*)itri.p, (const i32*)dtri.p,
                     (const i32*)dold2new.p, (const double*)dx.p, (const double*)dy.p, (const i64*)drow.p,
                     (const i32*)dcol.p, K.p, Gx.p, Gy.p, M.p, as.p);
  KCHK();
  if (ck.on) {
    HIPCHK(hipStreamSynchronize(st));
    ck.mark("  asm: incidence, pattern, values (device)");
  }
  dcol.get(P.col, nnz, c);
  P.val.clear();
  K.get(A.K, nnz, c);
  Gx.get(A.Gx, nnz, c);
  Gy.get(A.Gy, nnz, c);
  M.get(A.M, N, c);
  as.get(A.asum, N, c);
  HIPCHK(hipStreamSynchronize(st));
  ck.mark("  asm: downloads");
}

// device values and work vectors of every multigrid level in the V-cycle's type T.
// kp_vals: the finest operator's SELL values (fp64, = dKp_raw), reused for fp64 cycles.
template <typename T>
void mg_alloc(Ctx& c, const std::vector<double>& kp_vals) {
  const int Lv = c.mg_levels;
  std::vector<double> tmp;
  for (int l = 0; l <= Lv; ++l) {
    MgLevel& L = c.mg[l];
    MgBufs<T>& B = bufs<T>(L);
    const Csr& A = l == Lv ? c.Pp : L.Pp;
    const i64 n = L.lp.n_own;
    L.nloc = n + L.lp.n_ghost;
    // 1 / diag on owned AND ghost rows (the fused first smoothing step evaluates x1 = c Dinv b at
    // gathered columns)
    std::vector<double> dv(L.nloc);
    const i64 r0 = L.own0(c.rank);
    parallel_for(n, [&](i64 i0, i64 i1) {
      for (i64 i = i0; i < i1; ++i) dv[i] = 1.0 / diag_of(A, A.val, r0 + i);
    });
    for (i64 k = 0; k < L.lp.n_ghost; ++k) dv[n + k] = 1.0 / diag_of(A, A.val, L.lp.ghost_global[k]);
    if (L.deep && c.lattice && L.latl.F > 0 && !L.flook.starts.empty()) {
      // deep halos: every face-interior row's 1 / diag is its face record's (the face kernels' value), so the ghost
      // rows' steps repeat the owners' arithmetic (face_ghost_rows)
      for (size_t q = 0; q < L.lf_faces.size(); ++q) {
        const double di = L.lf_coef[q * lat::NCOEF + lat::C_DINV];
        const i64 b0 = L.latl.face_start[L.lf_faces[q]] - r0;
        for (i64 t = 0; t < L.latl.F; ++t) dv[b0 + t] = di;
      }
      for (i64 k = 0; k < L.lp.n_ghost; ++k) {
        const i32 g = L.lp.ghost_global[k];
        if (L.latl.type[g] == 0) dv[n + k] = face_dinv(c.macro, L.latl, L.flook, l, g);
      }
    }
    B.dinv = upload_as<T>(c, dv);
    if (l < Lv) {
      const Sell& S = L.sA;
      sell_values_x(A, r0, S, A.val, tmp);
      L.dA = DevSell{c.upload(S.slice_off), c.upload(S.slice_w), c.upload(S.col), nullptr, S.nslices, S.nrows,
                     S.rows.empty() ? A.rowptr[r0 + n] - A.rowptr[r0] : S.nnz, S.padded, 0};
      if (!S.rows.empty()) L.dA.rows = c.upload(S.rows);
      L.dA.n_own = n;
      L.dA.ghost_slices(S);
      c.attach_c16(S, L.nloc, L.dA);
      B.Aval = upload_as<T>(c, tmp);
      if constexpr (std::is_same<T, float>::value) B.Aval16 = upload_f16(c, tmp, false);
      L.nsend = (i64)L.lp.send_local.size();
      L.dsend = c.upload(L.lp.send_local);
      B.sendbuf = c.dalloc<T>(std::max<i64>(1, 2 * L.nsend));  // (two vectors per exchange: x and d)
    } else {
      if constexpr (std::is_same<T, double>::value) {
        B.Aval = c.dKp_raw;
      } else {
        B.Aval = upload_as<T>(c, kp_vals);
        B.Aval16 = upload_f16(c, kp_vals, true);
      }
      B.sendbuf = c.dalloc<T>(std::max<i64>(1, 2 * (i64)c.lp.send_local.size()));
    }
    if (l >= 1) {
      const Sell& S = L.sPr;
      sell_values_x(L.Pr, r0, S, L.Pr.val, tmp);
      L.dPr = DevSell{c.upload(S.slice_off), c.upload(S.slice_w), c.upload(S.col), nullptr, S.nslices, S.nrows,
                      S.rows.empty() ? L.Pr.rowptr[r0 + n] - L.Pr.rowptr[r0] : S.nnz, S.padded};
      if (!S.rows.empty()) L.dPr.rows = c.upload(S.rows);
      L.dPr.n_own = n;
      L.dPr.ghost_slices(S);
      B.Prval = upload_as<T>(c, tmp);
      const Sell& R = L.sR;
      sell_values_x(L.R, L.r_r0, R, L.R.val, tmp);
      L.dR = DevSell{c.upload(R.slice_off), c.upload(R.slice_w), c.upload(R.col), nullptr, R.nslices, R.nrows,
                     R.rows.empty() ? L.R.rowptr[L.r_r0 + R.nrows] - L.R.rowptr[L.r_r0] : R.nnz, R.padded};
      if (!R.rows.empty()) L.dR.rows = c.upload(R.rows);
      B.Rval = upload_as<T>(c, tmp);
    }
    for (T** f : {&B.x, &B.x2, &B.b, &B.d, &B.res}) *f = c.dalloc<T>(L.nloc);
  }
}


// Host half of the semi-Lagrangian / replica setup (build): node and triangle tables in internal
// numbering, the centroid grid, the lattice locator's tables, the initial dye.  It reads only the mesh,
// the ordering, the macro mesh and the finest lattice level, which nothing writes after the multigrid
// hierarchy exists, so build() runs it on a thread beside the operator uploads and SELL fills
// (round 4: ~1.3 s of L7 setup off the critical path); the uploads and kernels stay on the caller.
struct SlPrep {
  std::vector<double> X, Y, cx, cy, xy, c0;
  std::vector<i32> tri, home;
  Grid G, TG, MG;
  std::vector<lat::SlFace> sf;
  std::vector<uint32_t> cells;
  bool lat_sl = false;
};
void sl_prep(const Ctx& c, bool food, SlPrep& P) {
  SetupClock ck;  // (its own thread: the marks interleave with build()'s)
  const HostMesh& m = c.mesh;
  const i64 N = m.N;
  host_alloc_fresh(P.X, N);
  host_alloc_fresh(P.Y, N);
  parallel_for(N, [&](i64 g0, i64 g1) {
    for (i64 g = g0; g < g1; ++g) {
      P.X[g] = m.x[c.ord.new2old[g]];
      P.Y[g] = m.y[c.ord.new2old[g]];
    }
  });
  host_alloc_fresh(P.tri, 3 * m.T);
  parallel_for(3 * m.T, [&](i64 k0, i64 k1) {
    for (i64 k = k0; k < k1; ++k) P.tri[k] = c.ord.old2new[m.tri[k]];
  });
  // PointLocator centroids (StokesColor.py:321): (x1 + x2 + x3) / 3
  host_alloc_fresh(P.cx, m.T);
  host_alloc_fresh(P.cy, m.T);
  parallel_for(m.T, [&](i64 t0, i64 t1) {
    for (i64 t = t0; t < t1; ++t) {
      const i32 a = m.tri[3 * t], b = m.tri[3 * t + 1], d = m.tri[3 * t + 2];
      P.cx[t] = (m.x[a] + m.x[b] + m.x[d]) / 3;
      P.cy[t] = (m.y[a] + m.y[b] + m.y[d]) / 3;
    }
  });
  ck.mark("  sl: node / triangle tables, centroids");
  build_centroid_grid(P.cx, P.cy, 2.0, P.G);
  ck.mark("  sl: centroid grid");
  if (food) build_tri_grid(P.X, P.Y, P.tri, 4.0, P.TG);  // tracer location (StokesFood only)
  host_alloc_fresh(P.xy, 2 * (size_t)N);
  parallel_for(N, [&](i64 i0, i64 i1) {
    for (i64 i = i0; i < i1; ++i) {
      P.xy[2 * i] = P.X[i];
      P.xy[2 * i + 1] = P.Y[i];
    }
  });
  // semi-Lagrangian point location: on a lattice hierarchy the lattice locator (no per-triangle
  // records); PUCFEM_SL_RECORDS=1 forces the record locator (measurement / cross-check knob)
  P.lat_sl = c.lattice && !c.mg.empty() && !(std::getenv("PUCFEM_SL_RECORDS") && std::atoi(std::getenv("PUCFEM_SL_RECORDS")));
  if (P.lat_sl) {
    try {
      lattice_locator(c.macro, c.mg.back().latl, m, c.ord, P.sf, P.cells);
    } catch (const std::exception&) {
      P.lat_sl = false;  // a hierarchy not numbered face by face: the record locator
    }
  }
  ck.mark("  sl: xy, lattice locator");
  if (P.lat_sl) {
    build_tri_grid(c.macro.x, c.macro.y, c.macro.tri, 0.25, P.MG, 1e-6);
    // home faces: the macro face of every face-interior row (the first face tried)
    const LatticeLevel& LL = c.mg.back().latl;
    host_alloc_fresh(P.home, N);
    std::fill(P.home.begin(), P.home.end(), -1);
    parallel_for(c.macro.nf, [&](i64 f0, i64 f1) {
      for (i64 f = f0; f < f1; ++f)
        for (i64 k = 0; k < LL.F; ++k) P.home[LL.face_start[f] + k] = (i32)f;
    }, 1);
  }
  // initial dye c = 1[x < 0.5] (StokesColor.py:493-495)
  host_alloc_fresh(P.c0, N);
  parallel_for(N, [&](i64 g0, i64 g1) {
    for (i64 g = g0; g < g1; ++g) P.c0[g] = m.x[c.ord.new2old[g]] < 0.5 ? 1.0 : 0.0;
  });
  ck.mark("  sl: home faces, initial dye");
}

// Deep halos: a ghost row one layer out that is a macro-face interior node goes into the SELL as its face stencil --
// the node, then its six neighbours in lat::neighbours' order (the merged table's: slave columns are their masters),
// with the face record's coefficients -- so that a launch computing it does the owner's face-kernel arithmetic bit
// for bit (the stored row would sum the same terms in column order, and the assembled values agree with the
// records only to rounding); its 1 / diag is the record's too (face_dinv, mg_alloc).  This is what lets a rank use
// the ghost rows' results in place of exchanged values where the outer PCG needs one vector (z).
void build(Ctx& c) {
  SetupClock clk;
  require(c.has_mesh, "mesh not uploaded");
  const pucfem_params& prm = c.prm;
  c.scheme = prm.scheme;
  require(prm.scheme >= 0 && prm.scheme <= 3, "bad scheme");
  const bool stokes = prm.scheme == PUCFEM_STOKES_COLOR || prm.scheme == PUCFEM_STOKES_FOOD;
  const bool literal = !stokes;
  require(!(literal && c.dist()), "heat / Poisson literal operators run on one rank");
  require(!stokes || prm.sl_k == KNN, "sl_k must be 10 (PointLocator.find default)");
  HostMesh& m = c.mesh;
  // PUCFEM_PLAN_EMULATE="rank,world" (diagnostic, host-only contexts): build rank `rank`'s plans and deep-halo
  // flags of a `world`-rank run on the host (no communicator: nothing steps); with PUCFEM_DEEP_REPORT=1 the flags'
  // checks are reported
  if (const char* e = std::getenv("PUCFEM_PLAN_EMULATE")) {
    if (c.host_only && !c.dist()) {
      int r = 0, w = 1;
      if (std::sscanf(e, "%d,%d", &r, &w) == 2 && w > 1 && r >= 0 && r < w) {
        c.rank = r;
        c.world = w;
      }
    }
  }
  // lattice operators: a multigrid hierarchy of >= 2 red refinements (face interiors exist)
  c.lattice = stokes && prm.precond == 1 && c.mg_levels >= 2 && prm.assembled == 0;
  c.dye_impl = prm.scheme == PUCFEM_STOKES_COLOR && prm.dye_scheme == 1;
  require(prm.dye_scheme == 0 || prm.dye_scheme == 1, "dye_scheme must be 0 (semi-Lagrangian) or 1 (implicit)");
  require(!c.dye_impl || !c.dist(), "the implicit dye variant runs on one rank");
  if (c.lattice) {
    build_macro(c.coarse, prm.nstrips, c.mg_levels, c.macro);
    lattice_ordering(m, c.macro, c.mg_levels, c.ord, c.lat_fine);
  } else {
    make_ordering(m, prm.nstrips, c.ord);
  }
  clk.mark("ordering");
  // the multigrid hierarchy's refinements on a thread beside the finest assembly and pressure merge
  ThreadGroup refg;
  if (stokes && prm.precond == 1 && c.mg_levels > 0) {
    c.mg.clear();
    c.mg.resize(c.mg_levels + 1);
    refg.spawn([&c] { mg_refine(c); });
  }
  if (c.dev_asm()) {
    assemble_device(c, m, c.ord, c.P, c.as);
    clk.mark("pattern + assembly (device)");
  } else {
    Incidence inc;
    build_incidence(m, c.ord, inc);
    build_pattern(m, c.ord, c.P, &inc);
    clk.mark("pattern");
    assemble_stokes(m, c.ord, c.P, c.as, &inc);
  }
  const i64 N = m.N;

  // periodic pressure merge maps (internal numbering)
  c.dof.resize(N);
  for (i64 i = 0; i < N; ++i) c.dof[i] = (i32)i;
  c.slave_of.assign(N, -1);
  c.master_of.assign(N, -1);
  if (stokes) {
    for (auto& pr : c.op_pairs) {
      const i32 mi = c.ord.old2new[pr.first], si = c.ord.old2new[pr.second];
      require(c.master_of[si] < 0, "duplicate periodic slave: the pressure restatement needs unique slaves");
      require(c.dof[mi] == mi && c.slave_of[si] < 0, "chained periodic pairs are not supported for Stokes");
      c.dof[si] = mi;
      c.master_of[si] = mi;
      c.slave_of[mi] = si;
    }
    c.n_free = N - (i64)c.op_pairs.size();
    build_pressure(c.P, c.as.K, c.dof, c.slave_of, c.Pp);
    if (c.dye_impl) build_dye(m, c.ord, c.P, c.Pp, c.dof, c.dyeop);
  }
  c.use_mg = stokes && prm.precond == 1 && c.mg_levels > 0;
  clk.mark("assembly + pressure merge");
  refg.join();
  clk.mark("  mg: refinements (joined)");
  if (c.use_mg) build_mg_host(c, clk);
  if (literal) {
    assemble_literal(m, c.ord, c.g_tri, c.op_pairs, c.dir_nodes, c.dir_vals,
                     prm.scheme == PUCFEM_HEAT ? prm.dt : -1.0, c.Lit, c.litb);
  }
  clk.mark("multigrid hierarchy (host)");
  // the semi-Lagrangian tables' host half, beside everything up to the SL uploads below
  SlPrep slp;
  ThreadGroup slg;
  if (stokes) slg.spawn([&c, &slp, &prm] { sl_prep(c, prm.scheme == PUCFEM_STOKES_FOOD, slp); });
  // A_visc on P (StokesColor.py:471-475)
  std::vector<uint8_t> isdir(N, 0);
  for (i32 d : c.dir_nodes) isdir[c.ord.old2new[d]] = 1;
  const double dtnu = prm.dt * prm.nu;
  host_alloc_fresh(c.Kv, c.P.nnz());
  parallel_for(N, [&](i64 r0, i64 r1) {
    for (i64 r = r0; r < r1; ++r)
      for (i64 k = c.P.rowptr[r]; k < c.P.rowptr[r + 1]; ++k) {
        const i32 j = c.P.col[k];
        if (isdir[r]) c.Kv[k] = (j == r) ? 1.0 : 0.0;
        else if (isdir[j]) c.Kv[k] = 0.0;
        else c.Kv[k] = (j == r) ? 1.0 + dtnu * c.as.K[k] : dtnu * c.as.K[k];
      }
  });
  if (stokes) {  // spectral interval of the Jacobi-scaled A_visc (Ctx::visc_R, Ctx::visc_lo)
    std::vector<double> dg;
    host_alloc_fresh(dg, N);
    parallel_for(N, [&](i64 r0, i64 r1) {
      for (i64 r = r0; r < r1; ++r) dg[r] = diag_of(c.P, c.Kv, r);
    });
    std::vector<double> cr(PAR_CHUNKS, 0.0), cd(PAR_CHUNKS, 0.0);
    parallel_chunks(N, [&](int ch, i64 r0, i64 r1) {
      double R = 0.0, dmax = 0.0;
      for (i64 r = r0; r < r1; ++r) {
        double sr = 0.0;
        for (i64 k = c.P.rowptr[r]; k < c.P.rowptr[r + 1]; ++k)
          if (c.P.col[k] != r) sr += std::fabs(c.Kv[k]) / std::sqrt(dg[r] * dg[c.P.col[k]]);
        R = std::max(R, sr);
        dmax = std::max(dmax, dg[r]);
      }
      cr[ch] = R;
      cd[ch] = dmax;
    });
    c.visc_R = *std::max_element(cr.begin(), cr.end());
    // A_visc = I + DT nu K on the free rows (K PSD), identity on the Dirichlet rows: its eigenvalues are
    // >= 1, so the scaled x^T S A S x >= |S x|^2 >= |x|^2 / max_i a_ii (a rigorous lower end, tighter
    // than Gershgorin's 1 - R)
    c.visc_lo = std::max(1.0 - c.visc_R, 1.0 / *std::max_element(cd.begin(), cd.end()));
    if (const char* e = std::getenv("PUCFEM_VISC_SOLVER")) c.visc_solver = std::atoi(e);  // 1: CG (measurement)
    // test knob: a deliberately wrong (too short) interval [visc_lo, 1 + s R], for the post-check's test
    if (const char* e = std::getenv("PUCFEM_VISC_R_SCALE")) c.visc_R *= std::atof(e);
  }
  clk.mark("A_visc");
  // partition + local plan
  if (stokes) partition_rows(c.P, c.ord, c.world, c.row_start);
  else c.row_start = {0, N};
  std::vector<const Csr*> pats;
  if (stokes) pats = {&c.P, &c.Pp};
  else pats = {&c.P, &c.Lit};
  if (!c.use_mg) {
    make_local_plan(pats, c.row_start, c.rank, c.lp);
  } else {
    // every level cut at the same strips (y-cuts) as the finest partition
    const int Lv = c.mg_levels;
    std::vector<i64> cut(c.world + 1);
    for (int r = 0; r <= c.world; ++r)
      cut[r] = std::lower_bound(c.ord.strip_ptr.begin(), c.ord.strip_ptr.end(), c.row_start[r]) - c.ord.strip_ptr.begin();
    for (int l = 0; l <= Lv; ++l) {
      MgLevel& L = c.mg[l];
      L.rs.resize(c.world + 1);
      for (int r = 0; r <= c.world; ++r) L.rs[r] = L.ord.strip_ptr[cut[r]];
    }
    // replicated coarse levels (multi-rank): level 0 always, then every level up to mg_rep_nodes
    // default 1M: at L7 L5 (894k) and below are replicated.  Counted at W = 8 (tools/comm_probe.py, r8n):
    // grouped exchanges per PCG iteration 25 -> 17, per step 264-385 -> 184-265, for each rank smoothing
    // the whole L5 (latency-bound launches either way: ~11 against ~6 us)
    const i64 rep_max = prm.mg_rep_nodes > 0 ? prm.mg_rep_nodes : 1000000;
    for (int l = 0; l < Lv; ++l) c.mg[l].rep = c.dist() && (l == 0 || c.mg[l].mesh.N <= rep_max);
    for (int l = 1; l < Lv; ++l) c.mg[l].rep = c.mg[l].rep && c.mg[l - 1].rep;
    for (int l = 0; l <= Lv; ++l) {
      MgLevel& L = c.mg[l];
      if (L.rep) {  // the whole level on every rank: a single-rank plan (no ghosts)
        const std::vector<i64> full = {0, (i64)L.mesh.N};
        make_local_plan2({{&L.Pp, &full}}, full, 0, L.lp);
        continue;
      }
      std::vector<PatRows> pr;
      pr.push_back({l == Lv ? &c.Pp : &L.Pp, &L.rs});
      if (l >= 1) pr.push_back({&L.R, &c.mg[l - 1].rs});
      if (l < Lv) pr.push_back({&c.mg[l + 1].Pr, &c.mg[l + 1].rs});
      if (l == Lv) pr.push_back({&c.P, &L.rs});
      // deep halos on the partitioned lattice levels (Ctx::deep_halo): the ghost rows one layer out of the level
      // operator (the finest level: of the pressure and the K / A_visc patterns) and their columns
      std::vector<const Csr*> deep;
      if (c.deep_halo && c.lattice && c.world > 1) {
        deep.push_back(l == Lv ? &c.Pp : &L.Pp);
        if (l == Lv) deep.push_back(&c.P);
      }
      make_local_plan2(pr, L.rs, c.rank, L.lp, deep.empty() ? nullptr : &deep, deep.empty() ? nullptr : &L.g1);
      L.deep = !deep.empty();
    }
    c.lp = c.mg[Lv].lp;
    // lattice operators: SELL rows for the skeleton (macro edge / vertex nodes) only
    auto skel = [&](const LatticeLevel& LL, i64 r0, i64 n) {
      std::vector<i32> rows;
      for (i64 i = 0; i < n; ++i)
        if (LL.type[r0 + i] != 0) rows.push_back((i32)i);
      return rows;
    };
    for (int l = 0; l <= Lv; ++l) {  // host SELL images; resolving every column validates the plans
      MgLevel& L = c.mg[l];
      const i64 o0 = L.own0(c.rank);
      if (l < Lv) {
        if (c.lattice) build_sell_rows(L.Pp, o0, skel(L.latl, o0, L.lp.n_own), L.lp, L.sA);
        else build_sell_x(L.Pp, o0, L.lp.n_own, L.lp, L.sA, true);
        if (L.deep) {
          L.flook.init(c.macro, L.latl);
          const GhostRowFn fn = face_ghost_rows(c.macro, L.latl, L.flook, &L.dof, l, prm.dt * prm.nu);
          sell_append_ghost_rows(L.Pp, L.g1, L.lp, L.sA, nullptr, c.lattice ? &fn : nullptr);
        }
      }
      if (l >= 1) {
        const MgLevel& C = c.mg[l - 1];
        if (c.lattice) build_sell_rows(L.Pr, o0, skel(L.latl, o0, L.lp.n_own), C.lp, L.sPr);
        else build_sell_x(L.Pr, o0, L.lp.n_own, C.lp, L.sPr);
        // restriction rows: the coarse level's owned rows; into a replicated level from a
        // distributed one, this rank's strip rows of it (completed by the all-gather)
        const bool gather = C.rep && !L.rep;
        L.r_r0 = gather ? C.rs[c.rank] : C.own0(c.rank);
        const i64 nr = gather ? C.rs[c.rank + 1] - C.rs[c.rank] : C.lp.n_own;
        if (c.lattice) build_sell_rows(L.R, L.r_r0, skel(C.latl, L.r_r0, nr), L.lp, L.sR);
        else build_sell_x(L.R, L.r_r0, nr, L.lp, L.sR);
      }
    }
    // deep halos: which consumers can read the ghost rows one layer out instead of an exchange (every column
    // they gather outside the rank's rows must be one of them); all-reduced over the ranks at the upload
    for (int l = 1; l <= Lv; ++l) {
      MgLevel& L = c.mg[l];
      MgLevel& C = c.mg[l - 1];
      if (!L.deep) continue;
      const i64 lo = L.own0(c.rank), hi = lo + L.lp.n_own;
      auto in_g1 = [](const std::vector<i32>& g1, i32 g) { return std::binary_search(g1.begin(), g1.end(), g); };
      // the restriction's rows (on level l - 1) gather this level's residual
      const bool gather = C.rep && !L.rep;
      const i64 nr = gather ? C.rs[c.rank + 1] - C.rs[c.rank] : C.lp.n_own;
      bool ok = true;
      for (i64 r = L.r_r0; r < L.r_r0 + nr && ok; ++r)
        for (i64 k = L.R.rowptr[r]; k < L.R.rowptr[r + 1]; ++k) {
          const i32 j = L.R.col[k];
          if ((j < lo || j >= hi) && !in_g1(L.g1, j)) {
            ok = false;
            break;
          }
        }
      L.res_deep = ok;
      // the prolongation into this level gathers level l - 1's result: its ghosts one layer out suffice
      ok = C.deep && !C.rep;
      const i64 clo = C.own0(c.rank), chi = clo + C.lp.n_own;
      for (i64 r = lo; r < hi && ok; ++r)
        for (i64 k = L.Pr.rowptr[r]; k < L.Pr.rowptr[r + 1]; ++k) {
          const i32 j = L.Pr.col[k];
          if ((j < clo || j >= chi) && !in_g1(C.g1, j)) {
            ok = false;
            break;
          }
        }
      L.xc_deep = ok;
      // ... and on this level's ghost rows too (pr_deep): their coarse columns in level l - 1's own + G1 rows, or
      // any, from a replicated level l - 1 (whose every value every rank holds)
      ok = L.xc_deep || C.rep;
      for (size_t k = 0; k < L.lp.ghost_global.size() && ok; ++k) {
        const i32 r = L.lp.ghost_global[k];
        for (i64 e = L.Pr.rowptr[r]; e < L.Pr.rowptr[r + 1]; ++e) {
          const i32 j = L.Pr.col[e];
          if (!C.rep && (j < clo || j >= chi) && !in_g1(C.g1, j)) {
            ok = false;
            break;
          }
        }
      }
      L.pr_deep = ok;
      if (std::getenv("PUCFEM_DEEP_REPORT") && c.rank == 0) {  // (diagnostic: which rows fail the prolongation check)
        i64 bad_rows = 0, bad_g1 = 0;
        i32 ex = -1, exc = -1;
        for (const i32 r : L.lp.ghost_global) {
          bool bad = false;
          for (i64 e = L.Pr.rowptr[r]; e < L.Pr.rowptr[r + 1]; ++e) {
            const i32 j = L.Pr.col[e];
            if (!C.rep && (j < clo || j >= chi) && !in_g1(C.g1, j)) {
              bad = true;
              exc = j;
            }
          }
          if (bad) {
            ++bad_rows;
            bad_g1 += in_g1(L.g1, r) ? 1 : 0;
            ex = r;
          }
        }
        std::fprintf(stderr, "[deep] level %d: res %d xc %d pr %d; ghost rows failing the prolongation check %lld "
                     "(%lld of them G1), e.g. row %d (type %d) -> coarse %d (type %d)\n", l, (int)L.res_deep,
                     (int)L.xc_deep, (int)L.pr_deep, (long long)bad_rows, (long long)bad_g1, ex,
                     ex >= 0 ? (int)L.latl.type[ex] : -1, exc, exc >= 0 ? (int)C.latl.type[exc] : -1);
      }
      if (L.pr_deep)  // the prolongation's SELL: + every ghost row of this level (rows in this level's plan)
        sell_append_ghost_rows(L.Pr, L.lp.ghost_global, C.lp, L.sPr, &L.lp);
    }
    if (c.lattice) {  // face tables and coefficient records of every level (pucfem_lattice.hpp)
      const double dtnu = prm.dt * prm.nu;
      for (int l = 0; l <= Lv; ++l) {
        MgLevel& L = c.mg[l];
        const i64 o0 = L.own0(c.rank);
        L.lf_faces = lattice_faces(c.macro, L.latl, o0, L.lp.n_own);
        lattice_tabs(c.macro, L.latl, L.lf_faces, -1, L.lp, nullptr, L.lf_plain);
        lattice_tabs(c.macro, L.latl, L.lf_faces, -1, L.lp, &L.dof, L.lf_merged);
        lattice_coefs(c.macro, L.lf_faces, l, dtnu, L.lf_coef);
        if (l >= 1) {
          MgLevel& C = c.mg[l - 1];
          lattice_tabs(c.macro, C.latl, L.lf_faces, -1, C.lp, &C.dof, L.pr_tab2);
          const bool gather = C.rep && !L.rep;
          const i64 nr = gather ? C.rs[c.rank + 1] - C.rs[c.rank] : C.lp.n_own;
          L.r_faces = lattice_faces(c.macro, C.latl, L.r_r0, nr);
          lattice_tabs(c.macro, C.latl, L.r_faces, L.r_r0, C.lp, nullptr, L.r_tab);
          lattice_tabs(c.macro, L.latl, L.r_faces, -1, L.lp, nullptr, L.r_tab2);
        }
      }
    }
  }
  if (stokes && c.dist()) {  // wide-halo tables of the dye replica (Ctx::dye_halo)
    const i64 S = (i64)c.ord.strip_ptr.size() - 1;
    c.strip_ylo.assign(S, INFINITY);
    c.strip_yhi.assign(S, -INFINITY);
    for (i64 s = 0; s < S; ++s)
      for (i64 g = c.ord.strip_ptr[s]; g < c.ord.strip_ptr[s + 1]; ++g) {
        const double y = m.y[c.ord.new2old[g]];
        c.strip_ylo[s] = std::min(c.strip_ylo[s], y);
        c.strip_yhi[s] = std::max(c.strip_yhi[s], y);
      }
    c.rank_ylo.assign(c.world, INFINITY);
    c.rank_yhi.assign(c.world, -INFINITY);
    for (int r = 0; r < c.world; ++r)
      for (i64 g = c.row_start[r]; g < c.row_start[r + 1]; ++g) {
        const double y = m.y[c.ord.new2old[g]];
        c.rank_ylo[r] = std::min(c.rank_ylo[r], y);
        c.rank_yhi[r] = std::max(c.rank_yhi[r], y);
      }
    double hy = 0.0;
    for (i64 t = 0; t < m.T; ++t) {
      const double a = m.y[m.tri[3 * t]], b = m.y[m.tri[3 * t + 1]], d = m.y[m.tri[3 * t + 2]];
      hy = std::max(hy, std::max({a, b, d}) - std::min({a, b, d}));
    }
    c.tri_hy = hy;
  }
  clk.mark("partition, plans, level tables");
  if (c.lattice) {
    const LatticeLevel& LL = c.mg.back().latl;
    std::vector<i32> rows;
    for (i64 i = 0; i < c.lp.n_own; ++i)
      if (LL.type[c.lp.r0 + i] != 0) rows.push_back((i32)i);
    build_sell_rows(c.P, c.lp.r0, rows, c.lp, c.sP);
    build_sell_rows(c.Pp, c.lp.r0, rows, c.lp, c.sPp);
    if (c.use_mg && c.mg.back().deep) {  // deep halos: the finest level's ghost rows (pressure, A_visc / K)
      MgLevel& F = c.mg.back();
      F.flook.init(c.macro, F.latl);
      const GhostRowFn fn = face_ghost_rows(c.macro, F.latl, F.flook, &F.dof, c.mg_levels, prm.dt * prm.nu);
      sell_append_ghost_rows(c.Pp, F.g1, c.lp, c.sPp, nullptr, &fn);
      sell_append_ghost_rows(c.P, F.g1, c.lp, c.sP);
    }
  } else {
    build_sell(c.P, c.lp, c.sP);
    if (stokes) build_sell(c.Pp, c.lp, c.sPp);
  }
  if (literal) build_sell(c.Lit, c.lp, c.sLit);
  c.built = true;
  c.tr_D = 0.0;  // (pucfem_set_tracer_diffusion: off after every build)
  c.tr_seed = 0;
  c.tr_ylo = c.mesh.y.empty() ? 0.0 : *std::min_element(c.mesh.y.begin(), c.mesh.y.end());
  c.tr_yhi = c.mesh.y.empty() ? 0.0 : *std::max_element(c.mesh.y.begin(), c.mesh.y.end());
  // tooling hook (tools/spmv_lab.hip --real): the pressure operator's SELL image
  if (const char* path = std::getenv("PUCFEM_DUMP_SELL")) {
    if (stokes) {
      std::vector<double> v;
      sell_values(c.Pp, c.lp, c.sPp, c.Pp.val, v);
      dump_sell(path, c.sPp, v);
    }
  }
  if (clk.on) {  // slice widths of the skeleton SELLs (PUCFEM_SETUP_TIMING): > 14 runs the generic entry loop
    for (const auto* S : {&c.sP, &c.sPp}) {
      std::map<int, i64> h;
      for (i32 w : S->slice_w) ++h[w];
      std::fprintf(stderr, "[setup] SELL %s: %lld slices, widths", S == &c.sP ? "P (K, G)" : "Pp (pressure)",
                   (long long)S->nslices);
      for (auto& kv : h) std::fprintf(stderr, " %d:%lld", kv.first, (long long)kv.second);
      std::fprintf(stderr, "\n");
    }
  }
  clk.mark("SELL images");
  if (c.host_only) return;

  // ---------------------------------------------------------------- device upload
  LocalPlan& lp = c.lp;
  const i64 no = lp.n_own;
  c.nloc = no + lp.n_ghost;
  auto dsell = [&](const Sell& S, const Csr& A, DevSell& D) {
    D.off = c.upload(S.slice_off);
    D.w = c.upload(S.slice_w);
    D.col = c.upload(S.col);
    c.attach_c16(S, c.nloc, D);
    D.nslices = S.nslices;
    D.nrows = S.nrows;
    D.padded = S.padded;
    D.nnz = S.rows.empty() ? A.rowptr[lp.r1] - A.rowptr[lp.r0] : S.nnz;
    if (!S.rows.empty()) D.rows = c.upload(S.rows);
    D.n_own = lp.n_own;
    D.ghost_slices(S);
  };
  std::vector<double> tmp;
  dsell(c.sP, c.P, c.dP);
  sell_values(c.P, lp, c.sP, c.as.K, tmp);
  c.dK = c.upload(tmp);
  sell_values(c.P, lp, c.sP, c.as.Gx, tmp);
  c.dGx = c.upload(tmp);
  sell_values(c.P, lp, c.sP, c.as.Gy, tmp);
  c.dGy = c.upload(tmp);
  if (c.dye_impl) {  // implicit dye operator on the merged pattern, every row stored
    const DyeOp& D = c.dyeop;
    Sell S;
    build_sell(c.Pp, lp, S);
    dsell(S, c.Pp, c.dDye);
    const i64 nnzp = c.Pp.nnz();
    std::vector<double> eid(nnzp);
    for (i64 e = 0; e < nnzp; ++e) eid[e] = (double)(e + 1);
    sell_values(c.Pp, lp, S, eid, tmp);
    std::vector<i32> slot2e(S.padded);
    for (i64 q = 0; q < S.padded; ++q) slot2e[q] = tmp[q] > 0.0 ? (i32)(tmp[q] - 1.0) : -1;
    std::vector<double> mm(nnzp, 0.0);  // merged consistent mass, identity slave rows
    for (i64 e = 0; e < nnzp; ++e) {
      if (D.eptr[e] == D.eptr[e + 1]) mm[e] = 1.0;
      for (i64 z = D.eptr[e]; z < D.eptr[e + 1]; ++z) mm[e] += D.mc[D.ek[z]];
    }
    sell_values(c.Pp, lp, S, mm, tmp);
    c.dDyeM = c.upload(tmp);
    std::vector<i64> dslot(N);
    for (i64 r = 0; r < N; ++r) {
      const i64 e = c.Pp.find(r, (i32)r);
      require(e >= 0, "dye operator: a row without a diagonal");
      dslot[r] = S.slice_off[r / 64] + (e - c.Pp.rowptr[r]) * 64 + r % 64;
    }
    c.dDyeDiag = c.upload(dslot);
    c.dye = DyeDev{c.upload(slot2e), c.upload(D.eptr), c.upload(D.ek), c.upload(D.mc), c.upload(c.as.K),
                   c.upload(D.cptr), c.upload(D.cw), c.upload(D.diag_row), c.upload(c.dof), c.upload(c.as.M), S.padded};
    c.dye_nsrow = (int32_t)D.srow.size();
    if (c.dye_nsrow > 0) {
      c.dDyeSrow = c.upload(D.srow);
      c.dDyeSptr = c.upload(D.sptr);
      c.dDyeSk = c.upload(D.sk);
      c.dDyeSc = c.upload(D.sc);
    }
    c.dDyeVal = c.dalloc<double>(S.padded);
    c.dDyeW = c.dalloc<double>(3 * m.T);
    c.dDyeDinv = c.dalloc<double>(c.nloc);
    c.dDyeB = c.dalloc<double>(c.nloc);
  }
  clk.mark("device: K, G, dye operator");
  // Jacobi symmetric scaling S A S: s_g = 1 / sqrt(a_gg); the scaled values s_r a_rk s_col go straight into
  // the SELL image (only the skeleton rows on lattice hierarchies)
  auto scaling = [&](const Csr& A, const std::vector<double>& val, std::vector<double>& sg) {
    host_alloc_fresh(sg, N);
    parallel_for(N, [&](i64 g0, i64 g1) {
      for (i64 g = g0; g < g1; ++g) sg[g] = 1.0 / std::sqrt(diag_of(A, val, g));
    });
  };
  auto local_vec = [&](const std::vector<double>& g) {  // owned + ghost entries of a global vector
    std::vector<double> v;
    host_alloc_fresh(v, c.nloc);
    parallel_for(no, [&](i64 i0, i64 i1) { std::memcpy(v.data() + i0, g.data() + lp.r0 + i0, sizeof(double) * (i1 - i0)); });
    for (i64 k = 0; k < lp.n_ghost; ++k) v[no + k] = g[lp.ghost_global[k]];
    return v;
  };
  {
    std::vector<double> sg;
    scaling(c.P, c.Kv, sg);
    sell_values_fn(c.P, lp.r0, c.sP, [&](i64 r, i64 k) { return sg[r] * c.Kv[k] * sg[c.P.col[k]]; }, tmp);
    c.dKv = c.upload(tmp);
    c.dsv = c.upload(local_vec(sg));  // (k_visc_prep forms 1 / s itself)
    if (c.lattice) {  // scaled A_visc, skeleton columns: s_j, 0 for Dirichlet columns (StokesColor.py:473-475)
      std::vector<double> w = local_vec(sg);
      for (i64 i = 0; i < no; ++i)
        if (isdir[lp.r0 + i]) w[i] = 0.0;
      for (i64 k = 0; k < lp.n_ghost; ++k)
        if (isdir[lp.ghost_global[k]]) w[no + k] = 0.0;
      c.dwsk = c.upload(w);
    }
  }
  clk.mark("  dev: scaled A_visc");
  if (stokes) {
    dsell(c.sPp, c.Pp, c.dPp);
    if (!c.lattice) {  // the Jacobi-scaled pressure operator (Jacobi-CG and the SELL unit op; a lattice hierarchy
                       // always runs the multigrid PCG on the unscaled one)
      std::vector<double> sg;
      scaling(c.Pp, c.Pp.val, sg);
      sell_values_fn(c.Pp, lp.r0, c.sPp, [&](i64 r, i64 k) { return sg[r] * c.Pp.val[k] * sg[c.Pp.col[k]]; }, tmp);
      c.dKp = c.upload(tmp);
      c.dsp = c.upload(local_vec(sg));
    }
  }
  if (c.use_mg) {
    sell_values(c.Pp, lp, c.sPp, c.Pp.val, tmp);
    c.dKp_raw = c.upload(tmp);
    c.z = c.dalloc<double>(c.nloc);
    c.z32 = c.dalloc<float>(c.nloc);

    c.r32 = c.dalloc<float>(c.nloc);
    c.mg_single = c.prm.mg_single != 0;
    if (c.mg_single) mg_alloc<float>(c, tmp);
    else mg_alloc<double>(c, tmp);
    clk.mark("  dev: pressure SELL, level values");
    if (c.lattice) {  // the face parts of every lattice operator (pucfem_lattice.hpp)
      auto mkface = [&](const std::vector<lat::FaceTab>& tab, const std::vector<lat::FaceTab>* tab2, const double* coef,
                        const float* coef32, int l, int l2, int op) {
        HFace h;
        const i32 n = 1 << l, F = lat::interior_count(n);
        if (tab.empty() || F == 0) return h;
        h.d.tab = c.upload(tab);
        h.d.tab2 = tab2 ? c.upload(*tab2) : nullptr;
        h.d.coef = coef;
        h.d.coef32 = coef32;
        h.d.wsk = op == 1 ? c.dwsk : nullptr;
        h.d.nf = (int32_t)tab.size();
        h.d.n = n;
        h.d.F = F;
        h.d.cpf = (F + BS * FACE_RPT - 1) / (BS * FACE_RPT);
        h.d.n2 = l2 >= 0 ? 1 << l2 : 0;
        h.d.rinv = 1.0f / (float)(n - 1);
        h.d.nb = 0;
        h.d.op = op;
        h.items = h.d.nf * h.d.cpf;
        h.rows = (i64)h.d.nf * F;
        return h;
      };
      const int Lv = c.mg_levels;
      for (int l = 0; l <= Lv; ++l) {
        MgLevel& L = c.mg[l];
        const double* coef = c.upload(L.lf_coef);
        const float* coef32 = c.upload(std::vector<float>(L.lf_coef.begin(), L.lf_coef.end()));
        if (l < Lv) {
          L.hA = mkface(L.lf_merged, nullptr, coef, coef32, l, -1, 0);
        } else {
          c.fP = mkface(L.lf_merged, nullptr, coef, coef32, l, -1, 0);
          c.fK = mkface(L.lf_plain, nullptr, coef, coef32, l, -1, 0);
          c.fVisc = mkface(L.lf_plain, nullptr, coef, coef32, l, -1, 1);
        }
        if (l >= 1) {
          L.hPr = mkface(L.lf_plain, &L.pr_tab2, nullptr, nullptr, l, l - 1, 0);
          L.hR = mkface(L.r_tab, &L.r_tab2, nullptr, nullptr, l - 1, l, 0);
        }
      }
    }
    clk.mark("  dev: lattice face tables");
    // coarse solve: dense pseudo-inverse of the merged operator, constants regularised on the free dofs
    c.dAinv = c.upload(dense_coarse_inverse(c.mg[0]));
  }
  if (c.dist() && c.use_mg) {  // deep-halo flags: every rank takes the same exchanges (a flag off anywhere is off)
    const size_t nl = c.mg.size();
    std::vector<double> off(4 * nl);
    for (size_t l = 0; l < nl; ++l) {
      off[4 * l] = c.mg[l].deep ? 0.0 : 1.0;
      off[4 * l + 1] = c.mg[l].res_deep ? 0.0 : 1.0;
      off[4 * l + 2] = c.mg[l].xc_deep ? 0.0 : 1.0;
      off[4 * l + 3] = c.mg[l].pr_deep ? 0.0 : 1.0;
    }
    DevTmp<double> t(off, c.st);
    c.comm->allreduce(t.p, off.size(), true, c.st);
    t.get(off, off.size(), c.st);
    HIPCHK(hipStreamSynchronize(c.st));
    for (size_t l = 0; l < nl; ++l) {
      MgLevel& L = c.mg[l];
      L.deep = L.deep && off[4 * l] == 0.0;
      L.res_deep = L.deep && L.res_deep && off[4 * l + 1] == 0.0;
      L.xc_deep = l > 0 && c.mg[l - 1].deep && L.xc_deep && off[4 * l + 2] == 0.0;
      L.pr_deep = l > 0 && L.deep && (L.xc_deep || c.mg[l - 1].rep) && L.pr_deep && off[4 * l + 3] == 0.0;
      if (std::getenv("PUCFEM_DEEP_REPORT") && c.rank == 0)  // (diagnostic: tools/comm_probe.py)
        std::fprintf(stderr, "[deep] level %zu: rep %d deep %d res %d xc %d pr %d  own %lld ghosts %lld g1 %zu\n", l,
                     (int)L.rep, (int)L.deep, (int)L.res_deep, (int)L.xc_deep, (int)L.pr_deep, (long long)L.lp.n_own,
                     (long long)L.lp.n_ghost, L.g1.size());
    }
  }
  c.block_cg = c.prm.solver_path != 1;
  c.dense = stokes && !c.dist() && N <= DENSE_MAX && c.prm.precond != 1 && c.prm.solver_path != 1;
  // the small-mesh step is ~20 latency-bound launches replayed from a graph: its reductions finish inside their
  // producers (RedOut, the last block reduces) instead of a k_reduce launch after each (PUCFEM_FUSED_RED=0 keeps them)
  if (c.dense && !std::getenv("PUCFEM_FUSED_RED")) c.fused_red = true;
  clk.mark("device: A_visc, pressure, multigrid");
  // successive-RHS projections (multi-kernel CG paths only: the dense and one-workgroup solves of
  // small meshes need no better start)
  // (a basis needs room for the re-seeded span and one new direction: at least 3)
  auto proj_size = [](int k) { return k <= 0 ? 0 : std::max(3, std::min(k, (int)PROJ_MAX)); };
  c.proj_k = c.use_mg && !c.dense ? proj_size(c.prm.proj_k) : 0;
  c.proj_shared = c.prm.proj_shared != 0;
  // pending pressure directions and the gradient on y (Ctx::p_from_y): lattice operators, the multigrid PCG
  // with the projection, the explicit dye; PUCFEM_P_FROM_Y=0 keeps the stored form (a measurement knob: the
  // same values either way).  Partitioned runs exchange y's halo instead of p's.
  c.p_from_y = stokes && c.lattice && c.use_mg && c.proj_k > 0 && !c.dye_impl && c.dP.c16 == nullptr &&
               !(std::getenv("PUCFEM_P_FROM_Y") && std::atoi(std::getenv("PUCFEM_P_FROM_Y")) == 0);
  if (c.p_from_y) {  // dP with every column mapped to its periodic master (the dof map), in local ids
    std::vector<i32> colm(c.sP.col.size());
    const i64 nl = (i64)c.nloc;
    bool ok = true;
    for (size_t e = 0; e < colm.size() && ok; ++e) {
      const i32 j = c.sP.col[e];
      colm[e] = j;
      if (j < 0 || j >= nl) continue;
      const i32 g = j < no ? (i32)(lp.r0 + j) : lp.ghost_global[j - no];
      const i32 mg = c.dof[g];
      if (mg == g) continue;
      if (mg >= lp.r0 && mg < lp.r1) {
        colm[e] = (i32)(mg - lp.r0);
      } else {
        auto it = std::lower_bound(lp.ghost_global.begin(), lp.ghost_global.end(), mg);
        if (it == lp.ghost_global.end() || *it != mg) ok = false;  // a master outside the local columns
        else colm[e] = (i32)(no + (it - lp.ghost_global.begin()));
      }
    }
    // every rank takes the same path: a rank whose merged columns reach outside its local columns would
    // halo p while its neighbours send y (whose slave entries are not copies of their masters)
    if (c.dist()) {
      std::vector<double> bad(1, ok ? 0.0 : 1.0);
      DevTmp<double> t(bad, c.st);
      c.comm->allreduce(t.p, 1, true, c.st);
      t.get(bad, 1, c.st);
      HIPCHK(hipStreamSynchronize(c.st));
      ok = bad[0] == 0.0;
    }
    c.p_from_y = ok;
    if (ok) {
      c.dPm = c.dP;
      c.dPm.col = c.upload(colm);
    }
  }
  const bool block_visc = !c.dist() && c.block_cg && no <= (i64)CGB_THREADS * CGB_MAXR;
  c.proj_k_visc = stokes && !c.dense && !block_visc ? proj_size(c.prm.proj_k_visc) : 0;
  for (int w = 1; w <= 4; ++w) {
    const int k = w <= 2 ? c.proj_k : c.proj_k_visc;
    if (k > 0) {
      const i64 pn = (c.nloc + 63) / 64 * 64 * k;
      c.projX[w] = c.dalloc<ProjT>(pn);
      c.proj_x0[w] = c.dalloc<double>(c.nloc);
      c.projXalt[w] = c.dalloc<ProjT>(pn);  // re-seeding target
    }
  }
  if (stokes && !c.dense && !block_visc && c.proj_k_visc == 0 && c.visc_extrap > 0)
    for (int k = 0; k < 2 * c.visc_extrap; ++k) c.dvinc[k] = c.dalloc<float>(c.nloc);
  if (c.proj_k > 0 || c.proj_k_visc > 0) {
    for (int w = 1; w <= 4; ++w)
      if (c.projX[w]) {
        c.pv[w] = c.dalloc<double>(c.nloc);
        c.pav[w] = c.dalloc<double>(c.nloc);
      }
    c.proj_part = c.dalloc<double>((i64)Ctx::NCOEF * MAXB);
    c.dqm = c.dalloc<double>((i64)sizeof(QMat) / (i64)sizeof(double));
    c.proj_d = c.dalloc<double>(Ctx::NCOEF);
    c.proj_coef = c.dalloc<double>(Ctx::NCOEF);
  }
  if (c.dense) {
    // A_visc^-1 and the pseudo-inverse of the merged pressure operator (constants on the free dofs
    // regularised, as for the multigrid coarse level)
    std::vector<double> Dv(N * N, 0.0), Dp(N * N, 0.0);
    for (i64 r = 0; r < N; ++r) {
      for (i64 k = c.P.rowptr[r]; k < c.P.rowptr[r + 1]; ++k) Dv[r * N + c.P.col[k]] = c.Kv[k];
      for (i64 k = c.Pp.rowptr[r]; k < c.Pp.rowptr[r + 1]; ++k) Dp[r * N + c.Pp.col[k]] += c.Pp.val[k];
    }
    double dsum = 0.0;
    for (i64 r = 0; r < N; ++r)
      if (c.master_of[r] < 0) dsum += Dp[r * N + r];
    const double cc = dsum / (double)c.n_free / (double)c.n_free;
    for (i64 i = 0; i < N; ++i)
      if (c.master_of[i] < 0)
        for (i64 j = 0; j < N; ++j)
          if (c.master_of[j] < 0) Dp[i * N + j] += cc;
    require(spd_inverse(Dv, N), "A_visc is not SPD");
    require(spd_inverse(Dp, N), "regularised pressure operator is not SPD");
    c.dVinv = c.upload(Dv);
    c.dPinv = c.upload(Dp);
  }
  if (literal && !c.dist() && N <= DENSE_MAX && c.prm.solver_path != 1) {
    std::vector<double> D(N * N, 0.0);
    for (i64 r = 0; r < N; ++r)
      for (i64 k = c.Lit.rowptr[r]; k < c.Lit.rowptr[r + 1]; ++k) D[r * N + c.Lit.col[k]] += c.Lit.val[k];
    require(lu_inverse(D, N), "literal operator is singular");
    c.dLitInv = c.upload(D);
  }
  if (literal) {
    dsell(c.sLit, c.Lit, c.dLit);
    sell_values(c.Lit, lp, c.sLit, c.Lit.val, tmp);
    c.dLitv = c.upload(tmp);
    std::vector<double> dinv(N);
    for (i64 g = 0; g < N; ++g) dinv[g] = 1.0 / diag_of(c.Lit, c.Lit.val, g);
    c.dlit_dinv = c.upload(dinv);
  }
  clk.mark("device: projections, dense");
  // per-row data
  {
    std::vector<double> as1, mp, wm;
    std::vector<uint8_t> df;
    std::vector<i32> so, mo;
    host_alloc_fresh(as1, no);
    host_alloc_fresh(mp, no);
    host_alloc_fresh(wm, no);
    host_alloc_fresh(df, no);
    host_alloc_fresh(so, no);
    host_alloc_fresh(mo, no);
    parallel_for(no, [&](i64 i0, i64 i1) {
      for (i64 i = i0; i < i1; ++i) {
        const i64 g = lp.r0 + i;
        as1[i] = c.as.asum[g] + 1e-12;
        mp[i] = c.as.M[g] + 1e-12;
        wm[i] = m.mk[c.ord.new2old[g]] == 0 ? c.as.M[g] : 0.0;
        df[i] = isdir[g];
        so[i] = c.slave_of[g] >= 0 ? to_local(lp, c.slave_of[g]) : -1;
        mo[i] = c.master_of[g] >= 0 ? to_local(lp, c.master_of[g]) : -1;
        require(so[i] < (i32)no && mo[i] < (i32)no, "periodic partner on another rank");
      }
    });
    c.das1 = c.upload(as1);
    c.dmp = c.upload(mp);
    c.dwmix = c.upload(wm);
    c.ddir = c.upload(df);
    c.dslave_of = c.upload(so);
    c.dmaster_of = c.upload(mo);
  }
  clk.mark("  dev: per-row data");
  // BC lists: sequential copy semantics resolved symbolically (caller numbering), then local
  {
    std::vector<i64> src(N);
    for (i64 i = 0; i < N; ++i) src[i] = i;
    for (auto& pr : c.bc_pairs) src[pr.second] = src[pr.first];
    std::vector<i32> cd, cs;
    for (i64 o = 0; o < N; ++o)
      if (src[o] != o) {
        const i64 g = c.ord.old2new[o];
        if (g < lp.r0 || g >= lp.r1) continue;
        const i64 gs = c.ord.old2new[src[o]];
        require(gs >= lp.r0 && gs < lp.r1, "periodic BC source on another rank");
        cd.push_back((i32)(g - lp.r0));
        cs.push_back((i32)(gs - lp.r0));
      }
    // Dirichlet: last occurrence wins (sequential semantics), owned nodes only
    std::vector<i64> last(N, -1);
    for (size_t k = 0; k < c.dir_nodes.size(); ++k) last[c.dir_nodes[k]] = (i64)k;
    std::vector<i32> dn;
    std::vector<double> dv;
    for (size_t k = 0; k < c.dir_nodes.size(); ++k) {
      if (last[c.dir_nodes[k]] != (i64)k) continue;
      const i64 g = c.ord.old2new[c.dir_nodes[k]];
      if (g < lp.r0 || g >= lp.r1) continue;
      dn.push_back((i32)(g - lp.r0));
      for (int q = 0; q < c.dir_ncomp; ++q) dv.push_back(c.dir_vals[c.dir_ncomp * k + q]);
    }
    // a copy into a Dirichlet node is overwritten by its Dirichlet value: drop it, so the write sets
    // are disjoint
    {
      std::vector<char> written(no, 0);
      for (i32 d : dn) written[d] = 1;
      std::vector<i32> cd2, cs2;
      for (size_t k = 0; k < cd.size(); ++k)
        if (!written[cd[k]]) {
          cd2.push_back(cd[k]);
          cs2.push_back(cs[k]);
        }
      cd.swap(cd2);
      cs.swap(cs2);
      for (i32 d : cd) written[d] = 1;
      c.bc_gather = false;
      for (i32 sidx : cs) c.bc_gather = c.bc_gather || written[sidx];
    }
    c.ncopy = (int)cd.size();
    c.ndir = (int)dn.size();
    c.dcdst = c.upload(cd);
    c.dcsrc = c.upload(cs);
    c.ddnode = c.upload(dn);
    c.ddval = c.upload(dv);
    c.dval_build = dv;  // (what clearing a stroke restores)
    c.dbctmp = c.dalloc<double>(2 * std::max(1, c.ncopy));
    c.dspos = nullptr;  // (k_grad_proj_bc's position map follows the operators: rebuilt at the next step call)
    c.dbcsrc = c.dbcdir = nullptr;
    if (c.dense) {  // k_dense_mv2_bc's per-row maps
      std::vector<i32> bsrc(no), bdir(no, -1);
      for (i64 i = 0; i < no; ++i) bsrc[i] = (i32)i;
      for (size_t k = 0; k < cd.size(); ++k) bsrc[cd[k]] = cs[k];
      for (size_t k = 0; k < dn.size(); ++k) bdir[dn[k]] = (i32)k;
      c.dbcsrc = c.upload(bsrc);
      c.dbcdir = c.upload(bdir);
    }
  }
  clk.mark("  dev: BC lists");
  // halo plan
  c.nsend = (i64)lp.send_local.size();
  c.dsend = c.upload(lp.send_local);
  c.dsendbuf = c.dalloc<double>(4 * std::max<i64>(1, c.nsend));  // (two interleaved vectors: halo2(x, b))
  // fields + workspace
  for (double** f : {&c.p, &c.p2, &c.yp, &c.yp2, &c.yvx, &c.yvy, &c.div_star, &c.div_u, &c.final_div, &c.braw,
                     &c.bh, &c.bvx, &c.bvy, &c.scalar})
    *f = c.dalloc<double>(c.nloc);
  // u and u*: interleaved (x, y) pairs (VS); ux / usx point at the pairs, uy / usy at their y components
  c.ux = c.dalloc<double>(2 * c.nloc);
  c.uy = c.ux + 1;
  c.usx = c.dalloc<double>(2 * c.nloc);
  c.usy = c.usx + 1;
  for (int q = 0; q < 2; ++q) {
    c.cg_r[q] = c.dalloc<double>(c.nloc);
    c.cg_pa[q] = c.dalloc<double>(c.nloc);
    c.cg_pb[q] = c.dalloc<double>(c.nloc);
    c.cg_q[q] = c.dalloc<double>(c.nloc);
  }
  if (stokes && !c.dense) {  // the viscous Chebyshev solve's interleaved vectors
    for (auto& x : c.vx2) x = c.dalloc<dbl2>(c.nloc);
    c.vb2 = c.dalloc<dbl2>(c.nloc);
    for (auto& d : c.vd2) d = c.dalloc<flt2>(c.nloc);
  }
  // 6 MAXB: the recurrence CG direction kernel writes 3 dots per right-hand side
  for (double** f : {&c.part_a, &c.part_b, &c.part_c, &c.part_d}) *f = c.dalloc<double>(6 * MAXB);
  c.part_sl = c.dalloc<double>(3 * SLB);
  c.part_mx = c.dalloc<double>(MAXB);
  c.part_fd = c.dalloc<double>(2 * MAXB);
  if (const char* e = std::getenv("PUCFEM_SL_OVERLAP")) c.sl_overlap = std::atoi(e) != 0;  // 0: one stream
  c.part_u = c.dalloc<double>(2 * MAXB);
  c.yr_own = c.dalloc<double>(2);
  c.yr_all = c.dalloc<double>(2 * c.world);
  c.h_yr.assign(2 * c.world, 0.0);
  if (stokes) {
    c.sl_queue = c.dalloc<int32_t>(m.N);
    c.sl_qcnt = c.dalloc<int32_t>(SLB * BS / 64);
    c.sl_qoff = c.dalloc<int32_t>(SLB * BS / 64 + 1);
  }
  c.scal = c.dalloc<double>(32);
  c.part_cc = c.dalloc<double>(CGCG_NV * MAXB);
  c.cgcg_sc = c.dalloc<double>(8);
  c.ctl = c.dalloc<int>(8);  // [0..1] the control word, bytes 8..23: the PCG's initial <r, r>, <b, b> (k_conv's note)
  c.redbuf = c.dalloc<double>(8 * 64);
  c.dcnt = c.dalloc<unsigned>(Ctx::CNT_N);
  c.vals = c.dalloc<double>(16);
  c.bicg_sc = c.dalloc<double>(16);
  if (literal || c.dye_impl) {
    for (int q = 0; q < 9; ++q) c.litw[q] = c.dalloc<double>(c.nloc);
  }
  clk.mark("device: per-row data, BCs, halo, workspace");
  // full-mesh replica in internal numbering (the host half: sl_prep, on its thread since the hierarchy)
  if (!stokes) sl_prep(c, false, slp);
  slg.join();
  clk.mark("SL: host tables (joined)");
  {
    const std::vector<double>&X = slp.X, &Y = slp.Y;
    const std::vector<i32>& tri = slp.tri;
    c.mx = c.upload(X);
    c.my = c.upload(Y);
    c.mtri = c.upload(tri);
    auto dgrid = [&](const Grid& G, GridDev& D, bool pts) {
      D.nx = G.nx;
      D.ny = G.ny;
      D.x0 = G.x0;
      D.y0 = G.y0;
      D.hx = G.hx;
      D.hy = G.hy;
      D.start = c.upload(G.cell_start);
      D.item = c.upload(G.item);
      D.px = pts ? c.upload(G.px) : nullptr;
      D.py = pts ? c.upload(G.py) : nullptr;
    };
    if (stokes) {  // PointLocator centroids (StokesColor.py:321), their grid (sl_prep)
      const std::vector<double>&cx = slp.cx, &cy = slp.cy;
      const Grid& G = slp.G;
      dgrid(G, c.cgrid, true);
      c.has_cgrid = true;
      if (prm.scheme == PUCFEM_STOKES_FOOD) {  // tracer location (StokesFood only)
        dgrid(slp.TG, c.tgrid, false);
        c.has_tgrid = true;
      }
      clk.mark("SL: centroid / triangle grids");
      // fast-accept radii (k-NN of every centroid among the centroids, of every vertex among the
      // centroids): on the device (k_knn_radius2, bit-identical to the host's knn_radius2, which
      // PUCFEM_KNN_HOST=1 selects -- the cross-check of tests/test_gpu_parity.py)
      const bool knn_host = std::getenv("PUCFEM_KNN_HOST") && std::atoi(std::getenv("PUCFEM_KNN_HOST"));
      const bool knn_ok = (i64)G.item.size() - 1 >= KNN && (i64)G.item.size() >= KNN + 1;
      std::vector<float> rho2;
      const float* drho2 = nullptr;
      const float* drv2 = nullptr;
      if (knn_host || !knn_ok) {
        rho2 = centroid_knn_radius2(G, cx, cy, KNN);
        drho2 = c.upload(rho2);
        clk.mark("SL: centroid 10-NN radii");
        drv2 = c.upload(knn_radius2(G, X, Y, KNN + 1, false));
      } else {
        float* r2 = c.dalloc<float>(m.T);
        hipLaunchKernelGGL(k_knn_radius2, dim3((unsigned)std::min<i64>(65536, (m.T + BS - 1) / BS)), dim3(BS), 0, c.st,
                           c.cgrid, c.cgrid.px, c.cgrid.py, c.cgrid.item, (int64_t)m.T, KNN, 1, r2);
        KCHK();
        float* v2 = c.dalloc<float>(N);
        hipLaunchKernelGGL(k_knn_radius2, dim3((unsigned)std::min<i64>(65536, (N + BS - 1) / BS)), dim3(BS), 0, c.st,
                           c.cgrid, (const double*)c.mx, (const double*)c.my, (const int32_t*)nullptr, (int64_t)N,
                           KNN + 1, 0, v2);
        KCHK();
        drho2 = r2;
        drv2 = v2;
        clk.mark("SL: centroid 10-NN radii");
      }
      const double2* dxy = reinterpret_cast<const double2*>(c.upload(slp.xy));
      clk.mark("SL: vertex 11-NN radii");
      const int probe = std::getenv("PUCFEM_SL_PROBE") ? std::atoi(std::getenv("PUCFEM_SL_PROBE")) : 0;
      c.lat_sl = slp.lat_sl;  // the lattice locator (sl_prep decided), else the record locator below
      if (c.lat_sl) {
        GridDev mg{};
        dgrid(slp.MG, mg, false);
        c.llgrid = LatLocDev{mg.nx, mg.ny, mg.x0, mg.y0, 1.0 / mg.hx, 1.0 / mg.hy, mg.start, mg.item,
                             reinterpret_cast<const lat::SlFace*>(c.upload(slp.sf)), c.upload(slp.cells), dxy,
                             drho2, drv2, c.upload(slp.home), nullptr, c.mg.back().latl.n, probe};
        // zero-velocity rows (walls): the answer for the row's own node, once
        int32_t* dself = c.dalloc<int32_t>(N);
        hipLaunchKernelGGL(k_sl_self<LatLocDev>, dim3(2048), dim3(BS), 0, c.st, MeshDev{c.mx, c.my, c.mtri, m.T},
                           c.llgrid, c.cgrid, (int64_t)N, dself);
        KCHK();
        c.llgrid.self = dself;
      } else {
        // inflated-bbox grid (~1 triangle per cell) + packed records
        Grid LG;
        build_tri_grid(X, Y, tri, 1.0, LG, 1e-6);
        // records in node order: position p holds triangle p2t[p], sorted by smallest vertex id
        std::vector<i32> p2t(m.T), t2p(m.T), vmin(m.T);
        for (i64 t = 0; t < m.T; ++t) {
          p2t[t] = (i32)t;
          vmin[t] = std::min(tri[3 * t], std::min(tri[3 * t + 1], tri[3 * t + 2]));
        }
        std::stable_sort(p2t.begin(), p2t.end(), [&](i32 a, i32 b) { return vmin[a] < vmin[b]; });
        for (i64 p = 0; p < m.T; ++p) t2p[p2t[p]] = (i32)p;
        if (rho2.empty()) {  // the device radii, in triangle order, for the record permutation below
          rho2.resize(m.T);
          HIPCHK(hipMemcpyAsync(rho2.data(), drho2, sizeof(float) * m.T, hipMemcpyDeviceToHost, c.st));
          HIPCHK(hipStreamSynchronize(c.st));
        }
        std::vector<int32_t> rec(4 * (size_t)m.T);  // SlTri records (pucfem_kernels_impl.hpp)
        std::vector<float> rho2p(m.T);
        for (i64 p = 0; p < m.T; ++p) {
          const i64 t = p2t[p];
          for (int v = 0; v < 3; ++v) rec[4 * p + v] = tri[3 * t + v];
          rec[4 * p + 3] = (int32_t)t;
          rho2p[p] = rho2[t];
        }
        for (i64 cl = 0; cl + 1 < (i64)LG.cell_start.size(); ++cl) {
          auto b0 = LG.item.begin() + LG.cell_start[cl], b1 = LG.item.begin() + LG.cell_start[cl + 1];
          for (auto it = b0; it != b1; ++it) *it = t2p[*it];
          std::sort(b0, b1);
        }
        GridDev lg{};
        dgrid(LG, lg, false);
        c.lgrid = LocDev{lg.nx, lg.ny, lg.x0, lg.y0, lg.hx, lg.hy, lg.start, lg.item,
                         reinterpret_cast<const int4*>(c.upload(rec)), dxy, c.upload(rho2p), drv2, probe};
      }
    }
    c.c_full = c.dalloc<double>(N);
    c.c_new = c.dalloc<double>(N);
    c.dnotfound = c.dalloc<int32_t>(no);
    if (c.dist()) {
      c.ufx = c.dalloc<double>(N);
      c.ufy = c.dalloc<double>(N);
      if (c.lp.n_ghost > 0) c.dghost_global = c.upload(c.lp.ghost_global);
    }
  }
  // initial state: u = 0 then makeDirBCU (StokesColor.py:482-483); c = 1[x < 0.5] (:493-495)
  if (stokes) {
    c.bc(c.ux, c.uy);
    c.halo_v(c.ux);
    HIPCHK(hipMemcpyAsync(c.c_full, slp.c0.data(), sizeof(double) * N, hipMemcpyHostToDevice, c.st));
  }
  HIPCHK(hipStreamSynchronize(c.st));
  clk.mark("SL: locator / self table, initial state");
  if (c.use_mg && c.lmax_dev) {
    MgLevel& F = c.mg[c.mg_levels];
    F.lmax = c.lmax_device(F.lmax, &F.lam_dev);
    clk.mark("finest lmax (device power iteration)");
    for (int l = 1; l < c.mg_levels; ++l)
      c.mg[l].lmax = c.mg_single ? c.lmax_level_device<float>(c.mg[l], c.mg[l].lmax)
                                 : c.lmax_level_device<double>(c.mg[l], c.mg[l].lmax);
    clk.mark("coarse lmax (device power iterations)");
  }
}

// ---- tracer I/O of a run and of an ensemble's members: tracers first .. first + count - 1 of the arrays
// new positions from (count, 2) pairs, with what goes with them: status 0, not captured (-1), and the nctr step
// counters at trstep back to 0.  Ordered on st, not synchronised.
void tracers_put(Ctx& c, double* trx, double* try_, double* trs, int32_t* trcap, int32_t* trstep, i64 nctr, i64 first,
                 i64 count, const double* buf) {
  std::vector<double> xy(2 * (size_t)count);
  for (i64 k = 0; k < count; ++k) {
    xy[k] = buf[2 * k];
    xy[count + k] = buf[2 * k + 1];
  }
  HIPCHK(hipMemsetAsync(trstep, 0, sizeof(int32_t) * nctr, c.st));
  if (count == 0) return;
  c.h2d(trx + first, xy.data(), sizeof(double) * count);
  c.h2d(try_ + first, xy.data() + count, sizeof(double) * count);
  HIPCHK(hipMemsetAsync(trs + first, 0, sizeof(double) * count, c.st));
  HIPCHK(hipMemsetAsync(trcap + first, 0xFF, sizeof(int32_t) * count, c.st));
}
void tracers_get(Ctx& c, const double* trx, const double* try_, i64 first, i64 count, double* buf) {
  if (count == 0) return;
  std::vector<double> xy(2 * (size_t)count);
  c.d2h(xy.data(), trx + first, sizeof(double) * count);
  c.d2h(xy.data() + count, try_ + first, sizeof(double) * count);
  for (i64 k = 0; k < count; ++k) {
    buf[2 * k] = xy[k];
    buf[2 * k + 1] = xy[count + k];
  }
}
void capture_steps_get(Ctx& c, const int32_t* trcap, i64 first, i64 count, double* buf) {
  if (count == 0) return;
  std::vector<int32_t> cs((size_t)count);
  c.d2h(cs.data(), trcap + first, sizeof(int32_t) * count);
  for (i64 k = 0; k < count; ++k) buf[k] = (double)cs[k];
}

// ms per launch of `iters` launches on the context's stream (the caller has made its untimed first launch); the
// events are released on every path
template <class F>
double time_launches(Ctx& c, int iters, F&& launch) {
  struct Ev {
    hipEvent_t e = nullptr;
    Ev() { HIPCHK(hipEventCreate(&e)); }
    ~Ev() { (void)hipEventDestroy(e); }
  } a, b;
  HIPCHK(hipEventRecord(a.e, c.st));
  for (int k = 0; k < iters; ++k) launch();
  HIPCHK(hipEventRecord(b.e, c.st));
  HIPCHK(hipEventSynchronize(b.e));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, a.e, b.e));
  return (double)ms / iters;
}

// a probe's figures: every pass launched once untimed (the first launches), then `iters` launches of each pass timed
// on their own.  pass(mask) launches the passes in mask (1, 2 or 3)
template <class F>
void time_passes(Ctx& c, int iters, int npass, double* ms, F&& pass) {
  pass(npass == 2 ? 3 : 1);
  for (int k = 0; k < npass; ++k) ms[k] = time_launches(c, iters, [&] { pass(1 << k); });
}

// ---- the transport layer's unit operations and probes (Ctx::transport_fields / transport_pairs)
// Their scratch, slots 14 .. 23 of smp_scratch, by name (22 is pucfem_stroke_apply's).  tot: the doubles of one set
// of fields, nch x N or, for pairs, 2 N.
struct TransportSlots {
  Ctx& c;
  size_t tot;
  size_t N() const { return (size_t)c.mesh.N; }
  double* in() { return c.smp_scratch<double>(14, tot); }
  double* out() { return c.smp_scratch<double>(15, tot); }
  int32_t* nfpart() { return c.smp_scratch<int32_t>(16, (size_t)SLB); }
  double* ch() { return c.smp_scratch<double>(17, tot); }
  int4* rec() { return c.smp_scratch<int4>(18, N()); }
  int32_t* marks() { return c.smp_scratch<int32_t>(19, N()); }
  int32_t* tri() { return c.smp_scratch<int32_t>(20, N()); }
  int32_t* cnt() { return c.smp_scratch<int32_t>(21, 3 * (size_t)SLB); }
  int32_t* mid() { return c.smp_scratch<int32_t>(23, 2 * (size_t)SLB); }
  // the work buffers mode m uses; rows: with the per-row outputs (marks, tri)
  Ctx::TransportWork work(Ctx::TransportMode m, bool rows) {
    Ctx::TransportWork w;
    w.nfpart = nfpart();
    if (rows) w.marks = marks();
    if (m.mc()) w.ch = ch(), w.rec = rec(), w.cnt = cnt(), w.tri = rows ? tri() : nullptr;
    if (m.mid()) w.mid = mid();
    return w;
  }
};

// marks and tri of a unit operation back to the caller (T1 belongs to the two-pass scheme: -1 under a one-pass one)
void transport_rows_out(Ctx& c, Ctx::TransportMode m, const Ctx::TransportWork& w, int32_t* marks, int32_t* tri) {
  if (marks) c.get_all(1, 1, marks, w.marks);
  if (tri && m.mc()) c.get_all(1, 1, tri, w.tri);
  else if (tri) std::fill(tri, tri + c.mesh.N, -1);
}

// cout = transport(cin; u, dt) for nch plain fields on the whole mesh.  dnf: the rows' marks go through c.dnotfound
// (the first-order entry point's not-found flags)
void advect_fields_unit(Ctx& c, Ctx::TransportMode m, int32_t nch, const double* cin, const double* u, double dt,
                        double* cout, int32_t* marks, int32_t* tri, bool dnf = false) {
  c.dye_ready();
  require(nch >= 1 && nch <= DYE_MAX, "nch must be in 1 .. PUCFEM_MAX_DYES (16)");
  require(cin != nullptr && u != nullptr && cout != nullptr, "null fields");
  TransportSlots s{c, (size_t)nch * (size_t)c.mesh.N};
  double *tu = c.u_scratch(), *din = s.in(), *dout = s.out();
  Ctx::TransportWork w = s.work(m, !dnf);
  if (dnf) w.marks = c.dnotfound;
  c.put_all(1, nch, cin, din);
  c.put_all(2, 1, u, tu);
  c.transport_fields(m, 0, c.mesh.N, tu, dt, nullptr, nullptr, nch, din, dout, w);
  c.get_all(1, nch, cout, dout);
  transport_rows_out(c, m, w, marks, tri);
}

// f_out = transport(f; u, dt) for one field of interleaved pairs
void advect_pairs_unit(Ctx& c, Ctx::TransportMode m, const double* f, const double* u, double dt, double* f_out,
                       int32_t* marks, int32_t* tri, bool dnf = false) {
  c.inertia_ready();
  require(f != nullptr && u != nullptr && f_out != nullptr, "null fields");
  TransportSlots s{c, 2 * (size_t)c.mesh.N};
  double *tu = c.u_scratch(), *din = s.in(), *dout = s.out();
  Ctx::TransportWork w = s.work(m, !dnf);
  if (dnf) w.marks = c.dnotfound;
  c.put_all(2, 1, f, din);
  c.put_all(2, 1, u, tu);
  c.transport_pairs(m, 0, c.mesh.N, tu, dt, din, dout, w);
  c.get_all(2, 1, f_out, dout);
  transport_rows_out(c, m, w, marks, tri);
}

// ms per launch of mode m's passes (ms[1] only under a two-pass scheme) with the context's own u and dt: nch >= 1
// plain fields of zeros, or (nch = 0) the pairs f = u
void transport_probe(Ctx& c, Ctx::TransportMode m, int nch, int iters, double* ms) {
  const i64 N = c.mesh.N;
  TransportSlots s{c, nch ? (size_t)nch * (size_t)N : 2 * (size_t)N};
  const Ctx::TransportWork w = s.work(m, false);
  double *din = nch ? s.in() : nullptr, *dout = s.out();
  if (nch) HIPCHK(hipMemsetAsync(din, 0, sizeof(double) * s.tot, c.st));
  time_passes(c, iters, m.mc() ? 2 : 1, ms, [&](int pass) {
    if (nch) c.transport_fields(m, 0, N, c.ux, c.prm.dt, nullptr, nullptr, nch, din, dout, w, pass);
    else c.transport_pairs(m, 0, N, c.ux, c.prm.dt, c.ux, dout, w, pass);
  });
}

// One transported field of the ensemble -- the velocity of the inertial step, or the dye -- as its MacCormack and
// midpoint launches see it: the members' flags and how many members are on each, the three flag values that leave the
// first-order kernel, the MacCormack set's ch and records, the partials, ticket counters and value slots.  The
// ensemble twin of Ctx::transport_fields / transport_pairs: a new scheme or order is added to ens_transport below
// (and, with channels, to ens_enqueue_dyes, which takes its reductions from the dye's descriptor).
struct EnsTransport {
  const int32_t* on;                 // the members' flags as the kernels read them
  const int* n;                      // members per flag value
  int32_t f_mc, f_sl_mid, f_mc_mid;  // the flag values (ENS_ADV_* / ENS_DYE_*)
  double* ch;                        // the MacCormack set: pass 1's field ...
  int4* rec;                         // ... and triangles
  double *mc_part, *trj_part;        // the launches' partials
  unsigned *mc_cnt, *trj_cnt;        // their ticket counters: pass 1's M, then pass 2's
  double *v_nf, *v_mc;               // the members' vals: not-found rows; pass 2's rows without T2, clamped values
  double* t;                         // the members' trj_vals, the field's four slots (null: no part was ever on)
  size_t sM;
  int nb_sl;
  RedOut mc1() const { return {v_nf, nullptr, mc_cnt, 1, 0, 0u}; }
  RedOut mc2() const { return {v_mc, nullptr, mc_cnt + sM, 2, 0, 0u}; }
  RedOut trj1() const { return {v_nf, t ? t + ENS_T_MID1 : nullptr, trj_cnt, 2, 0, 0u}; }
  RedOut trj2() const { return {t + ENS_T_MC, nullptr, trj_cnt + sM, 3, 0, 0u}; }
  double* mc_part2() const { return mc_part + sM * nb_sl; }
  double* trj_part2() const { return trj_part + sM * 2 * nb_sl; }
  bool any_mid() const { return n[f_sl_mid] + n[f_mc_mid] > 0; }
};
EnsTransport ens_vel_transport(Ens& e) {
  const size_t sM = (size_t)e.M;
  return {e.adv_on_dev, e.vel_n, ENS_ADV_MC, ENS_ADV_SL_MID, ENS_ADV_MC_MID, e.mcv_ch, e.mcv_rec, e.mcv_part, e.trj_part_v,
          e.mcv_cnt, e.trj_cnt ? e.trj_cnt + 2 * sM : nullptr, e.vals + ENS_V_VEL_NF, e.vals + ENS_V_VEL_MC,
          e.trj_vals ? e.trj_vals + ENS_TRJ_VEL : nullptr, sM, e.nb_sl};
}
EnsTransport ens_dye_transport(Ens& e) {
  return {e.mc_on_dev, e.dye_n, ENS_DYE_MC, ENS_DYE_SL_MID, ENS_DYE_MC_MID, e.mc_ch, e.mc_rec, e.mc_part, e.trj_part_d,
          e.mc_cnt, e.trj_cnt, e.vals + ENS_V_DYE_NF, e.vals + ENS_V_DYE_MC,
          e.trj_vals ? e.trj_vals + ENS_TRJ_DYE : nullptr, (size_t)e.M, e.nb_sl};
}
// out = transport(f; u, dt) of the members whose flag left the first-order kernel (which skipped them): MacCormack's
// two passes, the midpoint trace in one pass straight into out, and with both pass 1 into the set's ch and records,
// pass 2 into out.  F: dbl2 (the velocity, Ctx::inertia_step per member) or double (the dye without channels,
// Ctx::dye_transport_step per member).  Pass 1's not-found count goes into v_nf; the sums are the caller's
template <class F>
void ens_transport(Ctx& c, Ens& e, const EnsTransport& t, const F* f, F* out) {
  const MeshDev Mh{c.mx, c.my, c.mtri, c.mesh.T};
  const dim3 grid(e.nb_sl, e.M);
  const int64_t n = e.n;
  const double *u = e.u, dt = c.prm.dt, hdt = 0.5 * c.prm.dt;
  F* ch = reinterpret_cast<F*>(t.ch);
  hipStream_t st = c.st;
  if (t.n[t.f_mc] > 0) {
    hipLaunchKernelGGL(k_ens_mc_fwd<F>, grid, dim3(BS), 0, st, Mh, c.lgrid, c.cgrid, n, u, dt, t.on, t.f_mc, f, ch,
                       t.rec, t.mc_part, t.mc1());
    KCHK();
    hipLaunchKernelGGL(k_ens_mc_bwd<F>, grid, dim3(BS), 0, st, Mh, c.lgrid, c.cgrid, n, u, dt, t.on, t.f_mc, f,
                       (const F*)ch, out, (const int4*)t.rec, t.mc_part2(), t.mc2());
    KCHK();
  }
  if (t.n[t.f_sl_mid] > 0) {
    hipLaunchKernelGGL(k_ens_trj_fwd<F>, grid, dim3(BS), 0, st, Mh, c.lgrid, c.cgrid, n, u, dt, hdt, t.on, t.f_sl_mid, f,
                       out, (int4*)nullptr, t.trj_part, t.trj1());
    KCHK();
  }
  if (t.n[t.f_mc_mid] > 0) {
    hipLaunchKernelGGL(k_ens_trj_fwd<F>, grid, dim3(BS), 0, st, Mh, c.lgrid, c.cgrid, n, u, dt, hdt, t.on, t.f_mc_mid, f,
                       ch, t.rec, t.trj_part, t.trj1());
    KCHK();
    hipLaunchKernelGGL(k_ens_trj_bwd<F>, grid, dim3(BS), 0, st, Mh, c.lgrid, c.cgrid, n, u, dt, hdt, t.on, t.f_mc_mid, f,
                       (const F*)ch, out, (const int4*)t.rec, t.trj_part2(), t.trj2(), t.v_mc);
    KCHK();
  }
}

}  // namespace

// =====================================================================================================
// One piece of the multigrid cycle on caller-numbered fp64 vectors (see pucfem.h).  The vectors go into the
// buffers the cycle itself uses (rounded to its type) and every launch is made by the member the cycle calls.
template <typename T>
void mg_probe_run(Ctx& c, int piece, int l, const double* b, const double* x, double* out, double* rz) {
  const int Lv = (int)c.mg.size() - 1;
  auto size_of = [&](int lv) { return (i64)c.mg[lv].ord.new2old.size(); };
  // a level's vector in the level's own ordering, rounded to / widened from the cycle's type
  auto up = [&](int lv, const double* src, auto* dst) { c.put(c.mg[lv].ord, 0, size_of(lv), 1, 1, src, dst); };
  auto down = [&](int lv, const T* src) { c.get(c.mg[lv].ord, 0, size_of(lv), 1, 1, out, src); };
  // the right-hand side of level lv where the cycle reads it
  auto rhs = [&](int lv) -> T* {
    if (lv < Lv) return bufs<T>(c.mg[lv]).b;
    if constexpr (std::is_same<T, float>::value) return c.r32;
    else return c.cg_r[0];
  };
  auto zbuf = [&]() -> T* {
    if constexpr (std::is_same<T, float>::value) return c.z32;
    else return c.z;
  };
  MgBufs<T>& B = bufs<T>(c.mg[l]);
  // the solves' control words: a converged solve leaves its flag set, and every cycle kernel returns at once then
  int ctl0[6];
  c.d2h(ctl0, c.ctl, sizeof(ctl0));
  HIPCHK(hipMemsetAsync(c.ctl, 0, 2 * sizeof(int), c.st));
  switch (piece) {
    case PUCFEM_MG_RESID:
      up(l, b, rhs(l));
      up(l, x, B.x);
      c.mg_resid<T, T>(l, rhs(l), (const T*)B.x);
      down(l, B.res);
      break;
    case PUCFEM_MG_SMOOTH0:
      up(l, b, rhs(l));
      down(l, c.mg_pre<T, T>(l, rhs(l)));
      break;
    case PUCFEM_MG_SMOOTHX:
      up(l, b, rhs(l));
      up(l, x, B.x);
      down(l, c.mg_post<T, T>(l, rhs(l), B.x, false, nullptr, nullptr));
      break;
    case PUCFEM_MG_RESTRICT:
      up(l, x, B.res);
      c.mg_restrict<T>(l);
      down(l - 1, bufs<T>(c.mg[l - 1]).b);
      break;
    case PUCFEM_MG_PROLONG:
      up(l - 1, b, bufs<T>(c.mg[l - 1]).x);
      up(l, x, B.x);
      c.mg_prolong<T>(l, bufs<T>(c.mg[l - 1]).x, B.x);
      down(l, B.x);
      break;
    case PUCFEM_MG_COARSE:
      up(0, b, rhs(0));
      down(0, c.mg_coarse<T>(rhs(0)));
      break;
    case PUCFEM_MG_CYCLE: {
      up(l, b, rhs(l));
      const T* r = c.vcycle<T, T>(l, rhs(l), nullptr, nullptr);
      down(l, r ? r : zbuf());  // (the finest level's last step writes z)
      break;
    }
    default: {  // PUCFEM_MG_PRECOND
      up(Lv, b, c.cg_r[0]);
      if constexpr (std::is_same<T, float>::value) up(Lv, b, c.r32);
      const Red red = c.precondition_rz(Ctx::grid_part(c.fP.part(), c.dPp));
      c.d2h(rz, red.p, sizeof(double));
      down(Lv, zbuf());
      break;
    }
  }
  HIPCHK(hipStreamSynchronize(c.st));
  c.h2d(c.ctl, ctl0, sizeof(ctl0));
  HIPCHK(hipStreamSynchronize(c.st));
}

extern "C" {

int pucfem_abi_version(void) { return PUCFEM_ABI_VERSION; }

const char* pucfem_last_error(const void* ctx) {
  return ctx ? static_cast<const Ctx*>(ctx)->err.c_str() : g_err.c_str();
}

int pucfem_device_count(int32_t* n) {
  return guard(nullptr, [&] {
    int k = 0;
    HIPCHK(hipGetDeviceCount(&k));
    *n = k;
  });
}

int pucfem_ctx_create(int32_t device, void** out) {
  return guard(nullptr, [&] {
    auto c = std::make_unique<Ctx>();
    c->device = device;
    c->host_only = device < 0;
    if (!c->host_only) {
      HIPCHK(hipSetDevice(device));
      HIPCHK(hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking));
      HIPCHK(hipHostMalloc((void**)&c->h_ctl, 8 * sizeof(int), hipHostMallocDefault));
      HIPCHK(hipHostMalloc((void**)&c->h_coef, 5 * Ctx::NCOEF * sizeof(double), hipHostMallocDefault));
      HIPCHK(hipHostMalloc((void**)&c->h_pinned, 64 * sizeof(double), hipHostMallocDefault));
    }
    *out = c.release();
  });
}

int pucfem_rccl_unique_id(uint8_t* out) {
  return guard(nullptr, [&] {
    ncclUniqueId id;
    NCCLCHK(ncclGetUniqueId(&id));
    static_assert(sizeof(ncclUniqueId) == PUCFEM_UNIQUE_ID_BYTES, "unique id size");
    std::memcpy(out, &id, sizeof(id));
  });
}

int pucfem_ctx_create_dist(int32_t device, int32_t rank, int32_t world, const uint8_t* uid, void** out) {
  void* p = nullptr;
  int rc = pucfem_ctx_create(device, &p);
  if (rc) return rc;
  rc = guard(p, [&] {
    Ctx& c = *C(p);
    require(world >= 1 && rank >= 0 && rank < world, "bad rank / world");
    c.rank = rank;
    c.world = world;
    static const char kLocal[] = "PUCFEM-LOCALCOMM";
    const bool local = std::memcmp(uid, kLocal, sizeof(kLocal) - 1) == 0;
    if (!c.host_only && (world > 1 || !local)) {
      if (local) {
        // test backend: W ranks as W contexts (host threads) of one process
        c.comm = std::make_unique<LocalComm>(std::string((const char*)uid, PUCFEM_UNIQUE_ID_BYTES), world, rank);
      } else {
        ncclUniqueId id;
        std::memcpy(&id, uid, sizeof(id));
        try {
          c.comm = std::make_unique<NcclComm>(world, id, rank);
        } catch (const std::exception& e) {
          throw Error(PUCFEM_ENCCL, e.what());
        }
      }
    }
  });
  if (rc) {
    g_err = C(p)->err;
    delete C(p);
    return rc;
  }
  *out = p;
  return 0;
}

int pucfem_ctx_destroy(void* ctx) {
  return guard(nullptr, [&] { delete C(ctx); });
}

int pucfem_mesh_upload(void* ctx, int64_t N, const double* xy, const int32_t* mk, int64_t T, const int32_t* tris,
                       int32_t coord_fp32) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    require(N > 0 && T > 0 && xy && mk && tris, "empty mesh");
    HostMesh& m = c.mesh;
    m.N = N;
    m.T = T;
    m.x.resize(N);
    m.y.resize(N);
    for (i64 i = 0; i < N; ++i) {
      m.x[i] = xy[2 * i];
      m.y[i] = xy[2 * i + 1];
    }
    m.mk.assign(mk, mk + N);
    m.tri.assign(tris, tris + 3 * T);
    bool ok = true;
    for (i64 k = 0; k < 3 * T; ++k) ok &= m.tri[k] >= 0 && m.tri[k] < N;
    require(ok, "triangle index out of range");
    m.fp32 = coord_fp32 != 0;
    c.has_mesh = true;
    c.built = false;
    c.surf_valid = false;
  });
}

int pucfem_set_pairs(void* ctx, int32_t kind, int64_t n, const int64_t* pairs) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    require(c.has_mesh, "mesh first");
    auto& v = kind == 0 ? c.op_pairs : c.bc_pairs;
    v.clear();
    for (i64 k = 0; k < n; ++k) {
      require(pairs[2 * k] >= 0 && pairs[2 * k] < c.mesh.N && pairs[2 * k + 1] >= 0 && pairs[2 * k + 1] < c.mesh.N,
              "pair index out of range");
      v.push_back({pairs[2 * k], pairs[2 * k + 1]});
    }
    c.built = false;
  });
}

int pucfem_set_dirichlet(void* ctx, int64_t n, const int32_t* nodes, const double* values, int32_t ncomp) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    require(c.has_mesh, "mesh first");
    require(ncomp == 1 || ncomp == 2, "ncomp must be 1 or 2");
    c.dir_nodes.assign(nodes, nodes + n);
    for (i32 d : c.dir_nodes) require(d >= 0 && d < c.mesh.N, "Dirichlet node out of range");
    c.dir_vals.assign(values, values + ncomp * n);
    c.dir_ncomp = ncomp;
    c.built = false;
  });
}

int pucfem_set_hierarchy(void* ctx, int64_t N0, const double* xy0, const int32_t* mk0, int64_t T0,
                         const int32_t* tris0, int32_t levels) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    require(levels >= 0 && levels <= 12, "levels in [0, 12]");
    require(N0 > 0 && T0 > 0, "empty coarse mesh");
    HostMesh& m = c.coarse;
    m.N = N0;
    m.T = T0;
    m.x.resize(N0);
    m.y.resize(N0);
    for (i64 i = 0; i < N0; ++i) {
      m.x[i] = xy0[2 * i];
      m.y[i] = xy0[2 * i + 1];
    }
    m.mk.assign(mk0, mk0 + N0);
    m.tri.assign(tris0, tris0 + 3 * T0);
    for (i64 k = 0; k < 3 * T0; ++k) require(m.tri[k] >= 0 && m.tri[k] < N0, "coarse triangle index out of range");
    c.mg_levels = levels;
    c.built = false;
  });
}

int pucfem_set_source(void* ctx, int64_t T, const float* g) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    require(c.has_mesh && T == c.mesh.T, "source must have one value per triangle");
    c.g_tri.assign(g, g + T);
    c.built = false;
  });
}

int pucfem_build_operators(void* ctx, const pucfem_params* prm) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    c.prm = *prm;
    c.built = false;
    if (c.ens) {  // (an ensemble lives on the operators being replaced)
      (void)hipStreamSynchronize(c.st);
      c.ens.reset();
    }
    c.drop_step_graphs();
    if (!c.host_only) c.drop_dyes();
    if (!c.host_only) c.drop_inertia();
    if (!c.host_only) c.drop_force();
    if (!c.host_only) c.drop_stroke(false);
    if (!c.host_only) c.drop_advection();
    if (!c.host_only) c.drop_trajectory();
    if (!c.host_only) c.drop_stretch();
    if (!c.host_only) c.drop_loads();
    build(c);
  });
}

// ---- fields
int pucfem_set_field(void* ctx, int32_t field, const double* buf, int64_t count) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    const bool dyef = field == PUCFEM_F_DYES || (field >= PUCFEM_F_DYE0 && field < PUCFEM_F_DYE0 + DYE_MAX);
    if (dyef) c.dye_ready();
    if (field == PUCFEM_F_DEFGRAD && !c.str_on)
      throw Error(PUCFEM_ESTATE, "tracer stretching is off: there is no deformation gradient (pucfem_set_tracer_stretch)");
    c.need_dev();
    c.need_built();
    const i64 N = c.mesh.N, no = c.lp.n_own;
    if (dyef) {
      if (field == PUCFEM_F_DYES) {
        require(count >= 0 && count % N == 0, "dyes must be (K, N)");
        require(count / N <= DYE_MAX, "at most PUCFEM_MAX_DYES (16) dye channels");
        require(count == 0 || buf != nullptr, "null dyes");
        c.set_dyes((int)(count / N), buf);
      } else {
        const int k = field - PUCFEM_F_DYE0;
        require(k < c.ndye, "dye channel index >= the number of channels");
        require(count == N && buf != nullptr, "a dye channel must be (N,)");
        c.put_all(1, 1, buf, c.dye_cur + (size_t)k * N);
        HIPCHK(hipStreamSynchronize(c.st));
      }
      return;
    }
    auto own2 = [&](double* a) {  // (the interleaved velocity: a = its pairs)
      require(count == 2 * N, "field must be (N, 2)");
      c.put(c.ord, c.lp.r0, no, 2, 1, buf, a, (double*)nullptr, false);
      HIPCHK(hipStreamSynchronize(c.st));
      c.halo_v(a);
    };
    switch (field) {
      case PUCFEM_F_U:
        own2(c.ux);
        c.have_vinc = 0;  // a new state: no last viscous increment
        break;
      case PUCFEM_F_USTAR: own2(c.usx); break;
      case PUCFEM_F_SCALAR:
        require(count == N, "field must be (N,)");
        c.put(c.ord, c.lp.r0, no, 1, 1, buf, c.scalar);
        c.halo(c.scalar);
        break;
      case PUCFEM_F_C:
        require(count == N, "c must be (N,)");
        c.put(c.ord, 0, N, 1, 1, buf, c.c_full, (double*)nullptr, false);
        break;
      case PUCFEM_F_TRACERS: {
        require(count % 2 == 0, "tracers must be (n, 2)");
        const i64 n = count / 2;
        require(n <= INT32_MAX, "at most 2^31 - 1 tracers");
        if (n != c.ntr || !c.trcap) {
          c.ntr = (int32_t)n;
          c.trx = c.dalloc<double>(n);
          c.try_ = c.dalloc<double>(n);
          c.trs = c.dalloc<double>(n);
          c.trcap = c.dalloc<int32_t>(n);
          if (c.dist()) c.trv = c.dalloc<double>(3 * n);
          HIPCHK(hipStreamSynchronize(c.st));
          c.drop_step_graphs();  // (they hold the old arrays and count)
        }
        if (!c.trstep) {
          c.trstep = c.dalloc<int32_t>(1);
          c.part_tr = c.dalloc<double>(TRACER_CLOUD_MAXB);
          c.trcensus = c.dalloc<unsigned long long>(2);
        }
        tracers_put(c, c.trx, c.try_, c.trs, c.trcap, c.trstep, 1, 0, n, buf);
        if (c.str_on) c.stretch_fit();  // (new tracers: F is the identity again, and its step count 0)
        break;
      }
      case PUCFEM_F_STATUS:
        require(count == c.ntr, "status must match the tracer count");
        c.h2d(c.trs, buf, sizeof(double) * count);
        break;
      case PUCFEM_F_DEFGRAD:  // (a run resumed: the rows as they were read; the step count stays)
        require(count == 4 * (i64)c.ntr, "the deformation gradient must be (n, 4)");
        if (count > 0) c.h2d(c.str_F, buf, sizeof(double) * count);
        break;
      default: throw Error(PUCFEM_EINVAL, "field cannot be set");
    }
    HIPCHK(hipStreamSynchronize(c.st));
  });
}

int pucfem_get_field(void* ctx, int32_t field, double* buf, int64_t count) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    const bool dyef = field == PUCFEM_F_DYES || (field >= PUCFEM_F_DYE0 && field < PUCFEM_F_DYE0 + DYE_MAX);
    if (dyef) c.dye_ready();
    if (field == PUCFEM_F_DEFGRAD && !c.str_on)
      throw Error(PUCFEM_ESTATE, "tracer stretching is off: there is no deformation gradient (pucfem_set_tracer_stretch)");
    c.need_dev();
    c.need_built();
    const i64 N = c.mesh.N, no = c.lp.n_own;
    if (dyef) {  // K x N, or channel k alone, into the caller's numbering
      const int k0 = field == PUCFEM_F_DYES ? 0 : field - PUCFEM_F_DYE0;
      const int nk = field == PUCFEM_F_DYES ? c.ndye : 1;
      require(k0 < c.ndye || field == PUCFEM_F_DYES, "dye channel index >= the number of channels");
      require(count == (i64)nk * N, field == PUCFEM_F_DYES ? "dyes are (K, N)" : "a dye channel is (N,)");
      if (nk == 0) return;
      require(buf != nullptr, "null output");
      c.get_all(1, nk, buf, c.dye_cur + (size_t)k0 * N);
      return;
    }
    switch (field) {
      case PUCFEM_F_P:
      case PUCFEM_F_P2:
      case PUCFEM_F_DIV_STAR:
      case PUCFEM_F_DIV_U:
      case PUCFEM_F_FINAL_DIV:
      case PUCFEM_F_VORTICITY:
      case PUCFEM_F_SCALAR: {  // one component, formed first (in place) when the step does not store it
        const double* a = c.formed(field, [&] {
          return field == PUCFEM_F_P           ? c.p
                 : field == PUCFEM_F_P2        ? c.p2
                 : field == PUCFEM_F_DIV_STAR  ? c.div_star
                 : field == PUCFEM_F_FINAL_DIV ? c.final_div
                                               : c.smp_scratch<double>(8, (size_t)c.nloc);
        });
        require(count == N, "field is (N,)");
        c.get(c.ord, c.lp.r0, no, 1, 1, buf, a);
        break;
      }
      case PUCFEM_F_U:
      case PUCFEM_F_USTAR:  // (the interleaved velocity)
        require(count == 2 * N, "field is (N, 2)");
        c.get(c.ord, c.lp.r0, no, 2, 1, buf, (const double*)(field == PUCFEM_F_U ? c.ux : c.usx), (const double*)nullptr, false);
        break;
      case PUCFEM_F_U_ADV:  // (the u_a of the last inertial step)
        c.inertia_ready();
        if (!c.adv_valid) throw Error(PUCFEM_ESTATE, "no inertial step has been taken: u_adv holds nothing");
        require(count == 2 * N, "field is (N, 2)");
        c.get(c.ord, c.lp.r0, no, 2, 1, buf, (const double*)c.u_adv, (const double*)nullptr, false);
        break;
      case PUCFEM_F_FORCE: {  // (the total f of the current state, formed when read; the owned rows)
        c.force_ready();
        require(count == 2 * N, "field is (N, 2)");
        double* s = c.smp_scratch<double>(15, 2 * (size_t)no);
        c.sl_join();
        c.force_launch<false>(nullptr, 0.0, s);
        c.get(c.ord, c.lp.r0, no, 2, 1, buf, (const double*)s, (const double*)nullptr, false);
        break;
      }
      case PUCFEM_F_U_RHS:  // (the r of the last forced step)
        c.force_ready();
        if (!c.rhs_valid) throw Error(PUCFEM_ESTATE, "no forced step has been taken: u_rhs holds nothing");
        require(count == 2 * N, "field is (N, 2)");
        c.get(c.ord, c.lp.r0, no, 2, 1, buf, (const double*)c.u_rhs, (const double*)nullptr, false);
        break;
      case PUCFEM_F_C:
        require(count == N, "c is (N,)");
        c.allgather_full(c.c_full);  // multi-rank: collective (every rank reads c), the full field
        c.get(c.ord, 0, N, 1, 1, buf, (const double*)c.c_full, (const double*)nullptr, false);
        break;
      case PUCFEM_F_TRACERS:
        require(count == 2 * (i64)c.ntr, "tracers are (n, 2)");
        tracers_get(c, c.trx, c.try_, 0, c.ntr, buf);
        break;
      case PUCFEM_F_STATUS:
        require(count == c.ntr, "status is (n,)");
        c.d2h(buf, c.trs, sizeof(double) * count);
        break;
      case PUCFEM_F_CAPTURE_STEP:
        require(count == c.ntr, "capture steps are (n,)");
        capture_steps_get(c, c.trcap, 0, c.ntr, buf);
        break;
      case PUCFEM_F_DEFGRAD:
        require(count == 4 * (i64)c.ntr, "the deformation gradient is (n, 4)");
        if (count > 0) c.d2h(buf, c.str_F, sizeof(double) * count);
        break;
      default: throw Error(PUCFEM_EINVAL, "unknown field");
    }
  });
}

// ---- stepping
int pucfem_step(void* ctx, int32_t nsteps, pucfem_step_stats* stats) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    c.need_dev();
    c.need_built();
    require(nsteps >= 0, "nsteps < 0");
    if (nsteps == 0) return;
    if (c.scheme == PUCFEM_STOKES_COLOR || c.scheme == PUCFEM_STOKES_FOOD) {
      double* rec = c.dalloc<double>(8 * (i64)nsteps);
      int* dits = c.dalloc<int>(3 * (i64)nsteps);
      std::vector<int32_t> its(3 * (size_t)nsteps);
      // (a context with dye channels steps uncaptured: the channels' buffers swap every step; so does one with
      // inertia on: the captured step has no inertial launch, and a toggle takes effect at the next step; so does one
      // whose dye moves by MacCormack steps, and one with a body force: the same launches behind k_force_rhs, whose
      // by-value terms and dye pointers change between steps; and one with a stroke: the same launches behind
      // k_stroke_bc, so that the captured graphs stay the unstroked step's, launch for launch; and one with a
      // midpoint trajectory on: the captured graphs hold the Euler launches; and one whose loads record is on: the same
      // launches in front of k_loads, so that the captured graphs stay the unrecorded step's; and one with tracer
      // stretching on: the captured graphs hold the plain tracer launch)
      if (c.dense && !c.timer.on && !c.dye_impl && c.ndye == 0 && !c.inertia && !c.adv_dye && !c.forced() &&
          !c.stroked() && !c.trj_any() && c.ld_cap == 0 && !c.str_on) {
        // direct-solve small-mesh path: every step is the same sequence of ~25 launches with no
        // host synchronisation -> capture it once (and GK steps of it once), replay them
        // capture `count` consecutive steps into one graph (the steps' buffers are fixed in graph mode)
        auto capture = [&](int count, hipGraph_t& gr, hipGraphExec_t& ex) {
          int32_t tmp[3];
          HIPCHK(hipStreamBeginCapture(c.st, hipStreamCaptureModeThreadLocal));
          try {
            c.gcapture = true;
            for (int k = 0; k < count; ++k) c.stokes_step(c.gstats, tmp);
            c.gcapture = false;
          } catch (...) {
            c.gcapture = false;
            hipGraph_t g;
            (void)hipStreamEndCapture(c.st, &g);
            c.graph_mode = c.gexec != nullptr;
            throw;
          }
          HIPCHK(hipStreamEndCapture(c.st, &gr));
          HIPCHK(hipGraphInstantiate(&ex, gr, nullptr, nullptr, 0));
        };
        c.prep_grad_proj_bc();
        if (!c.gexec) {
          c.gstats = c.dalloc<double>(8);
          c.gring = c.dalloc<double>(8 * (i64)Ctx::GRING);
          c.gcount = c.dalloc<int>(1);
          HIPCHK(hipStreamSynchronize(c.st));
          c.graph_mode = true;
          capture(1, c.graph, c.gexec);
        }
        if (!c.gexec_k && c.gk > 1 && nsteps >= c.gk) capture(c.gk, c.graph_k, c.gexec_k);
        HIPCHK(hipMemsetAsync(c.gcount, 0, sizeof(int), c.st));
        for (int s = 0, k = 0; s < nsteps;) {
          int d = 1;
          if (c.gexec_k && nsteps - s >= c.gk && k + c.gk <= Ctx::GRING) {
            HIPCHK(hipGraphLaunch(c.gexec_k, c.st));
            d = c.gk;
          } else {
            HIPCHK(hipGraphLaunch(c.gexec, c.st));
          }
          s += d;
          k += d;
          if (k == Ctx::GRING || s == nsteps) {  // the ring's records -> this call's records
            HIPCHK(hipMemcpyAsync(rec + 8 * (s - k), c.gring, sizeof(double) * 8 * k, hipMemcpyDeviceToDevice, c.st));
            if (s < nsteps) HIPCHK(hipMemsetAsync(c.gcount, 0, sizeof(int), c.st));
            k = 0;
          }
        }
      } else {
        c.graph_mode = c.gexec != nullptr;  // once captured, keep c in its fixed buffer
        c.dits = dits;
        c.prep_grad_proj_bc();
        try {
          for (int s = 0; s < nsteps; ++s) {
            c.cur_step = s;
            c.stokes_step(rec + 8 * s, its.data() + 3 * s);
          }
          c.proj_materialize();  // (no direction stays pending between API calls)
          c.dye_tail_dist();     // (nor a dye tail: the last step's, now)
          c.sl_join();
        } catch (...) {
          c.dits = nullptr;
          if (c.sl_pending) (void)hipStreamSynchronize(c.st_sl);
          c.sl_pending = false;
          c.tail_pend = false;
          throw;
        }
        c.dits = nullptr;
      }
      std::vector<double> h(8 * (size_t)nsteps);
      std::vector<int> hd(3 * (size_t)nsteps);
      HIPCHK(hipMemcpyAsync(h.data(), rec, sizeof(double) * h.size(), hipMemcpyDeviceToHost, c.st));
      HIPCHK(hipMemcpyAsync(hd.data(), dits, sizeof(int) * hd.size(), hipMemcpyDeviceToHost, c.st));
      HIPCHK(hipStreamSynchronize(c.st));
      if (c.timer.on) c.timer.flush();
      for (void* q : {(void*)rec, (void*)dits}) {
        HIPCHK(hipFree(q));
        c.allocs.erase(std::find(c.allocs.begin(), c.allocs.end(), q));
      }
      for (size_t k = 0; k < its.size(); ++k)
        if (its[k] < 0) {
          if (hd[k] < 0) throw Error(PUCFEM_ENOCONV, "single-workgroup CG did not converge (step " +
                                                         std::to_string(k / 3) + ")");
          its[k] = hd[k];
        }
      if (stats)
        for (int s = 0; s < nsteps; ++s) {
          pucfem_step_stats& o = stats[s];
          const double* r = h.data() + 8 * s;
          o.max_div_star = r[0];
          o.max_final_div = r[1];
          o.mix_I = r[2];
          o.mix_mu = r[3];
          o.mix_var = r[4];
          o.eaten = (int64_t)std::llround(r[5]);
          o.sl_notfound = (int32_t)std::llround(r[6]);
          o.it_visc = its[3 * s];
          o.it_p = its[3 * s + 1];
          o.it_p2 = its[3 * s + 2];
        }
    } else if (c.scheme == PUCFEM_HEAT) {
      // heatEq.py:321-325: u = solve(A, u + DT*b*0); reapply_periodic_u; reapply_dirchlect_u
      const i64 n = c.lp.n_own;
      for (int s = 0; s < nsteps; ++s) {
        int it = 0;
        if (c.dLitInv) {  // small mesh: u = A^-1 u (one launch, no host synchronisation)
          hipLaunchKernelGGL(k_dense_mv<double>, dim3((int)std::min<i64>(2048, (n + 3) / 4)), dim3(BS), 0, c.st, n,
                             (const double*)c.dLitInv, (const double*)c.scalar, c.litw[8], (const int*)nullptr);
          KCHK();
          std::swap(c.scalar, c.litw[8]);
        } else {
          HIPCHK(hipMemcpyAsync(c.litw[8], c.scalar, sizeof(double) * n, hipMemcpyDeviceToDevice, c.st));
          it = c.bicgstab(c.scalar, c.litw[8], c.prm.rtol_lin, c.prm.maxit_lin);
        }
        c.bc(c.scalar, nullptr);
        if (stats) {
          std::memset(&stats[s], 0, sizeof(pucfem_step_stats));
          stats[s].it_visc = it;
        }
      }
      HIPCHK(hipStreamSynchronize(c.st));
    } else {
      // poisson.py:283-285: f = solve(A, b)
      HIPCHK(hipMemcpyAsync(c.bh, c.litb.data(), sizeof(double) * c.lp.n_own, hipMemcpyHostToDevice, c.st));
      HIPCHK(hipMemsetAsync(c.scalar, 0, sizeof(double) * c.lp.n_own, c.st));
      int it = 0;
      if (c.dLitInv) {
        hipLaunchKernelGGL(k_dense_mv<double>, dim3((int)std::min<i64>(2048, (c.lp.n_own + 3) / 4)), dim3(BS), 0, c.st,
                           (int64_t)c.lp.n_own, (const double*)c.dLitInv, (const double*)c.bh, c.scalar,
                           (const int*)nullptr);
        KCHK();
      } else {
        it = c.bicgstab(c.scalar, c.bh, c.prm.rtol_lin, c.prm.maxit_lin);
      }
      HIPCHK(hipStreamSynchronize(c.st));
      if (stats) {
        std::memset(&stats[0], 0, sizeof(pucfem_step_stats));
        stats[0].it_visc = it;
      }
    }
  });
}

// ---- ensembles: M members on the context's shared small-mesh operators (kernels: pucfem_ensemble.hpp)
namespace {
Ens* ens_of(Ctx& c) {
  c.need_dev();
  c.need_built();
  if (!c.ens) throw Error(PUCFEM_ESTATE, "no ensemble on this context: call pucfem_ens_create first");
  return c.ens.get();
}
// The dye's launches of a step while the ensemble carries channels (e.dy_K > 0): per dye flag with members on it, the
// with-channels form of the launches ens_enqueue_step makes without channels -- the same buffers, partials, ticket
// counters and value slots for c, the channels beside it -- then the channels' next set copied into their current
// set.  Every member is on exactly one flag, so every plane of the next set is written.  rs: k_ens_sl's reduction.
void ens_enqueue_dyes(Ctx& c, Ens& e, const EnsTransport& t, const RedOut& rs, bool dye_alt) {
  const i64 n = e.n;
  const int32_t M = e.M, K = e.dy_K;
  hipStream_t st = c.st;
  const MeshDev Mh{c.mx, c.my, c.mtri, c.mesh.T};
  const dim3 grid(e.nb_sl, M);
  const double dt = c.prm.dt, hdt = 0.5 * c.prm.dt;
  const int32_t* on = dye_alt ? (const int32_t*)e.mc_on_dev : (const int32_t*)nullptr;
  const double *cc = e.c, *dy = e.dy_cur, *wm = c.dwmix, *nowm = nullptr;
  hipLaunchKernelGGL(k_ens_dye_fwd<false>, grid, dim3(BS), 0, st, Mh, c.lgrid, c.cgrid, (int64_t)n, (const double*)e.u,
                     dt, hdt, on, ENS_DYE_SL, K, cc, dy, e.cn, e.dy_nxt, (int4*)nullptr, wm, e.part_sl, rs);
  KCHK();
  if (e.dye_n[ENS_DYE_MC] > 0) {
    hipLaunchKernelGGL(k_ens_dye_fwd<false>, grid, dim3(BS), 0, st, Mh, c.lgrid, c.cgrid, (int64_t)n,
                       (const double*)e.u, dt, hdt, on, ENS_DYE_MC, K, cc, dy, e.mc_ch, e.dy_ch, e.mc_rec, nowm,
                       e.mc_part, t.mc1());
    KCHK();
    hipLaunchKernelGGL(k_ens_dye_bwd<false>, grid, dim3(BS), 0, st, Mh, c.lgrid, c.cgrid, (int64_t)n,
                       (const double*)e.u, dt, hdt, on, ENS_DYE_MC, K, cc, (const double*)e.mc_ch, dy,
                       (const double*)e.dy_ch, e.cn, e.dy_nxt, (const int4*)e.mc_rec, t.mc_part2(), t.mc2(),
                       (double*)nullptr);
    KCHK();
  }
  if (e.dye_n[ENS_DYE_SL_MID] > 0) {
    hipLaunchKernelGGL(k_ens_dye_fwd<true>, grid, dim3(BS), 0, st, Mh, c.lgrid, c.cgrid, (int64_t)n, (const double*)e.u,
                       dt, hdt, on, ENS_DYE_SL_MID, K, cc, dy, e.cn, e.dy_nxt, (int4*)nullptr, nowm, e.trj_part_d,
                       t.trj1());
    KCHK();
  }
  if (e.dye_n[ENS_DYE_MC_MID] > 0) {
    hipLaunchKernelGGL(k_ens_dye_fwd<true>, grid, dim3(BS), 0, st, Mh, c.lgrid, c.cgrid, (int64_t)n, (const double*)e.u,
                       dt, hdt, on, ENS_DYE_MC_MID, K, cc, dy, e.mc_ch, e.dy_ch, e.mc_rec, nowm, e.trj_part_d,
                       t.trj1());
    KCHK();
    hipLaunchKernelGGL(k_ens_dye_bwd<true>, grid, dim3(BS), 0, st, Mh, c.lgrid, c.cgrid, (int64_t)n, (const double*)e.u,
                       dt, hdt, on, ENS_DYE_MC_MID, K, cc, (const double*)e.mc_ch, dy, (const double*)e.dy_ch, e.cn,
                       e.dy_nxt, (const int4*)e.mc_rec, t.trj_part2(), t.trj2(), t.v_mc);
    KCHK();
  }
  const int64_t count = (int64_t)M * K * n;
  hipLaunchKernelGGL(k_ens_dye_copy, dim3(Ctx::grid_ew(count)), dim3(BS), 0, st, count, (const double*)e.dy_nxt,
                     e.dy_cur);
  KCHK();
}
// the ensemble's loads buffers, allocated at first use and kept
void ens_loads_bufs(Ctx& c, Ens& e) {
  c.loads_bufs();
  if (e.ld_part) return;
  const size_t sM = (size_t)e.M;
  e.ld_part = e.alloc<double>(sM * LOADS_NV * c.loads_grid(), c.st);
  e.ld_out = e.alloc<double>(sM * ENS_VALS, c.st);
  e.ld_eout = e.alloc<double>(sM * LOADS_EV * (size_t)c.ld_nE, c.st);
  e.ld_cnt = e.alloc<unsigned>(sM, c.st);
}
// k_loads over members m0 .. m0 + nm - 1 of their current u, p and p2: the values into the members' e.ld_out, with
// `store` the per-edge values into their e.ld_eout; rec: the record (its ring and counts are the whole ensemble's, so
// only with m0 = 0)
void ens_loads(Ctx& c, Ens& e, int32_t m0, int32_t nm, bool store, const LoadsRec& rec) {
  ens_loads_bufs(c, e);
  const size_t m = (size_t)m0;
  const RedOut r{e.ld_out + m * ENS_VALS, nullptr, e.ld_cnt + m, LOADS_NV, 0, 0u};
  c.loads_launch(nm, e.u + m * 2 * e.n, 2 * e.n, e.p + m * e.n, e.p2 + m * e.n, e.n, nullptr,
                 store ? e.ld_eout + m * LOADS_EV * (size_t)c.ld_nE : nullptr,
                 e.ld_part + m * LOADS_NV * (size_t)c.loads_grid(), r, rec);
}
// the record's ring of the ensemble follows the context's setting (pucfem_set_loads_record may come before or after
// pucfem_ens_create): a changed capacity makes a fresh ring, zero rows recorded
void ens_loads_ring_fit(Ctx& c, Ens& e, bool reset) {
  if (e.ld_cap == c.ld_cap && !reset) return;
  HIPCHK(hipStreamSynchronize(c.st));
  e.drop_graphs();  // (the ring's address and capacity are arguments of the captured launch)
  e.drop_loads_ring();
  if (c.ld_cap > 0) {
    ens_loads_bufs(c, e);
    e.ld_ring = c.loads_alloc<double>((size_t)e.M * c.ld_cap * LOADS_ROW);
    e.ld_count = c.loads_alloc<int64_t>((size_t)e.M);
    e.ld_cap = c.ld_cap;
    HIPCHK(hipStreamSynchronize(c.st));
  }
}
// One ensemble step: the dense small-mesh step's launches (Ctx::stokes_step in graph mode), each over every member,
// in one chain on the context's stream.
void ens_enqueue_step(Ctx& c) {
  Ens& e = *c.ens;
  const i64 n = e.n;
  const int32_t M = e.M;
  const int tiles = (M + ENS_TM - 1) / ENS_TM;
  hipStream_t st = c.st;
  const DevSell& A = c.dP;
  // with at least one member's inertia on: u_a = SL(u^n; u^n, dt) of those members in front, and the viscous product
  // takes it as their input (Ctx::inertia_step / Ctx::viscous of the single path)
  const bool adv = e.adv_any > 0;
  // with at least one member stroked: those members' boundary values of this step in front of everything
  // (Ctx::stroke_step), one block per member; the rows come from the members' counters in device memory
  if (e.stroke_any > 0) {
    hipLaunchKernelGGL(k_ens_stroke_bc, dim3(M), dim3(BS), 0, st, 0, (const int64_t*)e.sk_parm, e.sk_ctr, (int64_t)-1,
                       (const double*)e.sk_tab, e.sk_n, (const int32_t*)e.sk_q, (const double*)e.sk_shape,
                       reinterpret_cast<const dbl2*>(e.sk_dir), e.dval, (int64_t)e.dstride);
    KCHK();
  }
  if (adv) {
    const RedOut ra{e.vals + ENS_V_VEL_NF, nullptr, e.cnt_adv, 1, 0, 0u};
    hipLaunchKernelGGL(k_ens_sl_vel, dim3(e.nb_sl, M), dim3(BS), 0, st, MeshDev{c.mx, c.my, c.mtri, c.mesh.T}, c.lgrid,
                       c.cgrid, (int64_t)n, (const double*)e.u, c.prm.dt, (const int32_t*)e.adv_on_dev, e.ua,
                       e.part_adv, ra);
    KCHK();
    // the inertial members whose velocity moves by MacCormack, along the midpoint trace or both (flags ENS_ADV_MC,
    // ENS_ADV_SL_MID, ENS_ADV_MC_MID, which k_ens_sl_vel skips): u_a of those members into their planes of ua
    ens_transport(c, e, ens_vel_transport(e), reinterpret_cast<const dbl2*>(e.u), reinterpret_cast<dbl2*>(e.ua));
  }
  // with at least one member forced: r = base + dt * f of those members behind it (Ctx::force_step), and the viscous
  // product stages r for them.  c holds c^n: k_ens_mix2 of the previous step wrote it earlier in this chain
  const bool forced = e.force_any > 0;
  if (forced) {
    hipLaunchKernelGGL(k_ens_force_rhs<true>, dim3(Ctx::grid_ew(n), M), dim3(BS), 0, st, (int64_t)n,
                       (const int32_t*)e.fmask_dev, (const double*)e.fparm, reinterpret_cast<const dbl2*>(e.fnod),
                       reinterpret_cast<const dbl2*>(e.u), reinterpret_cast<const dbl2*>(e.ua),
                       adv ? (const int32_t*)e.adv_on_dev : (const int32_t*)nullptr, (const double*)e.c, c.prm.dt,
                       reinterpret_cast<dbl2*>(e.frhs));
    KCHK();
  }
  hipLaunchKernelGGL(k_ens_mv2_bc<ENS_TM>, dim3(e.gx_dense, tiles), dim3(BS), e.lds_mv, st, (int64_t)n, M,
                     (const double*)c.dVinv, (const double*)e.u, e.us, (const int32_t*)c.dbcsrc,
                     (const int32_t*)c.dbcdir, (const double*)e.dval, (int64_t)e.dstride,
                     adv ? (const double*)e.ua : (const double*)nullptr,
                     adv ? (const int32_t*)e.adv_on_dev : (const int32_t*)nullptr,
                     forced ? (const double*)e.frhs : (const double*)nullptr,
                     forced ? (const int32_t*)e.fmask_dev : (const int32_t*)nullptr);
  KCHK();
  // max |div| into vals slot `slot`; with rhs the pressure right-hand side and its sum (slot 9)
  auto div = [&](const double* u, int slot, bool rhs) {
    const RedOut r{e.vals + slot, rhs ? e.vals + ENS_V_BSUM : nullptr, e.cnt, rhs ? 2 : 1, 0, 1u};
    with_c16(A, [&](auto c16) {
      hipLaunchKernelGGL(k_ens_div<decltype(c16)::value>, dim3(e.nb_div, M), dim3(BS), 0, st, A.view(),
                         (const double*)c.dGx, (const double*)c.dGy, u, (const double*)c.das1, (const double*)c.dmp,
                         -(1.0 / c.prm.dt), rhs ? e.braw : (double*)nullptr, e.part_d, r);
    });
    KCHK();
  };
  auto pres = [&](double* pout) {
    hipLaunchKernelGGL(k_ens_pres<ENS_TM>, dim3(e.gx_dense, tiles), dim3(BS), e.lds_pres, st, (int64_t)n, M,
                       (const double*)c.dPinv, (const double*)e.braw, (const int32_t*)c.dslave_of,
                       (const int32_t*)c.dmaster_of, (const double*)e.vals, 1.0 / (double)c.n_free, pout);
    KCHK();
  };
  div(e.us, ENS_V_DIV_STAR, true);
  pres(e.p);
  const int nbg = (int)std::max<i64>(1, std::min<i64>(1024, (A.nslices * 64 + BS - 1) / BS));
  with_c16(A, [&](auto c16) {
    hipLaunchKernelGGL(k_ens_grad_proj_bc<decltype(c16)::value>, dim3(nbg, M), dim3(BS), 0, st, A.view(),
                       (const double*)c.dGx, (const double*)c.dGy, (const double*)e.p, (const double*)c.das1, c.prm.dt,
                       (const double*)e.us, e.u, (const int32_t*)c.dbcsrc, (const int32_t*)c.dbcdir,
                       (const int32_t*)c.dspos, (const double*)e.dval, (int64_t)e.dstride);
  });
  KCHK();
  div(e.u, ENS_V_SCRATCH, true);  // (its maximum is not recorded)
  pres(e.p2);
  with_c16(A, [&](auto c16) {
    hipLaunchKernelGGL(k_ens_grad_proj1<decltype(c16)::value>, dim3(c.nb_mg(A.nslices), M), dim3(BS), 0, st, A.view(),
                       (const double*)c.dGx, (const double*)c.dGy, (const double*)e.p2, (const double*)c.das1, c.prm.dt,
                       (const uint8_t*)c.ddir, e.u);
  });
  KCHK();
  div(e.u, ENS_V_FINAL_DIV, false);
  if (c.scheme == PUCFEM_STOKES_COLOR) {
    const RedOut rs{e.vals + ENS_V_SL, nullptr, e.cnt + M, 3, 0, 0u};
    // (a member whose dye flag is not 0 moves its dye below: by MacCormack, along the midpoint trace, or both)
    const bool dye_alt = e.dye_n[ENS_DYE_MC] + e.dye_n[ENS_DYE_SL_MID] + e.dye_n[ENS_DYE_MC_MID] > 0;
    // with dye channels (pucfem_ens_set_dyes): the with-channels kernels move c and the channels of every member from
    // one locate per pass and row, in place of the launches below up to the sums
    const EnsTransport td = ens_dye_transport(e);
    if (e.dy_K > 0)
      ens_enqueue_dyes(c, e, td, rs, dye_alt);
    else
      hipLaunchKernelGGL(k_ens_sl, dim3(e.nb_sl, M), dim3(BS), 0, st, MeshDev{c.mx, c.my, c.mtri, c.mesh.T}, c.lgrid,
                         c.cgrid, (int64_t)n, (const double*)e.u, c.prm.dt, (const double*)e.c, e.cn,
                         (const double*)c.dwmix, e.part_sl, rs,
                         dye_alt ? (const int32_t*)e.mc_on_dev : (const int32_t*)nullptr);
    KCHK();
    // the members whose dye left k_ens_sl: cn by MacCormack, along the midpoint trace or both, the final locate's
    // not-found count (pass 1's under MacCormack) into ENS_V_DYE_NF and the single path's k_wsum sums into ENS_V_SL
    // (Ctx::dye_transport_step / dye_transport_reduce)
    if (dye_alt) {
      if (e.dy_K == 0) ens_transport(c, e, td, (const double*)e.c, e.cn);
      const RedOut rw{e.vals + ENS_V_SL, nullptr, e.mc_cnt + 2 * (size_t)M, 2, 0, 0u};

      hipLaunchKernelGGL(k_ens_wsum, dim3(e.nb_ws, M), dim3(BS), 0, st, (int64_t)n, (const int32_t*)e.mc_on_dev,
                         (const double*)e.cn, (const double*)c.dwmix, e.mc_part_ws, rw);
      KCHK();
    }
    const RedOut rm{e.vals + ENS_V_MIX, nullptr, e.cnt + 2 * (size_t)M, 1, 0, 0u};
    hipLaunchKernelGGL(k_ens_mix2, dim3(e.nb_mix, M), dim3(BS), 0, st, (int64_t)n, (const double*)e.cn,
                       (const double*)c.dwmix, (const double*)e.vals, e.part_mx, rm, e.c);
    KCHK();
  } else if (e.ntr > 0) {
    // with at least one member's diffusion on: the BROWN instantiation of the same launch (which members walk, and
    // with what amplitude and key, the kernel reads from device memory)
    const MeshDev Mh{c.mx, c.my, c.mtri, c.mesh.T};
    const RedOut rt{e.vals + ENS_V_EATEN, nullptr, e.cnt + 3 * (size_t)M, 1, 0, 0u};
    auto launch = [&](auto brown, auto eb) {
      constexpr bool B = decltype(brown)::value;
      if (e.str_any > 0) {
        // with at least one member's stretching on: the STRETCH instantiation of whichever launch is due below (which
        // members carry F the kernel reads from device memory)
        const EnsStretch es{(const int32_t*)e.str_on_dev, e.str_F};
        if (e.trjt_any > 0) {
          const EnsMid em{(const int32_t*)e.trj_trc_dev, 0.5 * c.prm.dt, e.trj_vals + ENS_TRJ_FELL};
          const RedOut rm{e.vals + ENS_V_EATEN, e.trj_vals + ENS_TRJ_FELL, e.cnt + 3 * (size_t)M, 2, 0, 0u};
          if (e.nb_tr > 1)
            hipLaunchKernelGGL((k_ens_tracer_cloud<B, true, true>), dim3(e.nb_tr, M), dim3(BS), 0, st, Mh, c.tgrid,
                               (int64_t)n, (const double*)e.u, e.ntr, e.trx, e.try_, e.trs, e.trcap, e.trstep,
                               c.prm.dt, c.prm.center_x, c.prm.center_y, c.prm.capture_radius, e.part_tr, rm, eb, em,
                               es);
          else
            hipLaunchKernelGGL((k_ens_tracer<B, true, true>), dim3(1, M), dim3(BS), 0, st, Mh, c.tgrid, (int64_t)n,
                               (const double*)e.u, e.ntr, e.trx, e.try_, e.trs, e.trcap, e.trstep, c.prm.dt,
                               c.prm.center_x, c.prm.center_y, c.prm.capture_radius, e.vals, eb, em, es);
        } else if (e.nb_tr > 1) {
          hipLaunchKernelGGL((k_ens_tracer_cloud<B, false, true>), dim3(e.nb_tr, M), dim3(BS), 0, st, Mh, c.tgrid,
                             (int64_t)n, (const double*)e.u, e.ntr, e.trx, e.try_, e.trs, e.trcap, e.trstep, c.prm.dt,
                             c.prm.center_x, c.prm.center_y, c.prm.capture_radius, e.part_tr, rt, eb, EnsMidOff{}, es);
        } else {
          hipLaunchKernelGGL((k_ens_tracer<B, false, true>), dim3(1, M), dim3(BS), 0, st, Mh, c.tgrid, (int64_t)n,
                             (const double*)e.u, e.ntr, e.trx, e.try_, e.trs, e.trcap, e.trstep, c.prm.dt,
                             c.prm.center_x, c.prm.center_y, c.prm.capture_radius, e.vals, eb, EnsMidOff{}, es);
        }
        return;
      }
      if (e.trjt_any > 0) {
        // with at least one member's tracer part on: the MID instantiation of the same launch (which members take the
        // midpoint the kernel reads from device memory); the members' fell-back counts beside the eaten counts
        const EnsMid em{(const int32_t*)e.trj_trc_dev, 0.5 * c.prm.dt, e.trj_vals + ENS_TRJ_FELL};
        const RedOut rm{e.vals + ENS_V_EATEN, e.trj_vals + ENS_TRJ_FELL, e.cnt + 3 * (size_t)M, 2, 0, 0u};
        if (e.nb_tr > 1)
          hipLaunchKernelGGL((k_ens_tracer_cloud<B, true>), dim3(e.nb_tr, M), dim3(BS), 0, st, Mh, c.tgrid, (int64_t)n,
                             (const double*)e.u, e.ntr, e.trx, e.try_, e.trs, e.trcap, e.trstep, c.prm.dt,
                             c.prm.center_x, c.prm.center_y, c.prm.capture_radius, e.part_tr, rm, eb, em);
        else
          hipLaunchKernelGGL((k_ens_tracer<B, true>), dim3(1, M), dim3(BS), 0, st, Mh, c.tgrid, (int64_t)n,
                             (const double*)e.u, e.ntr, e.trx, e.try_, e.trs, e.trcap, e.trstep, c.prm.dt,
                             c.prm.center_x, c.prm.center_y, c.prm.capture_radius, e.vals, eb, em);
        return;
      }
      if (e.nb_tr > 1)
        hipLaunchKernelGGL(k_ens_tracer_cloud<B>, dim3(e.nb_tr, M), dim3(BS), 0, st, Mh, c.tgrid, (int64_t)n,
                           (const double*)e.u, e.ntr, e.trx, e.try_, e.trs, e.trcap, e.trstep, c.prm.dt,
                           c.prm.center_x, c.prm.center_y, c.prm.capture_radius, e.part_tr, rt, eb, EnsMidOff{});
      else
        hipLaunchKernelGGL(k_ens_tracer<B>, dim3(1, M), dim3(BS), 0, st, Mh, c.tgrid, (int64_t)n, (const double*)e.u,
                           e.ntr, e.trx, e.try_, e.trs, e.trcap, e.trstep, c.prm.dt, c.prm.center_x, c.prm.center_y,
                           c.prm.capture_radius, e.vals, eb, EnsMidOff{});
    };
    if (e.br_any > 0)
      launch(std::true_type{}, EnsBrown{(const double*)e.br_a, (const uint2*)e.br_key, c.tr_ylo, c.tr_yhi});
    else
      launch(std::false_type{}, EnsBrownOff{});
    KCHK();
    e.tr_blocks = e.nb_tr;
    e.tr_threads = BS;
  }
  hipLaunchKernelGGL(k_ens_record, dim3((M + 255) / 256), dim3(256), 0, st, M, (const double*)e.vals, e.ring, e.count);
  KCHK();
  // with the loads record on: every member's row from its final u and pressures, one launch (Ctx::loads_step); the
  // rows' indices come from the members' counts in device memory
  if (e.ld_cap > 0) ens_loads(c, e, 0, M, false, LoadsRec{e.ld_ring, e.ld_count, e.ld_cap});
}
// the ensemble's vorticity buffers, allocated at first use and kept
void ens_flow_bufs(Ctx& c, Ens& e) {
  if (e.vort) return;
  const size_t sM = (size_t)e.M;
  e.vort = e.alloc<double>(sM * e.n, c.st);
  e.part_curl = e.alloc<double>(sM * 4 * e.nb_div, c.st);
  e.flow = e.alloc<double>(sM * ENS_VALS, c.st);
  e.cnt_curl = e.alloc<unsigned>(sM, c.st);
}
// k_ens_curl over members m0 .. m0 + nm - 1 of the current u: the vorticity into e.vort (store) and the flow values
// into slots 0..3 of the members' e.flow (energy: with the |u|^2 pair).  Writes only those buffers.
void ens_curl(Ctx& c, Ens& e, int32_t m0, int32_t nm, bool store, bool energy) {
  ens_flow_bufs(c, e);
  const DevSell& A = c.dP;
  const size_t m = (size_t)m0;
  const RedOut r{e.flow + m * ENS_VALS, nullptr, e.cnt_curl + m, 4, 0, 0b1001u};
  with_c16(A, [&](auto c16) {
    hipLaunchKernelGGL(k_ens_curl<decltype(c16)::value>, dim3(e.nb_div, nm), dim3(BS), 0, c.st, A.view(),
                       (const double*)c.dGx, (const double*)c.dGy, (const double*)(e.u + m * 2 * e.n),
                       (const double*)c.das1, store ? e.vort + m * e.n : (double*)nullptr, energy ? 1 : 0,
                       e.part_curl + m * 4 * e.nb_div, r);
  });
  KCHK();
}
// field -> (device array, values per member, per-row components: 2 interleaved, 1 plain, 0 not row-indexed)
struct EnsField {
  double* a;
  i64 per;
  int comp;
};
EnsField ens_field(Ctx& c, Ens& e, int32_t field) {
  switch (field) {
    case PUCFEM_F_U: return {e.u, 2 * e.n, 2};
    case PUCFEM_F_USTAR: return {e.us, 2 * e.n, 2};
    case PUCFEM_F_P: return {e.p, e.n, 1};
    case PUCFEM_F_P2: return {e.p2, e.n, 1};
    case PUCFEM_F_C: return {e.c, e.n, 1};
    case PUCFEM_F_VORTICITY: ens_flow_bufs(c, e); return {e.vort, e.n, 1};  // (read only; ens_curl fills it)
    case PUCFEM_F_U_ADV:  // (read only: the members' u_a of their last inertial step)
      if (!e.ua) throw Error(PUCFEM_ESTATE, "no member has taken an inertial step: u_adv holds nothing");
      return {e.ua, 2 * e.n, 2};
    case PUCFEM_F_U_RHS:  // (read only: the members' r of their last forced step)
      if (!e.frhs) throw Error(PUCFEM_ESTATE, "no member has taken a forced step: u_rhs holds nothing");
      return {e.frhs, 2 * e.n, 2};
    case PUCFEM_F_FORCE:  // (read only, formed when read into the context's scratch: pucfem_ens_get_field)
      return {c.smp_scratch<double>(15, 2 * (size_t)e.n * (size_t)e.M), 2 * e.n, 2};
    case PUCFEM_F_TRACERS: return {nullptr, 2 * (i64)e.ntr, 0};
    case PUCFEM_F_STATUS: return {e.trs, (i64)e.ntr, 0};
    case PUCFEM_F_CAPTURE_STEP: return {nullptr, (i64)e.ntr, 0};
    case PUCFEM_F_DEFGRAD:  // (the members' F; identity rows for a member whose flag is off)
      if (e.str_any == 0)
        throw Error(PUCFEM_ESTATE, "no member's tracer stretching is on: there is no deformation gradient");
      return {e.str_F, 4 * (i64)e.ntr, 0};
    default:
      throw Error(PUCFEM_EINVAL,
                  "not an ensemble field (U, USTAR, P, P2, C, VORTICITY, U_ADV, FORCE, U_RHS, TRACERS, STATUS, "
                  "CAPTURE_STEP, DEFGRAD)");
  }
}
}  // namespace

int pucfem_ens_destroy(void* ctx) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    if (!c.ens) return;
    HIPCHK(hipStreamSynchronize(c.st));
    c.ens.reset();
  });
}

int pucfem_ens_create(void* ctx, int32_t members, const double* dir_values) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    c.need_dev();
    c.need_built();
    auto state = [](bool ok, const char* msg) {
      if (!ok) throw Error(PUCFEM_ESTATE, msg);
    };
    state(c.scheme == PUCFEM_STOKES_COLOR || c.scheme == PUCFEM_STOKES_FOOD, "ensembles step Stokes contexts");
    state(!c.dist(), "ensembles run on a single-rank context");
    state(!c.dye_impl, "ensembles step the semi-Lagrangian dye, not the implicit variant");
    state(!c.inertia, "ensembles step without inertia: switch it off first (pucfem_set_inertia)");
    state(!c.adv_dye && !c.adv_vel,
          "ensembles step the first-order advection: switch MacCormack off first (pucfem_set_advection)");
    state(!c.trj_any(), "the context's midpoint is on: switch it off first (members carry their own: pucfem_ens_set_trajectory)");
    state(!c.stroked(), "the context's stroke is on: clear it first (members carry their own: pucfem_ens_set_stroke)");
    state(!c.str_on,
          "the context's tracer stretching is on: switch it off first (members carry their own: "
          "pucfem_ens_set_tracer_stretch)");
    state(c.dense, "ensembles need the dense small-mesh path (N <= 1500, solver_path auto, no multigrid)");
    state(c.dir_ncomp == 2 && c.dbcsrc && c.fK.items == 0 && !c.p_from_y && c.fused_red && !c.lat_sl &&
              c.sl_rec_wave(c.lp.n_own) && (c.scheme != PUCFEM_STOKES_FOOD || c.has_tgrid),
          "the context's small-mesh step is not in its default form (measurement knobs set?)");
    require(members >= 1 && members <= 4096, "members must be in 1..4096");
    require(dir_values != nullptr, "dir_values is null");
    HIPCHK(hipStreamSynchronize(c.st));
    c.ens.reset();
    c.prep_grad_proj_bc();  // (the projection's position map, as the context's first step makes it)
    auto ep = std::make_unique<Ens>();
    Ens& e = *ep;
    const i64 n = c.lp.n_own, N = c.mesh.N;
    const int32_t M = members;
    const size_t sM = (size_t)M;
    e.M = M;
    e.n = n;
    e.ntr = c.scheme == PUCFEM_STOKES_FOOD ? c.ntr : 0;
    e.dstride = 2 * (i64)std::max(1, c.ndir);
    const int tiles = (M + ENS_TM - 1) / ENS_TM;
    // the dense products' grid in x: enough blocks to fill the device about twice over, each staging its tile's
    // vectors once for as many rows as that leaves (the rows' arithmetic does not depend on their block)
    e.gx_dense = (int)std::max<i64>(std::min<i64>(8, (n + 3) / 4), std::min<i64>((n + 3) / 4, 1024 / tiles));
    e.nb_div = c.div_grid();
    e.nb_sl = c.nb_sl(n);
    e.nb_mix = c.nb_rows(n);
    e.nb_ws = Ctx::nb_dye(n);
    e.lds_mv = sizeof(double) * 2 * (size_t)n * ENS_TM;
    e.lds_pres = sizeof(double) * (size_t)n * ENS_TM;
    HIPCHK(hipFuncSetAttribute((const void*)k_ens_mv2_bc<ENS_TM>, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)(sizeof(double) * 2 * DENSE_MAX * ENS_TM)));
    HIPCHK(hipFuncSetAttribute((const void*)k_ens_pres<ENS_TM>, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)(sizeof(double) * DENSE_MAX * ENS_TM)));
    hipStream_t st = c.st;
    e.u = e.alloc<double>(sM * 2 * n, st);
    e.us = e.alloc<double>(sM * 2 * n, st);
    for (double** f : {&e.p, &e.p2, &e.braw, &e.c, &e.cn}) *f = e.alloc<double>(sM * n, st);
    e.dval = e.alloc<double>(sM * e.dstride, st);
    for (double** f : {&e.trx, &e.try_, &e.trs}) *f = e.alloc<double>(sM * (size_t)e.ntr, st);
    e.vals = e.alloc<double>(sM * ENS_VALS, st);
    e.part_d = e.alloc<double>(sM * 3 * e.nb_div, st);
    e.part_sl = e.alloc<double>(sM * 3 * e.nb_sl, st);
    e.part_mx = e.alloc<double>(sM * 3 * e.nb_mix, st);
    // the member's grid in x: the single path's, capped so that the launch's blocks stay near the cloud kernels' cap
    e.nb_tr = std::max(1, std::min(Ctx::tracer_blocks(e.ntr), TRACER_CLOUD_MAXB / M));
    e.part_tr = e.alloc<double>(sM * 3 * e.nb_tr, st);
    e.trcap = e.alloc<int32_t>(sM * (size_t)e.ntr, st);
    HIPCHK(hipMemsetAsync(e.trcap, 0xFF, sizeof(int32_t) * std::max<size_t>(1, sM * (size_t)e.ntr), st));
    e.trstep = e.alloc<int32_t>(sM, st);
    e.cnt = e.alloc<unsigned>(4 * sM, st);
    e.count = e.alloc<int>(sM, st);
    e.ring_steps = (int)std::max<i64>(c.gk, std::min<i64>(Ctx::GRING, 65536 / M));
    e.ring = e.alloc<double>((size_t)e.ring_steps * sM * 8, st);
    // initial state, as build leaves the context: u = 0 then makeDirBCU with the member's values (the entries
    // kept by build: a node's last occurrence, in list order); c = 1[x < 0.5]; the context's tracers, status 0
    const size_t nd = c.dir_nodes.size();
    std::vector<i64> last(N, -1);
    for (size_t k = 0; k < nd; ++k) last[c.dir_nodes[k]] = (i64)k;
    std::vector<size_t> keep;
    for (size_t k = 0; k < nd; ++k)
      if (last[c.dir_nodes[k]] == (i64)k) keep.push_back(k);
    if ((int)keep.size() != c.ndir) throw Error(PUCFEM_ESTATE, "Dirichlet list changed since the build");
    std::vector<double> dv(sM * e.dstride, 0.0), u0(sM * 2 * n, 0.0), c0(sM * n);
    for (size_t m = 0; m < sM; ++m) {
      for (size_t q = 0; q < keep.size(); ++q) {
        const size_t k = keep[q];
        const double vx = dir_values[(m * nd + k) * 2], vy = dir_values[(m * nd + k) * 2 + 1];
        dv[m * e.dstride + 2 * q] = vx;
        dv[m * e.dstride + 2 * q + 1] = vy;
        const i64 g = c.ord.old2new[c.dir_nodes[k]];
        u0[(m * n + g) * 2] = vx;
        u0[(m * n + g) * 2 + 1] = vy;
      }
      for (i64 g = 0; g < n; ++g) c0[m * n + g] = c.mesh.x[c.ord.new2old[g]] < 0.5 ? 1.0 : 0.0;
    }
    c.h2d(e.dval, dv.data(), sizeof(double) * dv.size());
    e.dval0 = dv;  // (what clearing a member's stroke restores)
    c.h2d(e.u, u0.data(), sizeof(double) * u0.size());
    c.h2d(e.c, c0.data(), sizeof(double) * c0.size());
    for (size_t m = 0; m < sM && e.ntr > 0; ++m) {
      HIPCHK(hipMemcpyAsync(e.trx + m * e.ntr, c.trx, sizeof(double) * e.ntr, hipMemcpyDeviceToDevice, st));
      HIPCHK(hipMemcpyAsync(e.try_ + m * e.ntr, c.try_, sizeof(double) * e.ntr, hipMemcpyDeviceToDevice, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    c.ens = std::move(ep);
  });
}

int pucfem_ens_info(void* ctx, int64_t* out4) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    Ens& e = *ens_of(c);
    out4[0] = e.M;
    out4[1] = ENS_TM;
    out4[2] = (int64_t)e.bytes;
    out4[3] = e.steps;
  });
}

// ---- inertia per member (k_ens_sl_vel, pucfem_ensemble.hpp)
namespace {
// the members' inertia flags as the kernels read them: ENS_ADV_MC where the member's velocity scheme is MacCormack,
// ENS_ADV_SL_MID / ENS_ADV_MC_MID where its velocity part is on (pucfem_ens_set_trajectory)
// a member's (scheme, order) as one of the four flag values {SL, MC, SL_MID, MC_MID} of its field; counts the
// MacCormack members into mc_any and the members per flag into n
int32_t ens_mode_flag(const std::vector<int32_t>& scheme, const std::vector<int32_t>& order, size_t m,
                      const int32_t (&flag)[4], int& mc_any, int* n) {
  const bool mc = !scheme.empty() && scheme[m] != PUCFEM_ADV_SL;
  const bool mid = !order.empty() && order[m] == PUCFEM_TRJ_MIDPOINT;
  const int32_t f = flag[(mid ? 2 : 0) + (mc ? 1 : 0)];
  mc_any += mc ? 1 : 0;
  ++n[f];
  return f;
}
void ens_adv_upload(Ctx& c, Ens& e) {
  const size_t sM = (size_t)e.M;
  e.adv_any = (int)std::count(e.adv_on.begin(), e.adv_on.end(), 1);
  e.mc_vel_any = 0;
  for (int& k : e.vel_n) k = 0;
  if (!e.adv_on_dev) return;
  std::vector<int32_t> f(sM, ENS_ADV_OFF);
  for (size_t m = 0; m < sM; ++m)
    if (e.adv_on[m])
      f[m] = ens_mode_flag(e.mc_vel, e.trj_vel, m, {ENS_ADV_SL, ENS_ADV_MC, ENS_ADV_SL_MID, ENS_ADV_MC_MID}, e.mc_vel_any,
                           e.vel_n);
  c.h2d(e.adv_on_dev, f.data(), sizeof(int32_t) * sM);
  HIPCHK(hipStreamSynchronize(c.st));
}
// what k_ens_sl, k_ens_wsum and the dye's MacCormack / midpoint launches read, allocated when a member's dye first
// leaves k_ens_sl (its scheme or its trajectory part switched on) and kept: the members' dye flags (M), k_ens_wsum's
// partials and the ticket counters of the MacCormack launches and of the sums (3 M)
void ens_dye_flag_bufs(Ctx& c, Ens& e) {
  if (e.mc_on_dev) return;
  const size_t sM = (size_t)e.M;
  e.mc_part_ws = e.alloc<double>(sM * 2 * e.nb_ws, c.st);
  e.mc_on_dev = e.alloc<int32_t>(sM, c.st);
  e.mc_cnt = e.alloc<unsigned>(3 * sM, c.st);
}
void ens_dye_ch_fit(Ctx& c, Ens& e);  // (with the dye channels' calls below)
// the members' dye flags as the kernels read them (ENS_DYE_*): the scheme in bit 0, the trajectory part in bit 1
void ens_dye_upload(Ctx& c, Ens& e) {
  const size_t sM = (size_t)e.M;
  e.mc_dye_any = 0;
  for (int& k : e.dye_n) k = 0;
  std::vector<int32_t> f(sM, ENS_DYE_SL);
  for (size_t m = 0; m < sM; ++m)
    f[m] = ens_mode_flag(e.mc_dye, e.trj_dye, m, {ENS_DYE_SL, ENS_DYE_MC, ENS_DYE_SL_MID, ENS_DYE_MC_MID}, e.mc_dye_any,
                         e.dye_n);
  if (!e.mc_on_dev) return;
  c.h2d(e.mc_on_dev, f.data(), sizeof(int32_t) * sM);
  HIPCHK(hipStreamSynchronize(c.st));
}
}  // namespace

int pucfem_ens_set_inertia(void* ctx, int32_t member, int32_t on) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    Ens& e = *ens_of(c);
    require(member >= -1 && member < e.M, "member index out of range");
    c.inertia_ready();
    const size_t sM = (size_t)e.M;
    const int32_t v = on != 0 ? 1 : 0;
    const size_t m0 = member < 0 ? 0 : (size_t)member, m1 = member < 0 ? sM : m0 + 1;
    if (e.adv_on.empty()) {
      if (!v) return;  // (nothing was ever on: nothing to switch off, and nothing is allocated)
      const size_t before = e.bytes;
      e.ua = e.alloc<double>(sM * 2 * e.n, c.st);
      e.part_adv = e.alloc<double>(sM * e.nb_sl, c.st);
      e.adv_on_dev = e.alloc<int32_t>(sM, c.st);
      e.cnt_adv = e.alloc<unsigned>(sM, c.st);
      e.adv_bytes = e.bytes - before;
      e.adv_on.assign(sM, 0);
      e.adv_steps.assign(sM, 0);
    }
    bool changed = false;
    for (size_t m = m0; m < m1; ++m) {
      if (e.adv_on[m] == v) continue;
      e.adv_on[m] = v;
      changed = true;
      if (v) {  // (switched on: its counts start again, as pucfem_set_inertia's do)
        e.adv_steps[m] = 0;
        HIPCHK(hipMemsetAsync(e.vals + ENS_VALS * m + ENS_V_VEL_NF, 0, sizeof(double), c.st));
        e.adv_stale = true;
      }
    }
    if (!changed) return;
    ens_adv_upload(c, e);
  });
}

int pucfem_ens_inertia_info(void* ctx, int32_t member, int64_t* out4) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    Ens& e = *ens_of(c);
    require(member >= 0 && member < e.M, "member index out of range");
    require(out4 != nullptr, "null output");
    const size_t m = (size_t)member;
    const bool have = !e.adv_on.empty();
    if (have && e.adv_stale) {  // (one copy serves the calls for every member until the next step)
      e.adv_vals.resize((size_t)e.M * ENS_VALS);
      c.d2h(e.adv_vals.data(), e.vals, sizeof(double) * e.adv_vals.size());
      e.adv_stale = false;
    }
    out4[0] = have ? e.adv_on[m] : 0;
    out4[1] = have ? e.adv_steps[m] : 0;
    out4[2] = have ? (int64_t)std::llround(e.adv_vals[ENS_VALS * m + ENS_V_VEL_NF]) : 0;
    out4[3] = (int64_t)e.adv_bytes;
  });
}

// ---- MacCormack advection per member (k_ens_mc_fwd / k_ens_mc_bwd / k_ens_wsum, pucfem_ensemble.hpp)
int pucfem_ens_set_advection(void* ctx, int32_t member, int32_t what, int32_t scheme) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    Ens& e = *ens_of(c);
    require(member >= -1 && member < e.M, "member index out of range");
    if (what & ~(PUCFEM_ADV_DYE | PUCFEM_ADV_VELOCITY) || what == 0)
      throw Error(PUCFEM_EINVAL, "what is a mask of PUCFEM_ADV_DYE and PUCFEM_ADV_VELOCITY");
    if (scheme != PUCFEM_ADV_SL && scheme != PUCFEM_ADV_MACCORMACK)
      throw Error(PUCFEM_EINVAL, "unknown advection scheme");
    if ((what & PUCFEM_ADV_DYE) && c.scheme != PUCFEM_STOKES_COLOR)
      throw Error(PUCFEM_ESTATE, "the dye's scheme needs a STOKES_COLOR ensemble: STOKES_FOOD has no dye");
    const size_t sM = (size_t)e.M, sn = (size_t)e.n;
    const size_t m0 = member < 0 ? 0 : (size_t)member, m1 = member < 0 ? sM : m0 + 1;
    const size_t before = e.bytes;
    // one field: its set's buffers at the first switch-on, the members' schemes, and for a member switched on its
    // counts anew (as pucfem_set_advection's do)
    auto part = [&](std::vector<int32_t>& sch, std::vector<int64_t>& steps, int slot, auto&& bufs) {
      if (sch.empty()) {
        if (!scheme) return false;  // (nothing was ever on: nothing is allocated until now)
        bufs();
        sch.assign(sM, 0);
        steps.assign(sM, 0);
      }
      bool changed = false;
      for (size_t m = m0; m < m1; ++m) {
        if (sch[m] == scheme) continue;
        sch[m] = scheme;
        changed = true;
        if (scheme) {
          steps[m] = 0;
          HIPCHK(hipMemsetAsync(e.vals + ENS_VALS * m + slot, 0, 2 * sizeof(double), c.st));
        }
      }
      return changed;
    };
    bool up_dye = false, up_vel = false;
    if (what & PUCFEM_ADV_DYE)
      up_dye = part(e.mc_dye, e.mc_steps, ENS_V_DYE_MC, [&] {
        e.mc_ch = e.alloc<double>(sM * sn, c.st);
        e.mc_rec = e.alloc<int4>(sM * sn, c.st);
        e.mc_part = e.alloc<double>(sM * 3 * e.nb_sl, c.st);
        ens_dye_flag_bufs(c, e);
      });
    if (what & PUCFEM_ADV_VELOCITY)
      up_vel = part(e.mc_vel, e.mcv_steps, ENS_V_VEL_MC, [&] {
        e.mcv_ch = e.alloc<double>(sM * 2 * sn, c.st);
        e.mcv_rec = e.alloc<int4>(sM * sn, c.st);
        e.mcv_part = e.alloc<double>(sM * 3 * e.nb_sl, c.st);
        e.mcv_cnt = e.alloc<unsigned>(2 * sM, c.st);
      });
    e.mc_bytes += e.bytes - before;
    if (up_dye) ens_dye_upload(c, e);
    if (up_dye) ens_dye_ch_fit(c, e);  // (with dye channels: the set's ch of the channels)
    if (up_vel) ens_adv_upload(c, e);  // (takes effect while the member's inertia flag is on)
    e.adv_stale = true;
    HIPCHK(hipStreamSynchronize(c.st));
  });
}

int pucfem_ens_advection_info(void* ctx, int32_t member, int64_t* out11) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    Ens& e = *ens_of(c);
    require(member >= 0 && member < e.M, "member index out of range");
    require(out11 != nullptr, "null output");
    const size_t m = (size_t)member;
    const bool dye = !e.mc_dye.empty(), vel = !e.mc_vel.empty();
    if ((dye || vel) && (e.adv_stale || e.adv_vals.empty())) {  // (one copy serves every member until the next step)
      e.adv_vals.resize((size_t)e.M * ENS_VALS);
      c.d2h(e.adv_vals.data(), e.vals, sizeof(double) * e.adv_vals.size());
      e.adv_stale = false;
    }
    auto val = [&](int slot) { return (int64_t)std::llround(e.adv_vals[ENS_VALS * m + slot]); };
    for (int k = 0; k < 11; ++k) out11[k] = 0;
    out11[0] = dye ? e.mc_dye[m] : PUCFEM_ADV_SL;
    out11[1] = vel ? e.mc_vel[m] : PUCFEM_ADV_SL;
    out11[2] = dye ? e.mc_steps[m] : 0;
    out11[3] = vel ? e.mcv_steps[m] : 0;
    // (the counts of the member's last MacCormack launch while its scheme is on; 0 before the first and once it is off)
    if (out11[0] && out11[2] > 0) {
      out11[4] = val(ENS_V_DYE_NF);
      out11[5] = val(ENS_V_DYE_MC);
      out11[6] = val(ENS_V_DYE_MC + 1);
    }
    if (out11[1] && out11[3] > 0 && !e.adv_on.empty() && e.adv_on[m]) {
      out11[7] = val(ENS_V_VEL_NF);
      out11[8] = val(ENS_V_VEL_MC);
      out11[9] = val(ENS_V_VEL_MC + 1);
    }
    out11[10] = (int64_t)e.mc_bytes;
  });
}

// ---- midpoint trajectories per member (k_ens_trj_fwd / k_ens_trj_bwd, the MID tracer kernels, pucfem_ensemble.hpp)
int pucfem_ens_set_trajectory(void* ctx, int32_t member, int32_t what, int32_t order) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    Ens& e = *ens_of(c);
    require(member >= -1 && member < e.M, "member index out of range");
    constexpr int all = PUCFEM_TRJ_DYE | PUCFEM_TRJ_VELOCITY | PUCFEM_TRJ_TRACERS;
    if (what & ~all || what == 0)
      throw Error(PUCFEM_EINVAL, "what is a mask of PUCFEM_TRJ_DYE, PUCFEM_TRJ_VELOCITY and PUCFEM_TRJ_TRACERS");
    if (order != PUCFEM_TRJ_EULER && order != PUCFEM_TRJ_MIDPOINT)
      throw Error(PUCFEM_EINVAL, "unknown trajectory order");
    if ((what & PUCFEM_TRJ_DYE) && c.scheme != PUCFEM_STOKES_COLOR)
      throw Error(PUCFEM_ESTATE, "the dye's trajectory needs a STOKES_COLOR ensemble: STOKES_FOOD has no dye");
    if ((what & PUCFEM_TRJ_TRACERS) && e.ntr <= 0)
      throw Error(PUCFEM_ESTATE, "the tracers' trajectory needs a STOKES_FOOD ensemble with tracers");
    const size_t sM = (size_t)e.M;
    const size_t m0 = member < 0 ? 0 : (size_t)member, m1 = member < 0 ? sM : m0 + 1;
    const bool mid = order == PUCFEM_TRJ_MIDPOINT;
    const size_t before = e.bytes;
    if (mid && !e.trj_vals) {  // (nothing was ever on: nothing is allocated until now)
      e.trj_vals = e.alloc<double>(sM * ENS_VALS, c.st);
      e.trj_cnt = e.alloc<unsigned>(4 * sM, c.st);
    }
    // one part: its buffers at the first switch-on, the members' orders, and for a member switched on its counts anew
    auto part = [&](std::vector<int32_t>& ord, std::vector<int64_t>& steps, int slot0, int nslots, auto&& bufs) {
      if (ord.empty()) {
        if (!mid) return false;
        bufs();
        ord.assign(sM, PUCFEM_TRJ_EULER);
        steps.assign(sM, 0);
      }
      bool changed = false;
      for (size_t m = m0; m < m1; ++m) {
        if (ord[m] == order) continue;
        ord[m] = order;
        changed = true;
        if (mid) {
          steps[m] = 0;
          HIPCHK(hipMemsetAsync(e.trj_vals + ENS_VALS * m + slot0, 0, nslots * sizeof(double), c.st));
        }
      }
      return changed;
    };
    bool up_dye = false, up_vel = false, up_trc = false;
    if (what & PUCFEM_TRJ_DYE)
      up_dye = part(e.trj_dye, e.trjd_steps, ENS_TRJ_DYE, 4, [&] {
        e.trj_part_d = e.alloc<double>(sM * 5 * e.nb_sl, c.st);
        ens_dye_flag_bufs(c, e);
      });
    if (what & PUCFEM_TRJ_VELOCITY)
      up_vel = part(e.trj_vel, e.trjv_steps, ENS_TRJ_VEL, 4,
                    [&] { e.trj_part_v = e.alloc<double>(sM * 5 * e.nb_sl, c.st); });
    if (what & PUCFEM_TRJ_TRACERS)
      up_trc = part(e.trj_trc, e.trjt_steps, ENS_TRJ_FELL, 1, [&] { e.trj_trc_dev = e.alloc<int32_t>(sM, c.st); });
    e.trj_bytes += e.bytes - before;
    if (up_dye) ens_dye_upload(c, e);
    if (up_vel) ens_adv_upload(c, e);  // (takes effect while the member's inertia flag is on)
    if (up_trc) {
      std::vector<int32_t> f(sM);
      for (size_t m = 0; m < sM; ++m) f[m] = e.trj_trc[m] == PUCFEM_TRJ_MIDPOINT ? 1 : 0;
      e.trjt_any = (int)std::count(f.begin(), f.end(), 1);
      c.h2d(e.trj_trc_dev, f.data(), sizeof(int32_t) * sM);
    }
    e.trj_stale = e.adv_stale = true;
    HIPCHK(hipStreamSynchronize(c.st));
  });
}

int pucfem_ens_trajectory_info(void* ctx, int32_t member, int64_t* out10) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    Ens& e = *ens_of(c);
    require(member >= 0 && member < e.M, "member index out of range");
    require(out10 != nullptr, "null output");
    const size_t m = (size_t)member;
    if (e.trj_vals && (e.trj_stale || e.trj_host.empty())) {  // (one copy serves every member until the next step)
      e.trj_host.resize((size_t)e.M * ENS_VALS);
      c.d2h(e.trj_host.data(), e.trj_vals, sizeof(double) * e.trj_host.size());
      e.trj_stale = false;
    }
    auto val = [&](int slot) { return e.trj_vals ? (int64_t)std::llround(e.trj_host[ENS_VALS * m + slot]) : 0; };
    const bool dye = !e.trj_dye.empty(), vel = !e.trj_vel.empty(), trc = !e.trj_trc.empty();
    out10[0] = dye ? e.trj_dye[m] : PUCFEM_TRJ_EULER;
    out10[1] = vel ? e.trj_vel[m] : PUCFEM_TRJ_EULER;
    out10[2] = trc ? e.trj_trc[m] : PUCFEM_TRJ_EULER;
    out10[3] = dye ? e.trjd_steps[m] : 0;
    out10[4] = vel ? e.trjv_steps[m] : 0;
    out10[5] = trc ? e.trjt_steps[m] : 0;
    // (of the member's last launch with the part on, as pucfem_trajectory_info: with MacCormack both passes count)
    out10[6] = val(ENS_TRJ_DYE + ENS_T_MID1) + (!e.mc_dye.empty() && e.mc_dye[m] ? val(ENS_TRJ_DYE + ENS_T_MID2) : 0);
    out10[7] = val(ENS_TRJ_VEL + ENS_T_MID1) + (!e.mc_vel.empty() && e.mc_vel[m] ? val(ENS_TRJ_VEL + ENS_T_MID2) : 0);
    out10[8] = val(ENS_TRJ_FELL);
    out10[9] = (int64_t)e.trj_bytes;
  });
}

// ---- body forces per member (k_ens_force_rhs, pucfem_force.hpp)
namespace {
// the members' force buffers, allocated when a member is first forced; the nodal planes when first needed
void ens_force_bufs(Ctx& c, Ens& e, bool nodal) {
  const size_t sM = (size_t)e.M, before = e.bytes;
  if (e.fmask.empty()) {
    e.frhs = e.alloc<double>(sM * 2 * e.n, c.st);
    e.fparm = e.alloc<double>(sM * ENS_FORCE_PARM, c.st);
    e.fmask_dev = e.alloc<int32_t>(sM, c.st);
    e.fmask.assign(sM, 0);
    e.fpar.assign(sM * ENS_FORCE_PARM, 0.0);
    e.fsteps.assign(sM, 0);
  }
  if (nodal && !e.fnod) e.fnod = e.alloc<double>(sM * 2 * e.n, c.st);
  e.force_bytes += e.bytes - before;
}
// the members' settings to the device (the stream is idle between two pucfem_ens_step calls)
void ens_force_upload(Ctx& c, Ens& e) {
  e.force_any = (int)std::count_if(e.fmask.begin(), e.fmask.end(), [](int32_t k) { return k != 0; });
  c.h2d(e.fmask_dev, e.fmask.data(), sizeof(int32_t) * e.fmask.size());
  c.h2d(e.fparm, e.fpar.data(), sizeof(double) * e.fpar.size());
  HIPCHK(hipStreamSynchronize(c.st));
}
}  // namespace

int pucfem_ens_set_force(void* ctx, int32_t member, const double* F2, const double* field) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    if (F2) require(std::isfinite(F2[0]) && std::isfinite(F2[1]), "the force must be finite");
    Ens& e = *ens_of(c);
    require(member >= -1 && member < e.M, "member index out of range");
    const i64 N = c.mesh.N;
    if (field) {
      bool ok = true;
      for (i64 k = 0; k < 2 * N && ok; ++k) ok = std::isfinite(field[k]);
      require(ok, "the force field must be finite");
    }
    const bool uni = F2 && (F2[0] != 0.0 || F2[1] != 0.0);
    if (e.fmask.empty() && !uni && !field) return;  // (nothing was ever set: nothing to switch off)
    ens_force_bufs(c, e, field != nullptr);
    const size_t m0 = member < 0 ? 0 : (size_t)member, m1 = member < 0 ? (size_t)e.M : m0 + 1;
    for (size_t m = m0; m < m1; ++m) {
      e.fmask[m] = (e.fmask[m] & 4) | (uni ? 1 : 0) | (field ? 2 : 0);
      e.fpar[m * ENS_FORCE_PARM + 0] = uni ? F2[0] : 0.0;
      e.fpar[m * ENS_FORCE_PARM + 1] = uni ? F2[1] : 0.0;
      e.fsteps[m] = 0;
      if (field) c.put_all(2, 1, field, e.fnod + m * 2 * (size_t)e.n);  // (one N x 2 field, every requested member)
    }
    ens_force_upload(c, e);
  });
}

int pucfem_ens_set_buoyancy(void* ctx, int32_t member, const double* g2, double beta, double ref) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    if (g2) require(std::isfinite(g2[0]) && std::isfinite(g2[1]) && std::isfinite(beta) && std::isfinite(ref),
                    "g, beta and ref must be finite");
    Ens& e = *ens_of(c);
    require(member >= -1 && member < e.M, "member index out of range");
    if (g2 && c.scheme != PUCFEM_STOKES_COLOR)
      throw Error(PUCFEM_ESTATE, "buoyancy needs a STOKES_COLOR context: STOKES_FOOD has no dye");
    if (e.fmask.empty() && !g2) return;
    ens_force_bufs(c, e, false);
    const size_t m0 = member < 0 ? 0 : (size_t)member, m1 = member < 0 ? (size_t)e.M : m0 + 1;
    for (size_t m = m0; m < m1; ++m) {
      e.fmask[m] = (e.fmask[m] & 3) | (g2 ? 4 : 0);
      double* q = e.fpar.data() + m * ENS_FORCE_PARM;
      q[2] = g2 ? g2[0] : 0.0;
      q[3] = g2 ? g2[1] : 0.0;
      q[4] = g2 ? beta : 0.0;
      q[5] = g2 ? ref : 0.0;
      e.fsteps[m] = 0;
    }
    ens_force_upload(c, e);
  });
}

// ---- dye channels per member (k_ens_dye_fwd / k_ens_dye_bwd, pucfem_ensemble.hpp)
namespace {
// the ensemble of the channel calls: no ensemble is decided before the device is asked for
Ens* ens_dyes_of(Ctx& c) {
  c.need_built();
  if (!c.ens) throw Error(PUCFEM_ESTATE, "no ensemble on this context: call pucfem_ens_create first");
  c.need_dev();
  return c.ens.get();
}
bool ens_dye_field(int32_t field) {
  return field == PUCFEM_F_DYES || (field >= PUCFEM_F_DYE0 && field < PUCFEM_F_DYE0 + DYE_MAX);
}
// the MacCormack set's ch of the channels, while K > 0 and a member's dye scheme is on: the ensemble's mc_dye_fit
void ens_dye_ch_fit(Ctx& c, Ens& e) {
  if (e.dy_K == 0 || e.mc_dye_any == 0 || e.dy_ch) return;
  HIPCHK(hipStreamSynchronize(c.st));
  e.drop_graphs();
  const size_t b = sizeof(double) * (size_t)e.M * (size_t)e.dy_K * (size_t)e.n;
  HIPCHK(hipMalloc(reinterpret_cast<void**>(&e.dy_ch), b));
  HIPCHK(hipMemsetAsync(e.dy_ch, 0, b, c.st));
  HIPCHK(hipStreamSynchronize(c.st));
  e.dy_bytes += b;
}
// PUCFEM_F_DYES / PUCFEM_F_DYE0 + k of the requested members, to (put) or from the current set
void ens_dye_io(Ctx& c, Ens& e, int32_t field, int32_t member, const double* src, double* dst, int64_t count) {
  require(member >= -1 && member < e.M, "member index out of range");
  const i64 N = c.mesh.N, K = e.dy_K;
  const i64 m0 = member < 0 ? 0 : member, nm = member < 0 ? e.M : 1;
  if (field == PUCFEM_F_DYES) {
    require(K > 0 && count == nm * K * N, "count does not match the ensemble's channels (members x K x N)");
    require(src != nullptr || dst != nullptr, "null buffer");
    double* d = e.dy_cur + (size_t)(m0 * K) * (size_t)e.n;
    if (src) {
      c.put_all(1, nm * K, src, d);
      for (i64 m = m0; m < m0 + nm; ++m) e.dy_steps[(size_t)m] = 0;
    } else {
      c.get_all(1, nm * K, dst, d);
    }
  } else {
    const i64 k = field - PUCFEM_F_DYE0;
    require(k < K, "dye channel index >= the ensemble's number of channels");
    require(count == nm * N, "count does not match the field's shape (members x N)");
    require(src != nullptr || dst != nullptr, "null buffer");
    for (i64 m = m0; m < m0 + nm; ++m) {  // (a member's channel k: one plane out of its K)
      double* d = e.dy_cur + (size_t)(m * K + k) * (size_t)e.n;
      if (src) c.put_all(1, 1, src + (m - m0) * N, d);
      else c.get_all(1, 1, dst + (m - m0) * N, d);
    }
  }
  HIPCHK(hipStreamSynchronize(c.st));
}
}  // namespace

int pucfem_ens_set_dyes(void* ctx, int32_t K, const double* buf) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    Ens& e = *ens_dyes_of(c);
    if (c.scheme != PUCFEM_STOKES_COLOR)
      throw Error(PUCFEM_ESTATE, "dye channels need a STOKES_COLOR ensemble: STOKES_FOOD has no dye");
    require(K >= 0 && K <= DYE_MAX, "K must be in 0 .. PUCFEM_MAX_DYES (16)");
    require((K == 0) == (buf == nullptr), "buf is K x N; NULL iff K == 0");
    HIPCHK(hipStreamSynchronize(c.st));
    e.drop_graphs();
    const size_t sM = (size_t)e.M, sn = (size_t)e.n;
    if (K != e.dy_K) {
      e.drop_dyes();
      if (K > 0) {
        const size_t planes = sM * (size_t)K;
        auto get = [&](auto*& p, size_t count_) {
          const size_t b = sizeof(*p) * count_;
          HIPCHK(hipMalloc(reinterpret_cast<void**>(&p), b));
          HIPCHK(hipMemsetAsync(p, 0, b, c.st));
          e.dy_bytes += b;
        };
        e.dy_K = K;  // (set first: drop_dyes frees whatever was allocated if a later allocation throws)
        get(e.dy_cur, planes * sn);
        get(e.dy_nxt, planes * sn);
        get(e.dy_mvals, planes * ENS_VALS);
        get(e.dy_mpart, planes * 2 * (size_t)e.nb_mix);
        get(e.dy_mout, planes * 3);
        get(e.dy_mcnt, planes);
      }
    }
    e.dy_steps.assign(K > 0 ? sM : 0, 0);
    if (K > 0) {
      for (size_t m = 0; m < sM; ++m) c.put_all(1, K, buf, e.dy_cur + m * (size_t)K * sn);
      ens_dye_ch_fit(c, e);
    }
    HIPCHK(hipStreamSynchronize(c.st));
  });
}

int pucfem_ens_dyes_info(void* ctx, int32_t member, int64_t* out4) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    Ens& e = *ens_dyes_of(c);
    require(member >= 0 && member < e.M, "member index out of range");
    require(out4 != nullptr, "null output");
    const size_t m = (size_t)member;
    out4[0] = e.dy_K;
    out4[1] = e.dy_K > 0 ? e.dy_steps[m] : 0;
    out4[2] = 0;
    if (e.dy_K > 0 && e.dy_steps[m] > 0) {  // (the count of the member's last dye launch: pass 1's, slot 4)
      double v = 0.0;
      c.d2h(&v, e.vals + ENS_VALS * m + ENS_V_DYE_NF, sizeof(double));
      out4[2] = (int64_t)std::llround(v);
    }
    out4[3] = (int64_t)e.dy_bytes;
  });
}

int pucfem_ens_dyes_mixing(void* ctx, int32_t member, double* out) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    Ens& e = *ens_dyes_of(c);
    if (e.dy_K == 0) throw Error(PUCFEM_ESTATE, "the ensemble has no dye channels (pucfem_ens_set_dyes)");
    require(member >= -1 && member < e.M, "member index out of range");
    require(out != nullptr, "null output");
    const size_t K = (size_t)e.dy_K, m0 = member < 0 ? 0 : (size_t)member, nm = member < 0 ? (size_t)e.M : 1;
    const size_t q0 = m0 * K, planes = nm * K;
    double* vals = e.dy_mvals + q0 * ENS_VALS;
    // one launch per stage over every requested plane (a grid's y extent holds 65535: 4096 members x 16 channels go
    // in two halves)
    constexpr size_t YMAX = 32768;
    for (int stage = 0; stage < 2; ++stage)
      for (size_t p0 = 0; p0 < planes; p0 += YMAX) {
        const size_t q = q0 + p0, np = std::min(YMAX, planes - p0);
        hipLaunchKernelGGL(k_ens_dyes_mix, dim3(e.nb_mix, (unsigned)np), dim3(BS), 0, c.st, (int64_t)e.n, stage,
                           (const double*)(e.dy_cur + q * (size_t)e.n), (const double*)c.dwmix,
                           e.dy_mvals + q * ENS_VALS, e.dy_mpart + q * 2 * (size_t)e.nb_mix, e.dy_mcnt + q);
        KCHK();
      }
    hipLaunchKernelGGL(k_ens_dyes_stats, dim3((unsigned)((planes + 255) / 256)), dim3(256), 0, c.st, (int32_t)planes,
                       (const double*)vals, e.dy_mout + 3 * q0);
    KCHK();
    c.d2h(out, e.dy_mout + 3 * q0, sizeof(double) * 3 * planes);
  });
}

int pucfem_ens_set_field(void* ctx, int32_t field, int32_t member, const double* buf, int64_t count) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    Ens& e = *ens_of(c);
    if (ens_dye_field(field)) return ens_dye_io(c, e, field, member, buf, nullptr, count);
    require(member >= -1 && member < e.M, "member index out of range");
    require(field != PUCFEM_F_CAPTURE_STEP, "capture steps cannot be set");
    require(field != PUCFEM_F_VORTICITY, "the vorticity cannot be set");
    require(field != PUCFEM_F_U_ADV, "u_adv cannot be set: it is the inertial step's own output");
    require(field != PUCFEM_F_FORCE && field != PUCFEM_F_U_RHS, "the force and u_rhs cannot be set: they are formed");
    const EnsField f = ens_field(c, e, field);
    const i64 m0 = member < 0 ? 0 : member, nm = member < 0 ? e.M : 1;
    require(count == nm * f.per, "count does not match the field's shape (members x values per member)");
    if (f.per == 0) return;
    if (field == PUCFEM_F_TRACERS) {
      tracers_put(c, e.trx, e.try_, e.trs, e.trcap, e.trstep + m0, nm, m0 * e.ntr, nm * e.ntr, buf);
      if (e.str_F) {  // (new tracers: the members' F is the identity again, and their step counts 0)
        c.stretch_identity(e.str_F, m0 * e.ntr, nm * e.ntr);
        for (i64 m = m0; m < m0 + nm; ++m) e.str_steps[(size_t)m] = 0;
      }
    } else if (f.comp > 0) {  // (the members are the planes)
      c.put_all(f.comp, nm, buf, f.a + m0 * f.per);
    } else {
      c.h2d(f.a + m0 * f.per, buf, sizeof(double) * nm * f.per);
    }
    HIPCHK(hipStreamSynchronize(c.st));
  });
}

int pucfem_ens_get_field(void* ctx, int32_t field, int32_t member, double* buf, int64_t count) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    Ens& e = *ens_of(c);
    if (ens_dye_field(field)) return ens_dye_io(c, e, field, member, nullptr, buf, count);
    require(member >= -1 && member < e.M, "member index out of range");
    const EnsField f = ens_field(c, e, field);
    const i64 m0 = member < 0 ? 0 : member, nm = member < 0 ? e.M : 1;
    require(count == nm * f.per, "count does not match the field's shape (members x values per member)");
    if (field == PUCFEM_F_U_ADV)  // (every requested member's plane must hold the u_a of a step of its own)
      for (i64 m = m0; m < m0 + nm; ++m)
        if (e.adv_steps[(size_t)m] == 0)
          throw Error(PUCFEM_ESTATE, "a requested member has taken no inertial step since it was switched on");
    if (field == PUCFEM_F_U_RHS)  // (every requested member's plane must hold the r of a step of its own)
      for (i64 m = m0; m < m0 + nm; ++m)
        if (e.fsteps[(size_t)m] == 0)
          throw Error(PUCFEM_ESTATE, "a requested member has taken no forced step since its setting last changed");
    if (field == PUCFEM_F_FORCE) {  // (the members' f of the current state, every member's plane: zeros if unforced)
      if (e.fmask.empty()) {
        HIPCHK(hipMemsetAsync(f.a, 0, sizeof(double) * (size_t)(e.M * f.per), c.st));
      } else {
        hipLaunchKernelGGL(k_ens_force_rhs<false>, dim3(Ctx::grid_ew(e.n), e.M), dim3(BS), 0, c.st, (int64_t)e.n,
                           (const int32_t*)e.fmask_dev, (const double*)e.fparm, reinterpret_cast<const dbl2*>(e.fnod),
                           (const dbl2*)nullptr, (const dbl2*)nullptr, (const int32_t*)nullptr, (const double*)e.c,
                           0.0, reinterpret_cast<dbl2*>(f.a));
        KCHK();
      }
    }
    if (f.per == 0) return;
    if (field == PUCFEM_F_CAPTURE_STEP) return capture_steps_get(c, e.trcap, m0 * e.ntr, nm * e.ntr, buf);
    if (field == PUCFEM_F_TRACERS) return tracers_get(c, e.trx, e.try_, m0 * e.ntr, nm * e.ntr, buf);
    if (field == PUCFEM_F_VORTICITY) ens_curl(c, e, (int32_t)m0, (int32_t)nm, true, false);
    if (f.comp > 0)  // (the members are the planes)
      c.get_all(f.comp, nm, buf, f.a + m0 * f.per);
    else
      c.d2h(buf, f.a + m0 * f.per, sizeof(double) * nm * f.per);
  });
}

int pucfem_ens_step(void* ctx, int32_t nsteps, pucfem_step_stats* stats) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    Ens& e = *ens_of(c);
    require(nsteps >= 0, "nsteps < 0");
    if (nsteps == 0) return;
    const size_t sM = (size_t)e.M;
    // one step, and gk steps, captured once each as a single chain (every buffer was allocated at create)
    auto capture = [&](int count, hipGraph_t& gr, hipGraphExec_t& ex) {
      HIPCHK(hipStreamBeginCapture(c.st, hipStreamCaptureModeThreadLocal));
      try {
        for (int k = 0; k < count; ++k) ens_enqueue_step(c);
      } catch (...) {
        hipGraph_t g = nullptr;
        (void)hipStreamEndCapture(c.st, &g);
        if (g) (void)hipGraphDestroy(g);
        throw;
      }
      HIPCHK(hipStreamEndCapture(c.st, &gr));
      HIPCHK(hipGraphInstantiate(&ex, gr, nullptr, nullptr, 0));
    };
    // (the chain has the inertial launch iff a member's flag is on: graphs of the other chain are dropped.  Which
    // members are on is read from device memory by the kernels, so it needs no new capture.)
    // (the same for the tracers' diffusion: the BROWN tracer launch iff a member's D is positive)
    // (and for the body forces: the force launch iff a member is forced, with the nodal planes once they exist)
    // (and for MacCormack: the dye's three launches iff a member's dye scheme is on, the velocity's two iff an
    // inertial member's velocity scheme is)
    // (and for the midpoint trajectories: each of their launches iff a member runs it, Ens::trj_chain)
    // (and for the tracer stretching: the STRETCH tracer launch iff a member's flag is on)
    // (and for the strokes: the stroke launch iff a member has one; pucfem_ens_set_stroke drops the graphs itself when
    // it reallocates the tables or the shared shapes)
    if (e.chain_adv != (e.adv_any > 0) || e.chain_br != (e.br_any > 0) || e.chain_force != (e.force_any > 0) ||
        e.chain_fnod != (e.fnod != nullptr) || e.chain_mcd != (e.dye_n[ENS_DYE_MC] > 0) ||
        e.chain_mcv != (e.vel_n[ENS_ADV_MC] > 0) || e.chain_stroke != (e.stroke_any > 0) ||
        e.chain_trj != e.trj_chain() || e.chain_str != (e.str_any > 0)) {
      HIPCHK(hipStreamSynchronize(c.st));
      e.drop_graphs();
      e.chain_stroke = e.stroke_any > 0;
      e.chain_adv = e.adv_any > 0;
      e.chain_br = e.br_any > 0;
      e.chain_force = e.force_any > 0;
      e.chain_fnod = e.fnod != nullptr;
      e.chain_mcd = e.dye_n[ENS_DYE_MC] > 0;
      e.chain_mcv = e.vel_n[ENS_ADV_MC] > 0;
      e.chain_trj = e.trj_chain();
      e.chain_str = e.str_any > 0;
    }
    // (and for the loads record: k_loads behind the chain iff the record is on; a changed capacity drops the graphs)
    ens_loads_ring_fit(c, e, false);
    if (!e.gexec) capture(1, e.graph, e.gexec);
    if (!e.gexec_k && c.gk > 1 && nsteps >= c.gk) capture(c.gk, e.graph_k, e.gexec_k);
    std::vector<double> h(stats ? 8 * sM * (size_t)nsteps : 0);
    HIPCHK(hipMemsetAsync(e.count, 0, sizeof(int) * sM, c.st));
    for (int s = 0, k = 0; s < nsteps;) {
      int d = 1;
      if (e.gexec_k && nsteps - s >= c.gk && k + c.gk <= e.ring_steps) {
        HIPCHK(hipGraphLaunch(e.gexec_k, c.st));
        d = c.gk;
      } else {
        HIPCHK(hipGraphLaunch(e.gexec, c.st));
      }
      s += d;
      k += d;
      if (k + 1 > e.ring_steps || s == nsteps) {  // the ring's records -> this call's records
        if (stats)
          HIPCHK(hipMemcpyAsync(h.data() + 8 * sM * (size_t)(s - k), e.ring, sizeof(double) * 8 * sM * k,
                                hipMemcpyDeviceToHost, c.st));
        if (s < nsteps) HIPCHK(hipMemsetAsync(e.count, 0, sizeof(int) * sM, c.st));
        k = 0;
      }
    }
    HIPCHK(hipStreamSynchronize(c.st));
    e.steps += nsteps;
    // the members' step counts: a setting that was never switched on has empty vectors; the velocity's count only
    // while the member's inertia is on
    auto count = [&](std::vector<int64_t>& steps, const std::vector<int32_t>& setting, int32_t on, bool inertial) {
      for (size_t m = 0; m < setting.size(); ++m)
        if (setting[m] == on && (!inertial || (!e.adv_on.empty() && e.adv_on[m]))) steps[m] += nsteps;
    };
    count(e.adv_steps, e.adv_on, 1, false);
    count(e.mc_steps, e.mc_dye, PUCFEM_ADV_MACCORMACK, false);
    count(e.mcv_steps, e.mc_vel, PUCFEM_ADV_MACCORMACK, true);
    if (e.adv_any > 0 || e.mc_dye_any > 0 || e.mc_vel_any > 0) e.adv_stale = true;
    count(e.trjd_steps, e.trj_dye, PUCFEM_TRJ_MIDPOINT, false);
    count(e.trjv_steps, e.trj_vel, PUCFEM_TRJ_MIDPOINT, true);
    count(e.trjt_steps, e.trj_trc, PUCFEM_TRJ_MIDPOINT, false);
    if (e.trj_vals) e.trj_stale = e.adv_stale = true;
    count(e.str_steps, e.str_on, 1, false);
    for (size_t m = 0; m < sM && e.force_any > 0; ++m)
      if (e.fmask[m]) e.fsteps[m] += nsteps;
    for (size_t m = 0; m < sM && e.dy_K > 0; ++m) e.dy_steps[m] += nsteps;
    if (stats)
      for (size_t k = 0; k < (size_t)nsteps * sM; ++k) {
        pucfem_step_stats& o = stats[k];
        const double* r = h.data() + 8 * k;
        o.max_div_star = r[0];
        o.max_final_div = r[1];
        o.mix_I = r[2];
        o.mix_mu = r[3];
        o.mix_var = r[4];
        o.eaten = (int64_t)std::llround(r[5]);
        o.sl_notfound = (int32_t)std::llround(r[6]);
        o.it_visc = o.it_p = o.it_p2 = 0;
      }
  });
}

// ---- sampling and rasterising (pucfem_sample.hpp)
namespace {
// a context the samplers can read: a device, built, a Stokes scheme (the others have no locator), one rank
void sample_ready(Ctx& c) {
  c.need_dev();
  c.need_built();
  auto state = [](bool ok, const char* msg) {
    if (!ok) throw Error(PUCFEM_ESTATE, msg);
  };
  state(c.scheme == PUCFEM_STOKES_COLOR || c.scheme == PUCFEM_STOKES_FOOD,
        "sampling needs a Stokes context (heat / Poisson contexts have no point locator)");
  state(!c.dist(), "sampling is single-rank (the fields of a multi-rank context are partitioned)");
  state(c.has_locator(), "the context has no point locator");
}
void sample_push(SampleFields& F, const double* p, int32_t stride, int64_t member) {
  require(F.ncomp < SMP_MAXC, "too many field components in one call (16)");
  F.ptr[F.ncomp] = p;
  F.stride[F.ncomp] = stride;
  F.member[F.ncomp] = member;
  ++F.ncomp;
}
// the components of the requested context fields, in output order.  Fields that pucfem_get_field forms when read
// are formed here too, on the context's stream, into the samplers' own buffers.
SampleFields sample_fields(Ctx& c, int32_t nfields, const int32_t* fields) {
  require(nfields >= 1 && fields != nullptr, "nfields < 1");
  SampleFields F{};
  for (int32_t k = 0; k < nfields; ++k) {
    switch (fields[k]) {
      case PUCFEM_F_U:
        sample_push(F, c.ux, VS, 0);
        sample_push(F, c.uy, VS, 0);
        break;
      case PUCFEM_F_USTAR:
        sample_push(F, c.usx, VS, 0);
        sample_push(F, c.usy, VS, 0);
        break;
      case PUCFEM_F_P:
      case PUCFEM_F_P2:
      case PUCFEM_F_DIV_STAR:
      case PUCFEM_F_DIV_U:
      case PUCFEM_F_FINAL_DIV:
      case PUCFEM_F_VORTICITY: {  // (formed, when the step does not store it, into scratch slots 4..8)
        const int32_t f = fields[k];
        const int slot = f == PUCFEM_F_P ? 4 : f == PUCFEM_F_P2 ? 5 : f == PUCFEM_F_DIV_STAR ? 6 : f == PUCFEM_F_FINAL_DIV ? 7 : 8;
        sample_push(F, c.formed(fields[k], [&] { return c.smp_scratch<double>(slot, (size_t)c.nloc); }), 1, 0);
        break;
      }
      case PUCFEM_F_C: sample_push(F, c.c_full, 1, 0); break;
      default:
        if (fields[k] >= PUCFEM_F_DYE0 && fields[k] < PUCFEM_F_DYE0 + DYE_MAX) {
          const int ch = fields[k] - PUCFEM_F_DYE0;
          require(ch < c.ndye, "dye channel index >= the number of channels");
          sample_push(F, c.dye_cur + (size_t)ch * (size_t)c.mesh.N, 1, 0);
          break;
        }
        throw Error(PUCFEM_EINVAL,
                    "not a sampled field (U, USTAR, P, P2, DIV_STAR, DIV_U, FINAL_DIV, C, VORTICITY, DYE0 + k)");
    }
  }
  return F;
}
// a raster's window, tiles and grid
struct RasterPlan {
  RasterWin R;
  int32_t tiles_x;
  int64_t ntiles, plane;
  int grid;
};
RasterPlan raster_plan(int32_t W, int32_t H, const double* w4) {
  require(W >= 1 && H >= 1, "raster width and height must be positive");
  require((int64_t)W * H <= (int64_t)0x7fffffff, "more than 2^31 - 1 pixels");
  const double dflt[4] = {0.0, 0.0, 1.0, 1.0};
  const double* w = w4 ? w4 : dflt;
  require(std::isfinite(w[0]) && std::isfinite(w[1]) && std::isfinite(w[2]) && std::isfinite(w[3]) && w[2] > w[0] &&
              w[3] > w[1],
          "degenerate window (x0 < x1 and y0 < y1, finite)");
  RasterPlan p{};
  p.R = RasterWin{w[0], w[1], w[2], w[3], W, H};
  p.tiles_x = (W + RT - 1) / RT;
  p.ntiles = (int64_t)p.tiles_x * ((H + RT - 1) / RT);
  p.plane = (int64_t)W * H;
  p.grid = (int)std::min<int64_t>(p.ntiles, 262144);
  return p;
}
void launch_raster(Ctx& c, const RasterPlan& p, const SampleFields& F, float* dout) {
  c.with_loc([&](const auto& L) {
    hipLaunchKernelGGL(k_raster<std::decay_t<decltype(L)>>, dim3(p.grid), dim3(BS), 0, c.st, L, p.R, p.tiles_x, p.ntiles,
                       F, dout);
  });
  KCHK();
}
}  // namespace

int pucfem_sample_points(void* ctx, int32_t nfields, const int32_t* fields, int64_t npoints, const double* xy,
                         double* out, int32_t* tri_out) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    sample_ready(c);
    require(npoints >= 1 && npoints <= (int64_t)0x7fffffff, "npoints must be in 1 .. 2^31 - 1");
    require(xy != nullptr && out != nullptr, "null points or output");
    const SampleFields F = sample_fields(c, nfields, fields);
    const size_t np = (size_t)npoints;
    double* dxy = c.smp_scratch<double>(0, 2 * np);
    double* dout = c.smp_scratch<double>(1, (size_t)F.ncomp * np);
    int32_t* dtri = tri_out ? c.smp_scratch<int32_t>(2, np) : nullptr;
    c.h2d(dxy, xy, sizeof(double) * 2 * np);
    const int grid = (int)std::min<int64_t>(65536, (npoints + BS - 1) / BS);
    c.with_loc([&](const auto& L) {
      hipLaunchKernelGGL(k_sample_points<std::decay_t<decltype(L)>>, dim3(grid), dim3(BS), 0, c.st, L, npoints,
                         (const double*)dxy, F, dout, dtri);
    });
    KCHK();
    c.d2h(out, dout, sizeof(double) * (size_t)F.ncomp * np);
    if (tri_out) c.d2h(tri_out, dtri, sizeof(int32_t) * np);
  });
}

int pucfem_raster(void* ctx, int32_t nfields, const int32_t* fields, int32_t width, int32_t height,
                  const double* window4, float* out) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    sample_ready(c);
    const RasterPlan p = raster_plan(width, height, window4);
    require(out != nullptr, "null output");
    const SampleFields F = sample_fields(c, nfields, fields);
    const size_t count = (size_t)F.ncomp * (size_t)p.plane;
    float* dout = c.smp_scratch<float>(1, count);
    launch_raster(c, p, F, dout);
    c.d2h(out, dout, sizeof(float) * count);
  });
}

int pucfem_ens_raster(void* ctx, int32_t nfields, const int32_t* fields, int32_t member, int32_t width, int32_t height,
                      const double* window4, float* out) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    Ens& e = *ens_of(c);
    sample_ready(c);
    require(member >= -1 && member < e.M, "member index out of range");
    const RasterPlan p = raster_plan(width, height, window4);
    require(out != nullptr, "null output");
    require(nfields >= 1 && fields != nullptr, "nfields < 1");
    SampleFields F{};
    for (int32_t k = 0; k < nfields; ++k) {
      require(fields[k] != PUCFEM_F_TRACERS && fields[k] != PUCFEM_F_STATUS, "tracer fields are not rasterised");
      require(fields[k] != PUCFEM_F_U_ADV, "u_adv is read with pucfem_ens_get_field, not rasterised");
      if (fields[k] >= PUCFEM_F_DYE0 && fields[k] < PUCFEM_F_DYE0 + DYE_MAX) {  // (the member's plane of channel k)
        const int ch = fields[k] - PUCFEM_F_DYE0;
        require(ch < e.dy_K, "dye channel index >= the ensemble's number of channels");
        sample_push(F, e.dy_cur + (size_t)ch * (size_t)e.n, 1, (i64)e.dy_K * e.n);
        continue;
      }
      const EnsField f = ens_field(c, e, fields[k]);
      for (int q = 0; q < f.comp; ++q) sample_push(F, f.a + q, f.comp, f.per);
    }
    const int32_t m0 = member < 0 ? 0 : member, nm = member < 0 ? e.M : 1;
    if (std::find(fields, fields + nfields, (int32_t)PUCFEM_F_VORTICITY) != fields + nfields)
      ens_curl(c, e, m0, nm, true, false);
    const size_t count = (size_t)nm * (size_t)F.ncomp * (size_t)p.plane;
    float* dout = c.smp_scratch<float>(1, count);
    hipLaunchKernelGGL(k_ens_raster<LocDev>, dim3(p.grid), dim3(BS), 0, c.st, c.lgrid, p.R, p.tiles_x, p.ntiles, F, m0,
                       nm, dout);
    KCHK();
    c.d2h(out, dout, sizeof(float) * count);
  });
}

int pucfem_raster_probe(void* ctx, int32_t nfields, const int32_t* fields, int32_t width, int32_t height,
                        const double* window4, int32_t iters, double* out4) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    sample_ready(c);
    const RasterPlan p = raster_plan(width, height, window4);
    require(iters >= 1 && out4 != nullptr, "iters < 1 or null output");
    const SampleFields F = sample_fields(c, nfields, fields);
    const size_t count = (size_t)F.ncomp * (size_t)p.plane;
    float* dout = c.smp_scratch<float>(1, count);
    unsigned long long* dcnt = c.smp_scratch<unsigned long long>(3, 2);
    HIPCHK(hipMemsetAsync(dcnt, 0, 2 * sizeof(unsigned long long), c.st));
    c.with_loc([&](const auto& L) {
      hipLaunchKernelGGL(k_raster_count<std::decay_t<decltype(L)>>, dim3(p.grid), dim3(BS), 0, c.st, L, p.R, p.tiles_x,
                         p.ntiles, dcnt);
    });
    KCHK();
    launch_raster(c, p, F, dout);  // (untimed: the first launch)
    out4[0] = time_launches(c, iters, [&] { launch_raster(c, p, F, dout); });
    unsigned long long h[2] = {0, 0};
    c.d2h(h, dcnt, sizeof(h));
    out4[1] = (double)h[0];
    out4[2] = (double)h[1];
    out4[3] = (double)(sizeof(float) * count);
  });
}

// ---- streamlines (pucfem_streamline.hpp)
namespace {
// the checked scalars of a streamline call; members: the lines are integrated for that many velocity fields
SlnArgs sln_args(const Ctx& c, int64_t nseeds, const double* seeds, double h, int32_t nsteps, int32_t flags,
                 double vmin, int64_t members) {
  constexpr int64_t CAP = int64_t(1) << 26;  // stored points per call (1 GiB of output): a memory guard
  require(nseeds >= 1, "nseeds < 1");
  require(nsteps >= 1, "nsteps < 1");
  require(std::isfinite(h) && h != 0.0, "the step h must be finite and non-zero");
  require(std::isfinite(vmin) && vmin >= 0.0, "the speed floor vmin must be finite and >= 0");
  require((flags & ~(SLN_UNIT | SLN_EULER | SLN_BOTH)) == 0, "unknown streamline flag bits");
  require(nseeds <= CAP, "more than 2^26 stored points ((nsteps + 1) * lines * members)");
  const int64_t lines = (flags & SLN_BOTH) ? 2 * nseeds : nseeds;
  const int64_t per = ((int64_t)nsteps + 1) * lines;  // (< 2^59)
  require(per <= CAP && per * members <= CAP, "more than 2^26 stored points ((nsteps + 1) * lines * members)");
  require(seeds != nullptr, "null seeds");
  // PUCFEM_SLN_HINT=0: every locate from scratch (the A/B of tools/streamline_bench.py; the output is the same)
  const char* hv = std::getenv("PUCFEM_SLN_HINT");
  // lanes per wave: doubled while the launch keeps enough waves (pucfem_streamline.hpp); PUCFEM_SLN_LANES=1..64
  // fixes it (the same A/B)
  const int64_t total = lines * members;
  const int64_t waves = total > SLN_MANY ? SLN_WAVES_MANY : (c.lat_sl ? SLN_WAVES_LAT : SLN_WAVES_REC);
  int32_t lanes = 1;
  while (lanes < SLN_BS && (total + 2 * lanes - 1) / (2 * lanes) >= waves) lanes *= 2;
  if (const char* lv = std::getenv("PUCFEM_SLN_LANES")) lanes = std::min(std::max(std::atoi(lv), 1), SLN_BS);
  return SlnArgs{nseeds, lines, h, vmin, nsteps, flags, hv && std::atoi(hv) == 0 ? 0 : 1, lanes};
}
// the seeds' lines in the context's own velocity; st: status (lines), then npts (lines)
void sln_launch(Ctx& c, const SlnArgs& A, const SampleFields& F, const double* dseeds, double* dpts, int32_t* dst,
                double* dval) {
  const int grid = (int)((A.lines + A.lanes - 1) / A.lanes);
  c.with_loc([&](const auto& L) {
    hipLaunchKernelGGL(k_streamlines<std::decay_t<decltype(L)>>, dim3(grid), dim3(SLN_BS), 0, c.st, L, A, dseeds,
                       (const double*)c.ux, (const double*)c.uy, F, dpts, dst, dst + A.lines, dval);
  });
  KCHK();
}
}  // namespace

int pucfem_streamlines(void* ctx, int64_t nseeds, const double* seeds, double h, int32_t nsteps, int32_t flags,
                       double vmin, int32_t nfields, const int32_t* fields, double* points, int32_t* status,
                       int32_t* npts, double* values) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    sample_ready(c);
    const SlnArgs A = sln_args(c, nseeds, seeds, h, nsteps, flags, vmin, 1);
    require(nfields >= 0 && (nfields == 0 || fields != nullptr), "nfields < 0 or null fields");
    require(points != nullptr && status != nullptr && npts != nullptr, "null output");
    require((values == nullptr) == (nfields == 0), "values must be given exactly when fields are");
    SampleFields F{};
    if (nfields > 0) F = sample_fields(c, nfields, fields);
    const size_t lines = (size_t)A.lines, per = lines * ((size_t)nsteps + 1);
    double* dseeds = c.smp_scratch<double>(10, 2 * (size_t)nseeds);
    double* dpts = c.smp_scratch<double>(11, 2 * per);
    int32_t* dst = c.smp_scratch<int32_t>(12, 2 * lines);
    double* dval = F.ncomp ? c.smp_scratch<double>(13, (size_t)F.ncomp * per) : nullptr;
    c.h2d(dseeds, seeds, sizeof(double) * 2 * (size_t)nseeds);
    sln_launch(c, A, F, dseeds, dpts, dst, dval);
    c.d2h(points, dpts, sizeof(double) * 2 * per);
    c.d2h(status, dst, sizeof(int32_t) * lines);
    c.d2h(npts, dst + lines, sizeof(int32_t) * lines);
    if (dval) c.d2h(values, dval, sizeof(double) * (size_t)F.ncomp * per);
  });
}

int pucfem_streamlines_probe(void* ctx, int64_t nseeds, const double* seeds, double h, int32_t nsteps, int32_t flags,
                             double vmin, int32_t iters, double* out2) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    sample_ready(c);
    const SlnArgs A = sln_args(c, nseeds, seeds, h, nsteps, flags, vmin, 1);
    require(iters >= 1 && out2 != nullptr, "iters < 1 or null output");
    const SampleFields F{};
    const size_t lines = (size_t)A.lines, per = lines * ((size_t)nsteps + 1);
    double* dseeds = c.smp_scratch<double>(10, 2 * (size_t)nseeds);
    double* dpts = c.smp_scratch<double>(11, 2 * per);
    int32_t* dst = c.smp_scratch<int32_t>(12, 2 * lines);
    c.h2d(dseeds, seeds, sizeof(double) * 2 * (size_t)nseeds);
    sln_launch(c, A, F, dseeds, dpts, dst, nullptr);  // (untimed: the first launch)
    out2[0] = time_launches(c, iters, [&] { sln_launch(c, A, F, dseeds, dpts, dst, nullptr); });
    out2[1] = (double)(sizeof(double) * 2 * per + sizeof(int32_t) * 2 * lines);
  });
}

int pucfem_ens_streamlines(void* ctx, int32_t member, int64_t nseeds, const double* seeds, double h, int32_t nsteps,
                           int32_t flags, double vmin, double* points, int32_t* status, int32_t* npts) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    Ens& e = *ens_of(c);
    sample_ready(c);
    require(member >= -1 && member < e.M, "member index out of range");
    const int32_t m0 = member < 0 ? 0 : member, nm = member < 0 ? e.M : 1;
    const SlnArgs A = sln_args(c, nseeds, seeds, h, nsteps, flags, vmin, nm);
    require(points != nullptr && status != nullptr && npts != nullptr, "null output");
    const size_t lines = (size_t)A.lines * (size_t)nm, per = lines * ((size_t)nsteps + 1);
    double* dseeds = c.smp_scratch<double>(10, 2 * (size_t)nseeds);
    double* dpts = c.smp_scratch<double>(11, 2 * per);
    int32_t* dst = c.smp_scratch<int32_t>(12, 2 * lines);
    c.h2d(dseeds, seeds, sizeof(double) * 2 * (size_t)nseeds);
    const int grid = (int)((A.lines + A.lanes - 1) / A.lanes);
    hipLaunchKernelGGL(k_ens_streamlines, dim3(grid, nm), dim3(SLN_BS), 0, c.st, c.lgrid, A, (const double*)dseeds,
                       (const double*)e.u, (int64_t)e.n, m0, dpts, dst, dst + lines);
    KCHK();
    c.d2h(points, dpts, sizeof(double) * 2 * per);
    c.d2h(status, dst, sizeof(int32_t) * lines);
    c.d2h(npts, dst + lines, sizeof(int32_t) * lines);
  });
}

// ---- unit operations (single rank)
int pucfem_apply(void* ctx, int32_t op, const double* x, double* y) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    c.need_dev();
    c.need_built();
    require(!c.dist(), "pucfem_apply is single-rank");
    const i64 N = c.mesh.N;
    auto perm_in = [&](const double* src, int ncomp, double* d0, double* d1) { c.put_all(ncomp, 1, src, d0, d1); };
    auto perm_out = [&](double* dst, int ncomp, double* d0, double* d1) { c.get_all(ncomp, 1, dst, d0, d1); };
    double *t0 = c.cg_pa[0], *t1 = c.cg_pa[1], *o0 = c.cg_q[0], *o1 = c.cg_q[1];
    // the unscaled action of a scaled operator, S^-1 A^ S^-1 x: x / s in (same operands, same order as one loop over
    // the permutation), A^ by `mv`, the product / s out
    auto scaled = [&](const double* ds, auto&& mv) {
      std::vector<double> s(N), v(N);
      c.d2h(s.data(), ds, sizeof(double) * N);
      to_internal(c.ord, 0, N, 1, 1, N, x, N, v.data());
      for (i64 g = 0; g < N; ++g) v[g] = v[g] / s[g];
      c.h2d(t0, v.data(), sizeof(double) * N);
      mv();
      KCHK();
      c.d2h(v.data(), o0, sizeof(double) * N);
      for (i64 g = 0; g < N; ++g) v[g] = v[g] / s[g];
      to_caller(c.ord, 0, N, 1, 1, N, y, N, v.data());
    };
    switch (op) {
      case PUCFEM_OP_K:
      case PUCFEM_OP_GX:
      case PUCFEM_OP_GY: {
        perm_in(x, 1, t0, nullptr);
        require(op == PUCFEM_OP_K || !c.lattice, "Gx / Gy alone are not applied on lattice operators (use DIV / GRAD)");
        const double* v = op == PUCFEM_OP_K ? c.dK : op == PUCFEM_OP_GX ? c.dGx : c.dGy;
        spmv_on(c.st, c.dP, c.fK.full(), v, t0, o0);
        KCHK();
        perm_out(y, 1, o0, nullptr);
        break;
      }
      case PUCFEM_OP_PRES: {
        require(c.dKp || c.dKp_raw, "no pressure operator (scheme is not Stokes)");
        if (c.lattice) {  // the unscaled merged operator (the multigrid path's)
          perm_in(x, 1, t0, nullptr);
          spmv_on(c.st, c.dPp, c.fP.full(), c.dKp_raw, t0, o0);
          KCHK();
          perm_out(y, 1, o0, nullptr);
          break;
        }
        scaled(c.dsp, [&] { spmv_on(c.st, c.dPp, FaceDev{}, c.dKp, t0, o0); });
        break;
      }
      case PUCFEM_OP_LIT: {
        require(c.dLitv, "no literal operator (scheme is Stokes)");
        perm_in(x, 1, t0, nullptr);
        spmv_on(c.st, c.dLit, FaceDev{}, c.dLitv, t0, o0);
        KCHK();
        perm_out(y, 1, o0, nullptr);
        break;
      }
      case PUCFEM_OP_DIV: {
        perm_in(x, 2, t0, t1);
        with_c16(c.dP, [&](auto c16) {
          hipLaunchKernelGGL((k_div<decltype(c16)::value, false>), dim3(c.div_grid()), dim3(BS), 0, c.st, c.dP.view(),
                             c.fK.part(), c.dGx, c.dGy, t0, t1, c.das1, o0, c.dmp, -1.0, (double*)nullptr, c.part_d, RedOut{});
        });
        KCHK();
        perm_out(y, 1, o0, nullptr);
        break;
      }
      case PUCFEM_OP_CURL: {  // (the SoA form of the same kernel: no rotated copy of x)
        perm_in(x, 2, t0, t1);
        with_c16(c.dP, [&](auto c16) {
          hipLaunchKernelGGL((k_div<decltype(c16)::value, false, true>), dim3(c.div_grid()), dim3(BS), 0, c.st,
                             c.dP.view(), c.fK.part(), c.dGx, c.dGy, t0, t1, c.das1, o0, (const double*)nullptr, 0.0,
                             (double*)nullptr, c.part_d, RedOut{});
        });
        KCHK();
        perm_out(y, 1, o0, nullptr);
        break;
      }
      case PUCFEM_OP_GRAD: {
        perm_in(x, 1, t0, nullptr);
        with_c16(c.dP, [&](auto c16) {
          hipLaunchKernelGGL(k_grad<decltype(c16)::value>, dim3(c.grid_full(c.fK.full(), c.dP)), dim3(BS), 0, c.st,
                             c.dP.view(), c.fK.full(), c.dGx, c.dGy, t0, c.das1, o0, o1);
        });
        KCHK();
        perm_out(y, 2, o0, o1);
        break;
      }
      case PUCFEM_OP_VISC: scaled(c.dsv, [&] { spmv_on(c.st, c.dP, c.fVisc.full(), c.dKv, t0, o0); }); break;
      default: throw Error(PUCFEM_EINVAL, "unknown op");
    }
  });
}

int pucfem_flow_info(void* ctx, int32_t member, double* out4) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    c.need_dev();
    c.need_built();
    if (c.scheme != PUCFEM_STOKES_COLOR && c.scheme != PUCFEM_STOKES_FOOD)
      throw Error(PUCFEM_ESTATE, "flow summaries need a Stokes context");
    if (c.dist()) throw Error(PUCFEM_ESTATE, "flow summaries are single-rank (a multi-rank context is partitioned)");
    require(out4 != nullptr, "null output");
    double h[4];
    if (member < 0) {
      require(member == -1, "member index out of range");
      double* fp = c.flow_part();
      const RedOut r{fp + 4 * MAXB, nullptr, c.dcnt + Ctx::CNT_FLOW, 4, MAXB, 0b1001u};
      c.curl(c.ux, nullptr, true, r);
      c.d2h(h, fp + 4 * MAXB, sizeof(h));
    } else {
      Ens& e = *ens_of(c);
      require(member < e.M, "member index out of range");
      ens_curl(c, e, member, 1, false, true);
      c.d2h(h, e.flow + (size_t)member * ENS_VALS, sizeof(h));
    }
    out4[0] = h[0];
    out4[1] = 0.5 * h[1];
    out4[2] = 0.5 * h[2];
    out4[3] = std::sqrt(h[3]);
  });
}

// ---- swimmer loads (pucfem_loads.hpp)
int pucfem_host_surface_edges(void* ctx, int64_t* n, int32_t* tri, int32_t* a, int32_t* b, int32_t* opp) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    require(n != nullptr, "null count");
    const SurfaceEdges& S = c.surface();
    *n = S.size();
    if (!tri && !a && !b && !opp) return;
    require(tri && a && b && opp, "either every array or none");
    std::copy(S.tri.begin(), S.tri.end(), tri);
    std::copy(S.a.begin(), S.a.end(), a);
    std::copy(S.b.begin(), S.b.end(), b);
    std::copy(S.opp.begin(), S.opp.end(), opp);
  });
}

namespace {
// the values (and with eout the per-edge values) of the context (member -1) or a member, into host arrays
void loads_read(Ctx& c, int32_t member, double* out10, double* eout) {
  if (member < 0) {
    c.loads_bufs();  // (ld_eout exists before it is named)
    c.loads_own(eout ? c.ld_eout : nullptr, LoadsRec{nullptr, nullptr, 0});
    c.d2h(out10, c.ld_out, sizeof(double) * LOADS_NV);
    if (eout) c.d2h(eout, c.ld_eout, sizeof(double) * LOADS_EV * (size_t)c.ld_nE);
    return;
  }
  Ens& e = *ens_of(c);
  require(member < e.M, "member index out of range");
  ens_loads(c, e, member, 1, eout != nullptr, LoadsRec{nullptr, nullptr, 0});
  c.d2h(out10, e.ld_out + (size_t)member * ENS_VALS, sizeof(double) * LOADS_NV);
  if (eout)
    c.d2h(eout, e.ld_eout + (size_t)member * LOADS_EV * (size_t)c.ld_nE, sizeof(double) * LOADS_EV * (size_t)c.ld_nE);
}
}  // namespace

int pucfem_swimmer_loads(void* ctx, int32_t member, double* out10) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    require(out10 != nullptr, "null output");
    require(member >= -1, "member index out of range");
    c.loads_ready(member);
    loads_read(c, member, out10, nullptr);
  });
}

int pucfem_surface_traction(void* ctx, int32_t member, double* out) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    require(out != nullptr, "null output");
    require(member >= -1, "member index out of range");
    c.loads_ready(member);
    double v[LOADS_NV];
    loads_read(c, member, v, out);
  });
}

int pucfem_loads_apply(void* ctx, const double* u, const double* p, double* out10, double* edges) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    require(u != nullptr && p != nullptr && out10 != nullptr, "null fields or output");
    c.loads_ready(-1);
    c.loads_bufs();
    const i64 N = c.mesh.N;
    // the caller's u as the step stores it and its p beside a plane of zeros (p2), in scratch: no field is touched
    double* tu = c.u_scratch();
    double* tp = c.smp_scratch<double>(24, 2 * (size_t)N);
    c.put_all(2, 1, u, tu);
    c.put_all(1, 1, p, tp);
    HIPCHK(hipMemsetAsync(tp + N, 0, sizeof(double) * (size_t)N, c.st));
    const RedOut r{c.ld_out, nullptr, c.ld_cnt, LOADS_NV, 0, 0u};
    c.loads_launch(1, tu, 0, tp, tp + N, 0, nullptr, edges ? c.ld_eout : nullptr, c.ld_part, r,
                   LoadsRec{nullptr, nullptr, 0});
    c.d2h(out10, c.ld_out, sizeof(double) * LOADS_NV);
    if (edges) c.d2h(edges, c.ld_eout, sizeof(double) * LOADS_EV * (size_t)c.ld_nE);
  });
}

int pucfem_set_loads_record(void* ctx, int32_t capacity) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    require(capacity >= 0, "capacity < 0");
    c.loads_ready(-1);
    c.loads_record_set(capacity);
    if (c.ens) ens_loads_ring_fit(c, *c.ens, true);
  });
}

int pucfem_loads_record(void* ctx, int32_t member, int64_t first, int64_t count, double* out) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    require(member >= -1, "member index out of range");
    require(first >= 0 && count >= 0, "first or count < 0");
    c.loads_ready(member);
    const double* ring = c.ld_ring;
    const int64_t* cnt = c.ld_count;
    i64 cap = c.ld_cap;
    if (member >= 0) {
      Ens& e = *ens_of(c);
      require(member < e.M, "member index out of range");
      cap = e.ld_cap;  // (0 until the ensemble's first step with the record on)
      ring = cap ? e.ld_ring + (size_t)member * cap * LOADS_ROW : nullptr;
      cnt = cap ? e.ld_count + member : nullptr;
    }
    int64_t done = 0;
    if (cnt) c.d2h(&done, cnt, sizeof(int64_t));
    const i64 held = std::min<i64>(done, cap);
    require(first + count <= held, "rows out of range (pucfem_loads_info: rows held)");
    if (count == 0) return;
    require(out != nullptr, "null output");
    std::vector<double> h((size_t)cap * LOADS_ROW);
    c.d2h(h.data(), ring, sizeof(double) * h.size());
    for (i64 k = 0; k < count; ++k) {  // (oldest first: row k of the rows held is step done - held + k)
      const i64 slot = (done - held + first + k) % cap;
      std::copy(h.begin() + slot * LOADS_ROW, h.begin() + (slot + 1) * LOADS_ROW, out + k * LOADS_ROW);
    }
  });
}

int pucfem_loads_info(void* ctx, int32_t member, int64_t* out4) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    require(out4 != nullptr, "null output");
    require(member >= -1, "member index out of range");
    c.loads_ready(member);
    const int64_t* cnt = c.ld_count;
    if (member >= 0) {
      Ens& e = *ens_of(c);
      require(member < e.M, "member index out of range");
      cnt = e.ld_cap ? e.ld_count + member : nullptr;
    }
    int64_t done = 0;
    if (cnt) c.d2h(&done, cnt, sizeof(int64_t));
    out4[0] = c.surface().size();
    out4[1] = c.mesh.T;
    out4[2] = done;
    out4[3] = c.ld_cap;
  });
}

int pucfem_loads_probe(void* ctx, int32_t iters, double* out2) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    require(iters >= 1 && out2 != nullptr, "iters < 1 or null output");
    c.loads_ready(-1);
    auto launch = [&] { c.loads_own(nullptr, LoadsRec{nullptr, nullptr, 0}); };
    launch();  // (untimed: the first launch)
    out2[0] = time_launches(c, iters, launch);
    out2[1] = c.loads_launch_bytes();
  });
}

int pucfem_solve(void* ctx, int32_t op, const double* b, double* x, double rtol, int32_t maxit, int32_t* iters) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    c.need_dev();
    c.need_built();
    require(!c.dist(), "pucfem_solve is single-rank");
    const i64 N = c.mesh.N;
    int it = 0;
    // standalone solves run on scratch buffers with their own iteration-hint slots (3, 4) and no
    // projection basis: a context that is stepping keeps u, p, the warm starts and the bases intact
    double *s0 = c.u_scratch(), *s1 = s0 + c.nloc, *s2 = s1 + c.nloc, *s3 = s2 + c.nloc;
    if (op == PUCFEM_OP_VISC) {
      // rhs = b (as u^n, initial guess b): the viscous CG without BCs
      c.put_all(2, 1, b, s0);  // (k_visc_prep reads u interleaved: s0 / s0 + 1 over 2 N of scratch)
      hipLaunchKernelGGL(k_visc_prep<false>, dim3(Ctx::grid_ew(N)), dim3(BS), 0, c.st, N, c.dsv, s0, s0 + 1,
                         c.bvx, c.bvy, c.yvx, c.yvy, VincDev{});
      KCHK();
      double* y[2] = {c.yvx, c.yvy};
      const double* bb[2] = {c.bvx, c.bvy};
      it = c.cg<2>(c.dP, c.fVisc, c.dKv, y, bb, rtol, maxit, 3);
      hipLaunchKernelGGL(k_cg_fin, dim3(Ctx::grid_ew(N)), dim3(BS), 0, c.st, N, 2, c.dsv, c.yvx, c.yvy, s2, s3,
                         (const int32_t*)nullptr);
      KCHK();
      c.get_all(2, 1, x, s2, s3);
    } else if (op == PUCFEM_OP_PRES) {
      require(c.dKp || c.dKp_raw, "no pressure operator");
      // b = b_p: braw = (M + 1e-12) * b_p, then the same path as the step (slot 4: no projection)
      std::vector<double> mp(N), br(N);
      c.d2h(mp.data(), c.dmp, sizeof(double) * N);
      to_internal(c.ord, 0, N, 1, 1, N, b, N, br.data());
      double sum = 0.0;
      for (i64 g = 0; g < N; ++g) {
        br[g] = mp[g] * br[g];
        sum += br[g];
      }
      c.h2d(c.braw, br.data(), sizeof(double) * N);
      std::vector<double> part(4 * MAXB, 0.0);
      part[MAXB] = sum;
      c.h2d(c.part_d, part.data(), sizeof(double) * part.size());
      // pressure() reduces part_d + MAXB over nb_for(dP) blocks: only entry 0 is non-zero
      HIPCHK(hipMemsetAsync(s0, 0, sizeof(double) * c.nloc, c.st));
      pucfem_params save = c.prm;
      c.prm.rtol_pres = rtol;
      c.prm.maxit_pres = maxit;
      try {
        it = c.pressure(s0, s1, 4);
      } catch (...) {
        c.prm = save;
        throw;
      }
      c.prm = save;
      c.get_all(1, 1, x, s1);
    } else if (op == PUCFEM_OP_LIT) {
      require(c.dLitv, "no literal operator");
      c.put_all(1, 1, b, c.bh);
      c.put_all(1, 1, (const double*)x, c.scalar);
      it = c.bicgstab(c.scalar, c.bh, rtol, maxit);
      c.get_all(1, 1, x, c.scalar);
    } else {
      throw Error(PUCFEM_EINVAL, "op cannot be solved");
    }
    if (iters) *iters = it;
  });
}

int pucfem_sl_advect(void* ctx, const double* cin, const double* u, double dt, double* cout, int32_t* notfound) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    c.need_dev();
    c.need_built();
    require(!c.dist() && c.has_cgrid, "sl_advect needs a single-rank Stokes context");
    const i64 N = c.mesh.N;
    double *cf = c.litw[0] ? c.litw[0] : c.cg_pa[0], *cn = c.cg_pb[0], *tx = c.u_scratch(), *ty = tx + 1;
    c.put_all(1, 1, cin, cf);
    c.put_all(2, 1, u, tx);
    const int nb = c.nb_sl(N);
    c.sl_launch(nb, 0, N, tx, ty, dt, cf, cn, c.dwmix, c.dnotfound);
    KCHK();
    c.get_all(1, 1, cout, cn);
    if (notfound) c.get_all(1, 1, notfound, c.dnotfound);
  });
}

int pucfem_apply_bc(void* ctx, int32_t which, double* u) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    c.need_dev();
    c.need_built();
    require(!c.dist() && (c.scheme == PUCFEM_STOKES_COLOR || c.scheme == PUCFEM_STOKES_FOOD),
            "apply_bc needs a single-rank Stokes context");
    require(which >= 1 && which <= 3, "apply_bc: which must be 1 (periodic), 2 (Dirichlet) or 3 (both)");
    double *tx = c.cg_q[0], *ty = c.cg_q[1];  // scratch (the step's state stays untouched)
    c.put_all(2, 1, (const double*)u, tx, ty);
    const int ncopy = (which & 1) ? c.ncopy : 0, ndir = (which & 2) ? c.ndir : 0;
    if (ncopy + ndir > 0) {
      if (c.bc_gather && ncopy > 0) {
        hipLaunchKernelGGL(k_bc_gather, dim3(std::min(1024, (ncopy + BS - 1) / BS)), dim3(BS), 0, c.st, ncopy,
                           c.dcsrc, c.dbctmp, c.dir_ncomp, tx, ty, 1);
        KCHK();
      }
      const int nb = (int)std::min<i64>(1024, std::max<i64>(1, (ncopy + ndir + BS - 1) / BS));
      hipLaunchKernelGGL(k_bc_apply, dim3(nb), dim3(BS), 0, c.st, ncopy, c.dcdst, c.dcsrc,
                         c.bc_gather ? (const double*)c.dbctmp : nullptr, ndir, c.ddnode, c.ddval, c.dir_ncomp, tx, ty,
                         1);
      KCHK();
    }
    c.get_all(2, 1, u, tx, ty);
  });
}

int pucfem_dye_step(void* ctx, const double* cin, const double* u, double* cout, int32_t* iters) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    c.need_dev();
    c.need_built();
    require(c.dye_impl, "dye_step needs a context built with dye_scheme = 1 (implicit)");
    double *tx = c.u_scratch(), *ty = tx + 1, *cf = c.cg_pa[0], *cn = c.cg_pb[0], *dv = c.litw[8];
    c.put_all(1, 1, cin, cf);
    c.put_all(2, 1, u, tx);
    c.div(tx, ty, dv, false);
    const int it = c.dye_step(tx, ty, dv, cf, cn);
    c.get_all(1, 1, cout, cn);
    if (iters) *iters = it;
  });
}

int pucfem_tracer_step(void* ctx, const double* u, double dt, int32_t nsteps) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    c.need_dev();
    c.need_built();
    require(!c.dist(), "tracer_step unit op is single-rank");
    require(c.has_tgrid, "tracer_step needs a STOKES_FOOD context (the tracer grid)");
    c.put_all(2, 1, u, c.ux);  // (u interleaved, as the step stores it)
    for (int s = 0; s < nsteps; ++s) c.tracer_advance(dt);
    HIPCHK(hipStreamSynchronize(c.st));
  });
}

int pucfem_tracer_info(void* ctx, int32_t member, int64_t* out6) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    c.need_dev();
    c.need_built();
    require(out6 != nullptr, "out is null");
    require(member >= -1, "member index out of range");
    i64 n = c.ntr;
    const double *tx = c.trx, *ty = c.try_, *ts = c.trs;
    const int32_t* stepctr = c.trstep;
    int blocks = c.tr_blocks, threads = c.tr_threads;
    if (member >= 0) {
      Ens& e = *ens_of(c);
      require(member < e.M, "member index out of range");
      n = e.ntr;
      tx = e.trx + (i64)member * n;
      ty = e.try_ + (i64)member * n;
      ts = e.trs + (i64)member * n;
      stepctr = e.trstep + member;
      blocks = e.tr_blocks;
      threads = e.tr_threads;
    }
    unsigned long long cen[2] = {0, 0};
    int32_t steps = 0;
    if (n > 0) {
      if (!c.trcensus) c.trcensus = c.dalloc<unsigned long long>(2);
      HIPCHK(hipMemsetAsync(c.trcensus, 0, sizeof(cen), c.st));
      hipLaunchKernelGGL(k_tracer_census, dim3((unsigned)std::min<i64>(TRACER_CLOUD_MAXB, (n + BS - 1) / BS)), dim3(BS),
                         0, c.st, (int64_t)n, tx, ty, ts, c.trcensus);
      KCHK();
      HIPCHK(hipMemcpyAsync(cen, c.trcensus, sizeof(cen), hipMemcpyDeviceToHost, c.st));
    }
    if (stepctr) HIPCHK(hipMemcpyAsync(&steps, stepctr, sizeof(int32_t), hipMemcpyDeviceToHost, c.st));
    HIPCHK(hipStreamSynchronize(c.st));
    out6[0] = n;
    out6[1] = (int64_t)cen[0];
    out6[2] = (int64_t)cen[1];
    out6[3] = steps;
    out6[4] = blocks;
    out6[5] = threads;
  });
}

// ---- Brownian tracers (pucfem_brownian.hpp)
int pucfem_set_tracer_diffusion(void* ctx, double D, uint64_t seed) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    c.brownian_ready();
    require(std::isfinite(D) && D >= 0.0, "D must be finite and not negative");
    c.need_dev();
    if (D == c.tr_D && seed == c.tr_seed) return;
    // (the captured small-mesh step holds the amplitude and key as kernel arguments, and the plain or the BROWN
    // launch: the next pucfem_step captures again)
    HIPCHK(hipStreamSynchronize(c.st));
    c.drop_step_graphs();
    c.tr_D = D;
    c.tr_seed = seed;
  });
}

int pucfem_ens_set_tracer_diffusion(void* ctx, int32_t member, double D, uint64_t seed) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    c.brownian_ready();
    if (!c.ens) throw Error(PUCFEM_ESTATE, "no ensemble on this context: call pucfem_ens_create first");
    Ens& e = *c.ens;
    require(std::isfinite(D) && D >= 0.0, "D must be finite and not negative");
    require(member >= -1 && member < e.M, "member index out of range");
    const size_t sM = (size_t)e.M;
    const size_t m0 = member < 0 ? 0 : (size_t)member, m1 = member < 0 ? sM : m0 + 1;
    if (e.br_D.empty()) {  // (host values only: the device buffers wait for the first D > 0)
      e.br_D.assign(sM, 0.0);
      e.br_seed.assign(sM, 0);
    }
    bool changed = false;
    for (size_t m = m0; m < m1; ++m) {
      if (e.br_D[m] == D && e.br_seed[m] == seed) continue;
      e.br_D[m] = D;
      e.br_seed[m] = seed;
      changed = true;
    }
    if (!changed) return;
    std::vector<double> a(sM);
    std::vector<uint2> key(sM);
    int any = 0;
    for (size_t m = 0; m < sM; ++m) {
      a[m] = std::sqrt(6.0 * e.br_D[m] * c.prm.dt);
      key[m] = make_uint2((uint32_t)(e.br_seed[m] & 0xffffffffu), (uint32_t)(e.br_seed[m] >> 32));
      any += e.br_D[m] > 0.0 ? 1 : 0;
    }
    e.br_any = any;
    if (!e.br_a) {
      if (any == 0) return;  // (nothing was ever on: nothing is allocated and nothing launched)
      e.br_a = e.alloc<double>(sM, c.st);
      e.br_key = e.alloc<uint2>(sM, c.st);
    }
    c.h2d(e.br_a, a.data(), sizeof(double) * sM);
    c.h2d(e.br_key, key.data(), sizeof(uint2) * sM);
    HIPCHK(hipStreamSynchronize(c.st));
  });
}

int pucfem_get_tracer_diffusion(void* ctx, int32_t member, double* D, uint64_t* seed) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    c.brownian_ready();
    double d = c.tr_D;
    uint64_t s = c.tr_seed;
    if (member != -1) {
      if (!c.ens) throw Error(PUCFEM_ESTATE, "no ensemble on this context: call pucfem_ens_create first");
      require(member >= 0 && member < c.ens->M, "member index out of range");
      const bool have = !c.ens->br_D.empty();
      d = have ? c.ens->br_D[(size_t)member] : 0.0;
      s = have ? c.ens->br_seed[(size_t)member] : 0;
    }
    c.need_dev();
    if (D) *D = d;
    if (seed) *seed = s;
  });
}

int pucfem_tracer_probe(void* ctx, double dt, int32_t iters, double* out2) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    c.brownian_ready();
    c.need_dev();
    require(iters >= 1 && out2 != nullptr, "iters < 1 or null output");
    require(c.has_tgrid && c.ntr > 0, "tracer_probe needs a STOKES_FOOD context with tracers");
    auto launch = [&] { c.tracer_advance(dt); };
    launch();  // (untimed: the first launch)
    out2[0] = time_launches(c, iters, launch);
    out2[1] = (double)c.ntr;
  });
}

// ---- tracer stretching (the STRETCH tracer kernels and k_tracer_stretch, pucfem_kernels_impl.hpp)
int pucfem_set_tracer_stretch(void* ctx, int32_t on) {
  return guard(ctx, [&] { C(ctx)->set_stretch(on != 0); });
}

int pucfem_ens_set_tracer_stretch(void* ctx, int32_t member, int32_t on) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    c.stretch_ready();
    Ens& e = *ens_of(c);
    if (e.ntr <= 0) throw Error(PUCFEM_ESTATE, "tracer stretching needs a STOKES_FOOD ensemble with tracers");
    require(member >= -1 && member < e.M, "member index out of range");
    const size_t sM = (size_t)e.M;
    const size_t m0 = member < 0 ? 0 : (size_t)member, m1 = member < 0 ? sM : m0 + 1;
    const int32_t flag = on != 0 ? 1 : 0;
    if (e.str_on.empty()) {  // (nothing was ever on: nothing is allocated until now)
      if (!flag) return;
      const size_t before = e.bytes;
      e.str_F = e.alloc<double>(sM * 4 * (size_t)e.ntr, c.st);
      e.str_on_dev = e.alloc<int32_t>(sM, c.st);
      e.str_part = e.alloc<double>(sM * STRETCH_NV * TRACER_CLOUD_MAXB, c.st);
      e.str_out = e.alloc<double>(sM * STRETCH_NV, c.st);
      e.str_cnt = e.alloc<unsigned>(sM, c.st);
      e.str_bytes = e.bytes - before;
      c.stretch_identity(e.str_F, 0, (i64)sM * e.ntr);
      e.str_on.assign(sM, 0);
      e.str_steps.assign(sM, 0);
    }
    bool changed = false;
    for (size_t m = m0; m < m1; ++m) {
      if (e.str_on[m] == flag) continue;
      e.str_on[m] = flag;
      changed = true;
      // (switched on: F starts from the identity; switched off: the member's rows read as the identity again)
      c.stretch_identity(e.str_F, (i64)m * e.ntr, e.ntr);
      e.str_steps[m] = 0;
    }
    if (changed) {
      e.str_any = (int)std::count(e.str_on.begin(), e.str_on.end(), 1);
      c.h2d(e.str_on_dev, e.str_on.data(), sizeof(int32_t) * sM);
    }
    HIPCHK(hipStreamSynchronize(c.st));
  });
}

int pucfem_tracer_stretch_info(void* ctx, int32_t member, double* out8) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    c.stretch_ready();
    require(out8 != nullptr, "out is null");
    require(member >= -1, "member index out of range");
    for (int k = 0; k < 8; ++k) out8[k] = 0.0;
    i64 n = c.ntr;
    const double* F = c.str_on ? c.str_F : nullptr;
    double *part = nullptr, *out = nullptr;
    unsigned* cnt = nullptr;
    if (member >= 0) {
      Ens& e = *ens_of(c);
      require(member < e.M, "member index out of range");
      if (e.str_on.empty()) return;
      const size_t m = (size_t)member;
      n = e.ntr;
      F = e.str_F + m * 4 * (size_t)n;
      part = e.str_part + m * STRETCH_NV * TRACER_CLOUD_MAXB;
      out = e.str_out + m * STRETCH_NV;
      cnt = e.str_cnt + m;
      out8[0] = e.str_on[m];
      out8[1] = (double)e.str_steps[m];
    } else {
      if (!F) return;
      if (!c.str_part) {
        c.mc_alloc(c.str_part, (size_t)STRETCH_NV * TRACER_CLOUD_MAXB);
        c.mc_alloc(c.str_out, (size_t)STRETCH_NV);
        c.mc_alloc(c.str_cnt, (size_t)1);
      }
      part = c.str_part;
      out = c.str_out;
      cnt = c.str_cnt;
      out8[0] = 1.0;
      out8[1] = (double)c.str_steps;
    }
    const unsigned nb = (unsigned)std::max<i64>(1, std::min<i64>(TRACER_CLOUD_MAXB, (n + BS - 1) / BS));
    hipLaunchKernelGGL(k_tracer_stretch, dim3(nb, 1), dim3(BS), 0, c.st, (int64_t)n, F, part, out, cnt);
    KCHK();
    double v[STRETCH_NV];
    c.d2h(v, out, sizeof(v));
    out8[2] = v[0];
    out8[3] = v[1];
    out8[4] = v[2];
    out8[5] = stretch_min_key(v[3]);
    out8[6] = v[4];
    out8[7] = v[5];
  });
}

// (I, mu, var) of c with the node weights w (device, internal order) over the N nodes of a single-rank
// context: the two weighted sums, then the weighted variance about mu (k_mix2), then k_stats
static void mixing_dev(Ctx& c, const double* cf, const double* w, double* out3);
static void mixing_on(Ctx& c, const double* cin, const double* w, double* out3) {
  double* cf = c.cg_pa[0];
  c.put_all(1, 1, cin, cf);
  mixing_dev(c, cf, w, out3);
}
// the same of a field cf already on the device (internal order; pucfem_dyes_mixing: a channel where it lies)
static void mixing_dev(Ctx& c, const double* cf, const double* w, double* out3) {
  const i64 N = c.mesh.N;
  const int nb = c.nb_rows(N);
  // part_a[0..] = sum w c (the second dot, w w, is not used)
  hipLaunchKernelGGL(k_dot2, dim3(nb), dim3(BS), 0, c.st, N, w, (const double*)cf, w, w, c.part_a);
  KCHK();
  hipLaunchKernelGGL(k_reduce, dim3(1), dim3(RB), 0, c.st, c.part_a, nb, MAXB, 1, 0, c.vals + 2);
  std::vector<double> ones(N, 1.0);
  double* on = c.cg_pb[0];
  HIPCHK(hipMemcpyAsync(on, ones.data(), sizeof(double) * N, hipMemcpyHostToDevice, c.st));
  hipLaunchKernelGGL(k_dot2, dim3(nb), dim3(BS), 0, c.st, N, w, (const double*)on, (const double*)nullptr,
                     (const double*)nullptr, c.part_b);
  hipLaunchKernelGGL(k_reduce, dim3(1), dim3(RB), 0, c.st, c.part_b, nb, MAXB, 1, 0, c.vals + 3);
  hipLaunchKernelGGL(k_mix2, dim3(nb), dim3(BS), 0, c.st, (int64_t)0, N, cf, w, c.vals + 2, 1, 1, c.part_c, RedOut{});
  hipLaunchKernelGGL(k_reduce, dim3(1), dim3(RB), 0, c.st, c.part_c, nb, MAXB, 1, 0, c.vals + 5);
  HIPCHK(hipMemsetAsync(c.vals + 6, 0, 2 * sizeof(double), c.st));
  double* rec = c.vals + 8;
  hipLaunchKernelGGL(k_stats, dim3(1), dim3(64), 0, c.st, c.vals, rec, 7);
  KCHK();
  double h[8];
  HIPCHK(hipMemcpyAsync(h, rec, sizeof(double) * 7, hipMemcpyDeviceToHost, c.st));
  HIPCHK(hipStreamSynchronize(c.st));
  out3[0] = h[2];
  out3[1] = h[3];
  out3[2] = h[4];
}

int pucfem_mixing_index(void* ctx, const double* cin, double* out3) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    c.need_dev();
    c.need_built();
    require(!c.dist(), "mixing_index unit op is single-rank");
    mixing_on(c, cin, c.dwmix, out3);
  });
}

int pucfem_mixing_index_w(void* ctx, const double* cin, const double* w, double* out3) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    c.need_dev();
    c.need_built();
    require(!c.dist(), "mixing_index unit op is single-rank");
    require(w != nullptr, "mixing_index_w: weights");
    double* dw = c.cg_q[0];
    c.put_all(1, 1, w, dw);
    mixing_on(c, cin, dw, out3);
  });
}

// ---- dye channels (pucfem_dye_channels.hpp)
int pucfem_dyes_info(void* ctx, int64_t* out4) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    c.dye_ready();
    require(out4 != nullptr, "null output");
    out4[0] = c.ndye;
    out4[1] = c.dye_steps;
    out4[2] = c.nf_rows(c.dye_nfpart, c.dye_nb);
    out4[3] = (int64_t)c.dye_dev_bytes();
  });
}

int pucfem_dyes_mixing(void* ctx, double* out) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    c.dye_ready();
    require(out != nullptr || c.ndye == 0, "null output");
    for (int k = 0; k < c.ndye; ++k) mixing_dev(c, c.dye_cur + (size_t)k * (size_t)c.mesh.N, c.dwmix, out + 3 * k);
  });
}

int pucfem_sl_advect_multi(void* ctx, int32_t nch, const double* cin, const double* u, double dt, double* cout,
                           int32_t* notfound) {
  return guard(ctx, [&] { advect_fields_unit(*C(ctx), {}, nch, cin, u, dt, cout, notfound, nullptr, true); });
}

int pucfem_dyes_probe(void* ctx, int32_t nch, int32_t iters, double* out2) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    c.dye_ready();
    require(nch >= 1 && nch <= DYE_MAX, "nch must be in 1 .. PUCFEM_MAX_DYES (16)");
    require(iters >= 1 && out2 != nullptr, "iters < 1 or null output");
    transport_probe(c, {}, nch, iters, out2);
    out2[1] = c.dye_launch_bytes(nch, c.mesh.N);
  });
}

// ---- inertia (pucfem_inertia.hpp)
int pucfem_set_inertia(void* ctx, int32_t on) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    c.set_inertia(on != 0);
  });
}

int pucfem_inertia_info(void* ctx, int64_t* out4) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    c.inertia_ready();
    require(out4 != nullptr, "null output");
    out4[0] = c.inertia ? 1 : 0;
    out4[1] = c.adv_steps;
    out4[2] = c.nf_rows(c.adv_nfpart, c.adv_nb);
    out4[3] = (int64_t)c.inertia_dev_bytes();
  });
}

int pucfem_sl_advect_vel(void* ctx, const double* f, const double* u, double dt, double* f_out, int32_t* notfound) {
  return guard(ctx, [&] { advect_pairs_unit(*C(ctx), {}, f, u, dt, f_out, notfound, nullptr, true); });
}

int pucfem_inertia_probe(void* ctx, int32_t iters, double* out2) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    c.inertia_ready();
    require(iters >= 1 && out2 != nullptr, "iters < 1 or null output");
    transport_probe(c, {}, 0, iters, out2);
    out2[1] = c.vel_launch_bytes(c.mesh.N);
  });
}

// ---- body forces (pucfem_force.hpp)
static_assert(PUCFEM_F_FORCE == 15 && PUCFEM_F_U_RHS == 16, "the fields' numbers are part of the ABI");
namespace {
bool finite2(const double* v) { return std::isfinite(v[0]) && std::isfinite(v[1]); }
}  // namespace

int pucfem_set_force(void* ctx, const double* F2, const double* field) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    if (F2) require(finite2(F2), "the force must be finite");
    c.force_ready();
    const i64 N = c.mesh.N, no = c.lp.n_own;
    if (field) {
      bool ok = true;
      for (i64 k = 0; k < 2 * N && ok; ++k) ok = std::isfinite(field[k]);
      require(ok, "the force field must be finite");
    }
    c.need_dev();
    const bool uni = F2 && (F2[0] != 0.0 || F2[1] != 0.0);
    if (!uni && !field && !c.f_uni && !c.f_nodal) return;  // (off stays off: the step's state is not touched)
    c.f_uni = uni;
    c.f_F[0] = c.f_uni ? F2[0] : 0.0;
    c.f_F[1] = c.f_uni ? F2[1] : 0.0;
    if (field) {  // (the owned rows' pairs, in the internal numbering)
      if (!c.f_nodal) HIPCHK(hipMalloc(reinterpret_cast<void**>(&c.f_nodal), sizeof(double) * 2 * (size_t)std::max<i64>(1, no)));
      HIPCHK(hipStreamSynchronize(c.st));  // (a step still reading the old field)
      c.put(c.ord, c.lp.r0, no, 2, 1, field, c.f_nodal);
      HIPCHK(hipStreamSynchronize(c.st));
    } else if (c.f_nodal) {
      HIPCHK(hipStreamSynchronize(c.st));
      (void)hipFree(c.f_nodal);
      c.f_nodal = nullptr;
    }
    c.force_changed();
  });
}

int pucfem_set_buoyancy(void* ctx, const double* g2, int32_t nterms, const int32_t* fields, const double* beta,
                        const double* ref) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    require(nterms >= 0 && nterms <= FORCE_MAX_TERMS, "nterms must be in 0 .. 17 (c and PUCFEM_MAX_DYES channels)");
    if (nterms > 0) {
      require(g2 != nullptr && fields != nullptr && beta != nullptr && ref != nullptr, "null buoyancy arguments");
      require(finite2(g2), "g must be finite");
      for (int t = 0; t < nterms; ++t) {
        require(std::isfinite(beta[t]) && std::isfinite(ref[t]), "beta and ref must be finite");
        require(fields[t] == PUCFEM_F_C || (fields[t] >= PUCFEM_F_DYE0 && fields[t] < PUCFEM_F_DYE0 + DYE_MAX),
                "a buoyancy field is PUCFEM_F_C or PUCFEM_F_DYE0 + k");
        for (int q = 0; q < t; ++q) require(fields[q] != fields[t], "a buoyancy field is named twice");
      }
    }
    c.buoyancy_ready();
    for (int t = 0; t < nterms; ++t)
      if (fields[t] != PUCFEM_F_C && fields[t] - PUCFEM_F_DYE0 >= c.ndye)
        throw Error(PUCFEM_ESTATE, "a buoyancy term names a dye channel the context does not have");
    c.need_dev();
    if (nterms == 0 && c.b_n == 0) return;  // (off stays off)
    c.b_n = nterms;
    for (int t = 0; t < nterms; ++t) {
      c.b_field[t] = fields[t];
      c.b_beta[t] = beta[t];
      c.b_ref[t] = ref[t];
    }
    c.b_g[0] = nterms ? g2[0] : 0.0;
    c.b_g[1] = nterms ? g2[1] : 0.0;
    c.force_changed();
  });
}

int pucfem_force_info(void* ctx, int32_t member, int64_t* out4) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    require(out4 != nullptr, "null output");
    require(member >= -1, "member index out of range");
    c.force_ready();
    if (member >= 0) {  // (an ensemble member's own setting)
      require(c.ens == nullptr || member < c.ens->M, "member index out of range");
      Ens& e = *ens_of(c);
      const bool have = !e.fmask.empty();
      out4[0] = have ? e.fmask[(size_t)member] : 0;
      out4[1] = have ? e.fsteps[(size_t)member] : 0;
      out4[2] = have && (e.fmask[(size_t)member] & 4) ? 1 : 0;
      out4[3] = (int64_t)e.force_bytes;
      return;
    }
    c.need_dev();
    out4[0] = c.force_mask();
    out4[1] = c.force_steps;
    out4[2] = c.b_n;
    out4[3] = (int64_t)c.force_dev_bytes();
  });
}

int pucfem_force_apply(void* ctx, const double* base, double dt, double* out) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    require(base != nullptr && out != nullptr, "null fields");
    require(std::isfinite(dt), "dt must be finite");
    c.force_ready();
    c.need_dev();
    const i64 no = c.lp.n_own;
    double* din = c.smp_scratch<double>(14, 2 * (size_t)no);
    double* dout = c.smp_scratch<double>(15, 2 * (size_t)no);
    c.put(c.ord, c.lp.r0, no, 2, 1, base, din);
    c.sl_join();
    c.force_launch<true>(din, dt, dout);
    c.get(c.ord, c.lp.r0, no, 2, 1, out, (const double*)dout);
  });
}

int pucfem_force_probe(void* ctx, int32_t iters, double* out2) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    require(iters >= 1 && out2 != nullptr, "iters < 1 or null output");
    c.force_ready();
    c.need_dev();
    const i64 no = c.lp.n_own;
    double* dout = c.smp_scratch<double>(15, 2 * (size_t)no);
    c.sl_join();
    auto launch = [&] { c.force_launch<true>(c.ux, c.prm.dt, dout); };
    launch();  // (untimed: the first launch)
    out2[0] = time_launches(c, iters, launch);
    out2[1] = c.force_launch_bytes(c.force_mask(), c.b_n, no);
  });
}

// ---- time-dependent strokes (pucfem_stroke.hpp)
namespace {
// a stroke's arguments (PUCFEM_EINVAL): the positions in the Dirichlet value array of its driven nodes
void stroke_check(const Ctx& c, int32_t K, int32_t P, const double* amp, int32_t n, const int32_t* nodes,
                  const double* shape, const double* dir, int64_t start, std::vector<i32>& q) {
  require(K >= 1 && K <= STROKE_MAX_MODES, "K must be in 0 .. 8 (0 clears the stroke)");
  require(P >= 1 && P <= STROKE_MAX_PERIOD, "P must be in 1 .. 65536");
  require(start >= 0, "start < 0");
  require(amp != nullptr && nodes != nullptr && shape != nullptr && dir != nullptr, "null stroke arguments");
  require(n >= 1 && (int64_t)n <= c.mesh.N, "the count of driven nodes must be in 1 .. N");
  auto finite = [](const double* v, size_t k) {
    for (size_t i = 0; i < k; ++i)
      if (!std::isfinite(v[i])) return false;
    return true;
  };
  require(finite(amp, (size_t)P * K), "the table must be finite");
  require(finite(shape, (size_t)n * K) && finite(dir, 2 * (size_t)n), "the shapes and directions must be finite");
  const std::vector<i32> pos = c.dir_positions();
  std::vector<char> seen((size_t)c.mesh.N, 0);
  q.assign((size_t)n, 0);
  for (int32_t i = 0; i < n; ++i) {
    require(nodes[i] >= 0 && (int64_t)nodes[i] < c.mesh.N, "a driven node is out of range");
    require(pos[nodes[i]] >= 0, "a driven node is not in the Dirichlet list");
    require(!seen[nodes[i]], "a driven node is listed twice");
    seen[nodes[i]] = 1;
    q[i] = pos[nodes[i]];
  }
}
// the values of the device array val (positions) in the caller's list order: a duplicate entry gets the kept value
void dirichlet_out(Ctx& c, const double* val, double* out) {
  const int nc = c.dir_ncomp;
  std::vector<double> h((size_t)nc * std::max(1, c.ndir));
  c.d2h(h.data(), val, sizeof(double) * (size_t)nc * c.ndir);
  const std::vector<i32> pos = c.dir_positions();
  for (size_t k = 0; k < c.dir_nodes.size(); ++k)
    for (int q = 0; q < nc; ++q) out[nc * k + q] = h[(size_t)nc * pos[c.dir_nodes[k]] + q];
}
// the members' parameters and tables as k_ens_stroke_bc reads them (members given one table share its copy); the
// tables' buffer grows by reallocation, which drops the captured graphs
void ens_stroke_upload(Ctx& c, Ens& e) {
  const size_t sM = (size_t)e.M;
  std::vector<double> tab;
  for (size_t m = 0; m < sM; ++m) {
    int64_t* p = e.sk_par.data() + m * ENS_STROKE_PARM;
    p[3] = 0;
    if (p[0] == 0) continue;
    const std::vector<double>& t = e.sk_amp[m];
    size_t k = 0;  // (an earlier member with an equal table: member = -1 gives every member the same one)
    while (k < m && !(e.sk_par[k * ENS_STROKE_PARM] != 0 && e.sk_amp[k] == t)) ++k;
    if (k < m) {
      p[3] = e.sk_par[k * ENS_STROKE_PARM + 3];
      continue;
    }
    p[3] = (int64_t)tab.size();
    tab.insert(tab.end(), t.begin(), t.end());
  }
  e.stroke_any = 0;
  for (size_t m = 0; m < sM; ++m) e.stroke_any += e.sk_par[m * ENS_STROKE_PARM] != 0 ? 1 : 0;
  HIPCHK(hipStreamSynchronize(c.st));
  if (tab.size() > e.sk_cap) {
    if (e.sk_tab) {
      (void)hipFree(e.sk_tab);
      e.allocs.erase(std::find(e.allocs.begin(), e.allocs.end(), (void*)e.sk_tab));
      e.bytes -= sizeof(double) * e.sk_cap;
      e.stroke_bytes -= sizeof(double) * e.sk_cap;
    }
    e.sk_cap = std::max<size_t>({tab.size(), 2 * e.sk_cap, 4096});  // (room for small tables: no new capture per set)
    e.sk_tab = e.alloc<double>(e.sk_cap, c.st);
    e.stroke_bytes += sizeof(double) * e.sk_cap;
    e.drop_graphs();
  }
  if (!tab.empty()) c.h2d(e.sk_tab, tab.data(), sizeof(double) * tab.size());
  c.h2d(e.sk_parm, e.sk_par.data(), sizeof(int64_t) * e.sk_par.size());
  HIPCHK(hipStreamSynchronize(c.st));
}
}  // namespace

int pucfem_set_stroke(void* ctx, int32_t K, int32_t P, const double* amp, int32_t n, const int32_t* nodes,
                      const double* shape, const double* dir, int64_t start) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    c.stroke_ready();
    if (K == 0) {  // (off stays off: the step's state is not touched)
      c.drop_stroke(true);
      return;
    }
    if (c.ens) throw Error(PUCFEM_ESTATE, "the context has an ensemble: its members carry their own strokes (pucfem_ens_set_stroke)");
    std::vector<i32> q;
    stroke_check(c, K, P, amp, n, nodes, shape, dir, start, q);
    c.drop_stroke(true);  // (entries the new stroke does not drive hold build's values)
    c.sk_amp = c.stroke_buf(amp, (size_t)P * K);
    c.sk_shape = c.stroke_buf(shape, (size_t)n * K);
    c.sk_dir = c.stroke_buf(dir, 2 * (size_t)n);
    c.sk_q = c.stroke_buf<i32>(q.data(), (size_t)n);
    c.sk_ctr = c.stroke_buf<i64>(nullptr, 1);
    HIPCHK(hipStreamSynchronize(c.st));  // (the arguments are the caller's)
    c.sk_K = K;
    c.sk_P = P;
    c.sk_start = start % P;
    c.sk_n = n;
    c.have_vinc = 0;  // (as a force change: the boundary data of the viscous solve change)
  });
}

int pucfem_ens_set_stroke(void* ctx, int32_t member, int32_t K, int32_t P, const double* amp, int32_t n,
                          const int32_t* nodes, const double* shape, const double* dir, int64_t start) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    c.stroke_ready();
    Ens& e = *ens_of(c);
    require(member >= -1 && member < e.M, "member index out of range");
    const size_t sM = (size_t)e.M, m0 = member < 0 ? 0 : (size_t)member, m1 = member < 0 ? sM : (size_t)member + 1;
    if (K == 0) {  // off: the member's values as pucfem_ens_create uploaded them, its counter at 0
      if (e.sk_par.empty()) return;
      bool any = false;
      for (size_t m = m0; m < m1; ++m) {
        if (e.sk_par[m * ENS_STROKE_PARM] == 0) continue;
        any = true;
        std::fill_n(e.sk_par.begin() + m * ENS_STROKE_PARM, ENS_STROKE_PARM, (int64_t)0);
        e.sk_amp[m].clear();
        c.h2d(e.dval + m * e.dstride, e.dval0.data() + m * e.dstride, sizeof(double) * (size_t)e.dstride);
        HIPCHK(hipMemsetAsync(e.sk_ctr + m, 0, sizeof(int64_t), c.st));
      }
      if (any) ens_stroke_upload(c, e);
      return;
    }
    std::vector<i32> q;
    stroke_check(c, K, P, amp, n, nodes, shape, dir, start, q);
    const bool same = e.sk_n == n && e.sk_K == K && std::equal(nodes, nodes + n, e.sk_nodes.begin()) &&
                      std::equal(shape, shape + (size_t)n * K, e.sk_shape_h.begin()) &&
                      std::equal(dir, dir + 2 * (size_t)n, e.sk_dir_h.begin());
    if (!same) {  // the shared shapes: those of the first call, replaced only while no member has a stroke
      require(e.stroke_any == 0, "the shapes differ from the ensemble's: clear every member's stroke first");
      HIPCHK(hipStreamSynchronize(c.st));
      for (void** p : {(void**)&e.sk_shape, (void**)&e.sk_dir, (void**)&e.sk_q})
        if (*p) {
          (void)hipFree(*p);
          e.allocs.erase(std::find(e.allocs.begin(), e.allocs.end(), *p));
          *p = nullptr;
        }
      const size_t old = e.sk_n > 0 ? (sizeof(double) * (e.sk_K + 2) + sizeof(int32_t)) * (size_t)e.sk_n : 0;
      e.bytes -= old;
      e.stroke_bytes -= old;
      const size_t before = e.bytes;
      e.sk_shape = e.alloc<double>((size_t)n * K, c.st);
      e.sk_dir = e.alloc<double>(2 * (size_t)n, c.st);
      e.sk_q = e.alloc<int32_t>((size_t)n, c.st);
      if (!e.sk_parm) {
        e.sk_parm = e.alloc<int64_t>(sM * ENS_STROKE_PARM, c.st);
        e.sk_ctr = e.alloc<int64_t>(sM, c.st);
        e.sk_par.assign(sM * ENS_STROKE_PARM, 0);
        e.sk_amp.assign(sM, {});
      }
      e.stroke_bytes += e.bytes - before;
      e.sk_n = n;
      e.sk_K = K;
      e.sk_nodes.assign(nodes, nodes + n);
      e.sk_shape_h.assign(shape, shape + (size_t)n * K);
      e.sk_dir_h.assign(dir, dir + 2 * (size_t)n);
      c.h2d(e.sk_shape, shape, sizeof(double) * (size_t)n * K);
      c.h2d(e.sk_dir, dir, sizeof(double) * 2 * (size_t)n);
      c.h2d(e.sk_q, q.data(), sizeof(int32_t) * (size_t)n);
      HIPCHK(hipStreamSynchronize(c.st));
      e.drop_graphs();  // (they hold the old arrays as kernel arguments)
    }
    const std::vector<double> table(amp, amp + (size_t)P * K);
    for (size_t m = m0; m < m1; ++m) {
      int64_t* p = e.sk_par.data() + m * ENS_STROKE_PARM;
      p[0] = K;
      p[1] = P;
      p[2] = start % P;
      e.sk_amp[m] = table;
      HIPCHK(hipMemsetAsync(e.sk_ctr + m, 0, sizeof(int64_t), c.st));
    }
    ens_stroke_upload(c, e);
  });
}

int pucfem_stroke_info(void* ctx, int32_t member, int64_t* out6) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    require(out6 != nullptr, "null output");
    require(member >= -1, "member index out of range");
    c.stroke_ready();
    int64_t K = c.sk_K, P = c.sk_P, start = c.sk_start, s = 0, n = c.sk_n;
    if (member >= 0) {  // (an ensemble member's own stroke)
      require(c.ens == nullptr || member < c.ens->M, "member index out of range");
      Ens& e = *ens_of(c);
      const int64_t* p = e.sk_par.empty() ? nullptr : e.sk_par.data() + (size_t)member * ENS_STROKE_PARM;
      K = p ? p[0] : 0;
      P = p ? p[1] : 0;
      start = p ? p[2] : 0;
      n = K ? e.sk_n : 0;
      if (K) c.d2h(&s, e.sk_ctr + member, sizeof(int64_t));
    } else if (K) {
      c.d2h(&s, c.sk_ctr, sizeof(int64_t));
    }
    out6[0] = K;
    out6[1] = P;
    out6[2] = start;
    out6[3] = s;
    out6[4] = K ? (start + s) % P : 0;
    out6[5] = n;
  });
}

int pucfem_get_dirichlet(void* ctx, int32_t member, double* out) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    require(out != nullptr, "null output");
    require(member >= -1, "member index out of range");
    c.need_built();
    if (c.dist() || c.world != 1) throw Error(PUCFEM_ESTATE, "the Dirichlet values are read on single-rank contexts");
    c.need_dev();
    if (member < 0) {
      dirichlet_out(c, c.ddval, out);
      return;
    }
    require(c.ens == nullptr || member < c.ens->M, "member index out of range");
    Ens& e = *ens_of(c);
    dirichlet_out(c, e.dval + (size_t)member * e.dstride, out);
  });
}

int pucfem_stroke_apply(void* ctx, int32_t member, int64_t row, double* out) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    require(out != nullptr, "null output");
    require(member >= -1, "member index out of range");
    c.stroke_ready();
    const size_t nd = 2 * (size_t)std::max(1, c.ndir);
    if (member < 0) {
      if (!c.stroked()) throw Error(PUCFEM_ESTATE, "no stroke is set");
      require(row >= 0 && row < c.sk_P, "row must be in 0 .. P - 1");
      double* s = c.smp_scratch<double>(22, nd + 1);
      HIPCHK(hipMemcpyAsync(s, c.ddval, sizeof(double) * 2 * (size_t)c.ndir, hipMemcpyDeviceToDevice, c.st));
      c.stroke_launch(nullptr, row, s);
      dirichlet_out(c, s, out);
      return;
    }
    require(c.ens == nullptr || member < c.ens->M, "member index out of range");
    Ens& e = *ens_of(c);
    const int64_t* p = e.sk_par.empty() ? nullptr : e.sk_par.data() + (size_t)member * ENS_STROKE_PARM;
    if (!p || p[0] == 0) throw Error(PUCFEM_ESTATE, "the member has no stroke");
    require(row >= 0 && row < p[1], "row must be in 0 .. P - 1");
    double* s = c.smp_scratch<double>(22, nd + 1);
    HIPCHK(hipMemcpyAsync(s, e.dval + (size_t)member * e.dstride, sizeof(double) * 2 * (size_t)c.ndir,
                          hipMemcpyDeviceToDevice, c.st));
    hipLaunchKernelGGL(k_ens_stroke_bc, dim3(1), dim3(BS), 0, c.st, member, (const int64_t*)e.sk_parm, e.sk_ctr,
                       (int64_t)row, (const double*)e.sk_tab, e.sk_n, (const int32_t*)e.sk_q,
                       (const double*)e.sk_shape, reinterpret_cast<const dbl2*>(e.sk_dir), s, (int64_t)e.dstride);
    KCHK();
    dirichlet_out(c, s, out);
  });
}

int pucfem_stroke_probe(void* ctx, int32_t iters, double* out2) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    require(iters >= 1 && out2 != nullptr, "iters < 1 or null output");
    c.stroke_ready();
    if (!c.stroked()) throw Error(PUCFEM_ESTATE, "no stroke is set");
    // the step's launch (counter read, barrier, counter store) on a scratch copy of the values and a scratch counter
    const size_t nd = 2 * (size_t)std::max(1, c.ndir);
    double* s = c.smp_scratch<double>(22, nd + 1);
    i64* ctr = reinterpret_cast<i64*>(s + nd);
    HIPCHK(hipMemcpyAsync(s, c.ddval, sizeof(double) * 2 * (size_t)c.ndir, hipMemcpyDeviceToDevice, c.st));
    HIPCHK(hipMemsetAsync(ctr, 0, sizeof(i64), c.st));
    auto launch = [&] { c.stroke_launch(ctr, 0, s); };
    launch();  // (untimed: the first launch)
    out2[0] = time_launches(c, iters, launch);
    out2[1] = c.stroke_launch_bytes();
  });
}

// ---- MacCormack advection (pucfem_maccormack.hpp)
int pucfem_set_advection(void* ctx, int32_t what, int32_t scheme) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    c.set_advection(what, scheme);
  });
}

int pucfem_advection_info(void* ctx, int64_t* out11) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    c.inertia_ready();  // (a single-rank Stokes context on a device, built)
    require(out11 != nullptr, "null output");
    out11[0] = c.adv_dye;
    out11[1] = c.adv_vel;
    out11[2] = c.mc_steps;
    out11[3] = c.mcv_steps;
    if (c.st_sl) HIPCHK(hipStreamSynchronize(c.st_sl));
    c.mc_counts(c.mc_cnt, c.mc_nb, out11 + 4);
    c.mc_counts(c.mcv_cnt, c.mcv_nb, out11 + 7);
    out11[10] = (int64_t)c.advection_dev_bytes();
  });
}

int pucfem_sl_advect_mc(void* ctx, int32_t nch, const double* cin, const double* u, double dt, double* cout,
                        int32_t* marks, int32_t* tri) {
  return guard(ctx, [&] {
    advect_fields_unit(*C(ctx), {PUCFEM_ADV_MACCORMACK, PUCFEM_TRJ_EULER}, nch, cin, u, dt, cout, marks, tri);
  });
}

int pucfem_sl_advect_vel_mc(void* ctx, const double* f, const double* u, double dt, double* f_out, int32_t* marks,
                            int32_t* tri) {
  return guard(ctx, [&] {
    advect_pairs_unit(*C(ctx), {PUCFEM_ADV_MACCORMACK, PUCFEM_TRJ_EULER}, f, u, dt, f_out, marks, tri);
  });
}

int pucfem_advection_probe(void* ctx, int32_t what, int32_t nch, int32_t iters, double* out4) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    require(what == PUCFEM_ADV_DYE || what == PUCFEM_ADV_VELOCITY, "what is PUCFEM_ADV_DYE or PUCFEM_ADV_VELOCITY");
    if (what == PUCFEM_ADV_DYE) c.dye_ready();
    else c.inertia_ready();
    require(iters >= 1 && out4 != nullptr, "iters < 1 or null output");
    const i64 N = c.mesh.N;
    const bool dye = what == PUCFEM_ADV_DYE;
    if (dye) require(nch >= 1 && nch <= DYE_MAX, "nch must be in 1 .. PUCFEM_MAX_DYES (16)");
    transport_probe(c, {PUCFEM_ADV_MACCORMACK, PUCFEM_TRJ_EULER}, dye ? nch : 0, iters, out4);
    out4[2] = dye ? c.mc_bytes1(nch, N) : c.mcv_bytes1(N);
    out4[3] = dye ? c.mc_bytes2(nch, N) : c.mcv_bytes2(N);
  });
}

// ---- midpoint trajectories (pucfem_trajectory.hpp)
int pucfem_set_trajectory(void* ctx, int32_t what, int32_t order) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    c.set_trajectory(what, order);
  });
}

int pucfem_trajectory_info(void* ctx, int64_t* out10) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    c.inertia_ready();  // (a single-rank Stokes context on a device, built)
    require(out10 != nullptr, "null output");
    out10[0] = c.trj_dye;
    out10[1] = c.trj_vel;
    out10[2] = c.trj_trc;
    out10[3] = c.trjd_steps;
    out10[4] = c.trjv_steps;
    out10[5] = c.trjt_steps;
    if (c.st_sl) HIPCHK(hipStreamSynchronize(c.st_sl));
    out10[6] = c.trj_mid_rows(c.trjd_mid, c.trjd_nb, c.adv_dye != 0);
    out10[7] = c.trj_mid_rows(c.trjv_mid, c.trjv_nb, c.adv_vel != 0);
    int32_t fell = 0;
    if (c.trjt_fell && c.trjt_ran) c.d2h(&fell, c.trjt_fell, sizeof(int32_t));
    out10[8] = fell;
    out10[9] = (int64_t)c.trajectory_dev_bytes();
  });
}

namespace {
void trj_check(int32_t order, int32_t scheme) {
  require(order == PUCFEM_TRJ_EULER || order == PUCFEM_TRJ_MIDPOINT, "unknown trajectory order");
  require(scheme == PUCFEM_ADV_SL || scheme == PUCFEM_ADV_MACCORMACK, "unknown advection scheme");
}
}  // namespace

int pucfem_sl_advect_traj(void* ctx, int32_t order, int32_t scheme, int32_t nch, const double* cin, const double* u,
                          double dt, double* cout, int32_t* marks, int32_t* tri) {
  return guard(ctx, [&] {
    trj_check(order, scheme);
    advect_fields_unit(*C(ctx), {scheme, order}, nch, cin, u, dt, cout, marks, tri);
  });
}

int pucfem_sl_advect_vel_traj(void* ctx, int32_t order, int32_t scheme, const double* f, const double* u, double dt,
                              double* f_out, int32_t* marks, int32_t* tri) {
  return guard(ctx, [&] {
    trj_check(order, scheme);
    advect_pairs_unit(*C(ctx), {scheme, order}, f, u, dt, f_out, marks, tri);
  });
}

int pucfem_trajectory_probe(void* ctx, int32_t what, int32_t scheme, int32_t nch, int32_t iters, double* out4) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    require(what == PUCFEM_TRJ_DYE || what == PUCFEM_TRJ_VELOCITY, "what is PUCFEM_TRJ_DYE or PUCFEM_TRJ_VELOCITY");
    require(scheme == PUCFEM_ADV_SL || scheme == PUCFEM_ADV_MACCORMACK, "unknown advection scheme");
    if (what == PUCFEM_TRJ_DYE) c.dye_ready();
    else c.inertia_ready();
    require(iters >= 1 && out4 != nullptr, "iters < 1 or null output");
    const i64 N = c.mesh.N;
    const bool dye = what == PUCFEM_TRJ_DYE, mc = scheme == PUCFEM_ADV_MACCORMACK;
    out4[0] = out4[1] = out4[2] = out4[3] = 0.0;
    if (dye) require(nch >= 1 && nch <= DYE_MAX, "nch must be in 1 .. PUCFEM_MAX_DYES (16)");
    transport_probe(c, {scheme, PUCFEM_TRJ_MIDPOINT}, dye ? nch : 0, iters, out4);
    out4[2] = dye ? c.trj_bytes1(nch, N, mc) : c.trjv_bytes1(N, mc);
    if (mc) out4[3] = dye ? c.trj_bytes2(nch, N) : c.trjv_bytes2(N);
  });
}

// ---- measurement
int pucfem_timing_enable(void* ctx, int32_t on) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    c.need_dev();
    HIPCHK(hipStreamSynchronize(c.st));
    c.timer.flush();
    require(on >= 0 && on <= 2, "timing mode");
    c.timer.on = on != 0;
    // mode 2: the kernel classes with a share of the step (the roofline kernel is the largest of them); mode 1
    // adds the finest level's residual and transfers
    c.timer.mask = on == 2 ? ~((1u << 5) | (1u << 6) | (1u << 7)) : ~0u;
    for (int k = 0; k < Timer::NCLS; ++k) {
      c.timer.ms[k] = 0;
      c.timer.bytes[k] = 0;
      c.timer.n[k] = 0;
    }
  });
}

int pucfem_timing_get(void* ctx, int32_t k, double* ms, int64_t* n, double* bytes) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    require(k >= 0 && k < Timer::NCLS, "kernel class");
    if (!c.host_only) {
      HIPCHK(hipStreamSynchronize(c.st));
      c.timer.flush();
    }
    *ms = c.timer.ms[k];
    *n = c.timer.n[k];
    *bytes = c.timer.n[k] ? c.timer.bytes[k] / (double)c.timer.n[k] : 0.0;
  });
}

int pucfem_counters(void* ctx, int64_t* launches, double* bytes) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    *launches = g_nlaunch;
    *bytes = c.algo_bytes;
  });
}

int pucfem_class_counters(void* ctx, int32_t kclass, int64_t* launches, double* bytes) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    require(kclass >= 0 && kclass < Timer::NCLS, "kernel class out of range");
    *launches = c.cls_n[kclass];
    *bytes = c.cls_bytes[kclass];
  });
}

int pucfem_sync(void* ctx) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    if (!c.host_only) {
      HIPCHK(hipStreamSynchronize(c.st));
    }
  });
}

int pucfem_info(void* ctx, int64_t* o) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    c.need_built();
    o[0] = c.mesh.N;
    o[1] = c.mesh.T;
    o[2] = c.P.nnz();
    o[3] = c.Pp.nnz();
    o[4] = c.lp.n_own;
    o[5] = c.lp.n_ghost;
    o[6] = c.sP.padded;
    o[7] = c.sPp.padded;
    o[8] = (int64_t)c.op_pairs.size();
    o[9] = (int64_t)c.dir_nodes.size();
    o[10] = (c.dP.c16 ? 1 : 0) | (c.dPp.c16 ? 2 : 0) | (!c.mg.empty() && c.mg.back().f32.Aval16 ? 4 : 0);
    o[11] = (int64_t)c.mg.size();
  });
}

int pucfem_path_info(void* ctx, int64_t* o) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    c.need_built();
    for (int k = 0; k < 8; ++k) o[k] = 0;
    const bool stokes = c.scheme == PUCFEM_STOKES_COLOR || c.scheme == PUCFEM_STOKES_FOOD;
    if (!stokes) return;
    const bool block = !c.dist() && c.block_cg && c.lp.n_own <= (i64)CGB_THREADS * CGB_MAXR;
    o[0] = c.dense ? 0 : (block ? 1 : 2);
    o[1] = c.dense ? 0 : (c.use_mg ? 3 : (block ? 1 : 2));
    o[2] = c.n_reseed;
    o[3] = c.proj_m[1];
    o[4] = c.proj_m[2];
    o[5] = c.dvinc[0] && !c.proj_k_visc ? std::min(c.have_vinc, c.visc_extrap) : 0;
    o[6] = c.proj_k;
    o[7] = (c.lattice ? 1 : 0) | (c.lat_sl ? 2 : 0) |
           (!c.dense && !block && c.visc_solver == 0 && c.visc_R < 0.25 ? 4 : 0) | (c.visc_check_fail ? 8 : 0) |
           (c.visc_pairs ? 16 : 0) | (c.mg_pairs ? 32 : 0) | (c.p_from_y ? 64 : 0) | (c.cgcg_iters ? 128 : 0);
  });
}

int pucfem_mg_lmax(void* ctx, int32_t level, double* o) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    c.need_built();
    require(c.use_mg && level >= 0 && level <= c.mg_levels, "level of a multigrid hierarchy");
    require(!c.dist(), "a single-rank context (the host estimate iterates the whole level)");
    const MgLevel& L = c.mg[level];
    const Csr& A = level == c.mg_levels ? c.Pp : L.Pp;
    double lam = 0.0;
    o[0] = L.lmax;
    o[1] = L.lam_dev;
    o[3] = lmax_estimate(A, false);
    lmax_estimate(A, true, nullptr, &lam);
    o[2] = lam;
  });
}

int pucfem_proj_info(void* ctx, double* o) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    c.need_built();
    o[0] = (double)c.n_reseed;
    o[1] = (double)c.n_restart;
    o[2] = c.guess_last[1];
    o[3] = c.guess_last[2];
  });
}

int pucfem_visc_interval(void* ctx, double* o) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    c.need_built();
    require(c.scheme == PUCFEM_STOKES_COLOR || c.scheme == PUCFEM_STOKES_FOOD, "a Stokes context");
    o[0] = c.visc_lo;
    o[1] = 1.0 + c.visc_R;
  });
}

int pucfem_comm_info(void* ctx, int64_t* o) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    c.need_built();
    o[0] = c.dist() ? c.dye_halo_values : 0;
    o[1] = c.dist() ? c.mesh.N - c.lp.n_own : 0;
    o[2] = c.dist() ? 3 * (int64_t)c.ntr : 0;
    o[3] = !c.comm ? 0 : (dynamic_cast<NcclComm*>(c.comm.get()) ? 2 : 1);
  });
}

int pucfem_comm_counters(void* ctx, int64_t* o) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    for (int k = 0; k < 6; ++k) o[k] = 0;
    if (!c.comm) return;
    o[0] = c.comm->n_allreduce;
    o[1] = c.comm->v_allreduce;
    o[2] = c.comm->n_msg;
    o[3] = c.comm->b_msg;
    o[4] = c.comm->n_group;
    o[5] = c.comm->n_bcast;
  });
}

// Communicator self-test on the library stream: an all-reduce (sum and max) of 8 values and one grouped
// ring exchange (send to rank + 1, receive from rank - 1; on one rank a send to itself), checked on the
// device values.  out[0] = |sum - expected|, out[1] = |max - expected|, out[2] = |received - expected|,
// out[3] = backend (1 LocalComm, 2 RCCL).
int pucfem_comm_selftest(void* ctx, double* out4) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    c.need_dev();
    require(c.dist(), "comm_selftest needs a context created by pucfem_ctx_create_dist with a communicator");
    const int W = c.world, R = c.rank;
    constexpr int n = 8;
    std::vector<double> h(3 * n);
    for (int k = 0; k < n; ++k) {
      h[k] = (R + 1) * (k + 1.0);      // sum over ranks: (k + 1) W (W + 1) / 2
      h[n + k] = R + 0.25 * k;         // max over ranks: W - 1 + 0.25 k
      h[2 * n + k] = 1000.0 * R + k;   // sent to rank + 1
    }
    double* d = c.dalloc<double>(4 * n);
    HIPCHK(hipMemcpyAsync(d, h.data(), sizeof(double) * 3 * n, hipMemcpyHostToDevice, c.st));
    c.comm->allreduce(d, n, false, c.st);
    c.comm->allreduce(d + n, n, true, c.st);
    c.comm->group_start();
    c.comm->send(d + 2 * n, n, (R + 1) % W, c.st);
    c.comm->recv(d + 3 * n, n, (R + W - 1) % W, c.st);
    c.comm->group_end(c.st);
    std::vector<double> g(4 * n);
    HIPCHK(hipMemcpyAsync(g.data(), d, sizeof(double) * 4 * n, hipMemcpyDeviceToHost, c.st));
    HIPCHK(hipStreamSynchronize(c.st));
    double e0 = 0, e1 = 0, e2 = 0;
    const int from = (R + W - 1) % W;
    for (int k = 0; k < n; ++k) {
      e0 = std::max(e0, std::fabs(g[k] - (k + 1.0) * W * (W + 1) / 2.0));
      e1 = std::max(e1, std::fabs(g[n + k] - (W - 1 + 0.25 * k)));
      e2 = std::max(e2, std::fabs(g[3 * n + k] - (1000.0 * from + k)));
    }
    out4[0] = e0;
    out4[1] = e1;
    out4[2] = e2;
    out4[3] = dynamic_cast<NcclComm*>(c.comm.get()) ? 2 : 1;
  });
}

int pucfem_mg_probe(void* ctx, int32_t piece, int32_t level, const double* b, const double* x, double* out,
                    double* rz) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    c.need_built();
    require(c.use_mg && c.mg.size() >= 2, "mg_probe needs a context built with a multigrid hierarchy");
    if (c.host_only) throw Error(PUCFEM_ESTATE, "mg_probe runs the cycle's kernels: it needs a device context");
    require(!c.dist(), "mg_probe needs a single-rank context");
    const int Lv = (int)c.mg.size() - 1;
    require(piece >= PUCFEM_MG_RESID && piece <= PUCFEM_MG_PRECOND, "piece");
    const bool needs_b = piece != PUCFEM_MG_RESTRICT;
    const bool needs_x = piece == PUCFEM_MG_RESID || piece == PUCFEM_MG_SMOOTHX || piece == PUCFEM_MG_RESTRICT ||
                         piece == PUCFEM_MG_PROLONG;
    require(out != nullptr && (!needs_b || b != nullptr) && (!needs_x || x != nullptr), "null vector");
    if (piece == PUCFEM_MG_COARSE) require(level == 0, "the coarse solve is level 0");
    else if (piece == PUCFEM_MG_PRECOND) require(level == Lv && rz != nullptr, "precondition is the finest level, with rz");
    else if (piece == PUCFEM_MG_CYCLE) require(level >= 0 && level <= Lv, "level");
    else require(level >= 1 && level <= Lv, "level (this piece exists on levels >= 1)");
    if (c.mg_single) mg_probe_run<float>(c, piece, level, b, x, out, rz);
    else mg_probe_run<double>(c, piece, level, b, x, out, rz);
  });
}

int pucfem_cgcg_coef_probe(void* ctx, const double* red8, double bb, const double* sc5, double tol2, int32_t it,
                           int32_t maxit, double rho0, int32_t* ctl_out, double* sc_out5) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    c.need_dev();
    std::vector<double> h(24, 0.0);
    for (int k = 0; k < 8; ++k) h[k] = red8[k];
    h[8] = bb;
    h[9] = rho0;
    for (int k = 0; k < 5; ++k) h[16 + k] = sc5[k];
    DevTmp<double> d(h, c.st);
    DevTmp<int> ctl(std::vector<int>{0, 0}, c.st);
    hipLaunchKernelGGL(k_cgcg_coef, dim3(1), dim3(64), 0, c.st, (const double*)d.p, (const double*)(d.p + 8), d.p + 16,
                       tol2, ctl.p, (int)it, (int)maxit, (const double*)(d.p + 9));
    KCHK();
    std::vector<int> hc;
    std::vector<double> out;
    ctl.get(hc, 2, c.st);
    d.get(out, 24, c.st);
    HIPCHK(hipStreamSynchronize(c.st));
    ctl_out[0] = hc[0];
    ctl_out[1] = hc[1];
    for (int k = 0; k < 5; ++k) sc_out5[k] = out[16 + k];
  });
}

// ---- host-only
int pucfem_refine(int64_t N, const double* xy, const int32_t* mk, int64_t T, const int32_t* tris, int32_t levels,
                  int64_t* N_out, int64_t* T_out, double* xy_out, int32_t* mk_out, int32_t* tris_out) {
  return guard(nullptr, [&] {
    require(levels >= 0 && levels <= 12, "levels in [0, 12]");
    if (!xy_out) {  // sizes only: N' = N + E, T' = 4T, E = (3T + Eb) / 2 with Eb doubling per level
      std::vector<std::pair<i32, i32>> es(3 * (size_t)T);
      for (i64 t = 0; t < T; ++t)
        for (int e = 0; e < 3; ++e) {
          const i32 a = tris[3 * t + e], b = tris[3 * t + (e + 1) % 3];
          es[3 * t + e] = {std::min(a, b), std::max(a, b)};
        }
      std::sort(es.begin(), es.end());
      i64 Eb = 0;
      for (size_t i = 0; i < es.size();) {
        size_t j = i;
        while (j < es.size() && es[j] == es[i]) ++j;
        if (j - i == 1) ++Eb;
        i = j;
      }
      i64 n = N, t = T;
      for (int l = 0; l < levels; ++l) {
        n += (3 * t + Eb) / 2;
        t *= 4;
        Eb *= 2;
      }
      *N_out = n;
      *T_out = t;
      return;
    }
    HostMesh a;
    a.N = N;
    a.T = T;
    a.x.resize(N);
    a.y.resize(N);
    for (i64 i = 0; i < N; ++i) {
      a.x[i] = xy[2 * i];
      a.y[i] = xy[2 * i + 1];
    }
    a.mk.assign(mk, mk + N);
    a.tri.assign(tris, tris + 3 * T);
    for (int l = 0; l < levels; ++l) {
      HostMesh b;
      red_refine(a, b);
      a = std::move(b);
    }
    *N_out = a.N;
    *T_out = a.T;
    if (xy_out) {
      for (i64 i = 0; i < a.N; ++i) {
        xy_out[2 * i] = a.x[i];
        xy_out[2 * i + 1] = a.y[i];
      }
      std::copy(a.mk.begin(), a.mk.end(), mk_out);
      std::copy(a.tri.begin(), a.tri.end(), tris_out);
    }
  });
}

int pucfem_host_get_csr(void* ctx, int32_t op, int64_t* n_rows, int64_t* nnz, int64_t* rowptr, int64_t* col,
                        double* val) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    c.need_built();
    const Csr* A = nullptr;
    const std::vector<double>* v = nullptr;
    if (op >= 100) {  // multigrid level matrices (CPU tests): 100 + 3 l + {0: Pp_l, 1: Pr_l, 2: R_l}
      const int l = (op - 100) / 3, kind = (op - 100) % 3;
      require(c.use_mg && l >= 0 && l <= c.mg_levels, "no such multigrid level");
      const int Lv = c.mg_levels;
      const MgLevel& L = c.mg[l];
      require(kind == 0 || l >= 1, "level 0 has no transfer operators");
      const Csr& M = kind == 0 ? (l == Lv ? c.Pp : L.Pp) : kind == 1 ? L.Pr : L.R;
      const Ordering& ro = kind == 2 ? c.mg[l - 1].ord : L.ord;
      const Ordering& co = kind == 1 ? c.mg[l - 1].ord : L.ord;
      *n_rows = M.nrows;
      *nnz = M.nnz();
      if (!col) return;
      i64 k = 0;
      rowptr[0] = 0;
      std::vector<std::pair<i64, double>> tmp;
      for (i64 o = 0; o < M.nrows; ++o) {
        const i64 g = ro.old2new[o];
        tmp.clear();
        for (i64 e = M.rowptr[g]; e < M.rowptr[g + 1]; ++e) tmp.push_back({co.new2old[M.col[e]], M.val[e]});
        std::sort(tmp.begin(), tmp.end());
        for (auto& t : tmp) {
          col[k] = t.first;
          val[k] = t.second;
          ++k;
        }
        rowptr[o + 1] = k;
      }
      return;
    }
    if (op == PUCFEM_OP_MLUMP || op == PUCFEM_OP_ASUM) {  // diagonals, owned rows in caller numbering
      const std::vector<double>& d = op == PUCFEM_OP_MLUMP ? c.as.M : c.as.asum;
      require(!d.empty(), "operator not built for this scheme");
      std::vector<i64> rows;
      for (i64 g = c.lp.r0; g < c.lp.r1; ++g) rows.push_back(c.ord.new2old[g]);
      std::sort(rows.begin(), rows.end());
      *n_rows = (i64)rows.size();
      *nnz = (i64)rows.size();
      if (!col) return;
      rowptr[0] = 0;
      for (size_t r = 0; r < rows.size(); ++r) {
        col[r] = rows[r];
        val[r] = d[c.ord.old2new[rows[r]]];
        rowptr[r + 1] = (i64)r + 1;
      }
      return;
    }
    switch (op) {
      case PUCFEM_OP_K: A = &c.P; v = &c.as.K; break;
      case PUCFEM_OP_MCONS:
        require(c.dye_impl, "the consistent mass exists on dye_scheme = 1 contexts");
        A = &c.P;
        v = &c.dyeop.mc;
        break;
      case PUCFEM_OP_GX: A = &c.P; v = &c.as.Gx; break;
      case PUCFEM_OP_GY: A = &c.P; v = &c.as.Gy; break;
      case PUCFEM_OP_VISC: A = &c.P; v = &c.Kv; break;
      case PUCFEM_OP_PRES: A = &c.Pp; v = &c.Pp.val; break;
      case PUCFEM_OP_LIT: A = &c.Lit; v = &c.Lit.val; break;
      default: throw Error(PUCFEM_EINVAL, "op has no CSR");
    }
    require(A->nrows > 0, "operator not built for this scheme");
    const LocalPlan& lp = c.lp;
    // owned rows in caller numbering, ascending
    std::vector<i64> rows;
    for (i64 g = lp.r0; g < lp.r1; ++g) rows.push_back(c.ord.new2old[g]);
    std::sort(rows.begin(), rows.end());
    i64 total = 0;
    for (i64 o : rows) {
      const i64 g = c.ord.old2new[o];
      total += A->rowptr[g + 1] - A->rowptr[g];
    }
    *n_rows = (i64)rows.size();
    *nnz = total;
    if (!col) return;
    i64 k = 0;
    rowptr[0] = 0;
    std::vector<std::pair<i64, double>> tmp;
    for (size_t r = 0; r < rows.size(); ++r) {
      const i64 g = c.ord.old2new[rows[r]];
      tmp.clear();
      for (i64 e = A->rowptr[g]; e < A->rowptr[g + 1]; ++e) tmp.push_back({c.ord.new2old[A->col[e]], (*v)[e]});
      std::sort(tmp.begin(), tmp.end());
      for (auto& t : tmp) {
        col[k] = t.first;
        val[k] = t.second;
        ++k;
      }
      rowptr[r + 1] = k;
    }
  });
}

int pucfem_host_lattice_apply(void* ctx, int32_t level, int32_t kind, const double* x, double* y) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    c.need_built();
    require(c.lattice && !c.dist(), "needs a single-rank context with lattice operators");
    const int Lv = c.mg_levels;
    require(level >= 0 && level <= Lv, "level out of range");
    require(kind >= 0 && kind <= 6 && kind != 4, "kind");
    require(kind >= 3 || level == Lv, "kinds 0-2 are finest-level operators");
    require(kind < 5 || level >= 1, "transfers need level >= 1");
    MgLevel& L = c.mg[level];
    const int in_l = kind == 5 ? level - 1 : level, out_l = kind == 6 ? level - 1 : level;
    const Ordering& oin = c.mg[in_l].ord;
    const Ordering& oout = c.mg[out_l].ord;
    const i64 nin = (i64)oin.new2old.size(), nout = (i64)oout.new2old.size();
    const int ncomp = kind == 1 ? 2 : 1;
    std::vector<double> x0(nin), x1(ncomp > 1 ? nin : 0), yv(nout, NAN);
    for (i64 g = 0; g < nin; ++g) {
      const i64 o = oin.new2old[g];
      x0[g] = x[ncomp * o];
      if (ncomp > 1) x1[g] = x[ncomp * o + 1];
    }
    const int n = 1 << level;
    std::vector<double> wsk;
    if (kind == 2) {
      std::vector<uint8_t> isdir(c.mesh.N, 0);
      for (i32 d : c.dir_nodes) isdir[c.ord.old2new[d]] = 1;
      wsk.resize(c.mesh.N);
      for (i64 g = 0; g < c.mesh.N; ++g) wsk[g] = isdir[g] ? 0.0 : 1.0 / std::sqrt(diag_of(c.P, c.Kv, g));
    }
    if (kind <= 2) {
      lattice_apply_host(kind, n, L.lf_plain, L.lf_coef, x0.data(), ncomp > 1 ? x1.data() : nullptr,
                         kind == 2 ? wsk.data() : nullptr, yv.data());
    } else if (kind == 3) {
      lattice_apply_host(0, n, L.lf_merged, L.lf_coef, x0.data(), nullptr, nullptr, yv.data());
    } else if (kind == 5) {
      lattice_apply_host(3, n, L.lf_plain, L.lf_coef, x0.data(), nullptr, nullptr, yv.data(), &L.pr_tab2, n / 2);
    } else {
      lattice_apply_host(4, n / 2, L.r_tab, L.lf_coef, x0.data(), nullptr, nullptr, yv.data(), &L.r_tab2, n);
    }
    for (i64 g = 0; g < nout; ++g) y[oout.new2old[g]] = yv[g];
  });
}

int pucfem_host_partition(void* ctx, int32_t rank, int32_t world, int64_t* n_own, int64_t* n_ghost, int64_t* owned,
                          int64_t* ghosts, int32_t* ghost_owner, int64_t* n_send, int64_t* send_ids,
                          int32_t* send_peer) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    c.need_built();
    require(rank >= 0 && rank < world, "bad rank");
    std::vector<i64> rs;
    partition_rows(c.P, c.ord, world, rs);
    LocalPlan lp;
    std::vector<const Csr*> pats = {&c.P};
    if (c.Pp.nrows) pats.push_back(&c.Pp);
    // PUCFEM_HOST_PLAN_DEEP=1 (test knob): the deep-halo plan of the W > 1 multigrid runs (make_local_plan2 with the
    // patterns' ghost rows one layer out and their columns), as Ctx builds it for the finest level
    const char* deep_env = std::getenv("PUCFEM_HOST_PLAN_DEEP");
    if (deep_env && std::atoi(deep_env) != 0) {
      std::vector<PatRows> pr;
      for (const Csr* A : pats) pr.push_back({A, &rs});
      make_local_plan2(pr, rs, rank, lp, &pats);
    } else {
      make_local_plan(pats, rs, rank, lp);
    }
    *n_own = lp.n_own;
    *n_ghost = lp.n_ghost;
    *n_send = (i64)lp.send_local.size();
    if (!owned) return;
    for (i64 i = 0; i < lp.n_own; ++i) owned[i] = c.ord.new2old[lp.r0 + i];
    for (i64 k = 0; k < lp.n_ghost; ++k) {
      ghosts[k] = c.ord.new2old[lp.ghost_global[k]];
      ghost_owner[k] = lp.ghost_owner[k];
    }
    for (size_t q = 0; q < lp.send_peer.size(); ++q)
      for (i64 k = 0; k < lp.send_cnt[q]; ++k) {
        const i64 idx = lp.send_off[q] + k;
        send_ids[idx] = c.ord.new2old[lp.r0 + lp.send_local[idx]];
        send_peer[idx] = lp.send_peer[q];
      }
  });
}


// ---- kernel micro-benchmark (tools/spmv_variants.py): k_cg_dir variants on the pressure operator
int pucfem_bench_dir(void* ctx, int32_t variant, int32_t nblocks, int32_t iters, double* ms_out) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    c.need_dev();
    c.need_built();
    require(c.dKp && !c.lattice, "needs a Stokes context with SELL operators");
    const DevSell& A = c.dPp;
    const int nb = nblocks > 0 ? std::min(nblocks, MAXB) : Ctx::nb_for(A.nslices);
    CgVecs<1> v;
    v.y[0] = c.yp;
    v.b[0] = c.bh;
    v.r[0] = c.cg_r[0];
    v.po[0] = c.cg_pa[0];
    v.pn[0] = c.cg_pb[0];
    v.q[0] = c.cg_q[0];
    std::vector<double> ones(c.nloc, 1.0);
    HIPCHK(hipMemcpyAsync(c.cg_r[0], ones.data(), sizeof(double) * c.nloc, hipMemcpyHostToDevice, c.st));
    HIPCHK(hipMemcpyAsync(c.cg_pa[0], ones.data(), sizeof(double) * c.nloc, hipMemcpyHostToDevice, c.st));
    const double sc[16] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1};
    HIPCHK(hipMemcpyAsync(c.scal, sc, sizeof(sc), hipMemcpyHostToDevice, c.st));
    HIPCHK(hipMemcpyAsync(c.part_a, sc, sizeof(double), hipMemcpyHostToDevice, c.st));
    HIPCHK(hipMemsetAsync(c.ctl, 0, 2 * sizeof(int), c.st));
    auto launch = [&]() {
      switch (variant) {
        case 0: hipLaunchKernelGGL((k_cg_dir<1, 0, false, false>), dim3(nb), dim3(BS), 0, c.st, A.view(), FaceDev{}, c.dKp, v, (int64_t)0, c.part_a, 1, 1, c.part_a, 1, 1, c.scal, c.ctl, 1, 1 << 30, 0.0, c.part_c); break;
        case 1: hipLaunchKernelGGL((k_cg_dir<1, 8, false, false>), dim3(nb), dim3(BS), 0, c.st, A.view(), FaceDev{}, c.dKp, v, (int64_t)0, c.part_a, 1, 1, c.part_a, 1, 1, c.scal, c.ctl, 1, 1 << 30, 0.0, c.part_c); break;
        case 2: hipLaunchKernelGGL((k_cg_dir<1, 0, true, false>), dim3(nb), dim3(BS), 0, c.st, A.view(), FaceDev{}, c.dKp, v, (int64_t)0, c.part_a, 1, 1, c.part_a, 1, 1, c.scal, c.ctl, 1, 1 << 30, 0.0, c.part_c); break;
        case 3: hipLaunchKernelGGL((k_cg_dir<1, 8, true, false>), dim3(nb), dim3(BS), 0, c.st, A.view(), FaceDev{}, c.dKp, v, (int64_t)0, c.part_a, 1, 1, c.part_a, 1, 1, c.scal, c.ctl, 1, 1 << 30, 0.0, c.part_c); break;
        default: require(A.c16 != nullptr, "variant 4 needs int16 columns");
                 hipLaunchKernelGGL((k_cg_dir<1, 8, true, true>), dim3(nb), dim3(BS), 0, c.st, A.view(), FaceDev{}, c.dKp, v, (int64_t)0, c.part_a, 1, 1, c.part_a, 1, 1, c.scal, c.ctl, 1, 1 << 30, 0.0, c.part_c); break;
      }
      KCHK();
    };
    launch();
    *ms_out = time_launches(c, iters, launch);
  });
}

int pucfem_bench_kernel(void* ctx, int32_t kernel, int32_t iters, double* ms_batch, double* ms_each, double* bytes) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    c.need_dev();
    c.need_built();
    require(c.use_mg && c.mg_single && iters > 0, "bench_kernel needs a multigrid context with the fp32 V-cycle");
    MgLevel& L = c.mg.back();
    MgBufs<float>& B = L.f32;
    const DevSell& A = c.dPp;
    // kernel / 16 = untimed launches of a coarse level's smoother between the timed launches (how the
    // per-launch events behave when other kernels run in between, as inside a step)
    // kernel / 256 = 1: the host waits for every launch before it submits the next (the GPU is idle
    // when each launch's packet arrives)
    const bool idle = (kernel / 256) & 1;
    kernel %= 256;
    const int nfill = kernel / 16;
    kernel %= 16;
    const FaceDev ff = c.fP.full(), fpt = c.fP.part();
    const int nb_mg = c.grid_full(ff, A), nb = Ctx::grid_part(fpt, A);
    CgVecs<1> v;
    v.y[0] = c.yp;
    v.b[0] = c.bh;
    v.r[0] = c.z;
    v.po[0] = c.cg_pa[0];
    v.pn[0] = c.cg_pb[0];
    v.q[0] = c.cg_q[0];
    double by = 0.0;
    // scalar state of k_cg_dir: beta = 1, never converged
    const double sc[16] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1};
    double* one = c.redbuf + 8 * 60;
    HIPCHK(hipMemcpyAsync(c.scal, sc, sizeof(sc), hipMemcpyHostToDevice, c.st));
    HIPCHK(hipMemcpyAsync(one, sc, sizeof(double), hipMemcpyHostToDevice, c.st));
    int* ctl0 = reinterpret_cast<int*>(c.redbuf + 8 * 61);
    HIPCHK(hipMemsetAsync(ctl0, 0, 4 * sizeof(int), c.st));
    auto launch = [&](hipEvent_t a, hipEvent_t e) {
      with_c16(A, [&](auto c16) {
        constexpr bool C16 = decltype(c16)::value;
        SellDev none = A.view();
        none.nslices = 0;
        switch (kernel) {
          case 3:  // the face part alone
            hipExtLaunchKernelGGL(k_cheb<float, float, float, float, C16, 2>, dim3(ff.nb + 8), dim3(BS), 0, c.st, a, e, 0,
                                  none, ff, (const float*)B.Aval, (const float*)B.dinv, (const float*)c.r32,
                                  (const float*)B.x, B.x2, B.d, 0.3, 0.7, 0.0, 1, (const int*)nullptr,
                                  (const double*)nullptr, (double*)nullptr, RedOut{},
                                  (float*)nullptr);
            break;
          case 4:  // the SELL (skeleton) part alone
            hipExtLaunchKernelGGL(k_cheb<float, float, float, float, C16, 2>, dim3(c.nb_mg(A.nslices)), dim3(BS), 0, c.st,
                                  a, e, 0, A.view(), FaceDev{}, (const float*)B.Aval, (const float*)B.dinv,
                                  (const float*)c.r32, (const float*)B.x, B.x2, B.d, 0.3, 0.7, 0.0, 1,
                                  (const int*)nullptr, (const double*)nullptr, (double*)nullptr, RedOut{},
                                  (float*)nullptr);
            break;
          case 5:  // k_cg_dir, the face part alone
            hipExtLaunchKernelGGL(k_cg_dir<1, 8, true, C16>, dim3(fpt.nb + 8), dim3(BS), 0, c.st, a, e, 0, none, fpt,
                                  (const double*)c.dKp_raw, v, c.lp.n_ghost, (const double*)one, 1, 1,
                                  (const double*)one, 1, 1, c.scal, ctl0, 1, 1 << 30, 0.0, c.part_c,
                                  (const double*)nullptr, 0, 0, RedOut{});
            break;
          case 6:  // k_cg_dir, the SELL (skeleton) part alone
            hipExtLaunchKernelGGL(k_cg_dir<1, 8, true, C16>, dim3(Ctx::nb_for(A.nslices)), dim3(BS), 0, c.st, a, e, 0,
                                  A.view(), FaceDev{}, (const double*)c.dKp_raw, v, c.lp.n_ghost, (const double*)one,
                                  1, 1, (const double*)one, 1, 1, c.scal, ctl0, 1, 1 << 30, 0.0, c.part_c,
                                  (const double*)nullptr, 0, 0, RedOut{});
            break;
          case 0:
            hipExtLaunchKernelGGL(k_cheb<float, float, float, float, C16, 2>, dim3(nb_mg), dim3(BS), 0, c.st, a, e, 0,
                                  A.view(), ff, (const float*)B.Aval, (const float*)B.dinv, (const float*)c.r32,
                                  (const float*)B.x, B.x2, B.d, 0.3, 0.7, 0.0, 1, (const int*)nullptr,
                                  (const double*)nullptr, (double*)nullptr, RedOut{},
                                  (float*)nullptr);
            break;
          case 1:
            hipExtLaunchKernelGGL(k_resid<float, float, float, C16, 2>, dim3(nb_mg), dim3(BS), 0, c.st, a, e, 0, A.view(),
                                  ff, (const float*)B.Aval, (const float*)c.r32, (const float*)B.x, B.res,
                                  (const int*)nullptr);
            break;
          case 12:  // k_cheb_pair<1> (two smoothing steps on the face rows, general start)
          case 13:  // k_cheb_pair<2> (the fused first two steps from x = 0, then the third)
            if (c.mgp_x && c.fP.items > 0) {
              const HFace& hf = c.fP;
              MgPairVecs pv{(const float*)c.r32, (const float*)B.dinv, (const float*)B.x, B.x2, c.mgp_x,
                            (const float*)B.d, c.mgp_d};
              if (kernel == 12)
                hipExtLaunchKernelGGL(k_cheb_pair<1>, dim3(hf.items), dim3(BS), 0, c.st, a, e, 0, hf.full(), pv, 0.3f,
                                      0.7f, 0.0f, 0.3f, 0.7f, (const int*)nullptr);
              else
                hipExtLaunchKernelGGL(k_cheb_pair<2>, dim3(hf.items), dim3(BS), 0, c.st, a, e, 0, hf.full(), pv, 0.3f,
                                      0.7f, 0.5f, 0.3f, 0.7f, (const int*)nullptr);
            }
            break;
          case 15:  // k_reseed: the pressure basis (all proj_k vectors) into PROJ_KEEP_MAX new ones (scratch target)
            if (c.proj_k > 0 && c.dqm) {
              const i64 n = c.lp.n_own;
              hipExtLaunchKernelGGL(k_reseed, dim3(Ctx::grid_ew(n)), dim3(BS), 0, c.st, a, e, 0, (int64_t)n,
                                    (const ProjT*)c.projX[1], (int64_t)c.pld(1), c.proj_k, (const double*)c.dqm,
                                    (int)PROJ_KEEP_MAX, c.projXalt[1]);
            }
            break;
          case 14:  // k_vcheb_pair (two viscous Chebyshev steps on the face rows, general start)
            if (c.vx2[2] && c.fVisc.items > 0) {
              VPairVecs p{};
              p.xa = c.vx2[0];
              p.xb = c.vx2[1];
              p.xc = c.vx2[2];
              p.b = c.vb2;
              p.da = c.vd2[0];
              p.dc = c.vd2[1];
              hipExtLaunchKernelGGL(k_vcheb_pair, dim3(c.fVisc.items), dim3(BS), 0, c.st, a, e, 0, c.fVisc.part(), p,
                                    0.3, 0.7, 0.3, 0.7, (const int*)ctl0, (double*)nullptr, 0, 0, (double*)nullptr,
                                    (double*)nullptr);
            }
            break;
          case 7:   // k_div as in the step (interleaved u, the pressure rhs, partials)
          case 8:   // its face part alone
          case 9:   // its SELL (skeleton) part alone
          case 10:  // k_div on interleaved (x, y) pairs
          case 11:  // the same, face part alone
            with_c16(c.dP, [&](auto d16) {
              constexpr bool D16 = decltype(d16)::value;
              const FaceDev fd = c.fK.part();
              SellDev dv = c.dP.view();
              if (kernel == 8 || kernel == 11) dv.nslices = 0;
              const int g = kernel == 8 || kernel == 11 ? fd.nb + 8 : kernel == 9 ? c.div_grid() - fd.nb : c.div_grid();
              const FaceDev fk = kernel == 9 ? FaceDev{} : fd;
              const bool aos = true;  // (the step's u is interleaved: 7-9 on u itself, 10-11 on a viscous buffer)
              const double* xa = kernel >= 10 ? reinterpret_cast<const double*>(c.vx2[0]) : (const double*)c.ux;
              if (aos)
                hipExtLaunchKernelGGL(k_div<D16, true>, dim3(g), dim3(BS), 0, c.st, a, e, 0, dv, fk, (const double*)c.dGx,
                                      (const double*)c.dGy, xa, (const double*)nullptr, (const double*)c.das1,
                                      (double*)nullptr, (const double*)c.dmp, -1.0, c.braw, c.part_d, RedOut{});
              else
                hipExtLaunchKernelGGL(k_div<D16, false>, dim3(g), dim3(BS), 0, c.st, a, e, 0, dv, fk,
                                      (const double*)c.dGx, (const double*)c.dGy, xa, (const double*)c.uy,
                                      (const double*)c.das1, (double*)nullptr, (const double*)c.dmp, -1.0, c.braw,
                                      c.part_d, RedOut{});
            });
            break;
          default:
            hipExtLaunchKernelGGL(k_cg_dir<1, 8, true, C16>, dim3(nb), dim3(BS), 0, c.st, a, e, 0, A.view(), fpt,
                                  (const double*)c.dKp_raw, v, c.lp.n_ghost, (const double*)one, 1, 1,
                                  (const double*)one, 1, 1, c.scal, ctl0, 1, 1 << 30, 0.0, c.part_c,
                                  (const double*)nullptr, 0, 0, RedOut{});
        }
      });
      KCHK();
    };
    // face rows read no matrix (and the smoother no dinv: 24 B instead of 28)
    const double fr = (double)c.fP.rows, sk = (double)A.nrows, rb = A.row_bytes();
    switch (kernel) {
      case 0: by = (4.0 + A.idx_bytes()) * (double)A.nnz + (28.0 + rb) * sk + 24.0 * fr; break;
      case 3: by = 24.0 * fr; break;
      case 4: by = (4.0 + A.idx_bytes()) * (double)A.nnz + (28.0 + rb) * sk; break;
      case 5: by = 32.0 * fr; break;
      case 6: by = (8.0 + A.idx_bytes()) * (double)A.nnz + (32.0 + rb) * sk; break;
      case 1: by = (4.0 + A.idx_bytes()) * (double)A.nnz + (12.0 + rb) * sk + 12.0 * fr; break;
      case 7:
      case 10:
        by = (16.0 + c.dP.idx_bytes()) * (double)c.dP.nnz + c.dP.row_bytes() * (double)c.dP.nrows + 24.0 * (double)c.lp.n_own;
        break;
      case 8:
      case 11: by = 24.0 * (double)c.fK.rows; break;
      case 12: by = 20.0 * (double)c.fP.rows; break;  // x_a, d_a, b read; x_{a+2}, d_{a+2} written (fp32)
      case 13: by = 12.0 * (double)c.fP.rows; break;  // b read; x_{a+2}, d_{a+2} written
      case 14: by = 64.0 * (double)c.fVisc.rows; break;  // x_a, b, d_a read; x_{a+2}, d_{a+2} written
      case 15: by = 4.0 * (c.proj_k + PROJ_KEEP_MAX) * (double)c.lp.n_own; break;  // the basis read, the new one written
      case 9: by = (16.0 + c.dP.idx_bytes()) * (double)c.dP.nnz + (c.dP.row_bytes() + 24.0) * (double)c.dP.nrows; break;
      default: by = (8.0 + A.idx_bytes()) * (double)A.nnz + (32.0 + rb) * sk + 32.0 * fr;
    }
    MgLevel& Lc = c.mg[c.mg.size() >= 3 ? c.mg.size() - 3 : 0];
    auto fill = [&] {
      for (int f = 0; f < nfill; ++f) {
        with_c16(Lc.dA, [&](auto c16) {
          constexpr bool C16 = decltype(c16)::value;
          hipLaunchKernelGGL((k_cheb<float, float, float, float, C16, 0>), dim3(c.grid_full(Lc.hA.full(), Lc.dA)), dim3(BS),
                             0, c.st, Lc.dA.view(), Lc.hA.full(), (const float*)Lc.f32.Aval, (const float*)Lc.f32.dinv,
                             (const float*)Lc.f32.b, (const float*)nullptr, Lc.f32.x2, Lc.f32.d, 0.3, 0.7, 0.0, 2,
                             (const int*)nullptr, (const double*)nullptr, (double*)nullptr, RedOut{});
        });
        KCHK();
      }
    };
    launch(nullptr, nullptr);
    *ms_batch = time_launches(c, iters, [&] {
      launch(nullptr, nullptr);
      fill();
    });
    float ms = 0;
    std::vector<hipEvent_t> ev(2 * (size_t)iters);
    for (auto& x : ev) HIPCHK(hipEventCreate(&x));
    for (int k = 0; k < iters; ++k) {
      launch(ev[2 * k], ev[2 * k + 1]);
      fill();
      if (idle) HIPCHK(hipStreamSynchronize(c.st));
    }
    HIPCHK(hipEventSynchronize(ev.back()));
    double tot = 0.0;
    for (int k = 0; k < iters; ++k) {
      HIPCHK(hipEventElapsedTime(&ms, ev[2 * k], ev[2 * k + 1]));
      tot += ms;
    }
    *ms_each = tot / iters;
    for (auto& x : ev) (void)hipEventDestroy(x);
    *bytes = by;
  });
}

// the pressure projection's two basis passes outside the step (tools/proj_bench.py): k_mdot2 and k_pcomb at the
// first pressure solve's current basis size, in the step's form (a pending direction with an accumulated v, the
// right-hand side formed in the multi-dot pass).  Outputs go to scratch (a CG work vector, the re-seed target, the
// k_reduce-layout partials), so the context's state stays as it was
int pucfem_proj_probe(void* ctx, int32_t iters, double* out6) {
  return guard(ctx, [&] {
    Ctx& c = *C(ctx);
    c.need_dev();
    c.need_built();
    require(c.use_mg && c.proj_k > 0 && c.projX[1] && c.pv[1] && c.braw && iters > 0,
            "proj_probe needs a multigrid context with a pressure projection basis");
    const i64 n = c.lp.n_own;
    const int m = c.proj_m[1], mp = std::min(m, c.proj_k - 1);
    const int nb = Ctx::grid_ew(n);
    double* tmp = c.cg_q[0];
    const PendDir pd{nullptr, (const double*)c.proj_x0[1], (const double*)c.cg_r[0], (const double*)c.pv[1]};
    const RhsIn rin{c.braw, c.dslave_of, c.redbuf + 24, 1.0 / (double)c.n_free, tmp};
    double ms[2];
    time_passes(c, iters, 2, ms, [&](int mask) {
      if (mask & 1)
        hipLaunchKernelGGL(mdot2_kernel(m), dim3(nb), dim3(BS), 0, c.st, (int64_t)n, (const ProjT*)c.projX[1],
                           (int64_t)c.pld(1), (const double*)c.bh, (const double*)c.pav[1], (const double*)c.pv[1],
                           (const int32_t*)c.dmaster_of, c.proj_part, RedOut{}, pd, rin);
      if (mask & 2)
        hipLaunchKernelGGL(pcomb_kernel(mp), dim3(nb), dim3(BS), 0, c.st, (int64_t)n, (const ProjT*)c.projX[1],
                           (int64_t)c.pld(1), (const double*)c.proj_coef, (const double*)c.pv[1],
                           (const int32_t*)c.dmaster_of, c.projXalt[1] + c.pcol(1, mp), tmp, (double*)nullptr,
                           (const double*)nullptr, (double*)nullptr);
      KCHK();
    });
    out6[0] = ms[0];
    out6[1] = ms[1];
    out6[2] = (4.0 * m + 44.0) * (double)n;   // X, braw, slave_of, master_of, r0, r_final, v read; b written
    out6[3] = (4.0 * mp + 24.0) * (double)n;  // X, v, master_of read; the new direction and the guess written
    out6[4] = m;
    out6[5] = mp;
  });
}

}  // extern "C"
