/*
 * pucfem.h -- C ABI of libpucfem.so, the MI355X (gfx950) hot path of the
 * PUC-Fluidsimulation-Project Stokes/squirmer time-stepping core.
 *
 * The reference (TobiasHoffmannP/PUC-Fluidsimulation-Project, pure Python/NumPy)
 * has no FFI layer: its de-facto interface is a set of module-level functions plus
 * the np.linalg.solve call sites.  Each entry point below names the
 * reference code it replaces (file:line into /root/reference).  The Python host
 * (puc-fluidsimulation-project_amd/_lib.py) binds these with ctypes; INTEGRATION.md
 * shows the binding.
 *
 * Conventions
 *   - Every function returns int: 0 = ok, < 0 = error (PUCFEM_E*); the message is in
 *     pucfem_last_error(ctx) (or pucfem_last_error(NULL) for context-free calls).
 *   - Plain pointers and sizes only.  The library COPIES every input buffer; the caller
 *     keeps ownership.  Output buffers are caller-allocated.
 *   - Node / triangle numbering at the ABI is always the CALLER's (reference) numbering,
 *     0-based.  The library renumbers internally for locality and partitioning.
 *   - A context is bound to one HIP device (or none: device = PUCFEM_HOST_ONLY builds the
 *     host-side operators only, for CPU tests) and is NOT thread-safe.  Calls are
 *     synchronous at the ABI level; device streams are internal.
 *   - fp64 throughout, except the fp32-coordinate assembly of poisson.py / heatEq.py
 *     (poisson.py:40, :100-146), reproduced bit-for-bit on the host.
 */
#ifndef PUCFEM_H
#define PUCFEM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PUCFEM_ABI_VERSION 1
#define PUCFEM_HOST_ONLY (-1)
#define PUCFEM_UNIQUE_ID_BYTES 128

enum pucfem_status {
  PUCFEM_OK = 0,
  PUCFEM_EINVAL = -1,   /* bad argument / shape */
  PUCFEM_EHIP = -2,     /* HIP runtime error (no device, launch failure, ...) */
  PUCFEM_ENOCONV = -3,  /* iterative solver hit maxit without reaching rtol */
  PUCFEM_ESTATE = -4,   /* call out of order (e.g. step before build) */
  PUCFEM_ENCCL = -5,    /* RCCL error */
  PUCFEM_ENOMEM = -6,
  PUCFEM_ENODEV = -7    /* compute call on a host-only context */
};

/* which reference script's step loop the context runs */
enum pucfem_scheme {
  PUCFEM_STOKES_COLOR = 0, /* StokesColor.py:537-586  (Stokes + semi-Lagrangian dye) */
  PUCFEM_STOKES_FOOD = 1,  /* StokesFood.py:441-505   (Stokes + tracer capture)     */
  PUCFEM_HEAT = 2,         /* heatEq.py:304-325       (backward-Euler diffusion)    */
  PUCFEM_POISSON = 3       /* poisson.py:218-285      (steady Poisson)              */
};

typedef struct pucfem_params {
  int32_t scheme;      /* enum pucfem_scheme */
  int32_t nstrips;     /* y-strips of the node ordering / partition; 0 = auto */
  double dt;           /* DT  (StokesColor.py:43, StokesFood.py:42, heatEq.py:304) */
  double nu;           /* v   (kinematic viscosity, StokesColor.py:39) */
  double rtol_visc;    /* CG rtol, viscous solve  (replaces LU at StokesColor.py:544-545) */
  double rtol_pres;    /* CG rtol, pressure solve (replaces LU at StokesColor.py:555,569) */
  double rtol_lin;     /* BiCGStab rtol, heat / Poisson literal operators */
  int32_t maxit_visc, maxit_pres, maxit_lin;
  int32_t warm_start;  /* 1: start each solve from the previous step's solution */
  int32_t sl_k;        /* PointLocator k (StokesColor.py:324), 10 */
  double capture_radius; /* StokesFood.py:50-51, 0.28 */
  double center_x, center_y; /* squirmer centre (0.5, 0.5) */
  int32_t precond;     /* pressure solve: 0 = Jacobi-CG, 1 = geometric-multigrid-preconditioned CG
                          (needs pucfem_set_hierarchy) */
  int32_t mg_degree;   /* Chebyshev smoothing steps per level, pre and post (2) */
  double mg_ratio;     /* Chebyshev interval [lmax / mg_ratio, lmax] (10) */
  int32_t mg_post;     /* post-smoothing steps (0: same as mg_degree) */
  int32_t mg_single;   /* 1: fp32 V-cycle (values, vectors, halos) inside the fp64 CG */
  int64_t mg_rep_nodes; /* multi-rank: coarse levels up to this many nodes are replicated (0: 1000000) */
  int32_t mg_f32_vals; /* fp32 cycle: 0 = level operators stored in fp16 when every value is representable
                          (arithmetic stays fp32), 1 = all stored in fp32, 2 = the finest in fp32 and
                          the coarser levels in fp16 */
  int32_t idx32;       /* 0 = int16 column deltas for square operators whose band fits, 1 = int32 columns */
  int32_t proj_k;      /* pressure solves (multigrid path): initial guess = A-orthogonal projection onto a
                          basis of up to proj_k directions spanning the recent solutions of the same solve
                          (Fischer 1998, deferred basis update, re-seeded when full; 3..32, 0 = off: warm
                          start from the previous solution) */
  int32_t proj_k_visc; /* the same for the two components of the viscous solve (0 = off: warm start u^n
                          plus an extrapolation of the last viscous increments) */
  int32_t mg_kind;     /* smoother polynomial: 0/1 = Chebyshev (first kind) on [lmax / mg_ratio, lmax],
                          4 = Chebyshev of the fourth kind on [0, lmax] (Lottes 2022; no mg_ratio) */
  int32_t solver_path; /* 0 = auto; 1 = multi-kernel iterative solves on every mesh (no dense inverses and no
                          one-workgroup CG on small meshes: the large-mesh code path, for parity tests) */
  int32_t assembled;   /* 0 = auto: with a multigrid hierarchy of >= 2 levels, the rows of nodes inside the
                          coarse mesh's triangles are matrix-free lattice stencils (per-face constants) and only
                          the nodes on coarse edges / vertices keep stored SELL rows; 1 = stored SELL operators
                          for every row */
  int32_t dye_scheme;  /* STOKES_COLOR dye update: 0 = semi-Lagrangian (StokesColor.py:347-389); 1 = implicit
                          FEM advection-diffusion (scripts/good_visualization.py:700-718: consistent mass +
                          convection + diffusion, the periodic penalty restated as its exact merged limit,
                          BiCGStab); single rank */
  double dye_diffusivity; /* D of the implicit variant (good_visualization.py:404: 1e-3) */
  int32_t assembly;    /* 0 = auto: on a context bound to a device, the node-triangle incidence, the stiffness
                          pattern and the K / Gx / Gy / lumped-mass values of every level (buildStiffnessMatrix,
                          buildLumpedMassMatrix and the divergence / gradient coefficients, StokesColor.py:98-128,
                          130-284) are assembled on the device, bit-identical to the host assembly; 1 = host C++ */
  int32_t proj_shared; /* 1 = the two pressure solves of a step project onto ONE basis of up to proj_k
                          directions that collects the solutions of both (the same merged operator: one
                          A-orthonormal basis serves both); 0 = a basis per solve */
} pucfem_params;

/* per-step diagnostics, the values the reference prints (StokesColor.py:586, StokesFood.py:505) */
typedef struct pucfem_step_stats {
  double max_div_star;   /* max |div u*|          */
  double max_final_div;  /* max |div u^{n+1}|     */
  double mix_I, mix_mu, mix_var; /* mixing_index (StokesColor.py:391-403) over marker==0 */
  int64_t eaten;         /* StokesFood: sum(tracer_status) */
  int32_t it_visc, it_p, it_p2; /* CG iterations of the three solves */
  int32_t sl_notfound;   /* nodes that kept c[n] because PointLocator.find returned None */
} pucfem_step_stats;

/* fields exchanged with pucfem_set_field / pucfem_get_field (reference numbering) */
enum pucfem_field {
  PUCFEM_F_U = 0,         /* u      (N,2) row-major */
  PUCFEM_F_USTAR = 1,     /* u_star (N,2) */
  PUCFEM_F_P = 2,         /* p      (N)   zero-mean gauge */
  PUCFEM_F_P2 = 3,        /* p2     (N) */
  PUCFEM_F_DIV_STAR = 4,  /* div_u_star (N) */
  PUCFEM_F_DIV_U = 5,     /* div_u      (N) (before the 2nd projection) */
  PUCFEM_F_FINAL_DIV = 6, /* final_div  (N) */
  PUCFEM_F_C = 7,         /* dye c  (N) */
  PUCFEM_F_SCALAR = 8,    /* heat u / Poisson f (N) */
  PUCFEM_F_TRACERS = 9,   /* tracer_points (n_tr,2); set_field defines n_tr */
  PUCFEM_F_STATUS = 10,   /* tracer_status (n_tr) as 0.0 / 1.0 */
  /* capture steps (n_tr) as doubles, read only: the 1-based tracer step (counted since the tracers were last set)
     in which the tracer's status first became 1, -1 while it is uncaptured.  Setting TRACERS resets them (and the
     step count) as it clears the status; setting STATUS leaves them alone. */
  PUCFEM_F_CAPTURE_STEP = 11,
  /* vorticity w (N) of the current u, read only (setting it is PUCFEM_EINVAL): calculate_vorticity
     (scripts/good_visualization2.py:310-345), w = (Gx u_y - Gy u_x) / (area_sum + 1e-12), formed on the device when
     read, as DIV_STAR is formed from u*.  It is the divergence kernel applied to (u_y, -u_x) with the swap made in
     registers, so its bits are those of PUCFEM_OP_DIV on that rotated field (which the reference's
     calculate_vorticity equals bit for bit on the host).  Stokes contexts, else PUCFEM_ESTATE.  On a multi-rank
     context pucfem_get_field serves the rank's owned rows, as for FINAL_DIV; it is not collective: every call that
     writes u leaves its ghost values current. */
  PUCFEM_F_VORTICITY = 12,
  /* all dye channels, K x N channel-major (channel k at buf[k * N + node], the caller's numbering): see "dye
     channels" below.  pucfem_set_field with count = K * N defines K (0 .. PUCFEM_MAX_DYES); count = 0 removes the
     channels (buf may then be NULL). */
  PUCFEM_F_DYES = 13,
  /* u_a (N,2) of the last inertial step, read only (setting it is PUCFEM_EINVAL): the velocity the viscous solve
     took as its right-hand side, see "inertia" below.  PUCFEM_ESTATE before the first inertial step. */
  PUCFEM_F_U_ADV = 14,
  /* the total body force f (N,2) of the current state, read only (setting it is PUCFEM_EINVAL): formed on the device
     when read, as the vorticity is, see "body forces" below; zeros with no force set.  On a partitioned context
     pucfem_get_field serves the rank's owned rows.  (This and the next enumerator count on from PUCFEM_F_U_ADV:
     15 and 16.) */
  PUCFEM_F_FORCE,
  /* r (N,2) of the last forced step, read only (setting it is PUCFEM_EINVAL): what its viscous solve took as its
     right-hand side, see "body forces" below.  PUCFEM_ESTATE before the first forced step.  Owned rows on a
     partitioned context. */
  PUCFEM_F_U_RHS,
  /* channel k is field PUCFEM_F_DYE0 + k (N values, k < K) */
  PUCFEM_F_DYE0 = 64
};
/* Fields added since count on from PUCFEM_F_U_RHS in an enumeration of their own (the numbers of pucfem_field above
   are closed: 0 .. 16 and the channels from 64).
   PUCFEM_F_DEFGRAD (17): the tracers' deformation gradient F (n_tr,4) row-major, F00 F01 F10 F11 per tracer, see
   "tracer stretching" below.  Read and set (count = 4 * n_tr; setting it resumes a run and leaves the stretch step
   count alone); PUCFEM_ESTATE while stretching is off. */
enum pucfem_field_more { PUCFEM_F_DEFGRAD = PUCFEM_F_U_RHS + 1 };
#define PUCFEM_MAX_DYES 16

/* operators for pucfem_apply / pucfem_solve / pucfem_host_get_csr */
enum pucfem_op {
  PUCFEM_OP_K = 0,      /* stiffness K (StokesColor.py:98-128), y = K x */
  PUCFEM_OP_VISC = 1,   /* A_visc (StokesColor.py:471-475) */
  PUCFEM_OP_PRES = 2,   /* periodic-merged pressure operator P^T K P (+ identity slave rows) */
  PUCFEM_OP_GX = 3,     /* lumped gradient coefficients (StokesColor.py:224-263), x-part */
  PUCFEM_OP_GY = 4,
  PUCFEM_OP_DIV = 5,    /* calculate_divergence (StokesColor.py:130-165): x = u (N,2), y = div (N) */
  PUCFEM_OP_GRAD = 6,   /* calculate_gradiant  (StokesColor.py:224-263): x = p (N), y = (N,2) */
  PUCFEM_OP_LIT = 7,    /* literal heat operator I + DT*A (heatEq.py:305) or Poisson A (poisson.py:253-278) */
  PUCFEM_OP_MCONS = 8,  /* consistent mass of the implicit dye variant (StokesColor.py:286-312; host CSR only) */
  PUCFEM_OP_MLUMP = 9,  /* lumped mass M (StokesColor.py:266-284) as a diagonal (host CSR only) */
  PUCFEM_OP_ASUM = 10,  /* area_sum of calculate_divergence (StokesColor.py:151-163) as a diagonal (host CSR only) */
  PUCFEM_OP_CURL = 11   /* calculate_vorticity (scripts/good_visualization2.py:310-345): x = u (N,2), y = w (N);
                           pucfem_apply only, on PUCFEM_OP_DIV's path and with its refusals */
};

/* ---- library / context ---------------------------------------------------------- */
int pucfem_abi_version(void);
const char* pucfem_last_error(const void* ctx);
int pucfem_device_count(int32_t* n);
int pucfem_ctx_create(int32_t device, void** out_ctx);
/* multi-GPU: one process per GPU; rank/world from torch.distributed, unique id from
   rank 0's pucfem_rccl_unique_id broadcast over the control plane. */
int pucfem_rccl_unique_id(uint8_t* out_id /* PUCFEM_UNIQUE_ID_BYTES */);
int pucfem_ctx_create_dist(int32_t device, int32_t rank, int32_t world, const uint8_t* unique_id,
                           void** out_ctx);
/* world = 1 with a real unique id creates an RCCL communicator of one rank: the context then runs the
   multi-rank data path (all-reduced dots, broadcasts, the dye range exchange) through RCCL on one GPU.
   A unique id that starts with the 16 bytes "PUCFEM-LOCALCOMM" selects the in-process test backend:
   `world` contexts created from host threads of ONE process exchange data with device-to-device
   copies instead of RCCL (multi-rank validation on a one-GPU machine). */
int pucfem_ctx_destroy(void* ctx);

/* ---- mesh + boundary conditions (replaces readNode/readEle globals, StokesColor.py:437-464) */
int pucfem_mesh_upload(void* ctx, int64_t n_nodes, const double* xy /* N x 2 */,
                       const int32_t* markers, int64_t n_tris, const int32_t* tris /* T x 3 */,
                       int32_t coord_fp32 /* 1: poisson/heat fp32 coordinates (poisson.py:40) */);
/* periodic pairs (master, slave):
   kind 0 = operator pairs: filtered pairs of StokesColor.py:449-457 / poisson.py:242-253
   kind 1 = BC-copy pairs: makePerBCU (StokesColor.py:429-431) / reapply_periodic_u (heatEq.py:298-301,
            UNFILTERED).  Sequential semantics (u[s] = u[m] in list order) are preserved. */
int pucfem_set_pairs(void* ctx, int32_t kind, int64_t n_pairs, const int64_t* pairs /* P x 2 */);
/* Dirichlet nodes and values, applied in list order (makeDirBCU StokesColor.py:405-427,
   reapply_dirchlect_u heatEq.py:282-295, Dirichlet rows poisson.py:258-278). ncomp = 2 (Stokes) or 1. */
int pucfem_set_dirichlet(void* ctx, int64_t n, const int32_t* nodes, const double* values, int32_t ncomp);
/* Poisson load g(centroid) per triangle, evaluated by the host in the reference's dtype
   (poisson.py:135-144, g = 50 sin(3y) in fp32). */
int pucfem_set_source(void* ctx, int64_t n_tris, const float* g_tri);
/* Multigrid hierarchy: the uploaded mesh must be `levels` red refinements (pucfem_refine) of this
   coarse mesh; the library rebuilds the intermediate levels and checks the result bit for bit. */
int pucfem_set_hierarchy(void* ctx, int64_t n_nodes0, const double* xy0, const int32_t* markers0,
                         int64_t n_tris0, const int32_t* tris0, int32_t levels);
int pucfem_build_operators(void* ctx, const pucfem_params* params);

/* ---- fields ---------------------------------------------------------------------- */
int pucfem_set_field(void* ctx, int32_t field, const double* buf, int64_t count);
int pucfem_get_field(void* ctx, int32_t field, double* buf, int64_t count);

/* ---- time stepping: nsteps iterations of the scheme's loop body ------------------- */
/* Within one call, single-rank StokesColor with the semi-Lagrangian dye runs each step's dye tail
   (final divergence, advection, mixing sums) on a second stream overlapped with the next step's
   solves (PUCFEM_SL_OVERLAP=0: one stream); the call returns with all of it complete, so fields and
   stats read afterwards are those of the last step, as with one stream. */
int pucfem_step(void* ctx, int32_t nsteps, pucfem_step_stats* stats /* nsteps entries or NULL */);

/* ---- ensembles: several squirmers on one mesh and fluid, stepped together ----------- */
/* The reference's experiment is a comparison of swimmers on the same mesh (README.md:43-45: food eaten by the
   neutral, pusher and puller squirmers, one run of StokesFood.py each).  An ensemble is M members (1..4096)
   stepped together on ONE built context: they share everything pucfem_build_operators made (the dense inverses,
   the gradient / divergence coefficients, the point locator, the tracer grid) and differ in their Dirichlet
   values, their fields u / c and their tracers.  Every member's arithmetic is the single context's, operation
   for operation, so its fields are bit-identical to a pucfem_step run with its boundary values.
   Requirements: a single-rank STOKES_COLOR (semi-Lagrangian dye) or STOKES_FOOD context on the dense small-mesh
   path (pucfem_path_info out[0] == out[1] == 0: N <= 1500), else PUCFEM_ESTATE; a device, else PUCFEM_ENODEV.
   The ensemble owns its state: the context's own fields, step graph and records are not touched.  One ensemble
   per context; pucfem_ctx_destroy and pucfem_build_operators destroy it.
   dir_values: members x n_dirichlet x 2, each member's values in the node order given to pucfem_set_dirichlet.
   Members start as pucfem_build_operators leaves the context: u = 0 then makeDirBCU with the member's values
   (StokesColor.py:482-483), c = 1[x < 0.5] (:493-495), the context's current tracers with status 0. */
int pucfem_ens_create(void* ctx, int32_t members, const double* dir_values);
int pucfem_ens_destroy(void* ctx);
/* fields PUCFEM_F_U, _USTAR, _P, _P2, _C, _TRACERS, _STATUS (and, read only, _CAPTURE_STEP and _VORTICITY, the
   latter formed from the members' u when read into a buffer of the ensemble's own) in the caller's numbering;
   member = -1: all members, member-major (count = members x the field's values per member).  Setting
   TRACERS clears the status, the capture steps and the step count of the members it sets.
   PUCFEM_F_U_ADV, read only (setting it is PUCFEM_EINVAL): the member's u_a of its last inertial step, see
   pucfem_ens_set_inertia; PUCFEM_ESTATE when a requested member has taken none since it was switched on (with
   member = -1: as soon as any member has taken none). */
int pucfem_ens_set_field(void* ctx, int32_t field, int32_t member, const double* buf, int64_t count);
int pucfem_ens_get_field(void* ctx, int32_t field, int32_t member, double* buf, int64_t count);
/* nsteps steps of every member (StokesColor.py:537-586 / StokesFood.py:441-505 per member); stats: NULL or
   nsteps x members entries, step s of member m at s * members + m (it_* = 0: direct solves) */
int pucfem_ens_step(void* ctx, int32_t nsteps, pucfem_step_stats* stats);
/* out[0] members, [1] members per block of the dense products, [2] bytes of ensemble state on the device,
   [3] steps taken since pucfem_ens_create */
int pucfem_ens_info(void* ctx, int64_t* out4);

/* ---- sampling and rasterising: fields at arbitrary points and as images, on the device --- */
/* The reference reads a field at a point by locating the point's triangle and interpolating from its vertices
   (StokesFood.py:482-487, the tracers' velocity), and its results are frames: the dye under a quiver of the
   velocity (scripts/good_visualization2.py:536-571, a tripcolor of the whole mesh).  These calls do both from
   caller-given points on the device with the context's point locator, so a probe, a line cut or a frame costs
   its points, not a copy of the whole fields.
   Semantics, for a query point q = (x, y) taken as given (no periodic wrap, no clamp): among the triangles that
   pass the reference's weight test (|det| >= 1e-14 and all three weights >= 0, StokesColor.py:325-333) the one
   with the smallest (squared centroid distance, triangle id); the value is the reference's interpolation on it
   (StokesColor.py:374-386).  A point on a shared edge or vertex so has one answer.  PointLocator's restriction
   to the 10 nearest centroids (StokesColor.py:324) is NOT applied: a sampler wants containment.  Where no
   triangle passes (outside [0,1]^2, inside the swimmer, a non-finite q) the value is NaN and the triangle -1.
   Fields: PUCFEM_F_U and _USTAR (2 components: x then y), _P, _P2, _DIV_STAR, _DIV_U, _FINAL_DIV, _C, _VORTICITY
   (1 each);
   at most 16 components per call.  Single-rank STOKES_COLOR / STOKES_FOOD contexts after pucfem_build_operators,
   else PUCFEM_ESTATE (heat / Poisson contexts have no locator; a multi-rank context's fields are partitioned);
   PUCFEM_ENODEV on a host-only context; PUCFEM_EINVAL for another field, nfields < 1, a non-positive size, a
   window without x0 < x1 and y0 < y1, or more than 2^31 - 1 pixels.  The calls run on the context's stream after
   everything pending on it (after pucfem_step returns they see the last step's fields) and change no state of
   the context or its ensemble; their device buffers are allocated at first use and kept. */
/* out: fp64, field-major (component k of point e at out[k * npoints + e], components in the order of `fields`);
   tri_out (or NULL): the triangle in the caller's numbering, -1 where none passes */
int pucfem_sample_points(void* ctx, int32_t nfields, const int32_t* fields, int64_t npoints,
                         const double* xy /* npoints x 2 */, double* out /* sum(ncomp) x npoints */,
                         int32_t* tri_out /* npoints or NULL */);
/* A width x height image of the window [x0, x1] x [y0, y1]: pixel (i, j) is the value at its centre
   (x0 + (i + 0.5) (x1 - x0) / width, y0 + (j + 0.5) (y1 - y0) / height), row j = 0 the lowest y;
   out: fp32, [component][height][width] (the fp64 value rounded to nearest) */
int pucfem_raster(void* ctx, int32_t nfields, const int32_t* fields, int32_t width, int32_t height,
                  const double* window4 /* x0 y0 x1 y1, NULL = 0 0 1 1 */, float* out);
/* The same image of every member of the context's ensemble (README.md:43-45: the swimmers side by side), each
   pixel located once for all members; fields PUCFEM_F_U, _USTAR, _P, _P2, _C, _VORTICITY (formed from the members'
   u into an ensemble-owned buffer, allocated at first use and kept); member = -1: all members,
   out [member][component][height][width], else that member's [component][height][width].  PUCFEM_ESTATE without
   an ensemble. */
int pucfem_ens_raster(void* ctx, int32_t nfields, const int32_t* fields, int32_t member /* -1 = all */,
                      int32_t width, int32_t height, const double* window4, float* out);

/* ---- dye channels: several dyes advected per step from one back-trace ------------- */
/* The reference starts its dye three ways: the half plane (StokesColor.py:495), a thin stripe at x = 0.2
   (scripts/good_visualization2.py:520-524) and a blob at (0.5, 0.75) (scripts/good_visualization.py:555-559); how
   well a swimmer mixes depends on which one is asked about.  A context carries up to PUCFEM_MAX_DYES extra dye
   fields beside c.  Every pucfem_step advects all of them with that step's final u and dt by the semi-Lagrangian
   scheme of c (StokesColor.py:347-389), the departure point and its triangle found once per node for all channels.
   Channel k holds, bit for bit, what c would hold in a run whose c was started from channel k's values; u, p, c and
   the step statistics of the run are those of a run without channels.
   Single-rank PUCFEM_STOKES_COLOR contexts with dye_scheme = 0 after pucfem_build_operators, else PUCFEM_ESTATE
   (multi-rank, STOKES_FOOD, heat, Poisson, the implicit dye; before the build); PUCFEM_ENODEV on a host-only context;
   PUCFEM_EINVAL for a count that is no multiple of N, more than PUCFEM_MAX_DYES channels, nch outside
   1 .. PUCFEM_MAX_DYES, or a channel k >= K.  Setting PUCFEM_F_DYES resets the channel step count; setting one
   channel (PUCFEM_F_DYE0 + k), PUCFEM_F_C or PUCFEM_F_U leaves the channels and their count alone.
   pucfem_build_operators and pucfem_ctx_destroy drop the channels.  PUCFEM_F_DYE0 + k is also a one-component
   field of pucfem_sample_points, pucfem_raster and the values of pucfem_streamlines.  Ensembles carry channels of
   their own, the same number for every member (pucfem_ens_set_dyes below); an ensemble without channels takes no
   dye field (PUCFEM_EINVAL in the pucfem_ens_* calls).  A small-mesh context steps from a captured graph only while
   it has no channels; with channels it runs the same launches uncaptured (the same bits). */
/* out[0] K, [1] channel steps since the channels were set, [2] not-found rows of the last channel launch (the same
   for every channel; 0 before the first), [3] device bytes held for the channels */
int pucfem_dyes_info(void* ctx, int64_t* out4);
/* (I, mu, var) of every channel over marker == 0, out[3 * k + {0, 1, 2}]: computed at the call by the reduction
   of pucfem_mixing_index, so row k holds the bits of pucfem_mixing_index(ctx, channel k read back, ...).  Changes
   no state. */
int pucfem_dyes_mixing(void* ctx, double* out /* K x 3 */);
/* Measurement: the channels' kernel with nch channels (scratch buffers, zero fields) on the context's current u and
   dt, launched once untimed and then `iters` times back to back between two events.  out2[0]: milliseconds per
   launch; out2[1]: algorithmic bytes per launch. */
int pucfem_dyes_probe(void* ctx, int32_t nch, int32_t iters, double* out2);
/* Dye channels of an ensemble: K = 0 .. PUCFEM_MAX_DYES channels, the same K for every member, beside each member's
   c.  Every pucfem_ens_step advects a member's channels with that step's final u of that member along the path that
   moves its c -- the member's dye scheme (pucfem_ens_set_advection) and trajectory (pucfem_ens_set_trajectory) --
   the departure point and its triangle found once per pass and row for c and all channels.  Channel k of member m
   holds, bit for bit, channel k of a single-context run with the member's boundary values, settings and starting
   channels; the member's u, u*, p, p2, c and step records are those of the same ensemble without channels, its
   pucfem_ens_advection_info / pucfem_ens_trajectory_info counts those of the single run with the same channels (pass
   2 counts the clamped values of c and the channels).  The step stays a captured graph.
   pucfem_ens_set_dyes defines K; every member's channels start from buf (K x N, caller numbering; NULL iff K == 0).
   K = 0 removes the channels and frees their memory: the ensemble then steps as one that never had any, launch for
   launch.  The call resets the channel step counts and drops the captured graphs.  PUCFEM_ESTATE without an ensemble
   (decided before the device is asked for) or on a PUCFEM_STOKES_FOOD ensemble; PUCFEM_EINVAL for K outside
   0 .. PUCFEM_MAX_DYES or a NULL buf with K > 0; PUCFEM_ENODEV on a host-only context.
   pucfem_ens_set_field / pucfem_ens_get_field take PUCFEM_F_DYES (K * N values per member, channel-major; member = -1:
   M * K * N, member-major) and PUCFEM_F_DYE0 + k (N values per member).  A count that does not match the ensemble's K,
   or a channel k >= K, is PUCFEM_EINVAL -- every such call while K = 0 included; pucfem_ens_raster takes
   PUCFEM_F_DYE0 + k, k < K, as a one-component field, else PUCFEM_EINVAL.  Setting a field never changes K and leaves
   the channel step counts alone, except PUCFEM_F_DYES, which resets them for the members it sets.  Not done: buoyancy
   terms on a member's channels, channel values along pucfem_ens_streamlines, a different K per member. */
int pucfem_ens_set_dyes(void* ctx, int32_t K, const double* buf /* K x N; NULL iff K == 0 */);
/* out[0] K, [1] channel steps since the member's channels were last set, [2] not-found rows of the member's last dye
   launch (pass 1's; 0 before the first), [3] device bytes the ensemble holds for channels, all sets */
int pucfem_ens_dyes_info(void* ctx, int32_t member, int64_t* out4);
/* (I, mu, var) of every channel of the requested members, out[(m * K + k) * 3 + {0, 1, 2}]: computed at the call by
   the reduction of pucfem_mixing_index (one launch per stage over every member and channel), so each row holds the
   bits of pucfem_mixing_index(ctx, that channel read back, ...).  Changes no state.  PUCFEM_ESTATE with K = 0. */
int pucfem_ens_dyes_mixing(void* ctx, int32_t member /* -1 = all */, double* out /* [members x] K x 3 */);

/* ---- inertia: semi-Lagrangian advection of the velocity in front of the viscous solve ---- */
/* The reference's step is at Reynolds number zero: its viscous solve takes u + DT * 0 as the right-hand side
   (StokesColor.py:540-547), the inertial term still a placeholder.  With inertia on, every pucfem_step first advects
   the velocity by itself, each component by advect_semilagrange (StokesColor.py:347-389),
     u_a = SL(u^n; u^n, dt),   u* = A_visc^-1 u_a,   then the projections, the dye / the tracers as before
   (Stam's "stable fluids" splitting).  A step with inertia on holds, bit for bit on the direct-solve paths, what a
   step without it computes after pucfem_set_field(PUCFEM_F_U, pucfem_sl_advect_vel(u, u, dt)); the iterative paths
   also start the viscous solve from u_a and its increments.  A row whose departure point is not found keeps its
   value.  Single-rank PUCFEM_STOKES_COLOR (either dye scheme) and PUCFEM_STOKES_FOOD contexts after
   pucfem_build_operators, on every solver path, with or without dye channels; else PUCFEM_ESTATE (multi-rank, heat,
   Poisson; before the build); PUCFEM_ENODEV on a host-only context.  The context's flag is for pucfem_step alone:
   ensembles carry their own flags, one per member (pucfem_ens_set_inertia below), and the two stay apart --
   pucfem_ens_create on a context whose flag is on, and switching it on while an ensemble exists, are PUCFEM_ESTATE.
   The N x 2 buffer of u_a is allocated when inertia is first switched on; pucfem_build_operators and
   pucfem_ctx_destroy free it and switch inertia off.  Switching it on or off resets the viscous solve's
   extrapolation history, as setting u does.  A small-mesh context steps from its captured graph only while inertia
   is off; with it on it runs the same launches uncaptured behind the inertial one. */
int pucfem_set_inertia(void* ctx, int32_t on);
/* out[0] on, [1] inertial steps since it was switched on, [2] not-found rows of the last inertial launch (0 before
   the first), [3] device bytes held for it */
int pucfem_inertia_info(void* ctx, int64_t* out4);
/* Measurement: the inertial launch (f = u = the context's current u, its dt, a scratch output), launched once untimed
   and then `iters` times back to back between two events.  out2[0]: milliseconds per launch; out2[1]: algorithmic
   bytes per launch. */
int pucfem_inertia_probe(void* ctx, int32_t iters, double* out2);
/* Inertia per ensemble member: the reference's comparison of swimmers at finite Reynolds number, or a Stokes twin
   beside each inertial swimmer, in one launch chain.  A member whose flag is on steps u_a = SL(u^n; u^n, dt) and then
   the ensemble's step with u_a as the viscous product's input: bit for bit a pucfem_step run with inertia on and the
   member's boundary values.  A member whose flag is off steps as without this call.  Flags may differ between
   members; a flag set between two pucfem_ens_step calls takes effect at the next step, and switching a member on
   starts its counts again.  The step stays one captured chain, with the inertial launch in front while at least one
   flag is on.  The members' u_a (members x N x 2) and the launch's partials are allocated when a flag is first
   switched on, are counted in pucfem_ens_info's bytes and are freed with the ensemble.
   member = -1: every member.  PUCFEM_ESTATE without an ensemble; PUCFEM_EINVAL for a member out of range. */
int pucfem_ens_set_inertia(void* ctx, int32_t member /* -1 = all */, int32_t on);
/* member 0 .. members - 1: out[0] on, [1] inertial steps since the member was switched on, [2] not-found rows of its
   last inertial launch (summed on the device; 0 before the first), [3] device bytes the ensemble holds for inertia */
int pucfem_ens_inertia_info(void* ctx, int32_t member, int64_t* out4);

/* ---- body forces: driven channel flow and buoyant dye ---- */
/* The reference forms the viscous right-hand side as u + DT * b_force (StokesColor.py:485-486, 540-541,
   StokesFood.py:405-406, 444-445) and its experiments set b_force[:, 0] = 0.1, a mean pressure gradient in the
   x-periodic channel.  With a force set, every pucfem_step forms, for owned row i, every product and sum as written
   (base: what the viscous solve takes without a force -- u^n, or u_a with inertia on):
     f = (0, 0)
     constant F given:      f = F
     nodal field fn given:  f = f + fn[i]                       (per component; if no F was given, f = fn[i])
     buoyancy given:        b = beta_0 * (s_0[i] - ref_0)
                            for t = 1 .. nterms - 1:  b = b + beta_t * (s_t[i] - ref_t)
                            f = (f.x + g.x * b, f.y + g.y * b)
     r[i] = (base[i].x + dt * f.x,  base[i].y + dt * f.y)
   Terms that are not given are skipped, not added as zeros.  s_t is c or a dye channel as it stands at the start of
   the step (c^n: Boussinesq buoyancy, the dye pushes back).  r replaces base wherever the viscous solve reads it: as
   its right-hand side and as the base of its start and of its increments.  Nothing else in the step changes: the
   boundary rows of u* are overwritten as before, so a force at a Dirichlet node has no effect.  On the direct-solve
   paths a forced step holds, bit for bit, what an unforced step computes after
   pucfem_set_field(PUCFEM_F_U, pucfem_force_apply(u, dt)); PUCFEM_F_U_ADV still holds u_a without the force.
   PUCFEM_STOKES_COLOR (either dye scheme) and PUCFEM_STOKES_FOOD contexts after pucfem_build_operators, on every
   solver path, with or without inertia, dye channels, MacCormack advection and Brownian tracers.  The uniform and
   the nodal force are element-wise on the rows a rank owns and also run on partitioned contexts (every rank sets the
   same force; the field is N x 2 on every rank).  Buoyancy reads the dye the previous step's tail wrote: such steps
   wait for that tail in front of the viscous solve instead of overlapping it, and a partitioned context, whose tail
   runs behind the next viscous solve, refuses buoyancy.
   pucfem_set_force with both pointers NULL, or F = (0, 0) and no field, switches that part off; with every part off
   the step is the one without these calls, launch for launch.  The buffers (r, the nodal field; owned rows x 2) are
   allocated when first needed; pucfem_build_operators and pucfem_ctx_destroy free them and switch every force off.
   Setting or clearing a force resets the viscous solve's extrapolation history, as setting u does.  A small-mesh
   context steps from its captured graph only while no force is set; with one it runs the same launches uncaptured
   behind k_force_rhs.  The context's setting is for pucfem_step alone; ensembles carry their own settings, one per
   member (pucfem_ens_set_force / pucfem_ens_set_buoyancy below), and the two stay apart.
   PUCFEM_EINVAL: a non-finite value.  PUCFEM_ESTATE: before the build; heat and Poisson contexts.  PUCFEM_ENODEV on
   a host-only context. */
int pucfem_set_force(void* ctx, const double* F2 /* or NULL */, const double* field /* N x 2, caller numbering, or NULL */);
/* fields[t]: PUCFEM_F_C or PUCFEM_F_DYE0 + k; nterms = 0: off (the other arguments may then be NULL).
   PUCFEM_EINVAL: nterms outside 0 .. 17, a non-finite g, beta or ref, an unknown or repeated field.  PUCFEM_ESTATE:
   before the build, heat and Poisson contexts, PUCFEM_STOKES_FOOD (it has no dye), partitioned contexts, a channel
   k >= K.  Removing or redefining the channels (PUCFEM_F_DYES) while a term names one switches buoyancy off. */
int pucfem_set_buoyancy(void* ctx, const double* g2, int32_t nterms, const int32_t* fields, const double* beta,
                        const double* ref);
/* Body forces per ensemble member: a sweep over the background flow's strength against the neutral swimmer, the pusher
   and the puller, or a buoyant dye per member, in one launch chain.  A forced member steps r = base + dt * f (base:
   its u, or its u_a when its inertia flag is on) and then the ensemble's step with r as the viscous product's input:
   bit for bit a pucfem_step run with the same setting and the member's boundary values.  A member with no force
   steps as without these calls.  Settings may differ between members; one set between two pucfem_ens_step calls takes
   effect at the next step and starts the member's count again.  F2 NULL or (0, 0) and field NULL switch those parts
   off; field is one N x 2 array (caller numbering) given to every requested member.  Members have c only: their
   buoyancy is one term, f += g * beta * (c - ref); g2 NULL switches it off.  The step stays one captured chain,
   with k_ens_force_rhs in front of the viscous product while at least one member is forced; it is captured again only
   when that changes and when the nodal planes are first allocated (which members are forced, and how, the kernel
   reads from device memory).  The members' r (members x N x 2), masks and parameters (members x 8 doubles) are
   allocated when a member is first forced, the nodal planes (members x N x 2) when one is first given a field; they
   are counted in pucfem_ens_info's bytes and freed with the ensemble.
   member = -1: every member.  PUCFEM_ESTATE without an ensemble (and for buoyancy on PUCFEM_STOKES_FOOD);
   PUCFEM_EINVAL for a member out of range and for a non-finite value.
   pucfem_ens_get_field serves PUCFEM_F_FORCE (every member's f of the current state, zeros for an unforced member)
   and PUCFEM_F_U_RHS (PUCFEM_ESTATE when a requested member has taken no forced step since its setting last
   changed). */
int pucfem_ens_set_force(void* ctx, int32_t member /* -1 = all */, const double* F2, const double* field /* N x 2 or NULL */);
int pucfem_ens_set_buoyancy(void* ctx, int32_t member, const double* g2, double beta, double ref);
/* member = -1, the context: out[0] bit mask of the terms present (1 uniform, 2 nodal, 4 buoyancy), [1] forced steps
   since the setting last changed, [2] buoyancy terms, [3] device bytes held.  member 0 .. members - 1: the same of an
   ensemble member ([3]: the bytes the ensemble holds for forces); PUCFEM_ESTATE without an ensemble, PUCFEM_EINVAL for
   a member out of range. */
int pucfem_force_info(void* ctx, int32_t member, int64_t* out4);
/* Unit operation: out = r from the context's current setting and current dye fields and the caller's base (N x 2)
   and dt, through the step's kernel on scratch buffers; the step's state is not touched.  With no force set out is
   base + dt * 0. */
int pucfem_force_apply(void* ctx, const double* base, double dt, double* out);
/* Measurement: the step's launch (base = the context's current u, its dt, a scratch output), launched once untimed and
   then `iters` times back to back between two events.  out2[0]: milliseconds per launch; out2[1]: algorithmic bytes
   per launch (32 per row, 16 more with a nodal field, 8 more per buoyancy term). */
int pucfem_force_probe(void* ctx, int32_t iters, double* out2);

/* ---- time-dependent strokes: boundary values that vary per step ---- */
/* The Dirichlet values of pucfem_set_dirichlet are fixed for a run: every swimmer is steady, and a steady
   two-dimensional flow stretches dye along its streamlines without mixing it.  A stroke makes the values of `n` driven
   Dirichlet nodes periodic in time: K modes (1 .. 8), a table amp[P][K] (1 <= P <= 65536), a start row, and per driven
   node q a shape[q][K] and a direction dir[q] (a pair).  With s the steps taken since the stroke was set (a counter in
   device memory, advanced on the device), the step being taken imposes, every product and sum as written,

     row    = (start + s) mod P
     vt     = amp[row][0] * shape[q][0]
     vt     = vt + amp[row][j] * shape[q][j]      j = 1 .. K - 1, in this order
     val[q] = (vt * dir[q].x, vt * dir[q].y)

   written into the context's Dirichlet value array in front of the step's first launch (k_stroke_bc, one block) and
   held for every boundary-condition application of that step.  Dirichlet nodes the stroke does not drive (the walls)
   keep their values.  With shape = (sin th, sin 2 th, ...) and dir = (-sin th, cos th) a table whose rows are all
   (B1, B2) gives the bits of the static squirmer values.  The reference zeroes the Dirichlet rows and columns of the
   viscous matrix, so the values enter a step only through that array: a stroked step is, bit for bit on the
   direct-solve paths, the step of a context built with the row's values, taken from the same fields.
   Setting a stroke does not touch u; it resets s to 0 and the viscous solve's extrapolation history, as a force change
   does.  K = 0 clears the stroke and restores the values the build uploaded (off stays off: nothing is touched).
   pucfem_build_operators and pucfem_ctx_destroy clear it.  Off is the default, and with the stroke off a step is
   launch for launch what it was.  A small-mesh context steps from its captured graph only while no stroke is set; with
   one it runs the same launches uncaptured behind k_stroke_bc (the graph is kept: clearing the stroke returns to it).
   PUCFEM_ESTATE: a heat or Poisson context, a multi-rank context, a context that has an ensemble (its members carry
   their own strokes), pucfem_ens_create on a context whose stroke is on.  PUCFEM_EINVAL: K or P out of range,
   start < 0, a non-finite table, shape or direction, a driven node that is not in the Dirichlet list or is listed
   twice.  `nodes` are in the caller's numbering. */
int pucfem_set_stroke(void* ctx, int32_t K, int32_t P, const double* amp, int32_t n, const int32_t* nodes,
                      const double* shape /* n x K */, const double* dir /* n x 2 */, int64_t start);
/* The same per ensemble member: each member has its own table, period, start row and counter (k_ens_stroke_bc, one
   block per member, in front of the chain while at least one member has a stroke; the step stays one captured graph,
   captured again only when "any member stroked" changes or the tables or shapes are reallocated).  The shapes,
   directions and nodes are shared: those of the first call stand for all members, and a later call whose n, K, nodes,
   shapes or directions differ is PUCFEM_EINVAL unless every member's stroke is off.  A member without a stroke is
   skipped: its values and counter are left alone.  K = 0 clears the member's stroke and restores the values
   pucfem_ens_create gave it.  A stroked member steps bit for bit as a pucfem_step run with the same stroke. */
int pucfem_ens_set_stroke(void* ctx, int32_t member /* -1 = all */, int32_t K, int32_t P, const double* amp, int32_t n,
                          const int32_t* nodes, const double* shape, const double* dir, int64_t start);
/* member = -1, the context; 0 .. members - 1: an ensemble member.  out[0] K (0: off), [1] P, [2] start (mod P),
   [3] steps taken since the stroke was set (read from the device), [4] the row the next step imposes, [5] driven
   nodes. */
int pucfem_stroke_info(void* ctx, int32_t member, int64_t* out6);
/* The Dirichlet values the device holds now (the context's, or an ensemble member's), ndirlist x ncomp in the order of
   the list given to pucfem_set_dirichlet; a node listed more than once reports its kept (last) value in every place.
   Single-rank contexts. */
int pucfem_get_dirichlet(void* ctx, int32_t member, double* out);
/* Unit operation: row `row` of the stroke (the context's, or a member's) evaluated by the step's kernel into a scratch
   copy of the Dirichlet values, returned as pucfem_get_dirichlet returns them.  The step's state, the values and the
   counter are not touched.  PUCFEM_ESTATE with no stroke set. */
int pucfem_stroke_apply(void* ctx, int32_t member, int64_t row, double* out);
/* Measurement: the context's step launch (counter read, barrier, counter store) on a scratch copy of the values and a
   scratch counter, launched once untimed and then `iters` times back to back between two events.  out2[0]:
   milliseconds per launch; out2[1]: algorithmic bytes per launch (32 + 8 K per driven node). */
int pucfem_stroke_probe(void* ctx, int32_t iters, double* out2);

/* ---- Brownian tracers: food that diffuses ---- */
/* The tracers are deterministic points; in the steady flow a run settles to, a tracer on a streamline outside the
   capture annulus is never eaten.  With a diffusivity D > 0 every free tracer also takes a random-walk increment per
   tracer step, reproducible bit for bit from a 64-bit seed.  For tracer k in the 1-based tracer step `stepno` (the
   count pucfem_tracer_info reports, plus one), every product and sum as written:
     status[k] == 1 at the start of the step: absorbed food -- nothing is loaded or stored for it, it counts as eaten
     else  (vx, vy) as without diffusion (NaN outside the mesh)
           r0..r3 = Philox4x32-10(counter = (k, stepno, 0, 0), key = (seed & 0xffffffff, seed >> 32))
           U1 = ((r0 >> 5) * 67108864.0 + (r1 >> 6)) * 2^-53, U2 likewise from r2, r3      (in [0, 1), exact)
           a  = sqrt(6.0 * D * dt)                                                          (host, double)
           nx = (px + vx * dt) + a * (2.0 * U1 - 1.0),  ny = (py + vy * dt) + a * (2.0 * U2 - 1.0)
           nx = nx mod 1;  ny < ylo: ny = ylo + (ylo - ny), else ny > yhi: ny = yhi - (ny - yhi)
           store, then the capture test (sqrt(ddx*ddx + ddy*ddy) <= capture_radius; the capture step on the transition)
   ylo, yhi: the smallest and largest node y of the mesh (the no-slip walls), from the build.  The increments are
   uniform on [-a, a], variance 2 D dt per coordinate; NaN stays NaN.  The random stream depends on (seed, k, stepno)
   only -- not on the kernel form, the grid, the member index or the launch count -- and setting the tracers resets
   stepno and so restarts it.  D = 0 (the default) is the step without this call, bit for bit and launch for launch:
   eaten tracers keep moving there; the freeze belongs to D > 0.
   pucfem_set_tracer_diffusion governs pucfem_step and pucfem_tracer_step (there dt is the call's own) of single-rank
   PUCFEM_STOKES_COLOR / PUCFEM_STOKES_FOOD contexts after pucfem_build_operators, on every solver path, with or
   without inertia.  PUCFEM_ESTATE on multi-rank, heat and Poisson contexts and before the build (decided before the
   device is asked for); PUCFEM_EINVAL for D negative, NaN or infinite; PUCFEM_ENODEV on a host-only context.  A
   setting made between two steps takes effect at the next step (a small-mesh context captures its step again).
   pucfem_build_operators and pucfem_ctx_destroy set D back to 0.  The context holds no device memory for it. */
int pucfem_set_tracer_diffusion(void* ctx, double D, uint64_t seed);
/* The same per ensemble member (member = -1: every member); the context's setting and the members' stay apart.  Two
   members with one seed draw the same increments (common random numbers).  A member steps bit for bit as a
   pucfem_step run with its D and seed; a member with D = 0 takes the plain move.  The step stays one captured chain,
   captured again only between "no member on" and "some member on".  The members' amplitudes and keys (members each)
   are allocated when a member is first given D > 0, are counted in pucfem_ens_info's bytes and are freed with the
   ensemble.  PUCFEM_ESTATE as above and without an ensemble; PUCFEM_EINVAL as above and for a member out of range. */
int pucfem_ens_set_tracer_diffusion(void* ctx, int32_t member /* -1 = all */, double D, uint64_t seed);
/* The setting of the context (member = -1) or of ensemble member 0 .. members - 1; D or seed may be null. */
int pucfem_get_tracer_diffusion(void* ctx, int32_t member /* -1 = the context */, double* D, uint64_t* seed);
/* Measurement: the tracer launch of pucfem_step (the context's current u, tracers and diffusion setting; time step
   dt), launched once untimed and then `iters` times back to back between two events; the tracers move.
   out2[0]: milliseconds per launch; out2[1]: tracers. */
int pucfem_tracer_probe(void* ctx, double dt, int32_t iters, double* out2);

/* ---- tracer stretching: the deformation gradient and the FTLE per tracer ---- */
/* The dye's mixing index is mostly the interpolation's diffusion.  The diffusion-free measure of mixing is the
   stretching of material lines: the deformation gradient F = dPhi/dX of the flow map along each tracer's path, its
   largest singular value, and the finite-time Lyapunov exponent built from it.  The velocity is P1, so its gradient is
   constant per triangle and the tracer step is piecewise affine in the tracer's position: the update below is the
   exact Jacobian of the discrete step.  With stretching on, every tracer whose iteration of the tracer launch runs
   carries a row F00 F01 F10 F11 of F (n_tr x 4, row-major, the identity at first).  Every product and sum is as
   written, in double, without contraction.
   Per tracer and tracer step: the tracer is at p in triangle t; (ax, bx) are the plane coefficients of ux in t
   (ux = ax x + bx y + cx there), (ay, by) those of uy -- the values the interpolation of the velocity forms.
     Euler step          J00 = 1 + dt*ax   J01 = dt*bx   J10 = dt*ay   J11 = 1 + dt*by
     midpoint step (pucfem_set_trajectory, PUCFEM_TRJ_TRACERS), the midpoint found in triangle tm with the
     coefficients (cx, dx) of ux and (cy, dy) of uy there; hdt = 0.5 * dt from the host:
                         A00 = 1 + hdt*ax  A01 = hdt*bx  A10 = hdt*ay  A11 = 1 + hdt*by
                         B00 = cx*A00 + dx*A10   B01 = cx*A01 + dx*A11
                         B10 = cy*A00 + dy*A10   B11 = cy*A01 + dy*A11
                         J00 = 1 + dt*B00  J01 = dt*B01  J10 = dt*B10  J11 = 1 + dt*B11
     midpoint not found (the tracer fell back to its Euler step): the Euler J
     then                F00' = J00*F00 + J01*F10   F01' = J00*F01 + J01*F11
                         F10' = J10*F00 + J11*F10   F11' = J10*F01 + J11*F11
   A tracer without a velocity (outside the mesh, or not finite): all four entries become NaN, as its position does.
   The periodic wrap in x has unit Jacobian; the Brownian increment does not depend on p, so its Jacobian is the
   identity: neither changes F.  With Brownian food F is the Jacobian of the drift map only: the wall reflection would
   negate the second row, which changes no singular value, and is not applied.  An absorbed tracer (status 1, D > 0)
   skips its iteration, so its F freezes with it; with D = 0 an eaten tracer keeps moving and its F keeps evolving.
   Stretching only reads the path: positions, status, capture steps, eaten and fell-back counts are those of the run
   without it, bit for bit; with it off the step is the step without this call, launch for launch.
   pucfem_set_tracer_stretch governs pucfem_step, pucfem_tracer_step and pucfem_tracer_probe of a single-rank
   PUCFEM_STOKES_FOOD context with tracers.  Switching it on allocates F as the identity and sets the stretch step
   count to 0; switching it off frees F.  Setting PUCFEM_F_TRACERS resets F to the identity and the count to 0; setting
   PUCFEM_F_STATUS or PUCFEM_F_DEFGRAD leaves both alone.  PUCFEM_ESTATE -- decided before the device is asked for --
   on multi-rank contexts (their tracer step is another pair of kernels), heat, Poisson and PUCFEM_STOKES_COLOR
   contexts (no tracers) and before the build; PUCFEM_ESTATE on a context whose tracer set is empty, while the context
   has an ensemble (for on and off alike), and for pucfem_ens_create while it is on: members carry their own flags.
   PUCFEM_ENODEV on a host-only context.  pucfem_build_operators and pucfem_ctx_destroy switch it off.  A small-mesh
   context steps uncaptured while it is on.  Not done: F along pucfem_streamlines, multi-rank contexts. */
int pucfem_set_tracer_stretch(void* ctx, int32_t on);
/* The same per ensemble member (member = -1: every member), off at first.  A member whose flag is on is bit for bit
   in F a pucfem_step run with its settings and the flag on; everything else of every member is the ensemble without
   this call.  The members' F (members x n_tr x 4, identity rows for a member that is off), their flags and the
   summary's buffers are allocated when a member is first switched on, counted in pucfem_ens_info's bytes and freed
   with the ensemble.  Switching a member on or off sets its rows to the identity and its count to 0; so does setting
   its tracers.  The step stays one captured chain, the STRETCH instantiation of the tracer launch while any member is
   on, captured again only between "no member on" and "some member on".  pucfem_ens_get_field / pucfem_ens_set_field
   serve PUCFEM_F_DEFGRAD (4 * n_tr values per member) while a member is on.  PUCFEM_ESTATE as above, without an
   ensemble and on an ensemble without tracers; PUCFEM_EINVAL for a member out of range. */
int pucfem_ens_set_tracer_stretch(void* ctx, int32_t member /* -1 = all */, int32_t on);
/* The summary of the context's F (member = -1) or of ensemble member 0 .. members - 1, reduced on the device when
   called (never inside a step).  Per tracer
     C00 = F00*F00 + F10*F10,  C01 = F00*F01 + F10*F11,  C11 = F01*F01 + F11*F11
     lam = 0.5*((C00 + C11) + sqrt((C00 - C11)*(C00 - C11) + 4.0*(C01*C01)))      (the larger Cauchy-Green eigenvalue)
     det = F00*F11 - F01*F10
   out8[0] the flag; [1] the tracer steps taken with it on since F was last reset; [2] the tracers whose four entries
   are finite; [3] of those, the ones with det <= 0 (the discrete map folded there: dt is too large for a Lagrangian
   statement); [4] the largest and [5] the smallest lam over the finite ones (0 and +inf when there is none); [6] the
   sum of log(lam) over the finite ones with lam > 0 and [7] the number of its terms.  All zeros while the flag was
   never on.  The FTLE over an elapsed time T is log(lam) / (2 T) per tracer.  Readiness as pucfem_set_tracer_stretch. */
int pucfem_tracer_stretch_info(void* ctx, int32_t member /* -1 = the context */, double* out8);

/* ---- MacCormack advection: second-order transport of the dye and of the velocity ---- */
/* advect_semilagrange (StokesColor.py:347-389) is first order and its linear interpolation a diffusion of order
   h^2 / dt that no parameter controls.  With the MacCormack scheme of Selle et al. (J. Sci. Comput. 35, 2008) a field
   c moves by two such advections with the one velocity u and a clamp; per node g, every product and sum as written:
     pass 1   ch[g] = SL(c; u, +dt)[g], T1 = the triangle its point location returned (none: ch[g] = c[g])
     pass 2   cb    = SL(ch; u, -dt)[g], T2 its triangle
              T1 none:  out[g] = c[g]      (mark bit 0)
              T2 none:  out[g] = ch[g]     (mark bit 1; bit 1 is set whenever T2 is none, bit 0 decides the value)
              else      e = ch[g] + 0.5 * (c[g] - cb), clamped into [min, max] of c at T1's three vertices
   so ch and cb hold the bits of pucfem_sl_advect(c, u, dt) and pucfem_sl_advect(ch, u, -dt).  The limited result
   stays inside the range of c; the scheme is not conservative (the discrete u is not divergence-free).
   what is a mask: PUCFEM_ADV_DYE moves c and the dye channels of every pucfem_step this way, from one point location
   per pass and node for all of them (single-rank PUCFEM_STOKES_COLOR with dye_scheme = 0, as the dye channels);
   PUCFEM_ADV_VELOCITY the inertial step's u_a = MC(u^n; u^n, dt) (readiness as pucfem_set_inertia; it may be set
   while inertia is off and takes effect when inertia is on).  Else PUCFEM_ESTATE (multi-rank, heat, Poisson, the
   implicit dye, PUCFEM_ADV_DYE on STOKES_FOOD; before the build; while the context has an ensemble, and
   pucfem_ens_create while a scheme is set); PUCFEM_ENODEV on a host-only context; PUCFEM_EINVAL for an unknown mask
   or scheme.  With PUCFEM_ADV_SL (the default) a context steps as if this call did not exist.  The buffers -- per
   set the intermediate fields, 16 bytes per node for T1 and the blocks' counts -- are allocated when a scheme is
   first switched on, follow the number of dye channels, and are freed by pucfem_build_operators and
   pucfem_ctx_destroy, which also set both schemes back to PUCFEM_ADV_SL.  Switching the velocity's scheme resets the
   viscous solve's extrapolation history.  A small-mesh context steps from its captured graph only while the dye's
   scheme is PUCFEM_ADV_SL (and inertia is off).  The step record's sl_notfound is pass 1's count. */
enum { PUCFEM_ADV_DYE = 1, PUCFEM_ADV_VELOCITY = 2 };
enum { PUCFEM_ADV_SL = 0, PUCFEM_ADV_MACCORMACK = 1 };
int pucfem_set_advection(void* ctx, int32_t what /* bit mask */, int32_t scheme);
/* out[0] the dye's scheme, [1] the velocity's, [2] MacCormack dye steps since the scheme was switched on, [3] velocity
   steps, [4..6] of the last dye launch: rows whose back-trace found no triangle, rows whose forward trace found none,
   clamped values (every field counts), [7..9] the same of the last velocity launch (both components count),
   [10] device bytes held for both */
int pucfem_advection_info(void* ctx, int64_t* out11);
/* Measurement: the two passes on the context's current u and dt with scratch buffers -- what = PUCFEM_ADV_DYE: nch
   zero fields; PUCFEM_ADV_VELOCITY: f = u (nch ignored) -- each launched once untimed and then `iters` times back to
   back between two events.  out4: milliseconds per launch of pass 1, of pass 2, algorithmic bytes of each. */
int pucfem_advection_probe(void* ctx, int32_t what, int32_t nch, int32_t iters, double* out4);
/* MacCormack advection per ensemble member: the comparison of swimmers with a dye whose mixing index is the flow's,
   not the interpolation's, in one launch chain.  Each member has a dye scheme and a velocity scheme (both
   PUCFEM_ADV_SL at first), apart from the context's own, which keeps governing pucfem_step alone (and
   pucfem_set_advection beside an ensemble, and pucfem_ens_create with a scheme set, stay PUCFEM_ESTATE).  A member
   whose dye scheme is on moves its c by the two passes above with the step's final u: bit for bit the c, the mixing
   record and sl_notfound (pass 1's count) of a pucfem_step run with PUCFEM_ADV_DYE set and the member's boundary
   values.  A member whose velocity scheme is on steps u_a = MC(u^n; u^n, dt) while its inertia flag is on
   (pucfem_ens_set_inertia; the scheme may be set at any time and waits for the flag); PUCFEM_F_U_ADV, the forces and
   the viscous product read that u_a.  A member with both schemes PUCFEM_ADV_SL steps as without this call.  Schemes
   may differ between members; one set between two pucfem_ens_step calls takes effect at the next step, and switching
   a scheme on starts that member's counts again.  The step stays one captured chain -- three launches more behind
   the first-order dye launch while a member's dye scheme is on, two more behind the first-order inertial launch
   while an inertial member's velocity scheme is on -- captured again only when that changes; which members run
   which, the kernels read from device memory.  Per set, allocated when a scheme is first switched on: the members'
   intermediate field (members x N doubles for the dye, members x N x 2 for the velocity), 16 bytes per node and
   member for T1, the launches' partials and ticket counters; they are counted in pucfem_ens_info's bytes and freed
   with the ensemble.
   member = -1: every member.  PUCFEM_ESTATE without an ensemble and for PUCFEM_ADV_DYE on a PUCFEM_STOKES_FOOD
   ensemble; PUCFEM_EINVAL for a member out of range, an unknown mask or scheme; PUCFEM_ENODEV on a host-only
   context. */
int pucfem_ens_set_advection(void* ctx, int32_t member /* -1 = all */, int32_t what /* bit mask */, int32_t scheme);
/* member 0 .. members - 1, pucfem_advection_info's layout: out[0] the member's dye scheme, [1] its velocity scheme,
   [2] MacCormack dye steps since that scheme was switched on, [3] velocity steps (those taken with inertia on),
   [4..6] of the member's last dye launch: rows without T1, rows without T2, clamped values, [7..9] the same of its
   last velocity launch (both components count) -- summed on the device; 0 before the first launch and while the
   scheme (for the velocity: or the inertia flag) is off -- [10] device bytes the ensemble holds for MacCormack */
int pucfem_ens_advection_info(void* ctx, int32_t member, int64_t* out11);

/* ---- midpoint trajectories: second-order back-traces and tracer steps --- */
/* Every transported thing follows one straight step of the velocity at its starting point (PUCFEM_TRJ_EULER, the
   default: X - dt u(X) for a semi-Lagrangian row, p + dt v(p) for a tracer).  With PUCFEM_TRJ_MIDPOINT the velocity is
   read again half a step along that trace and the whole step is taken with it.  Every product and sum as written
   (the library is built with -ffp-contract=off); hdt = 0.5 * dt is formed on the host.
   Fields, per row g with v = u[g] (sl_point, sl_locate_row, sl_value: pucfem_locate.hpp):
       (xm, ym) = sl_point(X_g, v, hdt);          okm = sl_locate_row(g, v, (xm, ym)) -> Tm
       w        = okm ? sl_value(Tm, (xm, ym), u as interleaved pairs) : v
       (xb, yb) = sl_point(X_g, w, dt);           ok  = sl_locate_row(g, w, (xb, yb)) -> T
       value    = ok ? sl_value(T, (xb, yb), field) : field[g]
   A row whose midpoint is not found is an Euler row (counted, and marked by the unit operations).  The second locate
   is keyed on w.  That is, bit for bit, W = pucfem_sl_advect_vel(f = u, u, 0.5 * dt) followed by
   pucfem_sl_advect_multi(c, W, dt) (pucfem_sl_advect_vel(f, W, dt) for a pair field), in one launch, with w in
   registers.  With MacCormack (pucfem_set_advection) pass 1 is the above and T1 its final triangle; pass 2 is the same
   from the same node with -dt and -hdt (the midpoint read from u, the value from ch); the clamp is unchanged.
   Tracers, per tracer at p with (vx, vy) interpolated there (NaN outside the mesh):
       mx = py_mod(px + vx * hdt, 1.0);  my = py + vy * hdt
       (wx, wy) = the velocity interpolated at (mx, my); outside the mesh (or not finite): (wx, wy) = (vx, vy)
   and then the move (with or without the Brownian increment) with (wx, wy) in place of (vx, vy).  The capture test,
   the capture step, the Philox counters and the wall reflection are untouched.
   what is a mask: PUCFEM_TRJ_DYE moves c and the dye channels of every pucfem_step this way (readiness as
   pucfem_set_advection's PUCFEM_ADV_DYE; one launch where the Euler step has k_sl and k_sl_multi, one per pass with
   MacCormack), with the same mixing sums, and sl_notfound the final locate's count; PUCFEM_TRJ_VELOCITY the inertial
   step's u_a (readiness as pucfem_set_inertia; it waits for inertia); PUCFEM_TRJ_TRACERS the tracers of a
   single-rank PUCFEM_STOKES_FOOD context, in pucfem_step and in pucfem_tracer_step (which follows the setting with
   its own dt).  Else PUCFEM_ESTATE (multi-rank, heat, Poisson, the implicit dye or STOKES_FOOD for PUCFEM_TRJ_DYE, a
   context without tracers for PUCFEM_TRJ_TRACERS; before the build; while the context has an ensemble, for either
   order, and pucfem_ens_create while a part is on: members carry their own orders, pucfem_ens_set_trajectory) --
   decided before the device is asked
   for --; PUCFEM_EINVAL for an unknown mask or order; PUCFEM_ENODEV on a host-only context.  With PUCFEM_TRJ_EULER a
   context steps as if this call did not exist, launch for launch.  A part holds the blocks' counts only, allocated
   when it is first switched on and freed by pucfem_build_operators and pucfem_ctx_destroy, which also set every part
   back to PUCFEM_TRJ_EULER.  Switching the velocity's order resets the viscous solve's extrapolation history.  A
   small-mesh context steps uncaptured while a part is on and from its captured graph again when all are off.  The
   trace uses the step's one frozen u: second order along a steady flow, first order in the flow's change in time. */
enum { PUCFEM_TRJ_DYE = 1, PUCFEM_TRJ_VELOCITY = 2, PUCFEM_TRJ_TRACERS = 4 };
enum { PUCFEM_TRJ_EULER = 1, PUCFEM_TRJ_MIDPOINT = 2 };
int pucfem_set_trajectory(void* ctx, int32_t what /* bit mask */, int32_t order);
/* out[0..2] the orders of the dye, the velocity, the tracers; [3..5] the steps each has taken with its part on since
   it was switched on; [6] of the last dye launch with the part on, the rows whose midpoint was not found (with
   MacCormack: of both passes), [7] the same of the last velocity launch, [8] of the last tracer launch the tracers
   that had a velocity and whose midpoint left the mesh; [9] device bytes held.  Readiness as pucfem_inertia_info. */
int pucfem_trajectory_info(void* ctx, int64_t* out10);
/* Unit operations on scratch buffers (the step's state is not touched): one step of nch plain fields, or of one pair
   field, along the trajectory `order` with the scheme PUCFEM_ADV_SL or PUCFEM_ADV_MACCORMACK.  marks (N or NULL):
   bit 0 the final back-trace found no triangle, bit 1 the forward trace found none (MacCormack only), bit 2 pass 1's
   midpoint was not found, bit 3 pass 2's.  tri (N or NULL): T1 (MacCormack), else -1.  With PUCFEM_TRJ_EULER they
   return the bits of pucfem_sl_advect_multi / _vel / _mc / _vel_mc.  Readiness as those; PUCFEM_EINVAL for an unknown
   order or scheme. */
int pucfem_sl_advect_traj(void* ctx, int32_t order, int32_t scheme /* PUCFEM_ADV_* */, int32_t nch,
                          const double* c /* nch x N */, const double* u, double dt, double* c_out /* nch x N */,
                          int32_t* marks /* N or NULL */, int32_t* tri /* N or NULL */);
int pucfem_sl_advect_vel_traj(void* ctx, int32_t order, int32_t scheme, const double* f /* N x 2 */,
                              const double* u /* N x 2 */, double dt, double* f_out /* N x 2 */,
                              int32_t* marks /* N or NULL */, int32_t* tri /* N or NULL */);
/* Measurement, as pucfem_advection_probe: the fused midpoint launches on the context's current u and dt with scratch
   buffers -- what = PUCFEM_TRJ_DYE: nch zero fields; PUCFEM_TRJ_VELOCITY: f = u (nch ignored).  out4: milliseconds
   per launch of pass 1 (the whole step with PUCFEM_ADV_SL), of pass 2 (0 with PUCFEM_ADV_SL), algorithmic bytes of
   each. */
int pucfem_trajectory_probe(void* ctx, int32_t what, int32_t scheme, int32_t nch, int32_t iters, double* out4);
/* Midpoint trajectories per ensemble member: the comparison of swimmers without the first-order path error, in one
   launch chain.  Each member has an order per part -- its dye, its inertial velocity, its tracers, all
   PUCFEM_TRJ_EULER at first -- apart from the context's own, which keeps governing pucfem_step and
   pucfem_tracer_step alone (and pucfem_set_trajectory beside an ensemble, and pucfem_ens_create with a part on, stay
   PUCFEM_ESTATE).  The per-row and per-tracer formulas above, unchanged, with hdt = 0.5 * dt formed on the host.
   PUCFEM_TRJ_DYE (PUCFEM_STOKES_COLOR ensembles): the member's c moves along midpoint traces under whichever dye
   scheme it has (pucfem_ens_set_advection: one pass, or MacCormack's two with the same clamp and T1 record): bit for
   bit the c, the mixing record and sl_notfound (the final locate's count) of a pucfem_step run with PUCFEM_TRJ_DYE
   set, that scheme and the member's boundary values.  PUCFEM_TRJ_VELOCITY: the member's u_a moves along midpoint
   traces while its inertia flag is on (the part may be set at any time and waits for the flag), under either velocity
   scheme; PUCFEM_F_U_ADV, the forces and the viscous product read that u_a, and pucfem_ens_inertia_info's not-found
   count is the final locate's.  PUCFEM_TRJ_TRACERS (PUCFEM_STOKES_FOOD ensembles with tracers): the member's tracers
   read their velocity again at the midpoint, with or without its Brownian increment.  A member with every part
   PUCFEM_TRJ_EULER steps as without this call.  Orders may differ between members and between parts; one set between
   two pucfem_ens_step calls takes effect at the next step, and switching a part on starts that member's counts
   again.  The step stays one captured chain -- one launch more per pass behind the first-order dye / inertial launch
   while a member runs it, the MID instantiation of the tracer launch while a member's tracer part is on -- captured
   again only when the set of launches changes; which members run which, the kernels read from device memory.
   Allocated when a part is first switched on: the members' counts, the launches' partials and ticket counters (a
   MacCormack-and-midpoint member uses the MacCormack set's intermediate field and T1 records); they are counted in
   pucfem_ens_info's bytes and freed with the ensemble.
   member = -1: every member.  PUCFEM_ENODEV on a host-only context; PUCFEM_ESTATE without an ensemble, for
   PUCFEM_TRJ_DYE on a PUCFEM_STOKES_FOOD ensemble and for PUCFEM_TRJ_TRACERS on an ensemble without tracers;
   PUCFEM_EINVAL for a member out of range, an unknown mask or order. */
int pucfem_ens_set_trajectory(void* ctx, int32_t member /* -1 = all */, int32_t what /* PUCFEM_TRJ_* mask */,
                              int32_t order);
/* member 0 .. members - 1, pucfem_trajectory_info's layout: out[0..2] the member's orders, [3..5] the steps each part
   has taken while on (the velocity's: those taken with inertia on), [6] of the member's last dye launch with the part
   on the rows whose midpoint was not found (with MacCormack: of both passes), [7] the same of its last velocity
   launch, [8] of its last tracer launch the tracers that had a velocity and lost their midpoint -- summed on the
   device --, [9] device bytes the ensemble holds for trajectories */
int pucfem_ens_trajectory_info(void* ctx, int32_t member, int64_t* out10);

/* ---- streamlines: the frozen flow integrated from many seeds, on the device --- */
/* The reference's flow picture is ax.streamplot(...) of a resampled velocity (stokes_flow.py:536,
   good_visualization.py:738).  These calls integrate the context's current u from caller-given seeds with the
   samplers' locate and interpolation, the whole loop of a line in one kernel thread.
   Locating a point p: T(p) is the triangle pucfem_sample_points finds (above); V(p) = (u_x, u_y) interpolated on
   it; "none" when no triangle passes.  The direction D(v): with ax = |vx|, ay = |vy| the line is stagnant when
   !(ax > vmin || ay > vmin); else d = v (time mode), or with PUCFEM_SLN_UNIT d = (vx / m, vy / m),
   m = ax > ay ? ax : ay -- the max norm on purpose: the same curve re-parameterised with a step between |h| and
   sqrt(2) |h|, from a correctly rounded division alone.  One line, from the seed q0 with the signed step h:
     p = q0 (as given: no wrap, no clamp);  T(p) none: status SEED_OUTSIDE, npts 0, stop;  store p as point 0
     for s = 1 .. nsteps:
       d = D(V(p));                                             stagnant: status STAGNANT, stop
       midpoint (default): q = (mod1(p.x + (0.5 * h) * d.x), p.y + (0.5 * h) * d.y)
                           T(q) none: status LEFT, stop;  d = D(V(q));  stagnant: status STAGNANT, stop
       pn = (mod1(p.x + h * d.x), p.y + h * d.y);               T(pn) none: status LEFT, stop (pn is not stored)
       p = pn;  store p as point s
     status COMPLETE when all nsteps were taken
   with every product and sum as written (unfused fp64) and mod1 numpy's x % 1.0: only x wraps, the walls are at
   y = 0 and y = 1, and every stored point lies in a triangle.  PUCFEM_SLN_EULER takes one stage per step (the
   tracer step's integrator).  PUCFEM_SLN_BOTH: lines = 2 * nseeds, line e < nseeds runs with +h and line
   nseeds + e with -h; otherwise lines = nseeds.
   Outputs, step-major: points[(s * lines + e) * 2 + {0, 1}], s = 0 .. nsteps, NaN past the end of a line;
   status[e]: 0 COMPLETE, 1 LEFT, 2 STAGNANT, 3 SEED_OUTSIDE;  npts[e]: the points stored;
   values[(k * (nsteps + 1) + s) * lines + e]: component k of `fields` (those of pucfem_sample_points, at most 16
   components) at stored point s -- what pucfem_sample_points returns there -- NaN past the end.
   Readiness and refusals are the samplers'.  PUCFEM_EINVAL also for nseeds < 1, nsteps < 1, h zero or not finite,
   vmin negative or not finite, unknown flag bits, values given without fields or the reverse, or more than 2^26
   stored points ((nsteps + 1) * lines * members: 1 GiB of output).  The calls run on the context's stream after
   everything pending on it and change no state of the context or its ensemble. */
enum pucfem_streamline_flag { PUCFEM_SLN_UNIT = 1, PUCFEM_SLN_EULER = 2, PUCFEM_SLN_BOTH = 4 };
enum pucfem_streamline_status {
  PUCFEM_SLN_COMPLETE = 0,
  PUCFEM_SLN_LEFT = 1,
  PUCFEM_SLN_STAGNANT = 2,
  PUCFEM_SLN_SEED_OUTSIDE = 3
};
int pucfem_streamlines(void* ctx, int64_t nseeds, const double* seeds /* nseeds x 2 */, double h, int32_t nsteps,
                       int32_t flags, double vmin, int32_t nfields, const int32_t* fields /* may be 0 / NULL */,
                       double* points, int32_t* status, int32_t* npts, double* values /* NULL iff nfields == 0 */);
/* Measurement: the kernel of the call above without fields, launched once untimed and then `iters` times back to
   back between two events, the outputs left on the device.  out2[0]: milliseconds per launch; out2[1]: the bytes
   of its outputs. */
int pucfem_streamlines_probe(void* ctx, int64_t nseeds, const double* seeds, double h, int32_t nsteps, int32_t flags,
                             double vmin, int32_t iters, double* out2);
/* The same lines in every member of the context's ensemble (the neutral swimmer, the pusher and the puller side by
   side): each member locates for itself, since the velocities differ.  member = -1: all members, the outputs
   member-major (points [member][step][line][2], status and npts [member][line]); else that member's alone.
   PUCFEM_ESTATE without an ensemble. */
int pucfem_ens_streamlines(void* ctx, int32_t member /* -1 = all, member-major */, int64_t nseeds,
                           const double* seeds, double h, int32_t nsteps, int32_t flags, double vmin,
                           double* points, int32_t* status, int32_t* npts);

/* Flow summaries of the current u, reduced on the device in the pass that forms the vorticity (one launch, 32 bytes
   copied back): the scalars one plots against the swimmer's B2 -- how much it stirs and how much it moves.  With
   w_i the vorticity (PUCFEM_F_VORTICITY) and wt_i = area_sum_i + 1e-12 its row's denominator (the lumped mass to
   1e-12 absolute) over all N nodes:
     out[0] = max |w|,  out[1] = 1/2 sum wt w^2 (enstrophy),  out[2] = 1/2 sum wt |u|^2 (kinetic energy),
     out[3] = sqrt(max |u|^2) (peak speed).
   member = -1: the context's own run; otherwise that member of its ensemble (PUCFEM_ESTATE without one).  The sums
   are taken in a fixed order: two calls without a step in between return identical bits, and a member's values are
   those of a single run with its boundary values.  Changes no state of the context or its ensemble.  Single-rank
   Stokes contexts after pucfem_build_operators, else PUCFEM_ESTATE; PUCFEM_ENODEV on a host-only context. */
int pucfem_flow_info(void* ctx, int32_t member, double* out4);

/* ---- swimmer loads: force, torque, power and dissipation on the device ---- */
/* What the fluid does to the swimmer and what the swimmer spends, reduced on the device in one launch (k_loads,
   pucfem_loads.hpp) from the current u and the two projection pressures of the last step, P = p + p2 (zeros before any
   step).  The swimmer surface is the closed polygon of mesh edges whose two end nodes carry marker 2 and which lie in
   exactly one triangle, listed in ascending (triangle, local edge k) order; local edge k runs from vertex k to vertex
   (k + 1) mod 3 of its triangle and o is the third vertex.  Per edge (i, j) of triangle t, every product and sum as
   written (pucfem_loads.hpp spells out the order; tests/loads_reference.py restates it in numpy, bit for bit):
     e = X_j - X_i,  n = (e_y, -e_x), negated if n . (X_o - X_i) < 0   (length-weighted, from the body into the fluid)
     G = the constant P1 gradient of u on t (G_ab = d u_a / d x_b, formed with inv = 1 / det)
     f_p = -((P_i + P_j) / 2) n            f_v = nu (G + G^T) n              (force ON the swimmer, per unit density)
     torque = r x f  with r = (X_i + X_j) / 2 - center      power = -((u_i + u_j) / 2) . f   (delivered TO the fluid)
   and per triangle with |det| >= 1e-14 the dissipation nu A_t (2 G_xx^2 + 2 G_yy^2 + (G_xy + G_yx)^2).  The ten
   reduced values, in this order:
     [0] [1] pressure force x, y   [2] [3] viscous force x, y   [4] pressure torque   [5] viscous torque
     [6] pressure power            [7] viscous power            [8] dissipation        [9] perimeter (sum |e|)
   The sums are taken in a fixed order (a thread its items, the block, the blocks in order): two calls without a step
   in between return identical bits, and an ensemble member's values are those of a single run with its fields.
   member = -1: the context's own run; otherwise that member of its ensemble.  Changes no state: no field, no step
   buffer, no kernel-class counter.
   PUCFEM_ESTATE, decided before the device is asked for: before pucfem_build_operators, a heat or Poisson context, a
   multi-rank context, member >= 0 without an ensemble.  PUCFEM_ENODEV on a host-only context (every call below but
   pucfem_host_surface_edges).  PUCFEM_EINVAL: member < -1 or >= members, a negative capacity, rows out of range. */
int pucfem_swimmer_loads(void* ctx, int32_t member, double* out10);
/* The eight per-edge values [0] .. [7] of the list above, E x 8 in the surface list's order: the pressure and shear
   distribution around the body. */
int pucfem_surface_traction(void* ctx, int32_t member, double* out /* E x 8 */);
/* Unit operation on caller-supplied fields: u (N,2) and P = p (N) in the caller's numbering, p2 = 0, with the
   context's nu and centre; edges (E x 8) may be NULL.  The step's state is not touched. */
int pucfem_loads_apply(void* ctx, const double* u, const double* p, double* out10, double* edges /* E x 8 or NULL */);
/* The record: with capacity > 0 every pucfem_step, and every member's pucfem_ens_step, appends one row of 11 doubles
   -- the rows recorded since this call counting this one (1, 2, ...), then the ten values -- from the step's final u,
   p and p2, into a device ring of `capacity` rows (per member for an ensemble).  The row's index is a count in device
   memory taken modulo the capacity, advanced by the launch's reducing block.  capacity = 0 switches it off; every
   call frees the ring and starts again from zero rows.  The ensemble's step stays a captured graph (captured again
   when the capacity changes); a small-mesh single context steps uncaptured while recording, as a forced one does.
   Off is the default, and with the record off a step is launch for launch what it was.
   pucfem_build_operators clears it. */
int pucfem_set_loads_record(void* ctx, int32_t capacity);
/* Rows first .. first + count - 1 of the rows held (the last min(recorded, capacity), oldest first), count x 11. */
int pucfem_loads_record(void* ctx, int32_t member, int64_t first, int64_t count, double* out);
/* out[0] surface edges, [1] triangles visited, [2] rows recorded since the record was set, [3] capacity (0: off). */
int pucfem_loads_info(void* ctx, int32_t member, int64_t* out4);
/* Measurement: the context's launch once untimed and then `iters` times back to back between two events.  out2[0]:
   milliseconds per launch; out2[1]: algorithmic bytes per launch (12 per triangle for its ids, 32 per node for its
   coordinates and velocity, each counted once, and 40 per edge for its record and four pressures). */
int pucfem_loads_probe(void* ctx, int32_t iters, double* out2);

/* ---- unit operations (reference-named shims and parity tests) --------------------- */
int pucfem_apply(void* ctx, int32_t op, const double* x, double* y);
/* op VISC: b,x are (N,2) (both velocity components, StokesColor.py:544-545);
   op PRES: b = b_p (N) as formed at StokesColor.py:554, x = zero-mean p;
   op LIT : heat / Poisson literal system. */
int pucfem_solve(void* ctx, int32_t op, const double* b, double* x, double rtol, int32_t maxit,
                 int32_t* iters);
/* advect_semilagrange (StokesColor.py:347-389): c_out = SL(c, u, dt); notfound may be NULL */
int pucfem_sl_advect(void* ctx, const double* c, const double* u, double dt, double* c_out,
                     int32_t* notfound);
/* pucfem_sl_advect for nch fields at once (1 .. PUCFEM_MAX_DYES; c and c_out nch x N, field-major), through the dye
   channels' kernel on scratch buffers: one back-trace and one point location per node for all fields.  Field k of
   c_out and notfound (N or NULL) hold the bits pucfem_sl_advect returns for field k.  The step's state and the
   context's channels are not touched.  Readiness as for the dye channels (below). */
int pucfem_sl_advect_multi(void* ctx, int32_t nch, const double* c /* nch x N */, const double* u, double dt,
                           double* c_out /* nch x N */, int32_t* notfound /* N or NULL */);
/* pucfem_sl_advect for the two components of an interleaved field f (N,2) at once, through the inertial step's
   kernel on scratch buffers: one back-trace and one point location per node, each vertex's pair one load.
   Component k of f_out and notfound (N or NULL) hold the bits pucfem_sl_advect returns for the vector f[:, k].
   f may be u.  The step's state is not touched.  Readiness as for inertia (above). */
int pucfem_sl_advect_vel(void* ctx, const double* f /* N x 2 */, const double* u /* N x 2 */, double dt,
                         double* f_out /* N x 2 */, int32_t* notfound /* N or NULL */);
/* One MacCormack step (pucfem_set_advection above) of nch fields with a given u, on scratch buffers: the step's state
   is not touched.  marks (N or NULL): bit 0 / bit 1 as above; tri (N or NULL): T1's id in the mesh's triangle order,
   -1 when none.  Readiness and nch as pucfem_sl_advect_multi. */
int pucfem_sl_advect_mc(void* ctx, int32_t nch, const double* c /* nch x N */, const double* u, double dt,
                        double* c_out /* nch x N */, int32_t* marks /* N or NULL */, int32_t* tri /* N or NULL */);
/* ... of an interleaved field f (N,2), the two components limited separately: component k of f_out holds the bits
   pucfem_sl_advect_mc returns for the vector f[:, k].  f may be u.  Readiness as pucfem_sl_advect_vel. */
int pucfem_sl_advect_vel_mc(void* ctx, const double* f /* N x 2 */, const double* u /* N x 2 */, double dt,
                            double* f_out /* N x 2 */, int32_t* marks /* N or NULL */, int32_t* tri /* N or NULL */);
/* tracer step (StokesFood.py:482-499) on the tracers held in the context, with u given */
int pucfem_tracer_step(void* ctx, const double* u, double dt, int32_t nsteps);
/* the context's tracer set (member = -1) or that of member `member` of its ensemble: out[0] tracers, [1] tracers
   with status 1 (eaten), [2] tracers whose position is not finite (they left the mesh: NaN stays NaN,
   StokesFood.py:482-499) -- both counted by a reduction at this call --, [3] tracer steps since the set was set,
   [4] blocks in x of the last tracer launch (1: the one-block kernel; larger sets step one tracer per thread on a
   grid, with the same bits), [5] that launch's threads per block ([4], [5]: 0 before the first launch) */
int pucfem_tracer_info(void* ctx, int32_t member, int64_t* out6);
/* makePerBCU / makeDirBCU (StokesColor.py:405-431) on a host velocity u (N,2), in place, through the
   device's boundary kernels: which bit 0 = makePerBCU (slave <- master copies), bit 1 = makeDirBCU
   (walls and squirmer surface); both: the periodic copies first, as the step applies them.
   Single-rank Stokes contexts; the step's state is not touched (scratch buffers). */
int pucfem_apply_bc(void* ctx, int32_t which, double* u);
/* One implicit FEM dye step (scripts/good_visualization.py:700-718) on a context built with
   dye_scheme = 1: c_out = A^-1 (M c) with A = M + dt (C_u + D K) + diag(dt M_lumped div u), periodic
   pairs merged, then c[slave] = c[master]; c, c_out (N), u (N,2) in caller order; iters: BiCGStab
   iterations (may be NULL).  The step's state is not touched. */
int pucfem_dye_step(void* ctx, const double* c, const double* u, double* c_out, int32_t* iters);
/* mixing_index (StokesColor.py:391-403) over marker==0 nodes: out = (I, mu, var) */
int pucfem_mixing_index(void* ctx, const double* c, double* out3);
/* mixing_index(c, mass, mask) (StokesColor.py:391-403) with arbitrary node weights w (N, caller order): the
   reference's c[mask], mass[mask] is w = mass on the mask and 0 elsewhere (repeated mask entries count
   repeatedly); out = (I, mu, var) */
int pucfem_mixing_index_w(void* ctx, const double* c, const double* w, double* out3);

/* ---- measurement ------------------------------------------------------------------ */
/* HIP-event timing of each kernel class (bench.py roofline): the events are taken by each launch's own
   dispatch, on the stream the kernel runs on.  on: 0 off, 1 every class, 2 every class but 5-7 (the
   classes with a share of the step; the roofline kernel is the largest of them) */
int pucfem_timing_enable(void* ctx, int32_t on);
/* kernel classes: 0 = multigrid Chebyshev smoother on the finest level (k_cheb), 1 = CG SpMV+direction
   (k_cg_dir), 2 = CG update (k_cg_upd), 3 = gradient projection (k_grad_proj), 4 = semi-Lagrangian (k_sl),
   5 = multigrid residual on the finest level (k_resid), 6 = restriction from the finest level,
   7 = prolongation to the finest level (k_transfer), 8 = the semi-Lagrangian second pass (k_sl_slow: general
   locate and rank count of the rows off the lattice fast path), 9 = the viscous Chebyshev step over the whole
   grid (k_vcheb), 10 = two finest-level smoothing steps (k_cheb_pair), 11 = divergence (k_div), 12 = two
   viscous Chebyshev steps on the face rows (k_vcheb_pair), 13 = viscous right-hand side and warm start
   (k_visc_prep), 14 / 15 = the pressure projection's multi-dot and combination passes (k_mdot2, k_pcomb) */
int pucfem_timing_get(void* ctx, int32_t kclass, double* total_ms, int64_t* launches,
                      double* bytes_per_launch);
int pucfem_sync(void* ctx);
/* cumulative launches and algorithmic bytes of one kernel class (the classes of pucfem_timing_get) over EVERY
   launch since the context's creation, timed or not (launches of a solve after its convergence, which do no
   work, are taken back): with the timed launches' rate, bench.py weighs the classes over the whole timed
   window.  Measurement only. */
int pucfem_class_counters(void* ctx, int32_t kclass, int64_t* launches, double* bytes);
/* cumulative counters of the calling thread / context since its creation (bench.py's step roofline):
   launches = kernel launches issued by this thread through the library; bytes = the algorithmic bytes of
   the context's launched kernels (each vector counted once per row it is read or written, stored operators
   per entry; kernels launched after their solve had converged, which do no work, are not counted) --
   the HBM floor of the work the steps did.  Replaces nothing in the reference (measurement only). */
int pucfem_counters(void* ctx, int64_t* launches, double* bytes);
/* micro-benchmark of the pressure CG's SpMV + direction kernel (k_cg_dir; the round-1 roofline kernel,
   kept for A/B measurements) on the pressure operator: variant 0 plain loop, 1 unrolled, 2 non-temporal,
   3 unrolled + non-temporal; average ms/launch */
int pucfem_bench_dir(void* ctx, int32_t variant, int32_t nblocks, int32_t iters, double* ms_out);
/* timing of one kernel on the context's finest-level data (bench.py's roofline cross-check):
   kernel 0 = k_cheb general step (fp32 V-cycle), 1 = k_resid, 2 = k_cg_dir<1> of the pressure CG.
   ms_batch: `iters` back-to-back launches between two events, per launch; ms_each: the average of
   per-launch dispatch events (hipExtLaunchKernelGGL); bytes: algorithmic bytes per launch.
   kernel + 16*F: F untimed launches of a coarse level's smoother follow every timed launch
   (ms_batch then includes them; ms_each still times the kernel's own launches) */
int pucfem_bench_kernel(void* ctx, int32_t kernel, int32_t iters, double* ms_batch, double* ms_each, double* bytes);
/* timing of the pressure projection's two basis passes outside the step (tools/proj_bench.py), at the first
   pressure solve's current basis size m and in the step's form (a pending direction, the right-hand side formed in
   the multi-dot pass); the context's state is not changed (outputs go to scratch).  Each kernel is launched once
   untimed, then `iters` times between two events: out6[0] / [1] = ms per launch of k_mdot2<m> / k_pcomb<m'>,
   [2] / [3] = their algorithmic bytes per launch, [4] = m, [5] = m' = min(m, capacity - 1).  Needs a multigrid
   context with a pressure projection basis, else PUCFEM_EINVAL; meant to be called after steps. */
int pucfem_proj_probe(void* ctx, int32_t iters, double* out6);
/* timing and pixel bookkeeping of pucfem_raster's kernel (tools/raster_bench.py; arguments as pucfem_raster,
   the image stays on the device): out4[0] = ms per launch of `iters` back-to-back launches between two events
   (after one untimed launch), [1] = pixels no triangle holds, [2] = pixels the lattice locator answers with the
   inner test of the first macro face listed for the pixel (one lattice cell tested; the rest take its general
   search; 0 with the record locator), [3] = bytes of the image */
int pucfem_raster_probe(void* ctx, int32_t nfields, const int32_t* fields, int32_t width, int32_t height,
                        const double* window4, int32_t iters, double* out4);
/* sizes of the internal operators: out[0]=N, [1]=T, [2]=nnz(P), [3]=nnz(Pp), [4]=n_own,
   [5]=n_ghost, [6]=padded SELL entries (P), [7]=padded SELL entries (Pp), [8]=n_pairs, [9]=n_dirichlet,
   [10]=storage flags (bit 0: P has int16 columns, bit 1: Pp has int16 columns, bit 2: the finest
   V-cycle operator is stored in fp16), [11]=multigrid levels (0: none) */
int pucfem_info(void* ctx, int64_t* out12);
/* which code path the step runs (for tests of the production path): out[0] viscous solve (0 dense inverse,
   1 one-workgroup CG, 2 multi-kernel CG), [1] pressure solve (0 dense, 1 one-workgroup CG, 2 multi-kernel
   Jacobi CG, 3 multigrid-preconditioned CG), [2] projection bases re-seeded so far, [3] / [4] current
   basis sizes of the two pressure solves, [5] extrapolation order of the viscous warm start in use,
   [6] projection basis capacity (0: off), [7] bit 0: the operators are lattice stencils on the face
   interiors (pucfem_params.assembled = 0 with a hierarchy; clear: every row is a stored SELL row),
   bit 1: the semi-Lagrangian point location uses the lattice locator (else per-triangle records),
   bit 7: pressure PCG iterations ran in the single-reduction (Chronopoulos-Gear) form */
int pucfem_path_info(void* ctx, int64_t* out8);
/* multi-rank data flow of the last step: out[0] dye values this rank received in the wide halo before
   the semi-Lagrangian step, out[1] the values a full all-gather of the dye would have received
   (N - n_own), out[2] values all-reduced for the StokesFood tracers (3 x tracers), out[3] the data-path
   backend (0 none: single rank, 1 LocalComm test backend, 2 RCCL) */
int pucfem_comm_info(void* ctx, int64_t* out4);
/* Communicator self-test on the library stream (RCCL's first contact in a run): sum and max all-reduces
   of 8 values and one grouped ring exchange (rank -> rank + 1; a send to itself on one rank), checked
   against their known results: out = (|sum err|, |max err|, |recv err|, backend 1 LocalComm / 2 RCCL).
   The replaced reference sites are the dot products inside the np.linalg.solve calls
   (StokesColor.py:544-545, 555, 569), which become all-reduced CG dots on multi-rank runs. */
int pucfem_comm_selftest(void* ctx, double* out4);
/* unit probe of the single-reduction PCG's scalar kernel (k_cgcg_coef, the multi-rank pressure solve of
   StokesColor.py:555,569): one launch on the context's stream from the given 8 reduced values red8, <b, b> bb,
   the state sc5 (alpha, beta, gamma of the last iteration, alpha_(it-1), gamma_(it-1)) and iteration `it`;
   ctl_out[2] receives the control word ({0, 0} continue, {1, k} converged at iteration k, {2, it} maxit,
   {3, it} not finite), sc_out5 the new state.  Test infrastructure (tests/test_gpu_parity.py). */
int pucfem_cgcg_coef_probe(void* ctx, const double* red8, double bb, const double* sc5, double tol2, int32_t it,
                           int32_t maxit, double rho0, int32_t* ctl_out, double* sc_out5);
/* cumulative data-path traffic of this rank's communicator (zeros without one): out[0] all-reduce calls,
   [1] all-reduced values, [2] point-to-point sends, [3] bytes sent, [4] grouped launches (group_start),
   [5] broadcasts (DESIGN.md §7's per-step counts; measurement only) */
int pucfem_comm_counters(void* ctx, int64_t* out6);
/* The viscous Chebyshev iteration's interval for the Jacobi-scaled A_visc (StokesColor.py:471-475):
   out2 = [lo, hi], lo = max(1 - R, 1 / max_i a_ii), hi = 1 + R, R the Gershgorin radius.  Every
   eigenvalue lies inside (tests/test_host_assembly.py checks it against scipy's eigensolver). */
int pucfem_visc_interval(void* ctx, double* out2);
/* The pressure multigrid's smoothing interval on one level (0 = coarsest .. levels) of a single-rank context:
   the Chebyshev smoother of D^-1 A runs on [lmax / mg_ratio, lmax] (the np.linalg.solve sites
   StokesColor.py:555,569 it preconditions).  out4 = [lmax in use, the device power iteration's Rayleigh
   quotient (0: estimated on the host), the host 30-step power iteration's quotient on the level's fp64
   operator (computed by this call), the host Gershgorin bound]; lmax = min(Gershgorin, 1.1 x quotient). */
int pucfem_mg_lmax(void* ctx, int32_t level, double* out4);
/* One piece of the pressure multigrid's V-cycle (the preconditioner of the np.linalg.solve sites
   StokesColor.py:555,569) on given vectors, launched by the very members the cycle calls.  Test infrastructure
   (tests/test_gpu_mg_cycle.py compares every piece with an fp64 restatement); not on the step path.
   Vectors are fp64 in caller numbering of their level (0 = coarsest .. levels); they are rounded to the cycle's
   type (fp32 with mg_single, else fp64) on upload.  Only the cycle's scratch buffers are written: a run continues
   bit for bit.  Pieces (level l; unused vectors may be null):
     RESID     out = b - A_l x                                   l >= 1
     SMOOTH0   out = the pre-smoothing (mg_degree steps from a zero guess) for right-hand side b      l >= 1
     SMOOTHX   out = the post-smoothing (mg_post or mg_degree steps) from x for b; no z, no <r, z>    l >= 1
     RESTRICT  out (level l - 1) = R x, x on level l                                                  l >= 1
     PROLONG   out = x + P b, b on level l - 1, x on level l                                          l >= 1
     COARSE    out = the dense coarse solve of b                                                      l == 0
     CYCLE     out = the V-cycle from level l down for b                                              l >= 0
     PRECOND   out = z = M^-1 b as the PCG calls it, rz[0] = the reduced <b, z>                      l == levels
   A built single-rank device context with a multigrid hierarchy: PUCFEM_ESTATE before the build and on a host-only
   context, PUCFEM_EINVAL without a hierarchy, on a multi-rank context, for a piece / level that does not exist or
   a null vector the piece needs. */
enum {
  PUCFEM_MG_RESID = 0,
  PUCFEM_MG_SMOOTH0 = 1,
  PUCFEM_MG_SMOOTHX = 2,
  PUCFEM_MG_RESTRICT = 3,
  PUCFEM_MG_PROLONG = 4,
  PUCFEM_MG_COARSE = 5,
  PUCFEM_MG_CYCLE = 6,
  PUCFEM_MG_PRECOND = 7
};
int pucfem_mg_probe(void* ctx, int32_t piece, int32_t level, const double* b, const double* x, double* out,
                    double* rz);
/* The pressure solves' projected initial guesses (successive right-hand sides, pucfem_params.proj_k; the solves
   replace np.linalg.solve at StokesColor.py:555,569): out4 = [bases re-seeded so far, bases restarted by the guess
   monitor (a projected guess > 50x worse than the best of its basis' last 8), the last projected guess's relative residual
   |b - A x0| / |b| of basis 1 and of basis 2 (0: none yet)]. */
int pucfem_proj_info(void* ctx, double* out4);

/* ---- host-only (no device needed) ---------------------------------------------------- */
/* Red refinement, `levels` times.  Call with xy_out == NULL to get sizes. */
int pucfem_refine(int64_t n_nodes, const double* xy, const int32_t* markers, int64_t n_tris,
                  const int32_t* tris, int32_t levels, int64_t* n_nodes_out, int64_t* n_tris_out,
                  double* xy_out, int32_t* markers_out, int32_t* tris_out);
/* The host-assembled operator of this rank in the CALLER's numbering (rows owned by this rank,
   global column ids).  Call with col == NULL to get nnz.  For CPU tests of the assembly. */
int pucfem_host_get_csr(void* ctx, int32_t op, int64_t* n_rows, int64_t* nnz, int64_t* rowptr,
                        int64_t* col, double* val);
/* Host reference of the lattice face stencils (CPU tests of the index arithmetic and the per-face
   coefficients; single-rank contexts with lattice operators).  Rows of face-interior nodes of the output
   level are written, every other entry of y is NaN.  kind 0: K x, 1: Gx x0 + Gy x1 (x is (N, 2), the
   divergence numerator), 2: S A_visc S x, 3: the level's periodic-merged pressure operator (any level),
   5: prolongation from level-1 into level (x on level-1), 6: restriction from level into level-1.
   Vectors in the caller numbering of their level (level = the multigrid level, 0 = the coarse mesh). */
int pucfem_host_lattice_apply(void* ctx, int32_t level, int32_t kind, const double* x, double* y);
/* Partition plan for (rank, world) computed on a host-only context (pucfem_ctx_create(-1)):
   owned rows (caller numbering) in internal order, then the ghost ids; send lists per peer.
   Sizes first (arrays NULL), then contents. */
int pucfem_host_partition(void* ctx, int32_t rank, int32_t world, int64_t* n_own, int64_t* n_ghost,
                          int64_t* owned, int64_t* ghosts, int32_t* ghost_owner,
                          int64_t* n_send, int64_t* send_ids, int32_t* send_peer);

/* The swimmer surface's edge list (see "swimmer loads"): n edges, per edge its triangle, its end nodes a -> b (the
   triangle's local edge) and the opposite node, caller numbering, in ascending (triangle, local edge) order.  Every
   array NULL to get n.  Works on a host-only context once a mesh is uploaded. */
int pucfem_host_surface_edges(void* ctx, int64_t* n, int32_t* tri, int32_t* a, int32_t* b, int32_t* opp);

#ifdef __cplusplus
}
#endif
#endif /* PUCFEM_H */
