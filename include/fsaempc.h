/*
 * fsaempc.h -- C ABI of libfsaempc.so: the MI355X (gfx950) batched LTV-MPC QP path.
 *
 * This library is the drop-in for the ONE hot path of kerry-he/fsae-mpc:
 *   linearise -> condense -> build QP -> solve -> post-solve, for many independent instances.
 * Every entry point cites the reference interface it replaces (paths relative to the
 * reference repo).  Plain C types only; device entry points take raw device pointers and a
 * hipStream_t passed as void*.  All matrices are column-major (MATLAB layout); a batch is
 * stacked instance-major (instance b starts at b * <elements per instance>).
 *
 * Return value of every function: 0 on success, <0 = FSAEMPC_ERR_* (argument / runtime
 * errors -- the analogue of the MEX gateway's mexErrMsgTxt, never a solver outcome).
 * Solver outcomes are per-instance exit flags with qpOASES semantics
 * (optimizers/matlab/qpOASES/qpOASES.m:43-47): 0 solved, 1 iteration limit,
 * -1 internal error, -2 infeasible, -3 unbounded.  Whatever the flag, x / fval / lambda carry the last iterate
 * (NaN only where the data already held one): the reference's loop keeps driving on what the solver returned
 * (main.m:163-175).  -3 is returned only when the objective follows a diverging iterate to -infinity.
 */
#ifndef FSAEMPC_H
#define FSAEMPC_H

#ifdef __cplusplus
extern "C" {
#endif

#define FSAEMPC_ERR_ARG      (-1)  /* bad argument (null pointer, negative size, NaN in data ...) */
#define FSAEMPC_ERR_DIM      (-2)  /* unsupported dimension (nV > FSAEMPC_MAX_NV) */
#define FSAEMPC_ERR_HIP      (-3)  /* HIP runtime error (see fsaempc_last_error) */
#define FSAEMPC_ERR_NODEVICE (-4)  /* no gfx950 device / code object not loadable: there is NO CPU fallback */
#define FSAEMPC_ERR_WORKSPACE (-5) /* workspace too small */
#define FSAEMPC_ERR_SOLVER   (-6)  /* a call whose contract is "solve or fail" could not solve (fsaempc_seq_equality) */

#define FSAEMPC_MAX_NV 196   /* 12 column tiles of 16 + up to 4 border columns (config 5: dynamic N = 80, nV = 164) */

#define FSAEMPC_MODEL_KINEMATIC 0  /* mpc/ltv/kinematic/ltvmpc_kinetmatic_curvilinear.m */
#define FSAEMPC_MODEL_DYNAMIC   1  /* mpc/ltv/dynamic/ltvmpc_dynamic_curvilinear.m */

/* Solver options; the reference passes none (=> qpOASES defaults, qpOASES_options.m:180-213).
 * fsaempc_qp_default_opts fills the defaults of this build. */
typedef struct {
  double tol;        /* strict relative KKT tolerance (default 1e-8) */
  double tol_loose;  /* fall-back KKT tolerance = the specified 1e-6 */
  double tol_x;      /* Newton-decrement test on the affine direction (default 1e-7) */
  double inf_bound;  /* |bound| >= inf_bound is treated as infinite (default 1e9; covers the
                        reference's +-1e10 fillers, kinematic_state_constraints.m:38-39) */
  int    max_iter;   /* interior-point iteration limit (default 100) */
  int    polish;     /* 1 (default): active-set polish to the vertex-exact point an active-set solver returns;
                        accepted only if it is a KKT point, otherwise the interior-point iterate is kept */
} fsaempc_qp_opts;

void fsaempc_qp_default_opts(fsaempc_qp_opts* o);

/* Problem descriptor of one batched solve.
 * shared_HA != 0: H and A are given once and shared by all `batch` instances (the reference
 * API's own multi-column form, qpOASES.m:65-67); otherwise H and A are stacked per instance. */
typedef struct {
  int nV;        /* number of variables */
  int nC;        /* number of general constraint rows (0 => bounds-only form, qpOASES.m:34-35) */
  int batch;     /* number of independent QPs */
  int shared_HA;
} fsaempc_qp_desc;

/* Bytes of device workspace fsaempc_qp_solve_batch_device needs for `desc`. */
long long fsaempc_qp_workspace_bytes(const fsaempc_qp_desc* desc);

/*
 * Replaces: [x,fval,exitflag,iter,lambda] = qpOASES(H,g,A,lb,ub,lbA,ubA)
 *           optimizers/matlab/qpOASES/qpOASES.m:22-23 (call sites
 *           mpc/ltv/kinematic/ltvmpc_kinetmatic_curvilinear.m:52,
 *           mpc/ltv/dynamic/ltvmpc_dynamic_curvilinear.m:52), batched.
 * Device pointers, asynchronous on `stream`.  H: nV*nV, g: nV, A: nC*nV (column-major),
 * lb/ub: nV, lbA/ubA: nC per instance; +-inf allowed in bounds.
 * Outputs: x nV, fval 1, exitflag 1 (int), iter 1 (int) per instance; lambda (nV+nC per
 * instance, bounds first, >=0 lower side / <=0 upper side) may be NULL.
 * `workspace` must hold fsaempc_qp_workspace_bytes(desc) bytes.
 */
int fsaempc_qp_solve_batch_device(const fsaempc_qp_desc* desc,
                                  const double* H, const double* g, const double* A,
                                  const double* lb, const double* ub, const double* lbA, const double* ubA,
                                  const fsaempc_qp_opts* opts,
                                  double* x, double* fval, int* exitflag, int* iter, double* lambda,
                                  void* workspace, long long workspace_bytes, void* stream);

/* Optional per-instance diagnostics of a batched solve -- the analogue of qpOASES' sixth output `auxOutput`
 * (optimizers/matlab/qpOASES/qpOASES.m:55-62).  Device arrays of `batch` entries, each may be NULL.
 *   kkt:      relative KKT residual (max of stationarity, primal feasibility, complementarity) of the returned point as
 *             the solver measured it.  Exit flag 0 covers both iterates converged to opts->tol and the fall-back iterate
 *             that met opts->tol_loose; this value tells them apart.
 *   polished: > 0 the active-set refinement was accepted (the returned point is the vertex, value = attempts used),
 *             0 not attempted, < 0 rejected (the interior-point iterate is returned). */
typedef struct {
  double* kkt;
  int* polished;
  const double* x_init;   /* optional INPUT (device, nV per instance; NULL = none): starting point of the interior-point iteration,
                             clamped to the bounds -- the primal part of what qpOASES' auxInput.x0 / a hot start carries.  Slacks and
                             multipliers start as always.  Measured on closed-loop QPs (shifted previous plan vs cold):
                             profiles/round3/warm_start_ab.json */
  const int* difficulty;  /* optional INPUT (device, one int per instance; NULL = none): the caller's estimate of each instance's solve
                             effort, any monotone measure -- e.g. the iteration count of the same car's QP one MPC period earlier.
                             Batches of more than 256 instances are launched hardest-looking first (one wavefront / workgroup per
                             QP is dispatched in order, so a batch ends with its last-started instances); without this array the
                             library ranks by the number of rows and bounds that exclude x = 0.  Only the launch order depends on it,
                             never a result (profiles/round3/launch_order.txt) */
} fsaempc_qp_aux;

int fsaempc_qp_solve_batch_device_aux(const fsaempc_qp_desc* desc,
                                      const double* H, const double* g, const double* A,
                                      const double* lb, const double* ub, const double* lbA, const double* ubA,
                                      const fsaempc_qp_opts* opts,
                                      double* x, double* fval, int* exitflag, int* iter, double* lambda,
                                      const fsaempc_qp_aux* aux,
                                      void* workspace, long long workspace_bytes, void* stream);

/* Same call on host pointers: copies to the device, solves, copies back, synchronises.
 * This is what a MEX gateway calls (mex/qpOASES.cpp); validates like the original gateway
 * (NaN anywhere / Inf in H,g,A => FSAEMPC_ERR_ARG).  The _device entries cannot inspect device data before the launch: an
 * instance with NaN / Inf in H, g, A (or NaN in a bound) returns exitflag -1 with iter = 0 and x = clamp(0, lb, ub); the other
 * instances of the batch are unaffected. */
int fsaempc_qp_solve_batch(const fsaempc_qp_desc* desc,
                           const double* H, const double* g, const double* A,
                           const double* lb, const double* ub, const double* lbA, const double* ubA,
                           const fsaempc_qp_opts* opts,
                           double* x, double* fval, int* exitflag, int* iter, double* lambda);

/* ---- qpOASES_sequence: handle-based solves of a sequence of QPs -------------------------------
 * Replaces optimizers/matlab/qpOASES/qpOASES_sequence.m:23 ('i'), :39 ('h'), :51 ('m'), :76 ('c')
 * (commented call sites ltvmpc_kinetmatic_curvilinear.m:44-50, live cleanup main.m:193).  Host pointers,
 * one QP per call (k columns of g/lb/ub/lbA/ubA => k QPs, as in qpOASES.m:65-67).  The handle owns device copies of H and
 * A (uploaded by 'i' and 'm' only), the solver workspace and the per-call vectors, so a hot start transfers (3 nV + 2 nC) k
 * doubles and the results, nothing else.  Every call is a COLD interior-point solve: same results as a qpOASES hot start, but
 * the previous iterate is not used as a starting point (measured: 3-10 % fewer iterations per QP, profiles/round3/warm_start_ab.json,
 * DESIGN.md 6d; fsaempc_qp_aux.x_init of the batched entries takes a starting point for callers that want one).
 * fsaempc_seq_equality is qpOASES_sequence.m:64 ('e'): the equality-constrained QP fixed by the working set of the handle's
 * last 'i'/'h'/'m' solve (first column; a side is in the set iff its multiplier has the side's sign and exceeds the side's
 * slack -- on a refined vertex: iff the multiplier is non-zero); it returns FSAEMPC_ERR_SOLVER when that QP has no solution and
 * leaves the handle as is.
 * Errors mirror the gateway: unknown handle => FSAEMPC_ERR_ARG "Invalid handle to QP instance!", changed
 * dimensions => FSAEMPC_ERR_ARG "QP dimensions must be constant during a sequence!". */
int fsaempc_seq_init(int nV, int nC, const double* H, const double* g, const double* A,
                     const double* lb, const double* ub, const double* lbA, const double* ubA, int k,
                     const fsaempc_qp_opts* opts, int* handle,
                     double* x, double* fval, int* exitflag, int* iter, double* lambda);      /* 'i' */
int fsaempc_seq_hotstart(int handle, int nV, int nC, const double* g, const double* lb, const double* ub,
                         const double* lbA, const double* ubA, int k, const fsaempc_qp_opts* opts,
                         double* x, double* fval, int* exitflag, int* iter, double* lambda);  /* 'h' */
int fsaempc_seq_hotstart_matrices(int handle, int nV, int nC, const double* H, const double* g, const double* A,
                                  const double* lb, const double* ub, const double* lbA, const double* ubA, int k,
                                  const fsaempc_qp_opts* opts,
                                  double* x, double* fval, int* exitflag, int* iter, double* lambda);  /* 'm' */
int fsaempc_seq_equality(int handle, int nV, int nC, const double* g, const double* lb, const double* ub,
                         const double* lbA, const double* ubA, int k, const fsaempc_qp_opts* opts,
                         double* x, double* lambda, int* workingSetB, int* workingSetC);        /* 'e' */
int fsaempc_seq_cleanup(int handle);                                                         /* 'c' */

/* ---- sensitivities: vector-Jacobian product of the batched QP solve ---------------------------
 * The reference's route to sensitivities is qpOASES_sequence('e', ...) (optimizers/matlab/qpOASES/qpOASES_sequence.m:64): the
 * equality QP of the current working set solved for new right-hand sides (fsaempc_seq_equality above, one QP on a handle).  This is
 * its batched, on-device counterpart in reverse mode.  For a QP solved by fsaempc_qp_solve_batch_device(_aux) with lambda and
 * polished, the working set is the solver's refinement rule (a side is in it iff its multiplier has the side's sign and exceeds the
 * side's slack).  With A^ = the working rows plus unit rows of the active bounds, each cotangent column xbar (and fbar) solves
 *     H w + A^' mu = xbar + fbar (H x + g),   A^ w = 0
 * and gives gbar = -w + fbar x, bbar = mu on the active side of each working-set constraint (0 elsewhere),
 * Hbar = -(w x' + x w')/2 + fbar x x'/2, Abar row r = lambda_r w' - mu_r x' for working rows (0 otherwise).
 * Per-instance status: 0 vertex (polished > 0), solved, every working-set multiplier above tol (1 + |lambda|_inf); 1 as 0 with a
 * weakly active side kept (one-sided derivative); 2 the forward returned the interior-point iterate (polished <= 0), working set
 * of the rule used anyway; -1 system singular / not solved to a relative KKT residual of 1e-12 (zeros); -2 forward exit flag != 0
 * (zeros).  Results depend only on the instance's own data. */
#define FSAEMPC_VJP_OK 0
#define FSAEMPC_VJP_WEAK 1
#define FSAEMPC_VJP_INTERIOR 2
#define FSAEMPC_VJP_SINGULAR (-1)
#define FSAEMPC_VJP_FORWARD_FAILED (-2)

/* Cotangents in and out (device arrays, instance-major; column c of instance b starts at (b k + c) * <size>). */
typedef struct {
  const double* xbar;  /* IN  k * nV per instance (required) */
  const double* fbar;  /* IN  k per instance (NULL = 0) */
  double* gbar;        /* OUT k * nV (required) */
  double* lbbar;       /* OUT k * nV (NULL = not wanted) */
  double* ubbar;       /* OUT k * nV */
  double* lbAbar;      /* OUT k * nC */
  double* ubAbar;      /* OUT k * nC */
  double* Hbar;        /* OUT k * nV * nV, column-major (not with shared_HA) */
  double* Abar;        /* OUT k * nC * nV, column-major nC x nV as A (not with shared_HA) */
} fsaempc_qp_vjp_io;

/* Bytes of device workspace fsaempc_qp_vjp_batch_device needs for `desc` (at most 512 instances are in flight). */
long long fsaempc_qp_vjp_workspace_bytes(const fsaempc_qp_desc* desc);

/* x, lambda (nV + nC), exitflag, polished (may be NULL: every instance counts as unrefined, status 2) are the outputs of the forward
 * solve of the same data; opts (may be NULL) supplies inf_bound and the weak-multiplier tolerance tol.  k >= 1 columns.  Asking for
 * Hbar or Abar with desc->shared_HA returns FSAEMPC_ERR_ARG.  status: batch ints.  Asynchronous on `stream`. */
int fsaempc_qp_vjp_batch_device(const fsaempc_qp_desc* desc, int k,
                                const double* H, const double* g, const double* A,
                                const double* lb, const double* ub, const double* lbA, const double* ubA,
                                const double* x, const double* lambda, const int* exitflag, const int* polished,
                                const fsaempc_qp_opts* opts, const fsaempc_qp_vjp_io* io, int* status,
                                void* workspace, long long workspace_bytes, void* stream);

/* ---- LTV-MPC step (QP construction + solve + post-solve) ---------------------------------- */

/* Track spline table: the `kappa` closure of main.m:18 as data.  xP,yP: M x 4 column-major. */
typedef struct {
  int M;
  double dl;
  const double* xP;   /* device pointers for *_device entry points, host pointers otherwise */
  const double* yP;
} fsaempc_spline;

#define FSAEMPC_INT_DEFAULT (-1)  /* the one the reference driver calls: RK2 kinematic, RK4 dynamic (ltvmpc_*.m:38) */
#define FSAEMPC_INT_EULER 0       /* mpc/ltv/{kinematic,dynamic}/euler_*_curvilinear.m:24-30 */
#define FSAEMPC_INT_RK2   1       /* rk2_*_curvilinear.m:25-50 (midpoint rule) */
#define FSAEMPC_INT_RK4   2       /* rk4_*_curvilinear.m:25-59 */

typedef struct {
  int model;     /* FSAEMPC_MODEL_* */
  int N;         /* horizon steps (main.m:36) */
  int batch;
  double dt;     /* main.m:37 */
  int integrator; /* FSAEMPC_INT_*: lineariser of the continuous model (the reference keeps all three per model) */
} fsaempc_ltv_desc;

int fsaempc_ltv_nx(int model);            /* 5 / 7 */
int fsaempc_ltv_nV(int model, int N);     /* 2N + slack count */
int fsaempc_ltv_nC(int model, int N);     /* 6N / 20N */

/*
 * Replaces the QP construction of ltvmpc_*_curvilinear.m:38-41 (rk2/rk4 lineariser,
 * sequential_integration.m, *_state_constraints.m, generate_qp.m), batched, on device.
 * Inputs per instance: x0 nx, x_ref nx*N, x_lin nx*N, u_lin 2*N.
 * Outputs per instance: H,g,A,lb,ub,lbA,ubA as for the solver; pred = [A_bar*x0 + d_bar] (nx*N),
 * Bt (nx*N x nV, B_bar with slack columns), qconst 1.  Bt/pred/qconst may be NULL.
 */
int fsaempc_ltv_build_qp_batch_device(const fsaempc_ltv_desc* desc, const fsaempc_spline* sp,
                                      const double* x0, const double* x_ref, const double* x_lin, const double* u_lin,
                                      double* H, double* g, double* A, double* lb, double* ub, double* lbA, double* ubA,
                                      double* pred, double* Bt, double* qconst, void* stream);

/* Bytes of device workspace for fsaempc_ltv_step_batch_device (QP tensors + solver workspace). */
long long fsaempc_ltv_workspace_bytes(const fsaempc_ltv_desc* desc);

/*
 * Replaces [u_opt,x_opt,QP,exitflag,fval,slack_opt] = ltvmpc_*_curvilinear(x0,x_ref,kappa,dt,x_lin,u_lin,QP)
 * (ltvmpc_kinetmatic_curvilinear.m:1, ltvmpc_dynamic_curvilinear.m:1), batched, on device.
 * Outputs per instance: u_opt 2N, x_opt nx*N, slack ns, fval 1 (incl. the constant, :60), exitflag, iter.
 */
int fsaempc_ltv_step_batch_device(const fsaempc_ltv_desc* desc, const fsaempc_spline* sp,
                                  const double* x0, const double* x_ref, const double* x_lin, const double* u_lin,
                                  const fsaempc_qp_opts* opts,
                                  double* u_opt, double* x_opt, double* slack, double* fval, int* exitflag, int* iter,
                                  void* workspace, long long workspace_bytes, void* stream);

/* Same step with the per-instance diagnostics of the solve (fsaempc_qp_aux: achieved KKT residual, refinement outcome);
 * aux may be NULL.  The reference's drivers hand back the solver object `QP` at this position of their output list
 * (ltvmpc_*.m:1); a batched build has no such object, the diagnostics take its place. */
int fsaempc_ltv_step_batch_device_aux(const fsaempc_ltv_desc* desc, const fsaempc_spline* sp,
                                      const double* x0, const double* x_ref, const double* x_lin, const double* u_lin,
                                      const fsaempc_qp_opts* opts,
                                      double* u_opt, double* x_opt, double* slack, double* fval, int* exitflag, int* iter,
                                      const fsaempc_qp_aux* aux,
                                      void* workspace, long long workspace_bytes, void* stream);

/* ---- sensitivities of the LTV-MPC step (the step's counterpart of qpOASES_sequence('e'), qpOASES_sequence.m:64) ----
 * With x_lin, u_lin fixed the build depends on x0 and x_ref only through pred = Abar x0 + d_bar, g_u = 2 Phi' Qbar (pred - x_ref),
 * row shifts of lbA / ubA that are affine in the predicted state of the row's own step, and qconst; H, A, lb, ub do not move.
 * fsaempc_ltv_affine_maps_batch_device writes, per instance, Abar (nx N x nx, column-major: d pred / d x0) and Crow (nC x nx,
 * column-major): lbA_r and ubA_r move by -Crow_r . pred_k, k the step of row r (rows 0..4N: k = r mod N; kinematic rows 4N..6N:
 * (r - 4N) mod N; dynamic slip rows 4N..8N: ((r - 4N) mod 2N) / 2; dynamic tyre rows: (r - 8N) / 12).  Same linearisation and step
 * coefficients as the build. */
int fsaempc_ltv_affine_maps_batch_device(const fsaempc_ltv_desc* desc, const fsaempc_spline* sp, const double* x_lin, const double* u_lin,
                                         double* Abar, double* Crow, void* stream);

/* The fused step that also returns the multipliers of its QP (lambda: nV + nC per instance, layout of fsaempc_qp_solve_batch_device):
 * the forward of fsaempc_ltv_step_vjp_batch_device.  Same outputs and workspace as fsaempc_ltv_step_batch_device_aux. */
int fsaempc_ltv_step_batch_device_lambda(const fsaempc_ltv_desc* desc, const fsaempc_spline* sp,
                                         const double* x0, const double* x_ref, const double* x_lin, const double* u_lin,
                                         const fsaempc_qp_opts* opts, double* u_opt, double* x_opt, double* slack, double* fval,
                                         int* exitflag, int* iter, double* lambda, const fsaempc_qp_aux* aux,
                                         void* workspace, long long workspace_bytes, void* stream);

/* Cotangents of the step (device arrays; column c of instance b at (b k + c) * <size>). */
typedef struct {
  const double* ubar;  /* IN  k * 2N   cotangent of u_opt (NULL = 0) */
  const double* xbar;  /* IN  k * nx N cotangent of x_opt (NULL = 0) */
  const double* sbar;  /* IN  k * ns   cotangent of slack (NULL = 0) */
  const double* fbar;  /* IN  k        cotangent of fval  (NULL = 0) */
  double* x0bar;       /* OUT k * nx   (required) */
  double* xrefbar;     /* OUT k * nx N (NULL = not wanted) */
} fsaempc_ltv_vjp_io;

long long fsaempc_ltv_step_vjp_workspace_bytes(const fsaempc_ltv_desc* desc, int k);

/* VJP of the step in x0 and x_ref (x_lin, u_lin fixed).  u_opt, slack, lambda, exitflag, polished (may be NULL) are the outputs of
 * fsaempc_ltv_step_batch_device_lambda (with fsaempc_qp_aux.polished) on the same inputs.  The QP is rebuilt by the build kernel,
 * its VJP is fsaempc_qp_vjp_batch_device, and a chain kernel applies the transposed affine maps.  status: the QP VJP's status
 * (FSAEMPC_VJP_*); a negative status gives zeros.  k >= 1 columns; asynchronous on `stream`. */
int fsaempc_ltv_step_vjp_batch_device(const fsaempc_ltv_desc* desc, const fsaempc_spline* sp, int k,
                                      const double* x0, const double* x_ref, const double* x_lin, const double* u_lin,
                                      const double* u_opt, const double* slack, const double* lambda, const int* exitflag, const int* polished,
                                      const fsaempc_qp_opts* opts, const fsaempc_ltv_vjp_io* io, int* status,
                                      void* workspace, long long workspace_bytes, void* stream);

/*
 * Exact-linearisation build of the nonlinear MPC step (the NLP of DESIGN.md "Nonlinear MPC: batched SQP") at the inputs u_lin:
 * the states are the rollout x_k = Psi(x_{k-1}, u_k) of the integrator of desc->integrator (x_0 = x0; RK4 is the classical
 * one), step k is linearised exactly at (x_{k-1}, u_k) (Phi(i,i) = Bd_i, true df/dx including the curvature derivative of the
 * track table, true RK4 stage derivatives), and every constraint row is linearised at the rollout state it constrains.
 * Same outputs as fsaempc_ltv_build_qp_batch_device, with one difference: pred receives the rollout x_1..x_N itself.  The QP's
 * variables are still u (not a step), so its affine state offset is pred - Bt(:, 1:2N) u_lin (g = 2 Bt' Qbar (that offset - x_ref)).
 * The reference quirks the LTV build keeps are not applied here.
 */
int fsaempc_nlp_build_qp_batch_device(const fsaempc_ltv_desc* desc, const fsaempc_spline* sp,
                                      const double* x0, const double* x_ref, const double* u_lin,
                                      double* H, double* g, double* A, double* lb, double* ub, double* lbA, double* ubA,
                                      double* pred, double* Bt, double* qconst, void* stream);

/* ---- batched SQP of the nonlinear MPC step --------------------------------------
 * Gauss-Newton SQP with exact linearisation: each sweep builds the exact QP at the current inputs, solves it, and takes the
 * largest step 2^-i (i < trials) that satisfies Armijo on the l1 merit J + rho * |hard violation|_1 (slacks reset to the least
 * value their soft rows need at each trial point); rho >= 1.1 |lambda of the hard rows|_inf.  Instances leave the batch when
 * they are done; each sweep works on a dense sub-batch of the ones still running. */
typedef struct {
  int max_sweeps;    /* sweep limit (default 20) */
  int trials;        /* step lengths 2^0 .. 2^-(trials-1) tried at once, 1..64 (default 8) */
  double tol_step;   /* converged: |u_QP - u|_inf <= tol_step (1 + |u|_inf) ... (default 1e-6) */
  double tol_feas;   /* ... and max hard violation <= tol_feas (default 1e-6) */
  double armijo;     /* eta of phi(a) <= phi(0) - eta a pred (default 1e-4) */
  double rho0;       /* initial penalty (default 1) */
  int warm_start;    /* 1 (default): the QP of each sweep starts at (u, s) of the current iterate (fsaempc_qp_aux.x_init) */
} fsaempc_sqp_opts;

void fsaempc_sqp_default_opts(fsaempc_sqp_opts* o);

/* Optional per-instance outputs of fsaempc_sqp_batch_device (device arrays over the whole batch; each may be NULL). */
typedef struct {
  double* lambda;     /* nV + nC: multipliers of the instance's last QP (layout of fsaempc_qp_solve_batch_device) */
  int* qp_iter;       /* interior-point iterations summed over the instance's QPs */
  double* step_norm;  /* |u_QP - u|_inf of the last sweep */
  double* hard_viol;  /* max hard-row violation of the returned point */
  double* merit;      /* max_sweeps: merit after each sweep (NaN for sweeps not run) */
} fsaempc_sqp_aux;

/* Bytes of device workspace fsaempc_sqp_batch_device needs (QP tensors of the whole batch + solver workspace + SQP state). */
long long fsaempc_sqp_workspace_bytes(const fsaempc_ltv_desc* desc);

/*
 * Solves the nonlinear MPC step of `batch` instances from u_init (2N per instance; x0 nx, x_ref nx*N as for the LTV step).
 * Outputs per instance: u_opt 2N, x_opt nx*N (the rollout of u_opt), slack ns, fval (NLP objective incl. the constant),
 * status, sweeps (QPs solved).  status: 0 converged, 1 sweep limit, 2 no step accepted, -1 / -2 the QP of the last sweep failed
 * with that flag (every other failing flag is reported as -1); for every status but 0 the outputs are the last accepted iterate.
 * Instances never influence each other.  qp_opts / sqp_opts may be NULL (defaults).  The call blocks once per sweep (it reads
 * the number of instances still running); all other work is queued on `stream`.
 */
int fsaempc_sqp_batch_device(const fsaempc_ltv_desc* desc, const fsaempc_spline* sp,
                             const double* x0, const double* x_ref, const double* u_init,
                             const fsaempc_qp_opts* qp_opts, const fsaempc_sqp_opts* sqp_opts,
                             double* u_opt, double* x_opt, double* slack, double* fval, int* status, int* sweeps,
                             const fsaempc_sqp_aux* aux, void* workspace, long long workspace_bytes, void* stream);

/* Status of an instance the caller masked out of fsaempc_sqp_batch_device_m (distinct from the statuses above and from the internal
 * "still running" = 3). */
#define FSAEMPC_SQP_SKIPPED 4

/* Phase times of the last fsaempc_sqp_batch_device call, summed over its sweeps, by HIP events (switch: fsaempc_qp_set_timing;
 * with it on, the call also synchronises after every sweep).  compact = compaction + gather. */
int fsaempc_sqp_get_timing(double* build_ms, double* solve_ms, double* linesearch_ms, double* compact_ms);

/* ---- reference trajectories ---------------------------------------------------------------- */

/*
 * Replaces x_ref = obtain_reference(x, ds, N_s, t, s0, dt, N_t)   (util/obtain_reference.m:1-48; call site
 * main.m:115, commented in the live loop), batched over s0.  plan: the planner vector x (8 values per s-cell:
 * n, mu, x_d, y_d, theta_d, delta, a, delta_d; obtain_reference.m:7-15), t: per-cell traversal times (N_s),
 * s0: `batch` arc-length positions.  Output per instance: x_ref 7 x N_t column-major, row 1 =
 * s0 + mod(idx+rto-idx_1-rto_1, N_s)*ds, rows 2..7 linear interpolation of the six planner states.
 * Device pointers, asynchronous on `stream`.
 */
int fsaempc_obtain_reference_batch_device(const double* plan, double ds, int N_s, const double* t,
                                          const double* s0, double dt, int N_t, int batch,
                                          double* x_ref, void* stream);

/*
 * Replaces the live reference generator of main.m:107-114 (velocity ramp +-10 m/s^2 clipped at target_vel,
 * s_ref = s0 + cumsum(v_ref*dt), all other states 0), batched.  x0: batch x nx, x_ref: batch x (nx x N).
 */
int fsaempc_reference_live_batch_device(int nx, int N, double dt, double target_vel, int batch,
                                        const double* x0, double* x_ref, void* stream);

/* ---- closed loop around the step (main.m:91-179), batched: one car per instance ------------------- */

/*
 * Replaces main.m:93-114 per car: [s,n,mu] = cartesian_to_curvilinear(x(1),x(2),x(3),x_spline,y_spline,dl,x_opt(1))
 * (vehicle_models/cartesian_to_curvilinear.m:17-26, spline/closest_point.m:15-32 with epsilon 0.01), the x0 assembly
 * for the model (:94-98), the lap check s >= L (:101-104, sets finished[b] = 1; 2 = the closest-point search diverged,
 * the car left the track) and the live reference (:107-114).
 * cart: batch x 7 [x,y,theta,x_d,y_d,theta_d,delta]; s_guess: batch (first predicted s of the previous plan).
 * Outputs x0 (batch x nx), x_ref (batch x (nx x N)).
 */
int fsaempc_cl_pre_batch_device(int model, int N, double dt, double target_vel, double L, const fsaempc_spline* sp,
                                const double* cart, const double* s_guess, int batch,
                                double* x0, double* x_ref, int* finished, void* stream);

/*
 * Replaces main.m:163-175 per car: set points v_ref = x_opt(4), delta_ref = x_opt(N_x) from this step's plan, then ten
 * sub-steps of pid_controller (vehicle_models/pid_controller.m; gains main.m:84-88) + integrate_cart_dyn(x, u, dt/10)
 * (vehicle_models/cartesian_dynamic/integrate_cart_dyn.m, f_cart_dyn.m).  cart (batch x 7) and pid (batch x 4:
 * velocity integral / last error, steering integral / last error) are updated in place; cars with finished[b] != 0 or
 * a non-finite set point keep their state; exitflag (optional) holds a car only for values < -100 (a caller's own marker,
 * never a solver outcome: the reference drives on whatever the solver returned, main.m:163-175); u_last (optional,
 * batch x 2) = last actuator rates.
 */
int fsaempc_cl_plant_batch_device(int model, int N, double dt, int batch, double* cart, double* pid, const double* x_opt,
                                  const int* finished, const int* exitflag, double* u_last, void* stream);

/*
 * Replaces the hand-over of main.m:122-126 per car: this step's plan (x_new: nx*N, u_new: 2*N) becomes the linearisation
 * point and set-point source of the next step (x_keep, u_keep) when the solve ended with exit flag 0 or 1 (exitflag may
 * be NULL: every finite plan is taken) and the plan is finite; otherwise the car keeps its last good plan and keeps
 * driving on it.  (The reference takes over whatever qpOASES returned; the last iterate of an interior-point method
 * after an abnormal exit need not respect the actuator bounds, hence the deviation.)
 */
int fsaempc_cl_accept_batch_device(int model, int N, int batch, const double* x_new, const double* u_new, const int* exitflag,
                                   double* x_keep, double* u_keep, void* stream);

/* ---- per-instance vehicle, cost and limit parameters ---------------------------------
 * Every constant the reference assigns at the top of its drivers and models (ltvmpc_*_curvilinear.m:20-35, f_curv_*.m,
 * dynamic_tyre_linearise_constraints.m, f_cart_dyn.m, main.m:84-88) as one block of FSAEMPC_NPAR doubles, shared by the batch or
 * given per instance.  The entries without the _p suffix compute with the reference's values compiled in; the _p entries read
 * the block (a NULL block, or NULL values, means the defaults and gives what the entry without the suffix gives).
 * Fixed in both: the 5 exp(-x_d / 5) regularisation of the dynamic model, the plant's + 0.01, the 12 polygon sides and the
 * pseudo-infinite 1e10 fillers.
 * A block that cannot describe a car -- a non-finite entry; M, IZ, LF + LR or Q_TERMINAL <= 0; a negative weight, slack cost
 * or limit (V_MIN may be any finite value) -- does not stop the batch: the build writes NaN into that instance's g, so the solve
 * returns exit flag -1 with iter = 0 for it (the SQP: status -1), and the plant holds that car. */
#define FSAEMPC_NPAR 32
#define FSAEMPC_P_M            0   /* vehicle mass (280); also the divisor of the tyre rows */
#define FSAEMPC_P_IZ           1   /* yaw inertia (200) */
#define FSAEMPC_P_LF           2   /* centre of gravity to front axle (0.8672) */
#define FSAEMPC_P_LR           3   /* centre of gravity to rear axle (0.6183) */
#define FSAEMPC_P_GRAV         4   /* 9.81 */
#define FSAEMPC_P_PB           5   /* Pacejka B, C, D, E (12.56, 1.38, 1.60, -0.58) */
#define FSAEMPC_P_PC           6
#define FSAEMPC_P_PD           7
#define FSAEMPC_P_PE           8
#define FSAEMPC_P_Q_S          9   /* state weights on s, n, mu (5, 250, 2000) */
#define FSAEMPC_P_Q_N          10
#define FSAEMPC_P_Q_MU         11
#define FSAEMPC_P_Q_TERMINAL   12  /* factor on Q at k = N (10) */
#define FSAEMPC_P_R_ACC        13  /* input weights (10, 10) */
#define FSAEMPC_P_R_STEER      14
#define FSAEMPC_P_R_SOFT0      15  /* slack costs: kinematic 1e8 (entry 15 only); dynamic 1e8, 1e6, 1e6, 1e4 */
#define FSAEMPC_P_R_SOFT1      16
#define FSAEMPC_P_R_SOFT2      17
#define FSAEMPC_P_R_SOFT3      18
#define FSAEMPC_P_U_ACC_MAX    19  /* input boxes (10, 0.4) */
#define FSAEMPC_P_U_STEER_MAX  20
#define FSAEMPC_P_DELTA_MAX    21  /* hard steering-angle row (0.4) */
#define FSAEMPC_P_N_MAX        22  /* track half-width of the soft track rows (0.75) */
#define FSAEMPC_P_V_MIN        23  /* hard speed row (0) */
#define FSAEMPC_P_ALAT_MAX     24  /* kinematic: soft lateral-acceleration rows (5) */
#define FSAEMPC_P_SLIP_MAX     25  /* dynamic: soft slip-angle rows (0.1) */
#define FSAEMPC_P_ELL_LONG     26  /* dynamic: axes of the tyre ellipse behind the 12-gon rows (10.0, 9.163) */
#define FSAEMPC_P_ELL_LAT      27
#define FSAEMPC_P_PID_KP_V     28  /* plant only: velocity loop gain and force limit (16000, 2800) */
#define FSAEMPC_P_PID_MAX_F    29
#define FSAEMPC_P_PID_KP_D     30  /* plant only: steering loop gain and rate limit (80, 0.8) */
#define FSAEMPC_P_PID_MAX_DRATE 31

typedef struct {
  const double* values;   /* device; FSAEMPC_NPAR doubles, or batch * FSAEMPC_NPAR instance-major */
  int per_instance;       /* 0: one block shared by the batch; 1: one block per instance */
} fsaempc_ltv_params;

/* Host: the FSAEMPC_NPAR defaults of `model` (the values listed above) into out. */
int fsaempc_ltv_default_params(int model, double* out);

/* The entries above with a parameter block after `sp`.  Workspaces are those of the entries without the suffix.
 * fsaempc_ltv_step_batch_device_p covers the three step forms: lambda and aux may each be NULL.
 * The plant takes its own block (batch-shared or per car), so the controller's model and the car may differ. */
int fsaempc_ltv_build_qp_batch_device_p(const fsaempc_ltv_desc* desc, const fsaempc_spline* sp, const fsaempc_ltv_params* par,
                                        const double* x0, const double* x_ref, const double* x_lin, const double* u_lin,
                                        double* H, double* g, double* A, double* lb, double* ub, double* lbA, double* ubA,
                                        double* pred, double* Bt, double* qconst, void* stream);
int fsaempc_ltv_step_batch_device_p(const fsaempc_ltv_desc* desc, const fsaempc_spline* sp, const fsaempc_ltv_params* par,
                                    const double* x0, const double* x_ref, const double* x_lin, const double* u_lin,
                                    const fsaempc_qp_opts* opts, double* u_opt, double* x_opt, double* slack, double* fval,
                                    int* exitflag, int* iter, double* lambda, const fsaempc_qp_aux* aux,
                                    void* workspace, long long workspace_bytes, void* stream);
int fsaempc_nlp_build_qp_batch_device_p(const fsaempc_ltv_desc* desc, const fsaempc_spline* sp, const fsaempc_ltv_params* par,
                                        const double* x0, const double* x_ref, const double* u_lin,
                                        double* H, double* g, double* A, double* lb, double* ub, double* lbA, double* ubA,
                                        double* pred, double* Bt, double* qconst, void* stream);
int fsaempc_sqp_batch_device_p(const fsaempc_ltv_desc* desc, const fsaempc_spline* sp, const fsaempc_ltv_params* par,
                               const double* x0, const double* x_ref, const double* u_init,
                               const fsaempc_qp_opts* qp_opts, const fsaempc_sqp_opts* sqp_opts,
                               double* u_opt, double* x_opt, double* slack, double* fval, int* status, int* sweeps,
                               const fsaempc_sqp_aux* aux, void* workspace, long long workspace_bytes, void* stream);
int fsaempc_cl_plant_batch_device_p(int model, int N, double dt, int batch, const fsaempc_ltv_params* par, double* cart, double* pid,
                                    const double* x_opt, const int* finished, const int* exitflag, double* u_last, void* stream);
/* fsaempc_sqp_batch_device_p with a skip mask (device, batch ints; NULL: the entry above, launch for launch).  An instance with
 * skip[i] != 0 never enters a sub-batch: no QP is built or solved for it, and its outputs are what the start of the call wrote --
 * u_opt the clamped u_init, x_opt its rollout, the minimal slacks, fval of that point, sweeps 0, qp_iter 0 -- with status
 * FSAEMPC_SQP_SKIPPED.  The other instances are bit for bit what they are without the mask.  With every instance masked the call
 * returns after its first read. */
int fsaempc_sqp_batch_device_m(const fsaempc_ltv_desc* desc, const fsaempc_spline* sp, const fsaempc_ltv_params* par,
                               const double* x0, const double* x_ref, const double* u_init, const int* skip,
                               const fsaempc_qp_opts* qp_opts, const fsaempc_sqp_opts* sqp_opts,
                               double* u_opt, double* x_opt, double* slack, double* fval, int* status, int* sweeps,
                               const fsaempc_sqp_aux* aux, void* workspace, long long workspace_bytes, void* stream);

/* ---- lap report: what main.m:196-228 prints, accumulated per car on the device ----------
 * One record of FSAEMPC_NMETRIC doubles per car, instance-major, zeroed by the caller before the first step.  A step is "recorded"
 * for a car while it drives (finished[b] == 0 when fsaempc_cl_pre_batch_device returned). */
#define FSAEMPC_NMETRIC 16
#define FSAEMPC_M_STEPS          0   /* MPC steps solved while the car drove: main.m:203,216's i - 1 (lap time = STEPS dt) */
#define FSAEMPC_M_STATUS         1   /* 0 driving, 1 finished (s >= L, main.m:102-104), 2 lost; latched: a latched record is final */
#define FSAEMPC_M_N_VIOL_INT     2   /* sum (|n| - N_MAX) dt over recorded n with |n| > N_MAX (main.m:204,217) */
#define FSAEMPC_M_N_VIOL_MAX     3   /* max (|n| - N_MAX) over the same steps, 0 if none (main.m:205,218) */
#define FSAEMPC_M_N_ABS_MAX      4   /* largest |n| recorded (main.m:101, n_list) */
#define FSAEMPC_M_ABNORMAL       5   /* steps with exitflag != 0 (main.m:209,222) */
#define FSAEMPC_M_OBJ_SUM        6   /* fval summed over steps with exitflag == 0 and no slack in use (main.m:198,210,223) */
#define FSAEMPC_M_OBJ_CNT        7   /* number of those steps */
#define FSAEMPC_M_SLACK_N_CNT    8   /* steps with slack[0] in use (main.m:132,211,224) */
#define FSAEMPC_M_SLACK_TYRE_CNT 9   /* steps with the tyre slack in use: dynamic slack[3], kinematic slack[0] (main.m:133,214,227) */
#define FSAEMPC_M_ELL_VIOL_INT   10  /* sum (e - 1) dt over steps with e > 1, e = (Fcr / (M ELL_LAT))^2 + (a / ELL_LONG)^2 (main.m:180-182,199,212,225) */
#define FSAEMPC_M_ELL_VIOL_MAX   11  /* max (e - 1) over the same steps, 0 if none (main.m:213,226) */
#define FSAEMPC_M_ITER_SUM       12  /* solver iterations summed: the batch's stand-in for cpu_time (main.m:131,206,219) */
#define FSAEMPC_M_ITER_MAX       13  /* most iterations of one step (main.m:208,221) */
#define FSAEMPC_M_S_START        14  /* s at the first recorded step */
#define FSAEMPC_M_S_LAST         15  /* s at the last recorded step */

/*
 * One call per MPC period, after the plant; asynchronous on `stream`.  Per car, with finished[b] as the pre-step left it:
 *   record already latched (STATUS != 0): nothing is touched;
 *   finished[b] == 2: STATUS = 2, nothing else (x0 is a placeholder);
 *   otherwise n = x0[1] enters N_ABS_MAX and, if |n| > N_MAX, the track violation; then finished[b] == 1: STATUS = 1 and nothing
 *   else of this step (main.m:101 stores n_list(i) before the break of :102-104, and :204 sums over it);
 *   a driving car records the rest: STEPS, S_START / S_LAST = x0[0], the exit flag, iter, fval, the slacks and the ellipse value.
 * "In use" is slack > slack_tol (a NaN slack is not in use).  a = u_drive[0], the first acceleration of the plan the car drives on
 * (2N per car: u_keep after fsaempc_cl_accept_batch_device); Fcr is the rear lateral force of vehicle_models/curvilinear_dynamic/
 * f_curv_dyn.m:32-53 (x_d + 5 exp(-x_d / 5) in the slip angle) at the post-plant state cart (batch x 7).
 * par: NULL (the reference's constants), one shared block or one per car; N_MAX, ELL_LONG, ELL_LAT, M, LF, LR, GRAV, PB..PE are read.
 * A block that cannot describe a car leaves that car's record untouched.  slack: 1 (kinematic) or 4 (dynamic) per car.
 * FSAEMPC_ERR_ARG before any launch: a NULL pointer (par excepted), an unknown model, N < 1, batch < 0, dt not finite or <= 0,
 * slack_tol negative or NaN.  batch == 0 succeeds without a launch.
 */
int fsaempc_cl_metrics_batch_device(int model, int N, double dt, double slack_tol, int batch, const fsaempc_ltv_params* par,
                                    const double* x0, const int* finished, const int* exitflag, const int* iter, const double* fval,
                                    const double* slack, const double* u_drive, const double* cart, double* metrics, void* stream);

/* Batch summary of `batch` records on the HOST (no device needed), summed in index order: the same bits on every call. */
#define FSAEMPC_NREPORT 20
#define FSAEMPC_R_CARS_DRIVING    0   /* cars by STATUS */
#define FSAEMPC_R_CARS_FINISHED   1
#define FSAEMPC_R_CARS_LOST       2
#define FSAEMPC_R_LAP_MEAN        3   /* STEPS dt over the finished cars (main.m:203); NaN if none finished.  Lost cars are not in it */
#define FSAEMPC_R_LAP_MIN         4
#define FSAEMPC_R_LAP_MAX         5
#define FSAEMPC_R_STEPS           6   /* recorded steps of all cars: the denominator of the three percentages and of ITER_MEAN */
#define FSAEMPC_R_ABNORMAL_PCT    7   /* main.m:209 pooled over all recorded steps; NaN without a recorded step */
#define FSAEMPC_R_SLACK_N_PCT     8   /* main.m:211 */
#define FSAEMPC_R_SLACK_TYRE_PCT  9   /* main.m:214 */
#define FSAEMPC_R_OBJ_MEAN        10  /* main.m:210: OBJ_SUM / OBJ_CNT pooled; NaN if no step counted */
#define FSAEMPC_R_N_VIOL_INT_MEAN 11  /* main.m:204 as the mean over the cars with STEPS > 0 (NaN if none) ... */
#define FSAEMPC_R_N_VIOL_INT_MAX  12  /* ... and the largest of one car (0 for an empty batch) */
#define FSAEMPC_R_N_VIOL_MAX      13  /* main.m:205: largest of all cars */
#define FSAEMPC_R_ELL_VIOL_INT_MEAN 14 /* main.m:212, as N_VIOL_INT_MEAN */
#define FSAEMPC_R_ELL_VIOL_INT_MAX 15
#define FSAEMPC_R_ELL_VIOL_MAX    16  /* main.m:213 */
#define FSAEMPC_R_ITER_MEAN       17  /* main.m:206 with iterations for cpu_time; NaN without a recorded step */
#define FSAEMPC_R_ITER_MAX        18  /* main.m:208 */
#define FSAEMPC_R_N_ABS_MAX       19  /* largest |n| of all cars */
/* metrics_host: batch x FSAEMPC_NMETRIC (host); out: FSAEMPC_NREPORT doubles.  FSAEMPC_ERR_ARG: NULL (metrics_host may be NULL
 * with batch == 0), batch < 0, dt not finite or <= 0. */
int fsaempc_cl_report(const double* metrics_host, int batch, double dt, double* out);

/* ---- s-domain plans: a speed-profile planner and the loop that tracks a plan -----------
 * The reference's controller is meant to track a planned trajectory: main.m:20 computes an s-domain plan with
 * dynamic_minimum_time_planner (IPOPT; not part of this build) and main.m:115 resamples it in time with obtain_reference.
 * fsaempc_plan is that table as data; fsaempc_plan_profile_batch_device fills one with a stand-in: a quasi-steady-state
 * minimum-time speed profile on the centre line (n = 0, no lateral dynamics); fsaempc_plan_raceline_batch_device further down
 * chooses a line first. */
typedef struct {          /* a planner table as obtain_reference.m:7-15 reads it */
  const double* table;    /* device; N_s * 8 per plan (n, mu, x_d, y_d, theta_d, delta, a, delta_d per cell) */
  const double* t;        /* device; N_s per plan: per-cell traversal times (dynamic_minimum_time_planner.m:73-83) */
  int N_s; double ds;     /* cells per lap, cell length = L / N_s; cell i sits at s_i = i * ds */
  int per_instance;       /* 0: one plan shared by the batch; 1: one plan per instance, instance-major */
} fsaempc_plan;
#define FSAEMPC_PLAN_MAX_NS 4096   /* the planner keeps curvature and speed of a plan in LDS: 16 bytes per cell */

/*
 * Fills n_plans plans of N_s cells (table: n_plans * N_s * 8, t: n_plans * N_s; ds = L / N_s) for the track `sp` of length L.
 * Per cell: k = kappa(s_i), K = max(|k|, 1e-12), vlat = min(v_cap, sqrt(A_lat / K)); from the first cell of least vlat one forward
 * pass v_i = min(v_i, sqrt(v_p^2 + 2 a_x(v_p, K_p) ds)) over the lap and one backward pass with the successor in place of the
 * predecessor.  Limits by model: kinematic A_lat = grip ALAT_MAX, a_x = grip U_ACC_MAX; dynamic A_lat = grip ELL_LAT,
 * a_x = min(U_ACC_MAX, grip ELL_LONG X(min(v^2 K / A_lat, 1))), X the first-quadrant boundary of the 12-gon of the tyre rows
 * (dynamic_tyre_linearise_constraints.m:18-23).  Table: n = mu = y_d = 0, x_d = v, theta_d = v k, delta = atan((LF + LR) k),
 * a = (v_next^2 - v^2) / (2 ds), t = ds / v, delta_d = (delta_next - delta) / t, indices cyclic.
 * par: NULL (defaults), one shared block (n_plans must be 1) or n_plans blocks (per_instance).  A block that cannot describe a car
 * gives that plan NaN in every entry; the other plans are unaffected.
 * FSAEMPC_ERR_ARG before any launch: N_s < 2 or > FSAEMPC_PLAN_MAX_NS; v_cap, grip or L not finite or <= 0; grip > 1; n_plans < 1;
 * a shared block with n_plans > 1.
 */
int fsaempc_plan_profile_batch_device(int model, const fsaempc_spline* sp, double L, const fsaempc_ltv_params* par,
                                      int n_plans, int N_s, double v_cap, double grip,
                                      double* table, double* t, void* stream);

/*
 * obtain_reference (util/obtain_reference.m:1-48, main.m:115) on a plan, batched over s0, in the state layout of the model:
 * x_ref is nx x N column-major per instance; dynamic: the seven rows of obtain_reference.m:41-47; kinematic: rows
 * [s, n, mu, hypot(x_d, y_d), delta] (main.m:95's rule for x0).  The walk over the cells advances at most N_s cells per horizon
 * step, and it ends at the first cell it meets whose time is zero, negative or not finite: from that horizon step on the car's rows
 * are NaN (so is every row after a step that would circle the lap).  Never a hang, never a read outside the table.
 * A non-finite s0 is walked from 0 (finite placeholder rows).
 */
int fsaempc_plan_reference_batch_device(int model, const fsaempc_plan* plan, const double* s0, double dt, int N, int batch,
                                        double* x_ref, void* stream);   /* x_ref: nx x N per instance, model layout */

/*
 * fsaempc_cl_pre_batch_device with the live ramp of main.m:107-114 replaced by main.m:115: same frame transform, x0 assembly, lap
 * check and out-of-race rule, then x_ref from the plan at the car's own s (one kernel).  plan->per_instance: one plan per car.
 */
int fsaempc_cl_pre_plan_batch_device(int model, int N, double dt, double L, const fsaempc_spline* sp, const fsaempc_plan* plan,
                                     const double* cart, const double* s_guess, int batch,
                                     double* x0, double* x_ref, int* finished, void* stream);

/* ---- a minimum-curvature racing line for the s-domain plans ----------------------
 * The lateral offset n(s) of the line from the centre line is a uniform periodic cubic B-spline with N_c control points c (knot
 * spacing L / N_c), sampled at the N_s cells of a plan: cell i, q = i N_c / N_s, j = floor(q), u = q - j, weights
 * [(1-u)^3, 3u^3 - 6u^2 + 4, -3u^3 + 3u^2 + 3u + 1, u^3] / 6 on c_{j-1} .. c_{j+2} (cyclic).  The line minimises the summed squared
 * second difference of its points p_i = c_i + n_i nu_i (centre point, unit left normal: curvilinear_to_cartesian.m:16-26) over c
 * with |c_j| <= w: the weights are non-negative and sum to one, so the whole line stays within +-w.  That is the bounds-only QP
 * min 1/2 c'Hc + g'c, H = 2 ds G'G, g = 2 ds G'd (G_i c + d_i: the second difference at cell i over ds^2), solved by
 * fsaempc_qp_solve_batch_device_s (nC = 0, n_slack = 0, one H for the batch).  Minimum curvature, not minimum time. */
#define FSAEMPC_LINE_MAX_NS 2048   /* the profile on a line keeps curvature, speed and length of a cell in LDS: 24 bytes per cell */
#define FSAEMPC_LINE_MIN_NC 8      /* N_c: FSAEMPC_LINE_MIN_NC .. FSAEMPC_MAX_NV, and N_s >= 2 N_c (H is then cyclic-banded) */

/*
 * H (N_c * N_c, dense, exactly symmetric, zero beyond cyclic distance 4) and g (N_c) of the line QP of (track, N_s, N_c).
 * Every entry is a sum over cells in ascending order: the same bits on every call.
 * FSAEMPC_ERR_ARG before any launch: N_c < FSAEMPC_LINE_MIN_NC or > FSAEMPC_MAX_NV, N_s < 2 N_c or > FSAEMPC_LINE_MAX_NS, L not
 * finite or <= 0, a null pointer.
 */
int fsaempc_raceline_build_qp_device(const fsaempc_spline* sp, double L, int N_s, int N_c, double* H, double* g, void* stream);

/*
 * fsaempc_plan_profile_batch_device on a line: control points `line` (N_c, shared by the plans, or n_plans * N_c with
 * line_per_plan != 0).  Per cell: n and n' = dn/ds from the basis, kappa of the centre line, a = 1 - n kappa, r = sqrt(a^2 + n'^2),
 * mu = atan(n' / a), length dl = ds r, curvature k = (kappa + (mu_next - mu_prev) / (2 ds)) / r; then the recurrences of
 * fsaempc_plan_profile_batch_device with k for the curvature, the predecessor's dl in the forward and the cell's own dl in the
 * backward pass.  Table: n, mu, x_d = v, y_d = 0, theta_d = v k, delta = atan((LF + LR) k), a = (v_next^2 - v^2) / (2 dl),
 * delta_d = (delta_next - delta) / t, t = dl / v.  All-zero control points give the bits of fsaempc_plan_profile_batch_device.
 * A plan is NaN in every entry if its parameter block cannot describe a car or if a < 0.1 in any cell (the line comes too close
 * to the centre of a corner; NaN control points); the other plans are unaffected.
 * FSAEMPC_ERR_ARG before any launch: the cases of fsaempc_plan_profile_batch_device and of fsaempc_raceline_build_qp_device.
 */
int fsaempc_plan_line_profile_batch_device(int model, const fsaempc_spline* sp, double L, const fsaempc_ltv_params* par,
                                           int n_plans, int N_s, int N_c, const double* line, int line_per_plan,
                                           double v_cap, double grip, double* table, double* t, void* stream);

/*
 * Racing-line plans in one call, asynchronous on `stream`: the line QP, its solve with the bounds of each plan
 * (w_p = N_MAX_p - margin; N_MAX_p: FSAEMPC_P_N_MAX of the plan's block, default 0.75) and the profile on each plan's line.
 * line: n_plans * N_c control points, flag: n_plans exit flags of the QPs (fsaempc_qp_solve_batch_device).  A plan whose flag is
 * not 0 takes the centre line (control points written as zeros); a plan with a bad block, w_p <= 0 or a < 0.1 in a cell is NaN in
 * table, t and line.  opts: NULL = defaults.  workspace: fsaempc_plan_raceline_workspace_bytes(n_plans, N_c) bytes.
 * FSAEMPC_ERR_ARG before any launch: the cases of fsaempc_plan_line_profile_batch_device; margin < 0 or not finite.
 */
long long fsaempc_plan_raceline_workspace_bytes(int n_plans, int N_c);
int fsaempc_plan_raceline_batch_device(int model, const fsaempc_spline* sp, double L, const fsaempc_ltv_params* par,
                                       int n_plans, int N_s, int N_c, double margin, double v_cap, double grip,
                                       const fsaempc_qp_opts* opts, double* line, int* flag, double* table, double* t,
                                       void* workspace, long long workspace_bytes, void* stream);

/* ---- move blocking: held inputs --------------------------------------------------
 * The input is held constant over groups of consecutive horizon steps: block j covers steps start_j .. start_j + len_j - 1 and
 * u_k = v_block(k).  The QP's variables are [v_1 .. v_M; slacks], nV_b = 2 M + ns; its rows stay those of the unblocked problem
 * (nC = 6N / 20N).  With E the (2N + ns) x (2M + ns) matrix that copies v_block(k) to step k, the blocked QP is H_b = E'HE,
 * g_b = E'g, A_b = AE of the unblocked one, with the bounds of each block's first member.  One blocking is shared by the batch.
 * Errors: n_blocks < 1, a length < 1 or a sum other than desc->N give FSAEMPC_ERR_ARG; 2N + ns > FSAEMPC_MAX_NV stays
 * FSAEMPC_ERR_DIM (a long horizon does not become admissible by blocking it).  n_blocks == N is the unblocked problem: the entries
 * hand over to their _p forms and return bitwise what those return. */
typedef struct {
  int n_blocks;      /* M, 1..N */
  const int* len;    /* HOST array of M block lengths, each >= 1, sum == desc->N; shared by the batch */
} fsaempc_ltv_blocking;

/* 2 M + ns (host, no device needed); < 0: FSAEMPC_ERR_ARG */
int fsaempc_ltv_blocked_nV(int model, const fsaempc_ltv_blocking* blk);
/* fsaempc_ltv_build_qp_batch_device_p in blocked sizes (nV_b for nV everywhere: H nV_b^2, g / lb / ub nV_b, A nC x nV_b); Bt is
 * nx N x nV_b and holds the held-input response in the block columns (zeros in the slack columns).  par may be NULL. */
int fsaempc_ltv_build_qp_batch_device_b(const fsaempc_ltv_desc* desc, const fsaempc_spline* sp, const fsaempc_ltv_params* par,
                                        const fsaempc_ltv_blocking* blk,
                                        const double* x0, const double* x_ref, const double* x_lin, const double* u_lin,
                                        double* H, double* g, double* A, double* lb, double* ub, double* lbA, double* ubA,
                                        double* pred, double* Bt, double* qconst, void* stream);
long long fsaempc_ltv_workspace_bytes_b(const fsaempc_ltv_desc* desc, const fsaempc_ltv_blocking* blk);
/* The fused step (the _p form: lambda and aux may each be NULL).  u_opt is returned EXPANDED to 2N, the held values, so what
 * consumes a plan (fsaempc_cl_accept_batch_device, the plant, the next linearisation point) works unchanged; x_opt = pred + Bt_b z;
 * slack and fval (constant included) as always; lambda has nV_b + nC entries; aux->x_init is in the blocked variables (nV_b).
 * The solve goes through fsaempc_qp_solve_batch_device_s with the model's slack count. */
int fsaempc_ltv_step_batch_device_b(const fsaempc_ltv_desc* desc, const fsaempc_spline* sp, const fsaempc_ltv_params* par,
                                    const fsaempc_ltv_blocking* blk,
                                    const double* x0, const double* x_ref, const double* x_lin, const double* u_lin,
                                    const fsaempc_qp_opts* opts, double* u_opt, double* x_opt, double* slack, double* fval,
                                    int* exitflag, int* iter, double* lambda, const fsaempc_qp_aux* aux,
                                    void* workspace, long long workspace_bytes, void* stream);

/* The batched solve with the caller's count of trailing slack variables.  The solver keeps the 1 / 4 slack columns of an LTV-MPC QP
 * off the matrix cores (a "border"); without a count it recognises them by nV mod 16 or by the row / column signature of the
 * reference's QPs (nC = 3 (nV - 1) or 10 (nV - 4)), which a QP with condensed columns no longer has.  n_slack: 0, 1 or 4 -- the last
 * n_slack variables are the border, the core is padded to a multiple of 16 with dummy variables; negative -- none given, exactly
 * fsaempc_qp_workspace_bytes / fsaempc_qp_solve_batch_device_aux.  Results of a solve do not depend on the count beyond rounding;
 * the workspace size does: size and solve must be given the same count. */
long long fsaempc_qp_workspace_bytes_s(const fsaempc_qp_desc* desc, int n_slack);
int fsaempc_qp_solve_batch_device_s(const fsaempc_qp_desc* desc, int n_slack,
                                    const double* H, const double* g, const double* A,
                                    const double* lb, const double* ub, const double* lbA, const double* ubA,
                                    const fsaempc_qp_opts* opts,
                                    double* x, double* fval, int* exitflag, int* iter, double* lambda,
                                    const fsaempc_qp_aux* aux,
                                    void* workspace, long long workspace_bytes, void* stream);
/* Host only (no device needed): how a QP of this shape is laid out and which kernel solves it.  out[0] = 16-wide column tiles of
 * the matrix-core part, out[1] = border width of the kernel variant (0, 1 or 4), out[2] = the solver's variable count (dummy
 * padding included), out[3] = 1 for the one-wavefront kernel, 0 for the workgroup kernel. */
int fsaempc_qp_layout(const fsaempc_qp_desc* desc, int n_slack, int out[4]);

/* ---- s-varying track corridors -----------------------------------------------------
 * Everywhere else the track's width is the one number FSAEMPC_P_N_MAX.  A corridor gives the two edges as periodic tables over arc
 * length, linear between the cells.  Lookup at any finite s, negative values and values past L included: q = s / ds wrapped into
 * [0, N_w), i = floor(q), u = q - i, value = t[i] + u (t[(i + 1) mod N_w] - t[i]); a constant table returns the constant exactly.
 * A non-finite s, or one of the two cells read where n_lo < n_hi does not hold, gives NaN for both limits of that lookup only.
 * The limits are for the car's reference point: the caller subtracts the half-width of the car.  The tables are the caller's own, or come
 * from cone positions on the device (fsaempc_corridor_from_cones_device below).  The _c entries take `cor` after `blk`; cor == NULL hands over to the entry
 * without a corridor and returns its bits.  Before any launch FSAEMPC_ERR_ARG, with the argument named in fsaempc_last_error: a NULL
 * n_lo or n_hi, N_w < 2, ds not finite or <= 0. */
typedef struct {
  const double* n_lo;   /* device; N_w per corridor: least admissible n (right edge, usually < 0) at s_i = i * ds */
  const double* n_hi;   /* device; N_w per corridor: greatest admissible n (left edge) */
  int N_w; double ds;   /* cells per lap, ds = L / N_w; periodic */
  int per_instance;     /* 0: one corridor for the batch; 1: one per instance / plan, instance-major */
} fsaempc_corridor;

/*
 * The LTV build and the fused step with the corridor in place of N_MAX.  par and blk may each be NULL: blk == NULL (or one step per
 * block) is the build of fsaempc_ltv_build_qp_batch_device_p, otherwise that of fsaempc_ltv_build_qp_batch_device_b; sizes, outputs
 * and errors are theirs.  After the build one more kernel, one thread per (instance, step), overwrites the 2N track-row bounds:
 *   lbA[2N + k] = n_lo(s_k) - pred_n,k        ubA[3N + k] = n_hi(s_k) - pred_n,k
 * with s_k = x_lin[k nx + 0], the point the row's coefficients and kappa are linearised at, and pred_n,k entry 1 of step k of
 * `pred` (required with a corridor).  The 1e10 / -1e10 on the rows' other sides and the matrix A stay.  The first-order term
 * -n_hi'(s) (s_k - s_lin,k) is left out: the stated approximation.  A block's N_MAX is not read.  A NaN limit (see above) sits in
 * that row only; the solve answers -1 with iter = 0 for that instance, and its neighbours are unaffected.  In the fused step the
 * kernel runs between the build and the solve's preparation on `stream`.  Workspace of the step: fsaempc_ltv_workspace_bytes_b
 * (blk given) or fsaempc_ltv_workspace_bytes (blk == NULL); the corridor needs none.
 * The exact NLP build, the SQP, the affine maps and the VJPs have no corridor form.
 */
int fsaempc_ltv_build_qp_batch_device_c(const fsaempc_ltv_desc* desc, const fsaempc_spline* sp, const fsaempc_ltv_params* par,
                                        const fsaempc_ltv_blocking* blk, const fsaempc_corridor* cor,
                                        const double* x0, const double* x_ref, const double* x_lin, const double* u_lin,
                                        double* H, double* g, double* A, double* lb, double* ub, double* lbA, double* ubA,
                                        double* pred, double* Bt, double* qconst, void* stream);
int fsaempc_ltv_step_batch_device_c(const fsaempc_ltv_desc* desc, const fsaempc_spline* sp, const fsaempc_ltv_params* par,
                                    const fsaempc_ltv_blocking* blk, const fsaempc_corridor* cor,
                                    const double* x0, const double* x_ref, const double* x_lin, const double* u_lin,
                                    const fsaempc_qp_opts* opts, double* u_opt, double* x_opt, double* slack, double* fval,
                                    int* exitflag, int* iter, double* lambda, const fsaempc_qp_aux* aux,
                                    void* workspace, long long workspace_bytes, void* stream);

/*
 * fsaempc_cl_metrics_batch_device against the corridor: N_VIOL_INT and N_VIOL_MAX take v = max(n - n_hi(s), n_lo(s) - n) where
 * v > 0, at the recorded x0 (s = x0[0], n = x0[1]; NaN limits record no violation).  N_ABS_MAX and every other slot are as there.
 * per_instance: one corridor per car.
 */
int fsaempc_cl_metrics_batch_device_c(int model, int N, double dt, double slack_tol, int batch, const fsaempc_ltv_params* par,
                                      const fsaempc_corridor* cor,
                                      const double* x0, const int* finished, const int* exitflag, const int* iter, const double* fval,
                                      const double* slack, const double* u_drive, const double* cart, double* metrics, void* stream);

/*
 * fsaempc_plan_raceline_batch_device inside the corridor (same workspace): only the bounds of the line QP change.  Control point j:
 *   lb_j = max (n_lo(s_i) + margin)        ub_j = min (n_hi(s_i) - margin)
 * over the plan's cells i whose basis touches c_j, floor(i N_c / N_s) in {j - 2, j - 1, j, j + 1} (cyclic), s_i = i L / N_s.  The
 * weights are non-negative and sum to one, so the line is inside the corridor minus the margin at every cell.  Sufficient, not
 * necessary: a pinch is smeared over four knot spacings.  A control point with lb_j >= ub_j (or a NaN limit) gets NaN bounds, so that
 * plan's QP has non-finite data: its flag is -1 (no iteration) and the plan is NaN in table, t and line, like w_p <= 0 there; the other
 * plans are unaffected.  Unlike there, NO plan falls back to the centre line: the centre line may lie outside a corridor (a blocked
 * side, n_hi - margin < 0), so every plan whose flag is not 0 is NaN in table, t and line.  per_instance: one corridor per plan.  A
 * block's N_MAX is not read.
 */
int fsaempc_plan_raceline_batch_device_c(int model, const fsaempc_spline* sp, double L, const fsaempc_ltv_params* par,
                                         const fsaempc_corridor* cor,
                                         int n_plans, int N_s, int N_c, double margin, double v_cap, double grip,
                                         const fsaempc_qp_opts* opts, double* line, int* flag, double* table, double* t,
                                         void* workspace, long long workspace_bytes, void* stream);
/* The bounds alone, as the call above hands them to the solve (lb, ub: n_plans * N_c each, device; NaN where a control point has no
 * box): for inspection and timing.  FSAEMPC_ERR_ARG before the launch: the corridor's cases, a NULL pointer, L not finite or <= 0,
 * N_c, N_s outside the racing line's ranges, n_plans < 1, margin < 0 or not finite. */
int fsaempc_corridor_line_bounds_device(const fsaempc_corridor* cor, double L, int n_plans, int N_s, int N_c, double margin,
                                        double* lb, double* ub, void* stream);

/*
 * The racing line inside the corridor in its exact, cell-wise form (opt-in; the entries above are unchanged).  The offset at cell i is
 * n_i = sum_m w_m(u_i) c_{(j_i - 1 + m) mod N_c}, four non-negative weights that sum to one, so the corridor is one general constraint
 * row per cell and the control points are free variables:
 *   lbA_i = n_lo(s_i) + margin  <=  n_i  <=  ubA_i = n_hi(s_i) - margin,        s_i = i L / N_s,        lb_j = -1e10, ub_j = 1e10.
 * The matrix A of the rows (N_s x N_c, column-major; entry (i, k) = w_m(u_i) where k = (j_i - 1 + m) mod N_c, else 0) depends on
 * (N_s, N_c) alone: one A and one H serve the batch (shared_HA), lbA and ubA are per plan.  The QP goes to
 * fsaempc_qp_solve_batch_device_s with nV = N_c, nC = N_s and the slack count always given (0; 4 for N_c > 192, where the last four
 * control points form the border: 13 column tiles are more than the kernels are built for); a shape that solve refuses (column
 * tiles, LDS budget) is refused here with its code and text, before any launch.  Where the point boxes above smear a pinch over four knot spacings and are
 * conservative even in a constant band, this form uses every cell's own width; control points may lie outside the corridor.  The
 * stated approximation: the line is inside the corridor at the N_s cells, not between them, and the speed profile does not know the
 * corridor.  A cell whose lookup is NaN, or where lbA_i < ubA_i does not hold (n_hi - n_lo <= 2 margin), gets NaN for both bounds:
 * that plan's QP has non-finite data, its flag is -1 (no iteration) and the plan is NaN in table, t and line; the other plans are
 * unaffected.  As in the _c entry NO plan falls back to the centre line: every plan whose flag is not 0 is NaN in table, t and line.
 * cor is required; per_instance: one corridor per plan.  A block's N_MAX is not read.
 * row_lambda: NULL, or n_plans * N_s (device): the multipliers of the cell rows in the solver's sign convention (>= 0 where n_i sits
 * on lbA_i, <= 0 on ubA_i, 0 where the corridor does not bind); no other output depends on whether it is given.
 * workspace: fsaempc_plan_raceline_cells_workspace_bytes(n_plans, N_s, N_c) bytes, carved as
 *   H | A | g, lb, ub (n_plans x N_c each) | lbA, ubA (n_plans x N_s each) | fval | iter | lambda (n_plans x (N_c + N_s)) | the solver's own;
 * every element read is written by the call, nothing relies on a zeroed workspace.
 * FSAEMPC_ERR_ARG before any launch: cor == NULL, the corridor's cases, the cases of fsaempc_plan_raceline_batch_device_c;
 * FSAEMPC_ERR_WORKSPACE: workspace too small.  The size function answers FSAEMPC_ERR_ARG / FSAEMPC_ERR_DIM (< 0) for such shapes.
 */
long long fsaempc_plan_raceline_cells_workspace_bytes(int n_plans, int N_s, int N_c);
int fsaempc_plan_raceline_cells_batch_device(int model, const fsaempc_spline* sp, double L, const fsaempc_ltv_params* par,
                                             const fsaempc_corridor* cor,
                                             int n_plans, int N_s, int N_c, double margin, double v_cap, double grip,
                                             const fsaempc_qp_opts* opts, double* line, int* flag, double* table, double* t,
                                             double* row_lambda, void* workspace, long long workspace_bytes, void* stream);
/* The rows alone, as the call above hands them to the solve (A: N_s * N_c, written once; lbA, ubA: n_plans * N_s each, device; NaN
 * where a cell has no room): for inspection and timing, the counterpart of fsaempc_corridor_line_bounds_device, with its errors. */
int fsaempc_corridor_line_rows_device(const fsaempc_corridor* cor, double L, int n_plans, int N_s, int N_c, double margin,
                                      double* A, double* lbA, double* ubA, void* stream);

/* ---- a minimum-time racing line --------------------------------------------------
 * What the reference's planners are for (minimum_time_planner.m, dynamic_minimum_time_planner.m: the line that minimises the lap
 * time), approximated on the quasi-steady-state profile of fsaempc_plan_line_profile_batch_device: the lap time of a line is
 * T(c) = sum_i t_i of that profile, a function of the control points c through the line's length and curvature per cell, and it is
 * lowered by projected, H-preconditioned gradient steps from the minimum-curvature line.  What it is not: the reference's optimal
 * control problem.  The speed is still the quasi-steady-state profile (y_d = 0: no lateral dynamics, no yaw dynamics, no tyre
 * model), the line is searched in the B-spline's N_c control points inside a box, no IPOPT: a fixed number of steps, each no worse
 * than the last, from one start -- a local improvement, not a certified minimum. */
#define FSAEMPC_MINLAP_MAX_NS 1024   /* the lap-gradient kernel keeps eight doubles and the two win flags of a cell in LDS: 68 bytes per cell */
#define FSAEMPC_MINLAP_MAX_RHO 16    /* candidates per plan and iteration */

/*
 * T (n_plans) and grad = dT/dc (n_plans * N_c) of the lines `line`, inputs as fsaempc_plan_line_profile_batch_device.  The forward
 * arithmetic is that entry's, so T is the sum of its t (to the rounding of the sum: each lane adds its cells i = lane, lane + 64, ..
 * in ascending order, then the wave adds the 64 partial sums in a butterfly).  The gradient is the adjoint of the profile: the two
 * passes are undone in reverse order along the branches the forward run took (which argument won each min; the polygon edge and
 * the U_ACC_MAX / y = 1 branches of the longitudinal limit; |k| against 1e-12; the corner speed against v_cap), then the cell's
 * curvature, length and heading offset, then the basis.  T is piecewise smooth in c: where two arguments of a min tie, grad is the
 * one-sided derivative of the branch taken.  Every grad_j is a sum over its cells in ascending order: the same bits on every call.
 * A plan that fsaempc_plan_line_profile_batch_device makes NaN has T = NaN and a NaN gradient; the other plans are unaffected.
 * FSAEMPC_ERR_ARG before any launch: the cases of fsaempc_plan_line_profile_batch_device; N_s > FSAEMPC_MINLAP_MAX_NS.
 */
int fsaempc_plan_line_lapgrad_batch_device(int model, const fsaempc_spline* sp, double L, const fsaempc_ltv_params* par,
                                           int n_plans, int N_s, int N_c, const double* line, int line_per_plan,
                                           double v_cap, double grip, double* T, double* grad, void* stream);

/*
 * Minimum-time plans in one call, asynchronous on `stream`, with no host read inside: the start, then `iters` iterations, then the
 * table of the final control points by the path of fsaempc_plan_line_profile_batch_device.
 *   start      c_init == NULL: fsaempc_plan_raceline_batch_device (the minimum-curvature line).  c_init (n_plans * N_c, device):
 *              those control points, no solve, every flag 0.
 *   boxes      lo == hi == NULL: +-(N_MAX_p - margin), as in fsaempc_plan_raceline_batch_device.  lo, hi (n_plans * N_c each, device,
 *              both or neither; from fsaempc_corridor_line_bounds_device for instance): the box of every control point, for the
 *              initial QP and every step; margin and the block's N_MAX are then not read.  A plan with lo_j < hi_j false anywhere has
 *              flag -1 and is NaN; with boxes no plan falls back to the centre line (every plan whose flag is not 0 is NaN).
 *   iteration  per plan p and rho_j (rho: n_rho values on the HOST, 1 .. FSAEMPC_MINLAP_MAX_RHO, finite and > 0):
 *              d_pj = argmin 1/2 d'H d + (grad_p / rho_j)'d, lo_p - c_p <= d <= hi_p - c_p, with the H of
 *              fsaempc_raceline_build_qp_device -- one H for all n_plans * n_rho instances of fsaempc_qp_solve_batch_device_s, `opts`
 *              as given; candidates clamp(c_p + d_pj, lo_p, hi_p); their lap times and gradients from one launch of the
 *              lap-gradient kernel, each with its plan's block; the least finite T among the candidates whose QP flag is 0 (first
 *              index on ties) replaces the incumbent if strictly smaller, with its gradient.  A NaN plan never moves.
 * Outputs: line (n_plans * N_c) the final control points, flag (n_plans) of the initial QPs, table / t of the final line (bit for
 * bit fsaempc_plan_line_profile_batch_device on `line`), lap_hist (n_plans * (iters + 1), non-increasing in every finite row:
 * [p * (iters + 1)] is the start's T), step_hist (n_plans * iters: the index of the rho taken, -1 = stayed; may be NULL when
 * iters = 0).  With iters = 0 and neither boxes nor c_init line, flag, table and t are fsaempc_plan_raceline_batch_device's bits.
 * workspace: fsaempc_plan_minlap_workspace_bytes(n_plans, N_c, n_rho) bytes (< 0: FSAEMPC_ERR_ARG for such shapes); every element
 * read is written by the call.
 * FSAEMPC_ERR_ARG before any launch: the cases of fsaempc_plan_raceline_batch_device; N_s > FSAEMPC_MINLAP_MAX_NS; iters < 0; n_rho
 * outside 1 .. FSAEMPC_MINLAP_MAX_RHO; a rho that is not finite and > 0; lo without hi or hi without lo; a null pointer.
 * FSAEMPC_ERR_WORKSPACE: workspace too small (the code every entry of this library answers that with).
 */
long long fsaempc_plan_minlap_workspace_bytes(int n_plans, int N_c, int n_rho);
int fsaempc_plan_minlap_batch_device(int model, const fsaempc_spline* sp, double L, const fsaempc_ltv_params* par,
                                     int n_plans, int N_s, int N_c, double margin, double v_cap, double grip,
                                     const fsaempc_qp_opts* opts, int iters, const double* rho, int n_rho,
                                     const double* c_init, const double* lo, const double* hi,
                                     double* line, int* flag, double* table, double* t, double* lap_hist, int* step_hist,
                                     void* workspace, long long workspace_bytes, void* stream);

/* ---- track corridors from cone positions ---------------------------------------------
 * The tables of an fsaempc_corridor from the two rows of cones that mark the track, on the device and batched: n_corridors cone
 * maps (P noisy maps of one track, say) give n_corridors corridors, in exactly the layout fsaempc_corridor reads with
 * per_instance = 1 (or 0 for one).  One 256-thread workgroup per corridor.  Per side (left, right):
 *   1. Projection of every cone.  A cone with a non-finite coordinate is absent (maps of different sizes are padded with NaN).  The
 *      coarse start is the nearest of the 4M samples s = (j + 0.5) dl / 4, the first minimum in ascending j; then the Newton
 *      iteration of spline/closest_point.m (first over second derivative of the squared distance), until a step with
 *      |delta| <= 1e-10 has been applied, at most 30 iterations.  A cone is unprojected and dropped if the second derivative is
 *      <= 0, anything becomes non-finite, a step exceeds dl, or the limit is hit.  n is the offset along the unit left normal at the
 *      foot point; a cone with |n| > reach is dropped as a stray.  s is wrapped into [0, L).
 *   2. Order.  The kept cones are sorted by (s, input index); the edge is the closed polyline through them in that order.
 *   3. Cells.  Cell i is at s_i = i (L / N_w); p_i, T_i, N_i are the spline point, unit tangent and unit left normal there.  j is
 *      the last kept cone with s_j <= s_i (the last cone overall, shifted by -L, when there is none), j + 1 its cyclic successor,
 *      d = c_{j+1} - c_j.  t = ((p_i - c_j) . T_i) / (d . T_i); if d . T_i > 0 does not hold, t = (s_i - s_j) / (s_{j+1} - s_j)
 *      with the arc lengths unwrapped.  A t outside [-1e-9, 1 + 1e-9] counts the cell as off its segment; t is clamped to [0, 1]
 *      and edge_i = (c_j + t d - p_i) . N_i.  With one kept cone the edge is that cone's n in every cell, with none NaN.
 *   4. Tables.  n_hi[i] = edge_left,i - margin, n_lo[i] = edge_right,i + margin (margin: the car's half-width, say).
 * The nearest-point rule is the contract: a cone nearer to a foreign stretch of track than to its own is attributed to that stretch.
 * info (may be NULL): FSAEMPC_NCONEINFO doubles per corridor, counts summed over both sides --
 *   0 left cones kept, 1 right cones kept, 2 absent, 3 unprojected, 4 beyond reach, 5 cells off their segment,
 *   6 cells where n_lo < n_hi does not hold (a NaN cell counts), 7 least n_hi - n_lo over the cells (NaN if any cell is NaN).
 * One corridor's result does not depend on the others of the batch, bit for bit.  Asynchronous on `stream`; no workspace.
 * FSAEMPC_ERR_ARG before any launch, with the argument named in fsaempc_last_error: a NULL pointer (a side's pointer may be NULL
 * only with count 0; info may be NULL), n_corridors < 1, N_w < 2, L, margin or reach not finite, L <= 0, margin < 0, reach <= 0, a
 * negative count.  FSAEMPC_ERR_DIM: a count above FSAEMPC_CONES_MAX or sp->M above FSAEMPC_CONES_MAX_M. */
#define FSAEMPC_NCONEINFO 8
#define FSAEMPC_CONES_MAX 512     /* cones per side and map */
#define FSAEMPC_CONES_MAX_M 512   /* spline segments */
typedef struct {
  const double* left;    /* device; n_left x 2 doubles per map, xy interleaved */
  const double* right;   /* device; n_right x 2 doubles per map */
  int n_left, n_right;
  int per_corridor;      /* 0: one map for all corridors; 1: one per corridor, corridor-major */
} fsaempc_cones;
int fsaempc_corridor_from_cones_device(const fsaempc_spline* sp, double L, const fsaempc_cones* cones, int n_corridors,
                                       int N_w, double margin, double reach, double* n_lo, double* n_hi, double* info, void* stream);

/* ---- multi-lap closed loop: the lap gate ---------------------------------------------
 * The loop above ends a car's run the first time the pre-step sees s >= L (main.m:102-104).  The gate carries a car over the line
 * instead, up to `laps` laps: it times the crossing inside the period, hands the lap's record over and takes L off every arc
 * length the next step reads.  Everything downstream is periodic in s already.  Opt-in: a loop that never calls the gate is the
 * single-lap loop, and with laps = 1 the gate changes no datum of it. */
#define FSAEMPC_MAX_LAPS 64
#define FSAEMPC_NLAPSTATE 4
#define FSAEMPC_LS_DONE    0   /* laps completed */
#define FSAEMPC_LS_STEPS   1   /* periods on which the gate saw the car driving (finished[b] == 0 on exit) */
#define FSAEMPC_LS_S_PREV  2   /* the car's s at the previous such period, after any wrap */
#define FSAEMPC_LS_T_CROSS 3   /* time of the last crossing, 0 at the start */

/*
 * One call per MPC period, after the pre-step (either flavour) and before the step, on the same stream.  lap_state: batch x
 * FSAEMPC_NLAPSTATE, instance-major, zeroed by the caller before the first period.  Per car, with k = STEPS and s = x0[b][0]:
 *   finished[b] == 2, or finished[b] == 1 with DONE >= laps: nothing is touched;
 *   finished[b] == 1 is a crossing: f = (L - S_PREV) / (s - S_PREV) clamped to [0, 1] if k > 0 and s > S_PREV, else f = 1;
 *     t = (k - 1 + f) dt for k > 0, else 0; lap_times[b][DONE] = t - T_CROSS; T_CROSS = t; DONE += 1.
 *     DONE < laps afterwards, the car drives on: with metrics and lap_records given, metrics[b] goes to lap_records[b][DONE - 1]
 *     with STATUS = 1 and is zeroed; L is taken off x0[b][0] and off column 0 of every stage of x_ref[b] and of the kept plan
 *     x_keep[b] (the next linearisation point and closest-point guess); finished[b] = 0.
 *     DONE == laps, the final crossing: finished[b] stays 1 and the record stays where it is (the metrics entry latches it as it
 *     latches a single lap).
 *   finally, finished[b] == 0 on exit: S_PREV = x0[b][0], STEPS += 1.
 * lap_times: batch x laps, filled with NaN by the caller (a lap not completed stays NaN).  metrics (batch x FSAEMPC_NMETRIC) and
 * lap_records (batch x laps x FSAEMPC_NMETRIC, zeroed by the caller) are both given or both NULL.
 * FSAEMPC_ERR_ARG before any launch: laps outside 1 .. FSAEMPC_MAX_LAPS, nx not 5 or 7, N < 1, batch < 0, dt or L not finite
 * or <= 0, a NULL pointer among x0, x_ref, x_keep, finished, lap_state, lap_times, exactly one of metrics / lap_records.
 * batch == 0 succeeds without a launch.
 */
int fsaempc_cl_lap_gate_batch_device(int nx, int N, double dt, double L, int laps, int batch, double* x0, double* x_ref,
                                     double* x_keep, int* finished, double* lap_state, double* lap_times, double* metrics,
                                     double* lap_records, void* stream);

/* Per-lap summary of `batch` cars on the HOST (no device needed), summed in index order.  lap_times_host: batch x laps as the gate
 * left it.  out: laps x 4 -- per lap the number of cars that completed it (a time that is not NaN), then the mean, min and max of
 * its time over those cars (NaN for a lap nobody completed).  FSAEMPC_ERR_ARG: NULL (lap_times_host may be NULL with batch == 0),
 * batch < 0, laps outside 1 .. FSAEMPC_MAX_LAPS. */
int fsaempc_cl_lap_summary(const double* lap_times_host, int batch, int laps, double* out);

/* ---- closed loop: measurement noise, plan latency and delay compensation --------------
 * The loop above reads the exact state and computes in zero time: the plan solved from the state at t_k steers the plant during
 * [t_k, t_k + dt).  These entries replace nothing in main.m (like the lap gate); they add the two standard imperfections and the
 * standard remedy for the second.  Opt-in: a loop that never calls them is the ideal loop.
 *   observation   x0_obs[i] = x0_true[i] + sigma[i] z_i(seed, id, step) for every state component with sigma[i] > 0; a component with
 *                 sigma[i] == 0 is copied, not added to (keeps -0.0; "noise off" is exact).  A negative or non-finite sigma[i] lives
 *                 on the device and cannot be seen before the launch: it is treated as 0 (copy).
 *   draws         counter based, so a car's noise depends on (seed, id, step, i) only, never on the batch it sits in: Philox4x32-10
 *                 (multipliers 0xD2511F53, 0xCD9E8D57; Weyl constants 0x9E3779B9, 0xBB67AE85), key (seed & 0xffffffff, seed >> 32),
 *                 counter (step, j, id & 0xffffffff, id >> 32) with id = id0 + b; call j = 0 serves components 0 .. 3, call j = 1
 *                 components 4 .. 6.  Words (w0, w1, w2, w3) to normals: u1 = (w0 + 0.5) 2^-32, u2 = (w1 + 0.5) 2^-32,
 *                 r = sqrt(-2 ln u1), z0 = r cos(2 pi u2), z1 = r sin(2 pi u2); (w2, w3) give (z2, z3) the same way.
 *   latency       the plan accepted in period k reaches the plant `delay` periods later: the caller keeps delay + 1 plans, writes
 *                 the plan of period k to slot fsaempc_cl_history_slot(delay, k, 0) after the solve and hands the plant the slot
 *                 fsaempc_cl_history_slot(delay, k, delay); for k < delay that slot holds what the history was filled with.
 *   compensation  x0_mpc = x0_obs rolled over the `delay` periods that pass before this period's plan takes effect:
 *                 x <- Psi(x, u_hist[slot(delay, k, delay - j)][b][stage 1]) for j = 0 .. delay - 1, Psi the rollout step of the NLP
 *                 (fsaempc_nlp_build_qp_batch_device) with desc->integrator and the controller's block `par`.  If an input read or
 *                 a component of the result is not finite, or the block cannot describe a car, x0_mpc[b] = x0_obs[b] bit for bit.
 *                 With compensate == 0 or delay == 0, x0_mpc = x0_obs bit for bit.
 * A car with finished[b] != 0 keeps its state in both outputs.  sigma is in the model's state layout: kinematic
 * [s, n, mu, v, delta], dynamic [s, n, mu, x_d, y_d, theta_d, delta]. */
#define FSAEMPC_CL_MAX_DELAY 4
typedef struct {
  int delay;                 /* whole periods, 0 .. FSAEMPC_CL_MAX_DELAY */
  int compensate;            /* 0 / 1 */
  const double* sigma;       /* device; nx values, or batch * nx (sigma_per_instance); NULL: no noise */
  int sigma_per_instance;
  unsigned long long seed;
  long long id0;             /* id of instance 0 (a shard's first global id) */
} fsaempc_cl_latency;

/* z (batch x nx, instance-major): the nx standard normals of (seed, id0 + b, step), the draws the observation uses.
 * FSAEMPC_ERR_ARG before any launch: nx not 5 or 7, batch < 0, id0 < 0, step < 0 or >= 2^32, z NULL.  batch == 0 succeeds
 * without a launch. */
int fsaempc_cl_noise_batch_device(int nx, int batch, unsigned long long seed, long long id0, long long step,
                                  double* z /* batch x nx */, void* stream);
/* One call per MPC period, after the pre-step (and the lap gate) and before the step, on the same stream: observation and
 * prediction as above, x0_obs and x0_mpc (batch x nx each) written for every car.  The step then takes x0_mpc, and a reference
 * regenerated from it (fsaempc_plan_reference_batch_device with s0 = x0_mpc[:, 0], or fsaempc_reference_live_batch_device); the
 * metrics entry keeps reading x0_true.  finished is optional (NULL: every car drives).  u_hist is read only with compensate and
 * delay >= 1.  x0_obs and x0_mpc must not overlap x0_true or each other.
 * FSAEMPC_ERR_ARG before any launch: what the LTV entries refuse in desc and sp, lat NULL, delay outside
 * 0 .. FSAEMPC_CL_MAX_DELAY, compensate not 0 or 1, step < 0 or >= 2^32, id0 < 0, u_hist NULL with delay > 0, x0_true, x0_obs or
 * x0_mpc NULL.  desc->batch == 0 succeeds without a launch. */
int fsaempc_cl_observe_batch_device(const fsaempc_ltv_desc* desc, const fsaempc_spline* sp, const fsaempc_ltv_params* par,
                                    const fsaempc_cl_latency* lat, long long step, const double* x0_true, const int* finished,
                                    const double* u_hist /* (delay+1) x batch x N x 2, NULL iff delay == 0 */,
                                    double* x0_obs, double* x0_mpc, void* stream);
/* Host: the slot of plan_{step - lag} in a history of delay + 1 plans, (step - lag) mod (delay + 1), lag 0 .. delay.
 * Returns -1 for delay outside 0 .. FSAEMPC_CL_MAX_DELAY, step < 0 or lag outside 0 .. delay. */
int fsaempc_cl_history_slot(int delay, long long step, int lag);

/* ---- closed loop: the state estimator -------------------------------------------------
 * What a driverless car puts between its sensors and its MPC: one extended Kalman filter per car, run once per MPC period between
 * the observation and the step, on the stream, with no host read.  Opt-in like the entries above.  Per car the caller keeps the
 * estimate est_x (nx), its covariance est_P (nx x nx, row-major, symmetric) and two counters est_count[b] = {periods since the last
 * (re-)initialisation, re-initialisations}, zeroed before the first call.  The model is the controller's: Psi is the rollout step of
 * fsaempc_nlp_build_qp_batch_device with desc->integrator and the block `par`, F = dPsi/dx its exact Jacobian (forward mode through
 * the same code, kappa'(s) of the spline table included).  Q = diag(q) per period, R = diag(r), P0 = diag(p0), all in the model's
 * state layout (kinematic [s, n, mu, v, delta], dynamic [s, n, mu, x_d, y_d, theta_d, delta]); q and r for the batch or per car.
 * Component i is measured iff r[i] is finite and >= 0; r[i] = +Inf says "not measured" (a NaN or a negative r[i] lives on the device
 * and cannot be seen before the launch: it is treated as not measured).  Per period and car, in this order:
 *   1 finished    finished[b] != 0: x0_est[b] = z[b] bit for bit, innov = 0, nis = 0 (F_out = I, x_prior = z); est_x, est_P, est_count
 *                 are not written.
 *   2 first       est_count[b][0] == 0: the prior is x- = x_start[b], P- = diag(p0); no prediction, F_out = I.
 *   3 prediction  otherwise: x- = Psi(est_x, u), F = dPsi/dx(est_x, u), M = (F P) F', P- = (M + M') / 2 + diag(q) (exactly symmetric).
 *                 u = u_prev[b * u_stride + 0 .. 1], the input the plant followed in the period just past.
 *   4 reset       if the block cannot describe a car, u is not finite, an entry of x- or P- is not finite, or a P-_ii <= 0 (in a
 *                 first period too): x- = z, P- = diag(p0), est_count[b][1] += 1 and est_count[b][0] restarts.
 *   5 re-basing   if L > 0 and s is measured: x-[0] += L rint((z[0] - x-[0]) / L) (ties to even): the lap gate takes L off the arc
 *                 length before the observation and the estimate follows.  x_prior is x- at this point.
 *   6 update      sequentially for i = 0 .. nx - 1, measured components only: nu_i = z_i - x_i, s_i = P_ii + r_i; unless s_i > 0 the
 *                 component is skipped; c = P[:, i], x_a += c_a nu_i / s_i, P_ab -= (c_a c_b) / s_i (exactly symmetric).
 *                 innov_i = nu_i (0 for an unmeasured component), nis = sum of nu_i^2 / s_i over the components applied.  For
 *                 diagonal R this is the joint Kalman update, and the nu_i are its whitened innovations.
 *   7 check       a non-finite entry of the result, or a P_ii < 0: reset as in 4, then 6 again (every nu is 0: x = z bit for bit).
 *   8 write back  est_x = x0_est = x, est_P = P, est_count[b][0] += 1.
 * F_out is the F of step 2 / 3 whether or not step 4 then discards the prediction.
 * FSAEMPC_ERR_ARG before any launch: what the LTV entries refuse in desc and sp; est, q, r or p0 NULL; L negative or not finite;
 * u_stride < 2; z, x_start, u_prev, est_x, est_P, est_count, x0_est, innov or nis NULL; an output that overlaps another output or
 * an input.  desc->batch == 0 succeeds without a launch. */
typedef struct {
  const double* q;  int q_per_instance;   /* device; nx or batch*nx */
  const double* r;  int r_per_instance;   /* device; nx or batch*nx; +inf = not measured */
  const double* p0;                       /* device; nx */
  double L;                               /* lap length for re-basing s; 0 = none */
} fsaempc_cl_estimator;

int fsaempc_cl_estimate_batch_device(const fsaempc_ltv_desc* desc, const fsaempc_spline* sp, const fsaempc_ltv_params* par,
                                     const fsaempc_cl_estimator* est, const double* z /* batch x nx */, const double* x_start /* batch x nx */,
                                     const double* u_prev, long long u_stride /* doubles between cars */, const int* finished /* optional */,
                                     double* est_x, double* est_P, int* est_count /* batch x 2, zeroed by the caller */,
                                     double* x0_est, double* innov, double* nis /* batch */,
                                     double* F_out /* optional, batch x nx x nx */, double* x_prior /* optional, batch x nx */, void* stream);

/* ---- closed loop: Cartesian sensor models ----------------------------------------------
 * What the car measures is not the curvilinear state the MPC uses but its pose and motion in the Cartesian frame.  The sensor layout
 * is the model's state layout with (s, n, mu) replaced by (X, Y, psi): kinematic [X, Y, psi, v, delta], dynamic
 * [X, Y, psi, x_d, y_d, theta_d, delta].  Out of the plant's 7 Cartesian states c the exact measurement is, as the pre-step assembles
 * x0: kinematic y_true = [c0, c1, c2, sqrt(c3^2 + c4^2), c6], dynamic y_true = c.  Opt-in like the entries above.
 *
 * fsaempc_cl_sense_batch_device: one call per MPC period after the pre-step (and the lap gate), on the same stream.
 *   measurement   y[i] = y_true[i] + sigma[i] z_i(seed, id0 + b, step): the draws, their counter layout and the observation rule of
 *                 fsaempc_cl_observe_batch_device, component i of the sensor layout taking draw i (sigma[i] == 0 copies).
 *   projection    x_proj = the pre-step's frame transform (Newton closest point, n, mu, x0 assembly) of the Cartesian vector y stands
 *                 for -- kinematic (y0, y1, y2, y3, 0, 0, y4), dynamic y -- with the Newton search started at x0_true[b][0]: the
 *                 true arc length selects the lap and the branch, it is not a measurement.  The lap check of the transform is not
 *                 used.  If the transform loses the track (its out-of-race rule): x_proj[b] = x0_true[b] bit for bit and
 *                 proj_lost[b] += 1 (proj_lost: batch ints, zeroed by the caller).
 *   finished      finished[b] != 0: y = y_true and x_proj = x0_true, bit for bit.
 * x_proj is what a loop without a filter drives on, and the filter's first prior and re-initialisation state.
 * FSAEMPC_ERR_ARG before any launch: what the LTV entries refuse in desc and sp; sens or sens->sigma NULL; id0 < 0; step < 0 or
 * >= 2^32; cart, x0_true, y, x_proj or proj_lost NULL; an output that overlaps another output or an input.  desc->batch == 0
 * succeeds without a launch. */
typedef struct {
  const double* sigma;       /* device; nx values (sensor layout), or batch * nx (sigma_per_instance) */
  int sigma_per_instance;
  unsigned long long seed;
  long long id0;             /* id of instance 0 (a shard's first global id) */
} fsaempc_cl_sensors;

int fsaempc_cl_sense_batch_device(const fsaempc_ltv_desc* desc, const fsaempc_spline* sp, const fsaempc_cl_sensors* sens, long long step,
                                  const double* cart /* batch x 7 */, const double* x0_true /* batch x nx */, const int* finished /* optional */,
                                  double* y /* batch x nx */, double* x_proj /* batch x nx */, int* proj_lost /* batch */, void* stream);

/* fsaempc_cl_estimate_cart_batch_device: the filter of fsaempc_cl_estimate_batch_device reading the Cartesian measurement.  What the
 * caller keeps, the model, Q and P0 are those of that entry, in the state layout; est->r is in the sensor layout.  The measurement
 * function is h(x) (vehicle_models/curvilinear_to_cartesian.m:16-28): with the two Bezier tables at s, t = (-Y', X') / |(X', Y')|,
 * h0 = X + n t_x, h1 = Y + n t_y, h2 = atan2(Y', X') + mu, h_i = x_i for i >= 3; H = dh/dx is exact (forward mode through the same
 * code) and differs from the identity in rows and columns 0 .. 2 only.  Steps 1 .. 8 of that entry hold with x_proj in the place of
 * z in steps 1, 4 and 7 and of x_start in step 2, and with
 *   5 re-basing   if L > 0: x-[0] += L rint((x_proj[0] - x-[0]) / L) (the projection always carries an arc length).
 *   6 update      the EKF update linearised once at the prior and processed row by row: nu0 = y - h(x-), the heading entry wrapped
 *                 to [-pi, pi] (MATLAB's angdiff(h2, y2)), H = dh/dx(x-).  For i = 0 .. nx - 1, measured components only:
 *                 nu_i = nu0_i - H_i (x - x-), c = P H_i', s_i = H_i c + r_i; unless s_i > 0 the component is skipped;
 *                 x_a += c_a nu_i / s_i, P_ab -= (c_a c_b) / s_i (exactly symmetric).  innov_i = nu_i (0 for an unmeasured
 *                 component), nis = sum of nu_i^2 / s_i over the components applied.  For diagonal R this is the joint update
 *                 K = P H' (H P H' + R)^-1 with that H.
 *   7 check       as there; step 6 then runs again from x- = x_proj, linearised at x_proj.
 * H_out is the H the applied update was linearised with (the identity for a finished car).
 * FSAEMPC_ERR_ARG before any launch: what fsaempc_cl_estimate_batch_device refuses, with y and x_proj in the places of z and
 * x_start.  desc->batch == 0 succeeds without a launch. */
int fsaempc_cl_estimate_cart_batch_device(const fsaempc_ltv_desc* desc, const fsaempc_spline* sp, const fsaempc_ltv_params* par,
                                          const fsaempc_cl_estimator* est, const double* y /* batch x nx */, const double* x_proj /* batch x nx */,
                                          const double* u_prev, long long u_stride /* doubles between cars */, const int* finished /* optional */,
                                          double* est_x, double* est_P, int* est_count /* batch x 2, zeroed by the caller */,
                                          double* x0_est, double* innov, double* nis /* batch */,
                                          double* F_out /* optional, batch x nx x nx */, double* x_prior /* optional, batch x nx */,
                                          double* H_out /* optional, batch x nx x nx */, void* stream);

/* ---- closed loop: cone-based localisation ----------------------------------------------
 * The pose inferred from detections of the track's cones against a known map, as a lidar or a camera gives it: a cone sensor, and the
 * filter above with the rows of its observations behind the car's own.  Opt-in like the entries above.  A cone map is an
 * fsaempc_cones with at most FSAEMPC_CONES_MAX cones per side (per_corridor = 1: one map per car, car-major); cones are indexed
 * g = 0 .. n_left - 1 on the left side and n_left .. n_left + n_right - 1 on the right.  Data association is known: an observation
 * carries the index of its cone.
 *
 * fsaempc_cl_cone_sense_batch_device: one call per MPC period next to fsaempc_cl_sense_batch_device, on the same stream.  One
 * wavefront per car.  With (X, Y, psi) = cart[b][0 .. 2] and cone g of the truth map at (cx, cy):
 *   observation   dx = cx - X, dy = cy - Y, rho = sqrt(dx dx + dy dy), beta = angdiff(psi, atan2(dy, dx)) (MATLAB's angdiff: the bearing
 *                 in the car's frame, wrapped to [-pi, pi]).  The cone is in view iff r_min <= rho <= r_max and |beta| <= fov / 2.
 *   draws         the words (w0, w1, w2, w3) of the generator of fsaempc_cl_observe_batch_device with the counter (step, 2 + g, id lo,
 *                 id hi), id = id0 + b (calls 0 and 1 of that layout are the state draws: cone draws never collide with them under one
 *                 seed), and the normals (z0, z1) of (w0, w1).  The cone is detected iff (w2 + 0.5) 2^-32 < p_detect;
 *                 rho_m = rho + sigma_range z0, beta_m = angdiff(0, beta + sigma_bearing z1) (a sigma of 0 copies).  A cone's draw
 *                 depends on the seed, the car's id, the period and the cone's index only.
 *   selection     of the cones in view and detected (cone_seen[b] counts them) the min(cone_seen, k_max) smallest by the key
 *                 (rho, g) -- the true range, ties broken by the index -- in that order: cone_n[b] their number, cone_id[b][k] the
 *                 index (-1 past the count), cone_z[b][k] = (rho_m, beta_m) (0 past the count).
 *   finished      finished[b] != 0: cone_n = cone_seen = 0, every cone_id -1, every cone_z 0.
 * No atomics: the result does not depend on the batch or the launch geometry, bit for bit.
 * FSAEMPC_ERR_ARG before any launch, with the argument named: sensor, sensor->truth, cart, cone_n, cone_seen, cone_id or cone_z NULL; a
 * side's pointer NULL with a count > 0; batch < 0; k_max outside 1 .. FSAEMPC_CONE_OBS_MAX; r_min not > 0 or not < a finite r_max; fov
 * outside (0, 2 pi]; a negative or NaN sigma; p_detect outside [0, 1]; id0 < 0; step < 0 or >= 2^32; a negative count or a map with
 * no cones; an output that overlaps another output or an input.  FSAEMPC_ERR_DIM: more than FSAEMPC_CONES_MAX cones on a side.
 * batch == 0 succeeds without a launch. */
#define FSAEMPC_CONE_OBS_MAX 16   /* observations per car and period */
typedef struct {
  const fsaempc_cones* truth;   /* where the cones are */
  double r_min, r_max;          /* m */
  double fov;                   /* rad, the whole opening angle, centred on the heading */
  double sigma_range, sigma_bearing;
  double p_detect;
  int k_max;
  unsigned long long seed;
  long long id0;                /* id of instance 0 (a shard's first global id) */
} fsaempc_cl_cone_sensor;

int fsaempc_cl_cone_sense_batch_device(int batch, const fsaempc_cl_cone_sensor* sensor, long long step, const double* cart /* batch x 7 */,
                                       const int* finished /* optional */, int* cone_n /* batch */, int* cone_seen /* batch */,
                                       int* cone_id /* batch x k_max */, double* cone_z /* batch x k_max x 2 */, void* stream);

/* fsaempc_cl_estimate_cones_batch_device: fsaempc_cl_estimate_cart_batch_device with the cone rows.  Steps 1 .. 8 of that entry hold;
 * the update (step 6, and its second run of step 7, then linearised at x_proj) processes the nx own rows as there and then, per
 * observation k < cone_n[b] in order, its range row and its bearing row, linearised once at the same prior x-.  With
 * (h0, h1, h2) = h(x-)[0 .. 2], Hr the rows and columns 0 .. 2 of H = dh/dx(x-), id = cone_id[b][k], (mx, my) cone id of `map` (which may
 * differ from the truth the sensor read: same counts and indexing; per_corridor = 1: one map per car) and (rho_m, beta_m) = cone_z[b][k]:
 *   dx = mx - h0, dy = my - h1, q2 = dx dx + dy dy, rho^ = sqrt(q2), beta^ = angdiff(h2, atan2(dy, dx)),
 *   g_rho = (-dx / rho^, -dy / rho^, 0), g_beta = (dy / q2, -dx / q2, -1), G_i[c] = sum_k g_i[k] Hr[k][c] (k = 0, 1, 2 in this order; the
 *   state columns >= 3 are zero), nu0_rho = rho_m - rho^, nu0_beta = angdiff(beta^, beta_m).
 * A row with variance r (r_cone[0] for range, r_cone[1] for bearing, shared by the batch; +Inf switches the channel off):
 *   nu = nu0 - sum_c G[c] (x[c] - x-[c]), c = P G', s = G c + r; applied iff 0 <= id < n_left + n_right, rho^ > 0, r is finite and
 *   >= 0 and s > 0: x_a += c_a nu / s, P_ab -= (c_a c_b) / s (exactly symmetric).  A row that is not applied changes nothing and its
 *   innovation is 0.  A non-finite cone_z of an applied row spoils the update, which step 7 answers.
 * cone_innov[b][k] = the innovations of the two rows (0 for k >= cone_n[b]); rows_used[b] = the rows applied, own and cone rows; nis
 * sums over all of them; G_out (optional) = the two composed rows of every observation of the applied update (0 where not applied).
 * A finished car: cone_innov = 0, rows_used = 0, G_out = 0.  cone_n[b] is clamped to 0 .. k_max.  With cone_n = 0 everywhere, or both
 * variances +Inf, every common output equals fsaempc_cl_estimate_cart_batch_device's bit for bit.
 * FSAEMPC_ERR_ARG before any launch, with the argument named: what fsaempc_cl_estimate_cart_batch_device refuses; map, r_cone, cone_n,
 * cone_id, cone_z, cone_innov or rows_used NULL; a side's pointer NULL with a count > 0; k_max outside 1 .. FSAEMPC_CONE_OBS_MAX; a
 * negative count or a map with no cones; an output that overlaps another output or an input.  FSAEMPC_ERR_DIM: more than
 * FSAEMPC_CONES_MAX cones on a side.  desc->batch == 0 succeeds without a launch. */
int fsaempc_cl_estimate_cones_batch_device(const fsaempc_ltv_desc* desc, const fsaempc_spline* sp, const fsaempc_ltv_params* par,
                                           const fsaempc_cl_estimator* est, const double* y /* batch x nx */, const double* x_proj /* batch x nx */,
                                           const double* u_prev, long long u_stride /* doubles between cars */, const int* finished /* optional */,
                                           double* est_x, double* est_P, int* est_count /* batch x 2, zeroed by the caller */,
                                           double* x0_est, double* innov, double* nis /* batch */,
                                           double* F_out /* optional, batch x nx x nx */, double* x_prior /* optional, batch x nx */,
                                           double* H_out /* optional, batch x nx x nx */,
                                           const fsaempc_cones* map, int k_max, const double* r_cone /* host, 2 */,
                                           const int* cone_n /* batch */, const int* cone_id /* batch x k_max */,
                                           const double* cone_z /* batch x k_max x 2 */, double* cone_innov /* batch x k_max x 2 */,
                                           int* rows_used /* batch */, double* G_out /* optional, batch x k_max x 2 x 3 */, void* stream);

/* ---- closed loop: the batched SQP (nonlinear MPC) as the controller (main.m:118-160, MODE = "MS-NMPC") ----------
 * Between the pre-step (and lap gate, observation, estimator) and the plant, in place of the LTV step and
 * fsaempc_cl_accept_batch_device: shift -> fsaempc_sqp_batch_device_m -> accept.  Both entries return FSAEMPC_ERR_ARG, with a text
 * and before anything is launched or written, for a NULL required pointer, N < 1, batch < 0, an unknown model, a shift that is not
 * 0 or 1 and a u_init that overlaps u_keep; batch == 0 succeeds without a launch. */

/* The start of this period's solve from the plan the loop keeps (main.m:139-149: the previous solution goes back in):
 * u_init[b, k] = u_keep[b, k + 1] for k < N - 1, u_init[b, N - 1] = u_keep[b, N - 1]; shift = 0 copies u_keep (the first period:
 * the guess of main.m:47-55 is used as it is).  skip[b] = (finished[b] != 0), the mask of fsaempc_sqp_batch_device_m; finished may
 * be NULL (skip is then all zero).  u_keep, u_init: batch x N x 2. */
int fsaempc_cl_nmpc_shift_batch_device(int N, int batch, int shift, const double* u_keep, const int* finished, double* u_init, int* skip,
                                       void* stream);

/* Take-over of the SQP's result (x_new: nx*N, u_new: 2*N per car; status, qp_iter as the SQP returned them; qp_iter and skip may be
 * NULL).  A car with skip[b] != 0: x_keep, u_keep untouched, exitflag 0, iter 0.  Every other car: exitflag 0 for status 0 and 1
 * (under a sweep cap the sweep limit is the regular end of a period), the status itself (2, -1, -2) otherwise; iter = qp_iter (0
 * without it); the plan is taken over iff every entry of x_new and u_new is finite, whatever the status: every point the SQP returns
 * is the rollout of inputs inside their boxes from this period's state, after a failed QP that of the shifted previous plan
 * (unlike fsaempc_cl_accept_batch_device, which keeps the stale plan after an abnormal exit). */
int fsaempc_cl_nmpc_accept_batch_device(int model, int N, int batch, const double* x_new, const double* u_new, const int* status,
                                        const int* qp_iter, const int* skip, double* x_keep, double* u_keep, int* exitflag, int* iter,
                                        void* stream);

/* ---- track pipeline (host side) --------------------------------------------------- */

/* Spline table of a track as main.m:11-17 produces it: M arc-length segments, xP / yP = M x 4 Bezier control points per axis
 * (column-major: all P0, then all P1, P2, P3), dl = segment length, L = total length.  Host memory owned by the library
 * (fsaempc_track_free).  These are the tables fsaempc_spline points at (after a copy to the device). */
typedef struct {
  int M;
  double dl, L;
  double* xP;
  double* yP;
} fsaempc_track;

/* Replaces main.m:11-17: [x,y,...] = read_raceline_csv(file) (util/read_raceline_csv.m:6-19: one header line, columns 1-2 = X, Y),
 * x_spline = make_spline_periodic(x) (spline/make_spline_periodic.m:9-33), likewise y,
 * [x_spline,y_spline,dl,L] = arclength_reparam(x_spline,y_spline,M,true) (spline/arclength_reparam.m:15-64; M = 100 in main.m:17).
 * The reference's quirk in the speed integrand (arclength_reparam.m:20-23) is kept.  Host only, no GPU work. */
int fsaempc_track_from_csv(const char* path, int M, fsaempc_track* out);
int fsaempc_track_from_points(const double* x, const double* y, int n, int M, fsaempc_track* out);
void fsaempc_track_free(fsaempc_track* t);
/* On-disk table format "FSTRK001" (little endian): 8-byte magic, int32 M, int32 0, double dl, double L, xP (4M doubles), yP (4M). */
int fsaempc_track_save(const fsaempc_track* t, const char* path);
int fsaempc_track_load(const char* path, fsaempc_track* out);
/* The cone columns of the same CSV (util/read_raceline_csv.m:16-19: columns 8, 9 = rX, rY, the right cones; 10, 11 = lX, lY, the
 * left cones), read by the reader of fsaempc_track_from_csv: *left / *right are n x 2 doubles, xy interleaved, host memory owned by
 * the library (fsaempc_track_cones_free; NULL with a count of 0).  A row whose pair is empty or non-finite is skipped for that side
 * only.  FSAEMPC_ERR_ARG: a NULL argument, a file that cannot be opened, a row with fewer than 11 columns. */
int fsaempc_track_cones_from_csv(const char* path, double** left, int* n_left, double** right, int* n_right);
void fsaempc_track_cones_free(double* cones);
const char* fsaempc_track_last_error(void);

/* ---- diagnostics ---------------------------------------------------------------------------- */
const char* fsaempc_last_error(void);
/* Runs the on-device fp64 MFMA layout self-test (v_mfma_f64_16x16x4_f64 operand / accumulator
 * lane maps the kernels rely on).  Returns 0 if the hardware matches, >0 number of mismatches. */
int fsaempc_selftest_mfma(void);
/* Runs the on-device self-test of the cross-lane reductions of the solve kernel (DPP row reductions, single and batched, lane-swap
 * reductions over the four rows, whole-wave reductions) on 256 rounds of doubles that mix magnitudes 1e-300..1e300, +-0, denormals,
 * +-Inf and NaN: bit for bit against the zero-filling lane moves and against a tree through LDS with the same pairing.
 * Returns 0 if all agree, >0 number of mismatches, <0 without a device. */
int fsaempc_selftest_lane_reduce(void);
/* Runs the on-device self-test of the diagonal-tile factorisation of the solve kernel's register Cholesky: 64 tiles (SPD with condition
 * numbers 1..1e10, a pivot under the floor, a NaN, +Inf) through the former form of diag_factor and through the newer ones; the
 * factor, both companion tiles and the flag are compared bit for bit.  Returns 0 if all agree, >0 number of mismatches, <0 without a device. */
int fsaempc_selftest_diag_factor(void);
/* Runs the on-device self-test of the solve kernel's start-up pass on five small QPs with staircase sparsity and infinite, one-sided
 * and equality bounds, (nV, nC) = (20, 5), (35, 70), (32, 64), (25, 72), (81, 240), prepared by the real prep kernel: A~x and A~'w of
 * the initial multipliers from the one fused pass against a pass of its own for each, bit for bit.  Returns 0 if all agree, >0 number of
 * mismatches, <0 without a device. */
int fsaempc_selftest_initial_point(void);
/* Debug hook of the diagnostic builds only (libfsaempc_dbg.so, -DQP_DEBUG_DUMP; the shipped kernels carry no dump
 * branches and ignore it): dumps solver internals of instance 0 after `stage` (see qp_solver.hip) into `out` (device
 * pointer, >= 4*nV*nV+8*(nV+nC) doubles).  Process-global, not thread-safe. */
int fsaempc_debug_set_dump(double* out, int stage);

/* Kernel timing with HIP events recorded on the launch stream of the last fsaempc_qp_solve_batch_device
 * call (prep = scaling/repack kernel, solve = interior-point kernel).  get_timing synchronises on the events.
 * Process-global switch for benchmarks (bench.py); not thread-safe. */
int fsaempc_qp_set_timing(int enable);
int fsaempc_qp_get_timing(double* prep_ms, double* solve_ms);
/* Same switch, for the last fsaempc_ltv_step_batch_device[_aux] call: the four phases of the fused step (construction kernel,
 * prep = scaling / repack / launch order, interior-point solve, post-solve kernel) by HIP events on the launch stream.
 * Every phase is also a roctx range on the calling thread (fsaempc.ltv.step > fsaempc.ltv.build, fsaempc.qp.prep+solve,
 * fsaempc.ltv.post; `rocprofv3 --marker-trace --kernel-trace`), through librocprofiler-sdk-roctx (or roctracer's libroctx64) if the process can load it (FSAEMPC_ROCTX=0
 * turns the ranges off). */
int fsaempc_ltv_get_timing(double* build_ms, double* prep_ms, double* solve_ms, double* post_ms);

#ifdef __cplusplus
}
#endif
#endif
