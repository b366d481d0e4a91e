// sqp.h -- internal interface between the C ABI and the SQP kernels of sqp.hip (DESIGN.md "Nonlinear MPC: batched SQP")
#pragma once
#include <hip/hip_runtime.h>

struct SqpParams {
  int nx, N, integ, B;                 // B: instances of the whole batch
  double dt;
  int spM; double spdl; const double* xP; const double* yP;
  const double *x0, *x_ref;            // whole batch
  // iterate and outputs (whole batch, indexed by instance)
  double *u, *x, *s, *fval;            // u_opt, x_opt (rollout), slack, NLP objective
  int *status, *sweeps;
  double *rho, *J, *viol, *vmax;       // workspace: penalty, objective, l1 and max hard violation of the iterate
  double *lambda_out, *step_norm, *hard_viol, *merit;   // optional (fsaempc_sqp_aux)
  int* qp_iter;
  int max_sweeps, trials;
  double tol_step, tol_feas, armijo, rho0;
};

// status of an instance still in the batch
constexpr int SQP_RUNNING = 3;

// par (optional; here and in sqp_linesearch_launch): parameter blocks of the batch (include/fsaempc.h FSAEMPC_P_*), instance i reads
// par + i * par_stride; null: the kernels with the reference's constants compiled in
hipError_t sqp_init_launch(const SqpParams& P, const double* u_init, hipStream_t st, const double* par = nullptr, int par_stride = 0);
hipError_t sqp_compact_launch(const int* status, int B, int* idx, int* count, hipStream_t st);
hipError_t sqp_gather_launch(const SqpParams& P, const int* idx, int cnt, double* gx0, double* gxref, double* gu, double* xinit, int nV,
                             hipStream_t st);
// One launch per sweep: line search, penalty update, status, scatter of the accepted iterate.  Sub-batch arrays (cnt instances,
// instance b is idx[b] of the batch): QP solution z (nV), its objective fval_qp (without the constant) + qconst, flag, iterations, lambda.
hipError_t sqp_linesearch_launch(const SqpParams& P, const int* idx, int cnt, int sweep, const double* z, const double* fval_qp,
                                 const double* qconst, const int* flag, const int* iter, const double* lambda, hipStream_t st,
                                 const double* par = nullptr, int par_stride = 0);
