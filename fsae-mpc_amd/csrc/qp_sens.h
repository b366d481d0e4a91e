// qp_sens.h -- internal interface between the C ABI (capi_qp.hip) and the QP vector-Jacobian product kernel (qp_sens.hip)
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

// per-instance status of the VJP (include/fsaempc.h, fsaempc_qp_vjp_batch_device)
#define QPS_OK 0          // vertex, system solved, every working-set multiplier clearly non-zero
#define QPS_WEAK 1        // as 0, a weakly active side was kept in the working set (one-sided derivative)
#define QPS_IPM 2         // forward returned the interior-point iterate; working set of the rule used anyway
#define QPS_SINGULAR (-1) // equality-QP system singular / not solved to tolerance: zeros
#define QPS_FWD (-2)      // forward exit flag != 0: zeros

#define QPS_THREADS 256   // one workgroup (4 waves) per instance
#define QPS_MAX_SLOTS 512 // workgroups of one launch; each loops over instances b = slot, slot + slots, ... (own workspace slot)

struct QpsParams {
  int n, m, B, k, shared_HA;
  int np, ldm;               // n rounded up to 16; leading dimension of the dense n x n work matrices (np + 1)
  int m_in_lds;              // 1: the factor M lives in LDS, else in the slot's workspace
  int slots;
  double inf_bound, tol;
  const double *H, *g, *A, *lb, *ub, *lbA, *ubA;
  const double *x, *lam;
  const int *exitflag, *polished;
  const double *xbar, *fbar;
  double *gbar, *lbbar, *ubbar, *lbAbar, *ubAbar, *Hbar, *Abar;
  int* status;
  double* ws;                // slots * ws_per_slot doubles
  size_t ws_per_slot;        // doubles
  size_t lds_bytes;
};

// fills the launch geometry of P from n, m, B (everything but the pointers); returns the workspace bytes
size_t qps_plan(QpsParams* P);
hipError_t qps_launch(const QpsParams& P, hipStream_t st);
