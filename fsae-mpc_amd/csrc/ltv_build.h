// ltv_build.h -- internal interface between the C ABI and the LTV-MPC construction kernels
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

struct LtvParams {
  int nx, N, integ;   // integ: 0 Euler, 1 RK2 (midpoint), 2 RK4
  double dt;
  int spM; double spdl; const double* xP; const double* yP;   // spline table (device)
  const double *x0, *x_ref, *x_lin, *u_lin;
  double *H, *g, *A, *lb, *ub, *lbA, *ubA;
  double *pred, *Bt, *qconst;   // Bt is required (internal operand); pred/qconst optional
};

// Move blocking: M blocks of consecutive steps share one input pair.  start[j] is the first step of block j,
// start[M] = N; the map is a kernel argument (no device copy).  With a map all QP tensors of P are in blocked sizes (nV_b = 2 M + ns).
struct LtvBlockMap { int M; unsigned char start[98]; };

// The build (ltv_build_kernel.h).  bm = nullptr: unblocked.  exact = false: the LTV build of the reference; true: the exact build of
// the NLP at u_lin (x_lin is not read; it knows no blocks).  values = nullptr: the constants compiled in, else they are read from
// parameter blocks (include/fsaempc.h, FSAEMPC_P_*): workgroup b reads values + inst * stride (stride 0: one block for
// the batch), inst = idx ? idx[b] : b.
hipError_t ltv_build_launch(const LtvParams& P, const LtvBlockMap* bm, const double* values, int stride, const int* idx, int batch,
                            hipStream_t st, bool exact);
hipError_t ltv_build_launch_blocked_unit(const LtvParams& P, const LtvBlockMap& bm, const double* values, int stride, const int* idx,
                                         int batch, hipStream_t st);   // ltv_build_blocked.hip's instantiations, for ltv_build_launch
// dynamic LDS of the build, the kernel's carve term by term; par: with parameter blocks; M: blocks, 0 for unblocked
size_t ltv_build_lds_bytes(int nx, int N, int threads, bool exact = false, bool par = false, int M = 0);
// post-solve: x_opt = pred + Bt z, u_opt = z(1:2N) (bm = nullptr) or the held inputs expanded to 2N, slack, fval += const
hipError_t ltv_post_launch(int nx, int N, int ns, const LtvBlockMap* bm, int batch, const double* z, const double* pred, const double* Bt,
                           const double* qconst, double* u_opt, double* x_opt, double* slack, double* fval, hipStream_t st);

// sensitivities: the affine maps of the build in x0 / x_ref (Abar R x nx, Crow nC x nx per instance, column-major),
// the cotangent of the QP variables of a step (z = [u_opt; slack], zbar = [ubar; sbar] + Bt' xbar, kc columns) and the chain from the
// QP cotangents (gbar, lbAbar, ubAbar) to x0bar (kc x nx) / xrefbar (kc x R); status < 0 gives zeros
size_t ltv_affine_lds_bytes(int nx, int N);
hipError_t ltv_affine_launch(const LtvParams& P, int batch, double* Abar, double* Crow, hipStream_t st);
hipError_t ltv_vjp_pre_launch(int nx, int N, int ns, int batch, int kc, const double* Bt, const double* u_opt, const double* slack,
                              const double* ubar, const double* xbar, const double* sbar, double* z, double* zbar, hipStream_t st);
hipError_t ltv_vjp_chain_launch(int nx, int N, int batch, int kc, const double* Bt, const double* pred, const double* x_ref,
                                const double* Abar, const double* Crow, const double* gbar, const double* lbAbar, const double* ubAbar,
                                const double* xbar, const double* fbar, const int* status, double* x0bar, double* xrefbar, hipStream_t st);
