// cl_nmpc.hip -- the batched SQP (sqp.hip) as the controller of the closed loop (main.m:118-160, MODE = "MS-NMPC"):
// the plan the loop keeps is shifted by one stage into the start of this period's solve (main.m:139-149 hands x_mpc back in), cars
// that no longer drive are masked out of the SQP's sub-batch, and the SQP's result is taken over as the plan of the next period.
// Copies and selections only: tests/nmpc_loop_numpy.py restates all three bit for bit.
#include <hip/hip_runtime.h>
#include <math.h>
#include "fsaempc.h"
#include "cl_nmpc.h"

namespace {

// One thread per (car, stage): consecutive threads read and write consecutive input pairs.
__global__ __launch_bounds__(256) void cl_nmpc_shift_kernel(int N, int batch, int shift, const double* u_keep, const int* finished, double* u_init, int* skip) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (size_t)batch * (size_t)N) return;
  const int k = (int)(t % (size_t)N);
  const size_t b = t / (size_t)N;
  const size_t src = (shift && k < N - 1) ? t + 1 : t;   // the last stage is repeated
  u_init[2 * t] = u_keep[2 * src];
  u_init[2 * t + 1] = u_keep[2 * src + 1];
  if (k == 0) skip[b] = (finished && finished[b] != 0) ? 1 : 0;
}

__global__ __launch_bounds__(256) void sqp_skip_kernel(int batch, const int* skip, int* status) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)batch) return;
  if (skip[i] != 0) status[i] = FSAEMPC_SQP_SKIPPED;
}

// Take-over of the SQP's result, one 64-lane wavefront per car, lanes striding over the car's nx N and 2 N entries.  A skipped car
// keeps its plan and reports exit flag 0 with no iterations.  For every other car the plan is taken over iff all of its entries are
// finite, WHATEVER the status: sqp_init_kernel and the winner lane of the line search only ever write an evaluated point -- the
// rollout of clamped inputs -- so after a failed QP (status -1, -2) or a refused step (2) the output is the shifted previous plan
// rolled out from this period's state, which respects the input boxes and starts where the car is.  That is a better fallback than
// the stale plan cl_accept_kernel (plant.hip) leaves in place after an abnormal exit of the interior-point solve, whose last iterate
// may violate the boxes (documented difference).  Exit flag: 0 for status 0 and 1 (under a sweep cap the sweep limit is the regular
// end of a period), the status itself otherwise.
__global__ __launch_bounds__(64) void cl_nmpc_accept_kernel(int len_x, int len_u, int batch, const double* x_new, const double* u_new, const int* status,
                                                            const int* qp_iter, const int* skip, double* x_keep, double* u_keep, int* exitflag, int* iter) {
  const size_t b = blockIdx.x;
  const int lane = threadIdx.x;
  const bool skipped = skip && skip[b] != 0;            // uniform over the wavefront
  const double* xn = x_new + b * (size_t)len_x;
  const double* un = u_new + b * (size_t)len_u;
  bool finite = true;
  if (!skipped) {
    for (int j = lane; j < len_x; j += 64) finite = finite && fabs(xn[j]) < INFINITY;
    for (int j = lane; j < len_u; j += 64) finite = finite && fabs(un[j]) < INFINITY;
  }
  const bool take = __ballot(!finite) == 0ull && !skipped;   // every lane votes: nothing returns before this line
  if (take) {
    double* xk = x_keep + b * (size_t)len_x;
    double* uk = u_keep + b * (size_t)len_u;
    for (int j = lane; j < len_x; j += 64) xk[j] = xn[j];
    for (int j = lane; j < len_u; j += 64) uk[j] = un[j];
  }
  if (lane == 0) {
    const int st = status[b];
    exitflag[b] = (skipped || st == 0 || st == 1) ? 0 : st;
    iter[b] = (skipped || !qp_iter) ? 0 : qp_iter[b];
  }
}

}  // namespace

hipError_t cl_nmpc_shift_launch(int N, int batch, int shift, const double* u_keep, const int* finished, double* u_init, int* skip, hipStream_t st) {
  const size_t total = (size_t)batch * (size_t)N;
  if (total == 0) return hipSuccess;
  hipLaunchKernelGGL(cl_nmpc_shift_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, N, batch, shift, u_keep, finished, u_init, skip);
  return hipGetLastError();
}

hipError_t sqp_skip_launch(int batch, const int* skip, int* status, hipStream_t st) {
  if (batch <= 0) return hipSuccess;
  hipLaunchKernelGGL(sqp_skip_kernel, dim3((batch + 255) / 256), dim3(256), 0, st, batch, skip, status);
  return hipGetLastError();
}

hipError_t cl_nmpc_accept_launch(int len_x, int len_u, int batch, const double* x_new, const double* u_new, const int* status, const int* qp_iter,
                                 const int* skip, double* x_keep, double* u_keep, int* exitflag, int* iter, hipStream_t st) {
  if (batch <= 0) return hipSuccess;
  hipLaunchKernelGGL(cl_nmpc_accept_kernel, dim3(batch), dim3(64), 0, st, len_x, len_u, batch, x_new, u_new, status, qp_iter, skip, x_keep, u_keep,
                     exitflag, iter);
  return hipGetLastError();
}
