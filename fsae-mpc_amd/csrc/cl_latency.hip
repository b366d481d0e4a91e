// cl_latency.hip -- the imperfect closed loop (no counterpart in main.m, which reads the exact state and computes in
// zero time): state-estimate noise and the state predictor of the delay compensation, batched on the device.  One thread per car
// like the kernels of plant.hip: every piece is a short scalar recurrence, the batch of independent cars is the parallel axis.
//
//   cl_noise_kernel    the nx standard normals of (seed, id0 + b, step): the generator on its own (the test hook)
//   cl_observe_kernel  between the pre-step (and the lap gate) and the MPC step: x0_obs = x0_true + sigma z, then x0_mpc = x0_obs
//                      rolled over the `delay` periods that pass before this period's plan reaches the plant, with psi_step
//                      (nlp_model.h: the NLP's rollout step, the controller's own model and parameter block) under the first inputs
//                      of the plans that will be in effect then.  A car whose prediction cannot be trusted (an input or a result
//                      that is not finite, a block that cannot describe a car) gets x0_mpc = x0_obs bit for bit.
#include <hip/hip_runtime.h>
#include <math.h>
#include "cl_latency.h"
#include "mpc_params.h"
#include "nlp_model.h"

namespace {

__global__ void __launch_bounds__(64) cl_noise_kernel(int nx, int batch, unsigned long long seed, unsigned long long id0, unsigned long long step, double* z) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= batch) return;
  double d[8];
  cll_draws(seed, id0 + (unsigned long long)b, step, d);
  for (int i = 0; i < nx; ++i) z[(size_t)b * nx + i] = d[i];
}

template <int NX, class PAR> __global__ void __launch_bounds__(64) cl_observe_kernel(ClObserveParams P, typename PAR::Args pa) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= P.batch) return;
  double x[NX], xo[NX];
  for (int i = 0; i < NX; ++i) x[i] = P.x0_true[(size_t)b * NX + i];
  double* obs = P.x0_obs + (size_t)b * NX;
  double* mpc = P.x0_mpc + (size_t)b * NX;
  if (P.finished && P.finished[b]) {                 // out of the race or at the end of its run: the state stays as it is
    for (int i = 0; i < NX; ++i) { obs[i] = x[i]; mpc[i] = x[i]; }
    return;
  }
  if (P.sigma) {
    const double* sg = P.sigma + (P.sigma_per_instance ? (size_t)b * NX : (size_t)0);
    double s[NX], z[8];
    for (int i = 0; i < NX; ++i) s[i] = sg[i];
    cll_draws(P.seed, P.id0 + (unsigned long long)b, P.step, z);
    for (int i = 0; i < NX; ++i) xo[i] = cll_observe(x[i], s[i], z[i]);
  } else {
    for (int i = 0; i < NX; ++i) xo[i] = x[i];
  }
  for (int i = 0; i < NX; ++i) obs[i] = xo[i];
  bool ok = P.compensate != 0 && P.delay >= 1;
  PAR p;
  if constexpr (PAR::RT) {
    if (ok) {
      p = par_load(pa.values + (size_t)b * (size_t)pa.stride);
      ok = !p.bad;
    }
  }
  double xp[NX];
  for (int i = 0; i < NX; ++i) xp[i] = xo[i];
  if (ok) {
    const Spl sp{P.spM, P.spdl, P.xP, P.yP};
#pragma unroll 1
    for (int j = 0; j < P.delay && ok; ++j) {        // plan_{step - delay + j}: the one the plant follows j periods from now
      const int slot = cll_slot(P.delay, (long long)P.step, P.delay - j);
      const double* uh = P.u_hist + ((size_t)slot * (size_t)P.batch + (size_t)b) * (size_t)(2 * P.N);
      const double u[2] = {uh[0], uh[1]};
      ok = fabs(u[0]) < INFINITY && fabs(u[1]) < INFINITY;
      if (!ok) break;
      double xn[NX];
      psi_step<NX>(p, xp, u, sp, P.dt, P.integ, xn);
      for (int i = 0; i < NX; ++i) { xp[i] = xn[i]; ok = ok && fabs(xn[i]) < INFINITY; }
    }
  }
  for (int i = 0; i < NX; ++i) mpc[i] = ok ? xp[i] : xo[i];
}

template <int NX> hipError_t observe_launch(const ClObserveParams& P, hipStream_t st, const double* par, int par_stride) {
  if (par) hipLaunchKernelGGL((cl_observe_kernel<NX, RtPar>), dim3((P.batch + 63) / 64), dim3(64), 0, st, P, ParArgs{par, par_stride, nullptr});
  else hipLaunchKernelGGL((cl_observe_kernel<NX, FixedPar>), dim3((P.batch + 63) / 64), dim3(64), 0, st, P, NoParArgs{});
  return hipGetLastError();
}

}  // namespace

hipError_t cl_noise_launch(int nx, int batch, unsigned long long seed, unsigned long long id0, unsigned long long step, double* z, hipStream_t st) {
  if (batch == 0) return hipSuccess;
  hipLaunchKernelGGL(cl_noise_kernel, dim3((batch + 63) / 64), dim3(64), 0, st, nx, batch, seed, id0, step, z);
  return hipGetLastError();
}
hipError_t cl_observe_launch(const ClObserveParams& P, hipStream_t st, const double* par, int par_stride) {
  if (P.batch == 0) return hipSuccess;
  return P.nx == 5 ? observe_launch<5>(P, st, par, par_stride) : observe_launch<7>(P, st, par, par_stride);
}
