// cl_latency.h -- measurement noise, plan latency and delay compensation of the closed loop: the counter-based
// generator of the state-estimate noise, the map from its words to standard normals, the counter layout and the slot arithmetic of
// the plan history, written once for the host and the device, and the internal interface between the C ABI and the kernels of
// cl_latency.hip.
//
//   cll_philox     Philox4x32-10 (Salmon et al., SC'11): ten rounds, multipliers 0xD2511F53 / 0xCD9E8D57, the key bumped by the
//                  Weyl constants 0x9E3779B9 / 0xBB67AE85 between rounds
//   cll_normals    two Box-Muller pairs out of the four words of one call: u = (w + 0.5) 2^-32 lies in (0, 1), so the logarithm is
//                  finite and |z| <= sqrt(2 * 33 * ln 2) = 6.76
//   cll_draws      the nx normals of (seed, id, step): key (seed lo, seed hi), counter (step, j, id lo, id hi); call j = 0 serves
//                  components 0 .. 3, call j = 1 components 4 .. 6
//   cll_observe    x_obs[i] = x[i] + sigma[i] z[i] where sigma[i] > 0 and finite, a copy of x[i] everywhere else
//   cll_slot       slot of plan_{step - lag} in a history of delay + 1 plans: (step - lag) mod (delay + 1), never negative.  The
//                  plan of period k goes to slot k mod (delay + 1) after the solve; before that the slot still holds plan_{k-delay-1},
//                  and for k - lag < 0 what the caller filled the history with (the initial guess)
//
// The first part compiles as plain C++ (a host program may include this file without the HIP headers).  No FMA contraction in it:
// tests/latency_numpy.py restates every function operation for operation.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include "fsaempc.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CLL_HD __host__ __device__ __forceinline__
#else
#define CLL_HD inline
#endif

CLL_HD void cll_philox(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
  uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// (w + 0.5) 2^-32: exact in a double
CLL_HD double cll_u01(uint32_t w) { return ((double)w + 0.5) * (1.0 / 4294967296.0); }

CLL_HD void cll_normals(const uint32_t w[4], double z[4]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  for (int h = 0; h < 2; ++h) {
    const double u1 = cll_u01(w[2 * h]), u2 = cll_u01(w[2 * h + 1]);
    const double r = sqrt(-2.0 * log(u1)), a = 6.283185307179586 * u2;
    z[2 * h] = r * cos(a); z[2 * h + 1] = r * sin(a);
  }
}

CLL_HD void cll_words(unsigned long long seed, unsigned long long id, unsigned long long step, int j, uint32_t w[4]) {
  const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
  const uint32_t ctr[4] = {(uint32_t)step, (uint32_t)j, (uint32_t)id, (uint32_t)(id >> 32)};
  cll_philox(ctr, key, w);
}

// z: 8 doubles; entries 0 .. nx - 1 are the car's draws (entry 7, and 5 .. 6 of the kinematic model, are computed and unused)
CLL_HD void cll_draws(unsigned long long seed, unsigned long long id, unsigned long long step, double z[8]) {
  uint32_t w[4];
  cll_words(seed, id, step, 0, w); cll_normals(w, z);
  cll_words(seed, id, step, 1, w); cll_normals(w, z + 4);
}

CLL_HD double cll_observe(double x, double sigma, double z) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (!(sigma > 0.0 && sigma < INFINITY)) return x;   // zero, negative, NaN, Inf: the component is copied (keeps -0.0)
  const double e = sigma * z;
  return x + e;
}

CLL_HD int cll_slot(int delay, long long step, int lag) {
  const long long m = (long long)delay + 1;
  long long r = (step - (long long)lag) % m;
  if (r < 0) r += m;
  return (int)r;
}

#if defined(__HIPCC__)
struct ClObserveParams {
  int nx, N, batch, integ;        // integ: 0 Euler, 1 RK2, 2 RK4 (resolved by the caller)
  int delay, compensate, sigma_per_instance;
  double dt;
  unsigned long long seed, id0, step;
  int spM; double spdl; const double* xP; const double* yP;   // spline table (device)
  const double* sigma;            // optional: nx, or batch x nx
  const double* x0_true;          // batch x nx
  const int* finished;            // optional
  const double* u_hist;           // (delay + 1) x batch x N x 2; read only with compensate and delay >= 1
  double* x0_obs;                 // batch x nx
  double* x0_mpc;                 // batch x nx
};
hipError_t cl_noise_launch(int nx, int batch, unsigned long long seed, unsigned long long id0, unsigned long long step, double* z, hipStream_t st);
// par (optional): the controller's parameter blocks, car b reads par + b * par_stride; null: the constants compiled in
hipError_t cl_observe_launch(const ClObserveParams& P, hipStream_t st, const double* par = nullptr, int par_stride = 0);
#endif
