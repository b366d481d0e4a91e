// cl_estimator.hip -- the state estimator of the closed loop (no counterpart in main.m, which reads the exact state):
// one extended Kalman filter per car and MPC period, between the observation and the MPC step, batched on the device.  The
// algorithm is stated in include/fsaempc.h (fsaempc_cl_estimate_batch_device); the scalar rules are those of cl_estimator.h.
//
//   cl_estimate_kernel   a group of 8 lanes per car, 8 cars per wavefront.  Lane j < NX of a group runs the rollout step psi_step on
//                        dual numbers seeded in state direction j (nlp_model.h: the controller's own model, parameter block and
//                        integrator), so it ends with the predicted state and with column j of F = dPsi/dx; it owns column j of P
//                        too.  The products F P and (F P) F', the transposition behind (M + M') / 2 and the rank-one updates of the
//                        sequential scalar update take column k from lane k of the group with __shfl(v, k, 8).
//
// Every exchange runs with all 64 lanes active: there is no early return -- not for a finished car, not for the tail of the batch (the
// lanes past the last car read the last car and store nothing), not for a car that is re-initialised -- and every decision about a car
// is a select on values.  The only branch around an exchange is taken by the whole wavefront at once (the second pass of the update,
// skipped when no car of the wavefront needs it).  Lanes NX .. 7 of a group carry zero columns through the algebra.
#include <hip/hip_runtime.h>
#include <math.h>
#include "cl_estimator.h"
#include "mpc_params.h"
#include "nlp_model.h"

namespace {

constexpr int CLE_GROUP = 8;        // lanes per car
constexpr int CLE_CARS = 64 / CLE_GROUP;

// true in all 8 lanes of a group iff pred holds in one of them (one ballot of the whole wavefront, the group's byte cut out)
DEVINL bool cle_group_any(bool pred, int lane) {
  const unsigned long long m = __ballot(pred);
  return ((m >> (lane & 56)) & 0xffull) != 0ull;
}

// The sequential scalar update on the prior (x, column j of P in Pc): for every measured component i with s_i = P_ii + r_i > 0,
// x_a += c_a nu_i / s_i and P_ab -= (c_a c_b) / s_i with c = P[:, i], broadcast from lane i.  x is the same in all lanes of the group.
template <int NX> DEVINL void cle_update(int j, const double (&z)[NX], const double (&r)[NX], double (&x)[NX], double (&Pc)[NX], double (&nu)[NX],
                                         double& nis) {
#pragma clang fp contract(off)
  nis = 0.0;
#pragma unroll
  for (int i = 0; i < NX; ++i) {
    double c[NX];
#pragma unroll
    for (int a = 0; a < NX; ++a) c[a] = __shfl(Pc[a], i, CLE_GROUP);
    const double cj = Pc[i];                              // = c[j]: P is exactly symmetric here, by construction of the prior
    const bool meas = cle_measured(r[i]) != 0;
    const double v = z[i] - x[i], s = c[i] + r[i];
    const bool on = meas && cle_gain_ok(s);
    nu[i] = meas ? v : 0.0;
    nis = on ? nis + v * v / s : nis;
#pragma unroll
    for (int a = 0; a < NX; ++a) {
      x[a] = on ? x[a] + c[a] * v / s : x[a];
      Pc[a] = on ? Pc[a] - (c[a] * cj) / s : Pc[a];
    }
  }
}

template <int NX, class PAR> __global__ void __launch_bounds__(64) cl_estimate_kernel(ClEstimateParams P, typename PAR::Args pa) {
  const int lane = threadIdx.x, j = lane & (CLE_GROUP - 1);
  const int b = blockIdx.x * CLE_CARS + (lane >> 3);
  const bool live = b < P.batch;
  const size_t bb = (size_t)(live ? b : P.batch - 1);    // the tail of the batch reads the last car and stores nothing
  const bool col = j < NX;
  const int jc = col ? j : 0;

  double xh[NX];
#pragma unroll
  for (int i = 0; i < NX; ++i) xh[i] = P.est_x[bb * NX + i];
  const double u0 = P.u_prev[bb * (size_t)P.u_stride], u1 = P.u_prev[bb * (size_t)P.u_stride + 1];

  PAR p;
  bool bad = !cle_finite(u0) || !cle_finite(u1);
  if constexpr (PAR::RT) {
    p = par_load(pa.values + bb * (size_t)pa.stride);
    bad = bad || p.bad;
  }

  // prediction: value and, in lane j < NX, the derivative along state direction j
  const Spl sp{P.spM, P.spdl, P.xP, P.yP};
  Dl xd[NX], xn[NX];
  const Dl ud[2] = {Dl(u0), Dl(u1)};
#pragma unroll
  for (int i = 0; i < NX; ++i) xd[i] = Dl(xh[i], i == j ? 1.0 : 0.0);
  psi_step<NX>(p, xd, ud, sp, P.dt, P.integ, xn);

  // (everything else is read after the model: nothing but the state and the input lives across its four evaluations)
  double z[NX], r[NX], p0[NX], xs[NX], Pc[NX];
  const double* rp = P.r + (P.r_per_instance ? bb * NX : (size_t)0);
#pragma unroll
  for (int i = 0; i < NX; ++i) {
    z[i] = P.z[bb * NX + i]; xs[i] = P.x_start[bb * NX + i]; r[i] = rp[i]; p0[i] = P.p0[i];
    const double pv = P.est_P[(bb * NX + i) * NX + jc];
    Pc[i] = col ? pv : 0.0;
  }
  const double qv = P.q[(P.q_per_instance ? bb * NX : (size_t)0) + jc];
  const double qj = col ? qv : 0.0;
  const int cnt0 = P.est_count[2 * bb], cnt1 = P.est_count[2 * bb + 1];
  const bool fin = P.finished != nullptr && P.finished[bb] != 0;

  const bool first = cnt0 == 0;                           // the car's first period: the prior is (x_start, diag(p0)), F = I
  double xm[NX], Fc[NX];
#pragma unroll
  for (int a = 0; a < NX; ++a) {
    xm[a] = first ? xs[a] : xn[a].v;
    Fc[a] = first ? (a == j ? 1.0 : 0.0) : (col ? xn[a].d : 0.0);
  }

  // FP = F P (column j), and row j of F on the way: t = F[a][k] reaches every lane of the group
  double FP[NX], Fr[NX];
#pragma unroll
  for (int a = 0; a < NX; ++a) { FP[a] = 0.0; Fr[a] = 0.0; }
#pragma unroll
  for (int a = 0; a < NX; ++a)
#pragma unroll
    for (int k = 0; k < NX; ++k) {
      const double t = __shfl(Fc[a], k, CLE_GROUP);
      FP[a] += t * Pc[k];
      Fr[k] = (a == j) ? t : Fr[k];
    }
  // M = FP F' (column j): M[a][j] = sum_k FP[a][k] F[j][k]
  double Mc[NX], Mr[NX];
#pragma unroll
  for (int a = 0; a < NX; ++a) { Mc[a] = 0.0; Mr[a] = 0.0; }
#pragma unroll
  for (int a = 0; a < NX; ++a)
#pragma unroll
    for (int k = 0; k < NX; ++k) Mc[a] += __shfl(FP[a], k, CLE_GROUP) * Fr[k];
  // row j of M, then P- = (M + M') / 2 + diag(q): entries (a, j) and (j, a) add the same two numbers
#pragma unroll
  for (int a = 0; a < NX; ++a)
#pragma unroll
    for (int k = 0; k < NX; ++k) {
      const double t = __shfl(Mc[a], k, CLE_GROUP);
      Mr[k] = (a == j) ? t : Mr[k];
    }
  double Pm[NX];
#pragma unroll
  for (int a = 0; a < NX; ++a) {
    const double h = 0.5 * (Mc[a] + Mr[a]);
    const double pred = (a == j) ? h + qj : h;
    const double init = (a == j && col) ? p0[a] : 0.0;
    Pm[a] = first ? init : pred;
  }

  // re-initialisation before the update: the block, the input, x- or P- cannot be used
#pragma unroll
  for (int a = 0; a < NX; ++a) bad = bad || !cle_finite(xm[a]) || (col && cle_prior_bad(Pm[a], a == j));
  const bool reset1 = cle_group_any(bad, lane);
#pragma unroll
  for (int a = 0; a < NX; ++a) {
    xm[a] = reset1 ? z[a] : xm[a];
    Pm[a] = reset1 ? ((a == j && col) ? p0[a] : 0.0) : Pm[a];
  }
  xm[0] = cle_rebase(xm[0], z[0], P.L, cle_measured(r[0]));

  double x[NX], nu[NX], nis;
#pragma unroll
  for (int a = 0; a < NX; ++a) { x[a] = xm[a]; Pc[a] = Pm[a]; }
  cle_update<NX>(j, z, r, x, Pc, nu, nis);
  bool pb = false;
#pragma unroll
  for (int a = 0; a < NX; ++a) pb = pb || !cle_finite(x[a]) || (col && cle_post_bad(Pc[a], a == j));
  const bool reset2 = cle_group_any(pb, lane);
  if (__ballot(reset2) != 0ull) {                         // (the same in all 64 lanes) some car's update failed: x- = z, P- = diag(p0) again
    double x2[NX], P2[NX], nu2[NX], nis2;
#pragma unroll
    for (int a = 0; a < NX; ++a) { x2[a] = z[a]; P2[a] = (a == j && col) ? p0[a] : 0.0; }
    cle_update<NX>(j, z, r, x2, P2, nu2, nis2);
#pragma unroll
    for (int a = 0; a < NX; ++a) {
      x[a] = reset2 ? x2[a] : x[a]; Pc[a] = reset2 ? P2[a] : Pc[a]; nu[a] = reset2 ? nu2[a] : nu[a];
    }
    nis = reset2 ? nis2 : nis;
  }

  // stores: lane j < NX writes column j of the two matrices, lanes 0 .. 3 one vector each (no register array is indexed by the lane)
  if (live && col) {
    if (P.F_out) {
#pragma unroll
      for (int a = 0; a < NX; ++a) P.F_out[(bb * NX + a) * NX + j] = fin ? (a == j ? 1.0 : 0.0) : Fc[a];
    }
    if (!fin) {
#pragma unroll
      for (int a = 0; a < NX; ++a) P.est_P[(bb * NX + a) * NX + j] = Pc[a];
    }
    if (j == 0) {
#pragma unroll
      for (int a = 0; a < NX; ++a) P.x0_est[bb * NX + a] = fin ? z[a] : x[a];
      P.nis[bb] = fin ? 0.0 : nis;
    }
    if (j == 1) {
#pragma unroll
      for (int a = 0; a < NX; ++a) P.innov[bb * NX + a] = fin ? 0.0 : nu[a];
    }
    if (j == 2 && !fin) {
#pragma unroll
      for (int a = 0; a < NX; ++a) P.est_x[bb * NX + a] = x[a];
      const bool rs = reset1 || reset2;
      P.est_count[2 * bb] = (rs ? 0 : cnt0) + 1;
      P.est_count[2 * bb + 1] = cnt1 + (reset1 ? 1 : 0) + (reset2 ? 1 : 0);
    }
    if (j == 3 && P.x_prior) {
#pragma unroll
      for (int a = 0; a < NX; ++a) P.x_prior[bb * NX + a] = fin ? z[a] : xm[a];
    }
  }
}

template <int NX> hipError_t estimate_launch(const ClEstimateParams& P, hipStream_t st, const double* par, int par_stride) {
  const dim3 grid((P.batch + CLE_CARS - 1) / CLE_CARS), block(64);
  if (par) hipLaunchKernelGGL((cl_estimate_kernel<NX, RtPar>), grid, block, 0, st, P, ParArgs{par, par_stride, nullptr});
  else hipLaunchKernelGGL((cl_estimate_kernel<NX, FixedPar>), grid, block, 0, st, P, NoParArgs{});
  return hipGetLastError();
}

}  // namespace

hipError_t cl_estimate_launch(const ClEstimateParams& P, hipStream_t st, const double* par, int par_stride) {
  if (P.batch == 0) return hipSuccess;
  return P.nx == 5 ? estimate_launch<5>(P, st, par, par_stride) : estimate_launch<7>(P, st, par, par_stride);
}
