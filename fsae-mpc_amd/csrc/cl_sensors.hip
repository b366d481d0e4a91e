// cl_sensors.hip -- Cartesian sensor models of the closed loop (no counterpart in main.m, which reads the exact state):
// the measurement a car takes of itself in the Cartesian frame, its naive projection onto the track, and the extended Kalman filter
// that reads the measurement through h(x) of cl_sensors.h.  The algorithms are stated in include/fsaempc.h
// (fsaempc_cl_sense_batch_device, fsaempc_cl_estimate_cart_batch_device); the scalar rules are those of cl_latency.h (draws,
// observation), cl_frame.h (the projection), cl_estimator.h (the filter's decisions) and cl_sensors.h (h, H, the heading wrap).
//
//   cl_sense_kernel          one thread per car, like the kernels of plant.hip and cl_latency.hip: y = y_true + sigma z, then x_proj =
//                            cl_pre_frame of the Cartesian vector y stands for, started at the true arc length.
//   cl_estimate_cart_kernel  the layout and the rules of cl_estimate_kernel (cl_estimator.hip): a group of 8 lanes per car, 8 cars per
//                            wavefront, lane j < NX owns column j of F, of P and of H = dh/dx(x-) (h on dual numbers seeded in state
//                            direction j).  Every __shfl(v, k, 8) runs with all 64 lanes active: no early return, every decision about
//                            a car is a select, the lanes past the last car read the last car and store nothing; the only branch
//                            around an exchange is taken by the whole wavefront at once.
//
// The update is linearised once at the prior and processed row by row.  Only rows and columns 0 .. 2 of H differ from the identity,
// and the kernel uses that: for a row i < 3 the vector c = P H_i' is a sum over three columns of P and s_i = H_i c + r_i a sum of three
// products, for a row i >= 3 c is column i of P and s_i = c_i + r_i as in cl_estimate_kernel.  Every lane of a group forms the same
// c from the same broadcasts in the same order, so P_ab and P_ba lose the same number and P stays exactly symmetric.
#include <hip/hip_runtime.h>
#include <math.h>
#include "cl_sensors.h"
#include "cl_cone_loc.h"
#include "cl_estimator.h"
#include "cl_latency.h"
#include "cl_frame.h"
#include "mpc_params.h"
#include "nlp_model.h"

namespace {

template <int NX> __global__ void __launch_bounds__(64) cl_sense_kernel(ClSenseParams P) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= P.batch) return;
  double c[7], yt[NX], xt[NX];
  for (int i = 0; i < 7; ++i) c[i] = P.cart[(size_t)b * 7 + i];
  for (int i = 0; i < NX; ++i) xt[i] = P.x0_true[(size_t)b * NX + i];
  cls_y_true(NX, c, yt);
  double* y = P.y + (size_t)b * NX;
  double* xp = P.x_proj + (size_t)b * NX;
  if (P.finished && P.finished[b]) {                 // out of the race or at the end of its run: exact measurement, true state
    for (int i = 0; i < NX; ++i) { y[i] = yt[i]; xp[i] = xt[i]; }
    return;
  }
  const double* sg = P.sigma + (P.sigma_per_instance ? (size_t)b * NX : (size_t)0);
  double s[NX], z[8], ym[NX];
  for (int i = 0; i < NX; ++i) s[i] = sg[i];
  cll_draws(P.seed, P.id0 + (unsigned long long)b, P.step, z);
  for (int i = 0; i < NX; ++i) { ym[i] = cll_observe(yt[i], s[i], z[i]); y[i] = ym[i]; }
  // the naive projection: the loop's own frame transform on the measured pose.  The start of the Newton search is the true arc
  // length (it selects the lap and the branch); the lap check of the transform is not used (no lap length: s >= Inf never holds)
  double cm[7], xq[NX];
  cls_cart_from_y(NX, ym, cm);
  const Spl sp{P.spM, P.spdl, P.xP, P.yP};
  int fin = 0;
  cl_pre_frame(sp, NX, INFINITY, cm, xt[0], xq, &fin);
  const bool lost = fin == 2;
  for (int i = 0; i < NX; ++i) xp[i] = lost ? xt[i] : xq[i];
  if (lost) P.proj_lost[b] += 1;
}

constexpr int CLS_GROUP = 8;        // lanes per car
constexpr int CLS_CARS = 64 / CLS_GROUP;
constexpr int CLS_KH = 3;           // rows and columns 0 .. 2 of H: the block that differs from the identity

// true in all 8 lanes of a group iff pred holds in one of them (one ballot of the whole wavefront, the group's byte cut out)
DEVINL bool cls_group_any(bool pred, int lane) {
  const unsigned long long m = __ballot(pred);
  return ((m >> (lane & 56)) & 0xffull) != 0ull;
}

// h(x) and, in lane j < NX, column j of H = dh/dx(x): rows 0 .. 2 in Hc (rows >= 3 are rows of the identity)
template <int NX> DEVINL void cls_linearise(const ClEstimateCartParams& P, int j, const double (&x)[NX], double (&h)[NX], double (&Hc)[CLS_KH]) {
  ClsD xd[NX], hd[NX];
#pragma unroll
  for (int i = 0; i < NX; ++i) xd[i] = cls_mk(x[i], i == j ? 1.0 : 0.0);
  cls_h<ClsD>(P.spM, P.spdl, P.xP, P.yP, NX, xd, hd);
#pragma unroll
  for (int i = 0; i < NX; ++i) h[i] = hd[i].v;
#pragma unroll
  for (int i = 0; i < CLS_KH; ++i) Hc[i] = hd[i].d;
}

// The row-by-row update on the prior (x, column j of P in Pc), linearised at it: nu0 = y - h(x-) (heading wrapped), H rows 0 .. 2 from
// the lanes 0 .. 2 of the group.  For every measured component i: nu_i = nu0_i - H_i (x - x-), c = P H_i', s_i = H_i c + r_i, and with
// s_i > 0: x += c nu_i / s_i, P_ab -= (c_a c_b) / s_i.  x is the same in all lanes of the group.
template <int NX> DEVINL void cls_update(int j, const double (&y)[NX], const double (&r)[NX], const double (&h)[NX], const double (&Hc)[CLS_KH],
                                         double (&x)[NX], double (&Pc)[NX], double (&nu)[NX], double& nis) {
#pragma clang fp contract(off)
  double Hr[CLS_KH][CLS_KH], xm[NX], nu0[NX];
#pragma unroll
  for (int i = 0; i < CLS_KH; ++i)
#pragma unroll
    for (int k = 0; k < CLS_KH; ++k) Hr[i][k] = __shfl(Hc[i], k, CLS_GROUP);
#pragma unroll
  for (int a = 0; a < NX; ++a) { xm[a] = x[a]; nu0[a] = (a == 2) ? cls_angdiff(h[a], y[a]) : y[a] - h[a]; }
  nis = 0.0;
#pragma unroll
  for (int i = 0; i < NX; ++i) {
    double c[NX], v, s;
    if (i < CLS_KH) {
#pragma unroll
      for (int a = 0; a < NX; ++a) {
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < CLS_KH; ++k) acc += __shfl(Pc[a], k, CLS_GROUP) * Hr[i][k];
        c[a] = acc;
      }
      double hx = 0.0, hc = 0.0;
#pragma unroll
      for (int k = 0; k < CLS_KH; ++k) { hx += Hr[i][k] * (x[k] - xm[k]); hc += Hr[i][k] * c[k]; }
      v = nu0[i] - hx; s = hc + r[i];
    } else {
#pragma unroll
      for (int a = 0; a < NX; ++a) c[a] = __shfl(Pc[a], i, CLS_GROUP);
      v = nu0[i] - (x[i] - xm[i]); s = c[i] + r[i];
    }
    double cj = 0.0;                                      // c[j] without indexing a register array by the lane
#pragma unroll
    for (int a = 0; a < NX; ++a) cj = (a == j) ? c[a] : cj;
    const bool meas = cle_measured(r[i]) != 0;
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

template <int NX, class PAR> __global__ void __launch_bounds__(64) cl_estimate_cart_kernel(ClEstimateCartParams P, typename PAR::Args pa) {
  const int lane = threadIdx.x, j = lane & (CLS_GROUP - 1);
  const int b = blockIdx.x * CLS_CARS + (lane >> 3);
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

  double y[NX], r[NX], p0[NX], xq[NX], Pc[NX];
  const double* rp = P.r + (P.r_per_instance ? bb * NX : (size_t)0);
#pragma unroll
  for (int i = 0; i < NX; ++i) {
    y[i] = P.y[bb * NX + i]; xq[i] = P.x_proj[bb * NX + i]; r[i] = rp[i]; p0[i] = P.p0[i];
    const double pv = P.est_P[(bb * NX + i) * NX + jc];
    Pc[i] = col ? pv : 0.0;
  }
  const double qv = P.q[(P.q_per_instance ? bb * NX : (size_t)0) + jc];
  const double qj = col ? qv : 0.0;
  const int cnt0 = P.est_count[2 * bb], cnt1 = P.est_count[2 * bb + 1];
  const bool fin = P.finished != nullptr && P.finished[bb] != 0;

  const bool first = cnt0 == 0;                           // the car's first period: the prior is (x_proj, diag(p0)), F = I
  double xm[NX], Fc[NX];
#pragma unroll
  for (int a = 0; a < NX; ++a) {
    xm[a] = first ? xq[a] : xn[a].v;
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
      const double t = __shfl(Fc[a], k, CLS_GROUP);
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
    for (int k = 0; k < NX; ++k) Mc[a] += __shfl(FP[a], k, CLS_GROUP) * Fr[k];
  // row j of M, then P- = (M + M') / 2 + diag(q): entries (a, j) and (j, a) add the same two numbers
#pragma unroll
  for (int a = 0; a < NX; ++a)
#pragma unroll
    for (int k = 0; k < NX; ++k) {
      const double t = __shfl(Mc[a], k, CLS_GROUP);
      Mr[k] = (a == j) ? t : Mr[k];
    }
  double Pm[NX];
#pragma unroll
  for (int a = 0; a < NX; ++a) {
    const double hm = 0.5 * (Mc[a] + Mr[a]);
    const double pred = (a == j) ? hm + qj : hm;
    const double init = (a == j && col) ? p0[a] : 0.0;
    Pm[a] = first ? init : pred;
  }

  // re-initialisation before the update: the block, the input, x- or P- cannot be used
#pragma unroll
  for (int a = 0; a < NX; ++a) bad = bad || !cle_finite(xm[a]) || (col && cle_prior_bad(Pm[a], a == j));
  const bool reset1 = cls_group_any(bad, lane);
#pragma unroll
  for (int a = 0; a < NX; ++a) {
    xm[a] = reset1 ? xq[a] : xm[a];
    Pm[a] = reset1 ? ((a == j && col) ? p0[a] : 0.0) : Pm[a];
  }
  xm[0] = cle_rebase(xm[0], xq[0], P.L, 1);               // (the projection always carries an arc length)

  double h[NX], Hc[CLS_KH];
  cls_linearise<NX>(P, j, xm, h, Hc);
  double x[NX], nu[NX], nis;
#pragma unroll
  for (int a = 0; a < NX; ++a) { x[a] = xm[a]; Pc[a] = Pm[a]; }
  cls_update<NX>(j, y, r, h, Hc, x, Pc, nu, nis);
  bool pb = false;
#pragma unroll
  for (int a = 0; a < NX; ++a) pb = pb || !cle_finite(x[a]) || (col && cle_post_bad(Pc[a], a == j));
  const bool reset2 = cls_group_any(pb, lane);
  if (__ballot(reset2) != 0ull) {                         // (the same in all 64 lanes) some car's update failed: x- = x_proj, P- = diag(p0) again
    double x2[NX], P2[NX], nu2[NX], nis2, h2[NX], Hc2[CLS_KH];
#pragma unroll
    for (int a = 0; a < NX; ++a) { x2[a] = xq[a]; P2[a] = (a == j && col) ? p0[a] : 0.0; }
    cls_linearise<NX>(P, j, x2, h2, Hc2);
    cls_update<NX>(j, y, r, h2, Hc2, x2, P2, nu2, nis2);
#pragma unroll
    for (int a = 0; a < NX; ++a) {
      x[a] = reset2 ? x2[a] : x[a]; Pc[a] = reset2 ? P2[a] : Pc[a]; nu[a] = reset2 ? nu2[a] : nu[a];
    }
#pragma unroll
    for (int a = 0; a < CLS_KH; ++a) Hc[a] = reset2 ? Hc2[a] : Hc[a];
    nis = reset2 ? nis2 : nis;
  }

  // stores: lane j < NX writes column j of the matrices, lanes 0 .. 3 one vector each (no register array is indexed by the lane)
  if (live && col) {
    if (P.F_out) {
#pragma unroll
      for (int a = 0; a < NX; ++a) P.F_out[(bb * NX + a) * NX + j] = fin ? (a == j ? 1.0 : 0.0) : Fc[a];
    }
    if (P.H_out) {
#pragma unroll
      for (int a = 0; a < NX; ++a) {
        const double id = a == j ? 1.0 : 0.0;
        P.H_out[(bb * NX + a) * NX + j] = (fin || a >= CLS_KH) ? id : Hc[a < CLS_KH ? a : 0];
      }
    }
    if (!fin) {
#pragma unroll
      for (int a = 0; a < NX; ++a) P.est_P[(bb * NX + a) * NX + j] = Pc[a];
    }
    if (j == 0) {
#pragma unroll
      for (int a = 0; a < NX; ++a) P.x0_est[bb * NX + a] = fin ? xq[a] : x[a];
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
      for (int a = 0; a < NX; ++a) P.x_prior[bb * NX + a] = fin ? xq[a] : xm[a];
    }
  }
}

template <int NX> hipError_t estimate_cart_launch(const ClEstimateCartParams& P, hipStream_t st, const double* par, int par_stride) {
  const dim3 grid((P.batch + CLS_CARS - 1) / CLS_CARS), block(64);
  if (par) hipLaunchKernelGGL((cl_estimate_cart_kernel<NX, RtPar>), grid, block, 0, st, P, ParArgs{par, par_stride, nullptr});
  else hipLaunchKernelGGL((cl_estimate_cart_kernel<NX, FixedPar>), grid, block, 0, st, P, NoParArgs{});
  return hipGetLastError();
}

}  // namespace

hipError_t cl_sense_launch(const ClSenseParams& P, hipStream_t st) {
  if (P.batch == 0) return hipSuccess;
  const dim3 grid((P.batch + 63) / 64), block(64);
  if (P.nx == 5) hipLaunchKernelGGL((cl_sense_kernel<5>), grid, block, 0, st, P);
  else hipLaunchKernelGGL((cl_sense_kernel<7>), grid, block, 0, st, P);
  return hipGetLastError();
}

hipError_t cl_estimate_cart_launch(const ClEstimateCartParams& P, hipStream_t st, const double* par, int par_stride) {
  if (P.batch == 0) return hipSuccess;
  return P.nx == 5 ? estimate_cart_launch<5>(P, st, par, par_stride) : estimate_cart_launch<7>(P, st, par, par_stride);
}

/* ---- cone-based localisation ----
 * cl_estimate_cones_kernel is cl_estimate_cart_kernel with the rows of the cone observations behind the car's own rows: the same layout
 * (8 lanes per car, lane j owns column j), the same discipline (every __shfl(v, k, 8) and every ballot with all 64 lanes active, no
 * early return, every decision about a car a select, the batch tail reads the last car and stores nothing, no register array indexed
 * by the lane), and prediction, first prior, reset rules and re-basing stated exactly as there.  clc_update is cls_update's loop over the
 * own rows, counting the rows applied, followed by the cone rows.  A cone row G has three non-zero entries like an own row i < 3; with P
 * exactly symmetric, lane j forms c_j = sum_k P[k][j] G[k] out of its own column and the group exchanges the c_a -- NX broadcasts per row
 * instead of 3 NX -- so all lanes hold the same c, P_ab and P_ba lose the same number and P stays exactly symmetric.  The loop over the
 * observations runs k_max times in every lane; the work of a round is skipped by the whole wavefront when none of its 8 cars has an
 * observation k (one ballot), and a car without one passes through the round as selects. */
namespace {

template <int NX> DEVINL void clc_update(const ClEstimateConesParams& P, size_t bb, int j, int cn, bool store, const double (&y)[NX], const double (&r)[NX],
                                         const double (&h)[NX], const double (&Hc)[CLS_KH], double (&x)[NX], double (&Pc)[NX], double (&nu)[NX],
                                         double& nis, int& rows) {
#pragma clang fp contract(off)
  double Hr[CLS_KH][CLS_KH], xm[NX], nu0[NX];
#pragma unroll
  for (int i = 0; i < CLS_KH; ++i)
#pragma unroll
    for (int k = 0; k < CLS_KH; ++k) Hr[i][k] = __shfl(Hc[i], k, CLS_GROUP);
#pragma unroll
  for (int a = 0; a < NX; ++a) { xm[a] = x[a]; nu0[a] = (a == 2) ? cls_angdiff(h[a], y[a]) : y[a] - h[a]; }
  nis = 0.0; rows = 0;
  // the car's own rows: the loop of cls_update
#pragma unroll
  for (int i = 0; i < NX; ++i) {
    double c[NX], v, s;
    if (i < CLS_KH) {
#pragma unroll
      for (int a = 0; a < NX; ++a) {
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < CLS_KH; ++k) acc += __shfl(Pc[a], k, CLS_GROUP) * Hr[i][k];
        c[a] = acc;
      }
      double hx = 0.0, hc = 0.0;
#pragma unroll
      for (int k = 0; k < CLS_KH; ++k) { hx += Hr[i][k] * (x[k] - xm[k]); hc += Hr[i][k] * c[k]; }
      v = nu0[i] - hx; s = hc + r[i];
    } else {
#pragma unroll
      for (int a = 0; a < NX; ++a) c[a] = __shfl(Pc[a], i, CLS_GROUP);
      v = nu0[i] - (x[i] - xm[i]); s = c[i] + r[i];
    }
    double cj = 0.0;                                      // c[j] without indexing a register array by the lane
#pragma unroll
    for (int a = 0; a < NX; ++a) cj = (a == j) ? c[a] : cj;
    const bool meas = cle_measured(r[i]) != 0;
    const bool on = meas && cle_gain_ok(s);
    nu[i] = meas ? v : 0.0;
    nis = on ? nis + v * v / s : nis;
    rows = on ? rows + 1 : rows;
#pragma unroll
    for (int a = 0; a < NX; ++a) {
      x[a] = on ? x[a] + c[a] * v / s : x[a];
      Pc[a] = on ? Pc[a] - (c[a] * cj) / s : Pc[a];
    }
  }
  // the cone rows, linearised at the same prior: per kept cone its range row, then its bearing row
  const int ntot = P.map.n_left + P.map.n_right;
  for (int k = 0; k < P.k_max; ++k) {
    const bool have = k < cn;
    const size_t o = bb * (size_t)P.k_max + (size_t)k;
    double inn[2] = {0.0, 0.0}, Gs[2][CLS_KH] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    if (__ballot(have) != 0ull) {                         // (the same in all 64 lanes)
      const int id = P.cone_id[o];
      const double zr = P.cone_z[2 * o], zb = P.cone_z[2 * o + 1];
      const bool known = have && id >= 0 && id < ntot;
      double mx, my, G[2][CLS_KH], n0[2], rho_hat;
      clc_cone_at(P.map, bb, known ? id : 0, mx, my);
      clc_rows(h[0], h[1], h[2], Hr, mx, my, zr, zb, G, n0, rho_hat);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        double cj = 0.0;                                  // c_j = sum_k P[k][j] G[k]: column j of P is row j
#pragma unroll
        for (int q = 0; q < CLS_KH; ++q) cj += Pc[q] * G[i][q];
        double c[NX];
#pragma unroll
        for (int a = 0; a < NX; ++a) c[a] = __shfl(cj, a, CLS_GROUP);
        double hx = 0.0, hc = 0.0;
#pragma unroll
        for (int q = 0; q < CLS_KH; ++q) { hx += G[i][q] * (x[q] - xm[q]); hc += G[i][q] * c[q]; }
        const double v = n0[i] - hx, s = hc + P.r_cone[i];
        const bool on = known && rho_hat > 0.0 && cle_measured(P.r_cone[i]) != 0 && cle_gain_ok(s);
        inn[i] = on ? v : 0.0;
        nis = on ? nis + v * v / s : nis;
        rows = on ? rows + 1 : rows;
#pragma unroll
        for (int a = 0; a < NX; ++a) {
          x[a] = on ? x[a] + c[a] * v / s : x[a];
          Pc[a] = on ? Pc[a] - (c[a] * cj) / s : Pc[a];
        }
#pragma unroll
        for (int q = 0; q < CLS_KH; ++q) Gs[i][q] = on ? G[i][q] : 0.0;
      }
    }
    if (store && j == 4) {                                // (lane 4 owns a column in both models)
      P.cone_innov[2 * o] = inn[0]; P.cone_innov[2 * o + 1] = inn[1];
      if (P.G_out) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int q = 0; q < CLS_KH; ++q) P.G_out[(2 * o + i) * CLS_KH + q] = Gs[i][q];
      }
    }
  }
}

template <int NX, class PAR> __global__ void __launch_bounds__(64) cl_estimate_cones_kernel(ClEstimateConesParams PC, typename PAR::Args pa) {
  const ClEstimateCartParams& P = PC.E;
  const int lane = threadIdx.x, j = lane & (CLS_GROUP - 1);
  const int b = blockIdx.x * CLS_CARS + (lane >> 3);
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

  double y[NX], r[NX], p0[NX], xq[NX], Pc[NX];
  const double* rp = P.r + (P.r_per_instance ? bb * NX : (size_t)0);
#pragma unroll
  for (int i = 0; i < NX; ++i) {
    y[i] = P.y[bb * NX + i]; xq[i] = P.x_proj[bb * NX + i]; r[i] = rp[i]; p0[i] = P.p0[i];
    const double pv = P.est_P[(bb * NX + i) * NX + jc];
    Pc[i] = col ? pv : 0.0;
  }
  const double qv = P.q[(P.q_per_instance ? bb * NX : (size_t)0) + jc];
  const double qj = col ? qv : 0.0;
  const int cnt0 = P.est_count[2 * bb], cnt1 = P.est_count[2 * bb + 1];
  const bool fin = P.finished != nullptr && P.finished[bb] != 0;
  const int cn_in = PC.cone_n[bb];
  const int cn = fin ? 0 : (cn_in < 0 ? 0 : (cn_in > PC.k_max ? PC.k_max : cn_in));   // a finished car has no observation to process

  const bool first = cnt0 == 0;                           // the car's first period: the prior is (x_proj, diag(p0)), F = I
  double xm[NX], Fc[NX];
#pragma unroll
  for (int a = 0; a < NX; ++a) {
    xm[a] = first ? xq[a] : xn[a].v;
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
      const double t = __shfl(Fc[a], k, CLS_GROUP);
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
    for (int k = 0; k < NX; ++k) Mc[a] += __shfl(FP[a], k, CLS_GROUP) * Fr[k];
  // row j of M, then P- = (M + M') / 2 + diag(q): entries (a, j) and (j, a) add the same two numbers
#pragma unroll
  for (int a = 0; a < NX; ++a)
#pragma unroll
    for (int k = 0; k < NX; ++k) {
      const double t = __shfl(Mc[a], k, CLS_GROUP);
      Mr[k] = (a == j) ? t : Mr[k];
    }
  double Pm[NX];
#pragma unroll
  for (int a = 0; a < NX; ++a) {
    const double hm = 0.5 * (Mc[a] + Mr[a]);
    const double pred = (a == j) ? hm + qj : hm;
    const double init = (a == j && col) ? p0[a] : 0.0;
    Pm[a] = first ? init : pred;
  }

  // re-initialisation before the update: the block, the input, x- or P- cannot be used
#pragma unroll
  for (int a = 0; a < NX; ++a) bad = bad || !cle_finite(xm[a]) || (col && cle_prior_bad(Pm[a], a == j));
  const bool reset1 = cls_group_any(bad, lane);
#pragma unroll
  for (int a = 0; a < NX; ++a) {
    xm[a] = reset1 ? xq[a] : xm[a];
    Pm[a] = reset1 ? ((a == j && col) ? p0[a] : 0.0) : Pm[a];
  }
  xm[0] = cle_rebase(xm[0], xq[0], P.L, 1);               // (the projection always carries an arc length)

  double h[NX], Hc[CLS_KH];
  cls_linearise<NX>(P, j, xm, h, Hc);
  double x[NX], nu[NX], nis;
  int rows;
#pragma unroll
  for (int a = 0; a < NX; ++a) { x[a] = xm[a]; Pc[a] = Pm[a]; }
  clc_update<NX>(PC, bb, j, cn, live, y, r, h, Hc, x, Pc, nu, nis, rows);
  bool pb = false;
#pragma unroll
  for (int a = 0; a < NX; ++a) pb = pb || !cle_finite(x[a]) || (col && cle_post_bad(Pc[a], a == j));
  const bool reset2 = cls_group_any(pb, lane);
  if (__ballot(reset2) != 0ull) {                         // (the same in all 64 lanes) some car's update failed: x- = x_proj, P- = diag(p0) again
    double x2[NX], P2[NX], nu2[NX], nis2, h2[NX], Hc2[CLS_KH];
    int rows2;
#pragma unroll
    for (int a = 0; a < NX; ++a) { x2[a] = xq[a]; P2[a] = (a == j && col) ? p0[a] : 0.0; }
    cls_linearise<NX>(P, j, x2, h2, Hc2);
    clc_update<NX>(PC, bb, j, cn, live && reset2, y, r, h2, Hc2, x2, P2, nu2, nis2, rows2);   // (its cone outputs replace the first run's)
#pragma unroll
    for (int a = 0; a < NX; ++a) {
      x[a] = reset2 ? x2[a] : x[a]; Pc[a] = reset2 ? P2[a] : Pc[a]; nu[a] = reset2 ? nu2[a] : nu[a];
    }
#pragma unroll
    for (int a = 0; a < CLS_KH; ++a) Hc[a] = reset2 ? Hc2[a] : Hc[a];
    nis = reset2 ? nis2 : nis;
    rows = reset2 ? rows2 : rows;
  }

  // stores: lane j < NX writes column j of the matrices, lanes 0 .. 3 one vector each (no register array is indexed by the lane)
  if (live && col) {
    if (P.F_out) {
#pragma unroll
      for (int a = 0; a < NX; ++a) P.F_out[(bb * NX + a) * NX + j] = fin ? (a == j ? 1.0 : 0.0) : Fc[a];
    }
    if (P.H_out) {
#pragma unroll
      for (int a = 0; a < NX; ++a) {
        const double id = a == j ? 1.0 : 0.0;
        P.H_out[(bb * NX + a) * NX + j] = (fin || a >= CLS_KH) ? id : Hc[a < CLS_KH ? a : 0];
      }
    }
    if (!fin) {
#pragma unroll
      for (int a = 0; a < NX; ++a) P.est_P[(bb * NX + a) * NX + j] = Pc[a];
    }
    if (j == 0) {
#pragma unroll
      for (int a = 0; a < NX; ++a) P.x0_est[bb * NX + a] = fin ? xq[a] : x[a];
      P.nis[bb] = fin ? 0.0 : nis;
      PC.rows_used[bb] = fin ? 0 : rows;
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
      for (int a = 0; a < NX; ++a) P.x_prior[bb * NX + a] = fin ? xq[a] : xm[a];
    }
  }
}

template <int NX> hipError_t estimate_cones_launch(const ClEstimateConesParams& P, hipStream_t st, const double* par, int par_stride) {
  const dim3 grid((P.E.batch + CLS_CARS - 1) / CLS_CARS), block(64);
  if (par) hipLaunchKernelGGL((cl_estimate_cones_kernel<NX, RtPar>), grid, block, 0, st, P, ParArgs{par, par_stride, nullptr});
  else hipLaunchKernelGGL((cl_estimate_cones_kernel<NX, FixedPar>), grid, block, 0, st, P, NoParArgs{});
  return hipGetLastError();
}

}  // namespace

hipError_t cl_estimate_cones_launch(const ClEstimateConesParams& P, hipStream_t st, const double* par, int par_stride) {
  if (P.E.batch == 0) return hipSuccess;
  return P.E.nx == 5 ? estimate_cones_launch<5>(P, st, par, par_stride) : estimate_cones_launch<7>(P, st, par, par_stride);
}
