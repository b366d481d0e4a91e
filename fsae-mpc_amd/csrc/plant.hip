// plant.hip -- the closed loop around the LTV-MPC step, batched on the device (one thread per car:
// every piece is a short scalar recurrence, the batch of independent cars is the parallel axis).
//
//   cl_pre_kernel    main.m:93-114  Cartesian -> curvilinear frame (vehicle_models/cartesian_to_curvilinear.m:17-26 with
//                    the Newton search of spline/closest_point.m:15-32, epsilon 0.01, started from the first predicted
//                    state), x0 assembly for the kinematic / dynamic model, lap check (s >= L), live reference
//   cl_plant_kernel  main.m:163-175 first predicted state -> set points; ten sub-steps of the two PID actuator loops
//                    (vehicle_models/pid_controller.m:5-18, gains main.m:84-88) driving the Cartesian dynamic bicycle
//                    (cartesian_dynamic/f_cart_dyn.m:13-54) through the 6-stage scheme of integrate_cart_dyn.m:12-22
//                    (stage formulas exactly as written there, including the doubled k2 term of k5)
//   cl_metrics_kernel main.m:196-228 the lap report's figures, accumulated per car after every period (opt-in); corridor.hip's
//                    cor_metrics_kernel repeats its text with another track violation: a change here belongs there too
//   cl_lap_gate_kernel (no counterpart: main.m:102-104 ends the run at the line) multi-lap driving, opt-in, between cl_pre and the
//                    step: sub-period crossing time, per-lap times, the lap's record handed over, s wrapped by L
#include <hip/hip_runtime.h>
#include <math.h>
#include "plant.h"
#include "mpc_params.h"
#include "cl_frame.h"

namespace {

__global__ void cl_pre_kernel(ClPreParams P) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= P.batch) return;
  const Spl sp{P.spM, P.spdl, P.xP, P.yP};
  const int nx = P.nx, N = P.N;
  const double* c = P.cart + (size_t)b * 7;
  double* x0 = P.x0 + (size_t)b * nx;
  double* xr = P.x_ref + (size_t)b * nx * N;
  const double s = closest_point(sp, c[0], c[1], P.s_guess[b], 0.01);
  double X, Xd, Xdd, Y, Yd, Ydd;
  spline3(sp.xP, sp.M, sp.dl, s, X, Xd, Xdd);
  spline3(sp.yP, sp.M, sp.dl, s, Y, Yd, Ydd);
  double tx = -Yd, ty = Xd;
  const double nrm = sqrt(tx * tx + ty * ty);
  tx /= nrm; ty /= nrm;
  const double n = (c[0] - X) * tx + (c[1] - Y) * ty;
  const double mu = angdiff(atan2(Yd, Xd), c[2]);
  x0[0] = s; x0[1] = n; x0[2] = mu;
  if (nx == 5) { x0[3] = sqrt(c[3] * c[3] + c[4] * c[4]); x0[4] = c[6]; }   // main.m:95
  else { x0[3] = c[3]; x0[4] = c[4]; x0[5] = c[5]; x0[6] = c[6]; }           // main.m:97
  if (s >= P.L) P.finished[b] = 1;                                           // main.m:101-104
  {   // the car is out when the frame transform lost the track (Newton diverged) or its state left every physical range
    bool okc = fabs(s) < INFINITY && fabs(n) < 3.0 && fabs(c[3]) < 100.0 && fabs(c[4]) < 100.0;   // 3 m off a 1.5 m wide track: out of the race
    for (int j = 0; j < 7; ++j) okc = okc && fabs(c[j]) < 1e6;
    if (!okc) {
      P.finished[b] = 2;
      for (int j = 0; j < nx; ++j) x0[j] = 0.0;   // finite placeholder data for the (ignored) QP of this car
    }
  }
  double cum = 0.0;
  for (int k = 0; k < N; ++k) {                                              // main.m:107-114
    for (int j = 0; j < nx; ++j) xr[k * nx + j] = 0.0;
    double v;
    if (c[3] < P.target_vel) { v = x0[3] + 10 * P.dt * (k + 1); if (v > P.target_vel) v = P.target_vel; }
    else                     { v = x0[3] - 10 * P.dt * (k + 1); if (v < P.target_vel) v = P.target_vel; }
    xr[k * nx + 3] = v;
    cum += v * P.dt;
    xr[k * nx + 0] = x0[0] + cum;
  }
}

// (the car's constants come from a policy object p, mpc_params.h: FixedPar = f_cart_dyn.m's own, RtPar = the car's block)
template <class PAR> DEVINL void f_cart_dyn(const PAR p, const double* x, const double* u, double* f) {
  const double m = p.M, I = p.IZ, lr = p.LR, lf = p.LF;
  const double theta = x[2], x_d = x[3], y_d = x[4], theta_d = x[5], delta = x[6];
  const double alpha_f = delta - atan((y_d + lf * theta_d) / (x_d + 0.01));
  const double alpha_r = -atan((y_d - lr * theta_d) / (x_d + 0.01));
  const double Fzf = p.FZF, Fzr = p.FZR;
  const double B = p.PB, C = p.PC, D = p.PD, E = p.PE;
  const double Fcf = Fzf * D * sin(C * atan(B * alpha_f - E * (B * alpha_f - atan(B * alpha_f))));
  const double Fcr = Fzr * D * sin(C * atan(B * alpha_r - E * (B * alpha_r - atan(B * alpha_r))));
  f[0] = x_d * cos(theta) - y_d * sin(theta);
  f[1] = x_d * sin(theta) + y_d * cos(theta);
  f[2] = theta_d;
  f[3] = (u[0] - Fcf * sin(delta) + m * y_d * theta_d) / m;
  f[4] = (Fcr + Fcf * cos(delta) - m * x_d * theta_d) / m;
  f[5] = (lf * Fcf * cos(delta) - lr * Fcr) / I;
  f[6] = u[1];
}

template <class PAR> DEVINL void integrate_cart_dyn(const PAR p, double* x, const double* u, double dt) {
  double k1[7], k2[7], k3[7], k4[7], k5[7], k6[7], xs[7];
  f_cart_dyn(p, x, u, k1);
  for (int i = 0; i < 7; ++i) xs[i] = x[i] + k1[i] * dt / 2;
  f_cart_dyn(p, xs, u, k2);
  for (int i = 0; i < 7; ++i) xs[i] = x[i] + k1[i] * dt / 4 + k2[i] * dt / 8;
  f_cart_dyn(p, xs, u, k3);
  for (int i = 0; i < 7; ++i) xs[i] = x[i] - k2[i] * dt + 2 * k3[i] * dt;
  f_cart_dyn(p, xs, u, k4);
  for (int i = 0; i < 7; ++i) xs[i] = x[i] + 7.0 / 27 * k2[i] * dt + 10.0 / 27 * k2[i] * dt + k4[i] * dt / 27;
  f_cart_dyn(p, xs, u, k5);
  for (int i = 0; i < 7; ++i)
    xs[i] = x[i] + 28.0 / 625 * k1[i] * dt - k2[i] * dt / 5 + 546.0 / 625 * k3[i] * dt + 54.0 / 625 * k4[i] * dt - 378.0 / 625 * k5[i] * dt;
  f_cart_dyn(p, xs, u, k6);
  for (int i = 0; i < 7; ++i) x[i] = x[i] + dt * (k1[i] / 24 + 5.0 / 48 * k4[i] + 27.0 / 56 * k5[i] + 125.0 / 336 * k6[i]);
}

DEVINL double pid(double target, double current, double kp, double ki, double kd, double max_output, double* status) {
  const double error = target - current;
  const double integral_error = status[0] + error;
  const double derivative_error = error - status[1];
  double output = kp * error + ki * integral_error + kd * derivative_error;
  output = fmax(fmin(output, max_output), -max_output);
  status[0] = integral_error; status[1] = error;
  return output;
}

// PAR = RtPar: car b drives with the block pa.values + b * pa.stride (one car per lane: per-lane loads); a block that cannot
// describe a car holds it.
template <class PAR> __global__ void cl_plant_kernel(ClPlantParams P, typename PAR::Args pa) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= P.batch) return;
  PAR p;
  if constexpr (PAR::RT) {
    p = par_load(pa.values + (size_t)b * (size_t)pa.stride);
    if (p.bad) return;
  }
  if (P.finished && P.finished[b]) return;        // the reference leaves the loop when the lap is complete
  // The reference keeps driving on whatever plan the solver returned, whatever its exit flag (main.m:163-175); `exitflag`
  // (optional) only holds a car when the caller asks for it with a flag < -100 (not a solver outcome).
  if (P.exitflag && P.exitflag[b] < -100) return;
  double x[7], st[4], u[2] = {0.0, 0.0};
  for (int i = 0; i < 7; ++i) x[i] = P.cart[(size_t)b * 7 + i];
  for (int i = 0; i < 4; ++i) st[i] = P.pid[(size_t)b * 4 + i];
  const double* xo = P.x_opt + (size_t)b * P.nx * P.N;
  const double v_ref = xo[3], delta_ref = xo[P.nx - 1];     // main.m:167-168 (x_opt(4), x_opt(N_x))
  if (!(fabs(v_ref) < INFINITY) || !(fabs(delta_ref) < INFINITY)) return;   // no finite plan at all: hold the car
  for (int j = 0; j < 10; ++j) {                             // main.m:171-175
    u[0] = pid(v_ref, x[3], p.PID_KP_V, 0.0, 0.0, p.PID_MAX_F, st);
    u[1] = pid(delta_ref, x[6], p.PID_KP_D, 0.0, 0.0, p.PID_MAX_DRATE, st + 2);
    integrate_cart_dyn(p, x, u, P.dt / 10);
  }
  for (int i = 0; i < 7; ++i) P.cart[(size_t)b * 7 + i] = x[i];
  for (int i = 0; i < 4; ++i) P.pid[(size_t)b * 4 + i] = st[i];
  if (P.u_last) { P.u_last[(size_t)b * 2] = u[0]; P.u_last[(size_t)b * 2 + 1] = u[1]; }
}

// main.m:122-126: the plan of this step becomes the linearisation point (and the source of the set points) of the next
// one.  The reference takes over whatever qpOASES returned; this build takes a plan over when the solve ended with exit
// flag 0 or 1 and every entry is finite -- after an abnormal exit (-1, -2) the returned point is the last interior-point
// iterate, which unlike an active-set iterate need not respect the actuator bounds, so the car keeps driving on its last
// good plan instead (documented deviation).
__global__ void cl_accept_kernel(int len_x, int len_u, int batch, const double* x_new, const double* u_new, const int* exitflag, double* x_keep, double* u_keep) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= batch) return;
  bool ok = !exitflag || exitflag[b] == 0 || exitflag[b] == 1;
  for (int i = 0; i < len_x; ++i) ok = ok && fabs(x_new[(size_t)b * len_x + i]) < INFINITY;
  for (int i = 0; i < len_u; ++i) ok = ok && fabs(u_new[(size_t)b * len_u + i]) < INFINITY;
  if (!ok) return;
  for (int i = 0; i < len_x; ++i) x_keep[(size_t)b * len_x + i] = x_new[(size_t)b * len_x + i];
  for (int i = 0; i < len_u; ++i) u_keep[(size_t)b * len_u + i] = u_new[(size_t)b * len_u + i];
}

// main.m:196-228 per car, one MPC period at a time (include/fsaempc.h FSAEMPC_M_*).  Runs after the plant; `finished` is
// what cl_pre left.  Every slot is a count, a maximum or a sum in step order, so a record depends only on the car's own history.
template <class PAR> __global__ void cl_metrics_kernel(ClMetricsParams P, typename PAR::Args pa) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= P.batch) return;
  PAR p;
  if constexpr (PAR::RT) {
    p = par_load(pa.values + (size_t)b * (size_t)pa.stride);
    if (p.bad) return;
  }
  double* m = P.metrics + (size_t)b * FSAEMPC_NMETRIC;
  if (m[FSAEMPC_M_STATUS] != 0.0) return;                     // latched: later steps touch nothing
  const int fin = P.finished[b];
  if (fin == 2) { m[FSAEMPC_M_STATUS] = 2.0; return; }        // lost: x0 is a placeholder
  const double s = P.x0[(size_t)b * P.nx], an = fabs(P.x0[(size_t)b * P.nx + 1]);
  if (an > m[FSAEMPC_M_N_ABS_MAX]) m[FSAEMPC_M_N_ABS_MAX] = an;                 // main.m:101: n_list(i) precedes the lap check
  if (an > p.N_MAX) {                                                           // main.m:204-205
    const double v = an - p.N_MAX;
    m[FSAEMPC_M_N_VIOL_INT] += v * P.dt;
    if (v > m[FSAEMPC_M_N_VIOL_MAX]) m[FSAEMPC_M_N_VIOL_MAX] = v;
  }
  if (fin != 0) { m[FSAEMPC_M_STATUS] = 1.0; return; }        // main.m:102-104: the break; i - 1 steps were solved
  if (m[FSAEMPC_M_STEPS] == 0.0) m[FSAEMPC_M_S_START] = s;
  m[FSAEMPC_M_S_LAST] = s;
  m[FSAEMPC_M_STEPS] += 1.0;
  const int ef = P.exitflag[b];
  if (ef != 0) m[FSAEMPC_M_ABNORMAL] += 1.0;                                    // main.m:209
  const double it = (double)P.iter[b];
  m[FSAEMPC_M_ITER_SUM] += it;
  if (it > m[FSAEMPC_M_ITER_MAX]) m[FSAEMPC_M_ITER_MAX] = it;
  const bool use_n = P.slack[(size_t)b * P.ns] > P.slack_tol;                   // main.m:132-133 (NaN: not in use)
  const bool use_t = P.slack[(size_t)b * P.ns + P.tyre] > P.slack_tol;
  if (use_n) m[FSAEMPC_M_SLACK_N_CNT] += 1.0;
  if (use_t) m[FSAEMPC_M_SLACK_TYRE_CNT] += 1.0;
  if (ef == 0 && !use_n && !use_t) { m[FSAEMPC_M_OBJ_SUM] += P.fval[b]; m[FSAEMPC_M_OBJ_CNT] += 1.0; }   // main.m:198, 210
  // main.m:180-182, 199: rear lateral force of f_curv_dyn.m:32-53 at the post-plant state, acceleration of the driven plan
  const double* c = P.cart + (size_t)b * 7;
  const double x_d = c[3], y_d = c[4], theta_d = c[5];
  const double x_d_hat = x_d + 5 * exp(-x_d / 5);
  const double alpha_r = -atan((y_d - p.LR * theta_d) / x_d_hat);
  const double B = p.PB, C = p.PC, D = p.PD, E = p.PE;
  const double Fcr = p.FZR * D * sin(C * atan(B * alpha_r - E * (B * alpha_r - atan(B * alpha_r))));
  const double a = P.u_drive[(size_t)b * 2 * P.N];
  const double el = Fcr / (p.M * p.ELL_LAT), ea = a / p.ELL_LONG;
  const double e = el * el + ea * ea;
  if (e > 1.0) {                                                                // main.m:212-213
    m[FSAEMPC_M_ELL_VIOL_INT] += (e - 1.0) * P.dt;
    if (e - 1.0 > m[FSAEMPC_M_ELL_VIOL_MAX]) m[FSAEMPC_M_ELL_VIOL_MAX] = e - 1.0;
  }
}

// The lap gate (include/fsaempc.h FSAEMPC_LS_*): carries a car over the finish line.  Runs between the pre-step and the
// MPC step; `finished` is what the pre-step left.  One thread per car, like its neighbours: the every-period part is a handful of loads,
// compares and flops on the car's own four state slots; the strided column shift (2N + 1 doubles, and the record's 16) runs only for a car
// that crosses in this period -- about once in several hundred periods -- so spreading it over a wavefront would buy nothing
// (profiles/trackdrive/ has the kernel's time beside cl_pre and the plant).
__global__ void cl_lap_gate_kernel(ClLapGateParams P) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= P.batch) return;
  int fin = P.finished[b];
  double* ls = P.lap_state + (size_t)b * FSAEMPC_NLAPSTATE;
  double done = ls[FSAEMPC_LS_DONE];
  if (fin == 2 || (fin == 1 && done >= (double)P.laps)) return;   // lost, or the last lap is complete: the car's data stay as they are
  if (!(done >= 0.0)) return;                                      // (a state the caller did not zero indexes nothing)
  const int nx = P.nx;
  double* x0 = P.x0 + (size_t)b * nx;
  if (fin == 1) {                                                  // the pre-step saw s >= L on this call: a crossing
    const double k = ls[FSAEMPC_LS_STEPS], s = x0[0], s_prev = ls[FSAEMPC_LS_S_PREV];
    double f = 1.0;                                                // share of the period before the line, linear in s
    if (k > 0.0 && s > s_prev) f = fmin(fmax((P.L - s_prev) / (s - s_prev), 0.0), 1.0);
    const double t = k > 0.0 ? (k - 1.0 + f) * P.dt : 0.0;
    P.lap_times[(size_t)b * P.laps + (int)done] = t - ls[FSAEMPC_LS_T_CROSS];
    ls[FSAEMPC_LS_T_CROSS] = t;
    done += 1.0;
    ls[FSAEMPC_LS_DONE] = done;
    if (done < (double)P.laps) {                                   // the car drives on
      if (P.metrics && P.lap_records) {                            // the lap's record is closed and handed over, a fresh one starts
        double* m = P.metrics + (size_t)b * FSAEMPC_NMETRIC;
        double* r = P.lap_records + ((size_t)b * P.laps + (int)done - 1) * FSAEMPC_NMETRIC;
        double v[FSAEMPC_NMETRIC];                                 // (all loads, then all stores: one memory round trip, not sixteen)
        for (int i = 0; i < FSAEMPC_NMETRIC; ++i) v[i] = m[i];
        v[FSAEMPC_M_STATUS] = 1.0;
        for (int i = 0; i < FSAEMPC_NMETRIC; ++i) { r[i] = v[i]; m[i] = 0.0; }
      }
      x0[0] = s - P.L;                                             // the wrap: every arc length the next step reads
      double* xr = P.x_ref + (size_t)b * nx * P.N;
      double* xk = P.x_keep + (size_t)b * nx * P.N;
      for (int j0 = 0; j0 < P.N; j0 += 8) {                        // eight stages of both plans per round trip: the stores may alias the
        double a[8], c[8];                                         // loads for all the compiler knows, so a plain loop waits on every one
#pragma unroll
        for (int i = 0; i < 8; ++i) if (j0 + i < P.N) { a[i] = xr[(j0 + i) * nx]; c[i] = xk[(j0 + i) * nx]; }
#pragma unroll
        for (int i = 0; i < 8; ++i) if (j0 + i < P.N) { xr[(j0 + i) * nx] = a[i] - P.L; xk[(j0 + i) * nx] = c[i] - P.L; }
      }
      P.finished[b] = 0;
      fin = 0;
    }                                                              // (final crossing: finished stays 1, cl_metrics latches the record)
  }
  if (fin == 0) { ls[FSAEMPC_LS_S_PREV] = x0[0]; ls[FSAEMPC_LS_STEPS] += 1.0; }
}

}  // namespace

hipError_t cl_lap_gate_launch(const ClLapGateParams& P, hipStream_t st) {
  if (P.batch == 0) return hipSuccess;
  hipLaunchKernelGGL(cl_lap_gate_kernel, dim3((P.batch + 63) / 64), dim3(64), 0, st, P);
  return hipGetLastError();
}
hipError_t cl_metrics_launch(const ClMetricsParams& P, hipStream_t st, const double* par, int par_stride) {
  if (P.batch == 0) return hipSuccess;
  if (par) hipLaunchKernelGGL(cl_metrics_kernel<RtPar>, dim3((P.batch + 63) / 64), dim3(64), 0, st, P, ParArgs{par, par_stride, nullptr});
  else hipLaunchKernelGGL(cl_metrics_kernel<FixedPar>, dim3((P.batch + 63) / 64), dim3(64), 0, st, P, NoParArgs{});
  return hipGetLastError();
}
hipError_t cl_accept_launch(int len_x, int len_u, int batch, const double* x_new, const double* u_new, const int* exitflag, double* x_keep, double* u_keep, hipStream_t st) {
  if (batch == 0) return hipSuccess;
  hipLaunchKernelGGL(cl_accept_kernel, dim3((batch + 63) / 64), dim3(64), 0, st, len_x, len_u, batch, x_new, u_new, exitflag, x_keep, u_keep);
  return hipGetLastError();
}
hipError_t cl_pre_launch(const ClPreParams& P, hipStream_t st) {
  if (P.batch == 0) return hipSuccess;
  hipLaunchKernelGGL(cl_pre_kernel, dim3((P.batch + 63) / 64), dim3(64), 0, st, P);
  return hipGetLastError();
}
hipError_t cl_plant_launch(const ClPlantParams& P, hipStream_t st, const double* par, int par_stride) {
  if (P.batch == 0) return hipSuccess;
  if (par) hipLaunchKernelGGL(cl_plant_kernel<RtPar>, dim3((P.batch + 63) / 64), dim3(64), 0, st, P, ParArgs{par, par_stride, nullptr});
  else hipLaunchKernelGGL(cl_plant_kernel<FixedPar>, dim3((P.batch + 63) / 64), dim3(64), 0, st, P, NoParArgs{});
  return hipGetLastError();
}
