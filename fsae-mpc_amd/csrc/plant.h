// plant.h -- internal interface between the C ABI and the closed-loop kernels (plant.hip)
#pragma once
#include <hip/hip_runtime.h>

struct ClPreParams {
  int nx, N, batch;
  double dt, target_vel, L;
  int spM; double spdl; const double* xP; const double* yP;   // spline table (device)
  const double* cart;      // batch x 7  Cartesian state [x, y, theta, x_d, y_d, theta_d, delta]
  const double* s_guess;   // batch      start of the closest-point search (first predicted s)
  double* x0;              // batch x nx
  double* x_ref;           // batch x (nx x N)
  int* finished;           // batch      set to 1 when s >= L
};
struct ClPlantParams {
  int nx, N, batch;
  double dt;
  double* cart;            // batch x 7, in/out
  double* pid;             // batch x 4, in/out: [vel integral, vel last error, steer integral, steer last error]
  const double* x_opt;     // batch x (nx x N): predicted states of this step's plan
  const int* finished;     // optional
  const int* exitflag;     // optional: cars whose step did not solve keep their state
  double* u_last;          // optional batch x 2: actuator rates of the last sub-step
};
struct ClMetricsParams {   // lap report (include/fsaempc.h FSAEMPC_M_*): inputs of one MPC period, all per car
  int ns, N, batch, tyre;  // slack count of the model, horizon, cars, index of the tyre slack (main.m:133; kinematic: 0)
  double dt, slack_tol;
  int nx;
  const double* x0;        // batch x nx (entries 0 = s and 1 = n are read)
  const int* finished;     // as cl_pre left it
  const int* exitflag; const int* iter; const double* fval; const double* slack;   // of this period's solve
  const double* u_drive;   // batch x 2N: the plan the car drives on
  const double* cart;      // batch x 7, post-plant
  double* metrics;         // batch x FSAEMPC_NMETRIC, in/out
};
struct ClLapGateParams {   // lap gate (include/fsaempc.h FSAEMPC_LS_*): between the pre-step and the MPC step, all per car
  int nx, N, laps, batch;
  double dt, L;
  double* x0;              // batch x nx, in/out (entry 0 = s)
  double* x_ref;           // batch x (nx x N), in/out (column 0 of every stage)
  double* x_keep;          // batch x (nx x N), in/out: the kept plan (column 0 of every stage)
  int* finished;           // as the pre-step left it, in/out
  double* lap_state;       // batch x FSAEMPC_NLAPSTATE, in/out
  double* lap_times;       // batch x laps
  double* metrics;         // optional batch x FSAEMPC_NMETRIC, in/out; given together with ...
  double* lap_records;     // ... batch x laps x FSAEMPC_NMETRIC
};
hipError_t cl_lap_gate_launch(const ClLapGateParams& P, hipStream_t st);
hipError_t cl_metrics_launch(const ClMetricsParams& P, hipStream_t st, const double* par = nullptr, int par_stride = 0);
hipError_t cl_pre_launch(const ClPreParams& P, hipStream_t st);
// par (optional): parameter blocks (include/fsaempc.h FSAEMPC_P_*), car b reads par + b * par_stride; null: f_cart_dyn.m's own constants
hipError_t cl_plant_launch(const ClPlantParams& P, hipStream_t st, const double* par = nullptr, int par_stride = 0);
hipError_t cl_accept_launch(int len_x, int len_u, int batch, const double* x_new, const double* u_new, const int* exitflag, double* x_keep, double* u_keep, hipStream_t st);
