// capi_cl.hip -- the C ABI of libfsaempc.so (include/fsaempc.h), closed-loop part: reference, pre, plant and accept, the metrics
// and the lap gate with their two host-side reports, measurement noise, observation, the state estimator, the Cartesian sensor models and the SQP as the controller.  Host-side glue only:
// argument checks and kernel launches.
#include "capi_common.h"
#include "reference.h"
#include "plant.h"
#include "cl_latency.h"
#include "cl_estimator.h"
#include "cl_sensors.h"
#include "cl_cone_loc.h"
#include "cl_nmpc.h"
using namespace capi;

extern "C" {

int fsaempc_obtain_reference_batch_device(const double* plan, double ds, int N_s, const double* t, const double* s0, double dt,
                                          int N_t, int batch, double* x_ref, void* stream) {
  if (!plan || !t || !s0 || !x_ref) return fail(FSAEMPC_ERR_ARG, "null argument");
  if (N_s <= 0 || N_t <= 0 || batch < 0 || !(ds > 0) || !(dt > 0)) return fail(FSAEMPC_ERR_ARG, "bad dimensions");
  RefParams P; P.plan = plan; P.t = t; P.s0 = s0; P.x_ref = x_ref; P.ds = ds; P.dt = dt; P.N_s = N_s; P.N_t = N_t; P.batch = batch;
  return launched(obtain_reference_launch(P, (hipStream_t)stream), "obtain_reference_launch");
}

int fsaempc_reference_live_batch_device(int nx, int N, double dt, double target_vel, int batch, const double* x0, double* x_ref, void* stream) {
  if (!x0 || !x_ref) return fail(FSAEMPC_ERR_ARG, "null argument");
  if ((nx != 5 && nx != 7) || N <= 0 || batch < 0 || !(dt > 0)) return fail(FSAEMPC_ERR_ARG, "bad dimensions");
  return launched(reference_live_launch(nx, N, dt, target_vel, batch, x0, x_ref, (hipStream_t)stream), "reference_live_launch");
}

int fsaempc_cl_pre_batch_device(int model, int N, double dt, double target_vel, double L, const fsaempc_spline* sp, const double* cart,
                                const double* s_guess, int batch, double* x0, double* x_ref, int* finished, void* stream) {
  if (!sp || !sp->xP || !sp->yP || !cart || !s_guess || !x0 || !x_ref || !finished) return fail(FSAEMPC_ERR_ARG, "null argument");
  if (model != FSAEMPC_MODEL_KINEMATIC && model != FSAEMPC_MODEL_DYNAMIC) return fail(FSAEMPC_ERR_ARG, "unknown model");
  if (N <= 0 || batch < 0 || !(dt > 0) || sp->M <= 0 || !(sp->dl > 0) || !(L > 0)) return fail(FSAEMPC_ERR_ARG, "bad dimensions");
  ClPreParams P; P.nx = fsaempc_ltv_nx(model); P.N = N; P.batch = batch; P.dt = dt; P.target_vel = target_vel; P.L = L;
  set_spline(&P, sp); P.cart = cart; P.s_guess = s_guess; P.x0 = x0; P.x_ref = x_ref; P.finished = finished;
  return launched(cl_pre_launch(P, (hipStream_t)stream), "cl_pre_launch");
}

int fsaempc_cl_plant_batch_device(int model, int N, double dt, int batch, double* cart, double* pid, const double* x_opt,
                                  const int* finished, const int* exitflag, double* u_last, void* stream) {
  return fsaempc_cl_plant_batch_device_p(model, N, dt, batch, nullptr, cart, pid, x_opt, finished, exitflag, u_last, stream);
}

int fsaempc_cl_plant_batch_device_p(int model, int N, double dt, int batch, const fsaempc_ltv_params* par, double* cart, double* pid,
                                    const double* x_opt, const int* finished, const int* exitflag, double* u_last, void* stream) {
  if (!cart || !pid || !x_opt) return fail(FSAEMPC_ERR_ARG, "null argument");
  if (model != FSAEMPC_MODEL_KINEMATIC && model != FSAEMPC_MODEL_DYNAMIC) return fail(FSAEMPC_ERR_ARG, "unknown model");
  if (N <= 0 || batch < 0 || !(dt > 0)) return fail(FSAEMPC_ERR_ARG, "bad dimensions");
  ClPlantParams P; P.nx = fsaempc_ltv_nx(model); P.N = N; P.batch = batch; P.dt = dt; P.cart = cart; P.pid = pid; P.x_opt = x_opt;
  P.finished = finished; P.exitflag = exitflag; P.u_last = u_last;
  return launched(cl_plant_launch(P, (hipStream_t)stream, par_values(par), par_stride(par)), "cl_plant_launch");
}

int fsaempc_cl_accept_batch_device(int model, int N, int batch, const double* x_new, const double* u_new, const int* exitflag, double* x_keep, double* u_keep, void* stream) {
  if (!x_new || !u_new || !x_keep || !u_keep) return fail(FSAEMPC_ERR_ARG, "null argument");
  if (model != FSAEMPC_MODEL_KINEMATIC && model != FSAEMPC_MODEL_DYNAMIC) return fail(FSAEMPC_ERR_ARG, "unknown model");
  if (N <= 0 || batch < 0) return fail(FSAEMPC_ERR_ARG, "bad dimensions");
  return launched(cl_accept_launch(fsaempc_ltv_nx(model) * N, 2 * N, batch, x_new, u_new, exitflag, x_keep, u_keep, (hipStream_t)stream), "cl_accept_launch");
}

/* ---- lap report ---- */
static int cl_metrics(int model, int N, double dt, double slack_tol, int batch, const fsaempc_ltv_params* par, const fsaempc_corridor* cor,
                      const double* x0, const int* finished, const int* exitflag, const int* iter, const double* fval,
                      const double* slack, const double* u_drive, const double* cart, double* metrics, void* stream) {
  CorTable ct;
  if (cor) { if (int rc = cor_check(cor, &ct)) return rc; }
  if (!x0 || !finished || !exitflag || !iter || !fval || !slack || !u_drive || !cart || !metrics) return fail(FSAEMPC_ERR_ARG, "null argument");
  if (model != FSAEMPC_MODEL_KINEMATIC && model != FSAEMPC_MODEL_DYNAMIC) return fail(FSAEMPC_ERR_ARG, "unknown model");
  if (N <= 0 || batch < 0 || !pos_finite(dt)) return fail(FSAEMPC_ERR_ARG, "bad dimensions");
  if (!(slack_tol >= 0)) return fail(FSAEMPC_ERR_ARG, "slack_tol must be >= 0");
  if (batch == 0) return 0;
  ClMetricsParams P; P.ns = ltv_ns(model); P.N = N; P.batch = batch; P.tyre = model == FSAEMPC_MODEL_DYNAMIC ? 3 : 0;
  P.dt = dt; P.slack_tol = slack_tol; P.nx = fsaempc_ltv_nx(model); P.x0 = x0; P.finished = finished; P.exitflag = exitflag; P.iter = iter;
  P.fval = fval; P.slack = slack; P.u_drive = u_drive; P.cart = cart; P.metrics = metrics;
  hipError_t e = cor ? cor_metrics_launch(P, ct, (hipStream_t)stream, par_values(par), par_stride(par))
                     : cl_metrics_launch(P, (hipStream_t)stream, par_values(par), par_stride(par));
  return launched(e, cor ? "cor_metrics_launch" : "cl_metrics_launch");
}
int fsaempc_cl_metrics_batch_device(int model, int N, double dt, double slack_tol, int batch, const fsaempc_ltv_params* par,
                                    const double* x0, const int* finished, const int* exitflag, const int* iter, const double* fval,
                                    const double* slack, const double* u_drive, const double* cart, double* metrics, void* stream) {
  return cl_metrics(model, N, dt, slack_tol, batch, par, nullptr, x0, finished, exitflag, iter, fval, slack, u_drive, cart, metrics, stream);
}
int fsaempc_cl_metrics_batch_device_c(int model, int N, double dt, double slack_tol, int batch, const fsaempc_ltv_params* par,
                                      const fsaempc_corridor* cor,
                                      const double* x0, const int* finished, const int* exitflag, const int* iter, const double* fval,
                                      const double* slack, const double* u_drive, const double* cart, double* metrics, void* stream) {
  return cl_metrics(model, N, dt, slack_tol, batch, par, cor, x0, finished, exitflag, iter, fval, slack, u_drive, cart, metrics, stream);
}

// Host.  Every sum runs over the cars in index order.  Means over an empty set are NaN (MATLAB's mean([])).
int fsaempc_cl_report(const double* metrics_host, int batch, double dt, double* out) {
  if (!out || (!metrics_host && batch != 0)) return fail(FSAEMPC_ERR_ARG, "null argument");
  if (batch < 0 || !pos_finite(dt)) return fail(FSAEMPC_ERR_ARG, "bad dimensions");
  double cars[3] = {0, 0, 0}, lap_sum = 0, lap_min = NAN, lap_max = NAN, steps = 0, abn = 0, sl_n = 0, sl_t = 0, obj = 0, obj_cnt = 0;
  double recorded = 0, nv_sum = 0, nv_big = 0, nv_max = 0, el_sum = 0, el_big = 0, el_max = 0, it_sum = 0, it_max = 0, n_abs = 0;
  for (int b = 0; b < batch; ++b) {
    const double* m = metrics_host + (size_t)b * FSAEMPC_NMETRIC;
    const int st = m[FSAEMPC_M_STATUS] == 1.0 ? 1 : (m[FSAEMPC_M_STATUS] == 2.0 ? 2 : 0);
    cars[st] += 1;
    if (st == 1) {
      const double lap = m[FSAEMPC_M_STEPS] * dt;
      lap_sum += lap;
      if (!(lap_min <= lap)) lap_min = lap;
      if (!(lap_max >= lap)) lap_max = lap;
    }
    steps += m[FSAEMPC_M_STEPS]; abn += m[FSAEMPC_M_ABNORMAL]; sl_n += m[FSAEMPC_M_SLACK_N_CNT]; sl_t += m[FSAEMPC_M_SLACK_TYRE_CNT];
    obj += m[FSAEMPC_M_OBJ_SUM]; obj_cnt += m[FSAEMPC_M_OBJ_CNT]; it_sum += m[FSAEMPC_M_ITER_SUM];
    if (m[FSAEMPC_M_STEPS] > 0) { recorded += 1; nv_sum += m[FSAEMPC_M_N_VIOL_INT]; el_sum += m[FSAEMPC_M_ELL_VIOL_INT]; }
    if (m[FSAEMPC_M_N_VIOL_INT] > nv_big) nv_big = m[FSAEMPC_M_N_VIOL_INT];
    if (m[FSAEMPC_M_N_VIOL_MAX] > nv_max) nv_max = m[FSAEMPC_M_N_VIOL_MAX];
    if (m[FSAEMPC_M_ELL_VIOL_INT] > el_big) el_big = m[FSAEMPC_M_ELL_VIOL_INT];
    if (m[FSAEMPC_M_ELL_VIOL_MAX] > el_max) el_max = m[FSAEMPC_M_ELL_VIOL_MAX];
    if (m[FSAEMPC_M_ITER_MAX] > it_max) it_max = m[FSAEMPC_M_ITER_MAX];
    if (m[FSAEMPC_M_N_ABS_MAX] > n_abs) n_abs = m[FSAEMPC_M_N_ABS_MAX];
  }
  out[FSAEMPC_R_CARS_DRIVING] = cars[0]; out[FSAEMPC_R_CARS_FINISHED] = cars[1]; out[FSAEMPC_R_CARS_LOST] = cars[2];
  out[FSAEMPC_R_LAP_MEAN] = cars[1] > 0 ? lap_sum / cars[1] : NAN; out[FSAEMPC_R_LAP_MIN] = lap_min; out[FSAEMPC_R_LAP_MAX] = lap_max;
  out[FSAEMPC_R_STEPS] = steps;
  out[FSAEMPC_R_ABNORMAL_PCT] = steps > 0 ? abn / steps * 100 : NAN;
  out[FSAEMPC_R_SLACK_N_PCT] = steps > 0 ? sl_n / steps * 100 : NAN;
  out[FSAEMPC_R_SLACK_TYRE_PCT] = steps > 0 ? sl_t / steps * 100 : NAN;
  out[FSAEMPC_R_OBJ_MEAN] = obj_cnt > 0 ? obj / obj_cnt : NAN;
  out[FSAEMPC_R_N_VIOL_INT_MEAN] = recorded > 0 ? nv_sum / recorded : NAN; out[FSAEMPC_R_N_VIOL_INT_MAX] = nv_big; out[FSAEMPC_R_N_VIOL_MAX] = nv_max;
  out[FSAEMPC_R_ELL_VIOL_INT_MEAN] = recorded > 0 ? el_sum / recorded : NAN; out[FSAEMPC_R_ELL_VIOL_INT_MAX] = el_big; out[FSAEMPC_R_ELL_VIOL_MAX] = el_max;
  out[FSAEMPC_R_ITER_MEAN] = steps > 0 ? it_sum / steps : NAN; out[FSAEMPC_R_ITER_MAX] = it_max; out[FSAEMPC_R_N_ABS_MAX] = n_abs;
  return 0;
}

/* ---- multi-lap closed loop: the lap gate ---- */
int fsaempc_cl_lap_gate_batch_device(int nx, int N, double dt, double L, int laps, int batch, double* x0, double* x_ref, double* x_keep,
                                     int* finished, double* lap_state, double* lap_times, double* metrics, double* lap_records, void* stream) {
  if (laps < 1 || laps > FSAEMPC_MAX_LAPS) return fail(FSAEMPC_ERR_ARG, "laps must be 1 .. FSAEMPC_MAX_LAPS");
  if (nx != 5 && nx != 7) return fail(FSAEMPC_ERR_ARG, "nx must be 5 or 7");
  if (N < 1 || batch < 0) return fail(FSAEMPC_ERR_ARG, "bad dimensions");
  if (!pos_finite(dt) || !pos_finite(L)) return fail(FSAEMPC_ERR_ARG, "dt and L must be finite and > 0");
  if (!x0 || !x_ref || !x_keep || !finished || !lap_state || !lap_times) return fail(FSAEMPC_ERR_ARG, "null argument");
  if ((metrics == nullptr) != (lap_records == nullptr)) return fail(FSAEMPC_ERR_ARG, "metrics and lap_records are given together or not at all");
  if (batch == 0) return 0;
  ClLapGateParams P; P.nx = nx; P.N = N; P.laps = laps; P.batch = batch; P.dt = dt; P.L = L; P.x0 = x0; P.x_ref = x_ref; P.x_keep = x_keep;
  P.finished = finished; P.lap_state = lap_state; P.lap_times = lap_times; P.metrics = metrics; P.lap_records = lap_records;
  return launched(cl_lap_gate_launch(P, (hipStream_t)stream), "cl_lap_gate_launch");
}

// Host.  Every sum runs over the cars in index order; a lap nobody completed has NaN mean, min and max.
int fsaempc_cl_lap_summary(const double* lap_times_host, int batch, int laps, double* out) {
  if (!out || (!lap_times_host && batch != 0)) return fail(FSAEMPC_ERR_ARG, "null argument");
  if (batch < 0) return fail(FSAEMPC_ERR_ARG, "bad dimensions");
  if (laps < 1 || laps > FSAEMPC_MAX_LAPS) return fail(FSAEMPC_ERR_ARG, "laps must be 1 .. FSAEMPC_MAX_LAPS");
  for (int l = 0; l < laps; ++l) {
    double cnt = 0, sum = 0, lo = NAN, hi = NAN;
    for (int b = 0; b < batch; ++b) {
      const double t = lap_times_host[(size_t)b * laps + l];
      if (t != t) continue;
      cnt += 1; sum += t;
      if (!(lo <= t)) lo = t;
      if (!(hi >= t)) hi = t;
    }
    out[4 * l] = cnt; out[4 * l + 1] = cnt > 0 ? sum / cnt : NAN; out[4 * l + 2] = lo; out[4 * l + 3] = hi;
  }
  return 0;
}

/* ---- closed loop: measurement noise, plan latency and delay compensation ---- */
static int cl_draw_check(long long id0, long long step) {
  if (id0 < 0) return fail(FSAEMPC_ERR_ARG, "id0 must be >= 0");
  if (step < 0 || step >= (1LL << 32)) return fail(FSAEMPC_ERR_ARG, "step must be 0 .. 2^32 - 1");
  return 0;
}

int fsaempc_cl_noise_batch_device(int nx, int batch, unsigned long long seed, long long id0, long long step, double* z, void* stream) {
  if (nx != 5 && nx != 7) return fail(FSAEMPC_ERR_ARG, "nx must be 5 or 7");
  if (batch < 0) return fail(FSAEMPC_ERR_ARG, "bad dimensions");
  if (int rc = cl_draw_check(id0, step)) return rc;
  if (!z) return fail(FSAEMPC_ERR_ARG, "null argument");
  if (batch == 0) return 0;
  return launched(cl_noise_launch(nx, batch, seed, (unsigned long long)id0, (unsigned long long)step, z, (hipStream_t)stream), "cl_noise_launch");
}

int fsaempc_cl_observe_batch_device(const fsaempc_ltv_desc* desc, const fsaempc_spline* sp, const fsaempc_ltv_params* par,
                                    const fsaempc_cl_latency* lat, long long step, const double* x0_true, const int* finished,
                                    const double* u_hist, double* x0_obs, double* x0_mpc, void* stream) {
  if (int rc = ltv_check(desc, sp)) return rc;
  if (!lat) return fail(FSAEMPC_ERR_ARG, "null argument");
  if (lat->delay < 0 || lat->delay > FSAEMPC_CL_MAX_DELAY) return fail(FSAEMPC_ERR_ARG, "delay must be 0 .. FSAEMPC_CL_MAX_DELAY");
  if (lat->compensate != 0 && lat->compensate != 1) return fail(FSAEMPC_ERR_ARG, "compensate must be 0 or 1");
  if (int rc = cl_draw_check(lat->id0, step)) return rc;
  if (lat->delay > 0 && !u_hist) return fail(FSAEMPC_ERR_ARG, "null argument (u_hist is required with delay > 0)");
  if (!x0_true || !x0_obs || !x0_mpc) return fail(FSAEMPC_ERR_ARG, "null argument");
  if (desc->batch == 0) return 0;
  ClObserveParams P;
  P.nx = fsaempc_ltv_nx(desc->model); P.N = desc->N; P.batch = desc->batch; P.integ = ltv_integ(desc);
  P.delay = lat->delay; P.compensate = lat->compensate; P.sigma_per_instance = lat->sigma_per_instance ? 1 : 0; P.dt = desc->dt;
  P.seed = lat->seed; P.id0 = (unsigned long long)lat->id0; P.step = (unsigned long long)step;
  set_spline(&P, sp);
  P.sigma = lat->sigma; P.x0_true = x0_true; P.finished = finished; P.u_hist = u_hist; P.x0_obs = x0_obs; P.x0_mpc = x0_mpc;
  return launched(cl_observe_launch(P, (hipStream_t)stream, par_values(par), par_stride(par)), "cl_observe_launch");
}

// Host.
int fsaempc_cl_history_slot(int delay, long long step, int lag) {
  if (delay < 0 || delay > FSAEMPC_CL_MAX_DELAY || step < 0 || lag < 0 || lag > delay) return -1;
  return cll_slot(delay, step, lag);
}

/* ---- closed loop: the state estimator ---- */
namespace { struct ByteRange { const char* name; const void* p; size_t bytes; }; }
static bool ranges_overlap(const ByteRange& a, const ByteRange& b) {
  if (!a.p || !b.p || a.bytes == 0 || b.bytes == 0) return false;
  const uintptr_t a0 = (uintptr_t)a.p, b0 = (uintptr_t)b.p;
  return a0 < b0 + b.bytes && b0 < a0 + a.bytes;
}

// no output may overlap another output or an input
static int ranges_check(const ByteRange* out, int n_out, const ByteRange* in, int n_in) {
  for (int i = 0; i < n_out; ++i) {
    for (int k = i + 1; k < n_out; ++k)
      if (ranges_overlap(out[i], out[k])) return fail(FSAEMPC_ERR_ARG, "overlapping outputs");
    for (int k = 0; k < n_in; ++k)
      if (ranges_overlap(out[i], in[k])) return fail(FSAEMPC_ERR_ARG, "an output overlaps an input");
  }
  return 0;
}

int fsaempc_cl_estimate_batch_device(const fsaempc_ltv_desc* desc, const fsaempc_spline* sp, const fsaempc_ltv_params* par,
                                     const fsaempc_cl_estimator* est, const double* z, const double* x_start, const double* u_prev,
                                     long long u_stride, const int* finished, double* est_x, double* est_P, int* est_count, double* x0_est,
                                     double* innov, double* nis, double* F_out, double* x_prior, void* stream) {
  if (int rc = ltv_check(desc, sp)) return rc;
  if (!est || !est->q || !est->r || !est->p0) return fail(FSAEMPC_ERR_ARG, "null argument");
  if (!(est->L >= 0 && est->L < INFINITY)) return fail(FSAEMPC_ERR_ARG, "L must be finite and >= 0");
  if (u_stride < 2) return fail(FSAEMPC_ERR_ARG, "u_stride must be >= 2");
  if (!z || !x_start || !u_prev || !est_x || !est_P || !est_count || !x0_est || !innov || !nis) return fail(FSAEMPC_ERR_ARG, "null argument");
  const size_t B = (size_t)desc->batch, nx = (size_t)fsaempc_ltv_nx(desc->model), d = sizeof(double);
  const ByteRange out[] = {{"est_x", est_x, B * nx * d}, {"est_P", est_P, B * nx * nx * d}, {"est_count", est_count, B * 2 * sizeof(int)},
                           {"x0_est", x0_est, B * nx * d}, {"innov", innov, B * nx * d}, {"nis", nis, B * d},
                           {"F_out", F_out, B * nx * nx * d}, {"x_prior", x_prior, B * nx * d}};
  const ByteRange in[] = {{"z", z, B * nx * d}, {"x_start", x_start, B * nx * d},
                          {"u_prev", u_prev, B ? ((B - 1) * (size_t)u_stride + 2) * d : 0}, {"finished", finished, B * sizeof(int)},
                          {"q", est->q, (est->q_per_instance ? B : 1) * nx * d}, {"r", est->r, (est->r_per_instance ? B : 1) * nx * d},
                          {"p0", est->p0, nx * d}};
  if (int rc = ranges_check(out, (int)(sizeof(out) / sizeof(out[0])), in, (int)(sizeof(in) / sizeof(in[0])))) return rc;
  if (desc->batch == 0) return 0;
  ClEstimateParams P;
  P.nx = (int)nx; P.batch = desc->batch; P.integ = ltv_integ(desc); P.q_per_instance = est->q_per_instance ? 1 : 0;
  P.r_per_instance = est->r_per_instance ? 1 : 0; P.dt = desc->dt; P.L = est->L;
  set_spline(&P, sp);
  P.q = est->q; P.r = est->r; P.p0 = est->p0; P.z = z; P.x_start = x_start; P.u_prev = u_prev; P.u_stride = u_stride; P.finished = finished;
  P.est_x = est_x; P.est_P = est_P; P.est_count = est_count; P.x0_est = x0_est; P.innov = innov; P.nis = nis; P.F_out = F_out; P.x_prior = x_prior;
  return launched(cl_estimate_launch(P, (hipStream_t)stream, par_values(par), par_stride(par)), "cl_estimate_launch");
}

/* ---- closed loop: Cartesian sensor models ---- */
int fsaempc_cl_sense_batch_device(const fsaempc_ltv_desc* desc, const fsaempc_spline* sp, const fsaempc_cl_sensors* sens, long long step,
                                  const double* cart, const double* x0_true, const int* finished, double* y, double* x_proj, int* proj_lost,
                                  void* stream) {
  if (int rc = ltv_check(desc, sp)) return rc;
  if (!sens) return fail(FSAEMPC_ERR_ARG, "null argument (sens)");
  if (!sens->sigma) return fail(FSAEMPC_ERR_ARG, "null argument (sens->sigma)");
  if (int rc = cl_draw_check(sens->id0, step)) return rc;
  if (!cart) return fail(FSAEMPC_ERR_ARG, "null argument (cart)");
  if (!x0_true) return fail(FSAEMPC_ERR_ARG, "null argument (x0_true)");
  if (!y) return fail(FSAEMPC_ERR_ARG, "null argument (y)");
  if (!x_proj) return fail(FSAEMPC_ERR_ARG, "null argument (x_proj)");
  if (!proj_lost) return fail(FSAEMPC_ERR_ARG, "null argument (proj_lost)");
  const size_t B = (size_t)desc->batch, nx = (size_t)fsaempc_ltv_nx(desc->model), d = sizeof(double);
  const ByteRange out[] = {{"y", y, B * nx * d}, {"x_proj", x_proj, B * nx * d}, {"proj_lost", proj_lost, B * sizeof(int)}};
  const ByteRange in[] = {{"cart", cart, B * 7 * d}, {"x0_true", x0_true, B * nx * d}, {"finished", finished, B * sizeof(int)},
                          {"sigma", sens->sigma, (sens->sigma_per_instance ? B : 1) * nx * d}};
  if (int rc = ranges_check(out, (int)(sizeof(out) / sizeof(out[0])), in, (int)(sizeof(in) / sizeof(in[0])))) return rc;
  if (desc->batch == 0) return 0;
  ClSenseParams P;
  P.nx = (int)nx; P.batch = desc->batch; P.sigma_per_instance = sens->sigma_per_instance ? 1 : 0;
  P.seed = sens->seed; P.id0 = (unsigned long long)sens->id0; P.step = (unsigned long long)step;
  set_spline(&P, sp);
  P.sigma = sens->sigma; P.cart = cart; P.x0_true = x0_true; P.finished = finished; P.y = y; P.x_proj = x_proj; P.proj_lost = proj_lost;
  return launched(cl_sense_launch(P, (hipStream_t)stream), "cl_sense_launch");
}

// What the two filters on the Cartesian measurement share: the checks of their common arguments, the kernel's parameters and the byte
// ranges of what they write and read (the cone filter adds its own to both lists before the overlap check).
namespace {
struct CartArgs {
  const double* y; const double* x_proj; const double* u_prev; long long u_stride; const int* finished;
  double* est_x; double* est_P; int* est_count; double* x0_est; double* innov; double* nis; double* F_out; double* x_prior; double* H_out;
};
constexpr int CL_CART_OUT = 9, CL_CART_IN = 7;
}
static int cl_cart_check(const fsaempc_ltv_desc* desc, const fsaempc_spline* sp, const fsaempc_cl_estimator* est, const CartArgs& a,
                         ClEstimateCartParams* P, ByteRange* out, ByteRange* in) {
  if (int rc = ltv_check(desc, sp)) return rc;
  if (!est) return fail(FSAEMPC_ERR_ARG, "null argument (est)");
  if (!est->q) return fail(FSAEMPC_ERR_ARG, "null argument (est->q)");
  if (!est->r) return fail(FSAEMPC_ERR_ARG, "null argument (est->r)");
  if (!est->p0) return fail(FSAEMPC_ERR_ARG, "null argument (est->p0)");
  if (!(est->L >= 0 && est->L < INFINITY)) return fail(FSAEMPC_ERR_ARG, "L must be finite and >= 0");
  if (a.u_stride < 2) return fail(FSAEMPC_ERR_ARG, "u_stride must be >= 2");
  const struct { const char* name; const void* p; } need[] = {{"y", a.y}, {"x_proj", a.x_proj}, {"u_prev", a.u_prev}, {"est_x", a.est_x},
                                                               {"est_P", a.est_P}, {"est_count", a.est_count}, {"x0_est", a.x0_est},
                                                               {"innov", a.innov}, {"nis", a.nis}};
  for (const auto& n : need)
    if (!n.p) return fail(FSAEMPC_ERR_ARG, "null argument (%s)", n.name);
  const size_t B = (size_t)desc->batch, nx = (size_t)fsaempc_ltv_nx(desc->model), d = sizeof(double);
  const ByteRange o[CL_CART_OUT] = {{"est_x", a.est_x, B * nx * d}, {"est_P", a.est_P, B * nx * nx * d}, {"est_count", a.est_count, B * 2 * sizeof(int)},
                                    {"x0_est", a.x0_est, B * nx * d}, {"innov", a.innov, B * nx * d}, {"nis", a.nis, B * d},
                                    {"F_out", a.F_out, B * nx * nx * d}, {"x_prior", a.x_prior, B * nx * d}, {"H_out", a.H_out, B * nx * nx * d}};
  const ByteRange i[CL_CART_IN] = {{"y", a.y, B * nx * d}, {"x_proj", a.x_proj, B * nx * d},
                                   {"u_prev", a.u_prev, B ? ((B - 1) * (size_t)a.u_stride + 2) * d : 0}, {"finished", a.finished, B * sizeof(int)},
                                   {"q", est->q, (est->q_per_instance ? B : 1) * nx * d}, {"r", est->r, (est->r_per_instance ? B : 1) * nx * d},
                                   {"p0", est->p0, nx * d}};
  for (int k = 0; k < CL_CART_OUT; ++k) out[k] = o[k];
  for (int k = 0; k < CL_CART_IN; ++k) in[k] = i[k];
  P->nx = (int)nx; P->batch = desc->batch; P->integ = ltv_integ(desc); P->q_per_instance = est->q_per_instance ? 1 : 0;
  P->r_per_instance = est->r_per_instance ? 1 : 0; P->dt = desc->dt; P->L = est->L;
  set_spline(P, sp);
  P->q = est->q; P->r = est->r; P->p0 = est->p0; P->y = a.y; P->x_proj = a.x_proj; P->u_prev = a.u_prev; P->u_stride = a.u_stride;
  P->finished = a.finished; P->est_x = a.est_x; P->est_P = a.est_P; P->est_count = a.est_count; P->x0_est = a.x0_est; P->innov = a.innov;
  P->nis = a.nis; P->F_out = a.F_out; P->x_prior = a.x_prior; P->H_out = a.H_out;
  return 0;
}

int fsaempc_cl_estimate_cart_batch_device(const fsaempc_ltv_desc* desc, const fsaempc_spline* sp, const fsaempc_ltv_params* par,
                                          const fsaempc_cl_estimator* est, const double* y, const double* x_proj, const double* u_prev,
                                          long long u_stride, const int* finished, double* est_x, double* est_P, int* est_count, double* x0_est,
                                          double* innov, double* nis, double* F_out, double* x_prior, double* H_out, void* stream) {
  ClEstimateCartParams P;
  ByteRange out[CL_CART_OUT], in[CL_CART_IN];
  const CartArgs a{y, x_proj, u_prev, u_stride, finished, est_x, est_P, est_count, x0_est, innov, nis, F_out, x_prior, H_out};
  if (int rc = cl_cart_check(desc, sp, est, a, &P, out, in)) return rc;
  if (int rc = ranges_check(out, CL_CART_OUT, in, CL_CART_IN)) return rc;
  if (desc->batch == 0) return 0;
  return launched(cl_estimate_cart_launch(P, (hipStream_t)stream, par_values(par), par_stride(par)), "cl_estimate_cart_launch");
}

/* ---- closed loop: cone-based localisation ---- */
// a cone map as both entries read it: `who` names the argument in the message
static int cl_cone_map_check(const fsaempc_cones* m, const char* who, ClConeMap* out) {
  if (!m) return fail(FSAEMPC_ERR_ARG, "null argument (%s)", who);
  if (m->n_left < 0 || m->n_right < 0) return fail(FSAEMPC_ERR_ARG, "%s: a negative cone count", who);
  if (m->n_left > FSAEMPC_CONES_MAX || m->n_right > FSAEMPC_CONES_MAX) return fail(FSAEMPC_ERR_DIM, "%s: more than FSAEMPC_CONES_MAX cones on a side", who);
  if (m->n_left + m->n_right == 0) return fail(FSAEMPC_ERR_ARG, "%s: a map with no cones", who);
  if ((m->n_left > 0 && !m->left) || (m->n_right > 0 && !m->right)) return fail(FSAEMPC_ERR_ARG, "null argument (%s: a side with cones and no pointer)", who);
  out->left = m->left; out->right = m->right; out->n_left = m->n_left; out->n_right = m->n_right; out->per_car = m->per_corridor ? 1 : 0;
  return 0;
}

static int cl_k_max_check(int k_max) {
  return k_max >= 1 && k_max <= FSAEMPC_CONE_OBS_MAX ? 0 : fail(FSAEMPC_ERR_ARG, "k_max must be 1 .. FSAEMPC_CONE_OBS_MAX");
}

int fsaempc_cl_cone_sense_batch_device(int batch, const fsaempc_cl_cone_sensor* sensor, long long step, const double* cart, const int* finished,
                                       int* cone_n, int* cone_seen, int* cone_id, double* cone_z, void* stream) {
  if (batch < 0) return fail(FSAEMPC_ERR_ARG, "bad dimensions (batch)");
  if (!sensor) return fail(FSAEMPC_ERR_ARG, "null argument (sensor)");
  ClConeSenseParams P;
  if (int rc = cl_cone_map_check(sensor->truth, "sensor->truth", &P.truth)) return rc;
  if (int rc = cl_k_max_check(sensor->k_max)) return rc;
  if (!(sensor->r_max < INFINITY) || !(sensor->r_min > 0) || !(sensor->r_min < sensor->r_max))
    return fail(FSAEMPC_ERR_ARG, "r_min must be > 0 and below a finite r_max");
  if (!(sensor->fov > 0 && sensor->fov <= 2 * M_PI)) return fail(FSAEMPC_ERR_ARG, "fov must be in (0, 2 pi]");
  if (!(sensor->sigma_range >= 0)) return fail(FSAEMPC_ERR_ARG, "sigma_range must be >= 0");
  if (!(sensor->sigma_bearing >= 0)) return fail(FSAEMPC_ERR_ARG, "sigma_bearing must be >= 0");
  if (!(sensor->p_detect >= 0 && sensor->p_detect <= 1)) return fail(FSAEMPC_ERR_ARG, "p_detect must be in [0, 1]");
  if (int rc = cl_draw_check(sensor->id0, step)) return rc;
  const struct { const char* name; const void* p; } need[] = {{"cart", cart}, {"cone_n", cone_n}, {"cone_seen", cone_seen}, {"cone_id", cone_id},
                                                               {"cone_z", cone_z}};
  for (const auto& n : need)
    if (!n.p) return fail(FSAEMPC_ERR_ARG, "null argument (%s)", n.name);
  const size_t B = (size_t)batch, K = (size_t)sensor->k_max, d = sizeof(double), maps = P.truth.per_car ? B : 1;
  const ByteRange out[] = {{"cone_n", cone_n, B * sizeof(int)}, {"cone_seen", cone_seen, B * sizeof(int)}, {"cone_id", cone_id, B * K * sizeof(int)},
                           {"cone_z", cone_z, B * K * 2 * d}};
  const ByteRange in[] = {{"cart", cart, B * 7 * d}, {"finished", finished, B * sizeof(int)},
                          {"left", P.truth.left, maps * (size_t)P.truth.n_left * 2 * d}, {"right", P.truth.right, maps * (size_t)P.truth.n_right * 2 * d}};
  if (int rc = ranges_check(out, (int)(sizeof(out) / sizeof(out[0])), in, (int)(sizeof(in) / sizeof(in[0])))) return rc;
  if (batch == 0) return 0;
  P.batch = batch; P.k_max = sensor->k_max; P.r_min = sensor->r_min; P.r_max = sensor->r_max; P.fov = sensor->fov;
  P.sigma_rho = sensor->sigma_range; P.sigma_beta = sensor->sigma_bearing; P.p_detect = sensor->p_detect;
  P.seed = sensor->seed; P.id0 = (unsigned long long)sensor->id0; P.step = (unsigned long long)step;
  P.cart = cart; P.finished = finished; P.cone_n = cone_n; P.cone_seen = cone_seen; P.cone_id = cone_id; P.cone_z = cone_z;
  return launched(cl_cone_sense_launch(P, (hipStream_t)stream), "cl_cone_sense_launch");
}

int fsaempc_cl_estimate_cones_batch_device(const fsaempc_ltv_desc* desc, const fsaempc_spline* sp, const fsaempc_ltv_params* par,
                                           const fsaempc_cl_estimator* est, const double* y, const double* x_proj, const double* u_prev,
                                           long long u_stride, const int* finished, double* est_x, double* est_P, int* est_count, double* x0_est,
                                           double* innov, double* nis, double* F_out, double* x_prior, double* H_out, const fsaempc_cones* map,
                                           int k_max, const double* r_cone, const int* cone_n, const int* cone_id, const double* cone_z,
                                           double* cone_innov, int* rows_used, double* G_out, void* stream) {
  ClEstimateConesParams P;
  constexpr int N_OUT = CL_CART_OUT + 3, N_IN = CL_CART_IN + 5;
  ByteRange out[N_OUT], in[N_IN];
  const CartArgs a{y, x_proj, u_prev, u_stride, finished, est_x, est_P, est_count, x0_est, innov, nis, F_out, x_prior, H_out};
  if (int rc = cl_cart_check(desc, sp, est, a, &P.E, out, in)) return rc;
  if (int rc = cl_cone_map_check(map, "map", &P.map)) return rc;
  if (int rc = cl_k_max_check(k_max)) return rc;
  const struct { const char* name; const void* p; } need[] = {{"r_cone", r_cone}, {"cone_n", cone_n}, {"cone_id", cone_id}, {"cone_z", cone_z},
                                                               {"cone_innov", cone_innov}, {"rows_used", rows_used}};
  for (const auto& n : need)
    if (!n.p) return fail(FSAEMPC_ERR_ARG, "null argument (%s)", n.name);
  const size_t B = (size_t)desc->batch, K = (size_t)k_max, d = sizeof(double), maps = P.map.per_car ? B : 1;
  out[CL_CART_OUT] = {"cone_innov", cone_innov, B * K * 2 * d};
  out[CL_CART_OUT + 1] = {"rows_used", rows_used, B * sizeof(int)};
  out[CL_CART_OUT + 2] = {"G_out", G_out, B * K * 6 * d};
  in[CL_CART_IN] = {"cone_n", cone_n, B * sizeof(int)};
  in[CL_CART_IN + 1] = {"cone_id", cone_id, B * K * sizeof(int)};
  in[CL_CART_IN + 2] = {"cone_z", cone_z, B * K * 2 * d};
  in[CL_CART_IN + 3] = {"left", P.map.left, maps * (size_t)P.map.n_left * 2 * d};
  in[CL_CART_IN + 4] = {"right", P.map.right, maps * (size_t)P.map.n_right * 2 * d};
  if (int rc = ranges_check(out, N_OUT, in, N_IN)) return rc;
  if (desc->batch == 0) return 0;
  P.k_max = k_max; P.r_cone[0] = r_cone[0]; P.r_cone[1] = r_cone[1];
  P.cone_n = cone_n; P.cone_id = cone_id; P.cone_z = cone_z; P.cone_innov = cone_innov; P.rows_used = rows_used; P.G_out = G_out;
  return launched(cl_estimate_cones_launch(P, (hipStream_t)stream, par_values(par), par_stride(par)), "cl_estimate_cones_launch");
}

/* ---- closed loop: the batched SQP as the controller ---- */
int fsaempc_cl_nmpc_shift_batch_device(int N, int batch, int shift, const double* u_keep, const int* finished, double* u_init, int* skip,
                                       void* stream) {
  if (!u_keep || !u_init || !skip) return fail(FSAEMPC_ERR_ARG, "null argument");
  if (N < 1 || batch < 0) return fail(FSAEMPC_ERR_ARG, "bad dimensions");
  if (shift != 0 && shift != 1) return fail(FSAEMPC_ERR_ARG, "shift must be 0 or 1");
  const size_t bytes = (size_t)batch * (size_t)N * 2 * sizeof(double);
  if (ranges_overlap(ByteRange{"u_init", u_init, bytes}, ByteRange{"u_keep", u_keep, bytes}))
    return fail(FSAEMPC_ERR_ARG, "u_init must not alias u_keep");
  if (batch == 0) return 0;
  return launched(cl_nmpc_shift_launch(N, batch, shift, u_keep, finished, u_init, skip, (hipStream_t)stream), "cl_nmpc_shift_launch");
}

int fsaempc_cl_nmpc_accept_batch_device(int model, int N, int batch, const double* x_new, const double* u_new, const int* status,
                                        const int* qp_iter, const int* skip, double* x_keep, double* u_keep, int* exitflag, int* iter,
                                        void* stream) {
  if (!x_new || !u_new || !status || !x_keep || !u_keep || !exitflag || !iter) return fail(FSAEMPC_ERR_ARG, "null argument");
  if (model != FSAEMPC_MODEL_KINEMATIC && model != FSAEMPC_MODEL_DYNAMIC) return fail(FSAEMPC_ERR_ARG, "unknown model");
  if (N < 1 || batch < 0) return fail(FSAEMPC_ERR_ARG, "bad dimensions");
  if (batch == 0) return 0;
  return launched(cl_nmpc_accept_launch(fsaempc_ltv_nx(model) * N, 2 * N, batch, x_new, u_new, status, qp_iter, skip, x_keep, u_keep, exitflag, iter,
                                        (hipStream_t)stream), "cl_nmpc_accept_launch");
}

}  // extern "C"
