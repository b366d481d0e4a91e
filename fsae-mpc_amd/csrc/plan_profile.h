// plan_profile.h -- the speed profile of the s-domain plans, written once for the centre-line plan
// (planner.hip), the plan on a racing line (raceline.hip) and the lap-time gradient (minlap.hip), for the host and the device.
//
// Per cell: curvature k and length dl (the constant ds on the centre line, ds r on a line), K = max(|k|, 1e-12) and the grip-limited
// corner speed vlat = min(v_cap, sqrt(A_lat / K)).  From the first minimum i0 of vlat one forward pass (acceleration out of the
// predecessor over the predecessor's cell) and one backward pass (braking into the successor over the cell's own length), both under
// the longitudinal limit the controller's own QP rows carry; since vlat[i0] is the global minimum, one pass each way closes the lap.
//
//   pp_ax            the longitudinal limit a_x(v, K) and, on request, its partials in v and K
//   pp_corner_speed  vlat of one cell
//   pp_passes        the two passes from i0; where a cell's length comes from (PpConstLen or an array) and what is recorded on the
//                    way (PpNoRecord, or PpRecord for the reverse sweep of minlap.h) are chosen at compile time
//   pp_first_min     first index of the minimum of an array (the host's i0)
// and, for device code only, the phases the kernels are made of: pp_wave_first_min, pp_load_points, pp_line_geometry,
// pp_line_curvature, pp_corner_phase, pp_nan_table, pp_table_row.
//
// The first part compiles as plain C++ (a host program may include this file without the HIP headers).  No FMA contraction, in no
// function: every one is restated operation for operation in tests/plan_numpy.py, raceline_numpy.py and minlap_numpy.py.
#pragma once
#include <math.h>
#include <stddef.h>
#include "raceline.h"
#if defined(__HIPCC__)
#include "cl_frame.h"   // kappa().  It carries no pragma and is read before any unit's own: the default contraction in every unit
#endif

struct MlCar { double U_ACC_MAX, ELL_LONG; };   // the two limits of the block that the longitudinal limit reads

// Largest longitudinal acceleration at speed v in a cell of curvature magnitude K.
//   kinematic: the input box scaled by grip (with the soft +-ALAT_MAX rows a rectangle)
//   dynamic:   the boundary of the inscribed 12-gon of dynamic_tyre_linearise_constraints.m:18-23 in the first quadrant, at the
//              lateral share y = v^2 K / A_lat, capped by the input box.  The polygon is what the tyre rows enforce, and unlike the
//              ellipse it is Lipschitz at the apex.
// GRAD: also *dv = d a_x / d v and *dK = d a_x / d K, zero where U_ACC_MAX or y = 1 is the active branch.
template <bool DYN, bool GRAD = false>
RL_HD double pp_ax(const MlCar& p, double v, double K, double A_lat, double grip, double* dv = nullptr, double* dK = nullptr) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if constexpr (GRAD) { *dv = 0.0; *dK = 0.0; }
  if constexpr (!DYN) {
    return grip * p.U_ACC_MAX;
  } else {
    const double y0 = v * v * K / A_lat;
    const double y = fmin(y0, 1.0);
    double c0 = 1.0, c1 = 0.8660254037844386, s0 = 0.0, s1 = 0.5;                        // edge 0
    if (!(y <= 0.5)) { c0 = 0.8660254037844386; c1 = 0.5; s0 = 0.5; s1 = 0.8660254037844386; }   // edge 1
    if (!(y <= 0.8660254037844386)) { c0 = 0.5; c1 = 0.0; s0 = 0.8660254037844386; s1 = 1.0; }   // edge 2
    const double X = c0 + (c1 - c0) * (y - s0) / (s1 - s0);
    const double val = grip * p.ELL_LONG * X;
    if constexpr (GRAD) {
      if (val < p.U_ACC_MAX && y0 < 1.0) {
        const double slope = grip * p.ELL_LONG * ((c1 - c0) / (s1 - s0));
        *dv = slope * (2.0 * v * K / A_lat);
        *dK = slope * (v * v / A_lat);
      }
    }
    return fmin(p.U_ACC_MAX, val);
  }
}

// grip-limited corner speed of a cell of curvature k
RL_HD double pp_corner_speed(double k, double A_lat, double v_cap) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return fmin(v_cap, sqrt(A_lat / fmax(fabs(k), 1e-12)));
}

struct PpConstLen { double ds; RL_HD double operator[](int) const { return ds; } };   // every cell has the length ds

#define ML_WON_FWD 1   // the forward recurrence was strictly below the cell's corner speed
#define ML_WON_BWD 2   // the backward recurrence was strictly below the cell's speed after the forward pass

struct PpNoRecord {   // the profile alone
  RL_HD void forward(int, double, bool) const {}
  RL_HD void backward(int, bool) const {}
};
// vf: the speeds after the forward pass (the backward pass may lower a cell the forward pass read as its source); won: ML_WON_* per cell
struct PpRecord {
  double* vf; int* won;
  RL_HD void forward(int i, double v, bool w) const { won[i] = w ? ML_WON_FWD : 0; vf[i] = v; }
  RL_HD void backward(int i, bool w) const { if (w) won[i] |= ML_WON_BWD; }
};

// The two recurrences from cell i0.  k: curvature per cell; dl[i]: length of cell i (LEN: PpConstLen or const double*); v: in the
// corner speeds vlat, out the final speeds; rec: PpNoRecord or PpRecord.
template <bool DYN, class LEN, class REC>
RL_HD void pp_passes(const MlCar& p, int Ns, int i0, double A_lat, double grip, const double* k, const LEN dl, double* v, const REC rec) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double vp = v[i0]; int i = i0;
  for (int j = 1; j <= Ns; ++j) {                   // forward: acceleration out of the slower predecessor, over the predecessor's cell
    const int pr = i;
    i = i + 1; if (i >= Ns) i = 0;
    const double Kp = fmax(fabs(k[pr]), 1e-12);
    const double a = pp_ax<DYN>(p, vp, Kp, A_lat, grip);
    const double own = v[i], cand = sqrt(vp * vp + 2.0 * a * dl[pr]);
    const double vi = fmin(own, cand);
    rec.forward(i, vi, cand < own);
    v[i] = vi; vp = vi;
  }
  vp = v[i0]; i = i0;
  for (int j = 1; j <= Ns; ++j) {                   // backward: braking into the slower successor, over the cell being set
    const int nx = i;
    i = i - 1; if (i < 0) i = Ns - 1;
    const double Kn = fmax(fabs(k[nx]), 1e-12);
    const double a = pp_ax<DYN>(p, vp, Kn, A_lat, grip);
    const double own = v[i], cand = sqrt(vp * vp + 2.0 * a * dl[i]);
    const double vi = fmin(own, cand);
    rec.backward(i, cand < own);
    v[i] = vi; vp = vi;
  }
}

// first index of the minimum of v (what the lanes' scans and pp_wave_first_min find on the device)
inline int pp_first_min(const double* v, int Ns) {
  int i0 = 0;
  for (int i = 1; i < Ns; ++i)
    if (v[i] < v[i0]) i0 = i;
  return i0;
}

#if defined(__HIPCC__)
// ---- the phases of the kernels: one wavefront per plan, the cells lane, lane + 64, ... to a lane (per = ceil(N_s / 64) trips where
// given); every cross-lane operation comes after such a loop, never inside one ----
#define PP_DEV __device__ __forceinline__

// First index of the minimum over the wave from each lane's first minimum (best, ibest; no cell: INFINITY, 0x7fffffff).  Every lane
// takes part; a tie goes to the lower index.  best becomes the minimum on every lane; returns i0 (no cell compared below infinity,
// a table of NaN: 0, any start will do).
PP_DEV int pp_wave_first_min(double& best, int ibest, int Ns) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const double ob = __shfl_xor(best, m, 64);
    const int oi = __shfl_xor(ibest, m, 64);
    if (ob < best || (ob == best && oi < ibest)) { best = ob; ibest = oi; }
  }
  return ibest < Ns ? ibest : 0;
}

// Control points into LDS: c, zeros for the centre line, or with base the candidate clamp(base + c, lo, hi) (a NaN stays NaN).
PP_DEV void pp_load_points(double* cq, const double* c, int Nc, int lane, bool centre, const double* base, const double* lo, const double* hi) {
#pragma clang fp contract(off)
  for (int j = lane; j < Nc; j += 64) {
    double cj = centre ? 0.0 : c[j];
    if (base) {
      cj = base[j] + cj;
      cj = cj < lo[j] ? lo[j] : (cj > hi[j] ? hi[j] : cj);
    }
    cq[j] = cj;
  }
}

// Centre-line curvature, heading offset and |dp/ds| of every cell into kq, mq, rq.  True if the plan is NaN: some cell has
// a = 1 - n kappa < 0.1 (a line that folds over the centre of a corner) or NaN control points.  All 64 lanes call it.
PP_DEV bool pp_line_geometry(const Spl& sp, const double* cq, int Ns, int Nc, double ds, double h, int lane, int per, double* kq, double* mq,
                             double* rq) {
#pragma clang fp contract(off)
  bool a_ok = true;
  for (int it = 0; it < per; ++it) {
    const int i = lane + 64 * it;
    if (i < Ns) {
      const double k = kappa(sp, (double)i * ds);
      const RlPoint q = rl_point(cq, i, Ns, Nc, h, k);
      a_ok = a_ok && (q.a >= 0.1);
      kq[i] = k; mq[i] = q.mu; rq[i] = q.r;
    }
  }
  return __any(!a_ok) != 0;
}

// Curvature and length of the line per cell over kq and rq (own cell written, neighbours' heading offsets read)
PP_DEV void pp_line_curvature(double* kq, const double* mq, double* rq, int Ns, double ds, int lane, int per) {
#pragma clang fp contract(off)
  for (int it = 0; it < per; ++it) {
    const int i = lane + 64 * it;
    if (i < Ns) {
      const int pr = i > 0 ? i - 1 : Ns - 1, nx = i + 1 < Ns ? i + 1 : 0;
      const double r = rq[i];
      kq[i] = (kq[i] + (mq[nx] - mq[pr]) / (2.0 * ds)) / r;
      rq[i] = ds * r;
    }
  }
}

// Corner speed of every cell into vq; each lane keeps the first minimum among its cells (best, ibest).  CENTRE: the curvature is the
// centre line's, computed and kept in kq here; otherwise kq is read.
template <bool CENTRE>
PP_DEV void pp_corner_phase(const Spl& sp, double ds, double* kq, double* vq, int Ns, int lane, double A_lat, double v_cap, double& best, int& ibest) {
#pragma clang fp contract(off)
  best = INFINITY; ibest = 0x7fffffff;
  for (int i = lane; i < Ns; i += 64) {
    double k;
    if constexpr (CENTRE) { k = kappa(sp, (double)i * ds); kq[i] = k; } else { k = kq[i]; }
    const double vl = pp_corner_speed(k, A_lat, v_cap);
    vq[i] = vl;
    if (vl < best) { best = vl; ibest = i; }
  }
}

PP_DEV void pp_nan_table(double* tab, double* tt, int Ns, int lane) {   // this plan is NaN, the others are unaffected
  for (int i = lane; i < Ns; i += 64) {
    tt[i] = NAN;
    for (int c = 0; c < 8; ++c) tab[(size_t)i * 8 + c] = NAN;
  }
}

// The planner's 8 values of cell i and its traversal time (cyclic successor): offset n, heading offset mu, length dl.  dl / v is the
// reference's ds / s_d (dynamic_minimum_time_planner.m:73-83).
PP_DEV void pp_table_row(double WB, int i, int Ns, const double* kq, const double* vq, double dl, double n, double mu, double* tab, double* tt) {
#pragma clang fp contract(off)
  const int nx = i + 1 < Ns ? i + 1 : 0;
  const double v = vq[i], vn = vq[nx], k = kq[i], kn = kq[nx];
  const double delta = atan(WB * k), delta_n = atan(WB * kn);
  const double ti = dl / v;
  double* row = tab + (size_t)i * 8;
  row[0] = n; row[1] = mu; row[2] = v; row[3] = 0.0; row[4] = v * k; row[5] = delta;
  row[6] = (vn * vn - v * v) / (2.0 * dl);
  row[7] = (delta_n - delta) / ti;
  tt[i] = ti;
}
#endif
