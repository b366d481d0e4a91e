// raceline.h -- the minimum-curvature racing line of the s-domain plans: the per-cell geometry, written once for the
// host and the device, and the internal interface between the C ABI and the kernels of raceline.hip.
//
// The line is a lateral offset n(s) from the centre line, a uniform periodic cubic B-spline with N_c control points (knot spacing
// h = L / N_c) sampled at the N_s cells s_i = i ds of a plan.  Its points are p_i = c_i + n_i nu_i (centre point and unit left normal
// of the track, vehicle_models/curvilinear_to_cartesian.m:19-26), n = B c.
//
//   rl_basis / rl_weights / rl_dweights   cell -> first control point and the four weights (and their derivatives in u)
//   rl_offset_row  cell -> the offset n_i as a row of the control points: first column and the four weights
//   rl_cell        the second difference of the line's points at one cell as a function of the control points: at most five
//                  consecutive control points take part (N_s >= 2 N_c), so a cell is two local rows of five and the constant d_i
//   rl_row         one row of the band of H = 2 ds G'G and one entry of g = 2 ds G'd: the sum over the cells that touch the control
//                  point, in ascending cell order
//   rl_H_entry     the dense, exactly symmetric H from the band
//   rl_point       n, n', a = 1 - n kappa, r, mu of the line at one cell (the inputs of the speed profile on the line)
//
// The frame of a cell (c_i, nu_i) comes from a callable, so the host program of tests/test_raceline_cpu.py includes this file without
// the HIP headers.  No FMA contraction: tests/raceline_numpy.py restates every function operation for operation.
#pragma once
#include <math.h>
#include <stddef.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RL_HD __host__ __device__ __forceinline__
#else
#define RL_HD inline
#endif

#define RL_BAND 9   // candidates of a band row: columns j .. j + 4 and the up to four columns that reach j round the closed lap

struct RlFrame { double cx, cy, nx, ny; };   // centre point and unit left normal of a cell

// q = i N_c / N_s in exact integer arithmetic: j = floor(q), u = q - j
RL_HD void rl_basis(int i, int Ns, int Nc, int& j, double& u) {
  const long long q = (long long)i * (long long)Nc;
  j = (int)(q / Ns);
  u = (double)(q % Ns) / (double)Ns;
}

// weights of the control points j - 1 .. j + 2 (cyclic) at local coordinate u; non-negative, sum 1
RL_HD void rl_weights(double u, double* w) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double m = 1.0 - u;
  w[0] = m * m * m / 6.0;
  w[1] = (3.0 * u * u * u - 6.0 * u * u + 4.0) / 6.0;
  w[2] = (-3.0 * u * u * u + 3.0 * u * u + 3.0 * u + 1.0) / 6.0;
  w[3] = u * u * u / 6.0;
}

// d w / d u (divide by h for d / ds)
RL_HD void rl_dweights(double u, double* w) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double m = 1.0 - u;
  w[0] = -3.0 * m * m / 6.0;
  w[1] = (9.0 * u * u - 12.0 * u) / 6.0;
  w[2] = (-9.0 * u * u + 6.0 * u + 3.0) / 6.0;
  w[3] = 3.0 * u * u / 6.0;
}

// The offset at cell i as a row of the control points: n_i = sum_m w[m] c[(col0 + m) mod N_c], col0 = (j_i - 1) mod N_c.  The row of
// the cell-wise corridor constraints; with N_c >= 4 the four columns are distinct.
RL_HD void rl_offset_row(int i, int Ns, int Nc, int& col0, double* w) {
  int j; double u;
  rl_basis(i, Ns, Nc, j, u);
  rl_weights(u, w);
  col0 = j > 0 ? j - 1 : Nc - 1;
}

// first control point (cyclic) of the five a cell's second difference can touch: cell i - 1 starts the window
RL_HD int rl_cell_base(int i, int Ns, int Nc) {
  int j; double u;
  rl_basis(i > 0 ? i - 1 : Ns - 1, Ns, Nc, j, u);
  return j > 0 ? j - 1 : Nc - 1;
}

// Second difference of the line's points at cell i: (p_{i+1} - 2 p_i + p_{i-1}) / ds^2 = G_i c + d_i, with G_i zero outside the control
// points base .. base + 4 (cyclic).  gx, gy: the two local rows of G_i; dx, dy: d_i.
struct RlCell { int base; double gx[5], gy[5], dx, dy; };

template <class F> RL_HD RlCell rl_cell(const F& frame, int i, int Ns, int Nc, double ds) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  RlCell c;
  for (int a = 0; a < 5; ++a) { c.gx[a] = 0.0; c.gy[a] = 0.0; }
  const int cell[3] = {i > 0 ? i - 1 : Ns - 1, i, i + 1 < Ns ? i + 1 : 0};
  const double coef[3] = {1.0, -2.0, 1.0};
  RlFrame f[3];
  int j0 = 0;
  for (int m = 0; m < 3; ++m) {
    f[m] = frame(cell[m]);
    int j; double u, w[4];
    rl_basis(cell[m], Ns, Nc, j, u);
    rl_weights(u, w);
    if (m == 0) j0 = j;
    int o = j - j0;
    if (o < 0) o += Nc;   // 0 or 1: three neighbouring cells span at most one knot (N_s >= 2 N_c)
    for (int k = 0; k < 4; ++k) {
      const double vx = coef[m] * f[m].nx * w[k], vy = coef[m] * f[m].ny * w[k];
      if (o == 0) { c.gx[k] += vx; c.gy[k] += vy; } else { c.gx[k + 1] += vx; c.gy[k + 1] += vy; }
    }
  }
  const double ds2 = ds * ds;
  for (int a = 0; a < 5; ++a) { c.gx[a] = c.gx[a] / ds2; c.gy[a] = c.gy[a] / ds2; }
  c.dx = (f[2].cx - 2.0 * f[1].cx + f[0].cx) / ds2;
  c.dy = (f[2].cy - 2.0 * f[1].cy + f[0].cy) / ds2;
  c.base = j0 > 0 ? j0 - 1 : Nc - 1;
  return c;
}

// The band of row j holds H_jk for the columns k >= j within cyclic distance 4: candidate c = 0 .. 4 is k = j + c, candidate
// c = 5 .. 8 is k = j + N_c - (c - 4) (a pair joined round the closed lap; rows j < 4 only).  -1: no such column.
RL_HD int rl_band_col(int j, int c, int Nc) {
  if (c <= 4) return j + c < Nc ? j + c : -1;
  const int k = j + Nc - (c - 4);
  return (k < Nc && k > j + 4) ? k : -1;
}
// candidate index of the pair j <= k in row j's band, -1: H_jk = 0
RL_HD int rl_band_index(int j, int k, int Nc) {
  const int d = k - j;
  if (d <= 4) return d;
  if (Nc - d <= 4) return 4 + (Nc - d);
  return -1;
}
// entry (j, k) of the dense H from the band (Nc x RL_BAND): the value computed for the ordered pair, mirrored
RL_HD double rl_H_entry(const double* band, int j, int k, int Nc) {
  const int lo = j < k ? j : k, hi = j < k ? k : j;
  const int c = rl_band_index(lo, hi, Nc);
  return c >= 0 ? band[(size_t)lo * RL_BAND + c] : 0.0;
}

template <int N> RL_HD double rl_pick(const double* v, int a) {   // v[a] without a dynamic index into registers
  double r = v[0];
  for (int q = 1; q < N; ++q) r = a == q ? v[q] : r;
  return r;
}

// Row j of the band and g_j.  The cells whose window holds control point j are visited in ascending cell order (a range that runs
// over the start of the lap is split), every sum in that order: the result does not depend on who computes it.
template <class F> RL_HD void rl_row(const F& frame, int j, int Ns, int Nc, double ds, double* band, double& gj) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double acc[RL_BAND], g = 0.0;
  int col[RL_BAND];
  for (int c = 0; c < RL_BAND; ++c) { acc[c] = 0.0; col[c] = rl_band_col(j, c, Nc); }
  // a superset of the cells that touch j (their predecessor's first control point is j - 3 .. j + 1); each is tested below
  const long long nlo = (long long)(j - 3) * Ns, nhi = (long long)(j + 2) * Ns;
  const int lo = (int)(nlo >= 0 ? nlo / Nc : -((-nlo + Nc - 1) / Nc)), hi = (int)(nhi / Nc) + 1;   // floor of both quotients
  int a0 = lo, a1 = hi, b0 = 1, b1 = 0;   // [a0, a1] then [b0, b1], actual cell indices
  if (hi - lo + 1 >= Ns) { a0 = 0; a1 = Ns - 1; }
  else if (lo < 0) { a0 = 0; a1 = hi; b0 = lo + Ns; b1 = Ns - 1; }
  else if (hi >= Ns) { a0 = 0; a1 = hi - Ns; b0 = lo; b1 = Ns - 1; }
  for (int part = 0; part < 2; ++part) {
    const int i0 = part == 0 ? a0 : b0, i1 = part == 0 ? a1 : b1;
    for (int i = i0; i <= i1; ++i) {
      int aj = j - rl_cell_base(i, Ns, Nc);
      if (aj < 0) aj += Nc;
      if (aj > 4) continue;
      const RlCell ce = rl_cell(frame, i, Ns, Nc, ds);
      const double xj = rl_pick<5>(ce.gx, aj), yj = rl_pick<5>(ce.gy, aj);
      for (int c = 0; c < RL_BAND; ++c) {
        if (col[c] < 0) continue;
        int ak = col[c] - ce.base;
        if (ak < 0) ak += Nc;
        if (ak > 4) continue;
        acc[c] += xj * rl_pick<5>(ce.gx, ak) + yj * rl_pick<5>(ce.gy, ak);
      }
      g += xj * ce.dx + yj * ce.dy;
    }
  }
  for (int c = 0; c < RL_BAND; ++c) band[c] = 2.0 * ds * acc[c];
  gj = 2.0 * ds * g;
}

// The line at cell i for control points c (N_c values): offset n, slope n' = dn/ds, a = 1 - n kappa, r = |dp/ds| and the heading
// offset mu.  With c = 0: n = 0, n' = 0, a = 1, r = 1, mu = 0 exactly.
struct RlPoint { double n, nd, a, r, mu; };
RL_HD RlPoint rl_point(const double* c, int i, int Ns, int Nc, double h, double kappa) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  int j; double u, w[4], wd[4];
  rl_basis(i, Ns, Nc, j, u);
  rl_weights(u, w);
  rl_dweights(u, wd);
  int k0 = j > 0 ? j - 1 : Nc - 1;
  double n = 0.0, nd = 0.0;
  for (int k = 0; k < 4; ++k) {
    const double ck = c[k0];
    n += w[k] * ck; nd += wd[k] * ck;
    k0 = k0 + 1 < Nc ? k0 + 1 : 0;
  }
  RlPoint p;
  p.n = n; p.nd = nd / h;
  p.a = 1.0 - p.n * kappa;
  p.r = sqrt(p.a * p.a + p.nd * p.nd);
  p.mu = atan(p.nd / p.a);
  return p;
}

#if defined(__HIPCC__)
// ---- internal interface between the C ABI (capi_plan.hip) and raceline.hip ----
struct RacelineQpParams {
  int N_s, N_c;
  double ds;
  int spM; double spdl; const double* xP; const double* yP;   // spline table (device)
  double* H;      // N_c x N_c, dense and symmetric
  double* g;      // N_c
};
hipError_t raceline_qp_launch(const RacelineQpParams& P, hipStream_t st);

// bounds of the line QP per plan (lb = -w_p, ub = +w_p, w_p = N_MAX_p - margin; a plan without a usable width gets a unit box, its
// profile is NaN anyway) and the copies of g the solver reads per instance (g: n_plans x N_c, row 0 filled by raceline_qp_launch)
struct RacelineBoundsParams { int n_plans, N_c; double margin; double* g; double* lb; double* ub; };
hipError_t raceline_bounds_launch(const RacelineBoundsParams& P, const double* par, int par_stride, hipStream_t st);

struct PlanLineParams {
  int dynamic, n_plans, N_s, N_c;
  double ds, h, v_cap, grip;
  int check_width; double margin;   // check_width: a plan with N_MAX_p - margin <= 0 is NaN
  int spM; double spdl; const double* xP; const double* yP;
  const double* line; int line_stride;   // control points: plan p reads line + p * line_stride (0: shared)
  const int* flag;          // optional, n_plans: a plan whose flag is not 0 takes the centre line
  double* line_out;         // optional, n_plans x N_c: the control points the profile was made on (zeros for a flagged plan, NaN for a NaN plan)
  double* table;            // n_plans x N_s x 8
  double* t;                // n_plans x N_s
};
hipError_t plan_line_profile_launch(const PlanLineParams& P, const double* par, int par_stride, hipStream_t st);
#endif
