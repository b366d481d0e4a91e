// raceline.hip -- the minimum-curvature racing line of the s-domain plans, batched on the device.
//
//   raceline_qp_kernel        H and g of the line QP (min summed squared second difference of the line's points over the control
//                             points of the lateral offset).  They depend on the track, N_s and N_c only: one workgroup, one lane
//                             per control point, each summing its band row over the cells that touch it in ascending cell order
//                             (no atomics: the same bits on every run).  The band sits in LDS; every lane then writes its row of
//                             the dense H, zeros included, upper and lower triangle from the same band entry.
//   raceline_bounds_kernel    per plan: lb = -w_p, ub = +w_p (w_p = N_MAX_p - margin) and the plan's copy of g (the solver reads
//                             g per instance)
//   plan_line_profile_kernel  plan_profile_kernel (planner.hip) on a line: offset, heading offset, length and curvature of every
//                             cell from the control points, then the same corner speed, recurrences and rows with the cell's
//                             own length.  One wavefront per plan; curvature, speed and cell length sit in LDS.
// The solve between them is the library's own (qp_solve_launch through fsaempc_qp_solve_batch_device_s: nC = 0, shared H).
#include <hip/hip_runtime.h>
#include <math.h>
#include "raceline.h"
#include "mpc_params.h"
#include "cl_frame.h"   // (compiled as in planner.hip: the pragma below comes after it)

// plain IEEE operations in source order (no FMA contraction): restated operation for operation in tests/raceline_numpy.py
#pragma clang fp contract(off)

namespace {

struct TrackFrame {   // centre point and unit left normal at s_i = i ds (curvilinear_to_cartesian.m:16-23)
  Spl sp; double ds;
  DEVINL RlFrame operator()(int i) const {
    const double s = (double)i * ds;
    double X, Xd, Xdd, Y, Yd, Ydd;
    spline3(sp.xP, sp.M, sp.dl, s, X, Xd, Xdd);
    spline3(sp.yP, sp.M, sp.dl, s, Y, Yd, Ydd);
    const double tx = -Yd, ty = Xd;
    const double nrm = sqrt(tx * tx + ty * ty);
    return RlFrame{X, Y, tx / nrm, ty / nrm};
  }
};

__global__ void __launch_bounds__(256) raceline_qp_kernel(RacelineQpParams P) {
  extern __shared__ double lds[];   // the band: N_c x RL_BAND
  const int j = threadIdx.x, Nc = P.N_c;
  if (j < Nc) {
    const TrackFrame frame{Spl{P.spM, P.spdl, P.xP, P.yP}, P.ds};
    double band[RL_BAND], gj;
    rl_row(frame, j, P.N_s, Nc, P.ds, band, gj);
#pragma unroll
    for (int c = 0; c < RL_BAND; ++c) lds[j * RL_BAND + c] = band[c];
    P.g[j] = gj;
  }
  __syncthreads();
  if (j < Nc)
    for (int k = 0; k < Nc; ++k) P.H[(size_t)k * Nc + j] = rl_H_entry(lds, j, k, Nc);   // (column k, row j: lanes write neighbouring addresses)
}

template <class PAR> __global__ void __launch_bounds__(64) raceline_bounds_kernel(RacelineBoundsParams P, typename PAR::Args pa) {
  const int plan = blockIdx.x, Nc = P.N_c;
  const PAR p = par_get<PAR>(pa, plan);
  double w = p.N_MAX - P.margin;
  if (p.bad || !(w > 0.0) || !(w < INFINITY)) w = 1.0;   // (no usable width: any box will do, plan_line_profile_kernel makes this plan NaN)
  for (int j = threadIdx.x; j < Nc; j += 64) {
    P.lb[(size_t)plan * Nc + j] = -w;
    P.ub[(size_t)plan * Nc + j] = w;
    if (plan > 0) P.g[(size_t)plan * Nc + j] = P.g[j];
  }
}

// plan_ax of planner.hip (the same text: that unit is not to change)
template <bool DYN, class PAR> DEVINL double line_ax(const PAR& p, double v, double K, double A_lat, double grip) {
  if constexpr (!DYN) {
    return grip * p.U_ACC_MAX;
  } else {
    const double y = fmin(v * v * K / A_lat, 1.0);
    double c0 = 1.0, c1 = 0.8660254037844386, s0 = 0.0, s1 = 0.5;                        // edge 0
    if (!(y <= 0.5)) { c0 = 0.8660254037844386; c1 = 0.5; s0 = 0.5; s1 = 0.8660254037844386; }   // edge 1
    if (!(y <= 0.8660254037844386)) { c0 = 0.5; c1 = 0.0; s0 = 0.8660254037844386; s1 = 1.0; }   // edge 2
    const double X = c0 + (c1 - c0) * (y - s0) / (s1 - s0);
    return fmin(p.U_ACC_MAX, grip * p.ELL_LONG * X);
  }
}

template <bool DYN, class PAR> __global__ void __launch_bounds__(64) plan_line_profile_kernel(PlanLineParams P, typename PAR::Args pa) {
  extern __shared__ double lds[];
  const int plan = blockIdx.x, lane = threadIdx.x, Ns = P.N_s, Nc = P.N_c;
  const int per = (Ns + 63) / 64;   // cells per lane: every loop below runs `per` times on every lane
  double* kq = lds;              // Ns: curvature of the centre line, then of the line
  double* vq = lds + Ns;         // Ns: heading offset, then speed
  double* dq = lds + 2 * Ns;     // Ns: |dp/ds|, then the cell's length on the line
  double* cq = lds + 3 * Ns;     // Nc: control points
  double* tab = P.table + (size_t)plan * Ns * 8;
  double* tt = P.t + (size_t)plan * Ns;
  double* lout = P.line_out ? P.line_out + (size_t)plan * Nc : nullptr;
  const PAR p = par_get<PAR>(pa, plan);
  const bool flagged = P.flag && P.flag[plan] != 0;   // the QP of this plan was not solved: the centre line
  bool nan_plan = p.bad || (P.check_width && !(p.N_MAX - P.margin > 0.0));   // (uniform over the wave)
  const Spl sp{P.spM, P.spdl, P.xP, P.yP};
  const double ds = P.ds, grip = P.grip;

  if (!nan_plan) {
    const double* c = P.line + (size_t)plan * P.line_stride;
    for (int j = lane; j < Nc; j += 64) cq[j] = flagged ? 0.0 : c[j];
    __syncthreads();
    // centre-line curvature, heading offset and |dp/ds| of every cell; the smallest a = 1 - n kappa of the lane's cells
    bool a_ok = true;
    for (int it = 0; it < per; ++it) {
      const int i = lane + 64 * it;
      if (i < Ns) {
        const double k = kappa(sp, (double)i * ds);
        const RlPoint q = rl_point(cq, i, Ns, Nc, P.h, k);
        a_ok = a_ok && (q.a >= 0.1);
        kq[i] = k; vq[i] = q.mu; dq[i] = q.r;
      }
    }
    nan_plan = __any(!a_ok) != 0;   // (all 64 lanes are here: a line that folds over the centre of a corner, or NaN control points)
  }
  if (nan_plan) {   // (uniform over the wave) this plan is NaN, the others are unaffected
    for (int i = lane; i < Ns; i += 64) {
      tt[i] = NAN;
      for (int c = 0; c < 8; ++c) tab[(size_t)i * 8 + c] = NAN;
    }
    if (lout) for (int j = lane; j < Nc; j += 64) lout[j] = NAN;
    return;
  }
  if (lout) for (int j = lane; j < Nc; j += 64) lout[j] = cq[j];
  __syncthreads();

  // curvature and length of the line per cell (own cell written, neighbours' heading offsets read)
  for (int it = 0; it < per; ++it) {
    const int i = lane + 64 * it;
    if (i < Ns) {
      const int pr = i > 0 ? i - 1 : Ns - 1, nx = i + 1 < Ns ? i + 1 : 0;
      const double r = dq[i];
      kq[i] = (kq[i] + (vq[nx] - vq[pr]) / (2.0 * ds)) / r;
      dq[i] = ds * r;
    }
  }
  __syncthreads();

  const double A_lat = grip * (DYN ? p.ELL_LAT : p.ALAT_MAX);
  // grip-limited corner speed of every cell; each lane keeps the first minimum among its cells
  double best = INFINITY; int ibest = 0x7fffffff;
  for (int it = 0; it < per; ++it) {
    const int i = lane + 64 * it;
    if (i < Ns) {
      const double K = fmax(fabs(kq[i]), 1e-12);
      const double vl = fmin(P.v_cap, sqrt(A_lat / K));
      vq[i] = vl;
      if (vl < best) { best = vl; ibest = i; }
    }
  }
  // first index of the minimum over the wave (every lane takes part; a tie goes to the lower index)
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const double ob = __shfl_xor(best, m, 64);
    const int oi = __shfl_xor(ibest, m, 64);
    if (ob < best || (ob == best && oi < ibest)) { best = ob; ibest = oi; }
  }
  const int i0 = ibest < Ns ? ibest : 0;
  __syncthreads();

  if (lane == 0) {   // the two recurrences of 6i with the cells' own lengths
    double vp = vq[i0]; int i = i0;
    for (int j = 1; j <= Ns; ++j) {                 // forward: acceleration out of the slower predecessor, over the predecessor's cell
      const int pr = i;
      i = i + 1; if (i >= Ns) i = 0;
      const double Kp = fmax(fabs(kq[pr]), 1e-12);
      const double a = line_ax<DYN>(p, vp, Kp, A_lat, grip);
      const double v = fmin(vq[i], sqrt(vp * vp + 2.0 * a * dq[pr]));
      vq[i] = v; vp = v;
    }
    vp = vq[i0]; i = i0;
    for (int j = 1; j <= Ns; ++j) {                 // backward: braking into the slower successor, over the cell being set
      const int nx = i;
      i = i - 1; if (i < 0) i = Ns - 1;
      const double Kn = fmax(fabs(kq[nx]), 1e-12);
      const double a = line_ax<DYN>(p, vp, Kn, A_lat, grip);
      const double v = fmin(vq[i], sqrt(vp * vp + 2.0 * a * dq[i]));
      vq[i] = v; vp = v;
    }
  }
  __syncthreads();

  for (int it = 0; it < per; ++it) {   // the planner's 8 values per cell and the cell's traversal time (cyclic successor)
    const int i = lane + 64 * it;
    if (i < Ns) {
      const int n = i + 1 < Ns ? i + 1 : 0;
      const double v = vq[i], vn = vq[n], k = kq[i], kn = kq[n], dl = dq[i];
      const RlPoint q = rl_point(cq, i, Ns, Nc, P.h, kappa(sp, (double)i * ds));
      const double delta = atan(p.WB * k), delta_n = atan(p.WB * kn);
      const double ti = dl / v;
      double* row = tab + (size_t)i * 8;
      row[0] = q.n; row[1] = q.mu; row[2] = v; row[3] = 0.0; row[4] = v * k; row[5] = delta;
      row[6] = (vn * vn - v * v) / (2.0 * dl);
      row[7] = (delta_n - delta) / ti;
      tt[i] = ti;
    }
  }
}

template <bool DYN> hipError_t line_launch(const PlanLineParams& P, const double* par, int par_stride, hipStream_t st) {
  const size_t lds = sizeof(double) * ((size_t)3 * (size_t)P.N_s + (size_t)P.N_c);
  if (par) hipLaunchKernelGGL((plan_line_profile_kernel<DYN, RtPar>), dim3(P.n_plans), dim3(64), lds, st, P, ParArgs{par, par_stride, nullptr});
  else hipLaunchKernelGGL((plan_line_profile_kernel<DYN, FixedPar>), dim3(P.n_plans), dim3(64), lds, st, P, NoParArgs{});
  return hipGetLastError();
}

}  // namespace

hipError_t raceline_qp_launch(const RacelineQpParams& P, hipStream_t st) {
  hipLaunchKernelGGL(raceline_qp_kernel, dim3(1), dim3(256), sizeof(double) * (size_t)P.N_c * RL_BAND, st, P);
  return hipGetLastError();
}
hipError_t raceline_bounds_launch(const RacelineBoundsParams& P, const double* par, int par_stride, hipStream_t st) {
  if (P.n_plans == 0) return hipSuccess;
  if (par) hipLaunchKernelGGL((raceline_bounds_kernel<RtPar>), dim3(P.n_plans), dim3(64), 0, st, P, ParArgs{par, par_stride, nullptr});
  else hipLaunchKernelGGL((raceline_bounds_kernel<FixedPar>), dim3(P.n_plans), dim3(64), 0, st, P, NoParArgs{});
  return hipGetLastError();
}
hipError_t plan_line_profile_launch(const PlanLineParams& P, const double* par, int par_stride, hipStream_t st) {
  if (P.n_plans == 0) return hipSuccess;
  return P.dynamic ? line_launch<true>(P, par, par_stride, st) : line_launch<false>(P, par, par_stride, st);
}
