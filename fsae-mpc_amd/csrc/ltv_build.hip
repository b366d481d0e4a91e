// ltv_build.hip -- QP construction of one LTV-MPC step, batched, on MI355X (gfx950).
//
// Replaces (reference file:line):
//   spline/interpolate_spline_d.m:11-21, interpolate_spline_dd.m:11-21, interpolate_curvature.m:12-18   (kappa)
//   vehicle_models/curvilinear_kinematic/{f,A,B}_curv_kin.m, vehicle_models/curvilinear_dynamic/{f,A,B}_curv_dyn.m
//   mpc/ltv/kinematic/rk2_kinematic_curvilinear.m:25-50, mpc/ltv/dynamic/rk4_dynamic_curvilinear.m:25-59
//   mpc/ltv/sequential_integration.m:16-47 (condensing; the prediction offset A_bar*x0+d_bar is produced by
//        the equivalent one-step recursion instead of materialising the dense D matrix of :38-47)
//   mpc/ltv/kinematic/kinematic_state_constraints.m:11-48, kinematic_tyre_linearise_constraints.m:18-32
//   mpc/ltv/dynamic/dynamic_state_constraints.m:11-57, dynamic_slip_linearise_constraints.m:20-44,
//        dynamic_tyre_linearise_constraints.m:18-61
//   mpc/ltv/generate_qp.m:23-33 with the weights/limits of ltvmpc_*_curvilinear.m:20-35
// One 256-thread workgroup per instance.  Reference quirks are preserved: the diagonal block
// of B_bar is always slice 1, RK4's dkdu4 uses dt/2, A_curv_dyn is the Jacobian definition, shared kinematic slack.
// The build kernel's body is ltv_build_kernel.h; this unit instantiates it without blocks (kinematic / dynamic, LTV / exact,
// constants compiled in / parameter blocks: eight kernels; the four blocked ones are ltv_build_blocked.hip's) and holds the one
// launch, the LDS size, the post-solve kernel and the sensitivity kernels.
#include "ltv_build_kernel.h"

namespace {

// state weights of the cost (ltvmpc_*.m:32) and the factor the terminal step carries (:33), as the unparameterised VJP chain reads them
constexpr double QW[3] = {FixedPar::QW[0], FixedPar::QW[1], FixedPar::QW[2]};
constexpr double QTERM = FixedPar::Q_TERMINAL;

// post-solve: x_opt = aff + Bt z ; u_opt = z(1:2N), with blocks (bm.M > 0) the held values expanded to the N steps (u_k = v_block(k)) ;
// slack ; fval += const   (ltvmpc_*.m:57-60)
__global__ void ltv_post_kernel(int nx, int N, int ns, LtvBlockMap bm, const double* z, const double* pred, const double* Bt,
                                const double* qconst, double* u_opt, double* x_opt, double* slack, double* fval) {
  const int b = blockIdx.x, tid = threadIdx.x, nth = blockDim.x;
  const int M = bm.M ? bm.M : N, R = nx * N, nV = 2 * M + ns;
  const double* zb = z + (size_t)b * nV;
  const double* Btb = Bt + (size_t)b * R * nV;
  for (int r = tid; r < R; r += nth) {
    double s = pred[(size_t)b * R + r];
    for (int c = 0; c < nV; ++c) s += Btb[r + (size_t)c * R] * zb[c];
    x_opt[(size_t)b * R + r] = s;
  }
  for (int c = tid; c < 2 * N; c += nth) {
    int j = c >> 1;
    if (bm.M) { j = 0; while (j + 1 < M && (int)bm.start[j + 1] <= (c >> 1)) ++j; }
    u_opt[(size_t)b * 2 * N + c] = zb[2 * j + (c & 1)];
  }
  for (int c = tid; c < ns; c += nth) slack[(size_t)b * ns + c] = zb[2 * M + c];
  if (tid == 0) fval[b] += qconst[b];
}

// ---- sensitivities: the build is affine in x0 and x_ref once x_lin, u_lin are fixed ----
// Row `row` of the constraint block belongs to step row_step(): its bounds move by -Crow_row . pred_k (rows 0..4N: a unit
// coefficient on v, delta, n; the linearised rows: the coefficients of step 4a, as step 4b applies them).
template <int NX> DEVINL int row_step(int row, int N) {
  if (row < 4 * N) return row % N;
  if (NX == 5) return (row - 4 * N) % N;
  if (row < 8 * N) return ((row - 4 * N) % (2 * N)) >> 1;
  return (row - 8 * N) / 12;
}
template <int NX> DEVINL void row_coef(int row, int N, const double* ck, double* crow) {   // ck: the 4a coefficients of the row's step
  for (int j = 0; j < NX; ++j) crow[j] = 0.0;
  if (row < 4 * N) { const int blk = row / N; crow[blk == 0 ? 3 : (blk == 1 ? NX - 1 : 1)] = 1.0; return; }
  if (NX == 5) { crow[3] = ck[0]; crow[4] = ck[1]; return; }
  if (row < 8 * N) { const int q = ((row - 4 * N) % (2 * N)) & 1; for (int j = 0; j < 4; ++j) crow[3 + j] = ck[4 * q + j]; return; }
  const int j = (row - 8 * N) % 12;
  const double th0 = 2 * M_PI * (double)j / 12, th1 = (j + 1 == 12) ? 2 * M_PI : 2 * M_PI * (double)(j + 1) / 12;
  const double dal = FixedPar::ELL_LONG * cos(th1) - FixedPar::ELL_LONG * cos(th0);
  for (int jj = 0; jj < 3; ++jj) crow[3 + jj] = dal * ck[10 + jj];
}

// Abar (R x NX, column-major): d pred / d x0 = Ad_k ... Ad_1; Crow (nC x NX, column-major).  One workgroup per instance; the
// linearisation and the 4a coefficients are the build's own device functions at the same points.
template <int NX> __global__ __launch_bounds__(256) void ltv_affine_kernel(LtvParams P, double* Abar, double* Crow) {
  constexpr int NN = NX * NX, RPK = (NX == 5) ? 6 : 20, CW = (NX == 5) ? 3 : 16;
  const int b = blockIdx.x, tid = threadIdx.x, nth = blockDim.x, N = P.N, R = NX * N, nC = RPK * N;
  Spl sp{P.spM, P.spdl, P.xP, P.yP};
  const double* x_lin = P.x_lin + (size_t)b * R;
  const double* u_lin = P.u_lin + (size_t)b * 2 * N;
  extern __shared__ double sm[];
  double* Ad = sm; double* Bd = Ad + (size_t)N * NN; double* dd = Bd + (size_t)N * NX * 2; double* cc = dd + (size_t)N * NX;
  for (int k = tid; k < N; k += nth) {
    linearise_step<NX>(FixedPar{}, x_lin + (size_t)k * NX, u_lin + (size_t)k * 2, sp, P.dt, P.integ, Ad + (size_t)k * NN, Bd + (size_t)k * NX * 2, dd + (size_t)k * NX);
    step_coef<NX>(FixedPar{}, x_lin + (size_t)k * NX, sp, cc + (size_t)k * CW);
  }
  __syncthreads();
  double* Ab = Abar + (size_t)b * R * NX;
  if (tid < NX) {   // column tid: e_tid pushed through the recursion aff_k = Ad_k aff_{k-1}
    double cur[NX], nxt[NX];
    for (int j = 0; j < NX; ++j) cur[j] = j == tid ? 1.0 : 0.0;
    for (int k = 0; k < N; ++k) {
      const double* a = Ad + (size_t)k * NN;
      for (int r = 0; r < NX; ++r) { double v = 0.0; for (int c = 0; c < NX; ++c) v += a[r + c * NX] * cur[c]; nxt[r] = v; }
      for (int r = 0; r < NX; ++r) { cur[r] = nxt[r]; Ab[(size_t)k * NX + r + (size_t)tid * R] = nxt[r]; }
    }
  }
  double* Cr = Crow + (size_t)b * nC * NX;
  for (int row = tid; row < nC; row += nth) {
    double crow[NX];
    row_coef<NX>(row, N, cc + (size_t)row_step<NX>(row, N) * CW, crow);
    for (int j = 0; j < NX; ++j) Cr[row + (size_t)j * nC] = crow[j];
  }
}

// Cotangent of the QP's variables from the step's: zbar = [ubar; sbar] + Bt' xbar (x_opt = pred + Bt z), one column per block.y;
// z = [u_opt; slack] (the forward's QP solution).
__global__ void ltv_vjp_pre_kernel(int nx, int N, int ns, int kc, const double* Bt, const double* u_opt, const double* slack,
                                   const double* ubar, const double* xbar, const double* sbar, double* z, double* zbar) {
  const int b = blockIdx.x, c = blockIdx.y, tid = threadIdx.x, nth = blockDim.x;
  const int R = nx * N, nV = 2 * N + ns;
  const double* Btb = Bt + (size_t)b * R * nV;
  const size_t col = (size_t)b * kc + c;
  for (int i = tid; i < nV; i += nth) {
    double s = 0.0;
    if (i < 2 * N) s = ubar ? ubar[col * 2 * N + i] : 0.0;
    else s = sbar ? sbar[col * ns + i - 2 * N] : 0.0;
    if (xbar) for (int e = 0; e < R; ++e) s += Btb[e + (size_t)i * R] * xbar[col * R + e];
    zbar[col * nV + i] = s;
    if (c == 0) z[(size_t)b * nV + i] = i < 2 * N ? u_opt[(size_t)b * 2 * N + i] : slack[(size_t)b * ns + i - 2 * N];
  }
}

// The transposed affine maps: pred receives xbar (x_opt), 2 Qbar Bt gbar (g = 2 Bt' Qbar (pred - x_ref)), -Crow'(lbAbar + ubAbar)
// (row shifts) and 2 fbar Qbar (pred - x_ref) (qconst); x_ref receives minus the g and qconst parts; x0bar = Abar' predbar.
// Instances whose QP VJP failed (status < 0) get zeros.  One workgroup per (instance, column).
template <int NX> __global__ __launch_bounds__(256) void ltv_vjp_chain_kernel(int N, int kc, const double* Bt, const double* pred,
    const double* x_ref, const double* Abar, const double* Crow, const double* gbar, const double* lbAbar, const double* ubAbar,
    const double* xbar, const double* fbar, const int* status, double* x0bar, double* xrefbar) {
  constexpr int NS = (NX == 5) ? 1 : 4, RPK = (NX == 5) ? 6 : 20;
  const int b = blockIdx.x, c = blockIdx.y, tid = threadIdx.x, nth = blockDim.x;
  const int R = NX * N, nV = 2 * N + NS, nC = RPK * N;
  const size_t col = (size_t)b * kc + c;
  const bool ok = status[b] >= 0;
  extern __shared__ double pb[];   // R: cotangent of pred
  const double* Btb = Bt + (size_t)b * R * nV;
  const double* gb = gbar + col * nV;
  const double fb = fbar ? fbar[col] : 0.0;
  for (int e = tid; e < R; e += nth) {
    const int k = e / NX, r = e - k * NX;
    double p = xbar ? xbar[col * R + e] : 0.0, xr = 0.0;
    if (r < 3) {
      double G = 0.0;
      for (int i = 0; i < 2 * N; ++i) G += Btb[e + (size_t)i * R] * gb[i];
      const double w = ((k == N - 1) ? QTERM : 1.0) * QW[r];
      const double d = pred[(size_t)b * R + e] - x_ref[(size_t)b * R + e];
      const double t = 2.0 * w * G + 2.0 * fb * w * d;
      p += t; xr = -t;
    }
    pb[e] = p;
    if (xrefbar) xrefbar[col * R + e] = ok ? xr : 0.0;
  }
  __syncthreads();
  // rows of each step, in a fixed order per state: deterministic sums
  for (int e = tid; e < R; e += nth) {
    const int k = e / NX, j = e - k * NX;
    double s = 0.0;
    for (int row = 0; row < nC; ++row) {
      if (row_step<NX>(row, N) != k) continue;
      const double cr = Crow[(size_t)b * nC * NX + row + (size_t)j * nC];
      if (cr != 0.0) s += cr * (lbAbar[col * nC + row] + ubAbar[col * nC + row]);
    }
    pb[e] -= s;
  }
  __syncthreads();
  if (tid < NX) {
    double s = 0.0;
    for (int e = 0; e < R; ++e) s += Abar[(size_t)b * R * NX + e + (size_t)tid * R] * pb[e];
    x0bar[col * NX + tid] = ok ? s : 0.0;
  }
}

}  // namespace

// the kernel's LDS carve (ltv_build_kernel.h), term by term
size_t ltv_build_lds_bytes(int nx, int N, int threads, bool exact, bool par, int M) {
  const size_t CW = (nx == 5) ? 3 : 16, R = (size_t)nx * N;
  return ((size_t)N * nx * nx +                 // Ad
          (size_t)N * nx * 2 +                  // Bd
          (size_t)N * nx +                      // dd
          R +                                   // aff
          (size_t)N * CW +                      // cc
          threads +                             // red
          24 +                                  // ell
          (size_t)(threads / 64) * R +          // colst: the per-wavefront column stage of step 4c
          (exact ? (size_t)(N + 1) * nx : 0) +  // xs: the rollout of the NLP build
          (par || M ? 24 : 0)) * sizeof(double) +   // ell0: the second half of the ellipse table (read with a parameter block)
         (M ? (size_t)(M + 1 + N) : 0) * sizeof(int);   // bst, bos: the block map
}

// The kinematic default block (fsaempc_ltv_default_params) on the device, for the one build that is routed through its RtPar kernel.
// No device code names it: external linkage and `used` keep it in the code object, where hipGetSymbolAddress looks it up (a static
// or const one is dropped from the device side and the lookup aborts).  Nothing writes it.
__device__ __attribute__((used)) double fsaempc_kin_default_block[FSAEMPC_NPAR] = {
    FixedPar::M, FixedPar::IZ, FixedPar::LF, FixedPar::LR, FixedPar::GRAV, FixedPar::PB, FixedPar::PC, FixedPar::PD, FixedPar::PE,
    FixedPar::QW[0], FixedPar::QW[1], FixedPar::QW[2], FixedPar::Q_TERMINAL, FixedPar::R_ACC, FixedPar::R_STEER,
    FixedPar::R_SOFT0, 0, 0, 0, FixedPar::U_ACC_MAX, FixedPar::U_STEER_MAX, FixedPar::DELTA_MAX, FixedPar::N_MAX, FixedPar::V_MIN,
    FixedPar::ALAT_MAX, FixedPar::SLIP_MAX, FixedPar::ELL_LONG, FixedPar::ELL_LAT,
    FixedPar::PID_KP_V, FixedPar::PID_MAX_F, FixedPar::PID_KP_D, FixedPar::PID_MAX_DRATE};

hipError_t ltv_build_launch(const LtvParams& P, const LtvBlockMap* bm, const double* values, int stride, const int* idx, int batch,
                            hipStream_t st, bool exact) {
  if (bm) return exact ? hipErrorNotSupported : ltv_build_launch_blocked_unit(P, *bm, values, stride, idx, batch, st);
  // The exact kinematic build under RK4 with the constants compiled in, ltv_build_kernel<5, true, false, FixedPar>, returned wrong
  // linearisations (NaN or wrong Ad_k, Bd_k of whole steps, other steps in other runs) on the MI355X while its rollout stayed right;
  // the cause is not established.  Its RtPar sibling with the default block is the same arithmetic and does not, so
  // that one combination runs there: one block shared by the batch (stride 0).  Euler and RK2, the kinematic default, are not moved.
  if (exact && !values && P.nx == 5 && P.integ != 0 && P.integ != 1) {
    const double* block = nullptr;
    hipError_t e = hipGetSymbolAddress((void**)&block, HIP_SYMBOL(fsaempc_kin_default_block));
    if (e != hipSuccess) return e;
    return select_build<false>(P, nullptr, block, 0, nullptr, batch, st, true);
  }
  return select_build<false>(P, nullptr, values, stride, idx, batch, st, exact);
}

hipError_t ltv_post_launch(int nx, int N, int ns, const LtvBlockMap* bm, int batch, const double* z, const double* pred, const double* Bt,
                           const double* qconst, double* u_opt, double* x_opt, double* slack, double* fval, hipStream_t st) {
  hipLaunchKernelGGL(ltv_post_kernel, dim3(batch), dim3(256), 0, st, nx, N, ns, bm ? *bm : LtvBlockMap{}, z, pred, Bt, qconst, u_opt, x_opt, slack, fval);
  return hipGetLastError();
}

size_t ltv_affine_lds_bytes(int nx, int N) {
  const int CW = (nx == 5) ? 3 : 16;
  return ((size_t)N * nx * nx + (size_t)N * nx * 2 + (size_t)N * nx + (size_t)N * CW) * sizeof(double);
}

hipError_t ltv_affine_launch(const LtvParams& P, int batch, double* Abar, double* Crow, hipStream_t st) {
  const size_t lds = ltv_affine_lds_bytes(P.nx, P.N);
  const void* f = P.nx == 5 ? reinterpret_cast<const void*>(&ltv_affine_kernel<5>) : reinterpret_cast<const void*>(&ltv_affine_kernel<7>);
  hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  if (P.nx == 5) hipLaunchKernelGGL(ltv_affine_kernel<5>, dim3(batch), dim3(256), lds, st, P, Abar, Crow);
  else hipLaunchKernelGGL(ltv_affine_kernel<7>, dim3(batch), dim3(256), lds, st, P, Abar, Crow);
  return hipGetLastError();
}

hipError_t ltv_vjp_pre_launch(int nx, int N, int ns, int batch, int kc, const double* Bt, const double* u_opt, const double* slack,
                              const double* ubar, const double* xbar, const double* sbar, double* z, double* zbar, hipStream_t st) {
  hipLaunchKernelGGL(ltv_vjp_pre_kernel, dim3(batch, kc), dim3(256), 0, st, nx, N, ns, kc, Bt, u_opt, slack, ubar, xbar, sbar, z, zbar);
  return hipGetLastError();
}

hipError_t ltv_vjp_chain_launch(int nx, int N, int batch, int kc, const double* Bt, const double* pred, const double* x_ref,
                                const double* Abar, const double* Crow, const double* gbar, const double* lbAbar, const double* ubAbar,
                                const double* xbar, const double* fbar, const int* status, double* x0bar, double* xrefbar, hipStream_t st) {
  const size_t lds = (size_t)nx * N * sizeof(double);
  if (nx == 5) hipLaunchKernelGGL(ltv_vjp_chain_kernel<5>, dim3(batch, kc), dim3(256), lds, st, N, kc, Bt, pred, x_ref, Abar, Crow, gbar, lbAbar, ubAbar, xbar, fbar, status, x0bar, xrefbar);
  else hipLaunchKernelGGL(ltv_vjp_chain_kernel<7>, dim3(batch, kc), dim3(256), lds, st, N, kc, Bt, pred, x_ref, Abar, Crow, gbar, lbAbar, ubAbar, xbar, fbar, status, x0bar, xrefbar);
  return hipGetLastError();
}
