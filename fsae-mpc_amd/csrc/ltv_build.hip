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
#include <hip/hip_runtime.h>
#include <math.h>
#include "ltv_build.h"
#include "nlp_model.h"
#include "ltv_model.h"

namespace {

// Exact linearisation of one step of the NLP's rollout: Ad = dPsi/dx, Bd = dPsi/du at (xi, ui), one dual-number pass of psi_step per
// column (true df/dx including kappa'(s), classical RK4 stage derivatives).
template <int NX, class PAR> DEVINL void linearise_exact(const PAR p, const double* xi, const double* ui, const Spl& sp, double dt, int integ, double* Ad, double* Bd) {
  for (int c = 0; c < NX + 2; ++c) {
    Dl xd[NX], ud[2], xn[NX];
    for (int j = 0; j < NX; ++j) xd[j] = Dl(xi[j], j == c ? 1.0 : 0.0);
    for (int j = 0; j < 2; ++j) ud[j] = Dl(ui[j], NX + j == c ? 1.0 : 0.0);
    psi_step<NX>(p, xd, ud, sp, dt, integ, xn);
    double* col = c < NX ? Ad + c * NX : Bd + (c - NX) * NX;
    for (int r = 0; r < NX; ++r) col[r] = xn[r].d;
  }
}

// ---------------------------------------------------------------------------------------------
// EXACT = false: the LTV build of the reference (quirks C-1, C-3, C-4/C-5, C-8 kept; bitwise pinned by the parity tests).
// EXACT = true: the QP of the NLP of DESIGN.md "Nonlinear MPC: batched SQP" at u = u_lin: x_lin is not read, the states are the
// rollout x_k = Psi(x_{k-1}, u_k) (x_0 = x0), step k is linearised exactly at (x_{k-1}, u_k), Phi(i,i) = Bd_i, every constraint row
// is linearised at the rollout state it constrains, and pred receives the rollout (the affine offset of the QP, rollout - Phi u_lin,
// stays internal).
// state weights of the cost (ltvmpc_*.m:32) and the factor the terminal step carries (:33), as the unparameterised VJP chain reads them
constexpr double QW[3] = {FixedPar::QW[0], FixedPar::QW[1], FixedPar::QW[2]};
constexpr double QTERM = FixedPar::Q_TERMINAL;

// PAR: the constants (mpc_params.h).  FixedPar: the shipped build, pa is empty.  RtPar: the constants of the instance's block, loaded
// once through uniform addresses (pa.idx: the batch instance behind this workgroup, for sub-batches).
template <int NX, bool EXACT, class PAR> __global__ __launch_bounds__(256) void ltv_build_kernel(LtvParams P, typename PAR::Args pa) {
  const PAR p = par_get<PAR>(pa, blockIdx.x);
  constexpr int NN = NX * NX, NS = (NX == 5) ? 1 : 4, RPK = (NX == 5) ? 6 : 20;  // rows per step
  const int b = blockIdx.x, tid = threadIdx.x, nth = blockDim.x;
  const int N = P.N, R = NX * N, nV = 2 * N + NS, nC = RPK * N;
  const double dt = P.dt;
  Spl sp{P.spM, P.spdl, P.xP, P.yP};
  const double* x0 = P.x0 + (size_t)b * NX;
  const double* x_ref = P.x_ref + (size_t)b * R;
  const double* x_lin = P.x_lin + (size_t)b * R;
  const double* u_lin = P.u_lin + (size_t)b * 2 * N;
  double* H = P.H + (size_t)b * nV * nV;
  double* g = P.g + (size_t)b * nV;
  double* A = P.A + (size_t)b * nC * nV;
  double* lb = P.lb + (size_t)b * nV; double* ub = P.ub + (size_t)b * nV;
  double* lbA = P.lbA + (size_t)b * nC; double* ubA = P.ubA + (size_t)b * nC;
  double* Bt = P.Bt + (size_t)b * R * nV;

  extern __shared__ double sm[];
  double* Ad = sm;                 // N * NN
  double* Bd = Ad + (size_t)N * NN;  // N * NX*2 (only slice 0 is used by the condensing, kept for clarity)
  double* dd = Bd + (size_t)N * NX * 2;  // N * NX
  double* aff = dd + (size_t)N * NX;     // R   : A_bar*x0 + d_bar
  double* cc = aff + R;                  // per-step constraint coefficient scratch: N * CW
  constexpr int CW = (NX == 5) ? 3 : (2 * 4 + 2 + 4 + 2);  // kin: C3,C4,const ; dyn: slip rows (2x4 coef + 2 const), tyre (4 coef K-part) + 2
  double* red = cc + (size_t)N * CW;     // reduction scratch (nth)
  double* ell = red + nth;               // 24: dac[12], dal[12] of the inscribed 12-gon (dynamic_tyre_linearise_constraints.m:33-39)
  double* colst = ell + 24;              // one column of Bt (R doubles) per wavefront: stage of step 4c
  double* xs = colst + (size_t)(nth >> 6) * R;   // EXACT: rollout x_0 .. x_N ((N + 1) * NX)
  double* ell0 = xs + (EXACT ? (size_t)(N + 1) * NX : 0);   // runtime constants only: 24 more, ac0[12], al0[12] of the same 12-gon

  if (tid < 12) {
    const int j = tid;
    const double th0 = 2 * M_PI * (double)j / 12, th1 = (j + 1 == 12) ? 2 * M_PI : 2 * M_PI * (double)(j + 1) / 12;
    ell[j] = p.ELL_LAT * sin(th1) - p.ELL_LAT * sin(th0); ell[12 + j] = p.ELL_LONG * cos(th1) - p.ELL_LONG * cos(th0);
    if constexpr (PAR::RT) { ell0[j] = p.ELL_LAT * sin(th0); ell0[12 + j] = p.ELL_LONG * cos(th0); }
  }
  if constexpr (EXACT) {
    if (tid == 0) {
      for (int j = 0; j < NX; ++j) xs[j] = x0[j];
      for (int k = 0; k < N; ++k) psi_step<NX>(p, xs + (size_t)k * NX, u_lin + (size_t)k * 2, sp, dt, P.integ, xs + (size_t)(k + 1) * NX);
    }
    __syncthreads();
  }
  // ---- 1. linearise every step (one thread per step) ----
  for (int k = tid; k < N; k += nth) {
    if constexpr (EXACT) {
      const double* xi = xs + (size_t)k * NX;
      const double* ui = u_lin + (size_t)k * 2;
      double* a = Ad + (size_t)k * NN; double* bd = Bd + (size_t)k * NX * 2; double* d = dd + (size_t)k * NX;
      linearise_exact<NX>(p, xi, ui, sp, dt, P.integ, a, bd);
      for (int r = 0; r < NX; ++r) {     // dd_k = x_k - Ad_k x_{k-1} - Bd_k u_k: the recursion of step 2 reproduces the rollout at u_lin
        double v = xi[NX + r];
        for (int c = 0; c < NX; ++c) v -= a[r + c * NX] * xi[c];
        for (int c = 0; c < 2; ++c) v -= bd[r + c * NX] * ui[c];
        d[r] = v;
      }
    } else {
      linearise_step<NX>(p, x_lin + (size_t)k * NX, u_lin + (size_t)k * 2, sp, dt, P.integ, Ad + (size_t)k * NN, Bd + (size_t)k * NX * 2, dd + (size_t)k * NX);
    }
  }
  // zero Bt while the linearisation runs
  for (size_t i = tid; i < (size_t)R * nV; i += nth) Bt[i] = 0.0;
  __syncthreads();

  // ---- 2. prediction offset aff_k = Ad_k aff_{k-1} + dd_k, aff_0 = x0 (== A_bar*x0 + d_bar) ----
  if (tid == 0) {
    double cur[NX], nxt[NX];
    for (int j = 0; j < NX; ++j) cur[j] = x0[j];
    for (int k = 0; k < N; ++k) {
      const double* a = Ad + (size_t)k * NN;
      for (int r = 0; r < NX; ++r) {
        double s = dd[k * NX + r];
        for (int c = 0; c < NX; ++c) s += a[r + c * NX] * cur[c];
        nxt[r] = s;
      }
      for (int r = 0; r < NX; ++r) { cur[r] = nxt[r]; aff[k * NX + r] = nxt[r]; }
    }
  }
  // ---- 3. Phi columns: Phi(i,i) = Bd_1 (always slice 1, quirk C-1), Phi(j,i) = Ad_j Phi(j-1,i) ----
  for (int w = tid; w < 2 * N; w += nth) {
    const int i = w >> 1, col = w & 1;
    double cur[NX], nxt[NX];
    const double* bdi = EXACT ? Bd + (size_t)i * NX * 2 : Bd;
    for (int r = 0; r < NX; ++r) cur[r] = bdi[r + col * NX];
    double* dst = Bt + (size_t)w * R;
    for (int r = 0; r < NX; ++r) dst[i * NX + r] = cur[r];
    for (int j = i + 1; j < N; ++j) {
      const double* a = Ad + (size_t)j * NN;
      for (int r = 0; r < NX; ++r) {
        double s = 0;
        for (int c = 0; c < NX; ++c) s += a[r + c * NX] * cur[c];
        nxt[r] = s;
      }
      for (int r = 0; r < NX; ++r) { cur[r] = nxt[r]; dst[j * NX + r] = nxt[r]; }
    }
  }
  // ---- 4a. per-step constraint coefficients ----
  for (int k = tid; k < N; k += nth) {
    const double* xl = EXACT ? xs + (size_t)(k + 1) * NX : x_lin + (size_t)k * NX;   // (default: pairing quirk C-8)
    step_coef<NX>(p, xl, sp, cc + (size_t)k * CW);
  }
  __syncthreads();

  // (runtime constants: the linearisation above needs the vehicle entries, everything below the limits and the cost; the block is
  //  read a second time here instead of holding all of it in SGPRs across the linearisation)
  const PAR pl = par_get_again<PAR>(pa, blockIdx.x);
  // ---- 4b. variable bounds (ltvmpc_*.m:28-29) and constraint bounds ----
  for (int i = tid; i < nV; i += nth) {
    if (i < 2 * N) { lb[i] = (i & 1) ? -pl.U_STEER_MAX : -pl.U_ACC_MAX; ub[i] = (i & 1) ? pl.U_STEER_MAX : pl.U_ACC_MAX; }
    else { lb[i] = 0.0; ub[i] = INFINITY; }
  }
  const int vidx = 3, didx = NX - 1, nidx = 1, scol = 2 * N;
  for (int k = tid; k < N; k += nth) {
    const double cv = aff[k * NX + vidx], cd = aff[k * NX + didx], cn = aff[k * NX + nidx];
    lbA[k] = pl.V_MIN - cv;              ubA[k] = INFINITY;
    lbA[N + k] = -pl.DELTA_MAX - cd;     ubA[N + k] = pl.DELTA_MAX - cd;
    lbA[2 * N + k] = -pl.N_MAX - cn;     ubA[2 * N + k] = 1e10;    // *_state_constraints.m:38-39
    lbA[3 * N + k] = -1e10;             ubA[3 * N + k] = pl.N_MAX - cn;
    const double* xl = EXACT ? xs + (size_t)(k + 1) * NX : x_lin + (size_t)k * NX;
    const double* ck = cc + (size_t)k * CW;
    if (NX == 5) {
      const double cst = ck[2] + ck[0] * (aff[k * NX + 3] - xl[3]) + ck[1] * (aff[k * NX + 4] - xl[4]);
      lbA[4 * N + k] = -pl.ALAT_MAX - cst;  ubA[4 * N + k] = INFINITY;
      lbA[5 * N + k] = -INFINITY;          ubA[5 * N + k] = pl.ALAT_MAX - cst;
    } else {
      const double* ul = u_lin + (size_t)k * 2;
      for (int q = 0; q < 2; ++q) {
        double cst = ck[8 + q];
        for (int j = 0; j < 4; ++j) cst += ck[4 * q + j] * (aff[k * NX + 3 + j] - xl[3 + j]);
        lbA[4 * N + 2 * k + q] = -pl.SLIP_MAX - cst; ubA[4 * N + 2 * k + q] = INFINITY;
        lbA[6 * N + 2 * k + q] = -INFINITY;         ubA[6 * N + 2 * k + q] = pl.SLIP_MAX - cst;
      }
      for (int j = 0; j < 12; ++j) {
        double ac0, al0, dac, dal;
        if constexpr (PAR::RT) {   // the table of this instance's ellipse
          ac0 = ell0[j]; al0 = ell0[12 + j]; dac = ell[j]; dal = ell[12 + j];
        } else {                   // constants of the compiler
          const double th0 = 2 * M_PI * (double)j / 12, th1 = (j + 1 == 12) ? 2 * M_PI : 2 * M_PI * (double)(j + 1) / 12;
          const double ac1 = pl.ELL_LAT * sin(th1), al1 = pl.ELL_LONG * cos(th1);
          ac0 = pl.ELL_LAT * sin(th0); al0 = pl.ELL_LONG * cos(th0);
          dac = ac1 - ac0; dal = al1 - al0;
        }
        double cst = (ul[0] - al0) * dac - (ck[13] / pl.M - ac0) * dal;
        for (int jj = 0; jj < 3; ++jj) cst += dal * ck[10 + jj] * (aff[k * NX + 3 + jj] - xl[3 + jj]);
        cst -= dac * ul[0];
        lbA[8 * N + 12 * k + j] = -INFINITY; ubA[8 * N + 12 * k + j] = 0 - cst;
      }
    }
  }
  // ---- 4c. constraint matrix A (nC x nV, column-major).  One column at a time per wavefront: the column of Bt (R doubles,
  // contiguous) is staged in LDS with coalesced loads, then the nC entries of that column of A are formed from it and stored
  // with coalesced stores.  (Round 2 swept all entries with one thread each and read Bt with stride NX: 4.2 of the 10.3 ms of a
  // dynamic N = 60 batch.)  The 12 half-plane directions of the tyre ellipse come from a small LDS table. ----
  {
    const int lane = tid & 63, wv = tid >> 6, nwv = nth >> 6;
    double* bc = colst + (size_t)wv * R;                     // this wave's column stage
    for (int col = wv; col < nV; col += nwv) {
      const bool inp = col < 2 * N;                          // input column: a column of Bt; slack column: unit entries only
      for (int i = lane; i < R; i += 64) bc[i] = inp ? Bt[(size_t)col * R + i] : 0.0;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      double* acol = A + (size_t)col * nC;
      for (int row = lane; row < nC; row += 64) {
        double v = 0.0;
        if (row < 4 * N) {
          const int blk = row / N, k = row - blk * N;
          const int idx = blk == 0 ? vidx : (blk == 1 ? didx : nidx);
          v = bc[k * NX + idx];
          if (col == scol && blk == 2) v = 1.0;
          if (col == scol && blk == 3) v = -1.0;
        } else if (NX == 5) {
          const int blk = (row - 4 * N) / N, k = row - 4 * N - blk * N;
          const double* ck = cc + (size_t)k * CW;
          v = ck[0] * bc[k * NX + 3] + ck[1] * bc[k * NX + 4];
          if (col == scol) v = blk == 0 ? 1.0 : -1.0;   // shared slack (quirk C-7)
        } else if (row < 8 * N) {
          const int blk = (row - 4 * N) / (2 * N), rr = row - 4 * N - blk * 2 * N, k = rr >> 1, q = rr & 1;
          const double* ck = cc + (size_t)k * CW;
          for (int j = 0; j < 4; ++j) v += ck[4 * q + j] * bc[k * NX + 3 + j];
          if (col == scol + 1 + q) v = blk == 0 ? 1.0 : -1.0;
        } else {
          const int rr = row - 8 * N, k = rr / 12, j = rr - 12 * k;
          const double* ck = cc + (size_t)k * CW;
          const double dac = ell[j], dal = ell[12 + j];
          for (int jj = 0; jj < 3; ++jj) v += dal * ck[10 + jj] * bc[k * NX + 3 + jj];
          if (col == 2 * k) v += dac;
          if (col == scol + 3) v = -1.0;
        }
        acol[row] = v;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
  }
  // ---- 5. H = 2 (Bt' Qbar Bt + Rbar), g = 2 Bt' Qbar r  (generate_qp.m:29-31); only states 1..3 carry weight ----
  // The input block of H is a SYRK over the 3N weighted rows of Bt: on the matrix cores (v_mfma_f64_16x16x4_f64), one 16 x 16 tile
  // pair (I >= J) per wavefront at a time, operands gathered from Bt (column-major, just written by this workgroup: L2), k-steps
  // started at the first block row in which column tile I is non-zero (Bt is block lower-triangular).  (Round 2 computed every
  // entry as a scalar dot product with stride-NX loads: 3.5 of the 10.3 ms of a dynamic N = 60 batch, 0.95 of 2.26 ms on the
  // headline shape.)  Lane (c = l & 15, q = l >> 4): A operand = weight * Bt[row rho][16 I + c], B operand = Bt[row rho][16 J + c],
  // rho = 4 s + q over the weighted rows (k, r) = (rho / 3, rho % 3); result register p holds H[16 I + q + 4 p][16 J + c].
  const double Qw[3] = {pl.QW[0], pl.QW[1], pl.QW[2]};   // ltvmpc_*.m:32 ; Q_terminal = 10 Q (:33)
  {
    const int lane = tid & 63, wv = tid >> 6, nwv = nth >> 6, c = lane & 15, q = lane >> 4;
    const int nU = 2 * N, Tu = (nU + 15) >> 4, npairs = Tu * (Tu + 1) / 2, ksteps = (3 * N + 3) >> 2;
    for (int pidx = wv; pidx < npairs; pidx += nwv) {
      int I = 0;
      while ((I + 1) * (I + 2) / 2 <= pidx) ++I;
      const int J = pidx - I * (I + 1) / 2;                      // I >= J
      const int ci = 16 * I + c, cj = 16 * J + c;
      const double* pi_ = Bt + (size_t)(ci < nU ? ci : 0) * R;
      const double* pj_ = Bt + (size_t)(cj < nU ? cj : 0) * R;
      const bool oni = ci < nU, onj = cj < nU;
      v4d acc = {0.0, 0.0, 0.0, 0.0};
      const int s0 = (3 * 8 * I) >> 2;                            // column tile I starts at stage 8 I: weighted row 24 I
      int rho = 4 * s0 + q, k = rho / 3, r = rho - 3 * k;
      constexpr int UN = 8;                                       // k-steps per round: all 2 UN gathers in flight before the first MFMA
      for (int s = s0; s < ksteps; s += UN) {
        double av[UN], bv[UN];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
          const bool on = k < N;                                  // (rows beyond 3N: zero operands; the address stays inside Bt)
          const int off = (on ? k : 0) * NX + r;
          const double wq = ((k == N - 1) ? pl.Q_TERMINAL : 1.0) * (r == 0 ? Qw[0] : (r == 1 ? Qw[1] : Qw[2]));
          const double a_ = pi_[off], b_ = pj_[off];
          av[u] = (on && oni) ? wq * a_ : 0.0;
          bv[u] = (on && onj) ? b_ : 0.0;
          rho += 4; ++r; ++k; if (r == 3) { r = 0; ++k; }        // rho + 4 = 3 (k + 1) + (r + 1)
        }
#pragma unroll
        for (int u = 0; u < UN; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], bv[u], acc, 0, 0, 0);
      }
#pragma unroll
      for (int pp = 0; pp < 4; ++pp) {
        const int i = 16 * I + q + 4 * pp, j = cj;
        if (i < nU && j < nU) {
          const double v = 2.0 * (acc[pp] + (i == j ? ((i & 1) ? pl.R_STEER : pl.R_ACC) : 0.0));   // R = [10,10] (ltvmpc_*.m:34)
          H[(size_t)i + (size_t)j * nV] = v;
          H[(size_t)j + (size_t)i * nV] = v;
        }
      }
    }
    // slack rows / columns of H carry no quadratic cost
    for (int e = tid; e < NS * nV; e += nth) {
      const int sc = 2 * N + e / nV, i = e - (e / nV) * nV;
      H[(size_t)i + (size_t)sc * nV] = 0.0;
      H[(size_t)sc + (size_t)i * nV] = 0.0;
    }
  }
  double qc_local = 0.0;
  for (int i = tid; i < nV; i += nth) {
    double s = 0.0;
    if (i < 2 * N) {
      const double* ci = Bt + (size_t)i * R;
      for (int k = i >> 1; k < N; ++k) {
        const double wq = (k == N - 1) ? pl.Q_TERMINAL : 1.0;
        for (int r = 0; r < 3; ++r) s += ci[k * NX + r] * (wq * Qw[r]) * (aff[k * NX + r] - x_ref[k * NX + r]);
      }
      g[i] = 2 * s;
    } else {
      const int sidx = i - 2 * N;
      g[i] = (NX == 5 || sidx == 0) ? pl.R_SOFT0 : (sidx == 3 ? pl.R_SOFT3 : (sidx == 1 ? pl.R_SOFT1 : pl.R_SOFT2));   // R_soft (ltvmpc_*.m:35)
    }
    if constexpr (PAR::RT) { if (pl.bad) g[i] = NAN; }   // a block that cannot describe a car: the solve returns -1 for this instance

  }
  for (int e = tid; e < 3 * N; e += nth) {
    const int k = e / 3, r = e - 3 * k;
    const double wq = (k == N - 1) ? pl.Q_TERMINAL : 1.0;
    const double rr = aff[k * NX + r] - x_ref[k * NX + r];
    qc_local += rr * (wq * Qw[r]) * rr;
  }
  red[tid] = qc_local;
  __syncthreads();
  if (tid == 0) {
    double s = 0; for (int i = 0; i < nth; ++i) s += red[i];
    if (P.qconst) P.qconst[b] = s;
  }
  if (P.pred) for (int i = tid; i < R; i += nth) P.pred[(size_t)b * R + i] = EXACT ? xs[NX + i] : aff[i];
}

// post-solve: x_opt = aff + Bt z ; u_opt = z(1:2N) ; slack ; fval += const   (ltvmpc_*.m:57-60)
__global__ void ltv_post_kernel(int nx, int N, int ns, const double* z, const double* pred, const double* Bt, const double* qconst,
                                double* u_opt, double* x_opt, double* slack, double* fval) {
  const int b = blockIdx.x, tid = threadIdx.x, nth = blockDim.x;
  const int R = nx * N, nV = 2 * N + ns;
  const double* zb = z + (size_t)b * nV;
  const double* Btb = Bt + (size_t)b * R * nV;
  for (int r = tid; r < R; r += nth) {
    double s = pred[(size_t)b * R + r];
    for (int c = 0; c < nV; ++c) s += Btb[r + (size_t)c * R] * zb[c];
    x_opt[(size_t)b * R + r] = s;
  }
  for (int c = tid; c < 2 * N; c += nth) u_opt[(size_t)b * 2 * N + c] = zb[c];
  for (int c = tid; c < ns; c += nth) slack[(size_t)b * ns + c] = zb[2 * N + c];
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

size_t ltv_build_lds_bytes(int nx, int N, int threads, bool exact, bool par) {
  const int CW = (nx == 5) ? 3 : 16;
  return ((size_t)N * nx * nx + (size_t)N * nx * 2 + (size_t)N * nx + (size_t)nx * N + (size_t)N * CW + threads + 24 +
          (size_t)(threads / 64) * nx * N +    // the per-wavefront column stage of step 4c
          (exact ? (size_t)(N + 1) * nx : 0) +                     // the rollout of the NLP build
          (par ? 24 : 0)) * sizeof(double);                       // the second half of the ellipse table of a parameter block
}

template <int NX, bool EXACT> static hipError_t launch_build(const LtvParams& P, int batch, hipStream_t st) {
  const int threads = 256;
  const size_t lds = ltv_build_lds_bytes(NX, P.N, threads, EXACT);
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&ltv_build_kernel<NX, EXACT, FixedPar>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((ltv_build_kernel<NX, EXACT, FixedPar>), dim3(batch), dim3(threads), lds, st, P, NoParArgs{});
  return hipGetLastError();
}

template <int NX, bool EXACT> static hipError_t launch_build_par(const LtvParams& P, const ParArgs& pa, int batch, hipStream_t st) {
  const int threads = 256;
  const size_t lds = ltv_build_lds_bytes(NX, P.N, threads, EXACT, true);
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&ltv_build_kernel<NX, EXACT, RtPar>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((ltv_build_kernel<NX, EXACT, RtPar>), dim3(batch), dim3(threads), lds, st, P, pa);
  return hipGetLastError();
}

hipError_t ltv_build_par_launch(const LtvParams& P, const double* values, int stride, const int* idx, int batch, hipStream_t st, bool exact) {
  const ParArgs pa{values, stride, idx};
  if (exact) return P.nx == 5 ? launch_build_par<5, true>(P, pa, batch, st) : launch_build_par<7, true>(P, pa, batch, st);
  return P.nx == 5 ? launch_build_par<5, false>(P, pa, batch, st) : launch_build_par<7, false>(P, pa, batch, st);
}

hipError_t ltv_build_launch(const LtvParams& P, int batch, hipStream_t st, bool exact) {
  if (exact) return P.nx == 5 ? launch_build<5, true>(P, batch, st) : launch_build<7, true>(P, batch, st);
  return P.nx == 5 ? launch_build<5, false>(P, batch, st) : launch_build<7, false>(P, batch, st);
}

hipError_t ltv_post_launch(int nx, int N, int ns, int batch, const double* z, const double* pred, const double* Bt, const double* qconst,
                           double* u_opt, double* x_opt, double* slack, double* fval, hipStream_t st) {
  hipLaunchKernelGGL(ltv_post_kernel, dim3(batch), dim3(256), 0, st, nx, N, ns, z, pred, Bt, qconst, u_opt, x_opt, slack, fval);
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
