// ltv_build_blocked.hip -- QP construction of one LTV-MPC step with move blocking (held inputs), batched, on MI355X (gfx950).
//
// The horizon's N steps are grouped into M blocks of consecutive steps and the input is held over each block: u_k = v_block(k).
// The QP's variables are [v_1 .. v_M; slacks] (nV_b = 2M + ns); its rows stay those of the unblocked problem (nC = 6N / 20N).  With
// E the (2N + ns) x (2M + ns) matrix that copies v_block(k) to step k, the blocked QP is H_b = E'HE, g_b = E'g, A_b = AE of the
// unblocked one (ltv_build.hip); this kernel forms it directly: 2M condensing recursions instead of 2N, nC x nV_b entries of A, a
// SYRK over 2M columns.  The linearisation, the prediction offset, the per-step row coefficients and every row bound do not depend
// on the blocking and are those of ltv_build_kernel (same device functions, ltv_model.h; reference quirks C-1 .. C-8 kept).
// One 256-thread workgroup per instance.  The block map (at most 98 small integers) travels in the kernel arguments.
#include <hip/hip_runtime.h>
#include <math.h>
#include "ltv_build.h"
#include "nlp_model.h"
#include "ltv_model.h"

namespace {

template <int NX, class PAR> __global__ __launch_bounds__(256) void ltv_build_blocked_kernel(LtvParams P, LtvBlockMap bm, typename PAR::Args pa) {
  const PAR p = par_get<PAR>(pa, blockIdx.x);
  constexpr int NN = NX * NX, NS = (NX == 5) ? 1 : 4, RPK = (NX == 5) ? 6 : 20;  // rows per step
  const int b = blockIdx.x, tid = threadIdx.x, nth = blockDim.x;
  const int N = P.N, M = bm.M, R = NX * N, nU = 2 * M, nV = nU + NS, nC = RPK * N;
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
  double* Bd = Ad + (size_t)N * NN;  // N * NX*2 (only slice 0 is used by the condensing: quirk C-1)
  double* dd = Bd + (size_t)N * NX * 2;  // N * NX
  double* aff = dd + (size_t)N * NX;     // R   : A_bar*x0 + d_bar
  double* cc = aff + R;                  // per-step constraint coefficient scratch: N * CW
  constexpr int CW = (NX == 5) ? 3 : (2 * 4 + 2 + 4 + 2);
  double* red = cc + (size_t)N * CW;     // reduction scratch (nth)
  double* ell = red + nth;               // 24: dac[12], dal[12] of the inscribed 12-gon
  double* colst = ell + 24;              // one column of Bt (R doubles) per wavefront: stage of step 4c
  double* ell0 = colst + (size_t)(nth >> 6) * R;   // 24: ac0[12], al0[12] (read with runtime constants only)
  int* bst = reinterpret_cast<int*>(ell0 + 24);    // M + 1: first step of every block, bst[M] = N
  int* bos = bst + (M + 1);                        // N: block of step k

  if (tid < 12) {
    const int j = tid;
    const double th0 = 2 * M_PI * (double)j / 12, th1 = (j + 1 == 12) ? 2 * M_PI : 2 * M_PI * (double)(j + 1) / 12;
    ell[j] = p.ELL_LAT * sin(th1) - p.ELL_LAT * sin(th0); ell[12 + j] = p.ELL_LONG * cos(th1) - p.ELL_LONG * cos(th0);
    if constexpr (PAR::RT) { ell0[j] = p.ELL_LAT * sin(th0); ell0[12 + j] = p.ELL_LONG * cos(th0); }
  }
  for (int j = tid; j <= M; j += nth) {
    const int s = bm.start[j], e = j < M ? bm.start[j + 1] : s;
    bst[j] = s;
    for (int k = s; k < e; ++k) bos[k] = j;
  }
  // ---- 1. linearise every step (one thread per step) ----
  for (int k = tid; k < N; k += nth)
    linearise_step<NX>(p, x_lin + (size_t)k * NX, u_lin + (size_t)k * 2, sp, dt, P.integ, Ad + (size_t)k * NN, Bd + (size_t)k * NX * 2, dd + (size_t)k * NX);
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
  // ---- 3. held-input columns: the response of the states to input c held over block j.  cur = Bd(:,c) at the block's first step,
  // then cur <- Ad_i cur + (i in block j ? Bd(:,c) : 0): the sum of the block's columns of Phi, one recursion per column.  Bd is
  // slice 1 at every step (quirk C-1).  The column's rows above the block are zero; they and the slack columns are written here too
  // (every entry of Bt once, no separate clearing pass). ----
  for (int w = tid; w < nV; w += nth) {
    double* dst = Bt + (size_t)w * R;
    if (w >= nU) { for (int e = 0; e < R; ++e) dst[e] = 0.0; continue; }
    const int j = w >> 1, col = w & 1, s0 = bst[j], s1 = bst[j + 1];
    double cur[NX], nxt[NX], bd0[NX];
    for (int r = 0; r < NX; ++r) { bd0[r] = Bd[r + col * NX]; cur[r] = bd0[r]; }
    for (int e = 0; e < s0 * NX; ++e) dst[e] = 0.0;
    for (int r = 0; r < NX; ++r) dst[s0 * NX + r] = cur[r];
    for (int i = s0 + 1; i < N; ++i) {
      const double* a = Ad + (size_t)i * NN;
      const bool in = i < s1;
      for (int r = 0; r < NX; ++r) {
        double s = in ? bd0[r] : 0.0;
        for (int c = 0; c < NX; ++c) s += a[r + c * NX] * cur[c];
        nxt[r] = s;
      }
      for (int r = 0; r < NX; ++r) { cur[r] = nxt[r]; dst[i * NX + r] = nxt[r]; }
    }
  }
  // ---- 4a. per-step constraint coefficients (pairing quirk C-8) ----
  for (int k = tid; k < N; k += nth) step_coef<NX>(p, x_lin + (size_t)k * NX, sp, cc + (size_t)k * CW);
  __syncthreads();

  // (runtime constants: read a second time, as in ltv_build_kernel)
  const PAR pl = par_get_again<PAR>(pa, blockIdx.x);
  // ---- 4b. variable bounds (ltvmpc_*.m:28-29) and constraint bounds: the rows and their bounds are those of the unblocked QP ----
  for (int i = tid; i < nV; i += nth) {
    if (i < nU) { lb[i] = (i & 1) ? -pl.U_STEER_MAX : -pl.U_ACC_MAX; ub[i] = (i & 1) ? pl.U_STEER_MAX : pl.U_ACC_MAX; }
    else { lb[i] = 0.0; ub[i] = INFINITY; }
  }
  const int vidx = 3, didx = NX - 1, nidx = 1, scol = nU;
  for (int k = tid; k < N; k += nth) {
    const double cv = aff[k * NX + vidx], cd = aff[k * NX + didx], cn = aff[k * NX + nidx];
    lbA[k] = pl.V_MIN - cv;              ubA[k] = INFINITY;
    lbA[N + k] = -pl.DELTA_MAX - cd;     ubA[N + k] = pl.DELTA_MAX - cd;
    lbA[2 * N + k] = -pl.N_MAX - cn;     ubA[2 * N + k] = 1e10;    // *_state_constraints.m:38-39
    lbA[3 * N + k] = -1e10;             ubA[3 * N + k] = pl.N_MAX - cn;
    const double* xl = x_lin + (size_t)k * NX;
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
  // ---- 4c. constraint matrix A_b (nC x nV_b, column-major), one column at a time per wavefront through its LDS column stage.  The
  // direct term of the tyre polygon (+dac on the acceleration input of the row's own step) lands in column 2 block(k). ----
  {
    const int lane = tid & 63, wv = tid >> 6, nwv = nth >> 6;
    double* bc = colst + (size_t)wv * R;                     // this wave's column stage
    for (int col = wv; col < nV; col += nwv) {
      const bool inp = col < nU;                             // block column: a column of Bt; slack column: unit entries only
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
          if (col == 2 * bos[k]) v += dac;
          if (col == scol + 3) v = -1.0;
        }
        acol[row] = v;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
  }
  // ---- 5. H_b = 2 (Bt_b' Qbar Bt_b + Rbar_b), g_b = 2 Bt_b' Qbar r; only states 1..3 carry weight.  The SYRK over the 3N weighted
  // rows of the 2M block columns runs on the matrix cores (v_mfma_f64_16x16x4_f64) with the lane maps of ltv_build_kernel: lane
  // (c = l & 15, q = l >> 4): A operand = weight * Bt[row rho][16 I + c], B operand = Bt[row rho][16 J + c], rho = 4 s + q over the
  // weighted rows (k, r) = (rho / 3, rho % 3); result register pp holds H[16 I + q + 4 pp][16 J + c].  Column tile I begins with
  // block 8 I, whose column is zero above its first step: k-steps start at weighted row 3 bst[8 I].  Rbar_b carries len_j R. ----
  const double Qw[3] = {pl.QW[0], pl.QW[1], pl.QW[2]};   // ltvmpc_*.m:32 ; Q_terminal = 10 Q (:33)
  {
    const int lane = tid & 63, wv = tid >> 6, nwv = nth >> 6, c = lane & 15, q = lane >> 4;
    const int Tu = (nU + 15) >> 4, npairs = Tu * (Tu + 1) / 2, ksteps = (3 * N + 3) >> 2;
    for (int pidx = wv; pidx < npairs; pidx += nwv) {
      int I = 0;
      while ((I + 1) * (I + 2) / 2 <= pidx) ++I;
      const int J = pidx - I * (I + 1) / 2;                      // I >= J
      const int ci = 16 * I + c, cj = 16 * J + c;
      const double* pi_ = Bt + (size_t)(ci < nU ? ci : 0) * R;
      const double* pj_ = Bt + (size_t)(cj < nU ? cj : 0) * R;
      const bool oni = ci < nU, onj = cj < nU;
      v4d acc = {0.0, 0.0, 0.0, 0.0};
      const int s0 = (3 * bst[8 * I]) >> 2;                       // (8 I < M: tile I holds at least one block column)
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
          const double len = (double)(bst[(i >> 1) + 1] - bst[i >> 1]);
          const double v = 2.0 * (acc[pp] + (i == j ? len * ((i & 1) ? pl.R_STEER : pl.R_ACC) : 0.0));   // R = [10,10] per held step
          H[(size_t)i + (size_t)j * nV] = v;
          H[(size_t)j + (size_t)i * nV] = v;
        }
      }
    }
    // slack rows / columns of H carry no quadratic cost
    for (int e = tid; e < NS * nV; e += nth) {
      const int sc = nU + e / nV, i = e - (e / nV) * nV;
      H[(size_t)i + (size_t)sc * nV] = 0.0;
      H[(size_t)sc + (size_t)i * nV] = 0.0;
    }
  }
  double qc_local = 0.0;
  for (int i = tid; i < nV; i += nth) {
    double s = 0.0;
    if (i < nU) {
      const double* ci = Bt + (size_t)i * R;
      for (int k = bst[i >> 1]; k < N; ++k) {
        const double wq = (k == N - 1) ? pl.Q_TERMINAL : 1.0;
        for (int r = 0; r < 3; ++r) s += ci[k * NX + r] * (wq * Qw[r]) * (aff[k * NX + r] - x_ref[k * NX + r]);
      }
      g[i] = 2 * s;
    } else {
      const int sidx = i - nU;
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
  if (P.pred) for (int i = tid; i < R; i += nth) P.pred[(size_t)b * R + i] = aff[i];
}

// post-solve: x_opt = pred + Bt_b z ; u_opt = the held values expanded to the N steps (u_k = v_block(k)) ; slack ; fval += const
__global__ void ltv_post_blocked_kernel(int nx, int N, int ns, LtvBlockMap bm, const double* z, const double* pred, const double* Bt,
                                        const double* qconst, double* u_opt, double* x_opt, double* slack, double* fval) {
  const int b = blockIdx.x, tid = threadIdx.x, nth = blockDim.x;
  const int M = bm.M, R = nx * N, nV = 2 * M + ns;
  const double* zb = z + (size_t)b * nV;
  const double* Btb = Bt + (size_t)b * R * nV;
  for (int r = tid; r < R; r += nth) {
    double s = pred[(size_t)b * R + r];
    for (int c = 0; c < nV; ++c) s += Btb[r + (size_t)c * R] * zb[c];
    x_opt[(size_t)b * R + r] = s;
  }
  for (int k = tid; k < N; k += nth) {
    int j = 0;
    while (j + 1 < M && (int)bm.start[j + 1] <= k) ++j;
    u_opt[(size_t)b * 2 * N + 2 * k] = zb[2 * j];
    u_opt[(size_t)b * 2 * N + 2 * k + 1] = zb[2 * j + 1];
  }
  for (int c = tid; c < ns; c += nth) slack[(size_t)b * ns + c] = zb[2 * M + c];
  if (tid == 0) fval[b] += qconst[b];
}

template <int NX, class PAR> hipError_t launch_blocked(const LtvParams& P, const LtvBlockMap& bm, const typename PAR::Args& pa, int batch, hipStream_t st) {
  const int threads = 256;
  const size_t lds = ltv_build_blocked_lds_bytes(NX, P.N, bm.M, threads);
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&ltv_build_blocked_kernel<NX, PAR>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((ltv_build_blocked_kernel<NX, PAR>), dim3(batch), dim3(threads), lds, st, P, bm, pa);
  return hipGetLastError();
}

}  // namespace

size_t ltv_build_blocked_lds_bytes(int nx, int N, int M, int threads) {
  const int CW = (nx == 5) ? 3 : 16;
  return ((size_t)N * nx * nx + (size_t)N * nx * 2 + (size_t)N * nx + (size_t)nx * N + (size_t)N * CW + threads + 24 +
          (size_t)(threads / 64) * nx * N + 24) * sizeof(double) + (size_t)(M + 1 + N) * sizeof(int);
}

hipError_t ltv_build_blocked_launch(const LtvParams& P, const LtvBlockMap& bm, const double* values, int stride, int batch, hipStream_t st) {
  if (values) {
    const ParArgs pa{values, stride, nullptr};
    return P.nx == 5 ? launch_blocked<5, RtPar>(P, bm, pa, batch, st) : launch_blocked<7, RtPar>(P, bm, pa, batch, st);
  }
  return P.nx == 5 ? launch_blocked<5, FixedPar>(P, bm, NoParArgs{}, batch, st) : launch_blocked<7, FixedPar>(P, bm, NoParArgs{}, batch, st);
}

hipError_t ltv_post_blocked_launch(int nx, int N, int ns, const LtvBlockMap& bm, int batch, const double* z, const double* pred, const double* Bt,
                                   const double* qconst, double* u_opt, double* x_opt, double* slack, double* fval, hipStream_t st) {
  hipLaunchKernelGGL(ltv_post_blocked_kernel, dim3(batch), dim3(256), 0, st, nx, N, ns, bm, z, pred, Bt, qconst, u_opt, x_opt, slack, fval);
  return hipGetLastError();
}
