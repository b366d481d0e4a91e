// ltv_build_kernel.h -- the body of the LTV-MPC construction kernel, written once for the plain, the exact and the blocked build.
// Included by ltv_build.hip (the plain and exact instantiations) and by ltv_build_blocked.hip (the blocked ones); the file headers
// there say what is replaced and how the blocked QP relates to the unblocked one.
#pragma once
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

// The block map as the kernel body reads it from LDS (bst[j]: first step of block j, bst[M] = N; bos[k]: block of step k).  Without
// blocks input pair j acts at step j alone: nothing is carved or read, and each member reduces to the plain expression.
template <bool BLK> struct BlockIndex {
  const int* bst; const int* bos;
  DEVINL int first_step(int j) const { return bst[j]; }
  DEVINL int block_of(int k) const { return bos[k]; }
  DEVINL double times_len(int j, double x) const { return (double)(bst[j + 1] - bst[j]) * x; }
};
template <> struct BlockIndex<false> {
  DEVINL int first_step(int j) const { return j; }
  DEVINL int block_of(int k) const { return k; }
  DEVINL double times_len(int, double x) const { return x; }
};

// ---------------------------------------------------------------------------------------------
// EXACT = false: the LTV build of the reference (quirks C-1, C-3, C-4/C-5, C-8 kept; bitwise pinned by the parity tests).
// EXACT = true: the QP of the NLP of DESIGN.md "Nonlinear MPC: batched SQP" at u = u_lin: x_lin is not read, the states are the
// rollout x_k = Psi(x_{k-1}, u_k) (x_0 = x0), step k is linearised exactly at (x_{k-1}, u_k), Phi(i,i) = Bd_i, every constraint row
// is linearised at the rollout state it constrains, and pred receives the rollout (the affine offset of the QP, rollout - Phi u_lin,
// stays internal).
// BLK = false: one input pair per step, 2N input columns; there is no map argument and nothing of the map is carved.  BLK = true: the input is held
// over the M blocks of bm, 2M input columns; the rows and their bounds stay those of the unblocked QP.  The two differ
// in BlockIndex above and in the `if constexpr (BLK)` below; with one step per block each reduces to the plain expression.
// PAR: the constants (mpc_params.h).  FixedPar: the shipped build, pa is empty.  RtPar: the constants of the instance's block, loaded
// once through uniform addresses (pa.idx: the batch instance behind this workgroup, for sub-batches).
// The arguments are (LtvParams, LtvBlockMap, PAR::Args) with blocks and (LtvParams, PAR::Args) without: MAP is LtvBlockMap or
// nothing.  (An empty struct in the map's place would still take a byte of the argument segment and move what follows it, the
// parameter arguments or the hidden ones, and with them scalar loads of the shipped kernels: profiles/build_unify/README.md.)
DEVINL const LtvBlockMap& the_map(const LtvBlockMap& bm) { return bm; }
DEVINL int pair_count(int, const LtvBlockMap& bm) { return bm.M; }   // input pairs: one per block,
DEVINL int pair_count(int N) { return N; }                           // or one per step
template <int NX, bool EXACT, bool BLK, class PAR, class... MAP> __global__ __launch_bounds__(256)
void ltv_build_kernel(LtvParams P, MAP... bm, typename PAR::Args pa) {
  static_assert(!(EXACT && BLK), "the exact build knows no blocks (DESIGN.md 6h)");
  static_assert(sizeof...(MAP) == (BLK ? 1 : 0), "a block map with BLK, and only then");
  const PAR p = par_get<PAR>(pa, blockIdx.x);
  constexpr int NN = NX * NX, NS = (NX == 5) ? 1 : 4, RPK = (NX == 5) ? 6 : 20;  // rows per step
  const int b = blockIdx.x, tid = threadIdx.x, nth = blockDim.x;
  const int N = P.N, M = pair_count(N, bm...), R = NX * N, nV = 2 * M + NS, nC = RPK * N;   // M input pairs
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

  // the LDS carve: ltv_build_lds_bytes (ltv_build.hip) is this list, term by term
  extern __shared__ double sm[];
  double* Ad = sm;                 // N * NN
  double* Bd = Ad + (size_t)N * NN;  // N * NX*2 (only slice 0 is used by the LTV condensing: quirk C-1)
  double* dd = Bd + (size_t)N * NX * 2;  // N * NX
  double* aff = dd + (size_t)N * NX;     // R   : A_bar*x0 + d_bar
  double* cc = aff + R;                  // per-step constraint coefficient scratch: N * CW
  constexpr int CW = (NX == 5) ? 3 : (2 * 4 + 2 + 4 + 2);  // kin: C3,C4,const ; dyn: slip rows (2x4 coef + 2 const), tyre (4 coef K-part) + 2
  double* red = cc + (size_t)N * CW;     // reduction scratch (nth)
  double* ell = red + nth;               // 24: dac[12], dal[12] of the inscribed 12-gon (dynamic_tyre_linearise_constraints.m:33-39)
  double* colst = ell + 24;              // one column of Bt (R doubles) per wavefront: stage of step 4c
  double* xs = colst + (size_t)(nth >> 6) * R;   // EXACT: rollout x_0 .. x_N ((N + 1) * NX)
  double* ell0 = xs + (EXACT ? (size_t)(N + 1) * NX : 0);   // PAR::RT or BLK: 24 more, ac0[12], al0[12] of the same 12-gon (read with PAR::RT)
  int* bst = nullptr; int* bos = nullptr;
  BlockIndex<BLK> bix;
  if constexpr (BLK) {
    bst = reinterpret_cast<int*>(ell0 + 24);                   // M + 1 ints: first step of every block, bst[M] = N
    bos = bst + (M + 1);                                       // N ints: block of step k
    bix.bst = bst; bix.bos = bos;
  }

  if (tid < 12) {
    const int j = tid;
    const double th0 = 2 * M_PI * (double)j / 12, th1 = (j + 1 == 12) ? 2 * M_PI : 2 * M_PI * (double)(j + 1) / 12;
    ell[j] = p.ELL_LAT * sin(th1) - p.ELL_LAT * sin(th0); ell[12 + j] = p.ELL_LONG * cos(th1) - p.ELL_LONG * cos(th0);
    if constexpr (PAR::RT) { ell0[j] = p.ELL_LAT * sin(th0); ell0[12 + j] = p.ELL_LONG * cos(th0); }
  }
  if constexpr (BLK) {
    for (int j = tid; j <= M; j += nth) {
      const int s = the_map(bm...).start[j], e = j < M ? the_map(bm...).start[j + 1] : s;
      bst[j] = s;
      for (int k = s; k < e; ++k) bos[k] = j;
    }
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
  // zero Bt while the linearisation runs (BLK: step 3 writes every entry of Bt once, no separate clearing pass)
  if constexpr (!BLK) for (size_t i = tid; i < (size_t)R * nV; i += nth) Bt[i] = 0.0;
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
  // ---- 3. Phi columns: Phi(i,i) = Bd_1 (always slice 1, quirk C-1; EXACT: Bd_i), Phi(j,i) = Ad_j Phi(j-1,i).  BLK: the response
  // of the states to input c held over block j: cur = Bd(:,c) at the block's first step, then cur <- Ad_i cur + (i in block j ?
  // Bd(:,c) : 0), the sum of the block's columns of Phi in one recursion; the column's rows above the block and the slack columns
  // are written here too. ----
  for (int w = tid; w < (BLK ? nV : 2 * M); w += nth) {
    if constexpr (BLK) { if (w >= 2 * M) { for (int e = 0; e < R; ++e) Bt[(size_t)w * R + e] = 0.0; continue; } }
    const int j = w >> 1, col = w & 1, s0 = bix.first_step(j), s1 = bix.first_step(j + 1);
    double cur[NX], nxt[NX], bd0[NX];
    const double* bdi = EXACT ? Bd + (size_t)s0 * NX * 2 : Bd;
    for (int r = 0; r < NX; ++r) { bd0[r] = bdi[r + col * NX]; cur[r] = bd0[r]; }
    double* dst = Bt + (size_t)w * R;
    if constexpr (BLK) for (int e = 0; e < s0 * NX; ++e) dst[e] = 0.0;
    for (int r = 0; r < NX; ++r) dst[s0 * NX + r] = cur[r];
    for (int i = s0 + 1; i < N; ++i) {
      const double* a = Ad + (size_t)i * NN;
      const bool in = BLK && i < s1;
      for (int r = 0; r < NX; ++r) {
        double s = in ? bd0[r] : 0.0;
        for (int c = 0; c < NX; ++c) s += a[r + c * NX] * cur[c];
        nxt[r] = s;
      }
      for (int r = 0; r < NX; ++r) { cur[r] = nxt[r]; dst[i * NX + r] = nxt[r]; }
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
  // ---- 4b. variable bounds (ltvmpc_*.m:28-29) and constraint bounds: the rows and their bounds do not depend on the blocking ----
  for (int i = tid; i < nV; i += nth) {
    if (i < 2 * M) { lb[i] = (i & 1) ? -pl.U_STEER_MAX : -pl.U_ACC_MAX; ub[i] = (i & 1) ? pl.U_STEER_MAX : pl.U_ACC_MAX; }
    else { lb[i] = 0.0; ub[i] = INFINITY; }
  }
  const int vidx = 3, didx = NX - 1, nidx = 1, scol = 2 * M;
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
  // dynamic N = 60 batch.)  The 12 half-plane directions of the tyre ellipse come from a small LDS table; the polygon's direct
  // term (+dac on the acceleration input of the row's own step) lands in column 2 bix.block_of(k). ----
  {
    const int lane = tid & 63, wv = tid >> 6, nwv = nth >> 6;
    double* bc = colst + (size_t)wv * R;                     // this wave's column stage
    for (int col = wv; col < nV; col += nwv) {
      const bool inp = col < 2 * M;                            // input column: a column of Bt; slack column: unit entries only
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
          if (col == 2 * bix.block_of(k)) v += dac;
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
  // started at the first block row in which column tile I is non-zero (Bt is block lower-triangular: input pair 8 I, whose column
  // is zero above its first step).  (Round 2 computed every entry as a scalar dot product with stride-NX loads: 3.5 of the 10.3 ms
  // of a dynamic N = 60 batch, 0.95 of 2.26 ms on the headline shape.)  Lane (c = l & 15, q = l >> 4): A operand = weight *
  // Bt[row rho][16 I + c], B operand = Bt[row rho][16 J + c], rho = 4 s + q over the weighted rows (k, r) = (rho / 3, rho % 3);
  // result register p holds H[16 I + q + 4 p][16 J + c].  BLK: Rbar carries len_j R.
  const double Qw[3] = {pl.QW[0], pl.QW[1], pl.QW[2]};   // ltvmpc_*.m:32 ; Q_terminal = 10 Q (:33)
  {
    const int lane = tid & 63, wv = tid >> 6, nwv = nth >> 6, c = lane & 15, q = lane >> 4;
    const int nU = 2 * M, Tu = (nU + 15) >> 4, npairs = Tu * (Tu + 1) / 2, ksteps = (3 * N + 3) >> 2;
    for (int pidx = wv; pidx < npairs; pidx += nwv) {
      int I = 0;
      while ((I + 1) * (I + 2) / 2 <= pidx) ++I;
      const int J = pidx - I * (I + 1) / 2;                      // I >= J
      const int ci = 16 * I + c, cj = 16 * J + c;
      const double* pi_ = Bt + (size_t)(ci < nU ? ci : 0) * R;
      const double* pj_ = Bt + (size_t)(cj < nU ? cj : 0) * R;
      const bool oni = ci < nU, onj = cj < nU;
      v4d acc = {0.0, 0.0, 0.0, 0.0};
      int s0;                                                     // column tile I starts at the first step of input pair 8 I (8 I < M),
      if constexpr (BLK) s0 = (3 * bix.first_step(8 * I)) >> 2;   // 3 weighted rows per step
      else s0 = (3 * 8 * I) >> 2;
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
          const double v = 2.0 * (acc[pp] + (i == j ? bix.times_len(i >> 1, (i & 1) ? pl.R_STEER : pl.R_ACC) : 0.0));   // R = [10,10] per held step (ltvmpc_*.m:34)
          H[(size_t)i + (size_t)j * nV] = v;
          H[(size_t)j + (size_t)i * nV] = v;
        }
      }
    }
    // slack rows / columns of H carry no quadratic cost
    for (int e = tid; e < NS * nV; e += nth) {
      const int sc = 2 * M + e / nV, i = e - (e / nV) * nV;
      H[(size_t)i + (size_t)sc * nV] = 0.0;
      H[(size_t)sc + (size_t)i * nV] = 0.0;
    }
  }
  double qc_local = 0.0;
  for (int i = tid; i < nV; i += nth) {
    double s = 0.0;
    if (i < 2 * M) {
      const double* ci = Bt + (size_t)i * R;
      int k;                                           // (not bix.first_step(i >> 1) for both: the unblocked kernels then compile as they did)
      if constexpr (BLK) k = bix.first_step(i >> 1); else k = i >> 1;
      for (; k < N; ++k) {
        const double wq = (k == N - 1) ? pl.Q_TERMINAL : 1.0;
        for (int r = 0; r < 3; ++r) s += ci[k * NX + r] * (wq * Qw[r]) * (aff[k * NX + r] - x_ref[k * NX + r]);
      }
      g[i] = 2 * s;
    } else {
      const int sidx = i - 2 * M;
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

// The launch of one unit's instantiations (BLK is the unit's; bm: the map, or nullptr without blocks): PAR (values = nullptr: the
// constants compiled in), EXACT and NX are selected here, once.
template <int NX, bool EXACT, bool BLK, class PAR>
hipError_t launch_build(const LtvParams& P, const LtvBlockMap* bm, const typename PAR::Args& pa, int batch, hipStream_t st) {
  const int threads = 256;
  const size_t lds = ltv_build_lds_bytes(NX, P.N, threads, EXACT, PAR::RT, BLK ? bm->M : 0);
  const auto kernel = [] { if constexpr (BLK) return &ltv_build_kernel<NX, EXACT, BLK, PAR, LtvBlockMap>; else return &ltv_build_kernel<NX, EXACT, BLK, PAR>; }();
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  if constexpr (BLK) hipLaunchKernelGGL(kernel, dim3(batch), dim3(threads), lds, st, P, *bm, pa);
  else hipLaunchKernelGGL(kernel, dim3(batch), dim3(threads), lds, st, P, pa);
  return hipGetLastError();
}
template <bool BLK, class PAR>
hipError_t select_build_nx(const LtvParams& P, const LtvBlockMap* bm, const typename PAR::Args& pa, int batch, hipStream_t st, bool exact) {
  if constexpr (!BLK) if (exact) return P.nx == 5 ? launch_build<5, true, BLK, PAR>(P, bm, pa, batch, st) : launch_build<7, true, BLK, PAR>(P, bm, pa, batch, st);
  return P.nx == 5 ? launch_build<5, false, BLK, PAR>(P, bm, pa, batch, st) : launch_build<7, false, BLK, PAR>(P, bm, pa, batch, st);
}
template <bool BLK>
hipError_t select_build(const LtvParams& P, const LtvBlockMap* bm, const double* values, int stride, const int* idx, int batch, hipStream_t st, bool exact) {
  if (values) return select_build_nx<BLK, RtPar>(P, bm, ParArgs{values, stride, idx}, batch, st, exact);
  return select_build_nx<BLK, FixedPar>(P, bm, NoParArgs{}, batch, st, exact);
}

}  // namespace
