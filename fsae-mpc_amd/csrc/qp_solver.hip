// qp_solver.hip -- batched dense convex QP solve on MI355X (gfx950), one wavefront per QP.
//
// Replaces the qpOASES MEX call of the reference
//   (mpc/ltv/kinematic/ltvmpc_kinetmatic_curvilinear.m:52, mpc/ltv/dynamic/ltvmpc_dynamic_curvilinear.m:52,
//    contract optimizers/matlab/qpOASES/qpOASES.m:16-62)
// with a primal-dual interior-point method (Mehrotra predictor-corrector, single step length,
// OOQP-style step heuristic).  Not a port of qpOASES: the algorithm is chosen for the hardware --
// every iteration is one pass of fp64 MFMA (v_mfma_f64_16x16x4_f64) forming M = H + A'DA with the
// accumulators resident in registers, plus three light streaming passes over A.
//
// Data layout (all per QP, in the device workspace, written once by qp_prep_kernel):
//   rows             are permuted once (qp_prep_kernel): sorted by the last column tile that holds a nonzero, then dealt
//                    round-robin to the four lane groups: sorted position p <-> k-step s = p>>2, lane group q = p&3.
//                    A *trip* = 4 k-steps = 16 sorted rows; tcs[trip] = number of leading column tiles that hold a
//                    nonzero in any of them.  The condensed LTV-MPC constraints are block lower-triangular (row k only
//                    sees the inputs up to step k), so on average ~60 % of the tiles and ~47 % of the MFMAs remain; a
//                    dense A keeps tcs = T everywhere and costs nothing extra.
//   Aw               scaled A in MFMA-operand stream order: trip, pair of k-steps u, tile t < tcs[trip], lane, 2 k-steps
//                    (16-byte lane loads); lane (c=l&15,q=l>>4) of k-step s holds A~[perm[4s+q]][16t + c].
//                    aoff[trip] = start of the trip in records of 128 doubles; tend[C] = number of trips with tcs <= C.
//   Hw [T*T][4][64]  scaled H in accumulator (C/D) layout: tile (I,J), reg p, lane -> H~[16I+q+4p][16J+c]
//   row vectors      "owner layout" [slot][64]: slot js<J, lane (c,q) <-> k-step s = 16js + c, sorted position 4s + q;
//                    slots J..J+JB-1 hold the variable-bound rows i = (js-J)*64 + lane.
// fp64 MFMA lane maps (cdna_hip_programming.md section 3): A[i=l&15][k=l>>4], B[k=l>>4][j=l&15],
// C/D col = l&15, row = (l>>4) + 4*reg.  fsaempc_selftest_mfma() checks them on the device.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <stdio.h>
#include "qp_solver.h"
#include "qp_lane.h"

// Translation units: the solve kernel is instantiated for T = 1..7 and three border widths; the Makefile builds this
// file five times (-DQP_TU=0: prep kernel, dimensions, dispatch, self test; -DQP_TU=1: T = 1..4; -DQP_TU=2..4: T = 5..7).
// Without QP_TU everything lands in one object (used by the one-command diagnostic builds).  The kernel itself is
// qp_solve_kernel.h; the main unit reads it too, for diag_factor in the self tests (qp_selftest.h) and for the probes (qp_probe.h).
#if !defined(QP_TU) || QP_TU == 0
#define QP_MAIN_TU 1
#else
#define QP_MAIN_TU 0
#endif
#include "qp_solve_kernel.h"

#if QP_MAIN_TU
namespace {

// ---------------------------------------------------------------------------------------------
// qp_prep_kernel: scaling (E columns, F rows), repack of A and H, scaled g / bounds.  One workgroup per QP.
// ---------------------------------------------------------------------------------------------
// -DQP_PREP_STAMPS: diagnostic build; lane 0 of every workgroup leaves the cycles of its phases in the dump buffer (stage 10, eight
// doubles per QP: column scale, row pass, sort, trips, rows / bounds, A repack, H repack, tail).  tools/prep_phase_profile.py prints them.
#ifdef QP_PREP_STAMPS
#define PSTAMP(id) do { __builtin_amdgcn_sched_barrier(0); const unsigned long long t_ = __builtin_amdgcn_s_memtime(); pst[id] += t_ - pst_t0; pst_t0 = t_; __builtin_amdgcn_sched_barrier(0); } while (0)
#else
#define PSTAMP(id) do { } while (0)
#endif
__global__ __launch_bounds__(1024) void qp_prep_kernel(QpParams P) {
  // one workgroup per QP: 256 threads up to 512 rows, 1024 above (qp_launch, prep_thr) -- the staging tile allows one workgroup per
  // CU at the large shapes, and with four wavefronts the dependent LDS -> global chains of the repack ran at a tenth of the memory
  // rate (11 ms of a 145 ms dynamic N = 60 batch).  Up to about 500 rows two or more 256-thread workgroups share a CU and beat one
  // of 1024 threads (profiles/startup/prep_threads_sweep.txt: 288 rows 0.80 vs 1.13 ms per 4096, 500 rows 0.89 vs 0.96, 600 rows
  // 1.96 vs 1.20)
  const int b = blockIdx.x, tid = threadIdx.x, w = tid >> 6, lane = tid & 63, c = lane & 15, q = lane >> 4;
  const int NTH = blockDim.x, NW = NTH >> 6;
  const QpDims& d = P.d;
  const int n = d.n, nu = d.nu, m = d.m, T = d.T, Kq = d.Kq, J = d.J, JB = d.JB, np = d.np, nc = d.nc, nb = d.nb;
  const double* H = P.H + (P.shared_HA ? 0 : (size_t)b * nu * nu);
  const double* A = P.A + (P.shared_HA ? 0 : (size_t)b * m * nu);
  const double* g = P.g + (size_t)b * nu;
  // caller's data by SOLVER index (n = nu unless the core is padded with dummy variables, QpDims::nu): dummies have a unit Hessian
  // diagonal, nothing else
  auto U = [&](int i) { return qp_user_index(d, i); };
  auto Hat = [&](int i, int j) -> double { const int ui = U(i), uj = U(j); return (ui >= 0 && uj >= 0) ? H[(size_t)uj * nu + ui] : ((i == j && i < n) ? 1.0 : 0.0); };
  auto Aat = [&](int r, int j) -> double { const int uj = U(j); return uj >= 0 ? A[(size_t)uj * m + r] : 0.0; };
  double* ws = P.ws + (size_t)b * d.ws_per_qp;
  double* Aw = ws + d.off_Aw;
  double* Hw = ws + d.off_Hw;
  double* gw = ws + d.off_gw;
  double* Es = ws + d.off_E;
  double* Fs = ws + d.off_F;   // owner layout, J slots
  double* Ab = ws + d.off_Ab;  // 4 border columns of A~, owner layout
  double* Hb = ws + d.off_Hb;  // 4 border columns of H~ (full length np)
  int* perm_g = reinterpret_cast<int*>(ws + d.off_meta);          // owner layout: original row of each sorted position (-1: padding)
  int* tcs_g = perm_g + (size_t)(J > 0 ? J : 1) * 64;              // [ntr] tiles per trip
  int* aoff_g = tcs_g + d.ntr;                                     // [ntr+1] start of each trip in the operand stream
  int* tend_g = aoff_g + d.ntr + 1;                                // [T+1] trips with tcs <= C
  const int ntr = d.ntr;
  double* Lr = ws + d.off_rows + 0 * (size_t)d.rowlen;  // scaled lower bounds (owner layout, rows then vars)
  double* Ur = ws + d.off_rows + 1 * (size_t)d.rowlen;
  extern __shared__ double lds[];
  double* Esh = lds;            // np
  double* red = lds + np;       // 16 partial maxima
  double* tile = red + 16;       // 16 x (4Kq+1) staging for the A transpose
  const int TW = d.prep_tw;     // columns staged per pass (16, or fewer when 16 x 4Kq doubles would not fit the LDS)
  int* cls_sh = reinterpret_cast<int*>(tile + TW * (4 * Kq + 1));   // [4Kq] tile class of every original row
  int* perm_sh = cls_sh + 4 * Kq;                                    // [16 ntr] original row of every sorted position
  int* cnt_sh = perm_sh + 16 * ntr;                                  // [T+1] class counts / starts ; then tcs [ntr], aoff [ntr+1]
  int* tcs_sh = cnt_sh + 16;
  int* aoff_sh = tcs_sh + ntr;
  int* chc_sh = aoff_sh + ntr + 1;                                   // [ceil(m/64)][16] rows of each class per 64-row chunk, then their starts
  double* Fr_sh = reinterpret_cast<double*>((reinterpret_cast<uintptr_t>(chc_sh + ((m + 63) >> 6) * 16) + 7) & ~(uintptr_t)7);   // [m] row scale of every original row
#ifdef QP_PREP_STAMPS
  unsigned long long pst[8] = {0, 0, 0, 0, 0, 0, 0, 0}, pst_t0 = __builtin_amdgcn_s_memtime();
#endif

  // ---- column scaling E_j = 1/sqrt(H_jj), or 1/max|A_:j| where H_jj ~ 0 (slack columns) ----
  for (int j = tid; j < np; j += NTH) {
    double e = 1.0;
    if (j < n) {
      double hjj = Hat(j, j);
      if (hjj > 1e-12) e = 1.0 / sqrt(hjj);
      else e = -1.0;  // resolved below with a cooperative column max
    } else e = 0.0;   // padded columns carry zeros
    Esh[j] = e;
  }
  __syncthreads();
  for (int j = 0; j < n; ++j) {
    if (Esh[j] < 0) {  // uniform over the workgroup
      double cm = 0;
      for (int r = tid; r < m; r += NTH) cm = fmax(cm, fabs(Aat(r, j)));
      cm = wave_max_zf(cm);   // (prep kernel: keeps the zero-filling lane moves)
      if (lane == 0) red[w] = cm;
      __syncthreads();
      if (tid == 0) { double mx = 0.0; for (int i = 0; i < NW; ++i) mx = fmax(mx, red[i]); Esh[j] = mx > 1e-12 ? 1.0 / mx : 1.0; }
      __syncthreads();
    }
  }
  int bad = 0;   // NaN / Inf anywhere in H, g, A or NaN in a bound: the solve kernel answers -1 before its first iteration (the
                 // reference's MEX gateway rejects such a call; a device entry cannot look at the data before the launch)
  for (int j = tid; j < np; j += NTH) { const int uj = j < n ? U(j) : -1; const double gj = uj >= 0 ? g[uj] : 0.0; Es[j] = Esh[j]; gw[j] = gj * Esh[j]; bad |= !(fabs(gj) < INFINITY); }

  PSTAMP(0);
  // ---- one pass over A, thread = row (coalesced: consecutive threads read consecutive rows of a column, the loads of a thread are
  //      independent): row scaling F_r = 1 / max_j |A[r][j] E_j| and the row's class = last core column tile with a nonzero.
  //      (Round 2 scanned every row twice with dependent / uncoalesced loads and ranked the rows with an O(m^2) loop: 14 ms of
  //      the 200 ms of a dynamic N = 60 batch.) ----
  __syncthreads();   // Esh complete
  const int ncols = nc < n ? nc : n;
  const int nchunk = (m + 63) >> 6;
  for (int i = tid; i < nchunk * 16; i += NTH) chc_sh[i] = 0;
  if (tid < 16) cnt_sh[tid] = 0;
  __syncthreads();
  for (int r0 = 0; r0 < m; r0 += NTH) {
    const int r = r0 + tid;
    int e = 0;
    double rm = 0.0;
    if (r < m) {
      // (eight columns of loads in flight: with one load per iteration the loop ran at one memory latency per column, 30 % of
      //  this kernel on the headline shape)
      for (int col0 = 0; col0 < n; col0 += 8) {
        double av[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) av[u] = col0 + u < n ? Aat(r, col0 + u) : 0.0;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int col = col0 + u;
          const double a = fabs(av[u]);
          if (col < n) { rm = fmax(rm, a * Esh[col]); if (a != 0.0 && col < ncols) e = col >> 4; }
        }
      }
      cls_sh[r] = e;
      Fr_sh[r] = rm > 1e-12 ? 1.0 / rm : 1.0;
    }
    // stable counting sort by class, part 1: rows of each class in this 64-row chunk (the lanes of a wave hold consecutive rows)
    for (int cl = 0; cl < T; ++cl) {
      const unsigned long long mk = __ballot(r < m && e == cl);
      if (lane == 0 && r0 + 64 * w < m) chc_sh[((r0 >> 6) + w) * 16 + cl] = __popcll(mk);
    }
  }
  __syncthreads();
  PSTAMP(1);
  if (tid < T) {   // per class: running start of every chunk (after the total of the lower classes is known: two steps)
    int tot = 0;
    for (int ch = 0; ch < nchunk; ++ch) tot += chc_sh[ch * 16 + tid];
    cnt_sh[tid] = tot;
  }
  __syncthreads();
  if (tid < T) {
    int start = 0;
    for (int cl = 0; cl < tid; ++cl) start += cnt_sh[cl];
    for (int ch = 0; ch < nchunk; ++ch) { const int cn = chc_sh[ch * 16 + tid]; chc_sh[ch * 16 + tid] = start; start += cn; }
  }
  for (int p = tid; p < 16 * ntr; p += NTH) perm_sh[p] = -1;
  __syncthreads();
  for (int r0 = 0; r0 < m; r0 += NTH) {   // part 2: position = start of (chunk, class) + rank among the chunk's earlier rows of the class
    const int r = r0 + tid;
    const int e = r < m ? cls_sh[r] : -1;
    for (int cl = 0; cl < T; ++cl) {
      const unsigned long long mk = __ballot(e == cl);
      if (e == cl) perm_sh[chc_sh[((r0 >> 6) + w) * 16 + cl] + __popcll(mk & ((1ull << lane) - 1ull))] = r;
    }
  }
  __syncthreads();
  PSTAMP(2);
  // tiles per trip (16 sorted positions), stream offsets, phase ends
  for (int tr = tid; tr < ntr; tr += NTH) {
    int tc = 1;
    for (int p = 16 * tr; p < 16 * tr + 16; ++p) { const int r = perm_sh[p]; if (r >= 0) tc = max(tc, cls_sh[r] + 1); }
    tcs_sh[tr] = tc;
  }
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int tr = 0; tr < ntr; ++tr) { aoff_sh[tr] = run; run += 2 * tcs_sh[tr]; }
    aoff_sh[ntr] = run;
    for (int C = 0; C <= T; ++C) { int cn = 0; for (int tr = 0; tr < ntr; ++tr) cn += (tcs_sh[tr] <= C); tend_g[C] = cn; }
  }
  __syncthreads();
  for (int tr = tid; tr <= ntr; tr += NTH) { aoff_g[tr] = aoff_sh[tr]; if (tr < ntr) tcs_g[tr] = tcs_sh[tr]; }
  PSTAMP(3);

  // ---- row scaling F_r = 1/max_j |A[r][j] E_j| ; rows handled in owner layout, one slot per wavefront and trip ----
  int nexcl = 0;   // rows / bounds that exclude x = 0: the difficulty estimate behind the launch order (QpParams::order)
  for (int js = w; js < J; js += NW) {
    const int s = 16 * js + c, pp = 4 * s + q;
    const int r = (s < 4 * ntr) ? perm_sh[pp] : -1;
    const bool valid = r >= 0;
    const double f = valid ? Fr_sh[r] : 0.0;
    Fs[js * 64 + lane] = f;
    perm_g[js * 64 + lane] = r;
    double ab[4], lr = 0.0, ur = 0.0;   // (the slot's loads -- border columns, bounds -- are issued together, ahead of the stores)
#pragma unroll
    for (int bb = 0; bb < 4; ++bb) ab[bb] = (valid && bb < nb) ? Aat(r, nc + bb) : 0.0;
    if (valid) { lr = P.lbA[(size_t)b * m + r]; ur = P.ubA[(size_t)b * m + r]; }
#pragma unroll
    for (int bb = 0; bb < 4; ++bb)
    { const double v = (valid && bb < nb) ? ab[bb] * Esh[nc + bb] * f : 0.0; bad |= !(fabs(v) < INFINITY); Ab[(size_t)bb * J * 64 + js * 64 + lane] = v; }
    double l = -INFINITY, u = INFINITY;
    if (valid) {
      bad |= (lr != lr) || (ur != ur);
      nexcl += (lr > 0.0) || (ur < 0.0);
      l = lr > -P.inf_bound ? lr * f : -INFINITY;
      u = ur < P.inf_bound ? ur * f : INFINITY;
    }
    Lr[js * 64 + lane] = l;
    Ur[js * 64 + lane] = u;
  }
  for (int jb = w; jb < JB; jb += NW) {
    const int i = jb * 64 + lane;
    double l = -INFINITY, u = INFINITY;
    const int ui = i < n ? U(i) : -1;
    if (ui >= 0) {
      double lr = P.lb[(size_t)b * nu + ui], ur = P.ub[(size_t)b * nu + ui];
      bad |= (lr != lr) || (ur != ur);
      nexcl += (lr > 0.0) || (ur < 0.0);
      l = lr > -P.inf_bound ? lr / Esh[i] : -INFINITY;
      u = ur < P.inf_bound ? ur / Esh[i] : INFINITY;
    }
    Lr[(J + jb) * 64 + lane] = l;
    Ur[(J + jb) * 64 + lane] = u;
  }
  __syncthreads();  // Fs visible to the whole workgroup (global memory, same CU)
  PSTAMP(4);

  // ---- A -> operand stream.  Column tile by column tile: coalesced column reads -> LDS -> lane order ----
  const int R4 = 4 * Kq, mp1 = R4 + 1;  // padded LDS row length (odd => conflict-free across the 16 columns)
  const int RCH = (R4 + 63) >> 6, NIT = TW * RCH;   // staging items: (staged column, run of 64 rows), one wavefront each
  for (int t = 0; t < T; ++t)
    for (int c0 = 0; c0 < 16; c0 += TW) {
      // (eight items of loads in flight per wavefront, a wavefront reads 64 consecutive rows of one column: with one load per trip
      //  and a division per element this loop ran at one memory latency per 8 bytes and lane)
      for (int i0 = w; i0 < NIT; i0 += 8 * NW) {
        double av[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int i = i0 + u * NW, cc = i / RCH, r = (i - cc * RCH) * 64 + lane, col = 16 * t + c0 + cc;
          av[u] = (i < NIT && col < nc && col < n && r < m) ? Aat(r, col) : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int i = i0 + u * NW, cc = i / RCH, r = (i - cc * RCH) * 64 + lane, col = 16 * t + c0 + cc;
          if (i < NIT && r < R4) {
            double v = 0.0;
            if (col < nc && col < n && r < m) v = av[u] * Esh[col];
            bad |= !(fabs(v) < INFINITY);
            tile[cc * mp1 + r] = v;
          }
        }
      }
      __syncthreads();
      // k-steps are stored in pairs (16 B per lane and load): a lane writes both k-steps of a pair as one 16-byte store, a
      // wavefront a whole 1 KB record (TW = 16); padded positions carry zeros.  Four pairs per trip of the loop: their LDS reads
      // are independent and go ahead of the stores.
      for (int sp0 = w; sp0 < 2 * ntr; sp0 += 4 * NW) {
        int r0[4], r1[4]; bool on[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int sp = sp0 + u * NW;
          on[u] = sp < 2 * ntr && t < tcs_sh[sp < 2 * ntr ? sp >> 1 : 0] && c >= c0 && c < c0 + TW;
          r0[u] = on[u] ? perm_sh[8 * sp + q] : -1; r1[u] = on[u] ? perm_sh[8 * sp + 4 + q] : -1;
        }
        v2d v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {   // (row scale from LDS: the owner-layout copy in global memory cost a load latency per k-step)
          v[u][0] = r0[u] >= 0 ? tile[(c - c0) * mp1 + r0[u]] * Fr_sh[r0[u]] : 0.0;
          v[u][1] = r1[u] >= 0 ? tile[(c - c0) * mp1 + r1[u]] * Fr_sh[r1[u]] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int sp = sp0 + u * NW;
          if (on[u]) { const int tr = sp >> 1, tc = tcs_sh[tr]; *reinterpret_cast<v2d*>(Aw + ((size_t)aoff_sh[tr] + (sp & 1) * tc + t) * 128 + lane * 2) = v[u]; }
        }
      }
      __syncthreads();
    }
  PSTAMP(5);

  // ---- H -> accumulator-layout tiles (T x T grid of the core; symmetric read for coalescing); eight tiles of loads in flight ----
  for (int i0 = w; i0 < T * T * 4; i0 += 8 * NW) {
    double hv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int idx = i0 + u * NW, p = idx & 3, IJ = idx >> 2, I = IJ / T, Jt = IJ - I * T;
      const int row = 16 * I + q + 4 * p, col = 16 * Jt + c;
      hv[u] = (idx < T * T * 4 && row < nc && col < nc && row < n && col < n) ? Hat(col, row) : 0.0;  // H[col][row] == H[row][col]
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int idx = i0 + u * NW, p = idx & 3, IJ = idx >> 2, I = IJ / T, Jt = IJ - I * T;
      const int row = 16 * I + q + 4 * p, col = 16 * Jt + c;
      if (idx < T * T * 4) {
        double v = 0.0;
        if (row < nc && col < nc && row < n && col < n) v = hv[u] * Esh[row] * Esh[col];
        bad |= !(fabs(v) < INFINITY);
        Hw[(size_t)idx * 64 + lane] = v;
      }
    }
  }
  for (int i = tid; i < np; i += NTH) {   // the four border columns of an index together
    double hv[4];
#pragma unroll
    for (int bb = 0; bb < 4; ++bb) hv[bb] = (bb < nb && i < n) ? Hat(i, nc + bb) : 0.0;
#pragma unroll
    for (int bb = 0; bb < 4; ++bb) {
      const double v = (bb < nb && i < n) ? hv[bb] * Esh[nc + bb] * Esh[i] : 0.0;
      bad |= !(fabs(v) < INFINITY);
      Hb[bb * np + i] = v;
    }
  }
  PSTAMP(6);
  bad = __syncthreads_or(bad);
  if (tid == 0) ws[d.off_bad] = bad ? 1.0 : 0.0;
  if (P.score) {
    __shared__ int score_sh;
    if (tid == 0) score_sh = 0;
    __syncthreads();
    if (nexcl) atomicAdd(&score_sh, nexcl);
    __syncthreads();
    if (tid == 0) P.score[b] = P.score_in ? P.score_in[b] : score_sh;
  }
#ifdef QP_PREP_STAMPS
  PSTAMP(7);
  if (P.dump && P.dump_stage == 10 && tid == 0) for (int i = 0; i < 8; ++i) P.dump[(size_t)b * 8 + i] = (double)pst[i];
#endif
}

// ---------------------------------------------------------------------------------------------
// qp_order_kernel: order[] = instance ids by descending score, ties in index order (a stable counting sort by one workgroup:
// scores clipped to 1023; eight wavefronts each count and place a contiguous range of the ids, no atomics, so the order -- and
// with it the timing of a batch -- is the same every run)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void qp_order_kernel(const int* __restrict__ score, int* __restrict__ order, int batch) {
  constexpr int NBIN = 1024, NWV = 8;   // (10-bit keys: group() below)
  __shared__ int cnt[NWV][NBIN], scan[NBIN];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  for (int e = tid; e < NWV * NBIN; e += 1024) (&cnt[0][0])[e] = 0;
  __syncthreads();
  const int per = ((batch + NWV - 1) / NWV + 63) & ~63;   // ids per counting wavefront, a multiple of 64
  const int lo = w * per, hi = min(batch, lo + per);
  auto bin = [&](int i) { return NBIN - 1 - min(max(score[i], 0), NBIN - 1); };   // bin 0 = highest score
  // rank of this lane among the lanes of its wavefront holding the same bin (lower lanes first), and that group's size
  auto group = [&](int k, bool on, int& rank, int& size) {
    unsigned long long same = __builtin_amdgcn_ballot_w64(on);   // lanes holding the same bin: one ballot per key bit
#pragma unroll
    for (int bit = 0; bit < 10; ++bit) {
      const bool one = (k >> bit) & 1;
      const unsigned long long v = __builtin_amdgcn_ballot_w64(one);
      same &= one ? v : ~v;
    }
    rank = __popcll(same & ((1ull << lane) - 1ull)); size = __popcll(same);
  };
  // (eight rounds of ids per trip: their score loads are in flight together -- one dependent load per round made this kernel 44 us)
  if (w < NWV)
    for (int i0 = lo; i0 < hi; i0 += 512) {
      int kv[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) { const int i = i0 + 64 * r + lane; kv[r] = i < hi ? bin(i) : -1; }
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const bool on = kv[r] >= 0; const int k = on ? kv[r] : 0;
        int rank, size; group(k, on, rank, size);
        if (on && rank == 0) cnt[w][k] += size;
      }
    }
  __syncthreads();
  int v = 0;
  for (int ww = 0; ww < NWV; ++ww) v += cnt[ww][tid];
  scan[tid] = v;
  __syncthreads();
  for (int o = 1; o < NBIN; o <<= 1) {
    const int a = tid >= o ? scan[tid - o] : 0;
    __syncthreads();
    scan[tid] += a;
    __syncthreads();
  }
  int run = scan[tid] - v;   // start of bin tid; then the start of each wavefront's share of it
  for (int ww = 0; ww < NWV; ++ww) { const int c = cnt[ww][tid]; cnt[ww][tid] = run; run += c; }
  __syncthreads();
  if (w < NWV)
    for (int i0 = lo; i0 < hi; i0 += 512) {
      int kv[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) { const int i = i0 + 64 * r + lane; kv[r] = i < hi ? bin(i) : -1; }
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const bool on = kv[r] >= 0; const int k = on ? kv[r] : 0;
        int rank, size; group(k, on, rank, size);
        int base = on ? cnt[w][k] : 0;
        if (on) order[base + rank] = i0 + 64 * r + lane;
        if (on && rank == 0) cnt[w][k] = base + size;   // (one writer per bin and round; read above by every lane of the group first)
      }
    }
}

}  // namespace

#include "qp_selftest.h"
#ifdef QP_PROBE
#include "qp_probe.h"
#endif

void qp_make_dims(int n, int m, QpDims* d, int n_slack) {
  d->n = n; d->nu = n; d->m = m;
  // 1..4 trailing variables (the slack columns of the LTV-MPC QPs: nV = 2N + 1 or 2N + 4) are a *border*: they are
  // handled on the VALU instead of costing a whole 16-wide tile row/column of MFMA work and operand traffic
  const int rem = n % 16;
  if (n >= 16 && rem >= 1 && rem <= 4) { d->T = n / 16; d->nb = rem; } else { d->T = (n + 15) / 16; d->nb = 0; }
  // The slack columns of an LTV-MPC QP are touched by most rows (every soft constraint of every stage), while the input columns of
  // a row end at its own stage: with the slack columns inside the last core tile every trip of the operand stream reaches all T
  // tiles and the structural sparsity of the condensed constraints is lost (dynamic N = 60: nV = 124 = 7 x 16 + 12: measured
  // 10.8 k instead of 4.6 k MFMAs per iteration in pass 1).  Shapes with the row / column signature of the reference's QPs
  // (kinematic: nC = 6N, nV = 2N + 1; dynamic: nC = 20N, nV = 2N + 4 -- ltvmpc_*.m:38-41, *_state_constraints.m) therefore keep
  // their 1 / 4 trailing slack columns as the border whatever nV mod 16 is.  It began as a performance policy applied only where it
  // pays (a tile row / column saved, or T >= 6); it is applied to every such shape since the sweeps of the final round-3 build: with the
  // zero-curvature, 1e8-cost slack column INSIDE the MFMA core the one-wavefront kernel lost kinematic N = 20 instance 15377 (a step of
  // the end game went non-finite; ids 0..16383 all solved, vertex rate 98.7 -> 99.0 % with the column as the border; the cost measured
  // on that shape is within noise now, 910 k vs 914 k QP/s).  FSAEMPC_SLACK_BORDER=0 switches it off, =1 is the old "where it pays"
  // rule (A/B runs and tests).
  if (n_slack >= 0) {   // the caller names its trailing slack columns: they are the border, the core is padded with dummy variables
    d->T = (n - n_slack + 15) / 16; d->nb = n_slack;
    if (n_slack > 0) d->n = 16 * d->T + n_slack;
  } else if (d->nb == 0 && n >= 20) {
    const char* sb = getenv("FSAEMPC_SLACK_BORDER");
    const int ns = (m == 10 * (n - 4) && ((n - 4) % 2) == 0) ? 4 : ((m == 3 * (n - 1) && ((n - 1) % 2) == 0) ? 1 : 0);
    const int Tp = (n - ns + 15) / 16;
    const bool pays = !(sb && sb[0] == '1') || Tp < d->T || Tp >= 6;
    if (ns > 0 && pays && !(sb && sb[0] == '0') && Tp <= QP_MAX_T) {
      d->T = Tp; d->nb = ns;
      d->n = 16 * d->T + ns;     // the solver's variable count: the core padded with dummy variables (qp_solver.h: QpDims::nu)
    }
  }
  n = d->n;
  d->NB = d->nb == 0 ? 0 : (d->nb == 1 ? 1 : 4);
  d->nc = 16 * d->T;
  d->np = d->nc + (d->nb ? 16 : 0);
  d->Kq = (m + 3) / 4;
  d->J = (d->Kq + 15) / 16;
  d->JB = (d->np + 63) / 64;
  d->rowlen = (d->J + d->JB) * 64;
  size_t off = 0;
  d->ntr = (d->Kq + 3) / 4;   // trips of 4 k-steps (16 rows)
  d->off_Aw = off; off += (size_t)(2 * d->ntr) * d->T * 128;   // dense upper bound of the operand stream
  d->off_meta = off; off += ((size_t)(d->J > 0 ? d->J : 1) * 64 + 2 * (size_t)d->ntr + 1 + 16 + 1) / 2 + 1;   // int arrays: perm, tcs, aoff, tend
  off = (off + 1) & ~(size_t)1;   // keep every array 16-byte aligned (pairs of k-steps are read as 16-byte lane loads)
  d->off_Hw = off; off += (size_t)d->T * d->T * 4 * 64;
  d->off_gw = off; off += d->np;
  d->off_E = off; off += d->np;
  d->off_F = off; off += (size_t)(d->J > 0 ? d->J : 1) * 64;
  d->off_Ab = off; off += (size_t)4 * (d->J > 0 ? d->J : 1) * 64;
  d->off_Hb = off; off += (size_t)4 * d->np;
  d->off_rows = off; off += (size_t)R_NARR * d->rowlen;
  d->off_save = off; off += d->np + d->rowlen;
  d->off_bad = off; off += 2;
  off = (off + 1) & ~(size_t)1;
  d->off_U = off; off += (size_t)(d->T * (d->T + 1) / 2) * 256;   // (workgroup kernel)
  off = (off + 63) & ~(size_t)63;
  d->ws_per_qp = off;
  d->lds_solve = qp_solve_lds(d->T, d->NB, d->np).total() * sizeof(double);
  {   // workgroup solve kernel (qp_wg.hip), W = 8 wavefronts per QP
    d->W = QP_WG_W;
    d->NBk = d->nb == 0 ? 0 : 4;
    d->wg_ring = 1;
    d->lds_wg = qp_wg_lds_base_bytes(*d, d->W, d->NBk);
  }
  d->prep_tw = 16;
  for (;;) {
    d->lds_prep = ((size_t)d->np + 16 + (size_t)d->prep_tw * (4 * d->Kq + 1) + (size_t)m + 2) * sizeof(double) +
                  ((size_t)4 * d->Kq + 16 * (size_t)d->ntr + 16 + 2 * (size_t)d->ntr + 1 + (size_t)((m + 63) / 64) * 16 + 6) * sizeof(int);
    if (d->lds_prep <= 96 * 1024 || d->prep_tw == 2) break;   // keep the staging tile small enough for more than one workgroup per CU
    d->prep_tw >>= 1;
  }
}

#endif  // QP_MAIN_TU

#if defined(QP_TU)
hipError_t qp_launch_solve_g1(const QpParams& P, int batch, hipStream_t st);   // T = 1..4
hipError_t qp_launch_solve_g2(const QpParams& P, int batch, hipStream_t st);   // T = 5
hipError_t qp_launch_solve_g3(const QpParams& P, int batch, hipStream_t st);   // T = 6
hipError_t qp_launch_solve_g4(const QpParams& P, int batch, hipStream_t st);   // T = 7
#if QP_TU == 1
hipError_t qp_launch_solve_g1(const QpParams& P, int batch, hipStream_t st) {
  switch (P.d.T) {
    case 1: return launch_solve_T<1>(P, batch, st);
    case 2: return launch_solve_T<2>(P, batch, st);
    case 3: return launch_solve_T<3>(P, batch, st);
    case 4: return launch_solve_T<4>(P, batch, st);
    default: return hipErrorInvalidValue;
  }
}
#elif QP_TU == 2
hipError_t qp_launch_solve_g2(const QpParams& P, int batch, hipStream_t st) { return launch_solve_T<5>(P, batch, st); }
#elif QP_TU == 3
hipError_t qp_launch_solve_g3(const QpParams& P, int batch, hipStream_t st) { return launch_solve_T<6>(P, batch, st); }
#elif QP_TU == 4
hipError_t qp_launch_solve_g4(const QpParams& P, int batch, hipStream_t st) { return launch_solve_T<7>(P, batch, st); }
#endif
#endif

#if QP_MAIN_TU
// Kernel selection.  Two solve kernels share the prep kernel, the workspace layout and the algorithm:
//   - the one-wavefront kernel of qp_solve_kernel.h (T = 1..7 column tiles, border widths 0 / 1 / 4: nV <= 116), built as four
//     translation units by tile count;
//   - the workgroup-per-QP kernel of qp_wg.hip (T = 1..12, nV <= 196: eight wavefronts share one QP), five more units.
// qp_use_wavefront_kernel() holds the measured choice per shape.  Every unit goes through the build's
// assembly check (tools/check_isa_exec_prologue.py: the compiler defect behind the wrong iterates of some -O2/-O3 builds,
// DESIGN.md "Build-variant fragility: root cause") and tests/test_gpu_parity.py::test_shipped_build_matches_O1_build
// compares every instantiation of both kernels with an -O1 build on the GPU.  FSAEMPC_QP_KERNEL=wg|v1 overrides the choice
// (A/B runs).
#define QP_V1_MAX_T 7
// Measured on MI355X at 4096 QPs per launch (profiles/round2/kernel_ab.txt): the one-wavefront kernel is 1.1-2x faster up to
// T = 7 (nV <= 116); from T = 8 on its accumulators no longer fit the register file (it spills) and the workgroup kernel wins
// (dynamic N = 60: 18.6k vs 9.6k QP/s), so T = 8 is not instantiated here.  np <= 128 is also a hard limit of this kernel
// (two lanes-worth of n-vector elements per sweep).
static bool qp_use_wavefront_kernel(const QpDims& d) {
  return d.T <= QP_V1_MAX_T;
}
bool qp_runs_wavefront_kernel(const QpDims& d) {   // what qp_launch will pick (the C ABI checks the LDS budget of that kernel)
  static const char* force = getenv("FSAEMPC_QP_KERNEL");   // A/B runs only: "wg" or "v1"
  return d.T <= QP_V1_MAX_T && ((force && force[0] == 'v') || (!(force && force[0] == 'w') && qp_use_wavefront_kernel(d)));
}
// one translation unit of qp_wg.hip per tile count from T = 6 on (T = 1..5 share one: no bordered variants there): the build is
// bound by the largest kernels, and they compile side by side this way
hipError_t qp_wg_launch_1(const QpParams& P, int batch, hipStream_t st);
hipError_t qp_wg_launch_6(const QpParams& P, int batch, hipStream_t st);
hipError_t qp_wg_launch_7(const QpParams& P, int batch, hipStream_t st);
hipError_t qp_wg_launch_8(const QpParams& P, int batch, hipStream_t st);
hipError_t qp_wg_launch_9(const QpParams& P, int batch, hipStream_t st);
hipError_t qp_wg_launch_10(const QpParams& P, int batch, hipStream_t st);
hipError_t qp_wg_launch_11(const QpParams& P, int batch, hipStream_t st);
hipError_t qp_wg_launch_12(const QpParams& P, int batch, hipStream_t st);
static hipError_t qp_wg_launch(const QpParams& P, int batch, hipStream_t st) {
  switch (P.d.T) {
    case 1: case 2: case 3: case 4: case 5: return qp_wg_launch_1(P, batch, st);
    case 6: return qp_wg_launch_6(P, batch, st);
    case 7: return qp_wg_launch_7(P, batch, st);
    case 8: return qp_wg_launch_8(P, batch, st);
    case 9: return qp_wg_launch_9(P, batch, st);
    case 10: return qp_wg_launch_10(P, batch, st);
    case 11: return qp_wg_launch_11(P, batch, st);
    case 12: return qp_wg_launch_12(P, batch, st);
  }
  return hipErrorInvalidValue;
}
static int prep_thr() { static const char* e = getenv("FSAEMPC_PREP_THR"); return e ? atoi(e) : 512; }   // rows up to which the prep kernel runs on 256 threads (the variable: A/B runs)
hipError_t qp_launch(const QpParams& P, int batch, hipStream_t st, hipEvent_t ev_mid) {
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&qp_prep_kernel),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)P.d.lds_prep);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(qp_prep_kernel, dim3(batch), dim3(P.d.m > prep_thr() ? 1024 : 256), P.d.lds_prep, st, P);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (P.order) {
    hipLaunchKernelGGL(qp_order_kernel, dim3(1), dim3(1024), 0, st, P.score, P.order, batch);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (ev_mid) { e = hipEventRecord(ev_mid, st); if (e != hipSuccess) return e; }
#ifdef QP_PROBE
  if (P.dump && P.dump_stage == 7 && P.d.T == 5) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&factor_probe_kernel<5>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)P.d.lds_solve);
    hipLaunchKernelGGL((factor_probe_kernel<5>), dim3(batch), dim3(64), P.d.lds_solve, st, P, 8);
    return hipGetLastError();
  }
  if (P.dump && P.dump_stage == 8 && P.d.T == 5 && P.d.NB == 1) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&syrk_probe_kernel<5, 1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)P.d.lds_solve);
    hipLaunchKernelGGL((syrk_probe_kernel<5, 1>), dim3(batch), dim3(64), P.d.lds_solve, st, P, 16);
    hipLaunchKernelGGL(overlap_probe_kernel, dim3(batch), dim3(64), 0, st, P.dump + 2 * (size_t)batch, 2048);   // (the caller leaves 64 doubles there)
    return hipGetLastError();
  }
#endif
  if (!qp_runs_wavefront_kernel(P.d)) return qp_wg_launch(P, batch, st);
#if !defined(QP_TU)
  switch (P.d.T) {
#if defined(QP_ONLY_T)
    case QP_ONLY_T: return launch_solve_T<QP_ONLY_T>(P, batch, st);
#else
    case 1: return launch_solve_T<1>(P, batch, st);
    case 2: return launch_solve_T<2>(P, batch, st);
    case 3: return launch_solve_T<3>(P, batch, st);
    case 4: return launch_solve_T<4>(P, batch, st);
    case 5: return launch_solve_T<5>(P, batch, st);
    case 6: return launch_solve_T<6>(P, batch, st);
    case 7: return launch_solve_T<7>(P, batch, st);
#endif
    default: return hipErrorInvalidValue;
  }
#else
  switch (P.d.T) {
    case 1: case 2: case 3: case 4: return qp_launch_solve_g1(P, batch, st);
    case 5: return qp_launch_solve_g2(P, batch, st);
    case 6: return qp_launch_solve_g3(P, batch, st);
    case 7: return qp_launch_solve_g4(P, batch, st);
    default: return hipErrorInvalidValue;
  }
#endif
}

#endif  // QP_MAIN_TU
